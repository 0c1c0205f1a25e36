"""Retrieval and zero-shot evaluation on the global embeddings: image <-> text recall@K / mean and median rank over a whole
evaluation set, and zero-shot classification against prompt-ensembled class embeddings.

The scoring runs on two HIP launches (medmoe_amd.ops.sim_rank / sim_topk, csrc/retrieval.hip) that stream the keys past the queries and
keep only a rank or the K best entries per query: the [N, N] similarity matrix of an evaluation set is never stored.  Everything else in
this file - the growing bank, the gather across data-parallel ranks, the reducers - is plain torch and runs on any device.

Embeddings are L2-normalised on the way into the bank with eps = 1e-8, the clamp of medmoe_cos_scale, so the product of two rows is the
reference's cosine (losses.py:781-785) whenever both norms are above eps."""
from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.distributed as tdist

from . import ops

I32 = torch.int32


def _world() -> Tuple[int, int]:
    if tdist.is_available() and tdist.is_initialized():
        return tdist.get_world_size(), tdist.get_rank()
    return 1, 0


def _gather_var(t: torch.Tensor, counts: Sequence[int]) -> torch.Tensor:
    """Rows of every rank back to back in rank order; rank r contributes counts[r] rows (t holds this rank's).  Ranks pad to the largest
    count, exchange equal blocks (dist.gather_rows) and drop the padding."""
    from . import dist as D_
    m = max(counts)
    pad = torch.zeros((m,) + tuple(t.shape[1:]), device=t.device, dtype=t.dtype)
    pad[:t.shape[0]] = t
    allr = D_.gather_rows(pad)
    keep = torch.cat([torch.arange(r * m, r * m + n, device=t.device) for r, n in enumerate(counts)])
    return allr.index_select(0, keep)


class EmbeddingBank:
    """Growing fp32 buffers of L2-normalised image and text embeddings [n, d] plus int64 labels [n] (-1 where none was given), filled batch
    by batch; row i of the image buffer pairs with row i of the text buffer."""

    def __init__(self, d: int, device, capacity: int = 1024):
        self.d, self.device = int(d), torch.device(device)
        self.n = 0
        self.local_start = 0                                   # of a gathered bank: where this rank's rows start
        self.local_count = 0
        self._img = torch.empty((capacity, self.d), device=self.device, dtype=torch.float32)
        self._txt = torch.empty((capacity, self.d), device=self.device, dtype=torch.float32)
        self._lab = torch.empty((capacity,), device=self.device, dtype=torch.int64)

    def reset(self):
        self.n = self.local_start = self.local_count = 0

    def __len__(self):
        return self.n

    @property
    def img(self) -> torch.Tensor:
        return self._img[:self.n]

    @property
    def txt(self) -> torch.Tensor:
        return self._txt[:self.n]

    @property
    def labels(self) -> torch.Tensor:
        return self._lab[:self.n]

    def _reserve(self, n: int):
        cap = self._img.shape[0]
        if n <= cap:
            return
        cap = max(n, 2 * cap)
        for name in ("_img", "_txt", "_lab"):
            old = getattr(self, name)
            new = torch.empty((cap,) + tuple(old.shape[1:]), device=self.device, dtype=old.dtype)
            new[:self.n] = old[:self.n]
            setattr(self, name, new)

    def add(self, img_g: torch.Tensor, txt_g: torch.Tensor, labels: Optional[torch.Tensor] = None, normalize: bool = True):
        """Append a batch (the rows are copied: views of an engine's workspace may be handed in).  normalize=False: the rows are unit rows
        already and are stored as they are (no kernel runs: CPU tests)."""
        b = img_g.shape[0]
        if img_g.shape != (b, self.d) or txt_g.shape != (b, self.d):
            raise ValueError(f"EmbeddingBank.add: expected [B, {self.d}] image and text embeddings, got {tuple(img_g.shape)} / {tuple(txt_g.shape)}")
        if labels is not None and labels.numel() != b:
            raise ValueError("EmbeddingBank.add: one label per pair")
        self._reserve(self.n + b)
        for buf, src in ((self._img, img_g), (self._txt, txt_g)):
            dst = buf[self.n:self.n + b]
            if normalize:
                ops.l2_normalize(src.to(torch.float32).contiguous(), dst)
            else:
                dst.copy_(src)
        if labels is None:
            self._lab[self.n:self.n + b] = -1
        else:
            self._lab[self.n:self.n + b] = labels.reshape(-1).to(device=self.device, dtype=torch.int64)
        self.n += b
        self.local_count = self.n

    def gather(self) -> "EmbeddingBank":
        """Under data parallelism: a bank of every rank's rows in rank order (ranks may hold different counts), with local_start /
        local_count marking this rank's share.  A single process gets itself back."""
        W, rank = _world()
        if W == 1:
            self.local_start, self.local_count = 0, self.n
            return self
        from . import dist as D_
        counts = [int(v) for v in D_.gather_rows(torch.tensor([self.n], device=self.device, dtype=torch.int64)).tolist()]
        out = EmbeddingBank(self.d, self.device, capacity=max(1, sum(counts)))
        out._img[:sum(counts)] = _gather_var(self.img, counts)
        out._txt[:sum(counts)] = _gather_var(self.txt, counts)
        out._lab[:sum(counts)] = _gather_var(self.labels, counts)
        out.n = sum(counts)
        out.local_start, out.local_count = sum(counts[:rank]), counts[rank]
        return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# reducers: plain torch, any device, no kernel call
# ---------------------------------------------------------------------------------------------------------------------------------------------
def recall_at_k(rank: torch.Tensor, ks: Sequence[int]) -> Dict[int, float]:
    """R@k = the share of queries whose target is among the k best keys (rank < k; rank 0 = best)."""
    n = rank.numel()
    return {int(k): (float((rank < k).sum()) / n if n else float("nan")) for k in ks}


def rank_stats(rank: torch.Tensor) -> Tuple[float, float]:
    """(mean, median) of the 0-based ranks; the median of an even count is the mean of the two middle values."""
    n = rank.numel()
    if n == 0:
        return float("nan"), float("nan")
    s = torch.sort(rank.reshape(-1).to(torch.float64)).values
    return float(s.mean()), float((s[(n - 1) // 2] + s[n // 2]) / 2)


def precision_at_k(top_idx: torch.Tensor, query_label: torch.Tensor, key_label: torch.Tensor, ks: Sequence[int]) -> Dict[int, float]:
    """P@k = the share of a query's k best keys that carry the query's label, averaged over the queries.  top_idx [N, K] (-1 = no key: a
    miss), k <= K."""
    N, K = top_idx.shape
    hit = (key_label.to(top_idx.device)[top_idx.clamp(min=0).long()] == query_label.to(top_idx.device).reshape(N, 1)) & (top_idx >= 0)
    out = {}
    for k in ks:
        if k > K:
            raise ValueError(f"precision_at_k: k = {k} exceeds the list length {K}")
        out[int(k)] = float(hit[:, :k].double().mean()) if N else float("nan")
    return out


def _class_hits(top_idx: torch.Tensor, label: torch.Tensor, k: int, C: int):
    """(hits [C], counts [C]) int64: per true class, the samples whose label is among the first k entries, and the samples."""
    label = label.to(top_idx.device).long().reshape(-1)
    hit = (top_idx[:, :k].long() == label.reshape(-1, 1)).any(dim=1)
    counts = torch.bincount(label, minlength=C)[:C]
    hits = torch.bincount(label[hit], minlength=C)[:C]
    return hits, counts


def topk_accuracy(top_idx: torch.Tensor, label: torch.Tensor, ks: Sequence[int], num_classes: Optional[int] = None):
    """{"acc": {k: accuracy@k}, "per_class": {k: float64 [C], NaN for a class without a sample}}: a sample counts at k when its label is
    among the first min(k, K) entries of its row of top_idx [N, K] (class indices, -1 = none)."""
    C = int(num_classes) if num_classes is not None else int(max(int(label.max()) + 1 if label.numel() else 0, int(top_idx.max()) + 1 if top_idx.numel() else 0))
    acc, per = {}, {}
    for k in ks:
        hits, counts = _class_hits(top_idx, label, int(k), C)
        acc[int(k)] = float(hits.sum()) / float(counts.sum()) if int(counts.sum()) else float("nan")
        per[int(k)] = hits.double() / counts.double()            # 0 / 0 = NaN where a class has no sample
    return {"acc": acc, "per_class": per}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _ranks(q: torch.Tensor, keys: torch.Tensor, lo: int, n: int) -> torch.Tensor:
    """0-based rank of key lo + i for query i (rows lo .. lo + n of q against all of keys)."""
    if n == 0:
        return torch.empty(0, device=q.device, dtype=I32)
    return ops.sim_rank(q[lo:lo + n], keys, torch.arange(lo, lo + n, device=q.device, dtype=I32))


def retrieval_metrics(bank: EmbeddingBank, ks: Sequence[int] = (1, 5, 10), top_k: bool = False) -> Dict[str, object]:
    """Image-to-text and text-to-image retrieval over the bank; query i pairs with key i.  Returns {d}_R@{k}, {d}_mean_rank and
    {d}_median_rank (0-based ranks, ties broken towards the lower key index) for d in (i2t, t2i), from two sim_rank launches - no list,
    no [N, N] matrix.  top_k=True adds {d}_top_val / {d}_top_idx [n, K] (K = min(max(ks), 16)) from sim_topk, for this rank's queries.
    Under data parallelism every rank scores its own query slice against the gathered keys and the per-query ranks are exchanged
    (4 bytes per query): the median needs them all, and every rank returns the same numbers."""
    W, _ = _world()
    g = bank.gather()
    lo, n = g.local_start, g.local_count
    out: Dict[str, object] = {}
    for name, q, keys in (("i2t", g.img, g.txt), ("t2i", g.txt, g.img)):
        r = _ranks(q, keys, lo, n)
        if top_k and n:
            K = min(max(int(k) for k in ks), ops.SIM_TOPK_MAX)
            out[f"{name}_top_val"], out[f"{name}_top_idx"] = ops.sim_topk(q[lo:lo + n], keys, K)
        if W > 1:
            from . import dist as D_
            counts = [int(v) for v in D_.gather_rows(torch.tensor([n], device=r.device, dtype=torch.int64)).tolist()]
            r = _gather_var(r, counts)
        for k, v in recall_at_k(r, ks).items():
            out[f"{name}_R@{k}"] = v
        out[f"{name}_mean_rank"], out[f"{name}_median_rank"] = rank_stats(r)
    return out


def class_embeddings(engine, prompt_ids: torch.Tensor, prompt_mask: torch.Tensor, chunk: int = 64, ema: bool = False) -> torch.Tensor:
    """Class embeddings [C, d] from prompt_ids / prompt_mask [C, Pn, T] (Pn prompts per class): every prompt is embedded with
    Engine.embed_text (`chunk` prompts per pass), normalised, averaged over its class and normalised again - CLIP's prompt ensembling.
    The last chunk is filled up with repeats of the first prompt so that the engine's workspace is sized once."""
    if prompt_ids.dim() != 3 or prompt_mask.shape != prompt_ids.shape:
        raise ValueError("class_embeddings: prompt_ids and prompt_mask must both be [C, Pn, T]")
    C, Pn, T = prompt_ids.shape
    ids, mask = prompt_ids.reshape(C * Pn, T), prompt_mask.reshape(C * Pn, T)
    chunk = max(1, min(int(chunk), C * Pn))
    emb = None
    for s in range(0, C * Pn, chunk):
        n = min(chunk, C * Pn - s)
        sel = torch.cat([torch.arange(s, s + n), torch.zeros(chunk - n, dtype=torch.long)]).to(ids.device)
        e = engine.embed_text(ids.index_select(0, sel), mask.index_select(0, sel), ema=ema)
        if emb is None:
            emb = torch.empty((C * Pn, e.shape[1]), device=e.device, dtype=torch.float32)
        emb[s:s + n] = e[:n]
    ops.l2_normalize(emb, emb)
    cls = emb.view(C, Pn, -1).mean(dim=1).contiguous()
    return ops.l2_normalize(cls, cls)


def zero_shot_metrics(bank_or_img, class_emb: torch.Tensor, labels: Optional[torch.Tensor] = None, ks: Sequence[int] = (1, 5)) -> Dict[str, object]:
    """Zero-shot classification: every image embedding (a bank's, already normalised, with its labels; or a [N, d] tensor, normalised here,
    with `labels`) is scored against the class embeddings [C, d] with sim_topk (Nk = C).  Returns zs_acc@{k} and zs_per_class_acc@{k}
    (float64 [C], NaN for a class without a sample).  Under data parallelism the per-class hit and sample counts are all-reduced."""
    if isinstance(bank_or_img, EmbeddingBank):
        img = bank_or_img.img
        labels = bank_or_img.labels if labels is None else labels
    else:
        img = ops.l2_normalize(bank_or_img.to(torch.float32).contiguous())
    if labels is None:
        raise ValueError("zero_shot_metrics: labels are needed")
    C = class_emb.shape[0]
    K = min(max(int(k) for k in ks), ops.SIM_TOPK_MAX)
    n = img.shape[0]
    top_idx = ops.sim_topk(img, class_emb.contiguous(), K)[1] if n else torch.empty((0, K), device=class_emb.device, dtype=I32)
    labels = labels.to(top_idx.device).long().reshape(-1)
    if n and (int(labels.min()) < 0 or int(labels.max()) >= C):
        raise ValueError(f"zero_shot_metrics: labels must lie in [0, {C})")
    W, _ = _world()
    out: Dict[str, object] = {}
    for k in ks:
        hits, counts = _class_hits(top_idx, labels, min(int(k), K), C)
        if W > 1:
            both = torch.stack([hits, counts])
            tdist.all_reduce(both)
            hits, counts = both[0], both[1]
        out[f"zs_acc@{int(k)}"] = float(hits.sum()) / float(counts.sum()) if int(counts.sum()) else float("nan")
        out[f"zs_per_class_acc@{int(k)}"] = hits.double() / counts.double()
    return out
