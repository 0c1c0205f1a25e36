"""Retrieval and zero-shot evaluation on the global embeddings: image <-> text recall@K / mean and median rank over a whole
evaluation set, and zero-shot classification against prompt-ensembled class embeddings.

The scoring runs on two HIP launches (medmoe_amd.ops.sim_rank / sim_topk, csrc/retrieval.hip) that stream the keys past the queries and
keep only a rank or the K best entries per query: the [N, N] similarity matrix of an evaluation set is never stored.  Everything else in
this file - the growing bank, the gather across data-parallel ranks, the reducers - is plain torch and runs on any device.

Embeddings are L2-normalised on the way into the bank with eps = 1e-8, the clamp of medmoe_cos_scale, so the product of two rows is the
reference's cosine (losses.py:781-785) whenever both norms are above eps.

Candidate re-ranking with the GLoRIA local similarity: the model trains on the global AND the local loss, so a checkpoint can
also be ranked on both.  Scoring every pair of an evaluation set locally is quadratic; instead each query's K best keys by global
similarity (sim_topk) are scored with the local similarity (ops.local_sim_pairs: listed pairs, grouped by image) and re-ordered by the
weighted sum.  The region and word features come from a LocalBank filled beside the EmbeddingBank."""
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
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


class LocalBank:
    """Growing buffers of the LOCAL features beside an EmbeddingBank, row i of each belonging to pair i: img_l bf16 [n, P, D] (region
    features), words bf16 [n, T, D], cap_lens int32 [n]; the same doubling policy.  The loss weights and temperatures the local similarity
    is combined and computed with travel with the bank (an engine's cfg.w_global / w_local / temp1 / temp2)."""

    def __init__(self, P: int, T: int, D: int, device, capacity: int = 1024, w_global: float = 0.5, w_local: float = 0.5,
                 temp1: float = 4.0, temp2: float = 5.0):
        self.P, self.T, self.D, self.device = int(P), int(T), int(D), torch.device(device)
        self.w_global, self.w_local, self.temp1, self.temp2 = float(w_global), float(w_local), float(temp1), float(temp2)
        self.n = 0
        self._img_l = torch.empty((capacity, self.P, self.D), device=self.device, dtype=torch.bfloat16)
        self._words = torch.empty((capacity, self.T, self.D), device=self.device, dtype=torch.bfloat16)
        self._cap = torch.empty((capacity,), device=self.device, dtype=I32)

    @classmethod
    def for_engine(cls, engine, capacity: int = 1024) -> "LocalBank":
        c = engine.cfg
        if c.d_t != c.d_out:
            raise NotImplementedError(f"model.retrieval.local: word features of width d_t = {c.d_t} against regions of d_out = {c.d_out}")
        return cls(c.n_patch, c.max_len, c.d_out, engine.device, capacity, c.w_global, c.w_local, c.temp1, c.temp2)

    def reset(self):
        self.n = 0

    def __len__(self):
        return self.n

    @property
    def img_l(self) -> torch.Tensor:
        return self._img_l[:self.n]

    @property
    def words(self) -> torch.Tensor:
        return self._words[:self.n]

    @property
    def cap_lens(self) -> torch.Tensor:
        return self._cap[:self.n]

    def _reserve(self, n: int):
        cap = self._cap.shape[0]
        if n <= cap:
            return
        cap = max(n, 2 * cap)
        for name in ("_img_l", "_words", "_cap"):
            old = getattr(self, name)
            new = torch.empty((cap,) + tuple(old.shape[1:]), device=self.device, dtype=old.dtype)
            new[:self.n] = old[:self.n]
            setattr(self, name, new)

    def add_features(self, img_l: torch.Tensor, words: torch.Tensor, cap_lens: torch.Tensor):
        """Append a batch: img_l [B, P, D], words [B, T, D] (stored as bf16), cap_lens [B].  The rows are copied."""
        b = img_l.shape[0]
        if tuple(img_l.shape) != (b, self.P, self.D) or tuple(words.shape) != (b, self.T, self.D) or cap_lens.numel() != b:
            raise ValueError(f"LocalBank.add_features: expected [B, {self.P}, {self.D}] regions, [B, {self.T}, {self.D}] words and [B] lengths, "
                             f"got {tuple(img_l.shape)} / {tuple(words.shape)} / {tuple(cap_lens.shape)}")
        self._reserve(self.n + b)
        self._img_l[self.n:self.n + b].copy_(img_l)
        self._words[self.n:self.n + b].copy_(words)
        self._cap[self.n:self.n + b].copy_(cap_lens.reshape(-1))
        self.n += b

    def add(self, engine):
        """The local features an `embed` / `eval_step` forward of `engine` has just left in its workspace."""
        self.add_features(engine.ws["img_l"], engine.ws["words"], engine.cap_lens)


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


def rerank_ranks(top_idx: torch.Tensor, combined: torch.Tensor, target: torch.Tensor, global_rank: torch.Tensor) -> torch.Tensor:
    """The 0-based rank of every query's target after its candidate list top_idx [N, K] (key indices, -1 = none) was re-scored with
    combined [N, K].  A target inside its list: the number of candidates ordered before it under (combined score descending, key index
    ascending).  A target outside keeps global_rank[i] - it is >= K, and no key outside the list can overtake a listed one.  int64 [N]."""
    target = target.reshape(-1, 1).to(top_idx.device).long()
    idx = top_idx.long()
    valid = idx >= 0
    hit = valid & (idx == target)
    inside = hit.any(dim=1)
    ts = torch.where(hit, combined, torch.zeros_like(combined)).sum(dim=1, keepdim=True)        # the target's score (a list names a key once)
    before = valid & ((combined > ts) | ((combined == ts) & (idx < target)))
    return torch.where(inside, before.sum(dim=1), global_rank.reshape(-1).to(top_idx.device).long())


def build_pair_units(cand_idx, query_is_image: bool, cap_lens_host, T: int, unit_cap: int = 16) -> Dict[int, Tuple[np.ndarray, np.ndarray, np.ndarray]]:
    """The tables of ops.local_sim_pairs for a candidate matrix cand_idx [Nq, K] (key indices, -1 = none): {length class ntt: (units int32
    [n, 4] = (image, first entry, entry count, 0), pair_cap int32 [e], pair_slot int32 [e])}.  Entry e is the pair (image, caption
    pair_cap[e]) and pair_slot[e] = q * K + position its place in the flattened matrix.  query_is_image (i2t): the image is the query row,
    the caption the candidate; otherwise (t2i) the image is the candidate, and one image may collect many captions.  Within a class the
    entries are grouped by image in ascending order and every image's run is cut into units of at most unit_cap entries.  cap_lens_host:
    the length of every caption (clamped to 1 .. T as the kernels do).  Pure numpy."""
    cand = np.asarray(cand_idx.cpu().numpy() if torch.is_tensor(cand_idx) else cand_idx).astype(np.int64)
    if cand.ndim != 2:
        raise ValueError("build_pair_units: cand_idx must be [Nq, K]")
    unit_cap = int(unit_cap)
    if unit_cap < 1:
        raise ValueError(f"build_pair_units: unit_cap must be >= 1, got {unit_cap}")
    lens = np.clip(np.asarray(cap_lens_host, dtype=np.int64).reshape(-1), 1, int(T))
    K = cand.shape[1]
    q, pos = np.nonzero(cand >= 0)
    key = cand[q, pos]
    slot = q * K + pos
    img, cap = (q, key) if query_is_image else (key, q)
    ntt = (lens[cap] + 15) // 16
    out = {}
    for c in np.unique(ntt):
        m = np.nonzero(ntt == c)[0]
        m = m[np.argsort(img[m], kind="stable")]                      # grouped by image; a stable sort keeps (query, position) order inside
        im = img[m]
        start = np.nonzero(np.concatenate(([True], im[1:] != im[:-1])))[0]             # first entry of every image's run
        length = np.diff(np.concatenate((start, [im.shape[0]])))
        pieces = (length + unit_cap - 1) // unit_cap
        run = np.repeat(np.arange(start.shape[0]), pieces)
        within = np.arange(run.shape[0]) - np.repeat(np.cumsum(pieces) - pieces, pieces)
        units = np.zeros((run.shape[0], 4), np.int32)
        units[:, 0] = im[start][run]
        units[:, 1] = start[run] + within * unit_cap
        units[:, 2] = np.minimum(unit_cap, length[run] - within * unit_cap)
        out[int(c)] = (units, cap[m].astype(np.int32), slot[m].astype(np.int32))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _ranks(q: torch.Tensor, keys: torch.Tensor, lo: int, n: int) -> torch.Tensor:
    """0-based rank of key lo + i for query i (rows lo .. lo + n of q against all of keys)."""
    if n == 0:
        return torch.empty(0, device=q.device, dtype=I32)
    return ops.sim_rank(q[lo:lo + n], keys, torch.arange(lo, lo + n, device=q.device, dtype=I32))


def _local_refuse(local_bank: LocalBank, n: int):
    """What the local re-ranking does not cover, by the configuration key that asks for it."""
    W, _ = _world()
    if W > 1:
        raise NotImplementedError("model.retrieval.local under data parallelism (WORLD_SIZE > 1): the local banks are not gathered across "
                                  "ranks - a named follow-up (DESIGN 3q)")
    if not ops.local_pair3_supported(local_bank.P, local_bank.T) or local_bank.D % 64:
        raise NotImplementedError(f"model.retrieval.local with {local_bank.P} regions x {local_bank.T} words at width {local_bank.D}: the listed-"
                                  "pair kernel covers 196 regions with up to 80 words and 64 regions with up to 16, width a multiple of 64 "
                                  "(local_pair3_supported); the 256 / 576 regions of cfg4 / cfg3 are a named follow-up (DESIGN 3q)")
    if len(local_bank) != n:
        raise ValueError(f"the LocalBank holds {len(local_bank)} pairs, the embeddings {n}: fill both from the same batches")


def _local_weights(local_bank: LocalBank, weights, agg: str, temp1, temp2):
    wg, wl = (local_bank.w_global, local_bank.w_local) if weights is None else (float(weights[0]), float(weights[1]))
    if not wg + wl > 0.0 or wg < 0.0 or wl < 0.0:
        raise ValueError(f"local weights must be >= 0 with a positive sum, got {(wg, wl)}")
    if agg not in ("sum", "mean"):
        raise ValueError(f"local_agg must be 'sum' or 'mean', got {agg!r}")
    return wg, wl, local_bank.temp1 if temp1 is None else float(temp1), local_bank.temp2 if temp2 is None else float(temp2)


def local_rerank(bank: EmbeddingBank, local_bank: LocalBank, k: int = 16, weights: Optional[Sequence[float]] = None, agg: str = "sum",
                 temp1: Optional[float] = None, temp2: Optional[float] = None, chunk: int = 1024, unit_cap: int = 16) -> Dict[str, Dict[str, torch.Tensor]]:
    """Candidate re-ranking of both retrieval directions.  Per direction d in (i2t, t2i): the k best keys of every query by
    global cosine (sim_topk, k <= 16 and <= the bank size); the local similarity of exactly those (query, candidate) pairs, the images
    taken `chunk` at a time (the Gram GEMM and the word norms of local_sim_forward, then one local_sim_pairs launch per caption length
    class); combined = (w_g cos_global + w_l sim_local) / (w_g + w_l), weights default to the bank's (cfg.w_global, cfg.w_local), agg =
    "mean" takes log(len) off sim_local as src/losses.py does for the loss; the target's new rank by rerank_ranks.
    Returns {d: {"rank" int64 [N], "top_idx" int32 [N, k], "global" / "local" / "combined" fp32 [N, k]}}."""
    from .local_transposed import LocalSimScratch, local_gram, local_word_norms
    N = len(bank)
    _local_refuse(local_bank, N)
    wg, wl, temp1, temp2 = _local_weights(local_bank, weights, agg, temp1, temp2)
    if int(k) != k or not 1 <= k <= ops.SIM_TOPK_MAX:
        raise ValueError(f"local_rerank: k must be an integer in 1 .. {ops.SIM_TOPK_MAX}, got {k!r}")
    out: Dict[str, Dict[str, torch.Tensor]] = {}
    if N == 0:
        return out
    k, chunk = min(int(k), N), max(1, min(int(chunk), N))
    P, T, D = local_bank.P, local_bank.T, local_bank.D
    GR = (P + 31) // 32 * 32
    dev = bank.img.device
    words, caps = local_bank.words, local_bank.cap_lens
    lens_host = caps.cpu().numpy().astype(np.int64)
    wn = torch.empty(N, T, device=dev, dtype=torch.float32)
    local_word_norms(words, lens_host, wn, P)
    scratch = LocalSimScratch(chunk, P, dev)
    loglen = torch.log(caps.clamp(min=1, max=T).float())
    target = torch.arange(N, device=dev)
    for name, q, keys, q_is_img in (("i2t", bank.img, bank.txt, True), ("t2i", bank.txt, bank.img, False)):
        val, idx = ops.sim_topk(q, keys, k)
        tables = build_pair_units(idx, q_is_img, lens_host, T, unit_cap)
        loc = torch.full((N, k), float("nan"), device=dev, dtype=torch.float32)
        for lo in range(0, N, chunk):
            n = min(chunk, N - lo)
            todo = []
            for ntt, (units, pair_cap, pair_slot) in tables.items():
                u0, u1 = np.searchsorted(units[:, 0], (lo, lo + n))
                if u1 > u0:
                    e0, e1 = int(units[u0, 1]), int(units[u1 - 1, 1] + units[u1 - 1, 2])
                    sub = units[u0:u1].copy()
                    sub[:, 0] -= lo; sub[:, 1] -= e0
                    todo.append((ntt, sub, pair_cap[e0:e1], pair_slot[e0:e1]))
            if not todo:
                continue
            ctx = local_bank.img_l[lo:lo + n].view(n * P, D)
            gm3 = local_gram(ctx, scratch.gm3[:n * GR], **scratch.gram_kw(n))
            for ntt, sub, pair_cap, pair_slot in todo:
                ops.local_sim_pairs(ctx, words, caps, gm3, wn, loc, sub, pair_cap, pair_slot, P=P, ntt=ntt, temp1=temp1, temp2=temp2,
                                    cap_lens_host=lens_host)
        if agg == "mean":
            loc = loc - (loglen[idx.clamp(min=0).long()] if q_is_img else loglen.reshape(N, 1))
        combined = (wg * val + wl * loc) / (wg + wl)
        rank = rerank_ranks(idx, combined, target, _ranks(q, keys, 0, N))
        out[name] = {"rank": rank, "top_idx": idx, "global": val, "local": loc, "combined": combined}
    return out


def retrieval_metrics(bank: EmbeddingBank, ks: Sequence[int] = (1, 5, 10), top_k: bool = False, local: Optional[LocalBank] = None,
                      local_k: int = 16, local_weights: Optional[Sequence[float]] = None, local_agg: str = "sum",
                      local_chunk: int = 1024) -> Dict[str, object]:
    """Image-to-text and text-to-image retrieval over the bank; query i pairs with key i.  Returns {d}_R@{k}, {d}_mean_rank and
    {d}_median_rank (0-based ranks, ties broken towards the lower key index) for d in (i2t, t2i), from two sim_rank launches - no list,
    no [N, N] matrix.  top_k=True adds {d}_top_val / {d}_top_idx [n, K] (K = min(max(ks), 16)) from sim_topk, for this rank's queries.
    Under data parallelism every rank scores its own query slice against the gathered keys and the per-query ranks are exchanged
    (4 bytes per query): the median needs them all, and every rank returns the same numbers.
    local = a LocalBank filled from the same batches: adds {d}_local_R@{k}, {d}_local_mean_rank and {d}_local_median_rank, the ranks after
    re-ranking each query's local_k best keys with the combined global + local similarity (local_rerank; max(ks) <= local_k <= 16, one
    rank only); the global-only keys stay beside them with their values."""
    if local is not None and max(int(k) for k in ks) > int(local_k):
        raise ValueError(f"retrieval_metrics: R@{max(int(k) for k in ks)} needs a candidate list at least that deep, local_k = {local_k} "
                         "(a target outside its list keeps its global rank)")
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
    if local is not None:
        for name, res in local_rerank(bank, local, local_k, local_weights, local_agg, chunk=local_chunk).items():
            for k, v in recall_at_k(res["rank"], ks).items():
                out[f"{name}_local_R@{k}"] = v
            out[f"{name}_local_mean_rank"], out[f"{name}_local_median_rank"] = rank_stats(res["rank"])
    return out


def class_embeddings(engine, prompt_ids: torch.Tensor, prompt_mask: torch.Tensor, chunk: int = 64, ema: bool = False) -> torch.Tensor:
    """Class embeddings [C, d] from prompt_ids / prompt_mask [C, Pn, T] (Pn prompts per class): every prompt is embedded with
    Engine.embed_text (`chunk` prompts per pass), normalised, averaged over its class and normalised again - CLIP's prompt ensembling.
    The last chunk is filled up with repeats of the first prompt so that the engine's workspace is sized once."""
    C, Pn, _ = _prompt_shape("class_embeddings", prompt_ids, prompt_mask)
    emb = _prompt_passes(engine, prompt_ids, prompt_mask, chunk, ema, False)[0]
    ops.l2_normalize(emb, emb)
    cls = emb.view(C, Pn, -1).mean(dim=1).contiguous()
    return ops.l2_normalize(cls, cls)


def _prompt_shape(name, prompt_ids, prompt_mask):
    if prompt_ids.dim() != 3 or prompt_mask.shape != prompt_ids.shape:
        raise ValueError(f"{name}: prompt_ids and prompt_mask must both be [C, Pn, T]")
    return tuple(prompt_ids.shape)


def _prompt_passes(engine, prompt_ids, prompt_mask, chunk, ema, want_words):
    """(sentence embeddings fp32 [C*Pn, d], word features bf16 [C*Pn, T, d] or None, lengths int32 [C*Pn] or None) of every prompt from
    Engine.embed_text passes of `chunk` prompts."""
    C, Pn, T = prompt_ids.shape
    ids, mask = prompt_ids.reshape(C * Pn, T), prompt_mask.reshape(C * Pn, T)
    chunk = max(1, min(int(chunk), C * Pn))
    emb = words = lens = None
    for s in range(0, C * Pn, chunk):
        n = min(chunk, C * Pn - s)
        sel = torch.cat([torch.arange(s, s + n), torch.zeros(chunk - n, dtype=torch.long)]).to(ids.device)
        e = engine.embed_text(ids.index_select(0, sel), mask.index_select(0, sel), ema=ema)
        if emb is None:
            emb = torch.empty((C * Pn, e.shape[1]), device=e.device, dtype=torch.float32)
            if want_words:
                w = engine.ws["words"]
                words = torch.empty((C * Pn,) + tuple(w.shape[1:]), device=w.device, dtype=w.dtype)
                lens = torch.empty((C * Pn,), device=w.device, dtype=I32)
        emb[s:s + n] = e[:n]
        if want_words:
            words[s:s + n] = engine.ws["words"][:n]
            lens[s:s + n] = engine.cap_lens[:n]
    return emb, words, lens


def class_prompt_words(engine, prompt_ids: torch.Tensor, prompt_mask: torch.Tensor, chunk: int = 64, ema: bool = False):
    """(words bf16 [C*Pn, T, d], lengths int32 [C*Pn]): the word features and caption lengths of every class prompt, from the
    Engine.embed_text passes class_embeddings makes (the same chunks, so the same launches) - the captions of the local zero-shot score."""
    _prompt_shape("class_prompt_words", prompt_ids, prompt_mask)
    _, words, lens = _prompt_passes(engine, prompt_ids, prompt_mask, chunk, ema, True)
    return words, lens


def _zero_shot_local_top(img: torch.Tensor, class_emb: torch.Tensor, local, K: int, weights, agg: str, chunk: int) -> torch.Tensor:
    """The K best classes [N, K] under (w_g cos(image, class embedding) + w_l mean over the class's prompts of the local similarity) /
    (w_g + w_l), ordered (score descending, class index ascending).  The local similarities are local_sim_forward's - all images against
    all C * Pn prompts is what that kernel does - image chunk by image chunk; the [N, C] score matrix is small and sorted with torch."""
    from .local_transposed import LocalSimScratch, local_sim_forward
    local_bank, p_words, p_lens = local
    N, C = img.shape[0], class_emb.shape[0]
    _local_refuse(local_bank, N)
    wg, wl, temp1, temp2 = _local_weights(local_bank, weights, agg, None, None)
    P, T, D = local_bank.P, local_bank.T, local_bank.D
    p_words = p_words.reshape(-1, T, D).contiguous()
    p_lens = p_lens.reshape(-1).to(device=img.device, dtype=I32).contiguous()
    n_p = p_words.shape[0]
    if n_p == 0 or n_p % C or p_lens.numel() != n_p:
        raise ValueError(f"zero_shot_metrics: {n_p} prompts with {p_lens.numel()} lengths for {C} classes - the same number of prompts per class")
    lens_host = p_lens.cpu().numpy().astype(np.int64)
    chunk = max(1, min(int(chunk), N))
    GR = (P + 31) // 32 * 32
    scratch = LocalSimScratch(chunk, P, img.device)
    wn = torch.empty(n_p, T, device=img.device, dtype=torch.float32)
    sim = torch.empty(chunk, n_p, device=img.device, dtype=torch.float32)
    score = torch.empty(N, C, device=img.device, dtype=torch.float32)
    loglen = torch.log(p_lens.clamp(min=1, max=T).float()).reshape(1, n_p)
    for lo in range(0, N, chunk):
        n = min(chunk, N - lo)
        s = local_sim_forward(local_bank.img_l[lo:lo + n].view(n * P, D), p_words, p_lens, lens_host, temp1, temp2, gm3=scratch.gm3[:n * GR],
                              wn=wn, sim=sim[:n], **scratch.gram_kw(n))
        if agg == "mean":
            s = s - loglen
        score[lo:lo + n] = (wg * (img[lo:lo + n] @ class_emb.t()) + wl * s.view(n, C, n_p // C).mean(dim=2)) / (wg + wl)
    order = torch.sort(score, dim=1, descending=True, stable=True).indices[:, :K].to(I32)
    if order.shape[1] < K:
        order = torch.cat([order, torch.full((N, K - order.shape[1]), -1, device=order.device, dtype=I32)], dim=1)
    return order


def zero_shot_metrics(bank_or_img, class_emb: torch.Tensor, labels: Optional[torch.Tensor] = None, ks: Sequence[int] = (1, 5),
                      local=None, local_weights: Optional[Sequence[float]] = None, local_agg: str = "sum",
                      local_chunk: int = 1024) -> Dict[str, object]:
    """Zero-shot classification: every image embedding (a bank's, already normalised, with its labels; or a [N, d] tensor, normalised here,
    with `labels`) is scored against the class embeddings [C, d] with sim_topk (Nk = C).  Returns zs_acc@{k} and zs_per_class_acc@{k}
    (float64 [C], NaN for a class without a sample).  Under data parallelism the per-class hit and sample counts are all-reduced.
    local = (LocalBank of the same images, prompt_words, prompt_lens) with the prompts' word features and lengths of class_prompt_words
    ([C*Pn, T, d] / [C*Pn], class-major): adds zs_local_acc@{k} and zs_local_per_class_acc@{k}, the class score being the weighted sum of
    the global cosine and the mean over the class's prompts of the GLoRIA local similarity (one rank only)."""
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
    tops = [("zs", top_idx)]
    if local is not None and n:
        tops.append(("zs_local", _zero_shot_local_top(img, class_emb.contiguous(), local, K, local_weights, local_agg, local_chunk)))
    for prefix, top in tops:
        for k in ks:
            hits, counts = _class_hits(top, labels, min(int(k), K), C)
            if W > 1:
                both = torch.stack([hits, counts])
                tdist.all_reduce(both)
                hits, counts = both[0], both[1]
            out[f"{prefix}_acc@{int(k)}"] = float(hits.sum()) / float(counts.sum()) if int(counts.sum()) else float("nan")
            out[f"{prefix}_per_class_acc@{int(k)}"] = hits.double() / counts.double()
    return out
