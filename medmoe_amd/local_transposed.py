"""GLoRIA local loss (reference losses.py:961-1026, attention_fn :698-736) on TRANSPOSED ragged pair matrices - the fast path for 196 / 64
regions (csrc/pair3.hip): score GEMM with the word softmax fused -> forward pair launch (sim, A, per-word sums) -> [a head over the
similarity matrix chosen by the caller: cross-entropy, Soft-GLoRIA, ...] -> backward pair launch (dS over the log-probabilities in place,
one row weight d2 per word) -> two wgrad-shaped GEMMs.  One implementation, with buffers of its own, for the fused `Engine.train_step` and
for `src.losses.GLORIALocalContrastiveLoss` behind torch autograd."""
from typing import Callable, Dict, Optional

import numpy as np
import torch

from . import ops

BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32


def ragged_layout(cap_lens, T: int, Tp: int):
    """Column layout of the local-loss pair matrices (losses.py:961-1026 computes them per pair; the build stores them
    as [B*HWp, Kp] matrices).  Caption i (clamped to 1..T words) belongs to length class ntt_i = ceil(len_i / 16) and is
    16*ntt_i columns wide; classes are stored one after the other, members in original order.
    Returns perm (captions in column order), col_of_cap[i] (first column), ntts[i], cap_of_chunk (caption of every 8-column
    chunk, -1 for the zero padding up to Kp), classes = [(ntt, first index into perm, count, first column)], Kc, Kp."""
    lens = np.clip(np.asarray(cap_lens, dtype=np.int64), 1, T)
    B = lens.shape[0]
    ntts = (lens + 15) // 16
    perm = np.argsort(ntts, kind="stable")                       # class-major, original order inside a class
    width = 16 * ntts[perm]
    start = np.concatenate(([0], np.cumsum(width)))              # first column of each caption, in perm order
    col_of_cap = np.empty(B, np.int64); col_of_cap[perm] = start[:-1]
    Kc = int(start[-1]); Kp = (Kc + 63) // 64 * 64
    cap_of_chunk = np.full(Kp // 8, -1, np.int64)
    cap_of_chunk[:Kc // 8] = np.repeat(perm, width // 8)
    classes, pos = [], 0
    for ntt in range(1, Tp // 16 + 1):
        n_c = int((ntts == ntt).sum())
        if n_c:
            classes.append((ntt, pos, n_c, int(start[pos])))
            pos += n_c
    return perm, col_of_cap, ntts, cap_of_chunk, classes, Kc, Kp


def grow_pair_buffers(pair: Dict[str, torch.Tensor], have: int, Kp: int, Bc: int, Tp: int, alloc: Callable[[int], Dict[str, torch.Tensor]]) -> int:
    """The ragged pair matrices are sized from the batch's own Kp = sum of pad16(caption length) instead of the Bc*Tp worst case (3 x 24 GB
    instead of 3 x 35 GB at B = 1024 with lengths uniform in 8..77).  `pair` holds a set of `have` columns; when a batch needs more, the set
    is replaced by alloc(capacity) with 10 % head-room, rounded to the GEMM k-step of 64 and never above the worst case.  Returns the
    capacity `pair` now has."""
    if Kp <= have:
        return have
    cap = min((Bc * Tp + 63) // 64 * 64, (int(Kp * 1.1) + 63) // 64 * 64)
    pair.clear()                                                  # release before allocating: the old and new sets must not coexist
    pair.update(alloc(cap))
    return cap


def local_sim_forward(ctx: torch.Tensor, words: torch.Tensor, cap_lens: torch.Tensor, cap_lens_host, temp1: float, temp2: float, *, P: int,
                      gm3: torch.Tensor, gm3_crowmap: torch.Tensor, img_tiles: torch.Tensor, img_tile_count: torch.Tensor,
                      wn: torch.Tensor, sim: torch.Tensor) -> torch.Tensor:
    """The similarity matrix alone, for evaluation (csrc/local_eval.hip): ctx bf16 [B*P, Do], words bf16 [Bc, T, Do], cap_lens int32 [Bc] on
    the device + the same lengths on the host -> sim fp32 [B, Bc] BEFORE temp3.  The Gram GEMM and the word norms are the training path's;
    the scores, the two softmaxes and the per-word sums of a pair then stay on the chip: no pair matrix exists, the workspace is the
    caller's gm3 [B*GR, GR] (zero outside [P, P]), wn [Bc, T] and sim."""
    Bc, T, Do = words.shape
    B = ctx.shape[0] // P
    d_perm, classes = local_word_norms(words, cap_lens_host, wn, P)
    local_gram(ctx, gm3, P=P, gm3_crowmap=gm3_crowmap, img_tiles=img_tiles, img_tile_count=img_tile_count)
    for ntt, start, n_c, _ in classes:
        ops.call("local_sim_fwd", ctx, words, cap_lens, gm3, wn, sim, B, Bc, P, T, Do, temp1, temp2, 1e-8, d_perm[start:start + n_c], n_c, ntt)
    return sim


def local_word_norms(words: torch.Tensor, cap_lens_host, wn: torch.Tensor, P: int):
    """The word norms of local_sim_forward into wn fp32 [Bc, T].  Returns (d_perm, classes): the captions in class-major order on the device
    and ragged_layout's class table [(ntt, first index into d_perm, count, first column)]."""
    Bc, T, Do = words.shape
    _, Tp, _ = ops.local_geometry(P, T)
    perm, col_of_cap, ntts, _, classes, _, Kp = ragged_layout(cap_lens_host, T, Tp)
    meta = torch.from_numpy(np.concatenate((perm, col_of_cap, 16 * ntts)).astype(np.int32)).to(words.device, non_blocking=True)
    d_perm, d_col, d_tp = meta[:Bc], meta[Bc:2 * Bc], meta[2 * Bc:]
    ops.call("words_prep_ragged", words, wn, None, Bc, T, Tp, Do, d_col, d_tp, Kp)                         # word norms only
    return d_perm, classes


def local_gram(ctx: torch.Tensor, gm3: torch.Tensor, *, P: int, gm3_crowmap: torch.Tensor, img_tiles: torch.Tensor,
               img_tile_count: torch.Tensor) -> torch.Tensor:
    """The Gram matrices ctx_b ctx_b^T of local_sim_forward into gm3 bf16 [B*GR, GR] (zero outside [P, P]: the GEMM only fills [P][P])."""
    ops.gemm_nt(ctx, ctx, gm3, c_rowmap=gm3_crowmap, tiles=img_tiles, tile_count=img_tile_count, max_tiles=img_tiles.shape[0],
                stride_b=P * ctx.shape[1], M=ctx.shape[0], N=P)
    return gm3


class LocalSimScratch:
    """The workspace of local_sim_forward / ops.local_sim_pairs for up to `B` images of P regions outside an engine (evaluation over a bank,
    medmoe_amd/retrieval.py): the Gram matrices with their row map and tile table.  gram_kw(n) = the keywords of local_gram /
    local_sim_forward for the first n images."""

    def __init__(self, B: int, P: int, device):
        self.B, self.P, self.GR, dev = int(B), int(P), (P + 31) // 32 * 32, torch.device(device)
        self.gm3 = torch.zeros(self.B * self.GR, self.GR, device=dev, dtype=BF)
        arg = torch.arange(self.B * P, device=dev)
        self.crowmap = (arg // P * self.GR + arg % P).to(I32)
        tl = [[b, m, (b + 1) * P, 0] for b in range(self.B) for m in range(b * P, (b + 1) * P, 128)]
        self.tiles = torch.tensor(tl, device=dev, dtype=I32)
        self.tiles_per_image = len(tl) // self.B
        self._count = {}

    def gram_kw(self, n: int):
        if not 1 <= n <= self.B:
            raise ValueError(f"LocalSimScratch: {n} images, sized for 1 .. {self.B}")
        nt = n * self.tiles_per_image
        if n not in self._count:
            self._count[n] = torch.tensor([nt], device=self.gm3.device, dtype=I32)
        return dict(P=self.P, gm3_crowmap=self.crowmap[:n * self.P], img_tiles=self.tiles[:nt], img_tile_count=self._count[n])


class TransposedLocalLoss:
    """forward(ctx, words, cap_lens, cap_lens_host, temp1, temp2) fills self.sim ([B, Bc] fp32, BEFORE temp3); the caller turns it into
    gsim = d loss / d sim; backward(gsim, out) writes the bf16 gradient of the region features into `out`.
    The instance owns its buffers.  Construction allocates what does not depend on the captions' lengths (wn, sim, lse, the Gram matrices
    gm3 and their tile tables, dGm32, dGmq, dC32q); the ragged pair matrices self.pair = {l_dS, l_A, (l_U,) words_r, l_stats3, (l_d2,)
    (l_dwn)} are sized on the first forward (`grow_pair_buffers`), so evaluation through `local_sim_forward` never allocates them."""
    host_lens = True                                              # forward also takes the caption lengths on the host (the class tables are built there)
    det = None                                                    # ops.DetScratch (deterministic mode): the wgrad-shaped GEMMs take their staged / single-writer forms

    def __init__(self, B: int, P: int, T: int, Do: int, device, gram: bool = True, Bc: Optional[int] = None, word_grad: bool = False,
                 pitch: Optional[int] = None, sim: Optional[torch.Tensor] = None):
        """pitch: region columns stored per (word, image) in the pair matrices, default HWp (208 for 196 regions).  224 makes every 64-byte
        wave segment 64-byte aligned (448-byte rows); measured on one box at batch 1024: pair launches 36.3 -> 37.1 ms and 7.7 % more GEMM
        work, step 234.6 -> 241.2 ms - not used.  sim: write the similarities into this fp32 [B, Bc] tensor of the caller's."""
        self.HWp, self.Tp, _ = ops.local_geometry(P, T)
        GR = (P + 31) // 32 * 32
        Q = self.HWp if pitch is None else pitch
        if Q % 8 or not P <= Q <= GR:
            raise ValueError(f"pair-matrix region pitch {Q}: need a multiple of 8 in [{P}, {GR}]")
        self.B, self.P, self.T, self.Do, self.HWq = B, P, T, Do, Q
        self.Bc = Bc = B if Bc is None else Bc                   # captions: B images against Bc captions (Bc > B: the gathered captions of all ranks)
        self.device, self.gram = torch.device(device), gram
        # word_grad: backward also returns d loss / d words (losses.py:985-1012 differentiates the word embeddings too; needed when the text
        # tower trains).  The pair matrices then use the ROW-MAJOR layout [word rows][image x region columns] (pitch ldk = B * HWq rounded up
        # to the GEMM k-step): the gradient through the scores, dS . ctx, is one NT GEMM over it.
        self.word_grad = word_grad
        self.ldk = (B * Q + 63) // 64 * 64
        dev = self.device
        self.wn = torch.empty(Bc, T, device=dev, dtype=F32)
        self.sim = torch.empty(B, Bc, device=dev, dtype=F32) if sim is None else sim
        self.lse = torch.empty(B * self.HWp, Bc, device=dev, dtype=F32)
        self.gm3 = torch.zeros(B * GR, GR, device=dev, dtype=BF)  # plain Gram matrices [B][GR][GR]: zero outside [P][P], the GEMM only fills [P][P]
        arg = torch.arange(B * P, device=dev)
        self.gm3_crowmap = (arg // P * GR + arg % P).to(I32)
        self.dGm32 = torch.empty(B, Q, Q, device=dev, dtype=F32); self.dGmq = torch.empty(B * Q, Q, device=dev, dtype=BF)
        self.dC32q = torch.zeros(B * Q, Do, device=dev, dtype=F32)
        self.rowoff_q = (torch.arange(B + 1, device=dev) * Q).to(I32)
        arq = torch.arange(B * Q, device=dev)
        self.ctx_xmap_q = (arq // Q * P + torch.clamp(arq % Q, max=P - 1)).to(I32)
        tl = [[b, m, (b + 1) * P, 0] for b in range(B) for m in range(b * P, (b + 1) * P, 128)]
        self.img_tiles = torch.tensor(tl, device=dev, dtype=I32); self.img_tile_count = torch.tensor([len(tl)], device=dev, dtype=I32)
        self.pair: Dict[str, torch.Tensor] = {}
        self.cap = 0                                              # columns the pair matrices hold
        self._st = None
        self.generation = 0                                       # forward calls so far: a backward must belong to the latest one

    standalone = classmethod(lambda cls, *a, **kw: cls(*a, **kw))     # the constructor under the name tests and notebooks call it by

    def _alloc_pair(self, cap: int) -> Dict[str, torch.Tensor]:
        B, Q, Do, dev = self.B, self.HWq, self.Do, self.device
        # row-major matrices are zero-filled once: their pad columns (beyond B * Q) are operands of the word-gradient GEMM
        mat = (lambda: torch.zeros((cap, self.ldk), device=dev, dtype=BF)) if self.word_grad else (lambda: torch.empty((B * Q, cap), device=dev, dtype=BF))
        pair = {name: mat() for name in (("l_A", "l_dS") if self.gram else ("l_A", "l_dS", "l_U"))}
        pair["words_r"] = torch.empty((cap, Do), device=dev, dtype=BF)
        pair["l_stats3"] = torch.empty((B, cap, 2), device=dev, dtype=F32)
        if self.gram:
            pair["l_d2"] = torch.empty((B, cap), device=dev, dtype=F32)
        if self.word_grad:
            pair["l_dwn"] = torch.empty((B, cap), device=dev, dtype=F32)
        return pair

    # --------------------------------------------------------------------------------------------------------------------------
    def forward(self, ctx: torch.Tensor, words: torch.Tensor, cap_lens: torch.Tensor, cap_lens_host, temp1: float, temp2: float,
                att: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ctx bf16 [B*P, Do] region features, words bf16 [Bc, T, Do], cap_lens int32 [Bc] on the device + the same lengths on the host
        (the class tables are built there), att: optional fp32 [B, T, P] for the attention maps of the matching pairs (B == Bc)."""
        B, Bc, P, T, Do, Tp, HWq = self.B, self.Bc, self.P, self.T, self.Do, self.Tp, self.HWq
        perm, col_of_cap, ntts, cap_of_chunk, classes, Kc, Kp = ragged_layout(cap_lens_host, T, Tp)
        # row r of the matrices = word t of caption cap_of_chunk[r // 8]: its row in `words` (rows of padding words point at a
        # real row: their dS is exactly zero)
        rows = np.arange(Kp, dtype=np.int64)
        cap_of_row = np.repeat(cap_of_chunk, 8)
        t_of_row = rows - col_of_cap[np.maximum(cap_of_row, 0)]
        word_row = np.where(cap_of_row >= 0, cap_of_row * T + np.minimum(t_of_row, T - 1), 0)
        meta = torch.from_numpy(np.concatenate((perm, col_of_cap, 16 * ntts, word_row)).astype(np.int32)).to(self.device, non_blocking=True)
        d_perm, d_col, d_tp, d_wrow = meta[:Bc], meta[Bc:2 * Bc], meta[2 * Bc:3 * Bc], meta[3 * Bc:]
        self.cap = grow_pair_buffers(self.pair, self.cap, Kp, Bc, Tp, self._alloc_pair)
        pair = self.pair
        # image-major: element (row, image, region) at image*Kp*HWq + row*HWq + region - one (image, caption, word tile) unit of the pair
        # kernel is 16 x 448 contiguous bytes, and an image's block is a plain [Kp][HWq] matrix for the two wgrad-shaped GEMMs
        # (measured against [row][image][region] at batch 1024: pair launches 44.5 -> 36.3 ms)
        if self.word_grad:                                       # row-major: element (row, image, region) at row*ldk + image*HWq + region
            ld, bs = self.ldk, HWq
            tr = lambda name: pair[name].view(-1)[:Kp * ld].view(Kp, ld)
        else:
            ld, bs = HWq, Kp * HWq
            tr = lambda name: pair[name].view(-1)[:B * bs].view(B, Kp, HWq)
        X, AT = tr("l_dS"), tr("l_A")                           # X: log2-probabilities, then dS in place
        UT = None if self.gram else tr("l_U")
        Wr = pair["words_r"][:Kp]
        stats, srows = pair["l_stats3"], pair["l_stats3"].shape[1]      # (num, n2) of every (image, caption word): forward -> backward launch
        if Kp > Kc:
            for t_ in ((X, AT) if self.gram else (X, AT, UT)):
                if self.word_grad:
                    t_[Kc:].zero_()
                else:
                    t_[:, Kc:].zero_()
        ops.call("words_prep_ragged", words, self.wn, None, Bc, T, Tp, Do, d_col, d_tp, Kp)               # word norms only (no transposed copy: wT = null)
        torch.index_select(words.view(Bc * T, Do), 0, d_wrow, out=Wr)
        ops.gemm_nt(ctx, ctx, self.gm3, c_rowmap=self.gm3_crowmap, tiles=self.img_tiles, tile_count=self.img_tile_count,
                    max_tiles=self.img_tiles.shape[0], stride_b=P * Do, M=B * P, N=P)
        for ntt, start, n_c, cbase in classes:
            members = d_perm[start:start + n_c]
            ops.call("local_scores_t", ctx, words, cap_lens, X, self.lse, B, Bc, P, T, Do, members, n_c, ntt, cbase, ld, bs)
            ops.call("local_pair3", X, None, AT, None, self.lse, self.gm3, self.wn, cap_lens, None, self.sim, att,
                     stats, srows, B, Bc, P, T, temp1, temp2, 1e-8, members, n_c, ntt, cbase, ld, bs, HWq, None)
        self._st = (ctx, cap_lens, classes, d_perm, Kp, X, AT, UT, Wr, stats, srows, ld, bs, temp1, temp2)
        if self.word_grad:
            # matrix row of every (caption, word): the rows of the words gradient are gathered back through it (-1: padding word)
            lens = np.clip(np.asarray(cap_lens_host, dtype=np.int64), 1, T)
            tpos = np.arange(T, dtype=np.int64)[None, :]
            row_of_word = np.where(tpos < lens[:, None], col_of_cap[:, None] + tpos, -1)
            self._wg = (words, torch.from_numpy(row_of_word.reshape(-1)).to(self.device, non_blocking=True))
        self.generation += 1
        return self.sim

    def backward(self, gsim: torch.Tensor, out: torch.Tensor, generation: Optional[int] = None) -> Optional[torch.Tensor]:
        """gsim fp32 [B, Bc] = d loss / d sim; out bf16 [B, P, Do] receives d loss / d region features.  The pair matrices of the
        forward pass are consumed in place: `generation` (the value of self.generation right after that forward) makes a backward that
        arrives after ANOTHER forward fail loudly instead of differentiating the wrong batch.
        word_grad instances return d loss / d words, fp32 [Bc, T, Do] (None otherwise)."""
        if generation is not None and generation != self.generation:
            raise RuntimeError("TransposedLocalLoss: backward of an earlier forward - the instance keeps ONE forward's pair matrices "
                               "(call backward before the next forward of the same geometry)")
        pair, B, Bc, P, T, Do, HWq = self.pair, self.B, self.Bc, self.P, self.T, self.Do, self.HWq
        ctx, cap_lens, classes, d_perm, Kp, X, AT, UT, Wr, stats, srows, ld, bs, temp1, temp2 = self._st
        d2 = None
        if self.gram:
            # dGm_b = sum over the words of d2 a a^T: the backward launch stores the row weight d2 (4 bytes per word) instead of the
            # matrix U = d2 * A, and the Gram GEMM scales its first operand's fragments (medmoe_gemm_tn_gram); rows no launch covers
            # must hold finite weights
            d2 = pair["l_d2"]
            d2.zero_()
        dwn = None
        if self.word_grad:
            dwn = pair["l_dwn"]
            dwn.zero_()
        for ntt, start, n_c, cbase in classes:
            members = d_perm[start:start + n_c]
            if dwn is not None:
                ops.call("local_pair3_wgrad", X, X, AT, UT, self.lse, self.gm3, self.wn, cap_lens, gsim, self.sim, None,
                         stats, srows, B, Bc, P, T, temp1, temp2, 1e-8, members, n_c, ntt, cbase, ld, bs, HWq, d2, dwn)
            else:
                ops.call("local_pair3", X, X, AT, UT, self.lse, self.gm3, self.wn, cap_lens, gsim, self.sim, None,
                         stats, srows, B, Bc, P, T, temp1, temp2, 1e-8, members, n_c, ntt, cbase, ld, bs, HWq, d2)
        dC = self.dC32q
        dC.zero_(); self.dGm32.zero_()
        # dC = dS^T . W with the B image blocks seen as ONE [Kp][B*HWq] operand (chunks of HWq columns, bs apart): full 256-column tiles
        ops.gemm_tn_cols(X, ld, Wr, Do, dC, Do, Kp, B * HWq, Do, 1, 0, 0, 0, HWq, bs, det=self.det)
        if self.gram:
            ops.gemm_tn_gram(AT, ld, d2, srows, 1, self.dGm32, HWq, Kp, HWq, B, bs, HWq * HWq, det=self.det)         # dGm_b = A_b^T diag(d2_b) A_b
        else:
            ops.gemm_tn_cols(UT, ld, AT, ld, self.dGm32, HWq, Kp, HWq, HWq, B, bs, bs, HWq * HWq, 0, 0, det=self.det)  # dGm_b = U_b^T A_b
        self.dGmq.copy_(self.dGm32.view(B * HWq, HWq))
        ops.gemm_tn(self.dGmq, ctx, dC.view(B, HWq, Do), x_rowmap=self.ctx_xmap_q, row_off=self.rowoff_q, n_groups=B,
                    stride_w=HWq * Do, nsplit=1, M=B * HWq, det=self.det)                    # dC_b += dGm_b . ctx_b
        ops.call("unpad_cast", dC, out, B, P, HWq, Do)
        if not self.word_grad:
            return None
        # ---- d loss / d words (losses.py:985-1012): through the scores S = ctx . w  ->  dS . ctx, one NT GEMM over the row-major dS with
        # the contraction over (image, region); through the word's own norm in the cosine -> (sum over images of dwn) * w ----
        words, row_of_word = self._wg
        ctxT = torch.zeros(Do, self.ldk, device=self.device, dtype=BF)
        ctxT[:, :B * HWq] = ctx.index_select(0, self.ctx_xmap_q.long()).t()        # pad regions repeat a row: their dS columns are exact zeros
        dW = torch.empty(Kp, Do, device=self.device, dtype=F32)
        ops.gemm_nt(X, ctxT, dW)
        cw = dwn[:, :Kp].sum(dim=0)
        sel = row_of_word.clamp(min=0)
        g = dW.index_select(0, sel) + cw.index_select(0, sel)[:, None] * words.reshape(Bc * T, Do).float()
        return (g * (row_of_word >= 0)[:, None]).view(Bc, T, Do)
