"""GLoRIA local loss (reference losses.py:961-1026) on RAGGED [region][word] pair matrices - the LDS-tiled pair kernels for 256 regions
(and for 196 / 64 regions with MEDMOE_LOCAL_PAIR3=0, for A/B runs against medmoe_amd/local_transposed.py).

The [B*HWp, B*Tp] score / gradient matrices are the largest tensors of the step (3 x 35 GB at B = 1024) and most of their columns are
caption padding.  Captions are grouped into length classes (<= 16, 32, ... words); class c stores its members side by side, 16*c columns
each, so a row is Kp = sum_i pad16(len_i) (rounded up to 64) columns instead of B*Tp (`ragged_layout`).  That needs the lengths on the host."""
from typing import Dict, Optional

import numpy as np
import torch

from . import ops
from .local_transposed import grow_pair_buffers, ragged_layout

BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32


class RaggedLocalLoss:
    """forward(ctx, words, cap_lens, cap_lens_host, temp1, temp2) fills self.sim ([B, B] fp32, BEFORE temp3) - its pair launch already
    leaves the gradients for d loss / d sim = 1; the caller turns sim into gsim = d loss / d sim; backward(gsim, out) scales them per pair
    and writes the bf16 gradient of the region features into `out`.  The instance owns its buffers; the pair matrices self.pair =
    {l_A, l_dS, l_U, wT} are sized on the first forward (`grow_pair_buffers`)."""
    host_lens = True                                              # forward also takes the caption lengths on the host (the class tables are built there)
    det = None                                                    # ops.DetScratch (deterministic mode), handed to the wgrad-shaped GEMM

    def __init__(self, B: int, P: int, T: int, Do: int, device, sim: Optional[torch.Tensor] = None):
        """sim: write the similarities into this fp32 [B, B] tensor of the caller's."""
        self.B, self.Bc, self.P, self.T, self.Do = B, B, P, T, Do
        self.device = dev = torch.device(device)
        HWp, Tp, GW = ops.local_geometry(P, T)
        self.HWp, self.Tp = HWp, Tp
        self.wn = torch.empty(B, T, device=dev, dtype=F32)
        self.sim = torch.empty(B, B, device=dev, dtype=F32) if sim is None else sim
        self.lse = torch.empty(B * HWp, B, device=dev, dtype=F32)
        self.gmp = torch.zeros(B * HWp, GW, device=dev, dtype=BF)
        self.dGm = torch.empty(B * HWp, HWp, device=dev, dtype=BF)
        self.dC32 = torch.zeros(B * HWp, Do, device=dev, dtype=F32)
        # static per-image group tables
        tiles = lambda rows, step: [[b, m, (b + 1) * rows, 0] for b in range(B) for m in range(b * rows, (b + 1) * rows, step)]
        table = lambda tl: (torch.tensor(tl, device=dev, dtype=I32).reshape(-1, 4), torch.tensor([len(tl)], device=dev, dtype=I32))
        self.img_tiles, self.img_tile_count = table(tiles(P, 128))
        self.imgp_tiles, self.imgp_tile_count = table(tiles(HWp, 128))
        self.imgp_tiles256, self.imgp_tile256_count = table(tiles(HWp, 256) if HWp <= 256 else [])      # one 256-row tile per image
        ar = torch.arange(B * P, device=dev)
        self.gm_crowmap = (ar // P * HWp + ar % P).to(I32)
        self.imgp_row_off = (torch.arange(B + 1, device=dev) * HWp).to(I32)
        arp = torch.arange(B * HWp, device=dev)
        self.ctx_xmap = (arp // HWp * P + torch.clamp(arp % HWp, max=P - 1)).to(I32)
        self.pair: Dict[str, torch.Tensor] = {}
        self.cap = 0                                              # columns the pair matrices hold
        self._st = None

    def _alloc_pair(self, cap: int) -> Dict[str, torch.Tensor]:
        pair = {name: torch.empty((self.B * self.HWp, cap), device=self.device, dtype=BF) for name in ("l_A", "l_dS", "l_U")}
        pair["wT"] = torch.empty((self.Do, cap), device=self.device, dtype=BF)
        return pair

    def forward(self, ctx: torch.Tensor, words: torch.Tensor, cap_lens: torch.Tensor, cap_lens_host, temp1: float, temp2: float) -> torch.Tensor:
        """ctx bf16 [B*P, Do] region features, words bf16 [B, T, Do], cap_lens int32 [B] on the device + the same lengths on the host."""
        B, P, T, Do, HWp, Tp = self.B, self.P, self.T, self.Do, self.HWp, self.Tp
        perm, col_of_cap, ntts, cap_of_chunk, classes, Kc, Kp = ragged_layout(cap_lens_host, T, Tp)
        meta = torch.from_numpy(np.concatenate((perm, col_of_cap, 16 * ntts, cap_of_chunk)).astype(np.int32)).to(self.device, non_blocking=True)
        d_perm, d_col, d_tp, d_chunk = meta[:B], meta[B:2 * B], meta[2 * B:3 * B], meta[3 * B:]
        self.cap = grow_pair_buffers(self.pair, self.cap, Kp, B, Tp, self._alloc_pair)
        rag = lambda name: self.pair[name].view(-1)[:B * HWp * Kp].view(B * HWp, Kp)
        lA, ldS, lU = rag("l_A"), rag("l_dS"), rag("l_U")
        wT = self.pair["wT"].view(-1)[:Do * Kp].view(Do, Kp)
        if Kp > Kc:
            for t_ in (lA, ldS, lU, wT):
                t_[:, Kc:].zero_()
        ops.call("words_prep_ragged", words, self.wn, wT, B, T, Tp, Do, d_col, d_tp, Kp)
        ops.gemm_nt(ctx, ctx, self.gmp, c_rowmap=self.gm_crowmap, tiles=self.img_tiles, tile_count=self.img_tile_count,
                    max_tiles=self.img_tiles.shape[0], stride_b=P * Do, M=B * P, N=P, col_perm=True)
        for ntt, start, n_c, cbase in classes:
            members = d_perm[start:start + n_c]
            # all word-region scores of the class as ONE tiled GEMM with the word-softmax fused (A1 + row LSE); the
            # A1 tiles live in the l_A buffer (each pair's tile is read before the same workgroup overwrites it)
            ops.call("local_scores_ragged", ctx, words, cap_lens, lA, self.lse, B, B, P, T, Do, members, n_c, ntt, cbase, Kp)
            # single pass over the (image, caption) pairs: sim AND the gradients for dL/dsim = 1 ...
            ops.call("local_pair2_ragged", lA, self.lse, self.gmp, self.wn, cap_lens, None, self.sim, ldS, lU,
                     B, B, P, T, temp1, temp2, 1e-8, members, n_c, ntt, cbase, Kp)
        self._st = (ctx, d_chunk, Kp, lA, ldS, lU, wT)
        return self.sim

    def backward(self, gsim: torch.Tensor, out: torch.Tensor) -> None:
        """gsim fp32 [B, B] = d loss / d sim; out bf16 [B, P, Do] receives d loss / d region features.  Returns None (no word gradient)."""
        B, P, Do, HWp = self.B, self.P, self.Do, self.HWp
        ctx, d_chunk, Kp, lA, ldS, lU, wT = self._st
        # ... then the head over the sim matrix supplies the per-pair factor
        ops.call("scale_blocks_ragged", ldS, lU, gsim, B, B, HWp, d_chunk, Kp)
        ops.gemm_nt(ldS, wT, self.dC32)                                                     # dC = dS . W
        if Kp >= 128 and self.imgp_tiles256.shape[0]:                                       # dGm_b = U_b A_b^T
            ops.gemm_nt(lU, lA, self.dGm, tiles=self.imgp_tiles256, tile_count=self.imgp_tile256_count, max_tiles=B,
                        stride_b=HWp * Kp, M=B * HWp, N=HWp, tile_rows=256)
        else:
            ops.gemm_nt(lU, lA, self.dGm, tiles=self.imgp_tiles, tile_count=self.imgp_tile_count,
                        max_tiles=self.imgp_tiles.shape[0], stride_b=HWp * Kp, M=B * HWp, N=HWp)
        ops.gemm_tn(self.dGm, ctx, self.dC32.view(B, HWp, Do), x_rowmap=self.ctx_xmap, row_off=self.imgp_row_off, n_groups=B,
                    stride_w=HWp * Do, nsplit=1, M=B * HWp, det=self.det)                    # dC_b += dGm_b . ctx_b
        ops.call("unpad_cast", self.dC32, out, B, P, HWp, Do)
