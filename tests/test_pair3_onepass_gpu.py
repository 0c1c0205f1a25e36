"""The backward launch of the transposed pair stage (medmoe_amd/csrc/pair3.hip, BWD = true) on its own: dS, d2, dwn and U against float64 torch
evaluated on the kernel's OWN inputs (the fp16 log2-probabilities, the bf16 A of the forward launch, lse, the bf16 Gram matrices, stats, sim,
gsim, the word norms) with the formulas of the kernel's comments - nothing else of the model enters, so the bounds are those of the number
formats:
  dS   per (image, caption) unit, relative norm error <= 2^-8: one bf16 rounding of every element is 2^-9 norm-wise, the factor two covers
       the fp32 evaluation and the cancellation in da1 - rd;
  d2, dwn   relative norm error <= 1e-4 (fp32 arithmetic with the fast exp).
Every length class runs 3 * CPI + 1 captions (CPI = 16 // NTT captions per workgroup iteration): with one chunk per image a workgroup
then runs four epochs - both mailbox parities are used twice - and its last iteration has inactive caption groups.  The results must not
depend on how the captions are spread over workgroups (one chunk / automatic) nor on the run.

Recorded: this file passes against the library built from the commit before the one-pass backward (same bounds, same inputs)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
BF, I32, F64 = torch.bfloat16, torch.int32, torch.float64
TEMP1, TEMP2, EPS = 4.0, 5.0, 1e-8
LN2 = 0.6931471805599453
DS_BOUND, ROW_BOUND = 2.0 ** -8, 1e-4


def class_lengths(ntt, n, T):
    """n caption lengths of class ntt (16 (ntt-1) < len <= min(16 ntt, T)), its two ends included."""
    lo, hi = 16 * (ntt - 1) + 1, min(16 * ntt, T)
    return [lo, hi] + [lo + (5 * k + 3) % (hi - lo + 1) for k in range(n - 2)]


def caps_all_classes(T=77):
    per = [class_lengths(ntt, 3 * (16 // ntt) + 1, T) for ntt in range(1, 6)]       # 49, 25, 16, 13, 10 captions
    out, k = [], 0
    while any(per):                                                               # interleave the classes: the layout sorts them again
        if per[k % 5]:
            out.append(per[k % 5].pop(0))
        k += 1
    return out


class Inputs:
    """Scores + forward launch of B images against a separate caption list, with the project's own kernels; everything the backward launch
    reads is kept (lp as a pristine copy: the launch writes dS over it)."""

    def __init__(self, caps, B, HW, T, D, scale, seed):
        from medmoe_amd import ops
        from medmoe_amd.engine import ragged_layout
        dev = "cuda"
        self.caps, self.B, self.Bc, self.HW, self.T = list(caps), B, len(caps), HW, T
        Bc = self.Bc
        g = torch.Generator().manual_seed(seed)
        ctx = (torch.randn(B, HW, D, generator=g) * scale).to(BF)
        words = (torch.randn(Bc, T, D, generator=g) * scale).to(BF)
        self.gs = (torch.randn(B, Bc, generator=g) * 0.1).to(dev).contiguous()
        HWp, Tp, _ = ops.local_geometry(HW, T)
        self.HWp = HWp
        GR = (HW + 31) // 32 * 32
        self.GR = self.PW = GR                                  # image-major, 64-byte aligned rows: what the engine runs
        perm, col, ntts, _, classes, Kc, Kp = ragged_layout(np.array(caps), T, Tp)
        self.perm, self.classes, self.Kc, self.Kp = perm, classes, Kc, Kp
        d = lambda a: torch.from_numpy(np.asarray(a).astype(np.int32)).to(dev)
        self.d_perm = d(perm)
        c16 = ctx.to(dev).reshape(B * HW, D).contiguous(); w16 = words.to(dev).contiguous()
        self.wn = torch.empty(Bc, T, device=dev)
        ops.call("words_prep_ragged", w16, self.wn, None, Bc, T, Tp, D, d(col), d(16 * ntts), Kp)
        c = c16.view(B, HW, D).float()
        self.gm = torch.zeros(B, GR, GR, device=dev, dtype=BF)
        self.gm[:, :HW, :HW] = torch.bmm(c, c.transpose(1, 2)).to(BF)
        self.capd = torch.tensor(caps, dtype=I32, device=dev)
        self.ld, self.bs = self.PW, Kp * self.PW
        self.lse = torch.full((B, Bc, HWp), float("nan"), device=dev)
        lp = torch.full((Kp * B * self.PW,), float("nan"), device=dev, dtype=BF)     # regions >= HW stay poisoned: never written by the score kernel
        for ntt, start, n_c, cbase in classes:
            ops.call("local_scores_t", c16, w16, self.capd, lp, self.lse, B, Bc, HW, T, D, self.d_perm[start:start + n_c], n_c, ntt, cbase, self.ld, self.bs)
        self.sim = torch.full((B, Bc), float("nan"), device=dev)
        self.A = torch.full_like(lp, float("nan"))
        self.stats = torch.full((B, Kp, 2), float("nan"), device=dev)
        for ntt, start, n_c, cbase in classes:
            ops.call("local_pair3", lp, None, self.A, None, self.lse, self.gm, self.wn, self.capd, None, self.sim, None, self.stats, Kp, B, Bc, HW, T,
                     TEMP1, TEMP2, EPS, self.d_perm[start:start + n_c], n_c, ntt, cbase, self.ld, self.bs, self.PW, None)
        torch.cuda.synchronize()
        self.img(lp)[:, Kc:] = 0; self.img(self.A)[:, Kc:] = 0          # the zero padding rows up to Kp belong to no caption
        self.lp = lp

    def img(self, m):
        return m.view(self.B, self.Kp, self.PW)                  # [image][row][region]

    def backward(self, mode):
        """One backward launch per class, dS over a copy of lp (in place, as the engine runs it).  mode: 'd2' (row weights only), 'U' (U and
        d2), 'wn' (the wgrad entry point: d2 and dwn)."""
        from medmoe_amd import ops
        x = self.lp.clone()
        nan = lambda *s: torch.full(s, float("nan"), device=x.device)
        d2, dwn = nan(self.B, self.Kp), (nan(self.B, self.Kp) if mode == "wn" else None)
        U = torch.full_like(x, float("nan")) if mode == "U" else None
        for ntt, start, n_c, cbase in self.classes:
            args = (x, x, self.A, U, self.lse, self.gm, self.wn, self.capd, self.gs, self.sim, None, self.stats, self.Kp, self.B, self.Bc, self.HW, self.T,
                    TEMP1, TEMP2, EPS, self.d_perm[start:start + n_c], n_c, ntt, cbase, self.ld, self.bs, self.PW, d2)
            if mode == "wn":
                ops.call("local_pair3_wgrad", *args, dwn)
            else:
                ops.call("local_pair3", *args)
        torch.cuda.synchronize()
        return dict(dS=x, d2=d2, dwn=dwn, U=U)

    def reference(self):
        """float64 dS [B][Kc rows][HW], d2 and dwn [B][Kc rows] from the launch's inputs: the formulas in the comments of local_pair3_kernel."""
        B, HW, T, Kc = self.B, self.HW, self.T, self.Kc
        dS = torch.zeros(B, Kc, HW, dtype=F64, device="cuda"); d2o = torch.zeros(B, Kc, dtype=F64, device="cuda"); dwo = torch.zeros_like(d2o)
        Gm = self.gm[:, :HW, :HW].to(F64)
        for ntt, start, n_c, cbase in self.classes:
            TP = 16 * ntt
            rows = slice(cbase, cbase + n_c * TP)
            mem = torch.from_numpy(self.perm[start:start + n_c]).cuda()
            blk = lambda m: self.img(m)[:, rows, :HW].reshape(B, n_c, TP, HW)
            lp = blk(self.lp.view(torch.float16)).to(F64)         # log2-probabilities; -60000 on padding words: exp2 = 0
            a = blk(self.A).to(F64)
            a1 = torch.exp2(lp)
            S = lp * LN2 + self.lse[:, mem, None, :HW].to(F64)
            y = torch.einsum("bhk,bjtk->bjth", Gm, a)
            st = self.stats[:, rows].reshape(B, n_c, TP, 2).to(F64)
            num, n2 = st[..., 0], st[..., 1]
            t = torch.arange(TP, device="cuda")
            cap = self.capd[mem].clamp(1, min(T, TP))
            live = (t[None, :] < cap[:, None])[None]              # [1][n_c][TP]
            nw = self.wn[mem][:, t.clamp(max=T - 1)].to(F64)[None]
            n2c = n2.clamp_min(0.0)
            den = nw * n2c.sqrt()
            cosv = num / den.clamp_min(EPS)
            ev = torch.where(live, torch.exp(TEMP2 * cosv), torch.zeros_like(cosv))
            se = torch.exp(self.sim[:, mem].to(F64))[:, :, None]
            dcos = self.gs[:, mem].to(F64)[:, :, None] * TEMP2 * ev / se
            ok = den >= EPS
            dn = torch.where(ok, dcos / den, dcos / EPS)
            d2 = torch.where(ok, -dcos * cosv / n2c.clamp_min(1e-30), torch.zeros_like(dcos))
            dwn = torch.where(ok, -dcos * cosv / (nw * nw), torch.zeros_like(dcos))
            ca = dn * num + d2 * n2
            k1, k2, k3 = TEMP1 * dn, TEMP1 * d2, TEMP1 * ca
            da1 = a * (k1[..., None] * S + k2[..., None] * y - k3[..., None])
            rd = (a1 * da1).sum(dim=2, keepdim=True)              # over the caption's words
            ds = dn[..., None] * a + a1 * (da1 - rd)
            dS[:, rows] = ds.reshape(B, n_c * TP, HW)
            d2o[:, rows] = d2.reshape(B, -1); dwo[:, rows] = dwn.reshape(B, -1)
        return dict(dS=dS, d2=d2o, dwn=dwo)


def rel64(got, ref):
    return float((got.to(F64) - ref).norm() / ref.norm().clamp_min(1e-300))


class Case:
    """Inputs, the float64 reference and the backward launches of one geometry, each made once: the 'd2' and 'wn' forms twice with one caption
    chunk per image (every workgroup walks its whole list) and twice with the automatic spread, the 'U' form once with one chunk."""

    def __init__(self, caps, B, HW, T, D, scale, seed):
        from medmoe_amd import ops
        self.inp = Inputs(caps, B, HW, T, D, scale, seed)
        self.ref = self.inp.reference()
        self.runs = {}
        try:
            for chunks in (1, 0):
                ops.local_pair3_chunks(chunks)
                for rep in range(2):
                    self.runs[("d2", chunks, rep)] = self.inp.backward("d2")
                    self.runs[("wn", chunks, rep)] = self.inp.backward("wn")
            ops.local_pair3_chunks(1)
            self.runs[("U", 1, 0)] = self.inp.backward("U")
        finally:
            ops.local_pair3_chunks(0)


@pytest.fixture(scope="module")
def full():
    return Case(caps_all_classes(77), B=2, HW=196, T=77, D=128, scale=0.5, seed=11)


@pytest.fixture(scope="module")
def small():
    return Case([16, 3, 9, 1, 12, 16, 7, 5] * 5, B=2, HW=64, T=16, D=128, scale=0.5, seed=12)       # 40 captions: 16 + 16 + 8 per workgroup at one chunk


def bits(x):
    return x.view(torch.int16 if x.dtype == BF else torch.int32)


def check_parity(case):
    inp, ref = case.inp, case.ref
    B, HW, Kc = inp.B, inp.HW, inp.Kc
    for mode in ("d2", "wn"):
        r = case.runs[(mode, 1, 0)]
        dS = inp.img(r["dS"])
        assert bool(torch.isfinite(dS.float()).all())
        worst = (0.0, None)
        for ntt, start, n_c, cbase in inp.classes:
            TP = 16 * ntt
            rows = slice(cbase, cbase + n_c * TP)
            got = dS[:, rows].to(F64).reshape(B, n_c, TP, inp.PW)
            want = ref["dS"][:, rows].reshape(B, n_c, TP, HW)
            cap = inp.capd[torch.from_numpy(inp.perm[start:start + n_c]).cuda()].clamp(1, min(inp.T, TP))
            pad = torch.arange(TP, device="cuda")[None, :] >= cap[:, None]                         # [n_c][TP]: words beyond the caption
            assert float((got.abs().amax(dim=(0, 3)) * pad).max()) == 0.0, ntt
            err = (got[..., :HW] - want).flatten(2).norm(dim=2) / want.flatten(2).norm(dim=2).clamp_min(1e-300)      # per (image, caption) unit
            assert bool((want.flatten(2).norm(dim=2) > 0).all())
            k = int(err.argmax())
            worst = max(worst, (float(err.flatten()[k]), (mode, ntt, k // n_c, int(inp.perm[start + k % n_c]))))
        print(f"dS worst unit {worst[0]:.3e} = 2^-8 x {worst[0] / DS_BOUND:.3f} at (form, class, image, caption) {worst[1]}")
        assert worst[0] <= DS_BOUND, worst
        if inp.PW > HW:
            assert float(dS[:, :, HW:].float().abs().max()) == 0.0          # padding regions are written as zeros
        e2 = rel64(r["d2"][:, :Kc], ref["d2"][:, :Kc])
        print(f"d2 {e2:.3e}")
        assert e2 <= ROW_BOUND, e2
    ew = rel64(case.runs[("wn", 1, 0)]["dwn"][:, :Kc], ref["dwn"][:, :Kc])
    print(f"dwn {ew:.3e}")
    assert ew <= ROW_BOUND, ew


def check_scheduling(case):
    Kc = case.inp.Kc
    for mode, keys in (("d2", ("dS", "d2")), ("wn", ("dS", "d2", "dwn"))):
        base = case.runs[(mode, 1, 0)]
        for chunks in (1, 0):
            for rep in range(2):
                r = case.runs[(mode, chunks, rep)]
                for k in keys:
                    x, y = (r[k], base[k]) if k == "dS" else (r[k][:, :Kc], base[k][:, :Kc])
                    assert torch.equal(bits(x), bits(y)), (mode, chunks, rep, k)
    assert torch.equal(bits(case.runs[("wn", 1, 0)]["dS"]), bits(case.runs[("d2", 1, 0)]["dS"]))       # the WN build writes the same dS


def test_backward_outputs_all_classes_against_float64(full):
    assert [c[0] for c in full.inp.classes] == [1, 2, 3, 4, 5] and [c[2] for c in full.inp.classes] == [49, 25, 16, 13, 10]
    check_parity(full)


def test_backward_independent_of_scheduling(full):
    check_scheduling(full)


def test_64_regions_against_float64(small):
    check_parity(small)


def test_64_regions_independent_of_scheduling(small):
    check_scheduling(small)


def test_u_form_is_bf16_of_a_times_d2(full):
    inp, r = full.inp, full.runs[("U", 1, 0)]
    ntt2 = [c for c in inp.classes if c[0] >= 2]
    rows = slice(ntt2[0][3], inp.Kc)                             # classes 2..5 are stored behind class 1
    want = (inp.img(inp.A)[:, rows].float() * r["d2"][:, rows, None]).to(BF)
    assert torch.equal(bits(inp.img(r["U"])[:, rows]), bits(want))
    assert torch.equal(bits(r["dS"]), bits(full.runs[("d2", 1, 0)]["dS"]))
