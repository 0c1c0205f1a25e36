"""The references of test_gemm_tn_exact_gpu.py checked on the CPU: a case whose own reference is inexact must never reach the GPU test.

For every problem of the table: the operands are exact in bf16 and within their ranges, rows and columns are pairwise distinct, the float32
contraction equals the float64 one, every reference value times its unit (1, or 64 for the weighted Gram form) is an integer below 2^24 -
also after the second launch the GPU test makes - and, for the Gram form, w * A is exact in fp32 while its one bf16 rounding changes at
least one product and meets at least one tie.  The table reaches every kernel id, entry point and TnKind, and where the library is built
its scratch queries (host functions) agree with the kind and the slots each deterministic case expects."""
import ctypes
import functools
import os

import pytest
import torch

import tn_exact_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problems():
    seen = {}
    for c in T.CASES:
        seen.setdefault(c.geom, c)
    return list(seen.values())


PROBLEMS = _problems()


@functools.lru_cache(maxsize=None)
def _operands(geom):
    return T.make_operands(next(c for c in PROBLEMS if c.geom == geom))


def test_table_reaches_everything_and_stays_small():
    assert {c.kernel for c in T.CASES} == set(T.KERNEL_IDS)
    assert {c.entry for c in T.CASES} == set(T.ENTRIES)
    assert {c.det_kind for c in T.CASES if c.entry == "det"} == {T.TN_SMALL, T.TN_PLAIN, T.TN_ROWMAP, T.TN_GROUPS}
    assert all((c.det_kind is not None) == (c.entry == "det") for c in T.CASES)
    assert len({c.id for c in T.CASES}) == len(T.CASES)
    for c in T.CASES:
        assert set(dict(c.opts)) <= set(T.OPTION_DEFAULTS) <= {3, 4, 8, 9, 10}, c.id
        o = _operands(c.geom)
        for t in (o.g, o.x):
            if t is not None:
                assert t.shape[-2] <= T.MAX_ROWS, c.id          # gathered sources included; a matrix of column groups is wider than one group's Nn / Kk
        assert c.M <= T.MAX_ROWS and c.Nn <= T.MAX_COLS and c.Kk <= T.MAX_COLS, c.id
        assert not c.counts or sum(c.counts) == c.M, c.id
        assert c.split is not None and c.nondet in (0, 1), c.id
        if c.entry in ("det", "cols_det", "gram_det") or (c.entry == "staged" and c.scratch == "room") or (c.staged_launch and not c.db):
            assert c.nondet == 0, c.id                          # no deterministic or fully staged launch may count as order-dependent
        if c.entry in ("gram", "gram_det"):
            assert c.M <= 4224 and c.M % 32 == 0, c.id
    # the mechanisms the table exists for: ring refills on both 256 x 256 generations, sub-step counts 1..5 on both
    for k in (T.K4WM, T.K512M):
        assert any(c.kernel == k and max(c.counts or (c.M,)) > 12288 and (c.split == 1 or c.split > 12288) and (c.xmap or c.gmap) for c in T.CASES)
    assert {c.M // 32 for c in T.CASES if c.entry == "cols" and c.split == 1} >= {1, 2, 3, 4, 5}


def _distinct(t):
    return torch.unique(t, dim=0).shape[0] == t.shape[0]


@pytest.mark.parametrize("case", PROBLEMS, ids=lambda c: "-".join(str(v) for v in c.geom).replace(" ", ""))
def test_reference_is_exact(case):
    o = _operands(case.geom)
    gram = case.geom[0] == "gram"
    # operands: exact in bf16, in the stated ranges
    for t, lim in ((o.g, 3), (o.x, 2), (o.base_dw, 64), (o.base_db, 64)):
        if t is not None:
            assert torch.equal(t.to(torch.bfloat16).float(), t) and torch.equal(t, t.round()) and float(t.abs().max()) <= lim
    if o.g.numel() >= 512:
        assert float(o.g.min()) == -3 and float(o.g.max()) == 3
    g_used, x_used = T.used_sources(case, o)
    if case.M > 1:                                          # a shifted or transposed read shows
        for t in (g_used, x_used):
            assert _distinct(t) and _distinct(t.t().contiguous()), "two equal rows or columns"
    for m, src in ((o.gmap, o.g), (o.xmap, o.x)):
        if m is not None:
            assert m.unique().numel() == case.M and int(m.min()) >= 1 and int(m.max()) < src.shape[0]      # row 0 is named by no entry
    if o.row_off is not None:
        assert o.row_off.tolist() == [sum(case.counts[:i]) for i in range(len(case.counts) + 1)]
    # the fp32 accumulation is exact: the float32 CPU contraction equals the float64 one
    dw64, db64 = T.reference(case, o, torch.float64)
    dw32, db32 = T.reference(case, o, torch.float32)
    assert torch.equal(dw32.double(), dw64)
    assert (db64 is None) == (not case.db or case.geom[0] != "rows")
    if db64 is not None:
        assert torch.equal(db32.double(), db64)
    unit = T.GRAM_UNIT if gram else 1.0
    base = o.base_dw.double()
    for launches in (1, 2):                                 # the GPU test launches twice: base + 2 x product must be exact as well
        v = (base + launches * (dw64 - base)) * unit
        assert torch.equal(v, v.round()) and float(v.abs().max()) < 2 ** 24
        assert torch.equal((v / unit).float().double(), v / unit)
    # a bound on every partial sum, in any order: the sum of the magnitudes
    g_abs, x_abs = g_used.abs().double(), x_used.abs().double()
    if gram:
        g_abs = g_abs * 2.0
    assert float(g_abs.sum(0).max()) * float(x_abs.max()) * unit * 2 + 64 * unit < 2 ** 24
    if gram:
        w = o.w
        assert torch.equal(w * 64, (w * 64).round()) and float(w.abs().max()) <= 2
        assert bool((w == 0).any()) and bool((w > 0).any()) and bool((w < 0).any())
        a = o.g[:, :case.Nn]
        exact = a.double() * w[0].double()[:, None]
        assert torch.equal((a * w[0][:, None]).double(), exact)              # w * A is exact in fp32
        rounded = T.scaled_rows(a, w[0]).double()
        changed = rounded != exact
        assert bool(changed.any())
        # a tie: the product lies exactly between two neighbouring bf16 values (half an ulp of its binade from the rounded one)
        half_ulp = torch.exp2(torch.floor(torch.log2(exact.abs().clamp_min(2.0 ** -20))) - 8)
        tie = changed & ((rounded - exact).abs() == half_ulp)
        assert bool(tie.any())
        assert torch.equal(rounded * 64, (rounded * 64).round())


def _lib():
    path = os.path.join(ROOT, "medmoe_amd", "lib", "libmedmoe_hip.so")
    if not os.path.exists(path):
        pytest.skip("library not built")
    lib = ctypes.CDLL(path)
    lib.medmoe_gemm_tn_det_scratch.restype = ctypes.c_longlong
    lib.medmoe_gemm_tn_det_scratch.argtypes = [ctypes.c_int] * 7
    lib.medmoe_gemm_tn_cols_det_scratch.restype = ctypes.c_longlong
    lib.medmoe_gemm_tn_cols_det_scratch.argtypes = [ctypes.c_int] * 4
    return lib


def test_scratch_queries_agree_with_the_expected_kinds():
    """Host queries of the built library: every det case's scratch is slots x (65536 + 512) floats (0 for TN_SMALL), every cols_det case's
    slots x 65536 (0 with one range).  The last-kernel query reports -1 or a known id."""
    lib = _lib()
    checked = 0
    for c in T.CASES:
        if c.entry not in ("det", "cols_det"):
            continue
        try:
            for k, v in c.opts:
                assert lib.medmoe_set_option(k, v) == 0
            if c.entry == "det":
                got = lib.medmoe_gemm_tn_det_scratch(c.M, c.Nn, c.Kk, int(c.xmap), int(c.gmap), int(bool(c.counts)), c.n_groups)
                assert (c.det_kind == T.TN_SMALL) == (c.slots == 0) == (got == 0), c.id
                assert {T.TN_SMALL: c.kernel in (T.K128, T.K128M), T.TN_PLAIN: c.kernel == T.K4W_ST}.get(c.det_kind, c.kernel == T.K4WM_ST), c.id
            else:
                got = lib.medmoe_gemm_tn_cols_det_scratch(c.M, c.Nn, c.Kk, c.n_groups)
            assert got == T.scratch_floats(c), (c.id, got, T.scratch_floats(c))
            checked += 1
        finally:
            for k, v in T.OPTION_DEFAULTS.items():
                lib.medmoe_set_option(k, v)
    assert checked >= 20
    split = ctypes.c_int(-7)
    lib.medmoe_last_gemm_tn_kernel.restype = ctypes.c_int
    lib.medmoe_last_gemm_tn_kernel.argtypes = [ctypes.POINTER(ctypes.c_int)]
    assert lib.medmoe_last_gemm_tn_kernel(ctypes.byref(split)) in (-1,) + T.KERNEL_IDS and split.value >= 0
    assert lib.medmoe_last_gemm_tn_kernel(None) in (-1,) + T.KERNEL_IDS
