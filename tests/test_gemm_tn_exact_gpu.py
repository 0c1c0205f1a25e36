"""Exact per-element tests of every weight-gradient (TN) GEMM kernel and entry point: medmoe_gemm_tn, _staged, _det, _cols, _cols_det,
_gram and _gram_det on gemm_tn_kernel, gemm_tn512_kernel and gemm_tn4w_kernel in all their builds.

The data of tn_exact_cases.py makes the float64 reference THE result: dW and db are compared with torch.equal, every element.  Inputs sit
in buffers with NaN guard rows and NaN padding columns (ld > width), source rows no map entry names are NaN (physical row 0 among them),
the Gram weights have NaN between them (w_ld > 1) and past row M; outputs sit in buffers whose guards hold a fixed bit pattern that must
survive; a scratch is exactly as large as the form needs, pre-filled with NaN and followed by a patterned guard.  Every case asserts the
kernel that ran and the launch's split (medmoe_last_gemm_tn_kernel), by how much medmoe_nondet_launches moved, that a second launch
accumulates to base + 2 x product, and - deterministic and staged forms - that two runs agree bit for bit."""
import dataclasses

import pytest
import torch

import tn_exact_cases as T
from gemm_exact_cases import describe_mismatch
from test_gemm_nt_exact_gpu import DEV, PAT32, bits, blank, forced, guarded, ops  # noqa: F401  (ops: the fixture)

pytestmark = pytest.mark.gpu

SCRATCH_GUARD = 1024
W_GUARD_ROWS = 64


class ExactScratch:
    """`floats` floats of NaN followed by a patterned guard.  Stands in for ops.DetScratch: get() hands out the exact view and insists that
    the library asked for exactly this much."""

    def __init__(self, floats, expect=None):
        self.floats, self.expect = floats, floats if expect is None else expect
        self.buf = torch.empty(floats + SCRATCH_GUARD, device=DEV, dtype=torch.float32)
        self.buf[:floats] = float("nan")
        bits(self.buf[floats:]).fill_(PAT32)

    def view(self):
        return self.buf[:self.floats]

    def get(self, need):
        assert need == self.expect, f"the library asks for {need} scratch floats, the case expects {self.expect}"
        return self.view()

    def intact(self):
        return bool((bits(self.buf[self.floats:]) == PAT32).all())


_PROBLEMS = {}


def problem(case):
    """Device operands in guarded buffers and the float64 product, built once per geometry and never written again."""
    key = case.geom
    if key not in _PROBLEMS:
        if len(_PROBLEMS) >= 4:
            _PROBLEMS.pop(next(iter(_PROBLEMS)))
        o = T.to_device(T.make_operands(case), DEV)
        bf = torch.bfloat16
        p = dict(o=o, g=guarded(o.g, "nan", bf))
        if o.x is not None:
            p["x"] = guarded(o.x, "nan", bf)
        for name, m, src in (("g", o.gmap, o.g), ("x", o.xmap, o.x)):
            if m is not None:                            # rows of the source that no packed row names, row 0 among them: NaN
                unused = torch.ones(src.shape[0], dtype=torch.bool, device=DEV)
                unused[m.long()] = False
                assert bool(unused[0])
                p[name][:src.shape[0]][unused] = float("nan")
        if o.w is not None:                              # [groups, M + guard rows, w_ld]: NaN between the weights and past row M
            w = torch.full((o.w.shape[0], case.M + W_GUARD_ROWS, case.w_ld), float("nan"), device=DEV, dtype=torch.float32)
            w[:, :case.M, 0] = o.w
            p["w"] = w
        dw, db = T.reference(dataclasses.replace(case, db=True), o)
        p["prod_dw"] = dw - o.base_dw.double()
        p["prod_db"] = None if db is None else db - o.base_db.double()
        p["pristine"] = {k: p[k].clone() for k in ("g", "x", "w") if k in p}
        p["tables"] = {k: t.clone() for k, t in (("g_rowmap", o.gmap), ("x_rowmap", o.xmap), ("row_off", o.row_off)) if t is not None}
        _PROBLEMS[key] = p
    return _PROBLEMS[key]


def outputs(case, p):
    o = p["o"]
    dwbuf = guarded(o.base_dw, "pattern", torch.float32, cols=case.ldw_pad)      # [groups, Nn + guard rows, Kk + ldw_pad]
    dbbuf = guarded(o.base_db, "pattern", torch.float32, rows=0)                 # [groups, Nn + guard columns]
    return dwbuf, dbbuf


def launch(ops, case, p, dwbuf, dbbuf):
    """One launch of the case into the given output buffers.  Returns the scratch it used (or None)."""
    o = p["o"]
    M, Nn, Kk, G = case.M, case.Nn, case.Kk, case.n_groups
    ldw, stride_w = dwbuf.stride(1), dwbuf.stride(0)
    need = T.scratch_floats(case)
    if case.entry in ("tn", "staged", "det"):
        g, x = p["g"][:o.g.shape[0], :Nn], p["x"][:o.x.shape[0], :Kk]
        dw = dwbuf[:, :Nn, :Kk] if G > 1 else dwbuf[0, :Nn, :Kk]
        db = None if not case.db else (dbbuf[:, :Nn] if G > 1 else dbbuf[0, :Nn])
        kw = dict(db=db, x_rowmap=o.xmap, g_rowmap=o.gmap, row_off=o.row_off, n_groups=G, stride_w=stride_w, stride_db=dbbuf.stride(0), M=M)
        if case.entry == "tn":
            ops.gemm_tn(g, x, dw, nsplit=case.nsplit, **kw)
            return None
        sc = ExactScratch(need)
        if case.entry == "staged":
            ops.gemm_tn(g, x, dw, scratch=sc.view(), **kw)
        else:
            ops.gemm_tn(g, x, dw, det=sc, **kw)
        return sc
    if case.entry in ("cols", "cols_det"):
        gbuf, xbuf = p["g"], p["x"]
        sc = ExactScratch(need) if case.entry == "cols_det" else None
        ops.gemm_tn_cols(gbuf, gbuf.stride(-2), xbuf, xbuf.stride(-2), dwbuf, ldw, M, Nn, Kk, G, Nn if G > 1 else 0,
                         0 if (case.x_shared or G == 1) else Kk, stride_w, case.chunk_w, gbuf.stride(0) if case.chunk_w else 0, det=sc)
        return sc
    gbuf, w = p["g"], p["w"]
    ops.gemm_tn_gram(gbuf, gbuf.stride(-2), w, w.stride(0), case.w_ld, dwbuf, ldw, M, Nn, G, Nn, stride_w,
                     det=True if case.entry == "gram_det" else None)
    return None


def check_output(buf, before, exp64, what, written_rows):
    """buf [groups, rows + guards, cols + guards] (or [groups, cols + guards] with written_rows None): the top left corner of every group
    equals exp64, every element; everything else is bit-unchanged."""
    if written_rows is None:
        buf, before, exp64 = buf[:, None], before[:, None], exp64[:, None]
        written_rows = 1
    G, _, C = exp64.shape
    got = buf[:, :written_rows, :C]
    exp = exp64.float()
    assert torch.equal(exp.double(), exp64), what + ": the expectation is not exact in fp32"
    bad = ~(got == exp)                                  # NaN counts as wrong
    if bool(bad.any()):
        flat = bad.reshape(G * written_rows, C)
        pytest.fail(f"{what} (row = group * {written_rows} + n): " + describe_mismatch(flat, got.reshape(G * written_rows, C), exp.reshape(G * written_rows, C)))
    written = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    written[:, :written_rows, :C] = True
    moved = (bits(buf) != bits(before)) & ~written
    assert not bool(moved.any()), f"{what}: memory outside the result was written: " + describe_mismatch(moved.reshape(-1, buf.shape[-1]))


def check_all(case, p, dwbuf, dbbuf, before, launches, what):
    o = p["o"]
    check_output(dwbuf, before[0], o.base_dw.double() + launches * p["prod_dw"], what + " dW", case.Nn)
    if case.db and p["prod_db"] is not None:
        check_output(dbbuf, before[1], o.base_db.double() + launches * p["prod_db"], what + " db", None)
    else:
        assert torch.equal(bits(dbbuf), bits(before[1])), what + ": db was written without being asked for"
    for gi, n in enumerate(case.counts):                 # a group that owns no rows: not even a +0 lands in it
        if n == 0:
            assert torch.equal(bits(dwbuf[gi]), bits(before[0][gi])) and torch.equal(bits(dbbuf[gi]), bits(before[1][gi])), what + f": empty group {gi} was written"
    for k, t in p["pristine"].items():
        assert torch.equal(bits(p[k]), bits(t)), f"{what}: the launch wrote into its input `{k}`"
    tables = dict(g_rowmap=o.gmap, x_rowmap=o.xmap, row_off=o.row_off)
    for k, t in p["tables"].items():
        assert torch.equal(tables[k], t), f"{what}: the launch wrote into `{k}`"


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_gemm_tn_exact(ops, case):
    """One launch of the case's entry point: every element of dW and db against the float64 reference, guards and ownerless groups
    bit-unchanged, inputs unwritten, the scratch guard intact, the kernel id and split the case was written for, medmoe_nondet_launches
    moved by what the form implies; then a second launch on top (base + 2 x product); staged and deterministic forms once more from the
    base, bit for bit."""
    p = problem(case)
    dwbuf, dbbuf = outputs(case, p)
    before = (dwbuf.clone(), dbbuf.clone())
    with forced(ops, case.opts, T.OPTION_DEFAULTS):
        n0 = ops.nondet_launches()
        sc = launch(ops, case, p, dwbuf, dbbuf)
        ran, split, label = ops.last_gemm_tn_kernel()
        n1 = ops.nondet_launches()
        torch.cuda.synchronize()
        assert ran == case.kernel, f"{case.id}: ran on kernel {ran} ({label}), written for {case.kernel}"
        assert split == case.split, f"{case.id}: split {split}, written for {case.split}"
        assert n1 - n0 == case.nondet, f"{case.id}: medmoe_nondet_launches moved by {n1 - n0}, the form implies {case.nondet}"
        check_all(case, p, dwbuf, dbbuf, before, 1, case.id)
        assert sc is None or sc.intact(), f"{case.id}: the launch wrote past its scratch"
        first = (dwbuf.clone(), dbbuf.clone())
        sc = launch(ops, case, p, dwbuf, dbbuf)
        n2 = ops.nondet_launches()
        torch.cuda.synchronize()
        assert ops.last_gemm_tn_kernel()[:2] == (ran, split) and n2 - n1 == case.nondet
        check_all(case, p, dwbuf, dbbuf, before, 2, case.id + " second launch")
        assert sc is None or sc.intact(), f"{case.id}: the second launch wrote past its scratch"
        if case.nondet == 0:                             # deterministic, staged and single-writer forms: a rerun from the base, bit for bit
            dw2, db2 = outputs(case, p)
            sc = launch(ops, case, p, dw2, db2)
            torch.cuda.synchronize()
            assert torch.equal(bits(dw2), bits(first[0])) and torch.equal(bits(db2), bits(first[1])), f"{case.id}: two runs differ"
            assert sc is None or sc.intact()


def _ones(*shape):
    return torch.ones(*shape, device=DEV, dtype=torch.bfloat16)


@pytest.mark.parametrize("what", T.REFUSALS)
def test_gemm_tn_refuses(ops, what):
    """Argument checks: the wrapper raises, nothing is launched - dW bit-identical, the last-kernel state and the count of order-dependent
    launches where they were."""
    ops.gemm_tn(_ones(8, 8), _ones(8, 8), torch.zeros(8, 8, device=DEV), nsplit=1)
    state = ops.last_gemm_tn_kernel()
    assert state[:2] == (T.K128, 1)
    n0 = ops.nondet_launches()
    dwbuf = blank(256, 256, torch.float32)
    ldw = dwbuf.stride(0)
    w = torch.ones(64, device=DEV)
    if what == "Nn%8":
        fn = lambda: ops.gemm_tn(_ones(64, 16)[:, :12], _ones(64, 16), dwbuf[:12, :16], nsplit=1)
    elif what == "ld%8":
        fn = lambda: ops.gemm_tn(_ones(64, 20)[:, :16], _ones(64, 16), dwbuf[:16, :16], nsplit=1)
    elif what == "cols M%32":
        fn = lambda: ops.gemm_tn_cols(_ones(48, 16), 16, _ones(48, 16), 16, dwbuf, ldw, 48, 16, 16, 1, 0, 0, 0, 0, 0)
    elif what == "cols Nn>ldg":
        fn = lambda: ops.gemm_tn_cols(_ones(32, 8), 8, _ones(32, 16), 16, dwbuf, ldw, 32, 16, 16, 1, 0, 0, 0, 0, 0)
    elif what == "gram w_ld<1":
        fn = lambda: ops.gemm_tn_gram(_ones(32, 16), 16, w, 0, 0, dwbuf, ldw, 32, 16, 1, 0, 0)
    else:
        assert what == "det scratch short"
        need = 2 * (T.SLOT_FLOATS + T.SLOT_DB_FLOATS)    # TN_PLAIN, two ranges of one tile
        sc = ExactScratch(need - 1, expect=need)
        fn = lambda: ops.gemm_tn(_ones(4096, 256), _ones(4096, 256), dwbuf[:256, :256], det=sc)
    before = dwbuf.clone()
    with pytest.raises(RuntimeError):
        fn()
    torch.cuda.synchronize()
    assert torch.equal(bits(dwbuf), bits(before))
    assert ops.last_gemm_tn_kernel() == state and ops.nondet_launches() == n0
