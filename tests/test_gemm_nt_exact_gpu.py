"""Exact per-element tests of every NT GEMM kernel (medmoe_gemm_nt, _rows, _tiles256), edge and epilogue.

The data of gemm_exact_cases.py makes the float64 reference THE result: fp32 C is compared with torch.equal, bf16 C bit for bit
(as int16) against one round-to-nearest-even of the reference, every element of every output.  The GELU epilogues are compared per
element against float64 erf within the bf16 half-ulp plus a floor for the fp32 polynomial (the figures are in gemm_exact_cases.py and
measured by test_gemm_nt_exact_host.py).  Every operand sits in a buffer with guard rows and columns: outputs' guards hold a fixed bit
pattern that must survive the launch, inputs' padding holds NaN that must reach no result.  Every case asserts the kernel that ran."""
import contextlib

import pytest
import torch

import gemm_exact_cases as X

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD_ROWS, GUARD_COLS = 16, 8
PAT16, PAT32 = 0x5A5A, 0x5A5A5A5A          # finite in bf16 and fp32: a guard added into a result would show as a value, too


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from medmoe_amd import ops as o
    return o


@contextlib.contextmanager
def forced(ops, opts, defaults=X.OPTION_DEFAULTS):
    """Kernel-selection options for one launch; the defaults (of the family under test) come back whatever happens."""
    try:
        for k, v in opts:
            ops.set_option(k, v)
        yield
    finally:
        for k, v in defaults.items():
            ops.set_option(k, v)


def last_kernel(ops):
    return ops.load_library().medmoe_last_gemm_nt_kernel()


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def guarded(data, fill, dtype, rows=GUARD_ROWS, cols=GUARD_COLS):
    """data [..., R, C] (or [..., C] with rows = 0) in the top left corner of a buffer with guard rows and columns.
    fill: "nan" (inputs) or "pattern" (outputs)."""
    shp = list(data.shape)
    shp[-1] += cols
    if rows:
        shp[-2] += rows
    buf = torch.empty(shp, device=DEV, dtype=dtype)
    if fill == "nan":
        buf.fill_(float("nan"))
    else:
        bits(buf).fill_(PAT16 if buf.element_size() == 2 else PAT32)
    if rows:
        buf[..., :data.shape[-2], :data.shape[-1]] = data.to(dtype)
    else:
        buf[..., :data.shape[-1]] = data.to(dtype)
    return buf


def blank(rows, cols, dtype, guard_cols=GUARD_COLS):
    """An output buffer of rows x cols plus guards, the pattern everywhere."""
    buf = torch.empty(rows + GUARD_ROWS, cols + guard_cols, device=DEV, dtype=dtype)
    bits(buf).fill_(PAT16 if buf.element_size() == 2 else PAT32)
    return buf


_PROBLEMS = {}


def problem(shape, gelu):
    """Device operands in guarded buffers and the float64 product, built once per (shape, data kind) and never written again."""
    key = (shape, gelu)
    if key not in _PROBLEMS:
        if len(_PROBLEMS) >= 8:                      # the table is ordered by shape: keep the device memory of a few
            _PROBLEMS.pop(next(iter(_PROBLEMS)))
        o = X.to_device(X.make_operands(shape, gelu), DEV)
        bf = torch.bfloat16
        g = dict(o=o, acc=X.accumulate(o, torch.float64),
                 a=guarded(o.a, "nan", bf), b=guarded(o.b, "nan", bf), bias=guarded(o.bias, "nan", torch.float32, rows=0),
                 residual=guarded(o.residual, "nan", bf), aux_in=guarded(o.aux_in, "nan", bf))
        if o.amap is not None:                       # rows of the source that no packed row names: NaN
            unused = torch.ones(o.a.shape[0], dtype=torch.bool, device=DEV)
            unused[o.amap.long()] = False
            g["a"][:o.a.shape[0]][unused] = float("nan")
            g["count"] = torch.tensor([len(o.tiles)], device=DEV, dtype=torch.int32)
        g["pristine"] = {k: g[k].clone() for k in ("a", "b", "bias", "residual", "aux_in")}
        _PROBLEMS[key] = g
    return _PROBLEMS[key]


def launch(ops, g, e, *, rows=None, m_dev=None, a=None):
    """One launch of epilogue `e` on the problem `g`.  rows: gemm_nt with M = rows; m_dev: gemm_nt_rows.  Returns the output buffer, the
    aux output buffer (or None), their images from before the launch, and the residual the launch read."""
    o = g["o"]
    s = o.shape
    D = s.dst_rows or s.M
    N, K = s.N, s.K
    cdt = torch.float32 if e.f32 else torch.bfloat16
    a_buf = g["a"] if a is None else a
    kw = dict(alpha=e.alpha, epi=e.epi)
    res_data = None
    if e.inplace:
        cbuf = guarded(o.residual, "pattern", cdt)
    else:
        cbuf = blank(D, N, cdt)                       # the destination holds the pattern, too: a store that never came shows
    out = cbuf[:D, :N]
    if e.bias:
        kw["bias"] = g["bias"][0, :N] if not s.grouped else g["bias"][:, :N]
    if e.residual:
        kw["residual"] = out if e.inplace else g["residual"][:D, :N]
    auxbuf = None
    if e.aux == "out":
        auxbuf = blank(D, N, torch.bfloat16)
        kw["aux"] = auxbuf[:D, :N]
    elif e.aux == "in":
        kw["aux"] = g["aux_in"][:D, :N]
    before = (cbuf.clone(), None if auxbuf is None else auxbuf.clone())
    if e.inplace:
        res_data = before[0][:D, :N].float()          # the expectation comes from the copy, not from what the launch left
    if m_dev is not None:
        ops.gemm_nt_rows(a_buf[:s.M, :K], g["b"][0, :N, :K], out, m_dev, **kw)
    elif s.grouped:
        ops.gemm_nt(a_buf[:o.a.shape[0], :K], g["b"][:, :N, :K], out, a_rowmap=o.amap, c_rowmap=o.cmap, tiles=o.tiles, tile_count=g["count"],
                    max_tiles=len(o.tiles) + 2, stride_b=g["b"].stride(0), stride_bias=g["bias"].stride(0), M=s.M, tile_rows=s.tile_rows, **kw)
    elif rows is not None:
        ops.gemm_nt(a_buf[:rows, :K], g["b"][0, :N, :K], out[:rows], M=rows, **kw)
    else:
        ops.gemm_nt(a_buf[:s.M, :K], g["b"][0, :N, :K], out, **kw)
    return cbuf, auxbuf, before, res_data


def check_untouched(buf, before, rows_written, N, what):
    """Every element of the buffer outside (rows_written, :N) is bit-unchanged."""
    written = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    written[rows_written, :N] = True
    bad = (bits(buf) != bits(before)) & ~written
    assert not bool(bad.any()), f"{what}: memory outside the result was written: " + X.describe_mismatch(bad)


def check_inputs(g, used=("a", "b", "bias", "residual", "aux_in")):
    for k in used:
        assert torch.equal(bits(g[k]), bits(g["pristine"][k])), f"the launch wrote into its input `{k}`"


def check_exact(got, ref64, f32, what):
    """Every element: fp32 equal to the reference, bf16 bit-equal to its one rounding."""
    if f32:
        bad = got != ref64.float()
        exp = ref64
    else:
        exp = X.to_bf16_once(ref64)
        bad = bits(got.contiguous()) != bits(exp.contiguous())
    assert not bool(bad.any()), f"{what}: " + X.describe_mismatch(bad, got, exp)


BARS = {}


def check_gelu(got, ref64, scale, what, tag):
    """Every element: |got - ref| <= 2^-8 |ref| + GELU_FLOOR * s.  The worst excess over the half-ulp is kept for the [bar] line."""
    assert bool(torch.isfinite(got.float()).all()), f"{what}: non-finite output"
    ex = X.gelu_excess(got, ref64, scale)
    worst = float(ex.max())
    BARS[tag] = max(BARS.get(tag, -1.0), worst)
    print(f"[bar] {what}: worst excess over 2^-8 |ref| {worst:.3g} (floor {X.GELU_FLOOR:g}, {tag})")
    bad = ex > X.GELU_FLOOR
    assert not bool(bad.any()), f"{what}: " + X.describe_mismatch(bad, got, ref64)


def verify(g, e, cbuf, auxbuf, before, res_data, rows, what):
    """The first `rows` packed rows hold the result; everything else in both output buffers is as it was."""
    o = g["o"]
    N = o.shape.N
    dr = X.dest_rows(o, rows)
    ref, aux_ref, z, scale, _ = X.reference(o, e, g["acc"][:rows], residual=res_data)
    check_untouched(cbuf, before[0], dr, N, what + " C")
    got = cbuf[dr, :N]
    if not e.gelu:
        check_exact(got, ref, e.f32, what + " C")
    else:
        check_gelu(got, ref, scale if e.epi == X.EPI_MUL_DGELU else None, what + " C", {X.EPI_MUL_DGELU: "x GELU'"}.get(e.epi, "GELU"))
    if auxbuf is not None:
        check_untouched(auxbuf, before[1], dr, N, what + " aux")
        got_aux = auxbuf[dr, :N]
        if e.epi == X.EPI_GELU:
            check_exact(got_aux, aux_ref, False, what + " aux (the stored pre-activation)")
        else:
            check_gelu(got_aux, aux_ref, None, what + " aux", "GELU'")
    check_inputs(g)


@pytest.mark.parametrize("case", X.CASES, ids=lambda c: c.id)
def test_gemm_nt_exact(ops, case):
    """One launch of the case's kernel: every element of C (and of the aux output) against the float64 reference, every guard element
    of the output buffers bit-unchanged (ldc > N, rows past M, rows c_rowmap does not name), NaN in the padding of A and B (lda,
    ldb > K, rows past M, rows a_rowmap does not name) in no result, the inputs unwritten, and the kernel id the case was written for."""
    e = X.EPIS[case.ep]
    g = problem(case.shape, e.gelu)
    with forced(ops, case.opts):
        cbuf, auxbuf, before, res_data = launch(ops, g, e)
        ran = last_kernel(ops)
    torch.cuda.synchronize()
    assert ran == case.kernel, f"{case.id}: ran on kernel {ran}, written for {case.kernel}"
    verify(g, e, cbuf, auxbuf, before, res_data, case.shape.M, case.id)


ROWS = [(k, s, o, t, ep) for (k, s, o, t) in X.ROWS_CASES for ep in X.ROWS_EPIS]


@pytest.mark.parametrize("kernel,shape,opts,tile,ep", ROWS, ids=[f"k{k}-{s.M}x{s.N}x{s.K}-{ep}" for (k, s, o, t, ep) in ROWS])
def test_gemm_nt_rows_exact(ops, kernel, shape, opts, tile, ep):
    """gemm_nt_rows with the row count on the device (1, one tile - 1, one tile, one tile + 1, M): the rows below the count are exact and
    bit-equal to gemm_nt with M = count, the rows at and past it in `out` and `aux` are bit-unchanged, and the rows of A past the
    count hold NaN."""
    e = X.EPIS[ep]
    g = problem(shape, e.gelu)
    M = shape.M
    for count in X.rows_counts(M, tile):
        what = f"rows k{kernel} {M}x{shape.N}x{shape.K} {ep} count={count}"
        a = g["a"].clone()
        a[count:] = float("nan")
        m_dev = torch.tensor([count], device=DEV, dtype=torch.int32)
        with forced(ops, opts):
            cbuf, auxbuf, before, res_data = launch(ops, g, e, m_dev=m_dev, a=a)
            ran = last_kernel(ops)
            cbuf2, auxbuf2, _, _ = launch(ops, g, e, rows=count, a=a)
        torch.cuda.synchronize()
        assert ran == kernel, f"{what}: ran on kernel {ran}"
        verify(g, e, cbuf, auxbuf, before, res_data, count, what)
        if not e.gelu:                  # exact data: whatever kernel gemm_nt took for M = count, the bits agree
            assert torch.equal(bits(cbuf), bits(cbuf2)), what + ": differs from gemm_nt with M = count"
        if auxbuf is not None and e.epi == X.EPI_GELU:
            assert torch.equal(bits(auxbuf), bits(auxbuf2)), what + ": aux differs from gemm_nt with M = count"
        assert int(m_dev[0]) == count


def test_gelu_bars(ops):
    """The worst excess over the bf16 half-ulp that the cases above observed, per function, against the floor."""
    for tag, worst in sorted(BARS.items()):
        print(f"[bar] gemm_nt {tag}: worst excess over 2^-8 |ref| across all cases {worst:.3g}, floor {X.GELU_FLOOR:g}")
        assert worst <= X.GELU_FLOOR


# ------------------------------------------------------------------------------------------------------------------
# refusals: the wrapper raises and nothing is launched
# ------------------------------------------------------------------------------------------------------------------
def _refused(ops, out_buf, fn):
    before = out_buf.clone()
    ops.gemm_nt(torch.ones(4, 32, device=DEV, dtype=torch.bfloat16), torch.ones(4, 32, device=DEV, dtype=torch.bfloat16),
                torch.empty(4, 4, device=DEV, dtype=torch.bfloat16))
    assert last_kernel(ops) == X.K128
    with pytest.raises(RuntimeError):
        fn()
    torch.cuda.synchronize()
    assert torch.equal(bits(out_buf), bits(before))
    assert last_kernel(ops) == X.K128             # the refusal came before any kernel was chosen


def _bf(*shape):
    return torch.ones(*shape, device=DEV, dtype=torch.bfloat16)


@pytest.mark.parametrize("what", ["K%32", "N%4", "lda%8", "ldc%4", "mul_dgelu", "mul_drelu", "mul_aux"])
def test_gemm_nt_refuses(ops, what):
    M, N, K = 64, 64, 64
    a, b = _bf(M, K), _bf(N, K)
    cbuf = blank(M, N, torch.bfloat16)
    out = cbuf[:M, :N]
    if what == "K%32":
        fn = lambda: ops.gemm_nt(_bf(M, 48), _bf(N, 48), out)
    elif what == "N%4":
        fn = lambda: ops.gemm_nt(a, _bf(6, K), cbuf[:M, :6])
    elif what == "lda%8":
        fn = lambda: ops.gemm_nt(_bf(M, K + 4)[:, :K], b, out)
    elif what == "ldc%4":
        c2 = blank(M, N, torch.bfloat16, guard_cols=2)
        cbuf = c2
        fn = lambda: ops.gemm_nt(a, b, c2[:M, :N])
    else:
        epi = {"mul_dgelu": ops.EPI_MUL_DGELU, "mul_drelu": ops.EPI_MUL_DRELU, "mul_aux": ops.EPI_MUL_AUX}[what]
        fn = lambda: ops.gemm_nt(a, b, out, epi=epi)
    _refused(ops, cbuf, fn)


@pytest.mark.parametrize("what", ["K=64", "f32", "alpha", "col_perm"])
def test_gemm_nt_tiles256_refuses(ops, what):
    M, N = 300, 64
    K = 64 if what == "K=64" else 128
    a, b = _bf(M, K), _bf(1, N, K)
    cbuf = blank(M, N, torch.float32 if what == "f32" else torch.bfloat16)
    tiles = torch.tensor([[0, 0, M, 0], [0, 256, M, 0]], device=DEV, dtype=torch.int32)
    count = torch.tensor([2], device=DEV, dtype=torch.int32)
    kw = dict(tiles=tiles, tile_count=count, max_tiles=2, M=M, tile_rows=256)
    if what == "alpha":
        kw["alpha"] = 0.5
    if what == "col_perm":
        kw["col_perm"] = True
    _refused(ops, cbuf, lambda: ops.gemm_nt(a, b, cbuf[:M, :N], **kw))
