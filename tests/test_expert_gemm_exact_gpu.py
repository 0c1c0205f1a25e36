"""Exact per-element tests of the two grouped expert GEMMs (medmoe_gemm_fp8_grouped, medmoe_gemm_mx_grouped) and of their quantisers.

The data of expert_gemm_cases.py makes the float64 reference THE result (test_expert_gemm_exact_host.py proves it per case on the CPU):
every bf16 element of C is compared bit for bit with one round-to-nearest-even of the reference, the fused quantised output with the
CPU twin of the EXPECTED C, and every buffer a launch can reach - pad columns (ldc > N) and the guard band of 128 rows that the tile
entries past tile_count[0] describe - must keep its prefill: written exactly where it should be and nowhere else.  Every expectation
is computed on the CPU."""
import pytest
import torch

import expert_gemm_cases as X

pytestmark = pytest.mark.gpu

DEV = "cuda"
F8, U8, BF = X.F8, X.U8, torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from medmoe_amd import ops as o
    return o


_PROBLEMS = {}


def problem(case):
    """CPU operands, their device images and the float64 product, built once per problem and never written again."""
    key = case.problem_key
    if key not in _PROBLEMS:
        if len(_PROBLEMS) >= 6:
            _PROBLEMS.pop(next(iter(_PROBLEMS)))
        p = X.make_problem(case)
        d = dict(aq=p.aq.to(DEV), bq=p.bq.contiguous().to(DEV), sa=p.sa.contiguous().to(DEV), sb=None if p.sb is None else p.sb.contiguous().to(DEV),
                 bias=p.bias.to(DEV))
        _PROBLEMS[key] = (p, d, X.accumulate(p))
    return _PROBLEMS[key]


def prefilled(rows, cols, dtype, pat, data=None, width=None):
    """A device buffer of the pattern with `data` ([rows, width]) in its left columns."""
    buf = torch.empty(rows, cols, device=DEV, dtype=dtype)
    X.bits(buf).fill_(pat)
    if data is not None:
        buf[:, :width] = data.to(DEV).to(dtype)
    return buf


def launch(ops, case, p, d, quant=False):
    """One launch in the case's form.  Returns the buffers {name: (after, before)} and the residual image the launch read."""
    e = X.EPIS[case.ep]
    N, K, R, ldc = p.N, p.K, p.R, X.ldc_of(case)
    tiles, count = X.tile_table(p.counts, case.launch)
    tiles_d, count_d = tiles.to(DEV), torch.tensor([count], device=DEV, dtype=torch.int32)
    # residual and aux are read at the output's offsets (row * ldc + n): the same row stride, NaN in their pad columns
    res = prefilled(R, ldc, BF, X.PAT_C, p.residual, N) if e.residual else None
    aux = prefilled(R, ldc, BF, X.PAT_C, p.aux, N) if e.epi == X.EPI_MUL_DRELU else None
    c = prefilled(R, ldc, BF, X.PAT_C, p.residual if e.inplace else None, N)      # in place: the output holds the residual, guard band included
    if e.inplace:
        res = c
    bufs = {"C": c}
    bias = d["bias"] if e.bias else None
    sbias = N if e.bias else 0
    if case.kernel == "mx":
        if quant:
            bufs["Cq"] = prefilled(R, N, U8, X.PAT_Q)
            bufs["Csq"] = prefilled(R, N // 32, U8, X.PAT_S)
        before = {k: v.clone() for k, v in bufs.items()}
        ops.call("gemm_mx_grouped", d["aq"], d["sa"], d["bq"], d["sb"], bias, c, ldc, res, aux, bufs.get("Cq"), bufs.get("Csq"),
                 tiles_d, count_d, tiles.shape[0], N, K, N * K, N * (K // 32), sbias, e.epi)
    else:
        before = {k: v.clone() for k, v in bufs.items()}
        ops.call("gemm_fp8_grouped", d["aq"], d["sa"], d["bq"], d["sb"], bias, c, ldc, res, aux,
                 tiles_d, count_d, tiles.shape[0], N, K, N * K, 0 if d["sb"] is None else N, sbias, e.epi)
    torch.cuda.synchronize()
    assert int(count_d[0]) == count and torch.equal(tiles_d.cpu(), tiles)
    if aux is not None:
        assert torch.equal(X.bits(aux[:, :N]).cpu(), X.bits(p.aux.to(BF))), "the launch wrote into aux"
    if res is not None and not e.inplace:
        assert torch.equal(X.bits(res[:, :N]).cpu(), X.bits(p.residual.to(BF))), "the launch wrote into residual"
    return {k: (v.cpu(), before[k].cpu()) for k, v in bufs.items()}


@pytest.mark.parametrize("case", X.CASES, ids=lambda c: c.id)
def test_expert_gemm_exact(ops, case):
    """Every element of C bit-equal to the one rounding of the float64 reference; the fused Cq / Csq bit-equal to mx_quant (CPU twin) of
    the EXPECTED C; pad columns, guard rows and, with tile_count[0] = 0, the whole output bit-unchanged."""
    p, d, acc64 = problem(case)
    e = X.EPIS[case.ep]
    out = launch(ops, case, p, d, quant=bool(case.quant))
    exp = X.to_bf16_once(X.epilogue(p, e, acc64)[0])       # in place: p.residual IS the copy of what the output held
    nothing = case.launch == "count0"
    X.check_buffer(*out["C"], None if nothing else exp, p.M, p.N, case.id + " C")
    if case.quant:
        q, s = X.mx_quant(exp.float())
        X.check_buffer(*out["Csq"], s, p.M, p.N // 32, case.id + " Csq")
        X.check_buffer(*out["Cq"], q, p.M, p.N, case.id + " Cq")


@pytest.mark.parametrize("case", X.RAND_CASES, ids=lambda c: c.id)
def test_gemm_fp8_random_scales(ops, case):
    """Integer data (an exact accumulator S) under random fp32 sa, sb, bias: every element against float64 within the derived bar
    2^-8 |ref| + 2^-22 (|S sa sb| + |bias| + |residual|), masked elements exactly zero, nothing else written."""
    p, d, acc64 = problem(case)
    e = X.EPIS[case.ep]
    out = launch(ops, case, p, d)
    ref, _ = X.epilogue(p, e, acc64)
    bar = X.rand_bar(p, e, acc64, ref)
    got = out["C"][0][:p.M, :p.N].double()
    print(f"[bar] {case.id}: worst |got - ref| / bar {float(((got - ref).abs() / bar.clamp_min(1e-300)).max()):.3f}")
    X.check_rand(*out["C"], ref, bar, (p.aux[:p.M] <= 0) if e.epi == X.EPI_MUL_DRELU else None, p.M, p.N, case.id)


# ------------------------------------------------------------------------------------------------------------------
# refusals: the entry returns before any launch and ops.call raises
# ------------------------------------------------------------------------------------------------------------------
MX_REFUSALS = ["K%32", "N%4", "ldc%4", "Cq_without_Csq", "Cq_epi0", "Cq_N%32", "epi2_without_aux"]
F8_REFUSALS = ["K%64", "N%4", "ldc%4", "epi2_without_aux"]


@pytest.mark.parametrize("kernel,what", [("mx", w) for w in MX_REFUSALS] + [("fp8", w) for w in F8_REFUSALS])
def test_expert_gemm_refuses(ops, kernel, what):
    M, N, K, ldc, epi = 64, 64, 128, 64, 1
    if what in ("K%32", "K%64"):
        K = 48 if kernel == "mx" else 96
    if what == "N%4":
        N = 62
    if what == "ldc%4":
        ldc = 66
    if what == "Cq_N%32":
        N = 48
    if what == "Cq_epi0":
        epi = 0
    if what == "epi2_without_aux":
        epi = 2
    mx = kernel == "mx"
    aq = torch.full((M, 128), 0x38, device=DEV, dtype=U8); bq = torch.full((1, 64, 128), 0x38, device=DEV, dtype=U8)
    sa = torch.full((M, 4), 127, device=DEV, dtype=U8) if mx else torch.ones(M, device=DEV)
    sb = torch.full((1, 64, 4), 127, device=DEV, dtype=U8) if mx else torch.ones(1, 64, device=DEV)
    c = prefilled(M, 68, BF, X.PAT_C)
    cq, cs = prefilled(M, 64, U8, X.PAT_Q), prefilled(M, 2, U8, X.PAT_S)
    tiles = torch.tensor([[0, 0, M, 0]], device=DEV, dtype=torch.int32); cnt = torch.tensor([1], device=DEV, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        if mx:
            use_q = what.startswith("Cq")
            ops.call("gemm_mx_grouped", aq, sa, bq, sb, None, c, ldc, None, None, cq if use_q else None, cs if use_q and what != "Cq_without_Csq" else None,
                     tiles, cnt, 1, N, K, N * K, N * (K // 32), 0, epi)
        else:
            ops.call("gemm_fp8_grouped", aq, sa, bq, sb, None, c, ldc, None, None, tiles, cnt, 1, N, K, N * K, N, 0, epi)
    torch.cuda.synchronize()
    assert bool((X.bits(c) == X.PAT_C).all()) and bool((cq == X.PAT_Q).all()) and bool((cs == X.PAT_S).all())


# ------------------------------------------------------------------------------------------------------------------
# quantisers: bit-exact against the CPU twins
# ------------------------------------------------------------------------------------------------------------------
def e4m3_rows_twin(xr):
    """test_fp8_gpu.py's expressions, on the CPU: scale = amax / 448 (1 for an all-zero row), elements rne_e4m3(x * (1 / scale))."""
    amax = xr.abs().amax(-1)
    s = torch.where(amax > 0, amax * (1.0 / 448.0), torch.ones_like(amax))
    return (xr * (1.0 / s)[..., None]).to(F8).view(U8), s


def _rows_input(M, K, ldx, seed):
    """bf16 rows of very different magnitudes in a buffer of row stride ldx; the gap holds 3e38 (it must reach no amax)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-12, 6, (M, 1), generator=g).float())).to(BF)
    if M > 2:
        x[M // 2] = 0
    buf = torch.full((M, ldx), 3.0e38, dtype=BF)
    buf[:, :K] = x
    return x.float(), buf


ROW_SHAPES = [(1, 32, 0), (3, 32, 0), (5, 32, 0), (16389, 32, 0), (5, 96, 8), (7, 64, 64), (131, 1024, 8)]


@pytest.mark.parametrize("M,K,gap", ROW_SHAPES, ids=[f"M{m}-K{k}-ldx+{g}" for m, k, g in ROW_SHAPES])
@pytest.mark.parametrize("kind", ["mx", "e4m3"])
def test_row_quantisers_bit_exact(ops, kind, M, K, gap):
    """M not a multiple of the 4 rows of a workgroup, M past the grid cap of 4096 workgroups (the grid-stride loop), ldx = K + 8 and 2 K
    with a sentinel in the gap, plain and gathered with repeated source rows; the outputs are prefilled with one row past M."""
    x, buf = _rows_input(M, K, K + gap, 1000 * M + K)
    xd = buf.to(DEV)
    g = torch.Generator().manual_seed(M)
    rowmap = torch.randint(0, M, (M,), generator=g).int()                 # repeats (and leaves rows out) as soon as M > 1
    for use_map in (False, True):
        xr = x[rowmap.long()] if use_map else x
        rm = rowmap.to(DEV) if use_map else None
        q = prefilled(M + 1, K, U8, X.PAT_Q)
        if kind == "mx":
            s = prefilled(M + 1, K // 32, U8, X.PAT_S)
            q0, s0 = q.clone(), s.clone()
            ops.call("quant_rows_mx", xd, K + gap, rm, q, s, M, K)
            q_ref, s_ref = X.mx_quant(xr)
            X.check_buffer(s, s0, s_ref, M, K // 32, f"quant_rows_mx scales map={use_map}")
        else:
            s = prefilled(M + 1, 1, torch.float32, 0x7FC00001)
            q0, s0 = q.clone(), s.clone()
            ops.call("quant_rows_e4m3", xd, K + gap, rm, None, None, 1, q, s, M, K)
            q_ref, s_ref = e4m3_rows_twin(xr)
            X.check_buffer(s, s0, s_ref[:, None], M, 1, f"quant_rows_e4m3 scales map={use_map}")
        X.check_buffer(q, q0, q_ref, M, K, f"quant_rows_{kind} elements map={use_map}")
    assert torch.equal(X.bits(xd).cpu(), X.bits(buf))


@pytest.mark.parametrize("rows_per_slot", [1, 7])
def test_quant_rows_e4m3_column_scales(ops, rows_per_slot):
    """The dgrad form: the per-expert column scale multiplied in before the row's amax; slots map to experts out of order."""
    K, E = 96, 3
    slot_e = torch.tensor([2, 0, 1, 1, 2, 0, 0], dtype=torch.int32)
    M = rows_per_slot * len(slot_e) - (3 if rows_per_slot > 1 else 0)      # the last slot is not full
    x, buf = _rows_input(M + 4, K, K + 8, 77 + rows_per_slot)
    g = torch.Generator().manual_seed(3)
    cs = torch.rand(E, K, generator=g) + 0.5
    rowmap = torch.randint(0, M + 4, (M,), generator=g).int()
    xr = x[rowmap.long()] * cs[slot_e.long()].repeat_interleave(rows_per_slot, 0)[:M]
    q, s = prefilled(M + 1, K, U8, X.PAT_Q), prefilled(M + 1, 1, torch.float32, 0x7FC00001)
    q0, s0 = q.clone(), s.clone()
    ops.call("quant_rows_e4m3", buf.to(DEV), K + 8, rowmap.to(DEV), cs.to(DEV), slot_e.to(DEV), rows_per_slot, q, s, M, K)
    q_ref, s_ref = e4m3_rows_twin(xr)
    X.check_buffer(s, s0, s_ref[:, None], M, 1, "quant_rows_e4m3 colscale scales")
    X.check_buffer(q, q0, q_ref, M, K, "quant_rows_e4m3 colscale elements")


def test_quant_rows_mx_tiny_and_huge_blocks(ops):
    """Blocks whose amax / 448 is an fp32 subnormal (scale byte clamped to 1, inverse 2^126), bf16-subnormal inputs and 3.0e38: the rule in
    the header of mxfp8.hip keeps every denormal; the twin runs on the CPU, where nothing is flushed."""
    x = X.tiny_rows()
    q_ref, s_ref = X.mx_quant(x)
    assert s_ref[:, 0].tolist() == [3, 1, 1, 1, 1, 247] and int(q_ref[4, 1]) == 0x04
    M, K = x.shape
    q, s = prefilled(M + 1, K, U8, X.PAT_Q), prefilled(M + 1, K // 32, U8, X.PAT_S)
    q0, s0 = q.clone(), s.clone()
    ops.call("quant_rows_mx", x.to(BF).to(DEV), K, None, q, s, M, K)
    X.check_buffer(s, s0, s_ref, M, K // 32, "quant_rows_mx tiny / huge blocks: scales")
    X.check_buffer(q, q0, q_ref, M, K, "quant_rows_mx tiny / huge blocks: elements")


W8_SHAPES = [(1, 5, 4, True), (3, 7, 260, True), (2, 6, 1024, True), (2, 6, 1024, False), (2, 8195, 4, True), (2, 8195, 4, False)]


@pytest.mark.parametrize("G,N,K,with_t", W8_SHAPES, ids=[f"G{g}-N{n}-K{k}-{'qT' if t else 'noqT'}" for g, n, k, t in W8_SHAPES])
def test_quant_weights_e4m3_bit_exact(ops, G, N, K, with_t):
    """K = 4, 260, 1024: one pass, the second and the fourth pass of the 256-wide loop; N no multiple of the 4 rows of a workgroup;
    G N = 16390 rows: the grid-stride loop; qT = None; an all-zero row (scale 1)."""
    g = torch.Generator().manual_seed(G * 100 + N + K)
    w = torch.randn(G, N, K, generator=g) * 0.05 * torch.exp2(torch.randint(-6, 6, (G, N, 1), generator=g).float())
    w[G - 1, N // 2] = 0
    q, s = prefilled(G * N + 1, K, U8, X.PAT_Q), prefilled(G * N + 1, 1, torch.float32, 0x7FC00001)
    qT = prefilled(G * K + 1, N, U8, X.PAT_Q) if with_t else None
    q0, s0, t0 = q.clone(), s.clone(), None if qT is None else qT.clone()
    ops.call("quant_weights_e4m3", w.to(DEV), q, qT, s, G, N, K)
    q_ref, s_ref = e4m3_rows_twin(w)
    assert float(s_ref[G - 1, N // 2]) == 1.0
    X.check_buffer(s, s0, s_ref.reshape(-1, 1), G * N, 1, "quant_weights_e4m3 scales")
    X.check_buffer(q, q0, q_ref.reshape(G * N, K), G * N, K, "quant_weights_e4m3 elements")
    if with_t:
        X.check_buffer(qT, t0, q_ref.transpose(1, 2).reshape(G * K, N), G * K, N, "quant_weights_e4m3 transposed elements")


WMX_SHAPES = [(1, 32, 32), (2, 32, 160), (2, 160, 32)]


@pytest.mark.parametrize("G,N,K", WMX_SHAPES, ids=[f"G{g}-N{n}-K{k}" for g, n, k in WMX_SHAPES])
def test_quant_weights_mx_bit_exact(ops, G, N, K):
    """The minimum shape, a non-square one and its converse; a 32 x 32 block that is all zero along K for some rows but not along N
    (row scales 127, column scales not); a tiny-amax block (scale byte clamped to 1 in both directions)."""
    g = torch.Generator().manual_seed(G + N + K)
    w = torch.randn(G, N, K, generator=g) * 0.05 * torch.exp2(torch.randint(-4, 4, (G, N, 1), generator=g).float())
    w[0, 3:9, 0:32] = 0                                        # rows 3..8 of block (0, 0): zero along K, the columns still see the other rows
    if N > 32 or K > 32:
        n1, k1 = (N - 32, 0) if N > 32 else (0, K - 32)
        w[G - 1, n1:n1 + 32, k1:k1 + 32] = torch.randn(32, 32, generator=g) * 2.0 ** -122
    q, sq = prefilled(G * N + 1, K, U8, X.PAT_Q), prefilled(G * N + 1, K // 32, U8, X.PAT_S)
    qT, sT = prefilled(G * K + 1, N, U8, X.PAT_Q), prefilled(G * K + 1, N // 32, U8, X.PAT_S)
    b = [t.clone() for t in (q, sq, qT, sT)]
    ops.call("quant_weights_mx", w.to(DEV), q, sq, qT, sT, G, N, K)
    q_ref, s_ref = X.mx_quant(w)
    t_ref, st_ref = X.mx_quant(w.transpose(1, 2).contiguous())
    assert bool((s_ref[0, 3:9, 0] == 127).all()) and not bool((st_ref[0, :32, 0] == 127).any())
    assert N == 32 and K == 32 or (int(s_ref[G - 1].min()) == 1 and int(st_ref[G - 1].min()) == 1)
    X.check_buffer(sq, b[1], s_ref.reshape(G * N, -1), G * N, K // 32, "quant_weights_mx scales along K")
    X.check_buffer(q, b[0], q_ref.reshape(G * N, K), G * N, K, "quant_weights_mx elements along K")
    X.check_buffer(sT, b[3], st_ref.reshape(G * K, -1), G * K, N // 32, "quant_weights_mx scales along N")
    X.check_buffer(qT, b[2], t_ref.reshape(G * K, N), G * K, N, "quant_weights_mx elements along N")
