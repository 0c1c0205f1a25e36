"""The references of test_expert_gemm_exact_gpu.py checked on the CPU: a case whose own reference is inexact must never reach the GPU.

For every case of expert_gemm_cases.py: the operands survive the e4m3 round trip, the float32 product equals the float64 one in two
summation orders, every intermediate of the epilogue is exact in fp32, the bf16 expectation is one rounding of a finite, normal value,
the output is not degenerate, every tile entry (those past the count included) stays inside the allocated rows - and the comparison
routine of the GPU test rejects each reference once it is corrupted the way a kernel defect would corrupt the result."""
import functools

import pytest
import torch

import expert_gemm_cases as X

F8, U8 = X.F8, X.U8


@functools.lru_cache(maxsize=None)
def _problem(key):
    c = next(c for c in X.CASES + X.RAND_CASES if c.problem_key == key)
    p = X.make_problem(c)
    return p, X.accumulate(p, torch.float64)


def problem(c):
    return _problem(c.problem_key)


def test_table_coverage():
    """What the issue's geometry table asks for, read off the case list."""
    ids = [c.id for c in X.CASES + X.RAND_CASES]
    assert len(set(ids)) == len(ids)
    grid = [c for c in X.CASES if c.data == "int" and not c.quant]
    for kernel, ks in (("mx", X.MX_KS), ("fp8", X.F8_KS)):
        mine = [c for c in grid if c.kernel == kernel]
        assert {(c.K, c.ep) for c in mine} >= {(K, ep) for K in ks for ep in X.EPIS}            # every K meets every epilogue
        for K in (ks[0], ks[-1]):                                                                   # narrowest and widest K
            assert {c.N for c in mine if c.K == K} >= set(X.NS)
            assert {c.groups for c in mine if c.K == K} >= {"rag7", "two", "e0", "one"}
        assert {c.launch for c in mine} == set(X.LAUNCHES)
        assert any(EP.inplace and c.launch in ("ldc", "eng") for c in mine for EP in [X.EPIS[c.ep]])
        assert {c.data for c in X.CASES if c.kernel == kernel} == {"int", "onehotA", "onehotB"}
    assert {c.K // 32 % 4 for c in grid if c.kernel == "mx"} == {0, 1, 2, 3}
    assert {-(-c.K // 128) for c in grid if c.kernel == "mx"} == {1, 2, 3, 8} and {c.K // 64 for c in grid if c.kernel == "fp8"} == {1, 2, 3, 16}
    assert {c.offs for c in grid if c.kernel == "mx"} == set(X.OFFS_FREE)
    assert {c.sb_none for c in grid if c.kernel == "fp8"} == {False, True}
    assert {(c.N, c.groups) for c in X.CASES if c.quant} == {(N, "rag7") for N in (32, 64, 96, 160, 192)}
    assert {c.ep for c in X.RAND_CASES if c.K == 192} == set(X.EPIS)
    for c in X.CASES + X.RAND_CASES:
        assert sum(c.counts) <= 700 and c.N <= 260 and c.K <= 1024 and c.N % 4 == 0 and c.K % (32 if c.kernel == "mx" else 64) == 0
        assert c.why
    sizes = {n for c in grid for n in c.counts}
    assert sizes >= {0, 1, 16, 17, 127, 128, 129} and X.GROUPS["two"][1] % 128 == 1 and X.GROUPS["e0"][0] == 0


@pytest.mark.parametrize("launch", X.LAUNCHES)
@pytest.mark.parametrize("groups", list(X.GROUPS))
def test_tile_entries_stay_inside_the_allocated_rows(groups, launch):
    counts = X.GROUPS[groups]
    M, G = sum(counts), len(counts)
    t, count = X.tile_table(counts, launch)
    n_real = sum(-(-c // 128) for c in counts)
    assert count == (0 if launch == "count0" else n_real)
    assert len(t) == n_real + (3 if launch in ("guard", "eng") else 0) and len(t) > 0
    ends = torch.tensor(counts).cumsum(0)
    covered = torch.zeros(M + X.GUARD, dtype=torch.int32)
    for i, (g, m0, m_end, _) in enumerate(t.tolist()):
        assert 0 <= g < G and 0 <= m0 < m_end <= M + X.GUARD                # rows m0 .. min(m0 + 128, m_end) - 1, clamped reads at m_end - 1
        if i < n_real:
            assert m_end == int(ends[g]) and m0 >= int(ends[g]) - counts[g] and (m0 - (int(ends[g]) - counts[g])) % 128 == 0
            covered[m0:min(m0 + 128, m_end)] += 1
        else:
            assert m0 >= M                                                   # the guard band: never a row of the result
    assert bool((covered[:M] == 1).all()) and bool((covered[M:] == 0).all())
    if launch == "shuf" and n_real > 1:
        assert not torch.equal(t, X.tile_table(counts, "tight")[0])


def _exact_f32(m, what):
    assert bool(torch.isfinite(m).all()), what
    assert torch.equal(m.float().double(), m), what


@pytest.mark.parametrize("case", X.CASES, ids=lambda c: c.id)
def test_reference_is_exact(case):
    p, acc64 = problem(case)
    e = X.EPIS[case.ep]
    M, N, K = p.M, p.N, p.K
    # operands: e4m3 round trip, ranges, guard band filled
    for q in (p.aq, p.bq):
        f = q.view(F8).float()
        assert not bool(torch.isnan(f).any()) and torch.equal(f.to(F8).view(U8) & 0x7F, q & 0x7F)
    assert p.aq.shape == (p.R, K) and p.residual.shape == (p.R, N) and p.aux.shape == (p.R, N)
    assert bool((p.aq[M:] != 0).any(1).all())                                    # the band holds non-zero operands
    if case.data == "int":
        assert float(p.a.abs().max()) <= 4 and float(p.b.abs().max()) <= 3
        assert not torch.equal(p.b[0, -1], -p.b[0, -1]) and not torch.equal(p.b[0, -1], p.b[0, -2])
        assert not torch.equal(p.a[0], p.a[1])
    for t in (p.residual, p.aux):
        assert torch.equal(t.to(torch.bfloat16).float(), t) and torch.equal(t, t.round())
    assert float(p.residual.abs().max()) <= 8 and float(p.aux.abs().max()) <= 3
    if p.aux.numel() >= 1024:
        assert bool((p.aux == 0).any()) and bool((p.aux > 0).any()) and bool((p.aux < 0).any())
    tiny = case.quant == "tiny"           # bias = the quantiser's edge rows, bf16-subnormal outputs on purpose
    assert tiny or torch.equal(p.bias * 8, (p.bias * 8).round()) and (case.quant or float(p.bias.abs().max()) <= 16)
    if case.kernel == "mx":
        ja = p.sa.int() - 127 - case.offs[0]
        jb = p.sb.int() - 127 - case.offs[1]
        assert int(ja.min()) >= -2 and int(ja.max()) <= 2 and int(jb.min()) >= -1 and int(jb.max()) <= 1
        if K > 32:
            assert bool((ja[:, 1:] != ja[:, :-1]).all()) and bool((jb[..., 1:] != jb[..., :-1]).all())    # a stale scale byte shows
        assert bool((ja[1:] != ja[:-1]).all())
    else:
        for s in (p.sa,) + (() if p.sb is None else (p.sb,)):
            assert torch.equal(torch.log2(s), torch.log2(s).round()) and float(torch.log2(s).abs().max()) <= 3
        assert (p.sb is None) == case.sb_none
    # the product: float32 equals float64 in two summation orders
    a32, acc32 = X.dequant_a(p, torch.float32), X.accumulate(p, torch.float32)
    assert torch.equal(X.dequant_a(p).float(), a32)
    assert torch.equal(acc32.double(), acc64) and torch.equal(X.accumulate(p, torch.float32, flip=True).double(), acc64)
    assert torch.equal(X.accumulate(p, torch.float64, flip=True), acc64)
    if case.data == "int":               # the stated unit and bound (fp8: the scales come after the product)
        off = sum(case.offs)
        unit, bound = (2.0 ** (off - 3), 2.0 ** (off + 15)) if case.kernel == "mx" else (1.0, 2.0 ** 14)
        assert torch.equal(acc64 / unit, (acc64 / unit).round()) and float(acc64.abs().max()) < bound
    # the epilogue: every intermediate exact in fp32, and the float32 evaluation in the kernel's order gives the same numbers
    c64, inter = X.epilogue(p, e, acc64)
    c32, _ = X.epilogue(p, e, acc32, torch.float32)
    for m in inter + [c64]:
        _exact_f32(m, case.id)
    assert torch.equal(c32.double(), c64)
    exp = X.to_bf16_once(c64)
    assert torch.equal(exp, X.expected_c(p, case))
    assert bool(((exp.double() - c64).abs() <= 2.0 ** -8 * c64.abs()).all())
    nz = c64 != 0
    assert not bool(torch.isnan(exp.float()).any()) and not bool(torch.isinf(exp.float()).any())
    assert tiny or float(c64[nz].abs().min()) >= 2.0 ** -126 and float(exp.float()[nz].abs().min()) >= 2.0 ** -126       # never subnormal
    assert not bool((X.bits(exp) == X.PAT_C).any())
    # not degenerate
    if case.data == "int":
        if e.epi == X.EPI_NONE:
            assert float((c64 == 0).float().mean()) < 0.05
            # the output rounding is exercised: the mixed block scales of MX leave most sums with more than 8 significant bits; the fp8
            # sums are integers times ONE power of two, inexact in bf16 only above 256 (sigma is about 165 at K = 1024)
            if K >= 256:
                assert float((exp.double() != c64).float().mean()) > (0.3 if case.kernel == "mx" else 0.03 if K == 1024 else 0.0)
        pre = inter[-1]
        if e.epi == X.EPI_RELU and not case.quant:
            assert bool((pre > 0).any()) and bool((pre < 0).any())
        if e.epi == X.EPI_MUL_DRELU and M * N >= 64:
            aux = p.aux[:M]
            assert bool(((aux > 0) & (pre != 0)).any()) and bool(((aux <= 0) & (pre != 0)).any())
    elif case.data == "onehotA":
        # every output is one product: the dequantised code; every code meets every 16-byte run of the k-step (lane group x half)
        k = torch.arange(M) % K
        want = p.b[p.group_of_row][torch.arange(M), :, k].double()
        sc = (acc64 / want)[want != 0]
        assert torch.equal(torch.log2(sc), torch.log2(sc).round()) and bool((acc64[want == 0] == 0).all())
        seen = {(int(code), int(kk) >> 4 & 7) for g in range(p.G) for kk in k[p.group_of_row == g].unique().tolist() for code in p.bq[g, :, kk]}
        assert len(seen) == 254 * 8 and set(k.tolist()) == set(range(K))
        assert torch.equal(exp.float().double(), c64)                                      # every e4m3 value (scaled) is exact in bf16
    elif case.data == "onehotB":
        want = p.a[:M, torch.arange(N) % K].double()
        sc = (acc64 / want)[want != 0]
        assert torch.equal(torch.log2(sc), torch.log2(sc).round()) and bool((acc64[want == 0] == 0).all())
        seen = {(int(code), kk >> 4 & 7) for kk in range(K) for code in p.aq[:M, kk]}
        assert len(seen) == 254 * 8 and N >= K
        assert torch.equal(exp.float().double(), c64)
    if case.quant:
        q, s = X.mx_quant(exp.float())
        assert not bool(torch.isnan(q.view(F8).float()).any())
        if tiny:
            for g, (lo, cnt) in enumerate(zip([0] + torch.tensor(p.counts).cumsum(0).tolist(), p.counts)):
                assert bool((s[lo:lo + cnt, 0] == [3, 1, 1, 1, 1, 247][g % 6]).all())
                assert g % 6 != 4 or bool((q[lo:lo + cnt, 1] == 0x04).all() and (exp[lo:lo + cnt, 1].float() == 2.0 ** -133).all())
            assert torch.equal(exp[:, :32].float().double(), c64[:, :32])                  # the tiny block is exact in bf16
        if "neg" in case.quant:
            assert bool((s[:, -1] == 127).all()) and bool((q[:, N - 32:] == 0).all()) and bool((exp[:, N - 32:] == 0).all())
        if "pow2" in case.quant:
            assert bool((s[:, 0] == 124).all()) and bool((q[:, 5] == 0x7E).all())          # amax = 56 = 448 * 2^-3: not rounded up
        assert int((s != 127).sum()) > s.numel() // 4 and not bool((q == X.PAT_Q).all()) and len(s.unique()) >= 3


def _corruptions(case, p, acc64):
    """The reference of `case` corrupted the way a kernel defect would: (name, corrupted float64 product or None, raw edit)."""
    M, N, K = p.M, p.N, p.K
    r0 = max(0, min(M - 16, 130) // 16 * 16) if M >= 32 else 0
    hi = min(r0 + 16, M)
    rows = (r0, hi)
    out = []

    def patched(block):
        acc = acc64.clone()
        acc[r0:hi] = block
        return acc

    if M >= 32:
        acc = acc64.clone()
        acc[r0:hi, :min(16, N)] = acc64[r0 + 1:hi + 1, :min(16, N)] if hi < M else acc64[r0 - 1:hi - 1, :min(16, N)]
        out.append(("a 16-row subtile shifted by one row", acc))
    if case.kernel == "mx":
        sa = p.sa.clone()
        sa[r0, (K // 32) - 1] += 1
        out.append(("one scale byte of one 32-block off by one", patched(X.accumulate(p, a=X.dequant_a(p, sa=sa), rows=rows))))
        if K % 128:                     # the k-step's first 32-block past K left in: piece 0 of the row under scale byte 127
            extra = X.accumulate(X.Problem(p.kernel, N, 32, p.counts, p.aq[:, :32].contiguous(), p.bq[:, :, :32].contiguous(),
                                           torch.full((p.R, 1), 127, dtype=U8), torch.full((p.G, N, 1), 127, dtype=U8), p.bias, p.residual, p.aux), rows=rows)
            out.append(("one K-tail block left non-zero", patched(acc64[r0:hi] + extra)))
    else:
        sa = p.sa.clone()
        sa[r0] *= 2
        q = X.Problem(p.kernel, N, K, p.counts, p.aq, p.bq, sa, p.sb, p.bias, p.residual, p.aux)
        out.append(("one row scale off by one binade", ("problem", q)))
    run = 16 if case.kernel == "mx" else 8
    i, j = (16, 80) if K >= 128 else (0, run)
    aq = p.aq.clone()                   # the bytes move, the scale bytes stay with their blocks
    aq[r0:hi, i:i + run], aq[r0:hi, j:j + run] = p.aq[r0:hi, j:j + run], p.aq[r0:hi, i:i + run]
    out.append(("the two runs of a lane swapped", patched(X.accumulate(p, a=X.dequant_a(p, aq=aq), rows=rows))))
    return out


SENS = [c for c in X.CASES if c.data == "int" and not c.quant and c.launch != "count0" and c.N >= 16]      # N = 4: no 16-column subtile to shift


@pytest.mark.parametrize("case", SENS, ids=lambda c: c.id)
def test_comparison_rejects_a_corrupted_reference(case):
    """Sensitivity, shown on the CPU: the buffer the GPU test would read back, built from the true reference, passes X.check_buffer;
    built from a reference with one subtile shifted / one scale changed / one K-tail block left in / two k-runs swapped, or with one
    guard element written, it is rejected."""
    p, acc64 = problem(case)
    e = X.EPIS[case.ep]
    M, N, ldc = p.M, p.N, X.ldc_of(case)
    before = torch.empty(p.R, ldc, dtype=torch.bfloat16)
    X.bits(before).fill_(X.PAT_C)
    if e.inplace:
        before[:, :N] = p.residual.to(torch.bfloat16)
    exp = X.expected_c(p, case)

    def image(res):
        buf = before.clone()
        buf[:M, :N] = res
        return buf

    X.check_buffer(image(exp), before, exp, M, N, case.id)
    n = 0
    for name, acc in _corruptions(case, p, acc64):
        if isinstance(acc, tuple):
            wrong = X.to_bf16_once(X.epilogue(acc[1], e, acc64)[0])
        else:
            wrong = X.to_bf16_once(X.epilogue(p, e, acc)[0])
        with pytest.raises(AssertionError, match="result: "):
            X.check_buffer(image(wrong), before, exp, M, N, case.id + ": " + name)
        n += 1
    assert n >= 3
    for r, col in ((M, 0), (p.R - 1, N - 1)) + (((0, N),) if ldc > N else ()):      # a guard row / a pad column written
        buf = image(exp)
        X.bits(buf)[r, col] ^= 0x0040
        with pytest.raises(AssertionError, match="outside the result"):
            X.check_buffer(buf, before, exp, M, N, case.id)
    with pytest.raises(AssertionError):                                               # count0: nothing may be written
        X.check_buffer(image(exp), before, None, M, N, case.id)


@pytest.mark.parametrize("case", [c for c in X.CASES if c.quant], ids=lambda c: c.id)
def test_quantised_output_comparison_rejects_a_changed_block(case):
    p, _ = problem(case)
    exp = X.expected_c(p, case)
    q, s = X.mx_quant(exp.float())
    bq, bs = torch.full((p.R, p.N), X.PAT_Q, dtype=U8), torch.full((p.R, p.N // 32), X.PAT_S, dtype=U8)
    iq, isc = bq.clone(), bs.clone()
    iq[:p.M], isc[:p.M] = q, s
    X.check_buffer(iq, bq, q, p.M, p.N, case.id)
    X.check_buffer(isc, bs, s, p.M, p.N // 32, case.id)
    isc[2, 0] += 1
    with pytest.raises(AssertionError, match="result: "):
        X.check_buffer(isc, bs, s, p.M, p.N // 32, case.id)
    iq[p.M + 1, 3] = 0
    with pytest.raises(AssertionError, match="outside the result"):
        X.check_buffer(iq, bq, q, p.M, p.N, case.id)


@pytest.mark.parametrize("case", X.RAND_CASES, ids=lambda c: c.id)
def test_fp32_emulation_is_inside_the_derived_bar(case):
    """Non-power-of-two fp8 scales: the accumulator is exact, the epilogue is not.  A CPU fp32 evaluation in the kernel's order (each
    operation rounded once), rounded to bf16, stays inside 2^-8 |ref| + 2^-22 (|S sa sb| + |bias| + |residual|) for every element: the
    reference alone passes the GPU test's criterion, and a changed row scale does not."""
    p, acc64 = problem(case)
    e = X.EPIS[case.ep]
    M, N = p.M, p.N
    assert torch.equal(X.accumulate(p, torch.float32).double(), acc64) and torch.equal(acc64, acc64.round())
    ref, _ = X.epilogue(p, e, acc64)
    emu = X.epilogue(p, e, acc64.float(), torch.float32)[0].to(torch.bfloat16)
    bar = X.rand_bar(p, e, acc64, ref)
    masked = (p.aux[:M] <= 0) if e.epi == X.EPI_MUL_DRELU else None
    worst = float(((emu.double() - ref).abs() / bar.clamp_min(1e-300)).max())
    print(f"[bar] {case.id}: worst |emulation - ref| / bar {worst:.3f}")
    before = torch.zeros(p.R, X.ldc_of(case), dtype=torch.bfloat16)
    buf = before.clone()
    buf[:M, :N] = emu
    X.check_rand(buf, before, ref, bar, masked, M, N, case.id)
    assert masked is None or (bool((ref[masked] == 0).all()) and bool((ref[~masked] != 0).any()))
    sa = p.sa.clone()
    sa[7] *= 2.0
    q = X.Problem(p.kernel, N, p.K, p.counts, p.aq, p.bq, sa, p.sb, p.bias, p.residual, p.aux)
    buf[:M, :N] = X.epilogue(q, e, acc64.float(), torch.float32)[0].to(torch.bfloat16)
    with pytest.raises(AssertionError):
        X.check_rand(buf, before, ref, bar, masked, M, N, case.id)
    if masked is not None:
        buf[:M, :N] = emu
        r, col = masked.nonzero()[0].tolist()
        buf[r, col] = -0.0                                     # a masked element must be +0 exactly
        with pytest.raises(AssertionError):
            X.check_rand(buf, before, ref, bar, masked, M, N, case.id)


def test_every_e4m3_value_is_exact_in_bf16_and_the_tiny_block_rule():
    """The facts the GPU file's decode and quantiser-edge cases rest on, from the CPU twin."""
    v = X.CODES.view(F8).float()
    assert len(v) == 254 and bool(torch.isfinite(v).all()) and torch.equal(v.to(torch.bfloat16).float(), v)
    assert float(v.abs().max()) == 448.0 and int((v == 0).sum()) == 2 and float(v[v > 0].min()) == 2.0 ** -9
    x = X.tiny_rows()
    q, s = X.mx_quant(x)
    assert s[:, 0].tolist()[2:] == [1, 1, 1, 247] and int(s[0, 0]) > int(s[1, 0]) >= 1 and s[:2, 0].tolist() == [3, 1]
    assert int(q[4, 1]) == 0x04 and int(q[4, 0]) == 0x10 and bool((q[:6, :32] != 0).any(1).all())
    assert torch.equal(x.to(torch.bfloat16).float(), x)
