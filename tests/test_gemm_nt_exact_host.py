"""The references of test_gemm_nt_exact_gpu.py checked on the CPU: a case whose own reference is inexact must never reach the GPU test.

For every case of the table: the operands are exact in bf16, the float32 matmul equals the float64 one, every intermediate of the
epilogue is exact in fp32 (an integer or half-integer below 2^24; a multiple of 1/64 below 2^24 / 64 for the GELU data), the bf16
expectation is produced by one rounding, and the float32 emulation of common.h's GELU polynomial stays within the figures the GPU test's
floor is built on."""
import functools

import numpy as np
import pytest
import torch

import gemm_exact_cases as X


@functools.lru_cache(maxsize=None)
def _problem(shape, gelu):
    o = X.make_operands(shape, gelu)
    acc64 = X.accumulate(o, torch.float64)
    acc32 = X.accumulate(o, torch.float32)
    return o, acc64, acc32


def _problems():
    seen = {}
    for c in X.CASES:
        seen.setdefault((c.shape, X.EPIS[c.ep].gelu), []).append(c.ep)
    for _, shape, _, _ in X.ROWS_CASES:
        for ep in X.ROWS_EPIS:
            seen.setdefault((shape, X.EPIS[ep].gelu), []).append(ep)
    return [(s, g, tuple(sorted(set(eps)))) for (s, g), eps in seen.items()]


PROBLEMS = _problems()


def _pid(p):
    s, g, _ = p
    return f"{'g%d-' % s.tile_rows if s.grouped else ''}{s.M}x{s.N}x{s.K}{'-gelu' if g else ''}"


def test_table_covers_every_kernel_and_stays_small():
    assert {c.kernel for c in X.CASES} == set(range(7))
    assert len({c.id for c in X.CASES}) == len(X.CASES)
    for c in X.CASES:
        s = c.shape
        assert s.K % 32 == 0 and s.N % 4 == 0 and s.K <= 1088
        assert s.M <= 4100 and s.N <= 2056                     # the largest case is 4100 x 2056 x 1088
        assert set(dict(c.opts)) <= set(X.OPTION_DEFAULTS)
    for kernel, shape, _, tile in X.ROWS_CASES:
        assert kernel in (X.K128, X.K256, X.K512, X.K4W) and all(1 <= n <= shape.M for n in X.rows_counts(shape.M, tile))


@pytest.mark.parametrize("prob", PROBLEMS, ids=_pid)
def test_reference_is_exact(prob):
    shape, gelu, eps = prob
    o, acc64, acc32 = _problem(shape, gelu)
    unit = 128.0 if gelu else 2.0                      # every intermediate is a multiple of 1 / unit (alpha = 0.5 halves the 1/64 and the 1)
    # operands: exact in bf16, in the stated ranges, and not degenerate
    for t in (o.a, o.b, o.bias, o.residual, o.aux_in):
        assert torch.equal(t.to(torch.bfloat16).float(), t) or t is o.bias       # bias stays fp32
    s = 8.0 if gelu else 1.0
    assert float(o.a.abs().max()) * s <= 3 and float(o.b.abs().max()) * s <= 2
    big = o.aux_in.numel() >= 1024            # (1, 4, 32) is too small to hold every value
    if gelu:
        assert float(o.bias.abs().max()) <= 4 and torch.equal(o.bias * 8, (o.bias * 8).round())
        assert float(o.aux_in.abs().max()) <= 6
    else:
        assert float(o.bias.abs().max()) <= 16 and float(o.residual.abs().max()) <= 8 and float(o.aux_in.abs().max()) <= 3
        assert not big or bool((o.aux_in == 0).any()) and bool((o.aux_in > 0).any()) and bool((o.aux_in < 0).any())     # zeros: `>` against `>=`
    if shape.M > 1 and not shape.grouped:
        assert not torch.equal(o.a[0], o.a[1]) and not torch.equal(o.b[0, 0], o.b[0, 1])       # rows distinct: a shifted read shows
    if shape.grouped:
        assert o.amap.unique().numel() == shape.M and o.cmap.unique().numel() == shape.M
        assert int(o.tiles[:, 1].max()) < shape.M and len(o.tiles) == sum(-(-c // shape.tile_rows) for c in shape.counts)
    # the fp32 accumulation is exact: the float32 CPU matmul equals the float64 one
    assert torch.equal(acc32.double(), acc64)
    for ep in eps:
        e = X.EPIS[ep]
        assert e.gelu == gelu
        c, aux, z, scale, exact = X.reference(o, e, acc64)
        if e.gelu:
            assert float(z.abs().max()) <= X.GELU_RANGE, (ep, float(z.abs().max()))      # inside the range the emulation covers
        for m in exact:
            assert torch.equal(m * unit, (m * unit).round()), ep
            assert float((m * unit).abs().max()) < 2 ** 24, ep
            assert torch.equal(m.float().double(), m), ep
        if not e.gelu:
            # one rounding: the float32 step in front of the bf16 one loses nothing
            assert torch.equal(c.float().double(), c), ep
            if not e.f32:
                b = X.to_bf16_once(c)
                assert float((b.double() - c).abs().max()) <= float((X.HALF_ULP_BF16 * c.abs()).max())
                assert bool(((b.double() - c).abs() <= X.HALF_ULP_BF16 * c.abs()).all()), ep
        elif e.epi == X.EPI_GELU and e.aux == "out":
            assert torch.equal(aux.float().double(), aux), ep               # the stored pre-activation: one rounding to bf16


def test_gelu_emulation_within_the_floor():
    """common.h's half_tail2 / gauss2 / cdf2 in float32 against float64 erf over [-12, 12]: the deviation the floor of the GPU test is
    built on (4.3e-7 GELU, 3.0e-7 GELU', 1.35e-7 in excess of the bf16 half-ulp after rounding), and the floor has its factor over it."""
    x = np.concatenate([np.linspace(-12, 12, 1_200_001), np.arange(-12 * 64, 12 * 64 + 1) / 64.0]).astype(np.float32)
    gl, dg = X.emulate_gelu_f32(x)
    xt = torch.from_numpy(x).double()
    gref, dref = X.gelu64(xt), X.dgelu64(xt)
    gdev = float((torch.from_numpy(gl).double() - gref).abs().max())
    ddev = float((torch.from_numpy(dg).double() - dref).abs().max())
    print(f"[bar] fp32 emulation of the GELU polynomial over [-12, 12]: GELU {gdev:.3g} (<= {X.GELU_EMU_DEV}), GELU' {ddev:.3g} (<= {X.DGELU_EMU_DEV})")
    assert gdev <= X.GELU_EMU_DEV and ddev <= X.DGELU_EMU_DEV
    worst = 0.0
    for got, ref in ((gl, gref), (dg, dref)):
        b = torch.from_numpy(got).to(torch.bfloat16)
        worst = max(worst, float(X.gelu_excess(b, ref).max()))
    print(f"[bar] ... after the bf16 rounding, in excess of 2^-8 |ref|: {worst:.3g} (<= {X.GELU_EMU_EXCESS}); floor {X.GELU_FLOOR}")
    assert worst <= X.GELU_EMU_EXCESS
    assert X.GELU_FLOOR >= 4 * X.GELU_EMU_DEV and X.GELU_FLOOR <= 5 * X.GELU_EMU_DEV


def test_mismatch_report_names_the_elements():
    bad = torch.zeros(8, 8, dtype=torch.bool)
    bad[2, 3] = bad[5, 7] = True
    s = X.describe_mismatch(bad)
    assert "2 of 64" in s and "rows 2..5" in s and "columns 3..7" in s and "(2, 3)" in s
