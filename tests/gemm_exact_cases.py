"""Operands, references and the case table of the exact NT GEMM tests (test_gemm_nt_exact_gpu.py runs them on the GPU,
test_gemm_nt_exact_host.py checks on the CPU that every reference here is itself exact).  Plain module, no GPU needed to import it.

Integer data: A in {-3..3}, B in {-2..2}, bias in {-16..16}, residual in {-8..8}, aux in {-3..3}, alpha in {1, 0.5}.  With K <= 1088 every
intermediate of the epilogue is an integer or a half-integer below 2^24, so an fp32 accumulation is exact in any order and the float64
reference is THE result, not an approximation of it.  GELU data: the same A and B divided by 8 (products are multiples of 1/64), bias and
residual multiples of 1/8 in [-4, 4], the aux input of EPI_MUL_DGELU a multiple of 1/16 in [-6, 6]: the pre-activation is exact, the
activation is compared per element against float64 erf.  Everything comes from a CPU torch.Generator seeded by the shape: random, not
periodic in the row or the column, so a transposed or shifted read shows."""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

EPI_NONE, EPI_GELU, EPI_RELU, EPI_MUL_DGELU, EPI_MUL_DRELU, EPI_GELU_DAUX, EPI_MUL_AUX = range(7)

# medmoe_last_gemm_nt_kernel ids
K128, K256, K512, K512G, K4W, K4WG, KDIRECT = range(7)
# medmoe_set_option keys that pick the NT kernel, with their defaults
OPT_NT256, OPT_NT512, OPT_NT_GRID, OPT_NT4W, OPT_NT_DIRECT = 1, 2, 5, 7, 17
OPTION_DEFAULTS = {OPT_NT256: 1, OPT_NT512: 1, OPT_NT_GRID: 256, OPT_NT4W: 1, OPT_NT_DIRECT: 1}

HALF_ULP_BF16 = 2.0 ** -8
# the A&S 7.1.26 polynomial of common.h in fp32 deviates from float64 by 4.3e-7 (GELU) / 3.0e-7 (GELU') over [-12, 12]
# (test_gemm_nt_exact_host.py measures it); x 4 for the hardware rcp and exp2 (about one ulp each, not emulated), rounded up
GELU_FLOOR = 2e-6
# after the bf16 rounding the emulation exceeds 2^-8 |ref| by 1.35e-7 on the grid the host file samples
GELU_EMU_DEV, DGELU_EMU_DEV, GELU_EMU_EXCESS = 4.3e-7, 3.0e-7, 1.4e-7
GELU_RANGE = 12.0


@dataclass(frozen=True)
class Epi:
    """One epilogue form of medmoe_gemm_nt.  aux: None, "out" (EPI_GELU / EPI_GELU_DAUX store it) or "in" (the MUL_* factor)."""
    epi: int = EPI_NONE
    bias: bool = False
    residual: bool = False
    aux: Optional[str] = None
    f32: bool = False
    alpha: float = 1.0
    inplace: bool = False      # residual IS the output tensor
    gelu: bool = False         # GELU data (operands / 8), compared against float64 erf within the floor


EPIS = {
    "plain": Epi(),
    "f32": Epi(f32=True),
    "bias": Epi(bias=True),
    "bias_res": Epi(bias=True, residual=True),
    "res": Epi(residual=True),
    "gelu_aux": Epi(EPI_GELU, bias=True, aux="out", gelu=True),
    "gelu": Epi(EPI_GELU, bias=True, gelu=True),
    "gelu_daux": Epi(EPI_GELU_DAUX, bias=True, aux="out", gelu=True),
    "mul_dgelu": Epi(EPI_MUL_DGELU, aux="in", gelu=True),
    "mul_aux": Epi(EPI_MUL_AUX, aux="in"),
    # the grouped tables
    "relu_bias": Epi(EPI_RELU, bias=True),
    "mul_drelu_res": Epi(EPI_MUL_DRELU, residual=True, aux="in"),
    # no specialised build takes these: SPEC = -1
    "relu_bias_res": Epi(EPI_RELU, bias=True, residual=True),
    "alpha_half": Epi(bias=True, alpha=0.5),
    "f32_bias": Epi(bias=True, f32=True),
    "mul_dgelu_res_half": Epi(EPI_MUL_DGELU, residual=True, aux="in", alpha=0.5, gelu=True),
    # residual is out
    "bias_res_inplace": Epi(bias=True, residual=True, inplace=True),
    "res_inplace": Epi(residual=True, inplace=True),
}

SPECIALISED = ("plain", "f32", "bias", "bias_res", "res", "gelu_aux", "gelu", "gelu_daux", "mul_dgelu", "mul_aux")
GENERIC = ("relu_bias_res", "alpha_half", "f32_bias")
GROUP_TABLE = ("plain", "relu_bias", "mul_drelu_res", "res", "res_inplace")


@dataclass(frozen=True)
class Shape:
    """Plain: counts = (M,).  Grouped: ragged groups, A gathered from `src_rows` rows, C scattered over `dst_rows` rows."""
    N: int
    K: int
    counts: Tuple[int, ...]
    tile_rows: int = 0         # 0 plain, 128 / 256 grouped on that tile table
    src_rows: int = 0
    dst_rows: int = 0

    @property
    def M(self):
        return sum(self.counts)

    @property
    def grouped(self):
        return self.tile_rows != 0


def plain(M, N, K):
    return Shape(N, K, (M,))


@dataclass(frozen=True)
class Case:
    kernel: int
    shape: Shape
    ep: str
    opts: Tuple[Tuple[int, int], ...] = ()

    @property
    def id(self):
        s = self.shape
        o = "".join(f"-o{k}={v}" for k, v in self.opts)
        g = f"g{s.tile_rows}-" if s.grouped else ""
        return f"k{self.kernel}-{g}{s.M}x{s.N}x{s.K}-{self.ep}{o}"


def _cases():
    out = []

    def add(kernel, shape, eps, opts=()):
        for ep in eps:
            out.append(Case(kernel, shape, ep, tuple(opts)))

    everything = SPECIALISED + GENERIC + ("mul_dgelu_res_half", "bias_res_inplace")
    # --- 0: the 128x128 kernel (one build, every option at run time): M < 1024
    add(K128, plain(1, 4, 32), ("plain", "f32", "bias_res", "gelu_aux"))
    add(K128, plain(130, 132, 32), everything)                      # N % 8 == 4: narrow stores; half k-step
    add(K128, plain(257, 136, 96), everything)                      # paired stores; one and a half k-steps
    add(K128, plain(129, 264, 64), ("plain", "bias_res", "mul_aux", "gelu_daux", "f32_bias"))
    add(K128, plain(300, 128, 1088), ("plain", "f32", "bias_res", "alpha_half", "mul_aux"))
    # several tiles per workgroup: 33 x 17 tiles on a grid of 512
    add(K128, plain(4100, 2052, 64), ("plain", "bias_res_inplace", "relu_bias_res", "gelu_aux"), [(OPT_NT256, 0)])
    # --- 1: nt256
    add(K256, plain(1027, 136, 192), everything)
    add(K256, plain(1283, 132, 320), ("plain", "bias_res", "f32_bias", "gelu_aux", "mul_aux"))       # N % 8 == 4: the generic build
    # 17 x 17 tiles on a grid of 256: the parked stores of one tile leave under the next one
    add(K256, plain(4100, 2056, 192), ("plain", "bias", "bias_res", "res", "gelu_aux", "gelu", "gelu_daux", "mul_dgelu", "mul_aux",
                                       "relu_bias_res", "bias_res_inplace"), [(OPT_NT512, 0)])
    # --- 4 and 2: the 256x256 tile, four waves (default) and eight (option 7 = 0); the generic build exists on nt512 only
    for kernel, o in ((K4W, []), (K512, [(OPT_NT4W, 0)])):
        gen = (GENERIC + ("mul_dgelu_res_half",)) if kernel == K512 else ()
        add(kernel, plain(1027, 520, 128), SPECIALISED + ("bias_res_inplace",) + gen, o)
        add(kernel, plain(1283, 1048, 128), ("plain", "bias_res", "gelu_daux", "mul_aux") + gen[:1], o)
        for K in (192, 320, 1088):
            add(kernel, plain(4100, 2056, K), ("plain", "bias_res", "mul_aux") + (("gelu_aux", "gelu_daux", "res") if K == 192 else ()), o)
        # tile seam: a grid of 3, every workgroup walks five or more tiles
        seam = o + [(OPT_NT_GRID, 3)]
        add(kernel, plain(1027, 520, 128), SPECIALISED + ("bias_res_inplace",) + gen[:1], seam)
        add(kernel, plain(1283, 1048, 128), ("plain", "bias_res", "gelu_aux", "mul_aux"), seam)
        add(kernel, plain(4100, 2056, 192), ("bias_res", "gelu_daux"), seam)
        add(kernel, plain(4100, 2056, 1088), ("plain",), seam)
    # --- 6: direct (K % 64 == 32, M >= 4096)
    add(KDIRECT, plain(4100, 100, 96), ("plain", "bias_res", "f32", "gelu_aux", "mul_aux"))           # N % 8 == 4
    add(KDIRECT, plain(4100, 132, 32), ("plain", "bias", "relu_bias_res", "alpha_half", "gelu_daux"))
    add(KDIRECT, plain(4099, 288, 288), everything)
    # --- 5 and 3: grouped, gathered A, scattered C on the 256-row tile table
    for K in (128, 192):
        g = Shape(320, K, (700, 0, 1, 257, 390), 256, 2000, 1500)
        add(K4WG, g, GROUP_TABLE)
        add(K512G, g, GROUP_TABLE + ("bias_res",), [(OPT_NT4W, 0)])
    # --- 0 grouped: the 128-row tile table
    add(K128, Shape(132, 64, (130, 0, 1, 77), 128, 500, 400), GROUP_TABLE + ("bias", "f32_bias", "alpha_half"))
    return out


CASES = _cases()

# gemm_nt_rows: (kernel, shape, options); the counts on the device are 1, tile - 1, tile, tile + 1, M
ROWS_CASES = [
    (K128, plain(257, 136, 96), (), 128),
    (K256, plain(1027, 136, 192), (), 256),
    (K4W, plain(1027, 520, 128), (), 256),
    (K512, plain(1027, 520, 128), ((OPT_NT4W, 0),), 256),
]
ROWS_EPIS = ("bias_res", "f32", "gelu_aux")


def rows_counts(M, tile):
    return (1, tile - 1, tile, tile + 1, M)


# ------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------
@dataclass
class Operands:
    """CPU fp32 tensors, every value exact in bf16.  Row r of the product (packed order, group after group) reads src row amap[r] and
    lands in destination row cmap[r]; plain shapes have identity maps (None)."""
    shape: Shape
    gelu: bool
    a: torch.Tensor                 # [src_rows, K]
    b: torch.Tensor                 # [G, N, K]
    bias: torch.Tensor              # [G, N]
    residual: torch.Tensor          # [dst_rows, N]
    aux_in: torch.Tensor            # [dst_rows, N]
    amap: Optional[torch.Tensor]    # [M] int32
    cmap: Optional[torch.Tensor]
    group_of_row: torch.Tensor      # [M] int64
    tiles: Optional[torch.Tensor] = None    # [T, 4] int32: group, first row, end row of the group, 0


def _seed(shape: Shape, gelu: bool):
    return (shape.M * 1000003 + shape.N * 1009 + shape.K * 7 + len(shape.counts) * 131 + (1 if gelu else 0)) % (2 ** 31 - 1)


def make_operands(shape: Shape, gelu: bool) -> Operands:
    g = torch.Generator(device="cpu")
    g.manual_seed(_seed(shape, gelu))
    M, N, K, G = shape.M, shape.N, shape.K, len(shape.counts)
    S = shape.src_rows or M
    D = shape.dst_rows or M

    def ints(lo, hi, *size):
        return torch.randint(lo, hi + 1, size, generator=g).float()

    a, b = ints(-3, 3, S, K), ints(-2, 2, G, N, K)
    if gelu:
        a, b = a / 8, b / 8
        bias, residual, aux_in = ints(-32, 32, G, N) / 8, ints(-32, 32, D, N) / 8, ints(-96, 96, D, N) / 16
    else:
        bias, residual, aux_in = ints(-16, 16, G, N), ints(-8, 8, D, N), ints(-3, 3, D, N)
    amap = cmap = tiles = None
    if shape.grouped:
        amap = torch.randperm(S, generator=g)[:M].int()
        cmap = torch.randperm(D, generator=g)[:M].int()
        t, start = [], 0
        for gi, c in enumerate(shape.counts):
            for m in range(start, start + c, shape.tile_rows):
                t.append([gi, m, start + c, 0])
            start += c
        tiles = torch.tensor(t, dtype=torch.int32)
    group_of_row = torch.repeat_interleave(torch.arange(G), torch.tensor(shape.counts))
    return Operands(shape, gelu, a, b, bias, residual, aux_in, amap, cmap, group_of_row, tiles)


def to_device(o: Operands, device) -> Operands:
    mv = lambda t: None if t is None else t.to(device)
    return Operands(o.shape, o.gelu, mv(o.a), mv(o.b), mv(o.bias), mv(o.residual), mv(o.aux_in), mv(o.amap), mv(o.cmap), mv(o.group_of_row),
                    mv(o.tiles))


# ------------------------------------------------------------------------------------------------------------------
# references (any device, any dtype: float64 is the reference, float32 on the CPU is what the host file compares it with)
# ------------------------------------------------------------------------------------------------------------------
def accumulate(o: Operands, dtype=torch.float64) -> torch.Tensor:
    """A @ B^T of every packed row with its group's B: [M, N]."""
    a = o.a if o.amap is None else o.a[o.amap.long()]
    a, b = a.to(dtype), o.b.to(dtype)
    if len(o.shape.counts) == 1:
        return a[:o.shape.M] @ b[0].t()
    out, start = [], 0
    for gi, c in enumerate(o.shape.counts):
        out.append(a[start:start + c] @ b[gi].t())
        start += c
    return torch.cat(out)


def gelu64(z):
    return z * 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))


def dgelu64(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def dest_rows(o: Operands, rows=None):
    """Destination row of every packed row (int64), the first `rows` of them."""
    M = o.shape.M if rows is None else rows
    return torch.arange(M, device=o.a.device) if o.cmap is None else o.cmap.long()[:M]


def reference(o: Operands, e: Epi, acc: torch.Tensor, residual: Optional[torch.Tensor] = None):
    """float64, in the order of nt_epilogue: alpha * acc + bias, the activation, + residual, x the MUL_* factor.
    Returns (C, aux output or None, z, s, exact) for the packed rows of `acc`: z the pre-activation, s = max(1, |alpha acc + residual|)
    (the scale of the EPI_MUL_DGELU bar), `exact` the intermediates that fp32 must hold exactly (everything up to the first GELU or
    GELU').  `residual` overrides the operand's (the in-place form: a copy of the destination taken before the launch)."""
    rows = acc.shape[0]
    dr = dest_rows(o, rows)
    f64 = lambda t: t.to(torch.float64)
    z = e.alpha * f64(acc)
    exact = [f64(acc), z]
    if e.bias:
        z = z + f64(o.bias)[o.group_of_row[:rows]]
        exact.append(z)
    smooth = e.epi in (EPI_GELU, EPI_GELU_DAUX)        # from here on the values are no longer exact
    aux = None
    v = z
    if e.epi == EPI_GELU:
        aux, v = z, gelu64(z)
    elif e.epi == EPI_GELU_DAUX:
        aux, v = dgelu64(z), gelu64(z)
    elif e.epi == EPI_RELU:
        v = torch.relu(z)
    if e.residual:
        v = v + f64(o.residual if residual is None else residual)[dr]
        if not smooth:
            exact.append(v)
    scale = v.abs().clamp_min(1.0)
    if e.epi == EPI_MUL_DGELU:
        v = v * dgelu64(f64(o.aux_in)[dr])
    elif e.epi == EPI_MUL_DRELU:
        v = v * (f64(o.aux_in)[dr] > 0).to(torch.float64)
    elif e.epi == EPI_MUL_AUX:
        v = v * f64(o.aux_in)[dr]
    if not smooth and e.epi != EPI_MUL_DGELU:
        exact.append(v)
    return v, (aux if e.aux == "out" else None), z, scale, exact


def to_bf16_once(ref64: torch.Tensor) -> torch.Tensor:
    """The bf16 expectation: the float32 step is lossless for this data (the host file asserts it), so this is ONE round-to-nearest-even,
    which is what pack2bf does."""
    return ref64.float().to(torch.bfloat16)


def gelu_excess(got: torch.Tensor, ref64: torch.Tensor, scale=None) -> torch.Tensor:
    """Per element: (|got - ref| - 2^-8 |ref|) / s, to be held against GELU_FLOOR."""
    ex = (got.to(torch.float64) - ref64).abs() - HALF_ULP_BF16 * ref64.abs()
    return ex if scale is None else ex / scale


def describe_mismatch(bad: torch.Tensor, got=None, exp=None, limit=6) -> str:
    """Which elements: count, the bounding box, the first few coordinates (with values)."""
    idx = bad.nonzero()
    if idx.numel() == 0:
        return "no mismatch"
    r, c = idx[:, 0], idx[:, 1]
    s = f"{idx.shape[0]} of {bad.numel()} elements wrong, rows {int(r.min())}..{int(r.max())}, columns {int(c.min())}..{int(c.max())}; first:"
    for i in range(min(limit, idx.shape[0])):
        ri, ci = int(r[i]), int(c[i])
        s += f" ({ri}, {ci})"
        if got is not None and exp is not None:
            s += f" got {float(got[ri, ci]):.6g} want {float(exp[ri, ci]):.6g};"
    return s


# ------------------------------------------------------------------------------------------------------------------
# float32 emulation of common.h's half_tail2 / gauss2 / cdf2 (numpy, one rounding per operation; the hardware rcp and exp2
# are replaced by correctly rounded ones)
# ------------------------------------------------------------------------------------------------------------------
def emulate_gelu_f32(x):
    """x: numpy float32 array.  Returns (GELU, GELU') as float32, the arithmetic of gelu_and_grad2."""
    import numpy as np
    f = np.float32
    ax = np.abs(x).astype(f)
    a2 = (ax * ax).astype(f) * f(-0.5 * 1.4426950408889634)
    e = np.exp2(a2.astype(np.float64)).astype(f)
    d = f(1.0) + f(0.3275911 * 0.70710678118654752) * ax
    t = (1.0 / d.astype(np.float64)).astype(f)
    p = f(0.5 * 1.061405429) * t - f(0.5 * 1.453152027)
    p = p * t + f(0.5 * 1.421413741)
    p = p * t - f(0.5 * 0.284496736)
    p = p * t + f(0.5 * 0.254829592)
    h = p * t * e
    u = f(1.0) - h
    cdf = np.where(x >= 0, u, h).astype(f)
    gl = x * cdf
    dg = cdf + x * (f(0.39894228040143268) * e)
    return gl.astype(f), dg.astype(f)
