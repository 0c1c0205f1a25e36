"""Operands, references, case tables and the comparison routine of the exact tests of the two grouped expert GEMMs
(medmoe_gemm_fp8_grouped in csrc/fp8.hip, medmoe_gemm_mx_grouped in csrc/mxfp8.hip).  test_expert_gemm_exact_gpu.py runs the cases on
the GPU, test_expert_gemm_exact_host.py proves on the CPU that every reference here is itself exact.  Plain module: no GPU to import it,
and everything in it is computed on the CPU (a flush-to-zero of a device kernel cannot leak into an expectation).

Data (the construction of test_mxfp8_gpu.py::test_gemm_mx_layout_pin): A integers in [-4, 4], B integers in [-3, 3], from a CPU
torch.Generator seeded by the shape.  MX scale bytes 127 + off + j with j = -2..2 over (row, 32-block) of A and -1..1 over (group,
column, 32-block) of B, neighbours always different, and a per-case power-of-two offset `off` in {0, -20, +12} for each operand.  fp8
scales 2^j, j = -3..3 per row of A and per column of B.  Bias a multiple of 1/8 in [-16, 16], residual an integer in [-8, 8], aux an
integer in [-3, 3] (zeros included: `aux > 0` is strict).  For K <= 1024 every partial sum is a multiple of 2^(off - 3) below
2^(off + 15): exact in fp32 in any order, so the float64 result is THE result and the criterion is bit equality of every bf16 element
after one round-to-nearest-even.  A case that adds a bias or a residual keeps offA + offB in {0, -8}, so that the sum stays inside 24
bits (the host test proves it per case).

Launch forms.  Every buffer that a tile entry can reach has a GUARD BAND of 128 more rows [M, M + 128) filled with valid non-zero
operands.  `guard`: three more tile entries past tile_count[0] that describe rows of the band (max_tiles > count, as the engine always
launches); a kernel that ignored the count would write there, in bounds.  `ldc`: ldc = N + 12, the pad columns keep their prefill
(residual and aux share ldc, as in the kernels).  `eng`: both.  `count0`: tile_count[0] = 0.  `shuf`: the tile table shuffled."""
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from test_mxfp8_host import mx_dequant, mx_quant  # noqa: F401  (re-exported: the GPU file takes the twin from here)

F8 = torch.float8_e4m3fn
U8 = torch.uint8
GUARD = 128
LDC_PAD = 12
PAT_C = 0x7FC1           # a bf16 NaN: no result is ever NaN, compared as int16
PAT_Q, PAT_S = 0xAB, 0xCD
EPI_NONE, EPI_RELU, EPI_MUL_DRELU = 0, 1, 2


@dataclass(frozen=True)
class Epi:
    epi: int = EPI_NONE
    bias: bool = False
    residual: bool = False
    inplace: bool = False      # residual IS the output tensor


EPIS = {
    "none": Epi(),
    "bias": Epi(bias=True),
    "bias_relu": Epi(EPI_RELU, bias=True),
    "relu": Epi(EPI_RELU),
    "drelu_res": Epi(EPI_MUL_DRELU, residual=True),
    "drelu": Epi(EPI_MUL_DRELU),
    "drelu_inplace": Epi(EPI_MUL_DRELU, residual=True, inplace=True),
}

# sizes 1, 16, 17, 127, 128, 129 and an empty group, unaligned m0 | a two-tile group ending one row into its second tile |
# the first group empty | a single group
GROUPS = {"rag7": (1, 0, 129, 127, 128, 17, 16), "two": (3, 129), "e0": (0, 70, 33), "one": (77,),
          "two_big": (129, 0, 131)}        # the last one for the one-hot A only: 260 rows >= K = 256 reach every k
LAUNCHES = ("tight", "ldc", "guard", "eng", "count0", "shuf")
# 4: one quad, below a 16-column subtile | 60 | 128: the tile | 132: a second column tile 4 columns wide | 200
NS = (4, 60, 128, 132, 200)
# MX: K / 32 % 4 = 1, 2, 3, 0, 1, 3, 0, 0, 0; 1, 1, 1, 1, 2, 2, 2, 3 and 8 k-steps (3: the first reuse of ring slot 0)
MX_KS = (32, 64, 96, 128, 160, 224, 256, 384, 1024)
F8_KS = (64, 128, 192, 1024)                  # 1, 2, 3 and 16 k-steps of 64
OFFS_FREE = tuple((a, b) for a in (0, -20, 12) for b in (0, -20, 12))
OFFS_SUM = ((0, 0), (-20, 12), (12, -20))     # with a bias or a residual: the sum must stay inside 24 bits


@dataclass(frozen=True)
class Case:
    kernel: str                # "mx" | "fp8"
    K: int
    N: int
    groups: str
    ep: str
    launch: str
    offs: Tuple[int, int] = (0, 0)     # MX: global exponent offsets of A's and B's scale bytes
    sb_none: bool = False              # fp8: sb == nullptr, strideSb = 0 (the dgrad form)
    quant: str = ""                    # MX, bias_relu: the fused quantised output; "neg" / "pow2" / "neg+pow2" / "plain" / "tiny"
    data: str = "int"                  # "int" | "onehotA" (one-hot A, every code in B) | "onehotB" | "rand" (fp8, non-power-of-two scales)
    why: str = ""                      # the mechanism the case is there for

    @property
    def counts(self):
        return GROUPS[self.groups]

    @property
    def id(self):
        s = f"{self.kernel}-K{self.K}-N{self.N}-{self.groups}-{self.ep}-{self.launch}"
        if self.kernel == "mx":
            s += f"-a{self.offs[0]:+d}b{self.offs[1]:+d}"
        if self.sb_none:
            s += "-nosb"
        if self.quant:
            s += "-q_" + self.quant
        if self.data != "int":
            s += "-" + self.data
        return s

    @property
    def problem_key(self):
        return (self.kernel, self.K, self.N, self.groups, self.offs, self.sb_none, self.quant, self.data)


def _grid(kernel, ks):
    """Every K meets every epilogue once; N, group set, launch form and offsets rotate so that every N and every group set meets the
    narrowest and the widest K (the host file asserts the coverage)."""
    out = []
    eps = list(EPIS)
    gs = list(GROUPS)[:4]
    for ki, K in enumerate(ks):
        for ei, ep in enumerate(eps):
            e = EPIS[ep]
            N = NS[(ki + ei) % 5]
            groups = gs[(2 * ki + ei) % 4]
            launch = LAUNCHES[(ki + 2 * ei + ei // 2) % 4]
            if kernel == "mx":
                offs = OFFS_SUM[(ki + ei) % 3] if (e.bias or e.residual) else OFFS_FREE[(2 * ki + ei) % 9]
                nk, res = -(-K // 128), K // 32 % 4
                why = f"{nk} k-step(s), K/32 % 4 = {res}" + (": K tail (z0 / z1, scale 127, piece 0 re-read)" if res else "")
            else:
                offs = (0, 0)
                why = f"{K // 64} k-step(s) of 64"
            sb_none = kernel == "fp8" and e.epi == EPI_MUL_DRELU and ei != 5
            why += f"; N = {N}, groups {groups}, epilogue {ep}, launch {launch}"
            out.append(Case(kernel, K, N, groups, ep, launch, offs, sb_none, why=why))
    return out


def _cases():
    out = _grid("mx", MX_KS) + _grid("fp8", F8_KS)
    for kernel, ks in (("mx", (96, 384)), ("fp8", (64, 192))):
        for K in ks:
            out.append(Case(kernel, K, 132, "rag7", "bias_relu", "count0", why="tile_count[0] = 0: nothing is written"))
            out.append(Case(kernel, K, 132, "rag7", "drelu_res", "shuf", why="the tile table in shuffled order: the same bits"))
    # the fused quantised output of the MX ReLU epilogue, over the ragged group set: below / across a 64-column wave / across the tile
    for N, q, K in ((32, "plain", 1024), (96, "neg+pow2", 128), (160, "neg", 96), (192, "pow2", 32)):
        out.append(Case("mx", K, N, "rag7", "bias_relu", "eng", quant=q,
                        why=f"Cq / Csq = mx_quant of the EXPECTED C at N = {N}; {q}: a block of zeros (bias -1e3, byte 127) / amax = 448 * 2^-3"))
    out.append(Case("mx", 64, 64, "rag7", "bias_relu", "eng", quant="tiny",
                    why="the tiny / huge blocks of the row quantiser through the fused output: amax / 448 an fp32 subnormal (byte 1), bf16-subnormal C, 3.0e38"))
    # e4m3 decode through the MFMA: one product per output
    for kernel in ("mx", "fp8"):
        out.append(Case(kernel, 256, 64, "two_big", "none", "eng", (0, 0), data="onehotA",
                        why="A one-hot at k = m mod K, B holds all 254 finite e4m3 codes: the output is the dequantised code"))
        out.append(Case(kernel, 256, 256, "e0", "none", "eng", (0, 0), data="onehotB", why="the mirror image: the codes in A"))
    return out


CASES = _cases()
# fp8 with the non-power-of-two scales of test_fp8_gpu.py on the integer data: all epilogues, a derived bar
RAND_CASES = [Case("fp8", K, 200, "rag7", ep, "eng", sb_none=(ep == "drelu"), data="rand", why="random fp32 sa / sb / bias: two scale roundings, one add, one bf16 rounding")
              for K, eps in ((192, tuple(EPIS)), (1024, ("bias_relu", "drelu_res"))) for ep in eps]


# ------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------
CODES = torch.tensor([c for c in range(256) if c not in (0x7F, 0xFF)], dtype=U8)      # the 254 finite e4m3 codes


@dataclass
class Problem:
    """CPU tensors.  R = M + GUARD rows everywhere a tile entry can reach."""
    kernel: str
    N: int
    K: int
    counts: Tuple[int, ...]
    aq: torch.Tensor                   # [R, K] e4m3 bytes
    bq: torch.Tensor                   # [G, N, K]
    sa: torch.Tensor                   # mx: [R, K/32] bytes; fp8: [R] fp32
    sb: Optional[torch.Tensor]         # mx: [G, N, K/32]; fp8: [G, N] or None
    bias: torch.Tensor                 # [G, N] fp32
    residual: torch.Tensor             # [R, N] fp32, exact in bf16
    aux: torch.Tensor                  # [R, N]

    @property
    def M(self):
        return sum(self.counts)

    @property
    def R(self):
        return self.M + GUARD

    @property
    def G(self):
        return len(self.counts)

    @property
    def a(self):
        return self.aq.view(F8).float()

    @property
    def b(self):
        return self.bq.view(F8).float()

    @property
    def group_of_row(self):
        return torch.repeat_interleave(torch.arange(self.G), torch.tensor(self.counts))


def _seed(c: Case):
    return (sum(c.counts) * 1000003 + c.N * 1009 + c.K * 7 + len(c.counts) * 131 + (17 if c.kernel == "mx" else 0)
            + {"int": 0, "onehotA": 1, "onehotB": 2, "rand": 3}[c.data]) % (2 ** 31 - 1)


def make_problem(c: Case) -> Problem:
    g = torch.Generator(device="cpu")
    g.manual_seed(_seed(c))
    N, K, counts = c.N, c.K, c.counts
    M, G = sum(counts), len(counts)
    R = M + GUARD

    def ints(lo, hi, *size):
        return torch.randint(lo, hi + 1, size, generator=g).float()

    a, b = ints(-4, 4, R, K), ints(-3, 3, G, N, K)
    bias, residual, aux = ints(-128, 128, G, N) / 8, ints(-8, 8, R, N), ints(-3, 3, R, N)
    if "pow2" in c.quant:                # block 0 of every row: the product is zero, the bias tops out at exactly 448 * 2^-3
        b[:, :32] = 0
        bias[:, :32] = ints(-16, 16, G, 32) / 8
        bias[:, 5] = 56.0
    if c.quant == "tiny":                # block 0: the product is zero and group g's bias is row g % 6 of tiny_rows(): C = relu(bias) exactly
        b[:, :32] = 0
        bias[:, :32] = tiny_rows()[torch.arange(G) % 6, :32]
    if "neg" in c.quant:                 # the last 32-block: ReLU turns it into zeros
        bias[:, N - 32:] = -1e3
    aq, bq = a.to(F8).view(U8), b.to(F8).view(U8)
    if c.data == "onehotA":
        aq = torch.zeros(R, K, dtype=U8)
        aq[torch.arange(R), torch.arange(R) % K] = 0x38                    # 1.0
        n_i, k_i, g_i = torch.arange(N)[None, :, None], torch.arange(K)[None, None, :], torch.arange(G)[:, None, None]
        bq = CODES[(k_i + 37 * n_i + 101 * g_i) % 254]
    elif c.data == "onehotB":
        bq = torch.zeros(G, N, K, dtype=U8)
        bq[:, torch.arange(N), torch.arange(N) % K] = 0x38
        aq = CODES[(torch.arange(K)[None, :] + 37 * torch.arange(R)[:, None]) % 254]
    m_i = torch.arange(R)[:, None]
    if c.kernel == "mx":
        kb = torch.arange(K // 32)
        ja = (m_i * 3 + kb[None, :] * 2) % 5 - 2
        jb = (torch.arange(N)[None, :, None] * 2 + kb[None, None, :] + torch.arange(G)[:, None, None]) % 3 - 1
        sa, sb = (127 + c.offs[0] + ja).to(U8), (127 + c.offs[1] + jb).to(U8).contiguous()
    elif c.data == "rand":               # the scales and bias of test_fp8_gpu.py::test_gemm_fp8_grouped
        sa = torch.rand(R, generator=g) * 0.01 + 1e-3
        sb = torch.rand(G, N, generator=g) * 0.01 + 1e-3
        bias = torch.randn(G, N, generator=g) * 0.1
        residual = (torch.randn(R, N, generator=g) * 0.01).to(torch.bfloat16).float()    # the size of the product term
    else:
        sa = torch.pow(2.0, torch.randint(-3, 4, (R,), generator=g).float())
        sb = torch.pow(2.0, torch.randint(-3, 4, (G, N), generator=g).float())
    if c.kernel == "fp8" and c.sb_none:
        sb = None
    return Problem(c.kernel, N, K, counts, aq, bq, sa, sb, bias, residual, aux)


def tile_table(counts, launch: str):
    """([T, 4] int32 table, count): T > count for the `guard` / `eng` forms (three entries inside the guard band follow)."""
    t, start = [], 0
    for gi, c in enumerate(counts):
        for m in range(start, start + c, 128):
            t.append([gi, m, start + c, 0])
        start += c
    n = len(t)
    if launch == "shuf":
        t = t[::-1]                       # last tile first, then (three or more) the middle ones interleaved
        t = t[:1] + t[2::2] + t[1::2]
    if launch in ("guard", "eng"):
        M, G = start, len(counts)
        t += [[G - 1, M, M + GUARD, 0], [0, M + 5, M + 77, 0], [min(1, G - 1), M + 64, M + GUARD, 0]]
    return torch.tensor(t, dtype=torch.int32).reshape(-1, 4), (0 if launch == "count0" else n)


def ldc_of(c: Case):
    return c.N + (LDC_PAD if c.launch in ("ldc", "eng") else 0)


# ------------------------------------------------------------------------------------------------------------------
# references: float64 is the reference; float32 on the CPU is what the host file compares it with
# ------------------------------------------------------------------------------------------------------------------
def dequant_a(p: Problem, dtype=torch.float64, aq=None, sa=None):
    """What the MFMA multiplies: the MX block scales are applied inside the product, the fp8 scales after it (epilogue)."""
    aq, sa = p.aq if aq is None else aq, p.sa if sa is None else sa
    return (mx_dequant(aq, sa) if p.kernel == "mx" else aq.view(F8).float()).to(dtype)


def dequant_b(p: Problem, dtype=torch.float64):
    return (mx_dequant(p.bq, p.sb) if p.kernel == "mx" else p.bq.view(F8).float()).to(dtype)


def accumulate(p: Problem, dtype=torch.float64, a=None, rows=None, flip=False):
    """S = A @ B[group]^T of the rows [lo, hi) (default: all M).  flip: the other summation order."""
    a = dequant_a(p, dtype) if a is None else a.to(dtype)
    b = dequant_b(p, dtype)
    if flip:
        a, b = a.flip(-1), b.flip(-1)
    lo, hi = (0, p.M) if rows is None else rows
    out, start = [], 0
    for gi, c in enumerate(p.counts):
        l, h = max(lo, start), min(hi, start + c)
        if h > l:
            out.append(a[l:h] @ b[gi].t())
        start += c
    return torch.cat(out) + 0.0          # + 0.0: a sum of signed zeros is +0, as an accumulator that starts at +0 gives


def epilogue(p: Problem, e: Epi, S, dtype=torch.float64, rows=None, residual=None):
    """In the kernels' order: (fp8: S * sa * sb) + bias, ReLU | (+ residual) * (aux > 0).  Returns (C, intermediates): the
    intermediates are what fp32 must hold exactly.  `residual` overrides the operand's (in place: a copy taken before the launch)."""
    lo, hi = (0, p.M) if rows is None else rows
    grp = p.group_of_row[lo:hi]
    v = S.to(dtype)
    inter = [v]
    if p.kernel == "fp8":
        v = v * p.sa[lo:hi, None].to(dtype)
        inter.append(v)
        if p.sb is not None:
            v = v * p.sb[grp].to(dtype)
            inter.append(v)
    if e.bias:
        v = v + p.bias[grp].to(dtype)
        inter.append(v)
    if e.epi == EPI_RELU:
        v = torch.relu(v)
    elif e.epi == EPI_MUL_DRELU:
        if e.residual:
            v = v + (p.residual if residual is None else residual)[lo:hi].to(dtype)
            inter.append(v)
        v = torch.where(p.aux[lo:hi] > 0, v, torch.zeros_like(v))
    return v + 0.0, inter


def to_bf16_once(ref64):
    """The float32 step is lossless for this data (the host file asserts it): ONE round-to-nearest-even, as pack2bf."""
    return ref64.float().to(torch.bfloat16)


def expected_c(p: Problem, c: Case, residual=None):
    return to_bf16_once(epilogue(p, EPIS[c.ep], accumulate(p), residual=residual)[0])


def rand_bar(p: Problem, e: Epi, S64, ref64):
    """The per-element bar of the non-power-of-two fp8 cases: two fp32 roundings for the scale products, one for the bias / residual
    add (fma or not), one bf16 rounding.  |got - ref| <= 2^-8 |ref| + 2^-22 (|S sa sb| + |bias| + |residual|)."""
    grp = p.group_of_row
    t = (S64 * p.sa[:p.M, None].double() * (p.sb[grp].double() if p.sb is not None else 1.0)).abs()
    if e.bias:
        t = t + p.bias[grp].double().abs()
    if e.residual:
        t = t + p.residual[:p.M].double().abs()
    return 2.0 ** -8 * ref64.abs() + 2.0 ** -22 * t


# ------------------------------------------------------------------------------------------------------------------
# the comparison routine of the GPU test (the host file shows that it rejects corrupted references)
# ------------------------------------------------------------------------------------------------------------------
def bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def describe_mismatch(bad, got=None, exp=None, limit=6):
    idx = bad.nonzero()
    if idx.numel() == 0:
        return "no mismatch"
    r, c = idx[:, 0], idx[:, 1]
    s = f"{idx.shape[0]} of {bad.numel()} elements wrong, rows {int(r.min())}..{int(r.max())}, columns {int(c.min())}..{int(c.max())}; first:"
    for i in range(min(limit, idx.shape[0])):
        ri, ci = int(r[i]), int(c[i])
        s += f" ({ri}, {ci})"
        if got is not None and exp is not None:
            s += f" got {float(got[ri, ci]):.9g} want {float(exp[ri, ci]):.9g};"
    return s


def check_buffer(got, before, exp, M, N, what):
    """`got` (the whole buffer after the launch, guard rows and pad columns included) must hold `exp` bit for bit in [:M, :N] and be
    bit-identical to `before` (its image before the launch) everywhere else.  exp None: nothing may be written at all."""
    got, before = got.cpu(), before.cpu()
    assert got.shape == before.shape and got.dtype == before.dtype
    want = before.clone()
    if exp is not None:
        assert tuple(exp.shape) == (M, N) and exp.dtype == got.dtype, (exp.shape, exp.dtype, got.dtype)
        want[:M, :N] = exp
    bad = bits(got) != bits(want)
    if bool(bad.any()):
        inside = torch.zeros_like(bad)
        inside[:M, :N] = exp is not None
        parts = []
        if bool((bad & inside).any()):
            flt = got.dtype.is_floating_point
            parts.append("result: " + describe_mismatch(bad & inside, got.float() if flt else got, want.float() if flt else want))
        if bool((bad & ~inside).any()):
            parts.append("memory outside the result was written: " + describe_mismatch(bad & ~inside))
        raise AssertionError(f"{what}: " + "; ".join(parts))


def check_rand(got, before, ref64, bar, masked, M, N, what):
    """The non-power-of-two cases: every element within its bar, masked elements exactly zero, nothing else written."""
    got, before = got.cpu(), before.cpu()
    check_buffer(got, before, got[:M, :N].clone(), M, N, what)          # only the guard rows and the pad columns are compared here
    res = got[:M, :N].double()
    assert bool(torch.isfinite(res).all()), f"{what}: non-finite output"
    bad = (res - ref64).abs() > bar
    if masked is not None:
        bad |= masked & (bits(got[:M, :N].contiguous()) != 0)
    assert not bool(bad.any()), f"{what}: " + describe_mismatch(bad, res, ref64)


# ------------------------------------------------------------------------------------------------------------------
# quantiser edges
# ------------------------------------------------------------------------------------------------------------------
def tiny_rows(K=64):
    """Rows whose first 32-block has amax 2^-116, 2^-118 (either side of 448 * 2^-126: the last scale byte above the clamp, the clamp
    to 1), 2^-120, 2^-126, only bf16 subnormals (2^-131, 2^-133), 3.0e38; the other blocks hold ordinary values.  Exact in bf16."""
    x = torch.randn(6, K, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).float()
    x[:, :32] = 0
    for r, e in enumerate((-116, -118, -120, -126)):
        x[r, 3], x[r, 4], x[r, 20] = 2.0 ** e, -(2.0 ** (e - 1)), 2.0 ** (e - 3)
    x[4, 0], x[4, 1], x[4, 17] = 2.0 ** -131, 2.0 ** -133, -(2.0 ** -132)
    x[5, 7], x[5, 8] = 3.0e38, -1.0e38
    return x.to(torch.bfloat16).float()
