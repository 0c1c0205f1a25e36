"""Operands, references and the case table of the exact weight-gradient (TN) GEMM tests (test_gemm_tn_exact_gpu.py runs them on the GPU,
test_gemm_tn_exact_host.py checks on the CPU that every reference here is itself exact).  Plain module, no GPU needed to import it.

Integer data: G in {-3..3}, X in {-2..2}, the base of dW and of db in {-64..64}.  With M <= 2^17 every partial sum is an integer below
2^24, so an fp32 accumulation is exact in any order - atomics or staged partial tiles - and the float64 reference is THE result, not an
approximation of it.  The weighted Gram form multiplies A (the G data) by row weights that are multiples of 2^-6 in [-2, 2]; the SCALE build
rounds w * A to bf16 (round to nearest even) before the MFMA, and so does the reference: products k / 64 with 256 < |k| <= 384 need nine
bits, the odd ones are ties.  Every sum stays a multiple of 2^-6 below 2^18 at M <= 4224, so it is still exact.  Everything comes from a
CPU torch.Generator seeded by the case's geometry: random, not periodic in the row or the column, so a shifted or transposed read shows.

A case names the entry point, the geometry, the options it sets, the kernel it must reach (medmoe_last_gemm_tn_kernel) with that launch's
split, and whether medmoe_nondet_launches moves (the form has several atomic writers per element)."""
import itertools
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

# medmoe_last_gemm_tn_kernel ids: generation * 8 + build * 2 + staged
K128, K128M = 0, 2                       # gemm_tn_kernel<false> / <true>
K512, K512M = 8, 10                      # gemm_tn512_kernel<false> / <true>
K4W, K4W_ST, K4WM, K4WM_ST = 16, 17, 18, 19
KCOLG, KCOLG_ST, KGRAM = 20, 21, 22
KERNEL_IDS = (K128, K128M, K512, K512M, K4W, K4W_ST, K4WM, K4WM_ST, KCOLG, KCOLG_ST, KGRAM)
ENTRIES = ("tn", "staged", "det", "cols", "cols_det", "gram", "gram_det")
TN_SMALL, TN_PLAIN, TN_ROWMAP, TN_GROUPS = range(4)          # det_plan::TnKind

# medmoe_set_option keys that steer the TN dispatch, with their defaults
OPT_TN512, OPT_TN_ROWS, OPT_TN4W, OPT_TN_MIN_ROWS, OPT_TN_ROWS4W = 3, 4, 8, 9, 10
OPTION_DEFAULTS = {OPT_TN512: 1, OPT_TN_ROWS: 1024, OPT_TN4W: 1, OPT_TN_MIN_ROWS: 2048, OPT_TN_ROWS4W: 0}

MAX_ROWS, MAX_COLS = 16640, 768
SLOT_FLOATS, SLOT_DB_FLOATS = 65536, 512                       # one partial tile, its column sums of G
GRAM_UNIT = 64.0


@dataclass(frozen=True)
class Case:
    name: str
    entry: str
    kernel: int
    M: int
    Nn: int
    Kk: int
    counts: Tuple[int, ...] = ()        # row groups (row_off); () = ungrouped
    xmap: bool = False
    gmap: bool = False
    db: bool = True
    nsplit: int = 16                    # medmoe_gemm_tn's argument (the 128 x 128 kernel's ranges per tile)
    opts: Tuple[Tuple[int, int], ...] = ()
    split: Optional[int] = None         # the nsplit the launch must report (None: not asserted)
    nondet: int = 0                     # by how much medmoe_nondet_launches moves per launch
    scratch: str = ""                   # staged: "room" (tiles + db partials), "tiles" (no room for the db partials), "short" (one float short)
    slots: int = 0                      # partial tiles of a staged launch (scratch = slots * 65536, + slots * 512 for db)
    det_kind: Optional[int] = None      # medmoe_gemm_tn_det: the TnKind the plan must take
    col_groups: int = 1                 # cols / gram: column groups
    x_shared: bool = False              # cols: xcol_stride 0
    chunk_w: int = 0                    # cols: G stored in chunks of this many columns
    ldw_pad: int = 8                    # dW's pitch is Kk + ldw_pad
    w_ld: int = 1                       # gram: pitch of the weights

    @property
    def id(self):
        return f"{self.entry}-k{self.kernel}-{self.name}"

    @property
    def n_groups(self):
        return len(self.counts) if self.counts else (self.col_groups if self.entry in ("cols", "cols_det", "gram", "gram_det") else 1)

    @property
    def geom(self):
        """What the data depends on: cases that differ only in entry point, options or outputs share their operands."""
        if self.entry in ("gram", "gram_det"):
            return ("gram", self.M, self.Nn, self.col_groups, self.w_ld)
        if self.entry in ("cols", "cols_det"):
            return ("cols", self.M, self.Nn, self.Kk, self.col_groups, self.x_shared, self.chunk_w)
        return ("rows", self.M, self.Nn, self.Kk, self.counts, self.xmap, self.gmap)

    @property
    def staged_launch(self):
        return bool(self.kernel & 1)


GROUPS_B = (32, 4128, 8192)                 # three groups: average above the 4096 rows per group the 256 x 256 kernels ask for
GROUPS_B0 = (0, 32, 4128, 8192)             # with an empty one: average 3088 - deterministic mode (>= 2048) still takes the four-wave kernel
GROUPS_RING = (0, 32, 4128, 12320)          # 12320 rows = 385 sub-steps: as ONE range the row-map ring refills at sub-steps 128 and 256
GROUPS_SHORT = (31, 65, 288, 16096)         # ragged tails 31 and 1; ranges of 1, 3, 9 sub-steps and, cut by the options, 2, 4 and 5
GROUPS_SMALL = (70, 0, 133)


def _cases():
    out = []

    def add(name, entry, kernel, M, Nn, Kk, **kw):
        out.append(Case(name, entry, kernel, M, Nn, Kk, **kw))

    def o(*pairs):
        return tuple(pairs)

    # --- gemm_tn_kernel<false>: every shape the 256 x 256 kernels leave
    add("1x8x8", "tn", K128, 1, 8, 8, nsplit=1, split=1)
    add("63x8x136", "tn", K128, 63, 8, 136, nsplit=1, split=1)
    add("100x136x72-s4", "tn", K128, 100, 136, 72, nsplit=4, split=4, nondet=1)                 # chunk 64: two of the four splits are empty
    add("100x136x72-s4-nodb", "tn", K128, 100, 136, 72, nsplit=4, split=4, nondet=1, db=False)
    add("193x264x8-s2", "tn", K128, 193, 264, 8, nsplit=2, split=2, nondet=1)
    for ns in (1, 2, 5):                                                                        # 5, 3 (+2) and 1 k-steps per range
        add(f"320x128x128-s{ns}", "tn", K128, 320, 128, 128, nsplit=ns, split=ns, nondet=int(ns > 1))
    add("4064x256x256", "tn", K128, 4064, 256, 256, split=16, nondet=1)                          # just under the 4096-row threshold
    add("4064x256x256-nodb", "tn", K128, 4064, 256, 256, split=16, nondet=1, db=False)
    add("groups-small", "tn", K128, sum(GROUPS_SMALL), 136, 72, counts=GROUPS_SMALL, nsplit=2, split=2, nondet=1)
    # --- gemm_tn_kernel<true>: three groups with an empty one, ragged counts, physical row 0 NaN and unnamed
    for nm, xm, gm in (("x", True, False), ("g", False, True), ("xg", True, True)):
        add(f"groups-small-{nm}map", "tn", K128M, sum(GROUPS_SMALL), 136, 72, counts=GROUPS_SMALL, xmap=xm, gmap=gm, nsplit=2, split=2, nondet=1)
    add("203x136x72-xgmap-s1", "tn", K128M, 203, 136, 72, xmap=True, gmap=True, nsplit=1, split=1)
    # four groups that average 3088 rows stay on the 128 x 128 kernel outside deterministic mode
    add("groups-b0-xmap", "tn", K128M, sum(GROUPS_B0), 128, 256, counts=GROUPS_B0, xmap=True, split=16, nondet=1)

    # --- plain 256 x 256: gemm_tn4w_kernel<false>, gemm_tn512_kernel<false> under option 8 = 0; the staged form of the same shapes
    plain = [
        ("4096x256x256", 4096, 256, 256, (), 2, 1),
        ("4096x512x256", 4096, 512, 256, (), 2, 2),                                              # two n tiles: db from every workgroup, the pairs of waves alternate
        ("4128x256x512", 4128, 256, 512, (), 2, 2),                                              # 129 sub-steps: 65 + 64; two k tiles: db only from the k-tile-0 workgroups
        ("4096x256x256-r64", 4096, 256, 256, o((OPT_TN_MIN_ROWS, 64)), 64, 1),                   # 64 ranges of two sub-steps
        ("4096x256x256-r1365", 4096, 256, 256, o((OPT_TN_MIN_ROWS, 1365)), 3, 1),                # 43, 43 and 42 sub-steps
        ("4128x256x512-r64", 4128, 256, 512, o((OPT_TN_MIN_ROWS, 64)), 64, 2),                   # 43 ranges of three sub-steps, 21 empty ones
    ]
    for nm, M, Nn, Kk, op, ns, ntile in plain:
        add(nm, "tn", K4W, M, Nn, Kk, opts=op, split=ns, nondet=1)
        add(nm, "tn", K512, M, Nn, Kk, opts=op + o((OPT_TN4W, 0)), split=ns, nondet=1)
        add(nm + "-room", "staged", K4W_ST, M, Nn, Kk, opts=op, split=ns, scratch="room", slots=ns * ntile)
        add(nm + "-tiles", "staged", K4W_ST, M, Nn, Kk, opts=op, split=ns, scratch="tiles", slots=ns * ntile, nondet=1)   # db keeps its atomics
    add("4096x256x256-nodb", "tn", K4W, 4096, 256, 256, split=2, nondet=1, db=False)
    add("4096x256x256-nodb", "tn", K512, 4096, 256, 256, opts=o((OPT_TN4W, 0)), split=2, nondet=1, db=False)
    add("4096x512x256-tiles-nodb", "staged", K4W_ST, 4096, 512, 256, split=2, scratch="tiles", slots=4, db=False)
    add("4096x256x256-short", "staged", K4W, 4096, 256, 256, split=2, scratch="short", slots=2, nondet=1)      # falls back to the atomic form

    # --- MAPPED 256 x 256: gemm_tn4w_kernel<true> (ranges of R rows over the groups), gemm_tn512_kernel<true> under option 8 = 0
    def mapped(tag, counts, M, variants, o4w, s4w, o512, s512):
        for nm, Nn, xm, gm in variants:
            kw = dict(counts=counts, xmap=xm, gmap=gm, nondet=1)
            add(f"{tag}-n{Nn}-{nm}", "tn", K4WM, M, Nn, 256, opts=o4w, split=s4w, **kw)
            add(f"{tag}-n{Nn}-{nm}", "tn", K512M, M, Nn, 256, opts=o512 + o((OPT_TN4W, 0)), split=s512, **kw)

    three = tuple((nm, Nn, xm, gm) for Nn in (128, 384) for nm, xm, gm in (("xmap", True, False), ("gmap", False, True), ("nomap", False, False)))
    two = (("xmap", 128, True, False), ("gmap", 384, False, True))
    # (the library counts this form as order-dependent whatever the instance: several ranges may add to one tile)
    mapped("groups-b", GROUPS_B, sum(GROUPS_B), three, (), 4096, (), 4)
    # ONE range per group: the 385 sub-steps of the last group refill the ring twice, the 129 of the third once
    mapped("groups-ring", GROUPS_RING, sum(GROUPS_RING), two, o((OPT_TN_ROWS4W, 12320)), 12320, o((OPT_TN_ROWS, 8192)), 1)
    # short ranges: four-wave 1, 3, 5 + 4, 100 x 5 + 3 sub-steps; eight-wave 1, 3, 9, 503
    mapped("groups-short-a", GROUPS_SHORT, sum(GROUPS_SHORT), two[:1], o((OPT_TN_ROWS4W, 160)), 160, o((OPT_TN_ROWS, 8192)), 1)
    # four-wave 1, 2 + 1, 4 x 2 + 1, 251 x 2 + 1; eight-wave 1, 2 + 1, 5 + 4, 252 + 251
    mapped("groups-short-b", GROUPS_SHORT, sum(GROUPS_SHORT), two[1:], o((OPT_TN_ROWS4W, 64)), 64, o((OPT_TN_ROWS, 2048)), 2)
    # the ungrouped row-mapped form as ONE range of 385 sub-steps
    mapped("rowmap-12320", (), 12320, two, o((OPT_TN_ROWS, 16384)), 1, o((OPT_TN_ROWS, 16384)), 1)

    # --- medmoe_gemm_tn_det: every kind of det_plan::tn_plan
    add("320x128x128", "det", K128, 320, 128, 128, split=1, det_kind=TN_SMALL)
    add("groups-small-xgmap", "det", K128M, sum(GROUPS_SMALL), 136, 72, counts=GROUPS_SMALL, xmap=True, gmap=True, split=1, det_kind=TN_SMALL)
    add("4096x256x256", "det", K4W_ST, 4096, 256, 256, split=2, det_kind=TN_PLAIN, slots=2)
    add("4128x256x512-r64", "det", K4W_ST, 4128, 256, 512, opts=o((OPT_TN_MIN_ROWS, 64)), split=64, det_kind=TN_PLAIN, slots=128)
    add("rowmap-2080-n128-xmap", "det", K4WM_ST, 2080, 128, 256, xmap=True, split=1, det_kind=TN_ROWMAP, slots=1)     # only this mode sends 2080 rows here
    add("rowmap-2080-n384-gmap", "det", K4WM_ST, 2080, 384, 256, gmap=True, split=1, det_kind=TN_ROWMAP, slots=2)
    for nm, Nn, xm, gm in three:                                     # 12352 / 4096 + 4 = 7 ranges at most, per 256 x 256 tile
        add(f"groups-b0-n{Nn}-{nm}", "det", K4WM_ST, sum(GROUPS_B0), Nn, 256, counts=GROUPS_B0, xmap=xm, gmap=gm, split=4096, det_kind=TN_GROUPS,
            slots=7 * ((Nn + 255) // 256))
    add("groups-b0-n384-gmap-nodb", "det", K4WM_ST, sum(GROUPS_B0), 384, 256, counts=GROUPS_B0, gmap=True, split=4096, det_kind=TN_GROUPS, slots=14,
        db=False)
    # 2 x (12352 / 32 + 4) = 780 slots > 512: the plan doubles the range once, 2 x (12352 / 64 + 4) = 394
    add("groups-b0-n384-nomap-r32", "det", K4WM_ST, sum(GROUPS_B0), 384, 256, counts=GROUPS_B0, opts=o((OPT_TN_ROWS4W, 32)), split=64,
        det_kind=TN_GROUPS, slots=394)
    add("groups-ring-n128-xmap", "det", K4WM_ST, sum(GROUPS_RING), 128, 256, counts=GROUPS_RING, xmap=True, opts=o((OPT_TN_ROWS4W, 12320)),
        split=12320, det_kind=TN_GROUPS, slots=5)
    add("groups-short-n384-gmap-r160", "det", K4WM_ST, sum(GROUPS_SHORT), 384, 256, counts=GROUPS_SHORT, gmap=True, opts=o((OPT_TN_ROWS4W, 160)),
        split=160, det_kind=TN_GROUPS, slots=2 * (16480 // 160 + 4))

    # --- column groups: gemm_tn4w_kernel<false, COLG>; U = 1..5 sub-steps around the four-deep DMA ring
    def cols(name, M, Nn, Kk, ns, ntile, **kw):
        add(name, "cols", KCOLG, M, Nn, Kk, split=ns, nondet=int(ns > 1), **kw)
        add(name, "cols_det", KCOLG_ST if ns > 1 else KCOLG, M, Nn, Kk, split=ns, slots=ns * ntile if ns > 1 else 0, **kw)

    for M in (32, 64, 96, 128, 160):
        cols(f"{M}x208x264-g3", M, 208, 264, 1, 6, col_groups=3)
    cols("160x208x264-g3-r64", 160, 208, 264, 2, 6, col_groups=3, opts=o((OPT_TN_MIN_ROWS, 64)))            # two ranges: 96 and 64 rows
    cols("4224x624x208-g3-xshared", 4224, 624, 208, 2, 9, col_groups=3, x_shared=True)
    cols("4224x208x264-g3-ldw6", 4224, 208, 264, 2, 6, col_groups=3, ldw_pad=6)                             # ldw % 4 == 2: the summing kernel's scalar path
    cols("96x8x8", 96, 8, 8, 1, 1)
    cols("128x264x8", 128, 264, 8, 1, 2)
    cols("128x8x624", 128, 8, 624, 1, 3)
    cols("4224x624x264-chunk208", 4224, 624, 264, 2, 6, chunk_w=208)                                        # a 256-column tile spans a seam
    cols("160x264x208-chunk24", 160, 264, 208, 1, 2, chunk_w=24)                                            # 24 does not divide 256
    cols("160x264x208-chunk24-r64", 160, 264, 208, 2, 2, chunk_w=24, opts=o((OPT_TN_MIN_ROWS, 64)))

    # --- weighted Gram: gemm_tn4w_kernel<false, COLG, SCALE>
    for M, Q, w_ld in ((32, 8, 1), (96, 64, 1), (96, 208, 3), (32, 264, 1), (4224, 264, 1), (4224, 208, 3), (4224, 64, 1)):
        tiles = (Q + 255) // 256
        ns = max(1, min(256 // (tiles * tiles * 3), M // 2048))
        add(f"{M}x{Q}-g3-w{w_ld}", "gram", KGRAM, M, Q, Q, col_groups=3, w_ld=w_ld, split=ns, nondet=int(ns > 1), db=False)
        add(f"{M}x{Q}-g3-w{w_ld}", "gram_det", KGRAM, M, Q, Q, col_groups=3, w_ld=w_ld, split=1, db=False)
    return out


CASES = _cases()

# argument checks: nothing is launched, dW stays bit-identical
REFUSALS = ("Nn%8", "ld%8", "cols M%32", "cols Nn>ldg", "gram w_ld<1", "det scratch short")


# ------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------
@dataclass
class Operands:
    """CPU fp32 tensors, every value exact in bf16.
    rows forms: g [Sg, Nn], x [Sx, Kk]; packed row m reads g[gmap[m]] and x[xmap[m]] (None: identity); with a map, source row 0 and every
    row no entry names are unused (the GPU test fills them with NaN).
    cols forms: g [M, col_groups * Nn] (chunked: [chunks, M, chunk_w], one group), x [M, col_groups * Kk] ([M, Kk] when shared).
    gram: g [M, col_groups * Q], w [col_groups, M]."""
    case_geom: tuple
    g: torch.Tensor
    x: Optional[torch.Tensor]
    base_dw: torch.Tensor               # [n_groups, Nn, Kk]
    base_db: torch.Tensor               # [n_groups, Nn]
    gmap: Optional[torch.Tensor] = None
    xmap: Optional[torch.Tensor] = None
    row_off: Optional[torch.Tensor] = None
    w: Optional[torch.Tensor] = None


def _seed(geom):
    return zlib.crc32(repr(geom).encode()) % (2 ** 31 - 1)


def _ints(gen, lo, hi, *size):
    return torch.randint(lo, hi + 1, size, generator=gen).float()


def _distinct(t):
    return t.shape[0] < 2 or torch.unique(t, dim=0).shape[0] == t.shape[0]


def _matrix(gen, lim, rows, cols):
    """Integers in -lim..lim, [rows, cols], drawn again (from the same generator: still a function of the seed) until no two rows and no
    two columns are equal - narrow operands of eight columns collide now and then."""
    for _ in range(64):
        t = _ints(gen, -lim, lim, rows, cols)
        if rows == 1 or (_distinct(t) and _distinct(t.t().contiguous())):
            return t
    raise ValueError(f"no {rows} x {cols} matrix with distinct rows and columns in -{lim}..{lim}")


def make_operands(c: Case) -> Operands:
    gen = torch.Generator(device="cpu")
    gen.manual_seed(_seed(c.geom))
    G = c.n_groups
    base_dw, base_db = _ints(gen, -64, 64, G, c.Nn, c.Kk), _ints(gen, -64, 64, G, c.Nn)
    kind = c.geom[0]
    if kind == "gram":
        a = _matrix(gen, 3, c.M, G * c.Nn)
        w = _ints(gen, -128, 128, G, c.M) / GRAM_UNIT
        for i in range(G):                                  # 0 and both ends of the range in every group, whatever was drawn
            at = torch.randperm(c.M, generator=gen)[:3]
            w[i, at[0]], w[i, at[1]], w[i, at[2]] = 0.0, 2.0, -2.0
        return Operands(c.geom, a, None, base_dw, base_db, w=w)
    if kind == "cols":
        if c.chunk_w:
            chunks = -(-c.Nn // c.chunk_w)
            g = _matrix(gen, 3, c.M, chunks * c.chunk_w).view(c.M, chunks, c.chunk_w).permute(1, 0, 2).contiguous()
        else:
            g = _matrix(gen, 3, c.M, G * c.Nn)
        x = _matrix(gen, 2, c.M, c.Kk if c.x_shared else G * c.Kk)
        return Operands(c.geom, g, x, base_dw, base_db)
    extra_g, extra_x = (1 + 37 if c.gmap else 0), (1 + 21 if c.xmap else 0)
    g, x = _matrix(gen, 3, c.M + extra_g, c.Nn), _matrix(gen, 2, c.M + extra_x, c.Kk)
    gmap = (1 + torch.randperm(c.M + extra_g - 1, generator=gen)[:c.M]).int() if c.gmap else None      # never names row 0
    xmap = (1 + torch.randperm(c.M + extra_x - 1, generator=gen)[:c.M]).int() if c.xmap else None
    row_off = None
    if c.counts:
        row_off = torch.tensor([0] + list(itertools.accumulate(c.counts)), dtype=torch.int32)
    return Operands(c.geom, g, x, base_dw, base_db, gmap, xmap, row_off)


def to_device(o: Operands, device) -> Operands:
    mv = lambda t: None if t is None else t.to(device)
    return Operands(o.case_geom, mv(o.g), mv(o.x), mv(o.base_dw), mv(o.base_db), mv(o.gmap), mv(o.xmap), mv(o.row_off), mv(o.w))


# ------------------------------------------------------------------------------------------------------------------
# references: one plain function per entry-point form, each adds onto the base (any device; float64 is the reference, float32 on the CPU is
# what the host file compares it with).  Every one returns (dW [groups, Nn, Kk], db [groups, Nn]).
# ------------------------------------------------------------------------------------------------------------------
def ref_plain(g, x, base_dw, base_db, dtype=torch.float64):
    """dW += G^T X, db += column sums of G."""
    g, x = g.to(dtype), x.to(dtype)
    return base_dw.to(dtype) + (g.t() @ x)[None], base_db.to(dtype) + g.sum(0)[None]


def ref_row_groups(g, x, row_off, base_dw, base_db, dtype=torch.float64):
    """Group i owns the packed rows row_off[i] .. row_off[i + 1]; a group without rows keeps its base."""
    dw, db = base_dw.to(dtype).clone(), base_db.to(dtype).clone()
    for i in range(dw.shape[0]):
        a, b = int(row_off[i]), int(row_off[i + 1])
        if b > a:
            gi = g[a:b].to(dtype)
            dw[i] += gi.t() @ x[a:b].to(dtype)
            db[i] += gi.sum(0)
    return dw, db


def ref_mapped(g_src, x_src, gmap, xmap, row_off, base_dw, base_db, dtype=torch.float64):
    """Packed row m reads g_src[gmap[m]] and x_src[xmap[m]] (either map may be None); grouped by row_off when given."""
    M = (gmap if gmap is not None else xmap).shape[0]
    g = g_src[gmap.long()] if gmap is not None else g_src[:M]
    x = x_src[xmap.long()] if xmap is not None else x_src[:M]
    if row_off is None:
        return ref_plain(g, x, base_dw, base_db, dtype)
    return ref_row_groups(g, x, row_off, base_dw, base_db, dtype)


def ref_cols(g, x, Nn, Kk, n_groups, gcol_stride, xcol_stride, base_dw, dtype=torch.float64):
    """Column group i multiplies G[:, i * gcol_stride + (0..Nn)] and X[:, i * xcol_stride + (0..Kk)] over all rows (stride 0: shared)."""
    dw = base_dw.to(dtype).clone()
    for i in range(n_groups):
        gi = g[:, i * gcol_stride:i * gcol_stride + Nn].to(dtype)
        dw[i] += gi.t() @ x[:, i * xcol_stride:i * xcol_stride + Kk].to(dtype)
    return dw


def ref_cols_chunked(g_chunks, x, Nn, base_dw, dtype=torch.float64):
    """G's column c is column c % w of chunk c // w (g_chunks [chunks, M, w])."""
    g = g_chunks.permute(1, 0, 2).reshape(g_chunks.shape[1], -1)[:, :Nn].to(dtype)
    return base_dw.to(dtype) + (g.t() @ x.to(dtype))[None]


def scaled_rows(a, w):
    """bf16(w * A), the rounding of the SCALE build: the fp32 product (exact for this data), one round-to-nearest-even."""
    return (a.float() * w.float()[:, None]).to(torch.bfloat16)


def ref_gram(a, w, Q, n_groups, col_stride, base_dw, dtype=torch.float64):
    """dW[i] += bf16(w_i * A_i)^T A_i for the column blocks A_i = A[:, i * col_stride + (0..Q)]."""
    dw = base_dw.to(dtype).clone()
    for i in range(n_groups):
        ai = a[:, i * col_stride:i * col_stride + Q]
        dw[i] += scaled_rows(ai, w[i]).to(dtype).t() @ ai.to(dtype)
    return dw


def used_sources(c: Case, o: Operands):
    """The G and X rows a case multiplies, in packed order: ([M, *], [M, *]) of the whole matrices."""
    if c.geom[0] == "rows":
        g = o.g[o.gmap.long()] if o.gmap is not None else o.g[:c.M]
        x = o.x[o.xmap.long()] if o.xmap is not None else o.x[:c.M]
        return g, x
    g = o.g.permute(1, 0, 2).reshape(c.M, -1) if c.chunk_w else o.g
    return g, (o.g if o.x is None else o.x)


def reference(c: Case, o: Operands, dtype=torch.float64):
    """(dW, db or None) of ONE launch of the case on its base."""
    kind = c.geom[0]
    if kind == "gram":
        return ref_gram(o.g, o.w, c.Nn, c.n_groups, c.Nn, o.base_dw, dtype), None
    if kind == "cols":
        if c.chunk_w:
            return ref_cols_chunked(o.g, o.x, c.Nn, o.base_dw, dtype), None
        return ref_cols(o.g, o.x, c.Nn, c.Kk, c.n_groups, c.Nn, 0 if c.x_shared else c.Kk, o.base_dw, dtype), None
    if o.gmap is not None or o.xmap is not None:
        dw, db = ref_mapped(o.g, o.x, o.gmap, o.xmap, o.row_off, o.base_dw, o.base_db, dtype)
    elif o.row_off is not None:
        dw, db = ref_row_groups(o.g[:c.M], o.x[:c.M], o.row_off, o.base_dw, o.base_db, dtype)
    else:
        dw, db = ref_plain(o.g[:c.M], o.x[:c.M], o.base_dw, o.base_db, dtype)
    return dw, (db if c.db else None)


def scratch_floats(c: Case) -> int:
    """The scratch a staged case hands over: exactly what the form needs (0: none)."""
    if c.entry == "staged":
        return {"room": c.slots * (SLOT_FLOATS + SLOT_DB_FLOATS), "tiles": c.slots * SLOT_FLOATS,
                "short": c.slots * SLOT_FLOATS - 1}[c.scratch]
    if c.entry == "det":
        return c.slots * (SLOT_FLOATS + SLOT_DB_FLOATS)
    if c.entry == "cols_det":
        return c.slots * SLOT_FLOATS
    return 0
