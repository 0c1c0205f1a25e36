"""medmoe_local_sim_pairs (csrc/local_eval.hip): the local similarity of a LIST of (image, caption) pairs grouped by image,
against the all-pairs kernel medmoe_local_sim_fwd (bit for bit: the device body is shared) and against oracle.medmoe_oracle.gloria_local_sim
in fp32 on the CPU.  The all-pairs matrix and the oracle are computed once per case and shared."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32
TEMP1, TEMP2 = 4.0, 5.0
# SIM_BAR of tests/test_eval_step_gpu.py: twice the error of the training path's similarity matrix against the same oracle on the same
# inputs, measured on an MI355X (profiles/r05_notes.md).  The same inputs and the same arithmetic: the same bar.
SIM_BAR = {"seeded196": 2.844e-3, "fixture64": 3.116e-3}


def seeded_inputs():
    """The recipe of seeded_case in tests/test_eval_step_gpu.py: 4 images of 196 regions against 84 captions of up to T = 77 words, width 128,
    the lengths at both edges of every length class 1..5."""
    g = torch.Generator().manual_seed(1234)
    B, P, D, T = 4, 196, 128, 77
    lens = [1, 16, 17, 32, 33, 64, 65, T, 8, 48, 49, 70]
    lens += [int(v) for v in torch.randint(1, T + 1, (52,), generator=g)] + [int(v) for v in torch.randint(1, 17, (20,), generator=g)]
    img = (0.3 * torch.randn(B, D, 14, 14, generator=g)).to(BF).float()
    words = (0.3 * torch.randn(len(lens), D, T, generator=g)).to(BF).float()
    return img, words, lens


def fixture_inputs():
    d = np.load(os.path.join(GOLDEN, "gloria_local_mfma.npz"))
    return (torch.from_numpy(np.asarray(d["img_l"])).float(), torch.from_numpy(np.asarray(d["words"])).float(), [int(v) for v in d["cap_lens"]])


def pair_list(case, B, lens):
    """[(image, caption)] in list order.  seeded196: image 0 gets all 84 captions (every class, more than one iteration), image 1 none,
    image 2 the one caption of 77 words, image 3 sixteen captions of which caption 20 comes twice (and is listed for image 0 as well).
    fixture64: image 0 every caption, image 1 none, the others a few each with repeats across images."""
    Bc = len(lens)
    if case == "seeded196":
        return [(0, i) for i in range(Bc)] + [(2, 7)] + [(3, i) for i in (20, 1, 2, 12, 13, 20, 30, 31, 40, 41, 50, 60, 66, 70, 80, 83)]
    return [(0, i) for i in range(Bc)] + [(b, (b * 3 + j * 5) % Bc) for b in range(2, B) for j in range(1 + b % 3)]


class Case:
    """Device inputs, the all-pairs matrix of local_sim_forward (and the Gram matrices / word norms it left behind) and the oracle's."""

    def __init__(self, name):
        from medmoe_amd.local_transposed import LocalSimScratch, local_sim_forward
        from oracle.medmoe_oracle import gloria_local_sim
        img, words, lens = seeded_inputs() if name == "seeded196" else fixture_inputs()
        self.name, self.lens = name, lens
        self.B, self.D, self.P = img.shape[0], img.shape[1], img.shape[2] * img.shape[3]
        self.Bc, self.T = words.shape[0], words.shape[2]
        self.ctx = img.reshape(self.B, self.D, -1).transpose(1, 2).contiguous().view(-1, self.D).to("cuda", BF)
        self.words = words.transpose(1, 2).contiguous().to("cuda", BF)
        self.cap = torch.tensor(lens, device="cuda", dtype=I32)
        self.scratch = LocalSimScratch(self.B, self.P, "cuda")
        self.gm3 = self.scratch.gm3
        self.wn = torch.empty(self.Bc, self.T, device="cuda", dtype=F32)
        full = torch.full((self.B, self.Bc), float("nan"), device="cuda", dtype=F32)
        local_sim_forward(self.ctx, self.words, self.cap, np.asarray(lens), TEMP1, TEMP2, gm3=self.gm3, wn=self.wn, sim=full,
                          **self.scratch.gram_kw(self.B))
        self.full = full.cpu()
        assert torch.isfinite(self.full).all()
        self.oracle = gloria_local_sim(img, words, lens, TEMP1, TEMP2)[0]
        self.pairs = pair_list(name, self.B, lens)
        # a slot of its own for every list entry, scattered over a buffer twice as long: every other slot is named by no entry
        self.n_slots = 2 * len(self.pairs) + 3
        perm = torch.randperm(self.n_slots, generator=torch.Generator().manual_seed(9)).tolist()
        self.slots = perm[:len(self.pairs)]

    def ntt(self, i):
        return (min(max(self.lens[i], 1), self.T) + 15) // 16

    def tables(self, cuts=None):
        """{ntt: (units, pair_cap, pair_slot)} of the list, one unit per (class, image) - or, with cuts = (3, 5), image 0's run of every
        class cut into units of 3, of 5 and of the remainder."""
        out = {}
        for ntt in sorted({self.ntt(i) for _, i in self.pairs}):
            units, pc, ps = [], [], []
            for b in sorted({b for b, _ in self.pairs}):
                ent = [(i, s) for (bb, i), s in zip(self.pairs, self.slots) if bb == b and self.ntt(i) == ntt]
                if not ent:
                    continue
                first, n = len(pc), len(ent)
                pc += [i for i, _ in ent]; ps += [s for _, s in ent]
                if cuts and b == 0:
                    at = 0
                    for c in list(cuts) + [n]:
                        c = min(c, n - at)
                        if c > 0:
                            units.append([b, first + at, c, 0])
                        at += c
                else:
                    units.append([b, first, n, 0])
            out[ntt] = (np.asarray(units, np.int32), np.asarray(pc, np.int32), np.asarray(ps, np.int32))
        return out

    def run(self, tables=None):
        from medmoe_amd import ops
        out = torch.full((self.n_slots,), float("nan"), device="cuda", dtype=F32)
        for ntt, (units, pc, ps) in (tables or self.tables()).items():
            ops.local_sim_pairs(self.ctx, self.words, self.cap, self.gm3, self.wn, out, units, pc, ps, P=self.P, ntt=ntt, temp1=TEMP1,
                                temp2=TEMP2, cap_lens_host=self.lens)
        return out.cpu()


def same_bits(a, b):
    """Bit for bit, the NaN of the unnamed slots included (torch.equal calls NaN unequal to itself)."""
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@pytest.mark.parametrize("name", ["seeded196", "fixture64"])
def test_listed_pairs_equal_the_all_pairs_kernel_bit_for_bit_and_meet_the_oracle_bar(name):
    c = case(name)
    out = c.run()
    b, i = torch.tensor([p[0] for p in c.pairs]), torch.tensor([p[1] for p in c.pairs])
    got = out[torch.tensor(c.slots)]
    assert torch.equal(got, c.full[b, i])                                                     # 1. the same bits as local_sim_forward's matrix
    err = float((got - c.oracle[b, i]).abs().max())
    print(f"local_sim_pairs {name}: {len(c.pairs)} pairs, max abs error against the fp32 oracle {err:.3e} (bar {SIM_BAR[name]})")
    assert err <= SIM_BAR[name]                                                               # 2.
    named = torch.zeros(c.n_slots, dtype=torch.bool)
    named[torch.tensor(c.slots)] = True
    assert torch.isnan(out[~named]).all() and int((~named).sum()) > len(c.pairs)              # 4. slots no entry names keep their NaN
    assert same_bits(c.run(), out)                                                           # 5. two launches, the same bits


def test_the_seeded_list_covers_what_it_claims():
    c = case("seeded196")
    t = c.tables()
    assert sorted(t) == [1, 2, 3, 4, 5]                                                       # every length class
    per_iter = {1: 8, 2: 4, 3: 4, 4: 2, 5: 2}                                                 # ls_waves(ntt) / ntt captions per iteration
    for ntt, (units, pc, _) in t.items():
        u0 = units[units[:, 0] == 0]
        assert u0.shape[0] == 1 and u0[0, 2] > per_iter[ntt]                                  # image 0: more than one iteration in every class
        assert 1 not in units[:, 0]                                                           # image 1 has no entry
    u5, pc5, _ = t[5]
    assert [pc5[f] for b, f, n, _ in u5.tolist() if b == 2] == [7] and c.lens[7] == 77        # image 2: the one caption of 77 words
    assert sum(int(n) for tt in t.values() for b, _, n, _ in tt[0].tolist() if b == 3) == 16
    assert [p for p in c.pairs if p == (3, 20)] == [(3, 20), (3, 20)] and (0, 20) in c.pairs


def test_cutting_an_images_list_into_units_changes_no_bit():
    c = case("seeded196")
    cut = c.tables(cuts=(3, 5))
    assert all((u[:, 0] == 0).sum() == 3 for u, _, _ in cut.values())                         # units of 3, of 5 and of the remainder
    assert same_bits(c.run(cut), c.run())


def test_refusals_before_a_launch():
    from medmoe_amd import ops
    c = case("fixture64")
    units, pc, ps = c.tables()[1]
    kw = dict(P=c.P, ntt=1, temp1=TEMP1, temp2=TEMP2, cap_lens_host=c.lens)
    out = torch.full((c.n_slots,), 7.0, device="cuda", dtype=F32)
    a = (c.ctx, c.words, c.cap, c.gm3, c.wn, out)
    bad = lambda arr, at, v: (lambda x: (x.__setitem__(at, v), x)[1])(arr.copy())
    for tabs, what in (((bad(units, (0, 0), c.B), pc, ps), "image"), ((bad(units, (0, 0), -1), pc, ps), "image"),
                       ((units, bad(pc, 1, -1), ps), "pair_cap"), ((units, bad(pc, 1, c.Bc), ps), "pair_cap"),
                       ((units, pc, bad(ps, 2, c.n_slots)), "pair_slot"), ((units, pc, bad(ps, 2, -1)), "pair_slot"),
                       ((units, pc, bad(ps, 2, int(ps[3]))), "one owner"), ((bad(units, (0, 2), len(pc) + 1), pc, ps), "entries")):
        with pytest.raises(ValueError, match=what):
            ops.local_sim_pairs(*a, *tabs, **kw)
    s = case("seeded196")
    su, spc, sps = s.tables()[2]
    sout = torch.full((s.n_slots,), 7.0, device="cuda", dtype=F32)
    wrong = spc.copy(); wrong[0] = 7                                                          # a caption of 77 words in the list of class 2
    with pytest.raises(ValueError, match="length class"):
        ops.local_sim_pairs(s.ctx, s.words, s.cap, s.gm3, s.wn, sout, su, wrong, sps, P=s.P, ntt=2, temp1=TEMP1, temp2=TEMP2, cap_lens_host=s.lens)
    # geometries without a kernel: 256 regions, a width of 96 - the wrapper and the library both refuse
    z = lambda *sh, dt=BF: torch.zeros(*sh, device="cuda", dtype=dt)
    one = (np.asarray([[0, 0, 1, 0]], np.int32), np.asarray([0], np.int32), np.asarray([0], np.int32))
    for HW, D in ((256, 128), (196, 96)):
        GR = (HW + 31) // 32 * 32
        t = (z(2 * HW, D), z(2, 16, D), torch.full((2,), 9, device="cuda", dtype=I32), z(2 * GR, GR), z(2, 16, dt=F32), sout)
        with pytest.raises(ValueError, match="no kernel"):
            ops.local_sim_pairs(*t, *one, P=HW, ntt=1, temp1=TEMP1, temp2=TEMP2, cap_lens_host=[9, 9])
        dev = [torch.from_numpy(x).cuda() for x in one]
        with pytest.raises(RuntimeError, match="code -2"):
            ops.call("local_sim_pairs", *t, dev[0], 1, dev[1], dev[2], 2, 2, HW, 16, D, TEMP1, TEMP2, 1e-8, 1)
    # no unit: nothing is launched, through the wrapper and through the library (which does not look at its tables then)
    empty = np.zeros((0, 4), np.int32)
    assert ops.local_sim_pairs(*a, empty, pc[:0], ps[:0], **kw) is out
    ops.call("local_sim_pairs", *a, None, 0, None, None, c.B, c.Bc, c.P, c.T, c.D, TEMP1, TEMP2, 1e-8, 1)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((sout == 7.0).all())
