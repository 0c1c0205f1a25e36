"""Retrieval and zero-shot evaluation, host side (no GPU): the header and the signature table, the metric reducers against
brute-force loops, EmbeddingBank.gather under a two-rank gloo group with unequal row counts, the module's `model.retrieval` block and the
trainer's hooks, and the launches of Engine.embed against the stub library of tools/text_launch_trace.py."""
import importlib.util
import os
import re
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")
ENTRIES = ("medmoe_l2_normalize", "medmoe_sim_topk", "medmoe_sim_topk_scratch", "medmoe_sim_topk_splits", "medmoe_sim_rank")


# ------------------------------------------------------------------------------------------------------------------------------------------
# header, sources, signature table
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_five_entries_and_the_sources_exist():
    hdr = open(os.path.join(ROOT, "include", "medmoe_hip.h")).read()
    from medmoe_amd import ops
    for name in ENTRIES:
        m = re.search(r"^(int|long long) %s\((.*)\);" % name, hdr, re.M)
        assert m, name
        short = name[len("medmoe_"):]
        if short in ops._SIGS:
            assert len(m.group(2).split(",")) == len(ops._SIGS[short]) + 1, name              # + the stream
            assert m.group(2).endswith("hipStream_t stream"), name
    src = open(os.path.join(ROOT, "medmoe_amd", "csrc", "retrieval.hip")).read()
    assert '#include "topk_list.h"' in src and "__builtin_amdgcn_mfma_f32_16x16x4f32" in src and "atomic" not in src
    lst = open(os.path.join(ROOT, "medmoe_amd", "csrc", "topk_list.h")).read()
    assert "__host__ __device__" in lst and "topk_insert" in lst and "topk_merge" in lst
    assert os.path.exists(os.path.join(ROOT, "tools", "topk_list_check.cpp"))
    assert re.search(r"^check-topk:", open(os.path.join(ROOT, "Makefile")).read(), re.M)


def test_the_experiment_composes(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    from medmoe_amd.hydra_lite import compose
    cfg = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2_retrieval"])
    assert cfg.model.fused_step is True and list(cfg.model.retrieval.ks) == [1, 5, 10] and sorted(dict(cfg.model.retrieval)) == ["ks"]
    base = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2"])
    assert "retrieval" not in dict(base.model) and cfg.data.batch_size == base.data.batch_size
    on = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2", "+model.retrieval.ks=[1,5]", "+model.retrieval.label_key=label"])
    assert list(on.model.retrieval.ks) == [1, 5] and on.model.retrieval.label_key == "label"


# ------------------------------------------------------------------------------------------------------------------------------------------
# reducers against brute force
# ------------------------------------------------------------------------------------------------------------------------------------------
def _cases():
    g = torch.Generator().manual_seed(3)
    yield torch.randint(0, 50, (37,), generator=g)                   # random
    yield torch.randint(0, 3, (40,), generator=g)                    # tie-heavy
    yield torch.zeros(5, dtype=torch.int64)
    yield torch.tensor([7])


def test_recall_and_rank_stats_match_brute_force():
    from medmoe_amd.retrieval import rank_stats, recall_at_k
    for rank in _cases():
        r = rank.tolist()
        got = recall_at_k(rank.to(torch.int32), (1, 5, 10))
        for k in (1, 5, 10):
            assert got[k] == sum(1 for v in r if v < k) / len(r)
        s = sorted(r)
        n = len(s)
        med = s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2
        mean, median = rank_stats(rank.to(torch.int32))
        assert median == med and abs(mean - sum(r) / n) < 1e-12
    assert all(v != v for v in rank_stats(torch.empty(0, dtype=torch.int32)))            # NaN, NaN


def test_precision_and_topk_accuracy_match_brute_force():
    from medmoe_amd.retrieval import precision_at_k, topk_accuracy
    g = torch.Generator().manual_seed(4)
    for n_cls in (2, 7):                                             # tie-heavy labels, and spread ones
        N, Nk, K = 23, 31, 6
        top = torch.stack([torch.randperm(Nk, generator=g)[:K] for _ in range(N)]).to(torch.int32)
        top[3, 4:] = -1; top[9, :] = -1                              # short lists
        ql, kl = torch.randint(0, n_cls, (N,), generator=g), torch.randint(0, n_cls, (Nk,), generator=g)
        got = precision_at_k(top, ql, kl, (1, 3, 6))
        for k in (1, 3, 6):
            want = sum(sum(1 for j in top[i, :k].tolist() if j >= 0 and int(kl[j]) == int(ql[i])) / k for i in range(N)) / N
            assert abs(got[k] - want) < 1e-12
        with pytest.raises(ValueError):
            precision_at_k(top, ql, kl, (7,))
        # accuracy: rows of class indices
        C = 5
        cls_top = torch.stack([torch.randperm(C, generator=g)[:3] for _ in range(N)]).to(torch.int32)
        cls_top[5, 1:] = -1
        lab = torch.randint(0, C - 1, (N,), generator=g)             # class C - 1 has no sample
        acc = topk_accuracy(cls_top, lab, (1, 3), num_classes=C)
        for k in (1, 3):
            hit = [int(lab[i]) in cls_top[i, :k].tolist() for i in range(N)]
            assert acc["acc"][k] == sum(hit) / N
            for c in range(C):
                members = [i for i in range(N) if int(lab[i]) == c]
                v = float(acc["per_class"][k][c])
                if members:
                    assert v == sum(hit[i] for i in members) / len(members)
                else:
                    assert v != v


# ------------------------------------------------------------------------------------------------------------------------------------------
# the bank: growth on one process, gather under gloo world 2 with unequal counts
# ------------------------------------------------------------------------------------------------------------------------------------------
def _unit(n, d, seed):
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(seed))
    return x / x.norm(dim=1, keepdim=True)


def test_bank_grows_and_keeps_rows_single_process():
    from medmoe_amd.retrieval import EmbeddingBank
    bank = EmbeddingBank(8, "cpu", capacity=4)
    img, txt = _unit(11, 8, 0), _unit(11, 8, 1)
    for s, e in ((0, 3), (3, 4), (4, 11)):
        bank.add(img[s:e], txt[s:e], torch.arange(s, e) if s else None, normalize=False)
    assert len(bank) == 11 and torch.equal(bank.img, img) and torch.equal(bank.txt, txt)
    assert bank.labels.tolist() == [-1, -1, -1] + list(range(3, 11))
    g = bank.gather()
    assert g is bank and (g.local_start, g.local_count) == (0, 11)
    with pytest.raises(ValueError):
        bank.add(img[:2, :4], txt[:2, :4], normalize=False)
    with pytest.raises(RuntimeError, match="GPU"):                   # normalising is a kernel: no CPU fallback
        bank.add(img[:2], txt[:2])
    bank.reset()
    assert len(bank) == 0 and bank.img.shape == (0, 8)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


COUNTS = (5, 2)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from medmoe_amd.retrieval import EmbeddingBank
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    img, txt = _unit(sum(COUNTS), 16, 10), _unit(sum(COUNTS), 16, 11)
    lo = sum(COUNTS[:rank])
    bank = EmbeddingBank(16, "cpu", capacity=2)
    for i in range(lo, lo + COUNTS[rank]):                           # one pair at a time: the bank grows on the way
        bank.add(img[i:i + 1], txt[i:i + 1], torch.tensor([100 + i]), normalize=False)
    g = bank.gather()
    ok = len(g) == sum(COUNTS) and torch.equal(g.img, img) and torch.equal(g.txt, txt) \
        and g.labels.tolist() == [100 + i for i in range(sum(COUNTS))] and (g.local_start, g.local_count) == (lo, COUNTS[rank]) \
        and len(bank) == COUNTS[rank]
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_bank_gather_gloo_world2_unequal_counts():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=100) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
        assert p.exitcode == 0
    assert sorted(res) == [(0, True), (1, True)]


# ------------------------------------------------------------------------------------------------------------------------------------------
# module block, trainer hooks
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_module_block_refusals():
    from src.models.medmoe_module import MedMoEPretrainingLightningModule as M
    net = torch.nn.Identity()
    with pytest.raises(KeyError, match="kz"):
        M(net, {}, retrieval={"kz": [1]})
    with pytest.raises(NotImplementedError, match="model.retrieval.*fused_step"):
        M(net, {}, retrieval={"ks": [1, 5]})

    class SwinNet(torch.nn.Module):
        swin = object()

    with pytest.raises(NotImplementedError, match="model.retrieval.*swin_t"):
        M(SwinNet(), {}, fused_step=True, retrieval={"ks": [1, 5]})
    with pytest.raises(ValueError, match="ks"):
        M._retrieval_block(_Fused(), {"ks": [0]})
    assert M(net, {})._retrieval is None
    blk = M._retrieval_block(_Fused(), {"ks": [1, 5], "zero_shot": "p.pt"})
    assert blk == {"ks": (1, 5), "zero_shot": "p.pt", "zero_shot_ks": (1, 5), "label_key": "label"}


class _Fused:
    fused_step, model = True, None


def test_swin_engine_embed_is_a_named_follow_up():
    from medmoe_amd.swin_engine import SwinEngine
    eng = SwinEngine.__new__(SwinEngine)
    for call in (lambda: eng.embed({}), lambda: eng.embed_image(None), lambda: eng.embed_text(None, None)):
        with pytest.raises(NotImplementedError, match="named follow-up"):
            call()


class _Lit(torch.nn.Module):
    """A module with the reference's steps: counts hook calls, returns a fixed loss."""

    def __init__(self, hooks):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.calls = []
        if hooks:
            self.on_validation_epoch_start = lambda: self.calls.append("vs")
            self.on_validation_epoch_end = lambda: (self.calls.append("ve"), {"i2t_R@1": 0.5, "i2t_median_rank": 2.0})[1]
            self.on_test_epoch_start = lambda: self.calls.append("ts")
            self.on_test_epoch_end = lambda: (self.calls.append("te"), {"i2t_R@1": 0.25})[1]

    def validation_step(self, b, i):
        self.calls.append("step")
        return {"loss": torch.tensor(float(b))}

    test_step = validation_step


class _DM:
    def val_dataloader(self):
        return [1.0, 3.0]


def test_trainer_validate_calls_the_hooks_when_defined_and_is_unchanged_without_them():
    from medmoe_amd.trainer import Trainer
    tr = Trainer()
    plain = _Lit(False)
    assert tr.validate(plain, _DM()) == {"val/loss": 2.0} and plain.calls == ["step", "step"]
    hooked = _Lit(True)
    got = tr.validate(hooked, _DM())
    assert hooked.calls == ["vs", "step", "step", "ve"]
    assert got == {"val/loss": 2.0, "val/i2t_R@1": 0.5, "val/i2t_median_rank": 2.0}
    got = tr.test(hooked, _DM())
    assert hooked.calls[4:] == ["ts", "step", "step", "te"] and got["test/i2t_R@1"] == 0.25 and got["val/loss"] == 2.0


def test_module_without_the_block_fires_no_hook_work():
    from src.models.medmoe_module import MedMoEPretrainingLightningModule as M
    m = M(torch.nn.Identity(), {})
    assert m.on_validation_epoch_start() is None and m.on_validation_epoch_end() is None
    assert m.on_test_epoch_start() is None and m.on_test_epoch_end() is None and m._bank is None


# ------------------------------------------------------------------------------------------------------------------------------------------
# Engine.embed against the stub library
# ------------------------------------------------------------------------------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location("text_launch_trace", os.path.join(ROOT, "tools", "text_launch_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _trace(fn):
    """The launches `fn(engine, batch)` makes on a fresh tiny2 engine against the stub library."""
    tool = _tool()
    import medmoe_oracle as O
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    lib = tool._TraceLib()
    with tool._installed(lib, {}):
        eng = Engine(config_by_name("tiny2"), "cpu")
        batch = O.synthetic_batch(O.config_by_name("tiny2"), 8, min_len=4)
        lib.eng = eng
        fn(eng, batch)
    return lib.trace


def test_embed_issues_eval_steps_launches_up_to_the_first_loss_launch():
    ev = _trace(lambda e, b: e.eval_step(b))
    em = _trace(lambda e, b: e.embed(b))
    first_loss = next(i for i, l in enumerate(ev) if l.startswith("medmoe_rownorm("))        # global_loss opens with the row norms
    assert first_loss > 10 and em == ev[:first_loss]
    assert not any(l.startswith(("medmoe_rownorm", "medmoe_sgemm", "medmoe_router_eval", "medmoe_adam")) for l in em)
    # the halves: embed_image + embed_text make the same launches as embed (in tower order), each alone a strict part of them
    name = lambda l: l.split("(")[0]
    im = _trace(lambda e, b: e.embed_image(b["image"]))
    tx = _trace(lambda e, b: e.embed_text(b["ids"], b["attn_mask"], b.get("token_type")))
    assert im and tx and sorted(map(name, im + tx)) == sorted(map(name, em))
    assert "medmoe_patchify_ld" in map(name, im) and "medmoe_patchify_ld" not in map(name, tx)
