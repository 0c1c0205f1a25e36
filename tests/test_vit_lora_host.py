"""Frozen ViT tower and LoRA adapters on it, host side (no GPU): configuration rules, the Hydra keys, the experiment file, the header,
the parameter-group rules, the arena's frozen head, and the engine's launch sequences against a stub library that computes nothing."""
import os
import re

import pytest

from test_text_lora_host import stub  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")


def _cfg(**kw):
    from medmoe_amd.config import config_by_name
    c = config_by_name("tiny2")
    c.vit_lora = True
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_defaults_are_off_and_plain_configs_validate():
    from medmoe_amd.config import MedMoEConfig
    c = MedMoEConfig()
    assert (c.freeze_vit, c.vit_lora, c.vit_lora_r, c.vit_lora_alpha, c.vit_lora_dropout, tuple(c.vit_lora_targets)) == \
        (False, False, 8, 16.0, 0.0, ("query", "value"))
    assert not c.vit_frozen
    c.validate()
    _cfg().validate()
    assert _cfg().vit_frozen and _cfg(vit_lora=False, freeze_vit=True).vit_frozen          # adapters imply a frozen base, as get_peft_model does
    _cfg(vit_lora_r=1, vit_lora_targets=("value",)).validate()
    _cfg(vit_lora_r=16, vit_lora_targets=("query", "key", "value"), vit_lora_dropout=0.5, deterministic=True).validate()
    _cfg(vit_lora=False, freeze_vit=True, deterministic=True).validate()


def test_validate_rejects_every_bad_value():
    for r in (0, 17, -1):
        with pytest.raises(ValueError, match="vit_lora_r"):
            _cfg(vit_lora_r=r).validate()
    for a in (0.0, -1.0):
        with pytest.raises(ValueError, match="vit_lora_alpha"):
            _cfg(vit_lora_alpha=a).validate()
    for tg in ((), ("query", "query"), ("query", "output"), ("dense",)):
        with pytest.raises(ValueError, match="vit_lora_targets"):
            _cfg(vit_lora_targets=tg).validate()
    for p in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="vit_lora_dropout"):
            _cfg(vit_lora_dropout=p).validate()


def test_hydra_keys_reach_the_config_and_absent_keys_change_nothing():
    from src.models.components.med_moe import config_from_hydra
    c = config_from_hydra({"config_name": "tiny2"}, {})
    assert not c.freeze_vit and not c.vit_lora and not c.vit_frozen and c.vit_lora_dropout == 0.0
    # the yaml defaults of the reference's keys (lora_r 8, lora_alpha 16, lora_dropout 0.1) count only with lora_vit
    c = config_from_hydra({"config_name": "tiny2", "lora": False, "lora_r": 4, "lora_alpha": 32, "lora_dropout": 0.1}, {})
    assert not c.vit_lora and (c.vit_lora_r, c.vit_lora_alpha, c.vit_lora_dropout) == (8, 16.0, 0.0)
    c = config_from_hydra({"config_name": "tiny2", "freeze_cnn": True}, {})
    assert c.freeze_vit and not c.vit_lora and c.vit_frozen
    c.validate()
    c = config_from_hydra({"arch": "vit_b16", "lora_vit": True, "lora_r": 4, "lora_alpha": 32, "lora_dropout": 0.1,
                           "lora_targets": ["query", "key", "value"]}, {})
    assert c.vit_lora and c.vit_frozen and not c.freeze_vit and c.vit_lora_r == 4 and c.vit_lora_alpha == 32.0 and c.vit_lora_dropout == 0.1
    assert tuple(c.vit_lora_targets) == ("query", "key", "value")
    c.validate()
    c = config_from_hydra({"config_name": "tiny2", "lora_vit": True, "lora_targets": "value"}, {})
    assert tuple(c.vit_lora_targets) == ("value",) and c.vit_lora_dropout == 0.0
    with pytest.raises(ValueError, match="vit_lora_r"):
        config_from_hydra({"config_name": "tiny2", "lora_vit": True, "lora_r": 32}, {}).validate()


def test_vision_lora_is_still_rejected_also_next_to_lora_vit():
    from src.models.components.med_moe import config_from_hydra
    for vision in ({"config_name": "tiny2", "lora": True}, {"config_name": "tiny2", "lora": True, "lora_vit": True}):
        with pytest.raises(NotImplementedError, match="vision.lora"):
            config_from_hydra(vision, {})


def test_swin_refuses_both_keys():
    from src.models.components.med_moe import config_from_hydra
    for key in ("freeze_cnn", "lora_vit"):
        with pytest.raises(NotImplementedError, match=f"vision.{key}=true with vision.arch=swin_t"):
            config_from_hydra({"arch": "swin_t", key: True}, {})
        config_from_hydra({"arch": "swin_t", key: False}, {})


def test_swin_engine_refuses_a_frozen_vit():
    from medmoe_amd.swin_engine import SwinEngine

    class _E:
        deterministic, dist = False, False
    for kw in (dict(vit_lora=False, freeze_vit=True), dict()):
        e = _E()
        e.cfg = _cfg(**kw)
        with pytest.raises(NotImplementedError, match="freeze_vit / vit_lora"):
            SwinEngine(e, None)


def test_the_vit_lora_experiment_composes(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    from medmoe_amd.hydra_lite import compose
    from src.models.components.med_moe import config_from_hydra
    cfg = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2_vit_lora"])
    v = cfg.model.model.vision
    assert v.lora is False and v.lora_vit is True and v.lora_r == 8 and v.lora_alpha == 16 and v.lora_dropout == 0.1
    c = config_from_hydra(v, cfg.model.model.text)
    c.validate()
    assert c.vit_lora and c.vit_frozen and c.vit_lora_r == 8 and c.vit_lora_alpha == 16.0 and c.vit_lora_dropout == 0.1
    assert tuple(c.vit_lora_targets) == ("query", "value") and c.n_expert == 8 and c.top_k == 2 and c.max_len == 77 and not c.text_lora
    # cfg2 itself is unchanged by the new keys
    base = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg2"])
    cb = config_from_hydra(base.model.model.vision, base.model.model.text)
    assert not cb.vit_lora and not cb.freeze_vit and cb.vit_lora_dropout == 0.0


def test_header_declares_the_runs_entry_points_and_the_site_is_clear():
    hdr = open(os.path.join(ROOT, "include", "medmoe_hip.h")).read()
    assert re.search(r"^long long medmoe_lora_wgrad_runs_scratch\(int M, int D, int n, int run\);", hdr, re.M)
    decl = re.search(r"^int medmoe_lora_bwd_wgrad_runs\((.*)\);", hdr, re.M).group(1)
    from medmoe_amd import ops
    assert len(decl.split(",")) == len(ops._SIGS["lora_bwd_wgrad_runs"]) + 1          # + the stream
    assert len(ops._SIGS["lora_bwd_wgrad_runs"]) == len(ops._SIGS["lora_bwd_wgrad"]) + 1 and "int run" in decl
    src = open(os.path.join(ROOT, "medmoe_amd", "csrc", "philox.h")).read()
    site = int(re.search(r"#define DROPOUT_SITE_VIT_LORA (0x[0-9a-f]+)u", src).group(1), 16)
    assert site == ops.DROPOUT_SITE_VIT_LORA
    # clear of every other site for any depth up to 128 layers: the text tower's 4 * layer + {0..3}, stochastic depth, augmentation, embedding
    mine = set(range(site, site + 128))
    others = set(range(0, 4 * 128)) | set(range(ops.DROPOUT_SITE_VIT_DROP_PATH, ops.DROPOUT_SITE_VIT_DROP_PATH + ops.DROP_PATH_MAX_SITES)) \
        | {ops.DROPOUT_SITE_AUGMENT, ops.DROPOUT_SITE_EMBED}
    assert not mine & others


def test_wgrad_run_rule():
    """The engine's run: the largest of 16 / 8 / 4 / 2 that leaves four workgroups per CU (256 CUs), else 1 - the measured optimum at both
    cfg2 shapes (profiles/r19_notes.md)."""
    from medmoe_amd.engine import Engine
    assert Engine.vit_lora_wgrad_run(201728, 768) == 4 and Engine.vit_lora_wgrad_run(25216, 768) == 1
    assert Engine.vit_lora_wgrad_run(8 * 65, 64) == 1 and Engine.vit_lora_wgrad_run(1 << 22, 768) == 16


def test_group_rules_map_adapters_to_their_layer():
    """layer_decay: layer l's adapters get the multiplier of layer l's weights; the no_decay rules see the adapters as 2-D weights."""
    from medmoe_amd.optim_groups import GroupRules, build_assign, depth_of
    from medmoe_amd.text_lora import LoraStore
    cfg = _cfg(vit_lora_targets=("query", "key", "value"))
    names = [LoraStore.name(l, t, w) for l in range(cfg.n_layer_v) for t in ("query", "key", "value") for w in ("A", "B")]
    depth, L = depth_of("vit_lora", names)
    assert L == cfg.n_layer_v and all(depth[LoraStore.name(l, "key", "B")] == l + 1 for l in range(L))
    vit_names = [f"vit.layer.{l}.attention.input_proj.weight" for l in range(L)] + ["vit.pos_embed", "moe.router.0.weight"]
    vdepth, vL = depth_of("vit", vit_names)
    assert vL == L and all(vdepth[f"vit.layer.{l}.attention.input_proj.weight"] == depth[LoraStore.name(l, "query", "A")] for l in range(L))

    class _S:                                                        # what build_assign reads of a store
        def __init__(self, names, shape):
            self.offsets, self.groups, self.shapes = {n: 0 for n in names}, {}, {n: shape for n in names}
    rules = GroupRules(no_decay=(), no_decay_1d=True, layer_decay=0.5)
    out = build_assign({"vit": _S(vit_names, (4, 4)), "vit_lora": _S(names, (16, cfg.d_v))}, rules)
    for l in range(L):
        lm, wm = out["vit_lora"][LoraStore.name(l, "value", "A")]
        assert (lm, wm) == (0.5 ** (L - l), 1.0)                       # 2-D: decayed weights
        assert out["vit"][f"vit.layer.{l}.attention.input_proj.weight"][0] == lm
    out = build_assign({"vit_lora": _S(names, (16, cfg.d_v))}, GroupRules(no_decay=("layer.1.*lora_B",)))
    assert set(out["vit_lora"]) == {LoraStore.name(1, t, "B") for t in ("query", "key", "value")}


def test_arena_with_a_frozen_head():
    """FlatArena(train_from=...): the master and the working copies cover the arena, gradient / moments / average / bf16 gradient the
    trainable tail only; views find an entry in either kind of buffer; a frozen entry has no gradient; run tables are the tail's."""
    import torch
    from medmoe_amd.flat import FlatArena
    entries = [("a", (3, 8)), ("b", (5,)), ("c", (2, 8)), ("d", (7,))]
    ar = FlatArena("cpu", entries, gemm=[("a", False), ("c", False)], train_from="c")
    assert ar.offsets == {"a": 0, "b": 24, "c": 32, "d": 48} and ar.numel == 56 and ar.train_from == 32 and ar.n_train == 24
    assert ar.p32.numel() == ar.p16.numel() == ar.p16t.numel() == 56 and ar.g32.numel() == 24
    assert ar.is_frozen("a") and ar.is_frozen("b") and not ar.is_frozen("c")
    ar.g32.copy_(torch.arange(24.0))
    assert ar.grad("c").flatten().tolist() == list(range(16)) and ar.grad("d").tolist() == list(range(16, 23))
    for n in ("a", "b"):
        with pytest.raises(KeyError, match="frozen"):
            ar.grad(n)
    assert ar.f32("a").shape == (3, 8) and ar.w16t("c").shape == (8, 2)
    assert ar._tr_step.tolist() == [[32, 32, 2, 8]] and ar.tr_table.shape[0] == 2
    assert ar.grad_bounds([0, 24, 32, 48, 56]) == [0, 16, 24]
    ends, lrm, wdm = ar._upload_runs([(24, 1.0, 1.0), (32, 2.0, 1.0), (48, 3.0, 0.0), (56, 1.0, 1.0)])
    assert ends.tolist() == [16, 24] and lrm.tolist() == [3.0, 1.0] and wdm.tolist() == [0.0, 1.0]
    with pytest.raises(KeyError):
        FlatArena("cpu", entries, train_from="nope")
    # train_from = None is the arena as it was: every buffer full size
    full = FlatArena("cpu", entries, gemm=[("a", False), ("c", False)])
    assert full.train_from == 0 and full.n_train == 56 and full.g32.numel() == 56 and full._tr_step is full.tr_table
    assert full.grad_bounds([0, 24, 56]) == [0, 24, 56]


# ------------------------------------------------------------------------------------------------------------------------------------------
# the engine's launch sequences against the stub library
# ------------------------------------------------------------------------------------------------------------------------------------------
def _step(eng, stub, fn="train_step"):
    import medmoe_oracle as O
    batch = O.synthetic_batch(O.config_by_name("tiny2"), 8, min_len=4)
    del stub.calls[:]
    out = getattr(eng, fn)(batch)
    return out, [x for x in stub.calls if not x.endswith("_scratch")]


def test_plain_engine_keeps_its_arena_and_buckets(stub):
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    eng = Engine(config_by_name("tiny2"), "cpu")
    p = eng.params
    assert p.train_from == 0 and p.g32.numel() == p.numel and eng.vlora is None and not eng.vit_frozen
    assert len(eng.bucket_bounds) == eng.cfg.n_layer_v + 3 and eng.bucket_bounds[-1] == p.numel
    assert set(eng.optimizer_stores()) == {"vit"}


def test_engine_launch_sequence_with_a_frozen_tower(stub):
    """freeze_vit alone: the forward as ever; no launch of the tower's backward at all (every trainable gradient - router, experts - is final
    after the MoE backward); no state over the backbone; one bucket."""
    from medmoe_amd.engine import Engine
    cfg = _cfg(vit_lora=False, freeze_vit=True)
    eng = Engine(cfg, "cpu")
    p = eng.params
    tail = p.numel - p.offsets["moe.router.0.weight"]
    assert eng.vit_frozen and eng.vlora is None and p.train_from == p.offsets["moe.router.0.weight"] and p.n_train == tail
    assert all(b.numel() == tail for b in (p.g32, p.m, p.v)) and p.p32.numel() == p.numel and p.e32 is None and p._g16 is None
    assert eng.bucket_bounds == [0, tail] and set(eng.optimizer_stores()) == {"vit"}
    for n in ("vit.final_layer_norm.weight", "vit.layer.0.attention.input_proj.weight", "vit.pos_embed"):
        with pytest.raises(KeyError, match="frozen"):
            p.grad(n)
    seen = []
    inner = eng._wgrad
    eng._wgrad = lambda *a, **kw: (seen.append(a[2]), inner(*a, **kw))[1]
    out, n = _step(eng, stub)
    assert set(out) >= {"loss", "l_loss", "g_loss"}
    # the experts' two weight gradients per stage through Engine._wgrad, the local loss' one launch next to it: nothing of the tower
    assert n.count("medmoe_gemm_tn") == 8 + 1 and len(seen) == 8
    lo, hi = p.g32.data_ptr(), p.g32.data_ptr() + 4 * tail
    assert all(lo <= t.data_ptr() < hi for t in seen)
    assert n.count("medmoe_layernorm_bwd") == 0 and n.count("medmoe_attn_bwd") == 0 and n.count("medmoe_pos_cls_grad") == 0
    assert n.count("medmoe_broadcast_tokens") == 0 and n.count("medmoe_stage_grad_add") == 0
    assert n.count("medmoe_adam_step") == 1 and n.count("medmoe_sumsq_det") == 1
    assert n.count("medmoe_attn_fwd") == cfg.n_layer_v                 # the forward as ever (the frozen text tower runs its packed form)


@pytest.mark.parametrize("mode", ["none", "selective", "full"])
def test_engine_launch_sequence_with_vit_adapters(stub, mode):
    """vit_lora: per image layer one adapter forward launch right behind the input_proj GEMM; in the backward one d x and one
    weight-gradient launch behind the layer's attention backward; no weight-gradient GEMM, LayerNorm parameter sum or embedding backward of
    the tower; at layer 0 neither the base dgrad GEMM nor the first LayerNorm's backward; the optimiser steps two arenas."""
    from medmoe_amd.engine import Engine
    from medmoe_amd.text_lora import LoraStore
    cfg = _cfg(vit_lora_r=4, vit_lora_dropout=0.1, vit_checkpoint=mode)
    eng = Engine(cfg, "cpu")
    L, nt = cfg.n_layer_v, 2
    lo = eng.vlora
    assert isinstance(lo, LoraStore) and lo.prefix == "vit." and lo.targets == ("query", "value") and (lo.r, lo.D, lo.L) == (4, cfg.d_v, L)
    assert lo.numel == L * nt * 2 * 16 * cfg.d_v and eng.lora is None and not eng.train_text
    assert list(eng.optimizer_stores()) == ["vit", "vit_lora"] and eng.optimizer_stores()["vit_lora"] is lo
    assert eng.bucket_bounds == [0, eng.params.n_train]
    out, n = _step(eng, stub)
    fwd_runs = L + (L if mode == "full" else 0)                       # "full" recomputes qkv, and with it the adapter launch
    assert n.count("medmoe_lora_fwd") == fwd_runs and n.count("medmoe_lora_bwd_dx") == L and n.count("medmoe_lora_bwd_wgrad_runs") == L
    assert n.count("medmoe_lora_bwd_wgrad") == 0
    assert n.count("medmoe_gemm_tn") == 8 + 1 and n.count("medmoe_pos_cls_grad") == 0      # the experts' and the local loss' only
    assert n.count("medmoe_layernorm_bwd") == 1 + L + (L - 1)          # final, every feed-forward LayerNorm, every first LayerNorm but layer 0's
    assert n.count("medmoe_attn_bwd") == L
    assert n.count("medmoe_adam_step") == 2 and n.count("medmoe_sumsq_det") == 2
    f = [i for i, x in enumerate(n) if x == "medmoe_lora_fwd"]
    assert all(n[i - 1] == "medmoe_gemm_nt" and n[i + 1] == "medmoe_attn_fwd" for i in f)
    dx = [i for i, x in enumerate(n) if x == "medmoe_lora_bwd_dx"]
    assert all(n[i + 1] == "medmoe_lora_bwd_wgrad_runs" for i in dx)
    assert all(n[i - 1] == "medmoe_gemm_nt" and n[i - 2] == "medmoe_attn_bwd" for i in dx[:-1]) and n[dx[-1] - 1] == "medmoe_attn_bwd"
    assert n[dx[-1] + 2] != "medmoe_layernorm_bwd"
    assert eng.dropout_step == 1 and eng._vit_lora_drop_step is None
    out, n = _step(eng, stub, "eval_step")
    assert n.count("medmoe_lora_fwd") == L and n.count("medmoe_lora_bwd_dx") == 0 and eng.dropout_step == 1


def test_both_towers_adapters_and_graph_refusal(stub, monkeypatch):
    from medmoe_amd.engine import Engine
    eng = Engine(_cfg(text_lora=True), "cpu")
    assert list(eng.optimizer_stores()) == ["vit", "text", "vit_lora"] and eng.lora.prefix == "text." and eng.vlora.prefix == "vit."
    assert eng.lora is not eng.vlora
    out, n = _step(eng, stub)
    assert n.count("medmoe_adam_step") == 3 and n.count("medmoe_lora_bwd_wgrad") == eng.cfg.n_layer_t
    assert n.count("medmoe_lora_bwd_wgrad_runs") == eng.cfg.n_layer_v
    monkeypatch.setenv("MEDMOE_GRAPH", "1")
    with pytest.raises(NotImplementedError, match="vit_lora_dropout"):
        Engine(_cfg(vit_lora_dropout=0.1), "cpu")
    Engine(_cfg(), "cpu")

