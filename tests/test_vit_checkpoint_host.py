"""Activation recomputation of the ViT tower (cfg.vit_checkpoint), host side (no GPU): the config field, the Hydra key and the
environment variable, the refusals, the buffer plan against its closed forms, and the engine's launch sequence and workspace against a stub
library that computes nothing (the fixture of tests/test_vit_drop_path_host.py).

The closed forms, in units of M d_v bf16 values (M = B n_tok_v) with f = ff_v / d_v, from what a mode keeps per layer and what it recomputes
into the TWO shared sets (x 1, ln1 1, qkv 3, att 1, xmid 1, ln2 1, z f, h f):
    none       L (8 + 2 f)                     + x{L}
    selective  L 6  (x qkv att xmid)           + 2 (2 + 2 f)  (ln1 ln2 z h)           + x{L}
    full       L 1  (x)                        + 2 (7 + 2 f)  (ln1 qkv att xmid ln2 z h) + x{L}
At f = 4 (cfg3, every ViT of BASELINE) these are 16, 6 + 2 x 10, 1 + 2 x 15; `tiny` has f = 2.  Every mode adds the statistics
(2 x [2, M] fp32 per layer) and lse ([B n_head n_tok] fp32 per layer) as they are."""
import os
import re

import pytest
import torch

from test_vit_drop_path_host import _batch, _launches, stub  # noqa: F401  (stub: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("none", "selective", "full")


def _cfg(name="tiny2", **kw):
    from medmoe_amd.config import config_by_name
    c = config_by_name(name)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


# ------------------------------------------------------------------------------------------------------------------------------------------
# config, Hydra, environment
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_default_is_none_and_validate_rejects_other_names():
    from medmoe_amd.config import MedMoEConfig
    assert MedMoEConfig().vit_checkpoint == "none"
    for mode in MODES:
        _cfg(vit_checkpoint=mode).validate()
    for bad in ("half", "", True, None):
        with pytest.raises(ValueError, match=r"vit_checkpoint.*model\.model\.vision\.grad_checkpointing"):
            _cfg(vit_checkpoint=bad).validate()


def test_hydra_key_reaches_the_config_and_an_absent_key_changes_nothing():
    import dataclasses
    from src.models.components.med_moe import config_from_hydra
    for vision in ({"config_name": "tiny2"}, {"arch": "vit_l14_336", "num_experts": 8, "top_k": 2}):
        base = config_from_hydra(dict(vision), {})
        assert base.vit_checkpoint == "none"
        assert config_from_hydra(dict(vision, grad_checkpointing=False), {}).vit_checkpoint == "none"
        assert config_from_hydra(dict(vision, grad_checkpointing=True), {}).vit_checkpoint == "full"
        for mode in MODES:
            assert config_from_hydra(dict(vision, grad_checkpointing=mode), {}).vit_checkpoint == mode
        on = config_from_hydra(dict(vision, grad_checkpointing=True), {})
        on.validate()
        on.vit_checkpoint = "none"
        assert dataclasses.asdict(on) == dataclasses.asdict(base)
    with pytest.raises(ValueError, match="vit_checkpoint"):
        config_from_hydra({"config_name": "tiny2", "grad_checkpointing": "half"}, {}).validate()


def test_environment_variable_switches_it_on(monkeypatch):
    monkeypatch.delenv("MEDMOE_VIT_CHECKPOINT", raising=False)
    assert _cfg().vit_checkpoint_mode() == "none" and _cfg(vit_checkpoint="selective").vit_checkpoint_mode() == "selective"
    for mode in ("selective", "full"):
        monkeypatch.setenv("MEDMOE_VIT_CHECKPOINT", mode)
        assert _cfg().vit_checkpoint_mode() == mode
    monkeypatch.setenv("MEDMOE_VIT_CHECKPOINT", "half")
    with pytest.raises(ValueError, match="MEDMOE_VIT_CHECKPOINT"):
        _cfg().vit_checkpoint_mode()


def test_environment_variable_reaches_the_engine(stub, monkeypatch):
    from medmoe_amd.engine import Engine
    monkeypatch.setenv("MEDMOE_VIT_CHECKPOINT", "selective")
    eng = Engine(_cfg(), "cpu")
    assert eng.vit_checkpoint == "selective"
    eng._alloc(2)
    assert "ck1_h" in eng.ws and "h0" not in eng.ws and "qkv0" in eng.ws


def test_example_experiment_composes_to_full(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    from medmoe_amd.hydra_lite import compose
    from src.models.components.med_moe import config_from_hydra
    base = compose(os.path.join(ROOT, "configs"), "train.yaml", ["experiment=pretraining_medmoe_cfg3"])
    assert config_from_hydra(base.model.model.vision, base.model.model.text).vit_checkpoint == "none"
    on = compose(os.path.join(ROOT, "configs"), "train.yaml", ["experiment=pretraining_medmoe_cfg3_ckpt"])
    c = config_from_hydra(on.model.model.vision, on.model.model.text)
    assert c.vit_checkpoint == "full" and (c.n_layer_v, c.d_v, c.img_size) == (24, 1024, 336)
    sel = compose(os.path.join(ROOT, "configs"), "train.yaml", ["experiment=pretraining_medmoe_cfg2", "+model.model.vision.grad_checkpointing=selective"])
    assert config_from_hydra(sel.model.model.vision, sel.model.model.text).vit_checkpoint == "selective"


def test_swin_tower_refuses_the_key():
    from src.models.components.med_moe import config_from_hydra
    assert config_from_hydra({"arch": "swin_t"}, {}).vit_checkpoint == "none"
    assert config_from_hydra({"arch": "swin_t", "grad_checkpointing": False}, {}).vit_checkpoint == "none"
    for key in (True, "selective"):
        with pytest.raises(NotImplementedError, match=r"vit_checkpoint.*model\.model\.vision\.grad_checkpointing.*swin_t.*Swin tower"):
            config_from_hydra({"arch": "swin_t", "grad_checkpointing": key}, {})


def test_graph_mode_is_refused_and_names_both_keys(stub, monkeypatch):
    from medmoe_amd.engine import Engine
    monkeypatch.setenv("MEDMOE_GRAPH", "1")
    assert Engine(_cfg(), "cpu").vit_checkpoint == "none"                        # none: graphs as before
    for mode in ("selective", "full"):
        with pytest.raises(NotImplementedError, match=r"vit_checkpoint.*model\.model\.vision\.grad_checkpointing.*MEDMOE_GRAPH=1.*not been verified"):
            Engine(_cfg(vit_checkpoint=mode), "cpu")


def test_header_declares_layernorm_apply():
    hdr = open(os.path.join(ROOT, "include", "medmoe_hip.h")).read()
    from medmoe_amd import ops
    m = re.search(r"^int medmoe_layernorm_apply\((.*)\);", hdr, re.M)
    assert m and len(m.group(1).split(",")) == len(ops._SIGS["layernorm_apply"]) + 1          # + the stream


def test_wrapper_refuses_bad_shapes(stub):
    from medmoe_amd import ops
    BF = torch.bfloat16

    def args(rows, D, n_stat=None, n_g=None, ydt=BF):
        return (torch.zeros(rows, D, dtype=BF), torch.zeros(n_stat or rows), torch.ones(n_stat or rows), torch.ones(n_g or D), torch.zeros(n_g or D),
                torch.zeros(rows, D, dtype=ydt))
    ops.layernorm_apply(*args(5, 2048))
    assert stub.calls.count("medmoe_layernorm_apply") == 1
    for a in (args(5, 132), args(5, 2056), args(5, 128, n_stat=4), args(5, 128, n_g=64)):
        with pytest.raises(ValueError, match="layernorm_apply"):
            ops.layernorm_apply(*a)
    with pytest.raises((ValueError, TypeError)):
        ops.layernorm_apply(*args(5, 128, ydt=torch.float32))
    assert stub.calls.count("medmoe_layernorm_apply") == 1


# ------------------------------------------------------------------------------------------------------------------------------------------
# the buffer plan
# ------------------------------------------------------------------------------------------------------------------------------------------
def _closed_form(c, B, mode):
    L, D, M = c.n_layer_v, c.d_v, B * c.n_tok_v
    assert c.ff_v % D == 0
    f = c.ff_v // D
    unit = M * D * 2
    per_layer, shared = {"none": (8 + 2 * f, 0), "selective": (6, 2 + 2 * f), "full": (1, 7 + 2 * f)}[mode]
    stats = L * (2 * 2 * M * 4 + B * c.n_head_v * c.n_tok_v * 4)
    return L * per_layer * unit + 2 * shared * unit + unit + stats


@pytest.mark.parametrize("name,B", [("tiny", 5), ("cfg3", 64), ("cfg3", 3)])
def test_plan_bytes_equal_the_closed_forms(name, B):
    from medmoe_amd.engine import plan_bytes, vit_activation_plan
    c = _cfg(name)
    assert c.n_layer_v == {"tiny": 4, "cfg3": 24}[name]
    got = {m: plan_bytes(vit_activation_plan(c, B, m)) for m in MODES}
    for m in MODES:
        assert got[m] == _closed_form(c, B, m), (m, got[m])
    assert got["full"] < got["selective"] < got["none"]
    if name == "cfg3":                                                            # ff = 4 d_v: the constants of the issue
        L, unit = 24, B * 577 * 1024 * 2
        stats = L * (16 * B * 577 + 4 * B * 16 * 577)
        assert got["none"] == L * 16 * unit + unit + stats
        assert got["selective"] == L * 6 * unit + 2 * 10 * unit + unit + stats
        assert got["full"] == L * 1 * unit + 2 * 15 * unit + unit + stats


def test_plan_orders_the_modes_from_three_layers_on():
    from medmoe_amd.engine import plan_bytes, vit_activation_plan
    for L in (3, 4, 12):
        c = _cfg("cfg2", n_layer_v=L)
        b = [plan_bytes(vit_activation_plan(c, 7, m)) for m in ("full", "selective", "none")]
        assert b[0] < b[1] < b[2], (L, b)
    with pytest.raises(ValueError, match="vit_checkpoint"):
        vit_activation_plan(_cfg(), 4, "half")


def test_plan_of_mode_none_is_the_workspace_as_it_was():
    from medmoe_amd.engine import vit_activation_plan
    c = _cfg()
    L = c.n_layer_v
    names = [f"x{l}" for l in range(L + 1)]
    for l in range(L):
        names += [f"ln1_{l}", f"st1_{l}", f"qkv{l}", f"att{l}", f"lse{l}", f"xmid{l}", f"ln2_{l}", f"st2_{l}", f"z{l}", f"h{l}"]
    assert list(vit_activation_plan(c, 3, "none")) == names
    for m in ("selective", "full"):
        plan = vit_activation_plan(c, 3, m)
        for l in range(L):                                                        # always kept
            assert {f"x{l}", f"st1_{l}", f"st2_{l}", f"lse{l}"} <= set(plan)
            assert (f"qkv{l}" in plan) == (f"att{l}" in plan) == (f"xmid{l}" in plan) == (m == "selective")
            assert not {f"ln1_{l}", f"ln2_{l}", f"z{l}", f"h{l}"} & set(plan)
        assert {"ck0_h", "ck1_h", "ck0_ln1", "ck1_z"} <= set(plan) and ("ck0_qkv" in plan) == (m == "full")


@pytest.mark.parametrize("mode", MODES)
def test_workspace_is_built_from_the_plan(stub, mode):
    from medmoe_amd.engine import Engine, plan_bytes, vit_activation_plan
    eng = Engine(_cfg(vit_checkpoint=mode), "cpu")
    eng._alloc(5)
    plan = vit_activation_plan(eng.cfg, 5, mode)
    assert all(tuple(eng.ws[n].shape) == tuple(s) and eng.ws[n].dtype == dt for n, (s, dt) in plan.items())
    assert sum(eng.ws[n].numel() * eng.ws[n].element_size() for n in plan) == plan_bytes(plan)
    legacy = set(vit_activation_plan(eng.cfg, 5, "none"))
    assert {n for n in eng.ws if n in legacy or n.startswith("ck")} == set(plan)      # and nothing of another mode's


# ------------------------------------------------------------------------------------------------------------------------------------------
# launch sequences
# ------------------------------------------------------------------------------------------------------------------------------------------
def _step_launches(stub, batch, **kw):
    from medmoe_amd.engine import Engine
    eng = Engine(_cfg(**kw), "cpu")
    del stub.calls[:]
    eng.train_step(batch)
    train = _launches(stub)
    del stub.calls[:]
    eng.eval_step(batch)
    return train, _launches(stub)


@pytest.mark.parametrize("rate", [0.0, 0.5])
def test_launch_sequence_of_every_mode(stub, rate):
    """none: the sequence of an engine that has never heard of the key.  selective: 2 L layernorm_apply and L GEMMs (FC1) more.  full: 2 L
    layernorm_apply (under stochastic depth the layers with a positive rate rerun the fused site for the second one), 3 L GEMMs (QKV, out-proj,
    FC1) and L attention forwards more.  Nothing else changes, and evaluation launches the same in every mode."""
    batch = _batch()
    L = _cfg().n_layer_v
    base, base_eval = _step_launches(stub, batch, vit_drop_path=rate)
    dropped = (L - 1) if rate else 0                                             # layers with p_l > 0
    for mode, n_apply, n_gemm, n_attn, n_site in (("none", 0, 0, 0, 0), ("selective", 2 * L, L, 0, 0),
                                                  ("full", 2 * L - dropped, 3 * L, L, dropped)):
        train, ev = _step_launches(stub, batch, vit_drop_path=rate, vit_checkpoint=mode)
        assert ev == base_eval, mode
        if mode == "none":
            assert train == base
            continue
        want = {"medmoe_layernorm_apply": n_apply, "medmoe_gemm_nt": n_gemm, "medmoe_attn_fwd": n_attn, "medmoe_scale_add_layernorm_fwd": n_site}
        for name in set(base) | set(train):
            assert train.count(name) - base.count(name) == want.get(name, 0), (mode, name)
        # the forward half is the same launches; the first recompute comes after the MoE backward's dgrads, ahead of the last layer's backward
        first = train.index("medmoe_layernorm_apply")
        assert train[:first] == base[:first]
