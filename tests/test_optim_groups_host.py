"""CPU tests of the grouped optimiser's host side (no launch computes anything: the stub library of tests/test_host_logic.py): the run
table `FlatArena.set_param_groups` builds, the rule set of medmoe_amd/optim_groups.py on every store kind, which entry point a step issues,
and the new configuration keys."""
import ctypes
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _StubLib:
    def __init__(self):
        self.calls, self.args = [], []

    def __getattr__(self, name):
        if not name.startswith("medmoe_"):
            raise AttributeError(name)

        def f(*a):
            self.calls.append(name)
            self.args.append(a)
            if name == "medmoe_local_geometry":
                HW, T = a[0].value, a[1].value
                a[2]._obj.value = (HW + 15) // 16 * 16; a[3]._obj.value = (T + 15) // 16 * 16
                a[4]._obj.value = (((HW + 15) // 16) + 1) // 2 * 32
            if name == "medmoe_local_fast_path":
                nht, ntt = (a[0].value + 15) // 16, (a[1].value + 15) // 16
                return int((nht == 4 and ntt == 1) or (nht in (13, 16) and 1 <= ntt <= 5))
            if name == "medmoe_local_pair3_supported":
                HW, ntt = a[0].value, (a[1].value + 15) // 16
                return int((HW == 64 and ntt == 1) or (HW == 196 and 1 <= ntt <= 5))
            return 0
        return f


@pytest.fixture
def stub(monkeypatch):
    from medmoe_amd import _lib, ops
    lib = _StubLib()
    monkeypatch.setattr(_lib, "_LIB", lib)
    monkeypatch.setattr(ops, "load_library", lambda: lib)
    monkeypatch.setattr(ops, "_require_gpu", lambda t, name: None)
    monkeypatch.setattr(ops, "_stream", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(ops, "_stream_handle", lambda: 0)
    for cache in ("_FN", "_NT_FN", "_TN_FN"):
        monkeypatch.setattr(ops, cache, {})
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    return lib


def _layout_tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("record_store_layouts", os.path.join(ROOT, "tools", "record_store_layouts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _swin_t_names():
    """The floating parameter names of a Swin-T tower (depths 2, 2, 6, 2), shapes of one dimension where the model has them."""
    names = {"embeddings.patch_embeddings.projection.weight": (96, 3, 4, 4), "embeddings.patch_embeddings.projection.bias": (96,),
             "embeddings.norm.weight": (96,), "embeddings.norm.bias": (96,), "layernorm.weight": (768,), "layernorm.bias": (768,)}
    for s, depth in enumerate((2, 2, 6, 2)):
        C = 96 * 2 ** s
        for b in range(depth):
            pre = f"encoder.layers.{s}.blocks.{b}."
            for n in ("q_proj", "k_proj", "v_proj", "o_proj"):
                names[pre + f"attention.{n}.weight"] = (C, C); names[pre + f"attention.{n}.bias"] = (C,)
            names[pre + "attention.relative_position_bias.relative_position_bias_table"] = (169, 3 * 2 ** s)
            for n in ("layernorm_before", "layernorm_after"):
                names[pre + n + ".weight"] = (C,); names[pre + n + ".bias"] = (C,)
            names[pre + "mlp.fc1.weight"] = (4 * C, C); names[pre + "mlp.fc1.bias"] = (4 * C,)
            names[pre + "mlp.fc2.weight"] = (C, 4 * C); names[pre + "mlp.fc2.bias"] = (C,)
        if s < 3:
            pre = f"encoder.layers.{s}.downsample."
            names[pre + "reduction.weight"] = (2 * C, 4 * C); names[pre + "norm.weight"] = (4 * C,); names[pre + "norm.bias"] = (4 * C,)
    return names


class _Names:
    """What build_assign reads of a store: offsets (the names), groups, shapes."""

    def __init__(self, shapes):
        self.shapes, self.offsets, self.groups = dict(shapes), {n: 0 for n in shapes}, {}


# ---- 7. run-table construction ------------------------------------------------------------------------------------------------------------
def test_run_table_construction(stub):
    from medmoe_amd.flat import FlatArena
    # storage order: the group's members first, back to back (a: 0..3, b: 3..8, padded to 8), then c: 8..45 (pad to 48), d: 48..90 (pad
    # to 96), e: 96..102 (pad to 104)
    ar = FlatArena("cpu", [("c", (37,)), ("a", (3,)), ("d", (6, 7)), ("b", (5,)), ("e", (6,))], groups=[("ab", ["a", "b"])])
    assert (ar.offsets["a"], ar.offsets["b"], ar.offsets["c"], ar.offsets["d"], ar.offsets["e"], ar.numel) == (0, 3, 8, 48, 96, 104)
    assert ar.runs is None
    ar.set_param_groups({"a": (1.0, 0.0), "d": (0.5, 1.0), "e": (0.5, 1.0)})
    # a | b + c (equal values merge; b's and c's padding travel with them) | d + e (merged; the last end is numel)
    assert ar.runs == [(3, 1.0, 0.0), (48, 1.0, 1.0), (104, 0.5, 1.0)]
    ends, lrm, wdm = ar._run_table
    assert ends.dtype == torch.int64 and ends.tolist() == [3, 48, 104] and lrm.dtype == torch.float32 and lrm.tolist() == [1.0, 1.0, 0.5]
    assert wdm.tolist() == [0.0, 1.0, 1.0]
    # an unaligned boundary between two members of one group; the padding behind c belongs to c's run
    ar.set_param_groups({"b": (0.25, 1.0), "c": (1.0, 0.0)})
    assert ar.runs == [(3, 1.0, 1.0), (8, 0.25, 1.0), (48, 1.0, 0.0), (104, 1.0, 1.0)]
    assert ar.runs[0][0] % 4 == 3
    # a group alias covers all its members; a member's own entry wins over the alias
    ar.set_param_groups({"ab": (0.5, 0.0)})
    assert ar.runs == [(8, 0.5, 0.0), (104, 1.0, 1.0)]
    ar.set_param_groups({"ab": (0.5, 0.0), "b": (1.0, 1.0)})
    assert ar.runs == [(3, 0.5, 0.0), (104, 1.0, 1.0)]
    ar.set_param_groups({})
    assert ar.runs == [(104, 1.0, 1.0)]
    with pytest.raises(KeyError, match="nope"):
        ar.set_param_groups({"nope": (1.0, 1.0)})
    ar.clear_param_groups()
    assert ar.runs is None and ar._run_table is None


def test_run_tables_of_the_real_stores_end_at_numel(stub):
    from medmoe_amd.optim_groups import GroupRules, apply_rules
    st = _layout_tool().build_stores()
    rules = GroupRules(no_decay_1d=True, layer_decay=0.75)
    stores = {"vit": st["ParamStore:tiny"], "text": st["TextStore:tiny"], "swin_tower": st["FlatStore:swin-tiny"], "swin_moe": st["FlatStore:grouped-pyramid"]}
    apply_rules(stores, rules)
    for kind, s in stores.items():
        ends = [r[0] for r in s.runs]
        assert ends == sorted(set(ends)) and ends[-1] == s.numel and len(ends) > 1, kind
        assert all(a[1:] != b[1:] for a, b in zip(s.runs, s.runs[1:])), kind        # adjacent equal runs were merged
    # the experts' biases [Do] lie back to back in the pyramid arena: no-decay runs between decayed GEMM weights
    assert any(r[2] == 0.0 for r in stores["swin_moe"].runs) and any(r[2] == 1.0 for r in stores["swin_moe"].runs)
    apply_rules(stores, GroupRules())
    assert all(s.runs is None for s in stores.values())


# ---- 8. rules -----------------------------------------------------------------------------------------------------------------------------
def test_layer_decay_multipliers(stub):
    from medmoe_amd.config import config_by_name
    from medmoe_amd.optim_groups import GroupRules, build_assign
    from medmoe_amd.params import ParamStore
    from medmoe_amd.text_params import TextStore
    cfg = config_by_name("tiny")
    cfg.n_layer_v = 2
    ps = ParamStore(cfg, "cpu")
    ts = TextStore(cfg, "cpu", ps.text)                              # 4 text layers
    sw = _Names(_swin_t_names())
    d = 0.75
    a = build_assign({"vit": ps, "text": ts, "swin_tower": sw}, GroupRules(layer_decay=d, text_lr_mult=0.1))
    vit, text, swin = a["vit"], a["text"], a["swin_tower"]
    lr = lambda asg, n: asg.get(n, (1.0, 1.0))[0]
    # ViT, L = 2: embeddings depth 0 -> d^3, block k -> d^(2 - k), the head exactly 1
    for n in ("vit.patch_embed.weight", "vit.patch_embed.bias", "vit.cls_token", "vit.pos_embed"):
        assert lr(vit, n) == d ** 3, n
    assert lr(vit, "vit.layer.0.attention.input_proj.weight") == d ** 2 and lr(vit, "vit.layer.1.feedforward.model.2.bias") == d
    for n in ps.shapes:
        if n.startswith(("moe.", "vit.final_layer_norm")):
            assert lr(vit, n) == 1.0 and n not in vit, n
    assert min(lr(vit, n) for n in ps.shapes) == d ** 3
    # text tower, L = 4: composes with text_lr_mult
    assert lr(text, "word_embeddings") == pytest.approx(0.1 * d ** 5) and lr(text, "emb_layernorm.bias") == pytest.approx(0.1 * d ** 5)
    for i in range(4):
        assert lr(text, f"layer.{i}.attention.output_proj.weight") == pytest.approx(0.1 * d ** (4 - i))
    assert min(v[0] for v in text.values()) == lr(text, "position_embeddings")
    # Swin-T: 12 blocks, block ordinal k -> d^(12 - k); a stage's patch merging shares the depth of the stage's last block
    k = 0
    for s, depth in enumerate((2, 2, 6, 2)):
        for b in range(depth):
            assert lr(swin, f"encoder.layers.{s}.blocks.{b}.mlp.fc1.weight") == d ** (12 - k), (s, b)
            assert lr(swin, f"encoder.layers.{s}.blocks.{b}.attention.q_proj.bias") == d ** (12 - k), (s, b)
            k += 1
        if s < 3:
            assert lr(swin, f"encoder.layers.{s}.downsample.reduction.weight") == d ** (13 - k), s
    assert lr(swin, "embeddings.norm.weight") == d ** 13 == min(lr(swin, n) for n in sw.shapes)
    assert lr(swin, "layernorm.weight") == 1.0
    # the expert arena of the Swin model sits behind the tower
    moe = _layout_tool().build_stores()["FlatStore:grouped-pyramid"]
    assert build_assign({"swin_moe": moe}, GroupRules(layer_decay=d))["swin_moe"] == {}


def test_no_decay_rules(stub):
    from medmoe_amd.optim_groups import GroupRules, build_assign
    st = _layout_tool().build_stores()
    stores = {"vit": st["ParamStore:tiny"], "text": st["TextStore:tiny"], "swin_tower": _Names(_swin_t_names()), "swin_moe": st["FlatStore:grouped-pyramid"]}
    a = build_assign(stores, GroupRules(no_decay_1d=True))
    for kind, s in stores.items():
        for n in s.offsets:
            if n in s.groups:
                continue
            want = (n.endswith(".bias") or "layernorm" in n or "layer_norm" in n or ".norm." in n
                    or n in ("vit.cls_token", "vit.pos_embed", "position_embeddings", "token_type_embeddings")
                    or n.endswith("relative_position_bias_table"))
            assert (a[kind].get(n, (1.0, 1.0))[1] == 0.0) == want, (kind, n)
            if want:
                assert a[kind][n][0] == 1.0
    assert a["text"].get("word_embeddings") is None and a["vit"].get("moe.attn2.weight") is None
    assert a["vit"]["moe.proj.0.bias"] == (1.0, 0.0)                # stacked [E, Do]: a bias all the same
    # explicit patterns, over each store's own names
    b = build_assign(stores, GroupRules(no_decay=("vit.layer.*.feedforward.*", "word_embeddings")))
    assert b["vit"]["vit.layer.0.feedforward.model.0.weight"] == (1.0, 0.0) and "vit.layer.0.attention.input_proj.weight" not in b["vit"]
    assert b["text"] == {"word_embeddings": (1.0, 0.0)} and b["swin_tower"] == {}
    with pytest.raises(ValueError, match="vit.layr"):
        build_assign(stores, GroupRules(no_decay=("vit.layr.*", "word_embeddings")))


# ---- 9. dispatch --------------------------------------------------------------------------------------------------------------------------
def _stores():
    tool = _layout_tool()
    from medmoe_amd.config import config_by_name
    from medmoe_amd.flat import FlatStore
    from medmoe_amd.params import ParamStore
    from medmoe_amd.text_params import TextStore
    ps = ParamStore(config_by_name("tinyL8mx"), "cpu")
    return [("ParamStore", ps, ["medmoe_transpose_many"] + ["medmoe_quant_weights_mx"] * 5, "moe.router.0.bias"),
            ("TextStore", TextStore(config_by_name("tiny"), "cpu", ParamStore(config_by_name("tiny"), "cpu").text), ["medmoe_transpose_many"], "emb_layernorm.bias"),
            ("FlatStore", tool.build_stores()["FlatStore:grouped-pyramid"], ["medmoe_transpose_many"], "moe.stack.attn_proj.0.bias"),
            ("FlatStore:no-gemm", FlatStore({"a": torch.zeros(5, 3), "b": torch.zeros(7)}, "cpu"), [], "b")]


def test_default_step_issues_the_plain_kernel_and_groups_issue_one_grouped_launch(stub):
    for label, st, tail, name in _stores():
        del stub.calls[:]
        st.adam_step(st.sumsq(), 1e-4, 0.0, 0.25)
        assert stub.calls == ["medmoe_sumsq_det", "medmoe_adam_step"] + tail, label
        # AdamW without groups: a one-run table
        del stub.calls[:], stub.args[:]
        st.adam_step(st.sumsq(), 1e-4, 0.05, 0.25, decoupled=True)
        assert stub.calls == ["medmoe_sumsq_det", "medmoe_adam_groups_step"] + tail, label
        a = stub.args[1]
        assert a[0] == st.p32.data_ptr() and a[5] == st.numel and a[9] == 1 and a[15] == 1 and a[16] == st.step_count, label
        assert st._one_run[0].tolist() == [st.numel] and a[6] == st._one_run[0].data_ptr()
        # other betas / eps alone leave the plain entry point too
        for kw in (dict(betas=(0.9, 0.98)), dict(eps=1e-6)):
            del stub.calls[:]
            st.adam_step(st.sumsq(), 1e-4, 0.0, 0.25, **kw)
            assert stub.calls == ["medmoe_sumsq_det", "medmoe_adam_groups_step"] + tail, (label, kw)
        # groups with plain Adam: the arena's table, decoupled 0, betas and eps as given
        st.set_param_groups({name: (0.5, 0.0)})
        del stub.calls[:], stub.args[:]
        st.adam_step(st.sumsq(), 1e-4, 0.05, 0.25)
        assert stub.calls == ["medmoe_sumsq_det", "medmoe_adam_groups_step"] + tail, label
        a = stub.args[1]
        assert a[6] == st._run_table[0].data_ptr() and a[7] == st._run_table[1].data_ptr() and a[8] == st._run_table[2].data_ptr()
        assert a[9] == len(st.runs) >= 2 and a[15] == 0 and (a[10], a[11], a[12], a[13], a[14]) == (1e-4, 0.9, 0.999, 1e-8, 0.05), label
        st.clear_param_groups()
        del stub.calls[:]
        st.adam_step(st.sumsq(), 1e-4, 0.0, 0.25)
        assert stub.calls == ["medmoe_sumsq_det", "medmoe_adam_step"] + tail, label


def test_engine_default_step_has_no_grouped_launch_and_a_rule_set_has_one_per_store(stub):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import medmoe_oracle as O
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    cfg = config_by_name("tiny")
    cfg.freeze_text = False
    eng = Engine(cfg, "cpu")
    assert eng.params.runs is None and eng.tstore.runs is None
    batch = O.synthetic_batch(O.config_by_name("tiny"), 8, min_len=4)
    del stub.calls[:]
    eng.train_step(batch)
    default = list(stub.calls)
    assert "medmoe_adam_groups_step" not in default and default.count("medmoe_adam_step") == 2
    cfg2 = config_by_name("tiny")
    cfg2.freeze_text, cfg2.optimizer, cfg2.adam_betas, cfg2.adam_eps = False, "adamw", (0.9, 0.98), 1e-6
    cfg2.no_decay_1d, cfg2.layer_decay, cfg2.text_lr_mult, cfg2.weight_decay = True, 0.75, 0.5, 0.05
    eng2 = Engine(cfg2, "cpu")
    assert len(eng2.params.runs) > 8 and len(eng2.tstore.runs) > 8
    del stub.calls[:], stub.args[:]
    eng2.train_step(batch)
    assert [("medmoe_adam_step" if n == "medmoe_adam_groups_step" else n) for n in stub.calls] == default
    got = [a for n, a in zip(stub.calls, stub.args) if n == "medmoe_adam_groups_step"]
    assert len(got) == 2 and [a[0] for a in got] == [eng2.params.p32.data_ptr(), eng2.tstore.p32.data_ptr()]
    assert all((a[11], a[12], a[13], a[14], a[15]) == (0.9, 0.98, 1e-6, 0.05, 1) for a in got)
    # regrouping through the engine; back to the defaults the step is the plain one again
    eng2.set_optimizer_groups(no_decay_1d=False, layer_decay=1.0, text_lr_mult=1.0)
    assert eng2.params.runs is None and eng2.tstore.runs is None
    eng2.set_optimizer_groups(text_lr_mult=0.1)
    assert eng2.params.runs is None and eng2.tstore.runs == [(eng2.tstore.numel, pytest.approx(0.1), 1.0)]
    with pytest.raises(KeyError):
        eng2.set_optimizer_groups(lr_decay=0.5)


# ---- 10. config ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,value", [("optimizer", "sgd"), ("optimizer", "AdamW"), ("adam_betas", (1.0, 0.999)), ("adam_betas", (0.9, -0.1)),
                                         ("adam_betas", (0.9,)), ("adam_eps", 0.0), ("adam_eps", -1e-8), ("layer_decay", 0.0),
                                         ("layer_decay", -0.5), ("text_lr_mult", 0.0), ("text_lr_mult", -1.0), ("no_decay", "vit.*")])
def test_validate_rejects(field, value):
    from medmoe_amd.config import config_by_name
    cfg = config_by_name("tiny")
    cfg.validate()
    assert (cfg.optimizer, cfg.adam_betas, cfg.adam_eps, cfg.no_decay, cfg.no_decay_1d, cfg.text_lr_mult, cfg.layer_decay) == \
        ("adam", (0.9, 0.999), 1e-8, (), False, 1.0, 1.0)
    setattr(cfg, field, value)
    with pytest.raises(ValueError, match=field):
        cfg.validate()


def test_validate_accepts_the_new_experiment_keys():
    from medmoe_amd.config import config_by_name
    cfg = config_by_name("cfg2")
    cfg.optimizer, cfg.adam_betas, cfg.adam_eps, cfg.weight_decay, cfg.no_decay_1d, cfg.layer_decay = "adamw", (0.9, 0.98), 1e-6, 0.05, True, 0.75
    cfg.validate()
    assert math.isclose(cfg.layer_decay ** 13, 0.75 ** 13)


def test_new_experiment_composes_and_existing_ones_are_unchanged(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    from medmoe_amd.hydra_lite import compose
    configs = os.path.join(ROOT, "configs")
    c = compose(configs, "train.yaml", ["experiment=pretraining_medmoe_cfg2_adamw"])
    o = c.model.optimizer
    assert (o._target_, list(o.betas), o.eps, o.weight_decay, o.lr) == ("torch.optim.AdamW", [0.9, 0.98], 1e-6, 0.05, 5e-5)
    g = c.model.optimizer_groups
    assert g.no_decay_1d is True and g.layer_decay == 0.75 and c.model.fused_step is True and c.data.batch_size == 1024
    base = compose(configs, "train.yaml", ["experiment=pretraining_medmoe_cfg2"])
    assert "optimizer_groups" not in base.model and base.model.optimizer._target_ == "torch.optim.Adam"
