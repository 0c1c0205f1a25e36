"""Host side of the text tower's dropout (no GPU): a numpy restatement of the mask function of csrc/philox.h, the configuration keys,
the refusals at construction, the checkpoint round trip of the step counter and the host threshold."""
import os
import types
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")
SITE_EMBED = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------------------------
# Philox4x32-10 (Salmon et al., SC'11) and the mask contract of csrc/philox.h, restated in numpy
# ------------------------------------------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """uint32 arrays (or scalars) in, the four output words out"""
    c = [np.asarray(v, dtype=np.uint64) & 0xFFFFFFFF for v in (c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]            # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(0xFFFFFFFF),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(0xFFFFFFFF)]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def keep_mask(rows, cols, cols_padded, seed, step, site, p):
    """bool [rows, cols]: element (row, col) is word col % 4 of group row * cols_padded / 4 + col / 4; key = the halves of the seed,
    counter = (group lo, group hi, site, step); kept iff word >= floor(p * 2^32)"""
    gpr = cols_padded // 4
    group = np.arange(rows * gpr, dtype=np.uint64)
    seed &= 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10(group & np.uint64(0xFFFFFFFF), group >> np.uint64(32), np.full(group.shape, site & 0xFFFFFFFF, np.uint64),
                      np.full(group.shape, step & 0xFFFFFFFF, np.uint64), seed & 0xFFFFFFFF, seed >> 32)
    words = np.stack(w, axis=1).reshape(rows, gpr * 4)[:, :cols]
    return words >= np.uint32(int(Fraction(p) * 2 ** 32))


def test_philox_known_answers():
    """the Random123 known-answer vectors of philox4x32_10"""
    got = [int(v) for v in philox4x32_10(0, 0, 0, 0, 0, 0)]
    assert got == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    got = [int(v) for v in philox4x32_10(f, f, f, f, f, f)]
    assert got == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    got = [int(v) for v in philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)]
    assert got == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_mask_restatement_depends_on_every_input():
    a = keep_mask(5, 20, 20, 1, 2, 3, 0.5)
    assert a.shape == (5, 20) and 0.2 < a.mean() < 0.8
    assert np.array_equal(a, keep_mask(5, 20, 20, 1, 2, 3, 0.5))
    for other in (keep_mask(5, 20, 20, 9, 2, 3, 0.5), keep_mask(5, 20, 20, 1, 9, 3, 0.5), keep_mask(5, 20, 20, 1, 2, 9, 0.5),
                  keep_mask(5, 20, 20, 1 + (1 << 32), 2, 3, 0.5)):
        assert not np.array_equal(a, other)
    assert keep_mask(3, 7, 8, 0, 0, 0, 0.0).all()


# ------------------------------------------------------------------------------------------------------------------------------
# configuration
# ------------------------------------------------------------------------------------------------------------------------------
def test_defaults_are_zero_and_validate_refuses_bad_probabilities():
    from medmoe_amd.config import MedMoEConfig, config_by_name
    c = MedMoEConfig()
    assert (c.text_hidden_dropout, c.text_attn_dropout, c.dropout_seed) == (0.0, 0.0, 0)
    for key in ("text_hidden_dropout", "text_attn_dropout"):
        for bad in (1.0, -0.1):
            c = config_by_name("tiny")
            setattr(c, key, bad)
            with pytest.raises(ValueError, match=key):
                c.validate()
        c = config_by_name("tiny")
        setattr(c, key, 0.999)
        c.validate()


def test_hydra_keys_reach_the_engine_config():
    from medmoe_amd.hydra_lite import compose
    from src.models.components.med_moe import config_from_hydra
    text = {"freeze_bert": False, "hidden_dropout_prob": 0.1, "attention_probs_dropout_prob": 0.2, "dropout_seed": 77}
    for vision in ({"config_name": "tiny"}, {"arch": "vit_b16"}):
        c = config_from_hydra(vision, text)
        assert (c.text_hidden_dropout, c.text_attn_dropout, c.dropout_seed, c.freeze_text) == (0.1, 0.2, 77, False)
        c = config_from_hydra(vision, {"freeze_bert": False})
        assert (c.text_hidden_dropout, c.text_attn_dropout, c.dropout_seed) == (0.0, 0.0, 0)
    os.environ.setdefault("PROJECT_ROOT", ROOT)
    # every shipped experiment keeps 0.0; the keys exist in the model config and can be overridden from the command line
    for exp in sorted(f[:-5] for f in os.listdir(os.path.join(CONFIGS, "experiment"))):
        m = compose(CONFIGS, "train.yaml", [f"experiment={exp}"]).model.model
        c = config_from_hydra(m.vision, m.text)
        assert (c.text_hidden_dropout, c.text_attn_dropout, c.dropout_seed) == (0.0, 0.0, 0), exp
    m = compose(CONFIGS, "train.yaml", ["experiment=pretraining_medmoe_cfg1", "model.model.text.freeze_bert=false",
                                        "model.model.text.hidden_dropout_prob=0.1", "model.model.text.attention_probs_dropout_prob=0.1",
                                        "model.model.text.dropout_seed=5"]).model.model
    c = config_from_hydra(m.vision, m.text)
    assert (c.text_hidden_dropout, c.text_attn_dropout, c.dropout_seed, c.freeze_text) == (0.1, 0.1, 5, False)


@pytest.mark.parametrize("key", ["text_hidden_dropout", "text_attn_dropout"])
def test_refused_with_a_frozen_text_tower(key):
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    c = config_by_name("tiny")
    setattr(c, key, 0.1)
    with pytest.raises(NotImplementedError, match="hidden_dropout_prob.*freeze_bert"):
        Engine(c, "cpu")


def test_refused_with_the_captured_graph_step(monkeypatch):
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    monkeypatch.setenv("MEDMOE_GRAPH", "1")
    c = config_by_name("tiny")
    c.freeze_text, c.text_attn_dropout = False, 0.1
    with pytest.raises(NotImplementedError, match="attention_probs_dropout_prob.*MEDMOE_GRAPH"):
        Engine(c, "cpu")


def test_checkpoint_hooks_round_trip_the_step_counter():
    """the step counter travels next to `fused_adam` (the hooks only touch the engine's counter and the stores' Adam state)"""
    from src.models.medmoe_module import MedMoEPretrainingLightningModule

    def module(step):
        eng = types.SimpleNamespace(dropout_step=step)
        return types.SimpleNamespace(fused_step=True, model=types.SimpleNamespace(engine=eng), _fused_stores=lambda: {})

    src, dst = module(41), module(0)
    ck = {}
    MedMoEPretrainingLightningModule.on_save_checkpoint(src, ck)
    assert ck["text_dropout_step"] == 41 and ck["fused_adam"] == {}
    MedMoEPretrainingLightningModule.on_load_checkpoint(dst, ck)
    assert dst.model.engine.dropout_step == 41
    old = module(3)
    MedMoEPretrainingLightningModule.on_load_checkpoint(old, {"fused_adam": {}})         # a checkpoint from before the counter existed: left alone
    assert old.model.engine.dropout_step == 3


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_host_threshold(p):
    from medmoe_amd import ops
    want = int(Fraction(p) * 2 ** 32)                                   # floor of the exact product of the double p and 2^32
    assert ops.dropout_thresh(p) == want
    seed, step, site, thresh, scale = ops.dropout_rng(3, 4, 5, p)
    assert (seed, step, site, thresh) == (3, 4, 5, want) and scale == 1.0 / (1.0 - p)
    assert ops.dropout_rng((1 << 64) - 1, 0, ops.DROPOUT_SITE_EMBED, p)[:3] == (-1, 0, SITE_EMBED)
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError):
            ops.dropout_thresh(bad)


# ------------------------------------------------------------------------------------------------------------------------------
# launch sequence against the stub library of test_host_logic.py (every launch returns 0, nothing is computed)
# ------------------------------------------------------------------------------------------------------------------------------
from test_host_logic import stub  # noqa: E402,F401  (fixture)


@pytest.mark.parametrize("ph,pa", [(0.1, 0.1), (0.1, 0.0), (0.0, 0.1), (0.0, 0.0)])
def test_launch_sequence_with_dropout(stub, ph, pa):  # noqa: F811
    """per layer: attn_drop_fwd / _bwd where attention dropout is on; two dropout_add_layernorm_fwd launches in place of the two text
    LayerNorm launches and two dropout_apply launches in the backward where hidden dropout is on (+ the embedding site, forward and
    backward); with both at 0.0 none of the new entry points is called; evaluation never calls them; the step counter is a launch argument"""
    import medmoe_oracle as O
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    cfg = config_by_name("tiny")
    cfg.freeze_text, cfg.text_hidden_dropout, cfg.text_attn_dropout, cfg.dropout_seed = False, ph, pa, 9
    eng = Engine(cfg, "cpu")
    ocfg = O.config_by_name("tiny")
    batch = O.synthetic_batch(ocfg, 8, min_len=4)
    Lt, Lv = cfg.n_layer_t, cfg.n_layer_v
    eng.eval_step(batch)
    assert eng.dropout_step == 0 and not [n for n in stub.calls if "drop" in n]
    del stub.calls[:], stub.args[:]
    eng.dropout_step = 6
    eng.train_step(batch)
    n = stub.calls
    assert eng.dropout_step == 7
    assert n.count("medmoe_attn_drop_fwd") == n.count("medmoe_attn_drop_bwd") == (Lt if pa > 0 else 0)
    assert n.count("medmoe_attn_fwd") == n.count("medmoe_attn_bwd") == Lv + (0 if pa > 0 else Lt)
    assert n.count("medmoe_dropout_add_layernorm_fwd") == (2 * Lt if ph > 0 else 0)
    assert n.count("medmoe_dropout_apply") == (2 * Lt + 2 if ph > 0 else 0)
    assert n.count("medmoe_layernorm_fwd") == 2 * Lv + 1 + (0 if ph > 0 else 2 * Lt)
    assert n.count("medmoe_dropout_mask") == 0
    for name, a in zip(n, stub.args):
        if "drop" in name:
            seed, step, site, thresh = a[-6:-2]
            p = pa if name.startswith("medmoe_attn_drop") else ph
            assert (seed, step, thresh) == (9, 6, int(Fraction(p) * 2 ** 32)), name
            if name.startswith("medmoe_attn_drop"):
                assert site % 4 == 0 and site // 4 < Lt, (name, site)
            else:
                assert site == SITE_EMBED or (site % 4 in (1, 2) and site // 4 < Lt), (name, site)
