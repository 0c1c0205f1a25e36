"""The masked-language-model objective in the engine's training step (cfg.text_mlm), tiny configuration (vocabulary 97), and the
reference's MaskedPredictionLoss fixture (tests/golden/mlm_head.npz, tools/gen_golden_mlm.py) through `src.losses` on the GPU path.

Bars.  The head against float64: its activations t and z and the gradients dz, dt, d pre-activation (and dg for d hidden) are stored as bf16,
P is rounded to bf16 for the second product - k roundings of relative size <= 2^-9 along a gradient's path bound its rel-L2 error by
k 2^-9 (k = 6 for the head's parameters, 7 for d hidden, 4 for what sits behind the LayerNorm only); the loss sees t and z only.  Packed against
padded: the loss bar of tests/test_text_varlen_train_gpu.py (PACKED_VS_PADDED["loss"]).  Every test prints what it measured.

The file name sorts behind every other test file on purpose.  tests/test_text_varlen_train_gpu.py::test_packed_against_padded_full_tower holds
two engines' atomically summed losses to 2 x one measured spread (2.5e-7); measured in fresh processes on one MI355X, it failed 0 of 12 times
alone, 0 of 6 behind tests/test_mlm_kernels_gpu.py, and 8 of 12 behind this file (2 of 6 with the allocator emptied after it) - the engines
built here move where later buffers lie, and with that the order of those sums.  Run last, this file precedes nothing (profiles/r23_notes.md)."""
import math
import os

import numpy as np
import pytest
import torch

import mlm_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")
GOLDEN = os.path.join(ROOT, "tests", "golden", "mlm_head.npz")
BF16_STEP = 2.0 ** -9                  # the relative size of one bf16 rounding
PACKED_VS_PADDED_LOSS = 2 * 1.27e-7    # tests/test_text_varlen_train_gpu.py


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_empty():
    yield
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _cfg(mlm=True, **kw):
    from medmoe_amd.config import config_by_name
    c = config_by_name("tiny2")
    c.freeze_text, c.lr = False, 1e-3
    if mlm:
        c.text_mlm, c.mlm_prob, c.mlm_mask_id = True, 0.3, 4
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _engine(mlm=True, seed=0, **kw):
    from medmoe_amd.engine import Engine
    return Engine(_cfg(mlm, **kw), DEV, seed=seed)


def _batch(eng, B=8, seed=21):
    import bench
    return bench.synthetic_batch(eng.cfg, B, seed, eng.device)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def test_step_reports_a_finite_loss_near_ln_v_and_an_accuracy():
    eng = _engine()
    b = _batch(eng)
    out = eng.train_step(b, optimizer=False)
    torch.cuda.synchronize()
    loss, acc, n = float(out["mlm_loss"]), float(out["mlm_acc"]), int(eng.mlm.buf.counts[0])
    print(f"\nmlm_loss {loss:.4f} (ln V {math.log(97):.4f}) mlm_acc {acc:.3f} masked {n}")
    assert n > 10 and math.isfinite(loss) and abs(loss - math.log(97)) < 0.1 * math.log(97) and 0.0 <= acc <= 1.0
    plain = _engine(mlm=False).train_step(b, optimizer=False)
    assert "mlm_loss" not in plain and math.isfinite(float(out["loss"]))
    # the mask the step drew is the host rule's, and the tower ran on the masked ids
    want = R.mlm_mask_ref(b["ids"].cpu().numpy(), b["attn_mask"].cpu().numpy(), cls_id=1, sep_id=2, pad_id=0, mask_id=4, vocab=97, seed=0, step=0, p=0.3)
    ids_masked, labels, rows, row_labels, count = eng._tp.mlm
    assert int(count) == want["count"] == n and np.array_equal(ids_masked.cpu().numpy(), want["ids_masked"])
    assert np.array_equal(rows[:n].cpu().numpy(), want["rows"]) and eng._tp.ids32 is ids_masked and eng.dropout_step == 1


def test_head_alone_drives_the_tower_and_matches_float64():
    """w_cls = w_global = w_local = 0: what reaches the text tower comes from the head.  The head's d hidden and its arena's gradients against a
    float64 restatement from the engine's own last hidden state, rows and labels."""
    zero = dict(w_cls=0.0, w_global=0.0, w_local=0.0)
    off = _engine(mlm=False, **zero)
    b = _batch(off)
    off.train_step(b, optimizer=False)
    assert float(off.tstore.g32.abs().max()) == 0.0                  # nothing else reaches the tower
    eng = _engine(**zero)
    out = eng.train_step(b, optimizer=False)
    torch.cuda.synchronize()
    g = eng.tstore.export_named(eng.tstore.g32)
    assert all(torch.isfinite(v).all() for v in g.values())
    assert float(g["text.word_embeddings"].norm()) > 0 and float(g["text.layer.0.attention.input_proj.weight"].norm()) > 0
    # float64 restatement of the head
    st, buf = eng.mlm.store, eng.mlm.buf
    _, _, rows, row_labels, count = eng._tp.mlm
    n = int(count)
    hid = eng._tp.last.view(-1, eng.cfg.d_t)[rows[:n].long()].double().cpu().requires_grad_(True)
    P = {k: st.f32(k).double().cpu().requires_grad_(True) for k in st.names}
    W = st.w16("cls.dense.weight").double().cpu().requires_grad_(True)                     # the bf16 working copy the GEMM read
    E = eng.tstore.w16("word_embeddings").double().cpu()
    t = torch.nn.functional.gelu(hid @ W.t() + P["cls.dense.bias"])
    z = torch.nn.functional.layer_norm(t, (eng.cfg.d_t,), P["cls.layer_norm.weight"], P["cls.layer_norm.bias"], eng.mlm.eps)
    logits = z @ E.t() + P["cls.bias"]
    loss = torch.nn.functional.cross_entropy(logits, row_labels[:n].long().cpu())
    loss.backward()
    e_loss = abs(float(out["mlm_loss"]) - float(loss.detach())) / float(loss.detach())
    errs = {"d_hidden": rel(buf.dg[:n].cpu(), hid.grad), "cls.dense.weight": rel(st.grad("cls.dense.weight").cpu(), W.grad)}
    errs.update({k: rel(st.grad(k).cpu(), P[k].grad) for k in st.names if k != "cls.dense.weight"})
    print("\nhead against float64: loss", f"{e_loss:.3g}", {k: float(f"{v:.3g}") for k, v in errs.items()})
    assert e_loss < 2 * BF16_STEP
    bars = {"d_hidden": 7, "cls.dense.weight": 6, "cls.dense.bias": 6, "cls.layer_norm.weight": 4, "cls.layer_norm.bias": 4, "cls.bias": 3}
    for k, v in errs.items():
        assert v <= bars[k] * BF16_STEP, (k, v)


def test_padded_and_packed_passes_give_the_same_loss():
    pd, pk = _engine(), _engine(text_train_varlen=True)
    b = _batch(pd)
    a, c = pd.train_step(b, optimizer=False), pk.train_step(b, optimizer=False)
    torch.cuda.synchronize()
    assert pk.text_train_varlen_active and not pd.text_train_varlen_active
    la, lc = float(a["mlm_loss"]), float(c["mlm_loss"])
    n = int(pd.mlm.buf.counts[0])
    print(f"\npadded {la:.7f} packed {lc:.7f} rel {abs(la - lc) / la:.3g}")
    assert int(pk.mlm.buf.counts[0]) == n and abs(la - lc) <= PACKED_VS_PADDED_LOSS * la and float(a["mlm_acc"]) == float(c["mlm_acc"])
    # the packed list names the same tokens
    assert torch.equal(pk._tp.src_row[pk._tp.mlm[2][:n].long()], pd._tp.mlm[2][:n])


def test_two_half_scaled_micro_batches_equal_one_step():
    """The same batch twice at loss_scale 1/2 (the same mask: the step counter is put back) accumulates what one step at loss_scale 1 leaves.
    A factor 1/2 is exact in bf16 and fp32, so only the order of the fp32 atomic sums differs: 1e-4 is far above that and far below any
    missing or doubled scale."""
    one, two = _engine(), _engine()
    b = _batch(one)
    o1 = one.train_step(b, optimizer=False)
    two.train_step(b, optimizer=False, loss_scale=0.5)
    two.dropout_step = 0
    o2 = two.train_step(b, optimizer=False, zero_grad=False, loss_scale=0.5)
    torch.cuda.synchronize()
    assert abs(float(o2["mlm_loss"]) - 0.5 * float(o1["mlm_loss"])) < 1e-6 * float(o1["mlm_loss"])
    errs = {}
    for kind, s1 in one.optimizer_stores().items():
        s2 = two.optimizer_stores()[kind]
        g1, g2 = s1.export_named(s1.g32), s2.export_named(s2.g32)
        errs.update({k: rel(g2[k], g1[k]) for k in g1 if float(g1[k].norm()) > 1e-9})
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:3]
    print("\ntwo halves against one step, worst:", [(k, float(f"{v:.3g}")) for k, v in worst], "n", len(errs))
    assert any(k.startswith("mlm.") for k in errs) and max(errs.values()) < 1e-4, worst


def test_loss_falls_over_thirty_steps_and_evaluation_is_repeatable():
    eng = _engine()
    b = _batch(eng)
    before = eng.mlm_eval(b, step=0)
    again = eng.mlm_eval(b, step=0)
    other = eng.mlm_eval(b, step=1)
    l0 = float(before["mlm_loss"])
    assert float(again["mlm_loss"]) == l0 and float(again["mlm_acc"]) == float(before["mlm_acc"]) and float(other["mlm_loss"]) != l0
    p0, e0 = eng.mlm.store.p32.clone(), eng.tstore.p32.clone()
    assert eng.dropout_step == 0 and not eng.mlm.store.g32.any()      # an evaluation writes no gradient and draws no training mask
    first = last = None
    for it in range(30):
        out = eng.train_step(b)
        first = float(out["mlm_loss"]) if it == 0 else first
        last = float(out["mlm_loss"])
    after = float(eng.mlm_eval(b, step=0)["mlm_loss"])
    torch.cuda.synchronize()
    print(f"\nmlm_loss under the fixed mask of step 0: {l0:.4f} -> {after:.4f}; training steps {first:.4f} -> {last:.4f}")
    assert after < l0 and math.isfinite(after)
    assert not torch.equal(eng.mlm.store.p32, p0) and not torch.equal(eng.tstore.p32, e0) and eng.mlm.store.step_count == 30


def test_evaluation_and_embeddings_do_not_see_the_feature():
    on, off = _engine(), _engine(mlm=False)
    b = _batch(on)
    # every deterministic product of the evaluation pass, bit for bit: both towers' outputs, the MoE's, the router's probabilities
    off.eval_step(b); on.eval_step(b)
    for k in ("img_g", "img_l", "txt_g", "words", "probs"):
        assert torch.equal(off.ws[k], on.ws[k]), k
    # the reported scalars: bit-equal wherever the engine repeats ITSELF bit for bit; a loss whose terms meet in fp32 atomics does not
    # (tests/test_text_varlen_train_gpu.py measured that spread between two runs of one engine: its "loss" bar), and gets that bar
    # Whether an engine repeats itself is judged from six runs of each, not from one repeat: two equal runs of an atomic sum are common and
    # prove nothing (a run of this test saw off == off again in l_loss and the third run one ulp away, with g_loss differing off / off).
    runs_off, runs_on = ([{k: float(v) for k, v in e.eval_step(b).items()} for _ in range(6)] for e in (off, on))
    r0 = runs_off[0]
    print("\neval_step off x 6 / on x 6:", runs_off, runs_on)
    for k in r0:
        if len({r[k] for r in runs_off}) == 1 and len({r[k] for r in runs_on}) == 1:
            assert runs_on[0][k] == r0[k], k
        else:
            assert all(abs(r[k] - r0[k]) <= PACKED_VS_PADDED_LOSS * abs(r0[k]) for r in runs_off + runs_on), k
    ig0, tg0 = (t.clone() for t in off.embed(b))
    ig1, tg1 = on.embed(b)
    assert torch.equal(ig0, ig1) and torch.equal(tg0, tg1)
    assert torch.equal(off.embed_text(b["ids"], b["attn_mask"]).clone(), on.embed_text(b["ids"], b["attn_mask"]))
    assert on._tp.mlm is None and sorted(on.optimizer_stores()) == ["mlm", "text", "vit"] and sorted(off.optimizer_stores()) == ["text", "vit"]
    with pytest.raises(RuntimeError, match="no MLM head"):
        off.mlm_eval(b)


def test_ema_and_parameter_groups_cover_the_head():
    eng = _engine(ema_decay=0.9, no_decay_1d=True, weight_decay=0.1, optimizer="adamw")
    st = eng.mlm.store
    assert st.runs is not None and [r[1:] for r in st.runs] == [(1.0, 1.0), (1.0, 0.0)]       # the dense matrix decays, the 1-d entries do not
    b = _batch(eng)
    eng.train_step(b); eng.train_step(b)
    torch.cuda.synchronize()
    assert st.e32 is not None and st.ema_updates == 2 and not torch.equal(st.e32, st.p32)
    m = eng.mlm_eval(b, step=0)
    e = eng.mlm_eval(b, step=0, ema=True)
    assert float(m["mlm_loss"]) != float(e["mlm_loss"]) and not st.ema_loaded
    assert set(eng.ema_params()) >= {"mlm.cls.dense.weight", "mlm.cls.bias", "text.word_embeddings"}


def test_checkpoint_round_trip_restores_the_head_and_the_optimisation(monkeypatch, tmp_path):
    """The Lightning hooks: a module restored from a checkpoint continues the same optimisation - the head's third step equals the
    uninterrupted run's; restored without the hooks' state (fresh head, fresh moments) it does not.  The bars are those of
    tests/test_fused_module_gpu.py::test_fused_adam_state_travels_with_the_checkpoint."""
    import bench
    from medmoe_amd.hydra_lite import compose, instantiate
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    ov = ["experiment=pretraining_medmoe_cfg2", "model.model.vision.config_name=tiny2", "model.model.text.freeze_bert=false", "model.optimizer.lr=0.001",
          "+model.mlm.prob=0.3", "+model.mlm.mask_token_id=4", "+model.mlm.weight=1.0", "+model.mlm.validate=true"]

    def build():
        lit = instantiate(compose(CONFIGS, "train.yaml", ov).model)
        lit.train(); lit.configure_optimizers(); lit.configure_fused(1, 0.25)
        return lit

    def batch(lit, seed):
        b = bench.synthetic_batch(lit.model.cfg, 8, seed, lit.model.device)
        b["label"] = b["label"] % lit.model.cfg.n_expert
        return {"image": b["image"], "label": b["label"], "caption": {"ids": b["ids"], "attn_mask": b["attn_mask"], "token_type": b["token_type"]}}

    head = lambda lit: lit.model.engine.mlm.store.p32
    a = build()
    assert a.model.engine.cfg.text_mlm and a.model.engine.cfg.mlm_prob == 0.3
    for it in range(2):
        res = a.fused_training_step(batch(a, 90 + it))
        assert math.isfinite(float(res["mlm_loss"])) and 0.0 <= float(res["mlm_acc"]) <= 1.0
    val = a.validation_step(batch(a, 95))
    assert math.isfinite(float(val["mlm_loss"])) and "mlm_acc" in val
    ck = {"state_dict": a.state_dict()}
    a.on_save_checkpoint(ck)
    path = os.path.join(str(tmp_path), "c.ckpt")
    torch.save(ck, path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(ck["mlm_head"]) == ["cls.bias", "cls.dense.bias", "cls.dense.weight", "cls.layer_norm.bias", "cls.layer_norm.weight"]
    assert ck["fused_adam"]["mlm"]["step"] == 2 and ck["text_dropout_step"] == 2
    r, n = build(), build()
    r.load_state_dict(ck["state_dict"]); r.on_load_checkpoint(ck)
    n.load_state_dict(ck["state_dict"])
    p2 = head(a).clone()
    assert torch.equal(head(r), p2) and not torch.equal(head(n), p2)
    n.model.engine.mlm.store.load_named({"mlm." + k: v for k, v in ck["mlm_head"].items()})      # the head without its moments and step counter
    n.model.engine.dropout_step = 2
    b3 = batch(a, 93)
    for m in (a, r, n):
        m.training_step(b3, 2)
    torch.cuda.synchronize()
    ua, ur, un = head(a) - p2, head(r) - p2, head(n) - p2
    print(f"\nhead update after resume: rel {rel(ur, ua):.3g}; with fresh moments {rel(un, ua):.3g}")
    assert float(ua.norm()) > 0 and rel(ur, ua) < 2e-2, rel(ur, ua)
    assert rel(un, ua) > 0.2, rel(un, ua)


@pytest.mark.parametrize("case", [0, 1])
def test_reference_fixture_through_src_losses(case):
    """tests/golden/mlm_head.npz: the reference's MaskedPredictionLoss in float64 - the loss and every gradient through
    src.losses.MaskedPredictionLoss.  A gradient's bar is its count of bf16 roundings (module docstring); the fixture's dense and decoder
    matrices and hidden states are bf16 values, so the operands are the same numbers."""
    import src.losses as L
    fx = np.load(GOLDEN)
    p = f"c{case}_"
    hid = torch.tensor(fx[p + "hidden_states"], device=DEV, requires_grad=True)
    labels = torch.tensor(fx[p + "masked_labels"], device=DEV)
    D, V = hid.shape[-1], fx[p + "cls.bias"].shape[0]
    m = L.MaskedPredictionLoss(hidden_size=D, vocab_size=V).to(DEV).train()
    with torch.no_grad():
        for name, prm in m.named_parameters():
            prm.copy_(torch.tensor(fx[p + name]))
    out = m(hid, labels)
    out["loss"].backward()
    torch.cuda.synchronize()
    assert out["logits"] is None and m.counts.tolist()[0] == int((fx[p + "masked_labels"] != -1).sum())
    e_loss = abs(float(out["loss"].detach()) - float(fx[p + "loss"])) / float(fx[p + "loss"])
    errs = {"hidden": rel(hid.grad.cpu(), torch.tensor(fx[p + "grad_hidden"]))}
    errs.update({name: rel(prm.grad.cpu(), torch.tensor(fx[p + "grad_" + name])) for name, prm in m.named_parameters()})
    print(f"\nfixture case {case} (hidden {D}, vocab {V}): loss {float(out['loss'].detach()):.5f} rel {e_loss:.3g}", {k: float(f"{v:.3g}") for k, v in errs.items()})
    assert e_loss < 2 * BF16_STEP
    bars = {"hidden": 7, "cls.dense.weight": 6, "cls.dense.bias": 6, "cls.layer_norm.weight": 4, "cls.layer_norm.bias": 4, "cls.bias": 3,
            "cls.decoder.weight": 3}
    for k, v in errs.items():
        assert v <= bars[k] * BF16_STEP, (k, v)
    # the logits of the head (inspection path) against the fixture's logsumexp, and an empty selection: loss 0, not NaN
    lse = torch.logsumexp(m.cls(hid.detach()).double(), dim=-1).cpu().reshape(-1)[torch.tensor(fx[p + "masked_labels"]).reshape(-1) != -1]
    assert float((lse - torch.tensor(fx[p + "lse"])).abs().max()) < 8 * BF16_STEP
    none = m(hid.detach(), torch.full_like(labels, -1))
    assert float(none["loss"]) == 0.0 and m.counts.tolist() == [0, 0]
