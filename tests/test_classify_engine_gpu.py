"""Engine.classify_step / classify_eval and fit_linear_probe on the GPU: the online probe leaves the engine's stores alone, the
fine-tuning gradient equals the composition of already-tested parts, accumulation, the vit_lora case, bit-reproducibility in deterministic
mode, and the convergence of the linear probe."""
import math

import pytest
import torch

import classify_reference as R
from test_engine_gpu import make, rel, to_dev
from test_vit_lora_gpu import make_v

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, C = 8, 5
# two runs of the same backward differ by the order of their fp32 atomics: the bar of test_engine_gpu.test_gradient_accumulation_equals_one_step
REPEAT_BAR = 2e-3


def _head(eng, task="multiclass", init="normal", **kw):
    from medmoe_amd.classify import ClassifierHead
    return ClassifierHead(eng.cfg.d_out, C, eng.device, task=task, init=init, std=0.05, seed=5, **kw)


def _cls_batch(batch, task="multiclass", seed=0):
    g = torch.Generator().manual_seed(seed)
    if task == "multiclass":
        lab = torch.randint(0, C, (B,), generator=g)
        lab[1] = -1
    else:
        lab = (torch.rand(B, C, generator=g) < 0.4).long()
        lab[2, 3] = -1
    return {"image": batch["image"].cuda(), "label": lab.cuda()}


def _arena_snapshot(a):
    names = ("p32", "g32", "p16", "p16t", "m", "v", "e32")
    return {n: getattr(a, n).clone() for n in names if getattr(a, n, None) is not None}


@pytest.mark.parametrize("cfg_name", ["tiny", "tiny2"])
def test_probe_leaves_the_engine_alone(cfg_name):
    _, _, _, batch, eng = make(cfg_name, B)
    head = _head(eng, init="zeros")
    b = _cls_batch(batch)
    eng.train_step(to_dev(batch))                                    # the stores hold a gradient and Adam moments to be left alone
    torch.cuda.synchronize()
    before, step0 = _arena_snapshot(eng.params), eng.dropout_step
    w0 = head.weight.clone()
    out = None
    for _ in range(3):
        out = eng.classify_step(b, head, train_tower=False, head_lr=0.05)
    torch.cuda.synchronize()
    after = _arena_snapshot(eng.params)
    assert sorted(after) == sorted(before) and "m" in before
    for n in before:
        assert torch.equal(before[n], after[n]), n
    assert eng.dropout_step == step0 and eng.params.step_count == 1
    assert not torch.equal(head.weight, w0) and head.store.step_count == 3
    assert int(out["n_valid"]) == B - 1 and math.isfinite(float(out["loss"]))
    # forward only: classify_eval writes nothing of the head either
    hs = _arena_snapshot(head.store)
    logits, ev = eng.classify_eval(b, head)
    torch.cuda.synchronize()
    for n, v in _arena_snapshot(head.store).items():
        assert torch.equal(v, hs[n]), n
    assert logits.shape == (B, C) and math.isfinite(float(ev["loss"])) and torch.equal(logits, head.logits(eng.ws["img_g"]))


@pytest.mark.parametrize("cfg_name,task", [("tiny", "multiclass"), ("tiny2", "multilabel")])
def test_finetune_gradient_is_the_composition_of_tested_parts(cfg_name, task):
    _, _, _, batch, eng = make(cfg_name, B, seed=3)
    kw = {"label_smoothing": 0.1} if task == "multiclass" else {"pos_weight": torch.linspace(0.5, 2.0, C)}
    head = _head(eng, task, **kw)
    b = _cls_batch(batch, task)
    out = eng.classify_step(b, head, train_tower=True, optimizer=False)
    torch.cuda.synchronize()
    g_step = eng.params.g32.clone()
    gW, gb, loss = head.store.grad("classifier.weight").clone(), head.store.grad("classifier.bias").clone(), float(out["loss"])
    assert g_step.abs().max() > 0
    # the composition: the training image pass, dx of the float64 head at the engine's own features, backward(None)
    eng.params.zero_grad()
    eng._forward_image_train(b["image"])
    feat = eng.ws["img_g"].clone()
    args = (feat, head.weight, head.bias, b["label"], task)
    rkw = dict(label_smoothing=kw.get("label_smoothing", 0.0), pos_weight=kw.get("pos_weight"))
    ref, twin = R.head_reference(*args, dtype=torch.float64, **rkw), R.head_reference(*args, dtype=torch.float32, **rkw)
    eng.ws["d_img_g"].copy_(ref["dx"].float())
    eng.ws["d_img_l"].zero_()
    eng.backward(None)
    torch.cuda.synchronize()
    e = rel(eng.params.g32, g_step)
    print(f"{cfg_name} {task}: classify_step against the composition, relative L2 {e:.3e}")
    assert e < REPEAT_BAR, e
    for name, got in (("dW", gW), ("db", gb)):
        tol = R.tolerance(ref[name], twin[name])
        dev = float((got.double().cpu() - ref[name]).abs().max())
        print(f"{cfg_name} {task} head {name}: kernel {dev:.3e}  tolerance {tol:.3e}")
        assert dev <= tol, (name, dev, tol)
    assert abs(loss - float(ref["loss"])) <= R.tolerance(ref["loss"], twin["loss"])


def test_accumulation_of_two_half_scaled_micro_batches():
    _, _, _, batch, eng = make("tiny2", B)
    head = _head(eng)
    b = _cls_batch(batch)
    eng.classify_step(b, head, train_tower=True, optimizer=False)
    torch.cuda.synchronize()
    full = eng.params.export_named(eng.params.g32)
    g1, h1 = eng.params.g32.clone(), head.store.g32.clone()
    eng.classify_step(b, head, train_tower=True, optimizer=False, zero_grad=True, loss_scale=0.5)
    eng.classify_step(b, head, train_tower=True, optimizer=False, zero_grad=False, loss_scale=0.5)
    torch.cuda.synchronize()
    assert rel(eng.params.g32, g1) < REPEAT_BAR and rel(head.store.g32, h1) < REPEAT_BAR
    half = eng.params.export_named(eng.params.g32)
    groups = {}
    for k in full:                                                   # per parameter group: embeddings, each layer, the final norm, router, experts
        key = ".".join(k.split(".")[:3]) if k.startswith("vit.layer.") else ".".join(k.split(".")[:2])
        groups.setdefault(key, []).append(k)
    for key, names in groups.items():
        a, c = torch.cat([half[k].reshape(-1) for k in names]), torch.cat([full[k].reshape(-1) for k in names])
        if float(c.norm()) > 1e-7:
            assert rel(a, c) < REPEAT_BAR, (key, rel(a, c))


def test_vit_lora_engine_finetunes_adapters_moe_and_head_only():
    _, _, _, batch, eng, _ = make_v("tiny", B)
    head = _head(eng)
    b = _cls_batch(batch)
    p, tf = eng.params, eng.params.train_from
    assert tf > 0 and p.g32.numel() == p.numel - tf
    backbone, tail, w0, a0 = p.p32[:tf].clone(), p.p32[tf:].clone(), head.weight.clone(), eng.vlora.p32.clone()
    eng.classify_step(b, head, train_tower=True, optimizer=False)
    torch.cuda.synchronize()
    assert p.g32.abs().max() > 0 and eng.vlora.g32.abs().max() > 0 and head.store.g32.abs().max() > 0
    eng.classify_step(b, head, train_tower=True, head_lr=0.01)
    torch.cuda.synchronize()
    assert torch.equal(p.p32[:tf], backbone)                         # the backbone's arena is untouched
    assert not torch.equal(p.p32[tf:], tail) and not torch.equal(eng.vlora.p32, a0) and not torch.equal(head.weight, w0)


def _finetune_and_its_hand_run(new_engine, task):
    """One classify_step(train_tower=True, head_lr=0.01) on a deterministic engine, and on a second engine from `new_engine` the same step
    launch by launch.  Per run: (engine, head, loss, clip total)."""
    kw = {"label_smoothing": 0.1} if task == "multiclass" else {"pos_weight": torch.linspace(0.5, 2.0, C)}
    runs = []
    for hand in (False, True):
        batch, eng = new_engine()
        eng.set_deterministic(True)
        head = _head(eng, task, **kw)
        b = _cls_batch(batch, task)
        eng._alloc(B)
        eng.ws["d_img_g"].fill_(float("nan")); eng.ws["d_img_l"].fill_(float("nan"))
        if not hand:
            loss = eng.classify_step(b, head, train_tower=True, head_lr=0.01)["loss"].clone()
        else:
            c = eng.cfg
            eng.params.zero_grad()
            if eng.vlora is not None:
                eng.vlora.zero_grad()
            head.store.zero_grad()
            eng._forward_image_train(b["image"])
            loss = head.step(eng.ws["img_g"], b["label"], 1.0, dfeat=eng.ws["d_img_g"])[0].clone()
            eng.ws["d_img_l"].zero_()
            eng.backward(None, 1.0)
            eng.dropout_step += 1
            # the clip total: every other arena's sum of squares is launched before the image arena's, then added to it in the order
            # image arena, adapters, head - fp32 addition does not commute in its last bit, so the order is part of the step
            side = ([eng.vlora.sumsq()] if eng.vlora is not None else []) + [head.store.sumsq()]
            total = eng.params.sumsq()
            for part in side:
                total.add_(part)
            akw = dict(betas=tuple(c.adam_betas), eps=c.adam_eps, decoupled=c.optimizer == "adamw")
            eng.params.adam_step(total, c.lr, c.weight_decay, c.clip, **akw)
            if eng.vlora is not None:
                eng.vlora.adam_step(total, c.lr, c.weight_decay, c.clip, **akw)
            head.adam_step(0.01, c.weight_decay, c.clip, normsq_total=total, **akw)
        torch.cuda.synchronize()
        # the head wrote ALL of d_img_g (it was NaN) and d_img_l is zero
        assert bool(torch.isfinite(eng.ws["d_img_g"].float()).all()) and float(eng.ws["d_img_g"].float().abs().max()) > 0
        assert bool((eng.ws["d_img_l"] == 0).all())
        assert float(eng.params.g32.abs().max()) > 0 and eng.dropout_step == 1
        runs.append((eng, head, loss))
    return runs


def _step_record(eng, head, loss):
    rec = [eng.params.p32, eng.params.g32, eng.params.m, head.store.p32, head.store.g32, loss]
    if eng.vlora is not None:
        rec += [eng.vlora.p32, eng.vlora.g32]
    return [t.clone() for t in rec]


@pytest.mark.parametrize("task", ["multiclass", "multilabel"])
def test_finetune_is_the_hand_run_sequence_bit_for_bit(task):
    def new_engine():
        _, _, _, batch, eng = make("tiny2", B, seed=3)
        return batch, eng
    step, hand = _finetune_and_its_hand_run(new_engine, task)
    for a, c in zip(_step_record(*step), _step_record(*hand)):
        assert torch.equal(a, c)


@pytest.mark.parametrize("task", ["multiclass", "multilabel"])
def test_finetune_with_adapters_is_the_hand_run_sequence_bit_for_bit(task):
    """The only test of the three-arena clip total (image arena + adapters + head).  The comparison is torch.equal throughout, the
    adapters' parameters and gradients included: two independent classify_step runs of this engine in deterministic mode were measured
    bit-identical in every one of these buffers (deterministic mode covers the adapters' backward), so no repeat bar is needed."""
    def new_engine():
        _, _, _, batch, eng, _ = make_v("tiny", B)
        return batch, eng
    step, hand = _finetune_and_its_hand_run(new_engine, task)
    assert float(step[0].vlora.g32.abs().max()) > 0
    for a, c in zip(_step_record(*step), _step_record(*hand)):
        assert torch.equal(a, c)


def test_deterministic_engines_agree_bit_for_bit():
    from medmoe_amd import ops
    runs = []
    for _ in range(2):
        _, _, _, batch, eng = make("tiny2", B)
        eng.set_deterministic(True)
        head = _head(eng)
        b = _cls_batch(batch)
        before = ops.nondet_launches()
        losses = [eng.classify_step(b, head, train_tower=True, head_lr=0.01)["loss"].clone() for _ in range(2)]
        torch.cuda.synchronize()
        assert ops.nondet_launches() == before
        runs.append((eng.params.p32.clone(), eng.params.g32.clone(), head.store.p32.clone(), head.store.g32.clone(), torch.stack(losses)))
    for a, c in zip(*runs):
        assert torch.equal(a, c)


@pytest.mark.parametrize("task", ["multiclass", "multilabel"])
@pytest.mark.parametrize("seed", [0, 3])
def test_fit_linear_probe_converges(task, seed):
    """N = 300, D = 64, C = 5, cluster centres 2 randn, noise 0.5 randn; the head starts at zero and takes 100 full-batch Adam steps at lr
    0.05.  Required: multiclass accuracy exactly 1 and every class AUROC exactly 1 (the float64 restatement gets there in 25 - 50 steps)."""
    from medmoe_amd.classify import ClassifierHead, ScoreBank, classification_metrics, fit_linear_probe
    N, D = 300, 64
    g = torch.Generator().manual_seed(seed)
    centres = 2.0 * torch.randn(C, D, generator=g)
    if task == "multiclass":
        t = torch.randint(0, C, (N,), generator=g)
        x = centres[t] + 0.5 * torch.randn(N, D, generator=g)
    else:
        t = (torch.rand(N, C, generator=g) < 0.4).long()
        x = t.float() @ centres + 0.5 * torch.randn(N, D, generator=g)
    x, t = x.to(DEV), t.to(DEV)
    head = ClassifierHead(D, C, DEV, task=task)
    hist = fit_linear_probe(x, t, head, iters=100, lr=0.05)
    torch.cuda.synchronize()
    assert hist.shape == (100,) and hist.is_cuda
    assert abs(float(hist[0]) - (math.log(C) if task == "multiclass" else math.log(2.0))) < 1e-6
    assert float(hist[-1]) < float(hist[0])
    bank = ScoreBank(C, DEV, task=task)
    bank.add(head.logits(x), t)
    m = classification_metrics(bank)
    print(task, seed, "final loss", float(hist[-1]), m)
    if task == "multiclass":
        assert m["acc"] == 1.0
    assert all(m[f"auroc/{c}"] == 1.0 for c in range(C)) and m["auroc_mean"] == 1.0
