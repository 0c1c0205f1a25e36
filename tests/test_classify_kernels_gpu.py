"""The classification head and AUROC launches (csrc/classify.hip) against the float64 restatement of tests/classify_reference.py.

Tolerance of an output: 8 x the largest absolute deviation a torch fp32 CPU evaluation of the same formulas shows from the float64 one on
the same inputs, at least 4 ulp at the output's largest magnitude (classify_reference.tolerance).  The factor 8 covers the different
summation order (wave tree and staged records against sequential) and a few ulp of exp / log.  Every case prints both deviations."""
import functools

import numpy as np
import pytest
import torch

import classify_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (task, N, D, C, options): one row, fewer rows than a workgroup has waves, several row ranges (several staged records), the widest head;
# W in LDS (C D <= 16384) and W through the caches; every float4 count per lane (D / 256 rounded up = 1, 3, 8)
CASES = [
    ("multiclass", 1, 64, 1, {}),
    ("multiclass", 1, 768, 14, {"smooth": 0.1}),
    ("multiclass", 5, 768, 3, {"ignore": "some", "scale": 0.25}),
    ("multiclass", 5, 2048, 64, {"smooth": 0.1, "big": True}),
    ("multiclass", 300, 768, 14, {"ignore": "some", "smooth": 0.1, "scale": 0.25, "big": True}),
    ("multiclass", 300, 64, 3, {"ignore": "all"}),
    ("multiclass", 3000, 2048, 64, {"ignore": "some", "scale": 0.25}),
    ("multiclass", 3000, 64, 14, {"smooth": 0.1, "big": True}),
    ("multilabel", 1, 64, 1, {"pw": True}),
    ("multilabel", 1, 2048, 64, {"ignore": "some", "big": True}),
    ("multilabel", 5, 768, 14, {"ignore": "column", "pw": True, "scale": 0.25}),
    ("multilabel", 300, 768, 14, {"ignore": "column", "pw": True, "scale": 0.25, "big": True}),
    ("multilabel", 300, 2048, 3, {"ignore": "all"}),
    ("multilabel", 3000, 768, 64, {"ignore": "some", "pw": True, "big": True}),
    ("multilabel", 3000, 64, 3, {"ignore": "some", "scale": 0.25}),
]
IDS = [f"{t}-N{n}-D{d}-C{c}-" + "+".join(f"{k}={v}" for k, v in o.items()) for t, n, d, c, o in CASES]


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs (CPU) and the float64 / fp32-twin references of case i, computed once and shared."""
    task, N, D, C, o = CASES[i]
    g = torch.Generator().manual_seed(100 + i)
    x = torch.randn(N, D, generator=g)
    # logits of magnitude ~40 ("big") exercise the stable softmax / softplus; otherwise of magnitude ~2
    W = torch.randn(C, D, generator=g) * ((40.0 if o.get("big") else 2.0) / (3.0 * D ** 0.5))
    b = torch.randn(C, generator=g) * 0.1
    if task == "multiclass":
        t = torch.randint(0, C, (N,), generator=g)
        if o.get("ignore") == "some":
            t[torch.rand(N, generator=g) < 0.3] = -1
        elif o.get("ignore") == "all":
            t[:] = -1
        t = t.to(torch.int32)
    else:
        t = (torch.rand(N, C, generator=g) < 0.4).to(torch.int8)
        if o.get("ignore") in ("some", "column"):
            t[torch.rand(N, C, generator=g) < 0.2] = -1
        if o.get("ignore") == "column":
            t[:, C // 2] = -1
        elif o.get("ignore") == "all":
            t[:] = -1
    pw = (0.5 + 2.0 * torch.rand(C, generator=g)) if o.get("pw") else None
    kw = dict(label_smoothing=o.get("smooth", 0.0), pos_weight=pw, loss_scale=o.get("scale", 1.0))
    ref = R.head_reference(x, W, b, t, task, dtype=torch.float64, **kw)
    twin = R.head_reference(x, W, b, t, task, dtype=torch.float32, **kw)
    return x, W, b, t, pw, kw, ref, twin


def _run(i, dx=True, dW=None, db=None):
    from medmoe_amd import ops
    task, N, D, C, _ = CASES[i]
    x, W, b, t, pw, kw, _, _ = _case(i)
    xd, Wd, bd, td = x.to(DEV), W.to(DEV), b.to(DEV), t.to(DEV)
    dW = torch.zeros(C, D, device=DEV) if dW is None else dW
    db = torch.zeros(C, device=DEV) if db is None else db
    dxd = torch.full((N, D), float("nan"), device=DEV) if dx else None          # written, not accumulated: the NaNs must go
    z, loss, counts = ops.cls_head_step(xd, Wd, bd, td, dW, db, task=task, label_smoothing=kw["label_smoothing"],
                                        pos_weight=None if pw is None else pw.to(DEV), loss_scale=kw["loss_scale"], dx=dxd)
    return {"z": z, "loss": loss.reshape(()), "dx": dxd, "dW": dW, "db": db, "counts": counts}


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_head_step_matches_float64(i):
    from medmoe_amd import ops
    task, N, D, C, _ = CASES[i]
    x, W, b, t, pw, kw, ref, twin = _case(i)
    got = _run(i)
    torch.cuda.synchronize()
    for name in ("z", "loss", "dx", "dW", "db"):
        tol = R.tolerance(ref[name], twin[name])
        dev_k = float((got[name].double().cpu() - ref[name]).abs().max())
        dev_t = float((twin[name].double() - ref[name]).abs().max())
        print(f"{IDS[i]} {name}: kernel {dev_k:.3e}  fp32 twin {dev_t:.3e}  tolerance {tol:.3e}  max |ref| {float(ref[name].abs().max()):.3e}")
        assert torch.isfinite(got[name]).all(), name
        assert dev_k <= tol, (name, dev_k, tol)
    n_valid, n_correct = (int(v) for v in got["counts"].tolist())
    assert n_valid == ref["n_valid"]
    if ref["n_valid"] == 0:
        assert float(got["loss"]) == 0.0 and not got["dx"].any() and not got["dW"].any() and not got["db"].any()
    if task == "multiclass":
        # the kernel's argmax is that of ITS logits: equal to the float64 one wherever the top-two margin exceeds the tolerance of z
        tolz = R.tolerance(ref["z"], twin["z"])
        zk = got["z"].cpu()
        pred = (zk == zk.max(dim=1, keepdim=True).values).to(torch.int8).argmax(dim=1)                  # ties: the lowest class
        valid = t >= 0
        assert n_correct == int(((pred == t.long()) & valid).sum())
        if C > 1:
            top2 = ref["z"].topk(2, dim=1).values
            safe = (top2[:, 0] - top2[:, 1]) > tolz
            assert torch.equal(pred[safe], ref["pred"][safe])
    else:
        zk, valid = got["z"].cpu(), t >= 0
        assert n_correct == int((((zk > 0) == (t == 1)) & valid).sum())
    # the evaluation entry writes the same logits
    z2 = ops.cls_head_logits(x.to(DEV), W.to(DEV), b.to(DEV))
    assert torch.equal(z2, got["z"])


def test_ties_go_to_the_lowest_class():
    from medmoe_amd import ops
    x = torch.zeros(4, 64, device=DEV)
    W = torch.zeros(5, 64, device=DEV)
    b = torch.tensor([0.0, 1.0, 1.0, 0.5, 1.0], device=DEV)                        # classes 1, 2 and 4 tie: 1 wins
    t = torch.tensor([1, 2, 4, -1], device=DEV, dtype=torch.int32)
    _, _, counts = ops.cls_head_step(x, W, b, t, torch.zeros(5, 64, device=DEV), torch.zeros(5, device=DEV))
    assert counts.tolist() == [3, 1]


@pytest.mark.parametrize("i", [4, 11], ids=[IDS[4], IDS[11]])
def test_gradients_accumulate(i):
    first = _run(i, dx=False)
    g1, b1 = first["dW"].clone(), first["db"].clone()
    second = _run(i, dx=False, dW=first["dW"], db=first["db"])
    for once, twice in ((g1, second["dW"]), (b1, second["db"])):
        # g + g is exact, so the second call leaves 2 g up to the rounding of ONE addition: 1 ulp of the result per element
        ulp = torch.tensor([R.ulp32(abs(v)) for v in (2.0 * once.double()).reshape(-1).tolist()]).reshape(once.shape)
        assert ((twice.double().cpu() - 2.0 * once.double().cpu()).abs() <= ulp).all()
    assert g1.abs().max() > 0


@pytest.mark.parametrize("i", [6, 13], ids=[IDS[6], IDS[13]])
def test_two_runs_give_identical_bits_and_no_order_dependent_launch(i):
    from medmoe_amd import ops
    assert CASES[i][1] == 3000
    before = ops.nondet_launches()
    a, b = _run(i), _run(i)
    torch.cuda.synchronize()
    assert ops.nondet_launches() == before
    for name in ("z", "loss", "dx", "dW", "db", "counts"):
        assert torch.equal(a[name], b[name]), name


@pytest.mark.parametrize("N", [1, 2, 257, 2000])
@pytest.mark.parametrize("C", [1, 5])
def test_auroc_counts_match_brute_force(N, C):
    from medmoe_amd import ops
    g = torch.Generator().manual_seed(7 * N + C)
    scores = torch.randint(-8, 9, (N, C), generator=g).float() / 8.0               # multiples of 1/8: many ties, exact in fp32
    targets = (torch.rand(N, C, generator=g) < 0.4).to(torch.int8)
    targets[torch.rand(N, C, generator=g) < 0.15] = -1
    got = ops.auroc_counts(scores.to(DEV), targets.to(DEV)).cpu().numpy()
    want = R.auroc_counts_reference(scores.numpy(), targets.numpy())
    assert got.dtype == np.int64 and np.array_equal(got, want), (got, want)
    again = ops.auroc_counts(scores.to(DEV), targets.to(DEV)).cpu().numpy()
    assert np.array_equal(got, again)


def test_auroc_host_reducer_on_kernel_counts():
    from medmoe_amd.classify import auroc
    g = torch.Generator().manual_seed(11)
    scores = torch.randint(-4, 5, (300, 3), generator=g).float() / 4.0
    targets = (torch.rand(300, 3, generator=g) < 0.5).to(torch.int8)
    targets[:, 2] = 1                                                              # a one-sided class: NaN, left out of the mean
    per, mean = auroc(scores.to(DEV), targets.to(DEV))
    want_per, want_mean = R.auroc_reference(scores.numpy(), targets.numpy())
    assert per.dtype == torch.float64 and np.array_equal(per[:2].cpu().numpy(), want_per[:2]) and per[2] != per[2]
    assert mean == want_mean
