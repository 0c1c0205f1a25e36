"""Engine.ground on the GPU, on tiny2: it is the two ops calls on the features its own forward left, bit for bit; it writes no
parameter, gradient, moment or average; under ema=True it agrees with itself inside and outside ema_weights(); token spans go through the
segment map; it refuses what it names."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 8


def _engine(**over):
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    cfg = config_by_name("tiny2")
    for k_, v in over.items():
        setattr(cfg, k_, v)
    torch.manual_seed(0)
    return Engine(cfg, DEV), cfg


def _batch(cfg, seed=41):
    """A synthetic batch with seeded word spans inside every caption and two boxes per image (the second absent for odd images)."""
    import bench
    b = bench.synthetic_batch(cfg, B, seed, torch.device(DEV))
    from medmoe_amd.engine import VocabTables
    _, cap = VocabTables.synthetic(cfg.vocab, "cpu").segment_map_torch(b["ids"].cpu())
    g = torch.Generator().manual_seed(seed)
    lo = torch.stack([torch.randint(0, int(c), (1,), generator=g)[0] for c in cap])
    hi = torch.minimum(lo + 1 + torch.randint(0, 3, (B,), generator=g), cap.long())
    b["span"] = torch.stack([lo, hi], dim=1)
    s = cfg.img_size
    box = torch.zeros(B, 2, 4, dtype=torch.int32)
    for i in range(B):
        x0, y0 = (int(v) for v in torch.randint(0, s - 4, (2,), generator=g))
        box[i, 0] = torch.tensor([x0, y0, min(s, x0 + 1 + s // 3), min(s, y0 + 1 + s // 2)])
        if i % 2 == 0:
            box[i, 1] = torch.tensor([s // 2, s // 2, s, s])
    b["box"] = box
    return b, cap


REC = ("rec_f", "rec_i", "rec_d", "h")


@pytest.mark.parametrize("mode", ["attention", "cosine"])
def test_ground_is_the_two_ops_calls_on_the_workspace(mode):
    from medmoe_amd import ops
    eng, cfg = _engine()
    b, cap = _batch(cfg)
    out = eng.ground(b, mode=mode, thetas=(0.3, 0.5), want_map=True)
    torch.cuda.synchronize()
    assert torch.equal(eng.cap_lens.cpu().long(), cap.long())
    P, s = cfg.n_patch, cfg.img_size
    assert tuple(out["h"].shape) == (B, P) and tuple(out["hf"].shape) == (B, s, s) and out["size"] == (s, s) and out["thetas"] == (0.3, 0.5)
    pair = torch.arange(B)
    ent = torch.stack([pair, pair, b["span"][:, 0], b["span"][:, 1]], dim=1)
    h = ops.ground_maps(eng.ws["img_l"], eng.ws["words"], eng.cap_lens, ent, mode=mode, temp1=cfg.temp1)
    want = ops.ground_score(h, b["box"], (s, s), thetas=(0.3, 0.5), want_map=True)
    assert torch.equal(h, out["h"])
    for k in ("rec_f", "rec_i", "rec_d", "hf"):
        assert torch.equal(out[k], want[k]), k
    assert bool(torch.isfinite(out["h"]).all()) and int(out["rec_i"][:, 3].min()) > 0
    if mode == "attention":
        assert float((out["h"].double().sum(dim=1) - 1.0).abs().max()) < 1e-5
    # ground is embed + ground_workspace; another size and no stored map: the same grid maps
    small = eng.ground(b, mode=mode, size=(40, 52))
    assert "hf" not in small and small["size"] == (40, 52) and torch.equal(small["h"], out["h"]) and tuple(small["rec_f"].shape) == (B, 3)
    eng.embed(b)
    again = eng.ground_workspace(b, mode=mode, thetas=(0.3, 0.5))
    assert all(torch.equal(again[k], out[k]) for k in REC)
    # token spans: through the segment map of this batch (the synthetic vocabulary has no continuation piece: word w is token w)
    tok = dict(b)
    del tok["span"]
    tok["tok_span"] = b["span"]
    via = eng.ground(tok, mode=mode, thetas=(0.3, 0.5))
    assert all(torch.equal(via[k], out[k]) for k in REC)
    # a bank over the records
    from medmoe_amd.ground import GroundBank, grounding_metrics
    bank = GroundBank((0.3, 0.5), DEV)
    bank.add(out)
    met = grounding_metrics(bank)
    assert met["n_entries"] == B and 0.0 <= met["pg_acc"] <= 1.0 and met["cnr_mean"] >= 0.0 and 0.0 <= met["iou@0.3"] <= met["dice@0.3"] <= 1.0


def test_ground_writes_no_state_and_agrees_with_itself_under_ema():
    eng, cfg = _engine(ema_decay=0.99)
    b, _ = _batch(cfg)
    eng.train_step({k: v for k, v in b.items() if k not in ("span", "box")})
    torch.cuda.synchronize()
    state = lambda: [t.detach().clone() for st in eng.optimizer_stores().values() for t in (st.p32, st.g32, st.m, st.v, st.e32) if t is not None]
    before, step0 = state(), eng.dropout_step
    assert len(before) >= 5
    plain = eng.ground(b)
    outside = eng.ground(b, ema=True)
    with eng.ema_weights():
        inside = eng.ground(b, ema=True)
        inside2 = eng.ground(b)
    back = eng.ground(b)
    torch.cuda.synchronize()
    for k in REC:
        assert torch.equal(outside[k], inside[k]) and torch.equal(inside[k], inside2[k]), k
        assert torch.equal(plain[k], back[k]), k
    assert not torch.equal(plain["h"], outside["h"])                    # the master moved away from the average
    after = state()
    assert len(after) == len(before) and all(torch.equal(x, y) for x, y in zip(before, after)) and eng.dropout_step == step0


def test_ground_refuses_what_it_names():
    eng, cfg = _engine()
    b, cap = _batch(cfg)
    with pytest.raises(KeyError, match="neither 'span'"):
        eng.ground({k: v for k, v in b.items() if k != "span"})
    with pytest.raises(KeyError, match="holds no 'box'"):
        eng.ground({k: v for k, v in b.items() if k != "box"})
    bad = dict(b)
    bad["span"] = b["span"].clone()
    bad["span"][3, 1] = int(cap[3]) + 1
    with pytest.raises(ValueError, match=r"entries\[3\] has the word span"):
        eng.ground(bad)
    with pytest.raises(ValueError, match="mode must be one of"):
        eng.ground(b, mode="softmax")
    with pytest.raises(ValueError, match="NTH = 5"):
        eng.ground(b, thetas=(0.1, 0.2, 0.3, 0.4, 0.5))
    with pytest.raises(ValueError, match="smaller than the region grid"):
        eng.ground(b, size=(4, 64))
    with pytest.raises(ValueError, match="spans for a batch of"):
        eng.ground(dict(b, span=b["span"][:4]))
    d_t = cfg.d_t
    try:
        eng.cfg.d_t = 2 * d_t
        with pytest.raises(NotImplementedError, match="d_t = .* against regions of d_out"):
            eng.ground(b)
    finally:
        eng.cfg.d_t = d_t
    from medmoe_amd.swin_engine import SwinEngine
    with pytest.raises(NotImplementedError, match="SwinEngine.ground"):
        SwinEngine.ground(object.__new__(SwinEngine), b)
    with pytest.raises(NotImplementedError, match="SwinEngine.ground"):
        SwinEngine.ground_workspace(object.__new__(SwinEngine), b)
