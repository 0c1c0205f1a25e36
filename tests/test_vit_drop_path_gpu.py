"""Stochastic depth of the ViT tower on the GPU (csrc/dropout.hip medmoe_drop_path_scales / medmoe_scale_add_layernorm_fwd).

1. the per-sample scales against medmoe_dropout_mask, bit for bit (the mask contract itself is tests/test_text_dropout_gpu.py's first test);
2. the fused scale + residual + LayerNorm launch against float64: x1 within one bf16 ulp of res + s z (the `close` form of
   tests/test_text_lora_gpu.py: one bf16 ulp of the exact value + 2 * 2^-23 * (|res| + |s z|) for the fp32 product and sum), y / mean / rstd
   bit-equal to medmoe_layernorm_fwd on the stored x1, dropped rows bit-equal to the residual whatever z holds;
3. the reference's own TransformerEncoder with drop_path_rate = 0.3 under fixed masks (tools/gen_golden_drop_path.py) fed to
   Engine._vit_blocks / _vit_backward with the same scales injected, at the bars of test_prenorm_encoder_reference_fixture;
4. whole engine steps: drops where the scales say so, evaluation, deterministic mode, resume, ranks."""
import os

import numpy as np
import pytest
import torch

from test_text_dropout_host import keep_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SITE0 = 0x40000000


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from medmoe_amd import ops as o
    return o


def bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == BF else t.contiguous().view(torch.int32)


def rel(a, b):
    a, b = a.detach().float().cpu(), torch.as_tensor(b).float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def load(golden_dir, name):
    d = np.load(os.path.join(golden_dir, name))
    return {k: torch.from_numpy(np.asarray(d[k])) for k in d.files}


def dev16(t):
    return t.to(DEV, BF).contiguous()


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the scales
# ------------------------------------------------------------------------------------------------------------------------------
def mask_row(ops, cols, seed, step, site, p):
    """row 0 of the [1][cols_padded] mask array medmoe_dropout_mask draws, as bool"""
    out = torch.full((1, cols), 7, dtype=torch.uint8, device=DEV)
    ops.dropout_mask(out, 1, cols, (cols + 3) // 4 * 4, ops.dropout_rng(seed, step, site, p))
    assert bool((out <= 1).all())
    return out[0].bool()


def scales(ops, probs, B, sample0, seed, step, site0=SITE0):
    buf = torch.full((len(probs) * B + 64,), -3.0, device=DEV)
    out = buf[:len(probs) * B].view(len(probs), B)
    ops.drop_path_scales(out, probs, B, sample0, seed, step, site0)
    torch.cuda.synchronize()
    assert bool((buf[len(probs) * B:] == -3.0).all()), "drop_path_scales wrote past the end"
    return out.clone()


@pytest.mark.parametrize("B", [1, 5, 8, 130])
def test_scales_equal_the_exported_mask_bit_for_bit(ops, B):
    """Two ranks of B samples: rank r's scales are columns [r B, (r + 1) B) of the one-process draw over [1][2 B], which is 0 | fp32(1 / (1 - p))
    exactly where medmoe_dropout_mask keeps; p = 0 keeps everything at scale 1; another step draws another vector."""
    probs = [0.0, 0.1, 0.0, 0.37, 0.1]
    seed, step = 0x123456789ABCDEF, 7
    whole = scales(ops, probs, 2 * B, 0, seed, step)
    r0, r1 = scales(ops, probs, B, 0, seed, step), scales(ops, probs, B, B, seed, step)
    assert torch.equal(whole[:, :B], r0) and torch.equal(whole[:, B:], r1)
    for s, p in enumerate(probs):
        keep = mask_row(ops, 2 * B, seed, step, SITE0 + s, p)
        assert np.array_equal(keep.cpu().numpy(), keep_mask(1, 2 * B, (2 * B + 3) // 4 * 4, seed, step, SITE0 + s, p)[0])
        want = keep.float() * torch.tensor(1.0 / (1.0 - p), dtype=F32, device=DEV)
        assert torch.equal(bits(whole[s]), bits(want)), (s, p)
        if p == 0.0:
            assert bool((whole[s] == 1.0).all())
    if B == 130:
        assert not torch.equal(whole[1], whole[4])                    # the same p at another site: another draw
    if B >= 8:
        other = scales(ops, probs, 2 * B, 0, seed, step + 1)
        assert not torch.equal(other[3], whole[3]) and torch.equal(other[0], whole[0])
        assert not torch.equal(scales(ops, probs, 2 * B, 0, seed + 1, step)[3], whole[3])


def test_scales_kept_fraction_and_values(ops):
    p = 0.1
    sc = scales(ops, [p], 4096, 0, 11, 3)[0]
    kept = float((sc != 0).float().mean())
    print(f"kept fraction at p = 0.1, B = 4096: {kept:.4f}")
    assert abs(kept - 0.9) <= 0.02                                    # four binomial standard deviations: 4 sqrt(0.09 / 4096) = 0.019
    assert torch.equal(bits(sc[sc != 0]), bits(torch.full_like(sc[sc != 0], 1.0 / (1.0 - p))))
    assert bool(((sc == 0) | (sc == torch.tensor(1.0 / (1.0 - p), dtype=F32, device=DEV))).all())


# ------------------------------------------------------------------------------------------------------------------------------
# 2. scale + residual + LayerNorm
# ------------------------------------------------------------------------------------------------------------------------------
def ulp_bf16(v):
    a = v.abs()
    return torch.where(a > 0, torch.exp2(torch.floor(torch.log2(a.clamp_min(1e-300))) - 7), torch.zeros_like(a))


def close(got, exact, terms, K, ulps=1.0, what=""):
    """|got - exact| <= ulps * ulp_bf16(exact) + K * 2^-23 * sum|terms|, elementwise (tests/test_text_lora_gpu.py)."""
    err = (got.to(F64) - exact).abs()
    tol = ulps * ulp_bf16(exact) + K * 2.0 ** -23 * terms
    bad = err > tol
    worst = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"    {what}: worst error / tolerance {worst:.3f}")
    assert not bool(bad.any()), (what, int(bad.sum()), worst)


SAL_SCALES = {2: [0.0, 1.0 / (1.0 - 0.2)], 3: [1.0 / (1.0 - 0.15), 0.0, 1.0], 5: [1.0 / (1.0 - 0.3), 0.0, 0.0, 1.0 / (1.0 - 0.1), 1.0]}


def guarded(shape, dtype):
    n = int(np.prod(shape))
    buf = torch.full((n + 512,), 3.0, dtype=dtype, device=DEV)
    return buf, buf[:n].view(*shape)


@pytest.mark.parametrize("B,rps,D", [(3, 17, 128), (2, 65, 64), (5, 197, 768), (2, 257, 1024)])
def test_scale_add_layernorm(ops, B, rps, D):
    g = torch.Generator().manual_seed(B * 1000 + D)
    rows, eps = B * rps, 1e-6
    z = (torch.randn(rows, D, generator=g) * 2 + 0.5).to(BF).to(DEV)
    res = torch.randn(rows, D, generator=g).to(BF).to(DEV)
    gam = (torch.rand(D, generator=g) + 0.5).to(DEV); bet = (torch.randn(D, generator=g) * 0.1).to(DEV)
    sc = torch.tensor(SAL_SCALES[B], dtype=F32, device=DEV)
    dropped = (sc == 0).repeat_interleave(rps)
    assert bool(dropped.any()) and not bool(dropped.all())
    zbad = z.clone()                                                  # whatever a dropped sample's branch holds must not reach x1
    zbad[dropped] = float("inf")
    zbad[dropped, 1::2] = float("nan")
    outs = []
    for zz in (zbad, zbad, z):
        b1, x1 = guarded((rows, D), BF); b2, y = guarded((rows, D), BF); b3, mean = guarded((rows,), F32); b4, rstd = guarded((rows,), F32)
        ops.scale_add_layernorm_fwd(zz, res, sc, rps, gam, bet, x1, y, mean, rstd, eps)
        torch.cuda.synchronize()
        for b, t in ((b1, x1), (b2, y), (b3, mean), (b4, rstd)):
            assert bool((b[t.numel():] == 3.0).all()), "wrote past the end"
        outs.append((x1, y, mean, rstd))
    for a, b in zip(outs[0], outs[1]):                                # two launches: the same bits
        assert torch.equal(bits(a), bits(b))
    for a, b in zip(outs[0], outs[2]):                                # and nothing of a dropped sample's z in any output
        assert torch.equal(bits(a), bits(b))
    x1, y, mean, rstd = outs[0]
    assert bool(torch.isfinite(x1.float()).all()) and bool(torch.isfinite(y.float()).all())
    assert torch.equal(bits(x1[dropped]), bits(res[dropped]))         # a dropped sample's rows COPY the residual
    s64 = sc.to(F64).repeat_interleave(rps)[:, None]
    z64 = torch.where(dropped[:, None], torch.zeros((), dtype=F64, device=DEV), z.to(F64))
    close(x1, res.to(F64) + s64 * z64, res.to(F64).abs() + (s64 * z64).abs(), 2, what=f"x1 {B}x{rps}x{D}")
    # the statistics and y are those of layernorm_fwd on the stored bf16 x1
    y2, st = torch.empty_like(x1), torch.empty(2, rows, device=DEV)
    ops.layernorm_fwd(x1, gam, bet, y2, st[0], st[1], eps)
    assert torch.equal(bits(y), bits(y2)) and torch.equal(bits(mean), bits(st[0])) and torch.equal(bits(rstd), bits(st[1]))


def test_scale_add_layernorm_refuses_bad_shapes(ops):
    def args(rows, D, n_scale, rps):
        t = lambda: torch.zeros(rows, D, dtype=BF, device=DEV)
        return (t(), t(), torch.ones(n_scale, device=DEV), rps, torch.ones(D, device=DEV), torch.zeros(D, device=DEV), t(), t(),
                torch.zeros(rows, device=DEV), torch.zeros(rows, device=DEV), 1e-6)
    for a in (args(34, 132, 2, 17), args(34, 2056, 2, 17), args(34, 128, 3, 17), args(34, 128, 1, 17)):
        with pytest.raises(ValueError, match="scale_add_layernorm_fwd"):
            ops.scale_add_layernorm_fwd(*a)
    ops.scale_add_layernorm_fwd(*args(34, 2048, 2, 17))               # the widest row the kernel takes
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the reference's encoder with stochastic depth
# ------------------------------------------------------------------------------------------------------------------------------
def _enc_config(**kw):
    from medmoe_amd.config import MedMoEConfig
    base = dict(img_size=64, patch=16, d_v=128, n_layer_v=2, n_head_v=2, ff_v=256, vocab=97, max_len=16, d_t=128, n_layer_t=2, n_head_t=2,
                ff_t=256, n_expert=4, top_k=1, d_out=128)
    base.update(kw)
    return MedMoEConfig(**base)


def _run_encoder(f, L, scales_, **cfg):
    """Engine._vit_blocks / _vit_backward on a fixture's weights, x and gy with `scales_` [L, 2, B] injected -> (engine, error dict)."""
    from medmoe_amd.engine import Engine
    B, N, D = 4, 17, 128
    eng = Engine(_enc_config(n_layer_v=L, **cfg), "cuda:0")
    assert eng.cfg.n_tok_v == N
    eng._alloc(B)
    p, ws = eng.params, eng.ws
    names = [k for k in f if k.startswith("layer.") or k.startswith("final_layer_norm.")]
    assert len(names) == 12 * L + 2
    for k in names:
        p.f32("vit." + k).copy_(f[k].cuda().reshape(p.shapes["vit." + k]))
    p.sync_working_copies()
    ws["x0"].copy_(dev16(f["x"]).view(B * N, D))
    eng.vit_drop_scales = scales_.to(DEV, F32).contiguous()
    eng._vit_blocks(B)
    torch.cuda.synchronize()
    e = {"hs": [rel(ws[f"x{l}"].view(B, N, D), f[f"hs{l}"]) for l in range(L + 1)], "last": rel(ws["lnf"].view(B, N, D), f["last"])}
    p.zero_grad()
    ws["dln"].copy_(dev16(f["gy"]).view(B * N, D))
    eng._wgrad_begin()
    eng._wait(eng._vit_backward(stage_grads=False))
    torch.cuda.synchronize()
    eng.vit_drop_scales = None
    e["gx"] = rel(ws["dxa"].view(B, N, D), f["gx"])
    e["grads"] = {k: rel(p.grad("vit." + k), f["grad." + k].reshape(p.shapes["vit." + k])) for k in names}
    e["gmax"], e["gmed"] = max(e["grads"].values()), float(np.median(list(e["grads"].values())))
    return eng, e


def _show(tag, e):
    worst = sorted(e["grads"].items(), key=lambda kv: -kv[1])[:4]
    print(f"{tag}: hidden states {[round(v, 5) for v in e['hs']]} last {e['last']:.5f} gx {e['gx']:.5f} "
          f"grads max {e['gmax']:.5f} median {e['gmed']:.5f} worst {[(k, round(v, 5)) for k, v in worst]}")


# the bars of tests/test_ref_fixtures_gpu.py::test_prenorm_encoder_reference_fixture (one bf16 rounding per residual add there; the scaled
# launches round the branch once more before the add)
BARS = {"hs": 1e-2, "last": 1e-2, "gx": 2e-2, "gmax": 3e-2, "gmed": 1.5e-2}


def _check(e, tag):
    assert e["hs"][0] == 0.0
    got = {"hs": max(e["hs"]), "last": e["last"], "gx": e["gx"], "gmax": e["gmax"], "gmed": e["gmed"]}
    for k, bar in BARS.items():
        assert got[k] < bar, (tag, k, got[k], bar)
    return got


def test_reference_encoder_with_fixed_drop_masks(golden_dir):
    f = load(golden_dir, "enc_prenorm_droppath_mfma.npz")
    for part in ("_wgrad_a", "_wgrad_b"):
        f.update(load(golden_dir, f"enc_prenorm_droppath_mfma{part}.npz"))
    L, B, N, D = 3, 4, 17, 128
    rates, keep = [float(v) for v in f["rates"]], f["keep"]
    from medmoe_amd.config import MedMoEConfig
    assert MedMoEConfig(n_layer_v=L, vit_drop_path=0.3).vit_drop_path_rates() == rates
    sc = torch.stack([keep[l] / (1.0 - rates[l]) for l in range(L)])                       # as the fixture's modules scaled, in fp32
    # all scales 1 on the EXISTING undropped 2-layer fixture: the same launches (layer 1 takes the scaled ones), nothing dropped
    f0 = load(golden_dir, "enc_prenorm_mfma.npz")
    _, e1 = _run_encoder(f0, 2, torch.ones(2, 2, B), vit_drop_path=0.3)
    _show("all-ones, undropped 2-layer fixture", e1)
    ones = _check(e1, "all-ones")
    for k, v in ones.items():
        print(f"    all-ones {k}: {v:.5f} = {v / BARS[k]:.2f} of its bar")
    eng, e = _run_encoder(f, L, sc, ff_v=128, vit_drop_path=0.3)
    _show("dropped 3-layer fixture", e)
    _check(e, "dropped")
    ws = eng.ws
    # teeth: the drops matter - against the same encoder's undropped result
    far = rel(ws["lnf"].view(B, N, D), f["last_undropped"])
    print(f"    dropped lnf against the undropped last: {far:.3f}")
    assert far > 0.1
    # a sample dropped at both sites of a layer passes the layer bit-unchanged
    x = [ws[f"x{l}"].view(B, N, D) for l in range(L + 1)]
    for l in range(L):
        for b in range(B):
            both = keep[l, 0, b] == 0 and keep[l, 1, b] == 0
            assert torch.equal(bits(x[l + 1][b]), bits(x[l][b])) == bool(both), (l, b)
    assert int(((keep[:, 0] == 0) & (keep[:, 1] == 0)).sum()) == 2


# ------------------------------------------------------------------------------------------------------------------------------
# 4. engine steps (tiny2: 4 layers, p = 0, 1/6, 1/3, 1/2; B = 8)
# ------------------------------------------------------------------------------------------------------------------------------
def _engine(rate, seed=3, dropout_seed=5, deterministic=False):
    from medmoe_amd.config import config_by_name
    from medmoe_amd.engine import Engine
    cfg = config_by_name("tiny2")
    cfg.vit_drop_path, cfg.dropout_seed, cfg.deterministic = rate, dropout_seed, deterministic
    return Engine(cfg, "cuda:0", seed=seed)


def _batches(n=3, B=8):
    import bench
    from medmoe_amd.config import config_by_name
    return [bench.synthetic_batch(config_by_name("tiny2"), B, 50 + i, "cuda:0") for i in range(n)]


def _expected_scales(eng, step, rank=0, B=8):
    """numpy restatement (tests/test_text_dropout_host.keep_mask) of the engine's draw"""
    rates = eng.cfg.vit_drop_path_rates()
    cols = (rank + 1) * B
    out = torch.zeros(len(rates), 2, B)
    for l, p in enumerate(rates):
        for j in range(2):
            k = keep_mask(1, cols, (cols + 3) // 4 * 4, eng.cfg.dropout_seed, step, SITE0 + 2 * l + j, p)[0][rank * B:]
            out[l, j] = torch.from_numpy(k.astype(np.float32)) * torch.tensor(1.0 / (1.0 - p), dtype=F32)
    return out


def test_train_step_drops_where_the_scales_say(ops):
    eng = _engine(0.5)
    B, Nt, Dv, L = 8, eng.cfg.n_tok_v, eng.cfg.d_v, eng.cfg.n_layer_v
    out = eng.train_step(_batches(1)[0])
    torch.cuda.synchronize()
    assert eng.dropout_step == 1 and eng.vit_drop_scales is None
    for k in ("loss", "g_loss", "l_loss", "classifier_loss"):
        assert np.isfinite(float(out[k])), k
    sc = eng.ws["vit_dp"].cpu()
    assert torch.equal(sc, _expected_scales(eng, 0))
    assert bool((sc[0] == 1.0).all())
    for l in range(1, L):                                             # dropout_seed 5, step 0: every site of layers 1-3 keeps some and drops some
        for j in range(2):
            assert bool((sc[l, j] == 0).any()) and bool((sc[l, j] != 0).any()), (l, j)
    ws = eng.ws
    for l in range(L):
        x, xm, xo = (ws[n].view(B, Nt, Dv) for n in (f"x{l}", f"xmid{l}", f"x{l + 1}"))
        for b in range(B):
            assert torch.equal(bits(xm[b]), bits(x[b])) == bool(sc[l, 0, b] == 0), (l, 0, b)
            assert torch.equal(bits(xo[b]), bits(xm[b])) == bool(sc[l, 1, b] == 0), (l, 1, b)
    assert bool(torch.isfinite(eng.params.g32).all()) and float(eng.params.g32.abs().max()) > 0
    eng.train_step(_batches(1)[0])
    torch.cuda.synchronize()
    assert eng.dropout_step == 2 and torch.equal(eng.ws["vit_dp"].cpu(), _expected_scales(eng, 1)) and not torch.equal(eng.ws["vit_dp"].cpu(), sc)


def test_eval_step_never_drops(ops):
    """eval_step of a rate-0.3 engine = eval_step of a rate-0 engine on the same weights, bit for bit, and no counter moves.  The loss heads of
    the default mode sum with fp32 atomics (two runs of ONE engine differ in the last bit there), so the loss dict is compared between
    deterministic engines, where evaluation repeats bit for bit (tests/test_deterministic_gpu.py); the towers' outputs are compared in both modes."""
    batch = _batches(1)[0]
    for det in (True, False):
        ed, e0 = _engine(0.3, deterministic=det), _engine(0.0, deterministic=det)
        assert torch.equal(ed.params.p32, e0.params.p32)
        ed.dropout_step = 4
        od = {k: v.clone() for k, v in ed.eval_step(batch).items()}
        o0 = e0.eval_step(batch)
        torch.cuda.synchronize()
        assert ed.dropout_step == 4 and ed.vit_drop_scales is None
        for k in o0:
            if det:
                assert torch.equal(od[k], o0[k]), k
            else:
                assert abs(float(od[k]) - float(o0[k])) <= 1e-6 * max(1.0, abs(float(o0[k]))), k
        for name in ("lnf", "img_l", "img_g", "probs"):
            assert torch.equal(bits(ed.ws[name]), bits(e0.ws[name])), (det, name)
        # after a training step too: a bare forward_image runs the undropped tower
        ed.train_step(batch, optimizer=False)
        ed.forward_image(batch["image"])
        e0.forward_image(batch["image"])
        torch.cuda.synchronize()
        assert ed.dropout_step == 5 and torch.equal(bits(ed.ws["lnf"]), bits(e0.ws["lnf"]))


def test_deterministic_mode_repeats_bit_for_bit(ops):
    batches = _batches(2)
    runs = []
    before = ops.nondet_launches()
    for _ in range(2):
        eng = _engine(0.2, deterministic=True)
        keepers = []
        for b in batches:
            out = eng.train_step(b)
            keepers += [eng.ws["vit_dp"].clone()] + [out[k].clone() for k in sorted(out)]
        torch.cuda.synchronize()
        m, v = eng.params.adam_state()
        runs.append(keepers + [eng.params.p32.clone(), m.clone(), v.clone()])
    assert ops.nondet_launches() == before, "a launch of the deterministic step took an order-dependent form"
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), i
    assert bool((runs[0][0] == 0).any())                              # something was dropped in the first step


def test_resumed_run_repeats_the_masks(ops):
    batches = _batches(3)
    a = _engine(0.5)
    for b in batches[:2]:
        a.train_step(b)
    torch.cuda.synchronize()
    r = _engine(0.5, seed=9)                                          # the state a checkpoint carries: master, moments, step counts
    r.params.p32.copy_(a.params.p32)
    for dst, src in zip(r.params.adam_state(), a.params.adam_state()):
        dst.copy_(src)
    r.params.step_count = a.params.step_count
    r.params.refresh()
    r.dropout_step = a.dropout_step
    a.train_step(batches[2]); r.train_step(batches[2])
    torch.cuda.synchronize()
    assert a.dropout_step == r.dropout_step == 3
    assert torch.equal(a.ws["vit_dp"], r.ws["vit_dp"]) and torch.equal(a.ws["vit_dp"].cpu(), _expected_scales(a, 2))
    fresh = _engine(0.5)
    fresh.train_step(batches[2])
    assert not torch.equal(fresh.ws["vit_dp"], a.ws["vit_dp"])        # step 0's masks are others


def test_ranks_draw_their_own_columns(ops):
    batch = _batches(1)[0]
    e0, e1 = _engine(0.5), _engine(0.5)
    e1.rank, e1.world = 1, 2                                          # no process group: only the column offset of the draw follows
    e0.train_step(batch, optimizer=False); e1.train_step(batch, optimizer=False)
    torch.cuda.synchronize()
    whole = scales(ops, [p for p in e0.cfg.vit_drop_path_rates() for _ in range(2)], 16, 0, 5, 0).view(4, 2, 16)
    assert torch.equal(e0.ws["vit_dp"], whole[:, :, :8]) and torch.equal(e1.ws["vit_dp"], whole[:, :, 8:])
    assert torch.equal(e1.ws["vit_dp"].cpu(), _expected_scales(e1, 0, rank=1)) and not torch.equal(e0.ws["vit_dp"], e1.ws["vit_dp"])
