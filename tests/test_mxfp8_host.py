"""MXFP8 expert format (DESIGN.md "MXFP8 expert weights"), host side: the torch twin of the quantisation rule and its properties,
the named configurations, the flag check, the library's three entry points.  tests/test_mxfp8_gpu.py checks the kernels against
this twin bit for bit."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F8 = torch.float8_e4m3fn


def mx_quant(x):
    """[..., K] (K % 32 == 0) -> (e4m3 bytes [..., K], E8M0 scale bytes [..., K/32]), blocks of 32 along the last dimension.
    s = amax * (1/448) in fp32; e = biased exponent of s, plus one if any mantissa bit is set (round UP to a power of two), clamped
    to [1, 254], 127 for an all-zero block; elements = rne_e4m3(v * 2^(127 - e)) - an exact multiplication."""
    shp = x.shape
    v = x.float().reshape(*shp[:-1], shp[-1] // 32, 32)
    amax = v.abs().amax(-1)
    bits = (amax * torch.tensor(1.0 / 448.0, dtype=torch.float32, device=x.device)).view(torch.int32)
    e = ((bits >> 23) & 0xff) + ((bits & 0x7fffff) != 0).to(torch.int32)
    e = torch.where(amax > 0, e.clamp(1, 254), torch.full_like(e, 127))
    inv = torch.where(e < 254, (254 - e) << 23, torch.full_like(e, 0x00400000)).view(torch.float32)
    q = (v * inv[..., None]).to(F8).view(torch.uint8).reshape(shp)
    return q, e.to(torch.uint8)


def mx_dequant(q, e):
    shp = q.shape
    scale = (e.to(torch.int32) << 23).view(torch.float32)            # 2^(e - 127), e >= 1
    return (q.view(F8).float().reshape(*shp[:-1], shp[-1] // 32, 32) * scale[..., None]).reshape(shp)


def fake_quant_mx(x):
    """The oracle's fake_quant_rows in this format: quantise-dequantise along the last dimension, straight-through gradient."""
    q, e = mx_quant(x.detach())
    return x + (mx_dequant(q, e) - x.detach())


def edge_rows(K):
    """Rows that exercise the rule's corners: all zero; one huge element in an otherwise small block; amax / 448 exactly a power of
    two (448 * 2^-3 = 56) and one bf16 step above it."""
    r = torch.zeros(5, K)
    r[1] = 1e-3 * torch.randn(K, generator=torch.Generator().manual_seed(1)); r[1, 5] = 28672.0
    r[2] = torch.linspace(-56.0, 56.0, K)
    r[3] = r[2]; r[3, 0] = -56.25
    r[4, 40] = 2.0 ** -20
    return r.to(torch.bfloat16).float()


def test_mx_twin_properties():
    torch.manual_seed(0)
    x = torch.randn(4096, 256) * torch.rand(4096, 1) * 8
    x[:5] = edge_rows(256)
    q, e = mx_quant(x)
    v = x.reshape(4096, 8, 32)
    amax = v.abs().amax(-1)
    f = q.view(F8).float()
    assert not torch.isnan(f).any() and float(f.abs().max()) <= 448.0
    # every scale is the smallest power of two that is >= amax / 448
    s = amax.double() / 448.0
    p2 = torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double() - 127.0)
    nz = amax > 0
    assert (p2[nz] >= s[nz]).all() and (p2[nz] * 0.5 < s[nz]).all()
    # all-zero block: byte 127 and zero elements
    assert (e[~nz] == 127).all() and int((~nz).sum()) >= 8 and (q[0] == 0).all()
    # amax / 448 exactly a power of two is not rounded up: 56 = 448 * 2^-3 maps to 448 (byte 0x7e) under scale byte 124
    assert int(e[2, 0]) == 124 and int(e[2, 7]) == 124 and int(q[2, 255]) == 0x7E and int(q[2, 0]) == 0xFE
    assert int(e[3, 0]) == 125 and int(e[3, 7]) == 124                   # one bf16 step above the boundary: the next power of two
    # one huge element in a small block: the block's scale follows it, the small elements underflow to zero, nothing overflows
    assert int(e[1, 0]) == 133 and mx_dequant(q, e)[1, 5] == x[1, 5] and (q[1, :5] & 0x7f).max() == 0
    # dequantised error: at most 2^-4 of the block's amax (half a unit of the 3-bit mantissa in the top binade, 16 / 272 at worst)
    err = (mx_dequant(q, e) - x).reshape(4096, 8, 32).abs().amax(-1)
    ratio = float((err[nz] / amax[nz]).max())
    print("mx_quant: worst |error| / amax", ratio, "largest magnitude", float(f.abs().max()))
    assert ratio <= 2.0 ** -4
    # the straight-through twin is the dequantised value with the gradient of the identity
    t = x[:8].clone().requires_grad_(True)
    y = fake_quant_mx(t)
    y.sum().backward()
    assert torch.equal(y.detach(), mx_dequant(q, e)[:8]) and torch.equal(t.grad, torch.ones_like(t))


def test_mx_configs_and_flag_check():
    from medmoe_amd.config import config_by_name
    c4, c4f = config_by_name("cfg4_mx"), config_by_name("cfg4")
    assert c4.expert_mx and not c4.expert_fp8 and c4f.expert_fp8 and not c4f.expert_mx
    for k in ("patch", "d_v", "n_layer_v", "n_head_v", "ff_v", "n_expert", "top_k", "d_out", "img_size", "max_len"):
        assert getattr(c4, k) == getattr(c4f, k), k
    t, tl = config_by_name("tinyL8mx"), config_by_name("tinyL")
    assert t.expert_mx and not t.expert_fp8 and not tl.expert_mx
    assert (t.d_v, t.d_out, t.n_expert, t.top_k, t.n_patch) == (tl.d_v, tl.d_out, tl.n_expert, tl.top_k, tl.n_patch)
    c4.validate(); t.validate()
    t.expert_fp8 = True
    with pytest.raises(ValueError):
        t.validate()


def test_mxfp8_hydra_key_and_experiment(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    from medmoe_amd.hydra_lite import compose
    from src.models.components.med_moe import config_from_hydra
    mm = compose(os.path.join(ROOT, "configs"), "train.yaml", ["experiment=pretraining_medmoe_cfg4_mx"])
    v = mm.model.model.vision
    assert (v.arch, v.num_experts, v.top_k, v.expert_dtype) == ("vit_l14", 16, 2, "mxfp8") and mm.model.fused_step is True
    c = config_from_hydra(v, mm.model.model.text)
    assert c.expert_mx and not c.expert_fp8 and (c.d_v, c.n_expert, c.top_k, c.max_len) == (1024, 16, 2, 77)
    bad = dict(v); bad["expert_dtype"] = "fp4"
    with pytest.raises(NotImplementedError, match="bf16.*fp8.*mxfp8"):
        config_from_hydra(bad, mm.model.model.text)


def test_library_exports_the_mx_entry_points():
    from medmoe_amd import lib_path, ops
    if not os.path.exists(lib_path()):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(lib_path())
    hdr = open(os.path.join(ROOT, "include", "medmoe_hip.h")).read()
    for n in ("quant_rows_mx", "quant_weights_mx", "gemm_mx_grouped"):
        assert hasattr(lib, "medmoe_" + n) and f"int medmoe_{n}(" in hdr and n in ops._SIGS, n
