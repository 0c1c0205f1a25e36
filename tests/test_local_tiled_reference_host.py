"""The float64 restatements of tests/local_tiled_reference.py proved on the CPU: without any fp16 / bf16 rounding their chain scores -> pair
forward -> pair backward reproduces medmoe_oracle.gloria_local_sim and the autograd gradient of the oracle's local loss with respect to the
image features and the words, 1e-9 relative - at the three tiled geometries with ragged caption lengths.  The bar is the one the
generic-kernel file uses for its own chain."""
import pytest
import torch

import medmoe_oracle as O
from local_tiled_reference import F64, LOGP_MIN, chain, clamp_caps, ref_bwd_s, ref_scores

T1, T2 = 4.0, 5.0
GEOMETRIES = [(8, 8, 16, [16, 1, 7]), (14, 14, 77, [77, 1, 33]), (16, 16, 77, [65, 17, 48])]


def _inputs(H, W, T, seed):
    B, D = 3, 16
    g = torch.Generator().manual_seed(seed)
    img = (0.7 * torch.randn(B, D, H, W, generator=g, dtype=F64)).requires_grad_(True)
    words = (0.7 * torch.randn(B, D, T, generator=g, dtype=F64)).requires_grad_(True)
    return B, D, img, words


@pytest.mark.parametrize("H,W,T,caps", GEOMETRIES)
def test_chain_reproduces_the_oracle(H, W, T, caps):
    B, D, img, words = _inputs(H, W, T, seed=H + T)
    sim_o = O.gloria_local_sim(img, words, caps, T1, T2)[0]
    l0, l1, _ = O.gloria_local(img, words, caps, T1, T2, 10.0)
    (l0 + l1).backward()
    got = chain(img.detach().reshape(B, D, H * W).transpose(1, 2), words.detach().transpose(1, 2), caps, T1, T2)
    for name, a, b in (("sim", got["sim"], sim_o.detach()), ("d ctx", got["dctx"], img.grad.reshape(B, D, H * W).transpose(1, 2)),
                       ("d words", got["dwords"], words.grad.transpose(1, 2))):
        e = float((a - b).abs().max() / b.abs().max())
        print(f"HW={H * W} T={T} {name}: {e:.2e}")
        assert e < 1e-9, (name, e)


@pytest.mark.parametrize("H,W,T,caps", GEOMETRIES)
def test_closed_form_ca_is_the_generic_softmax_backward(H, W, T, caps):
    """Without the bf16 rounding of A the closed form cA = dn num + d2 n2 is sum_hw A dA, so a1 (da1 - rd) of ref_pair_bwd is ref_bwd_s of the
    generic-geometry file on the same dA; dS adds dn A, the direct path of num through S."""
    B, D, img, words = _inputs(H, W, T, seed=H + T + 1)
    got = chain(img.detach().reshape(B, D, H * W).transpose(1, 2), words.detach().transpose(1, 2), caps, T1, T2)
    f, bw = got["fwd"], got["bwd"]
    want = ref_bwd_s(got["lp"], f["A"], bw["dA"], got["caps"], H * W, T1) + bw["dn"][:, None] * f["A"]
    assert float((bw["dS"] - want).abs().max()) < 1e-12 * float(want.abs().max())


def test_scores_contract_edges():
    """LOGP_MIN exactly on every word at or beyond cap, an empty caption counted as its first word (lp = 0, lse = S_0), the log2 form."""
    g = torch.Generator().manual_seed(3)
    ctx, words = torch.randn(2, 5, 8, generator=g, dtype=F64), torch.randn(3, 9, 8, generator=g, dtype=F64)
    caps = clamp_caps([0, 4, 30], 9, 16)
    assert caps == [1, 4, 9]
    r, r2 = ref_scores(ctx, words, torch.tensor(caps), 16), ref_scores(ctx, words, torch.tensor(caps), 16, log2=True)
    for i, c in enumerate(caps):
        assert bool((r["lp"][:, :, i, c:] == LOGP_MIN).all()) and bool((r["lp"][:, :, i, :c] > LOGP_MIN).all())
        assert torch.allclose(torch.exp(r["lp"][:, :, i, :c]).sum(-1), torch.ones(2, 5, dtype=F64), atol=1e-12)
        assert torch.allclose(torch.exp2(r2["lp"][:, :, i, :c]).sum(-1), torch.ones(2, 5, dtype=F64), atol=1e-12)
    assert bool((r["lp"][:, :, 0, 0] == 0).all()) and torch.equal(r["lse"][:, :, 0], r["S"][:, :, 0, 0])
