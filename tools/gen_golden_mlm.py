"""TEST INFRASTRUCTURE ONLY.  Generates tests/golden/mlm_head.npz: the REFERENCE's own MaskedPredictionLoss (losses.py:189-245: dense + GELU +
fp32 LayerNorm + decoder with an output-only bias, cross-entropy over the positions whose label is not -1) in float64, so that the GPU test
(tests/test_zz_mlm_engine_gpu.py::test_reference_fixture_through_src_losses) can hold the fused head against the reference's numbers.
Run in the build container only:  python tools/gen_golden_mlm.py
The fixture holds data - seeded parameters, hidden_states, masked_labels, the loss, the selected rows' logsumexp and every gradient - and no
reference source.  The model runs in float64; parameters, hidden states and gradients are stored as fp32 (the parameters exactly), the loss
and the logsumexp as float64.  Matrices and hidden states are bf16 values (the operands the MFMA path reads); two cases, keys prefixed c0_ / c1_:
hidden 64 / vocab 97 (B = 2, T = 5, 3 masked tokens) and hidden 128 / vocab 300 (B = 3, T = 9, 7 masked tokens, one of them the last id)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import _ref_import  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "mlm_head.npz")
CASES = [(64, 97, 2, 5, 3), (128, 300, 3, 9, 7)]            # hidden, vocab, B, T, masked tokens


def bf(t):
    return t.to(torch.bfloat16).to(torch.float64)


def main():
    ref = _ref_import.load()
    out = {}
    for i, (D, V, B, T, n_mask) in enumerate(CASES):
        g = torch.Generator().manual_seed(2300 + i)
        m = ref.losses.MaskedPredictionLoss(hidden_size=D, vocab_size=V).double()
        m.train()
        with torch.no_grad():
            m.cls.dense.weight.copy_(bf(torch.randn(D, D, generator=g) / D ** 0.5))
            m.cls.dense.bias.copy_((torch.randn(D, generator=g) * 0.1).double())
            m.cls.layer_norm.weight.copy_((1.0 + torch.randn(D, generator=g) * 0.1).double())
            m.cls.layer_norm.bias.copy_((torch.randn(D, generator=g) * 0.1).double())
            m.cls.decoder.weight.copy_(bf(torch.randn(V, D, generator=g) / D ** 0.5))
            m.cls.bias.copy_((torch.randn(V, generator=g) * 0.1).double())
        hidden = bf(torch.randn(B, T, D, generator=g)).requires_grad_(True)
        labels = torch.full((B * T,), -1, dtype=torch.int64)
        pos = torch.randperm(B * T, generator=g)[:n_mask]
        labels[pos] = torch.randint(0, V, (n_mask,), generator=g)
        labels[pos[0]] = V - 1
        labels = labels.view(B, T)
        res = m(hidden, labels)
        res["loss"].backward()
        sel = labels.ne(-1)
        p = f"c{i}_"
        out[p + "hidden_states"] = hidden.detach().numpy().astype(np.float32)
        out[p + "masked_labels"] = labels.numpy()
        out[p + "loss"] = res["loss"].detach().numpy()
        out[p + "lse"] = torch.logsumexp(res["logits"].detach(), dim=-1).numpy()
        out[p + "grad_hidden"] = hidden.grad.numpy().astype(np.float32)
        for name, prm in m.named_parameters():
            out[p + name] = prm.detach().numpy().astype(np.float32)          # fp32-exact values: seeded in fp32 (vectors) / bf16 (matrices)
            assert np.array_equal(out[p + name].astype(np.float64), prm.detach().numpy())
            out[p + "grad_" + name] = prm.grad.numpy().astype(np.float32)
        assert int(sel.sum()) == n_mask
        print(f"case {i}: hidden {D} vocab {V}, {n_mask} masked tokens, loss {float(res['loss'].detach()):.4f}; parameters {[n for n, _ in m.named_parameters()]}")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
