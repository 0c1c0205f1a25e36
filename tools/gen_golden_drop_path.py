"""TEST INFRASTRUCTURE ONLY.  Generates tests/golden/enc_prenorm_droppath_mfma*.npz: the REFERENCE's own pre-norm TransformerEncoder with
stochastic depth (drop_path_rate = 0.3 over 3 layers: p = 0, 0.15, 0.3) under FIXED per-sample keep masks, so that the GPU test
(tests/test_vit_drop_path_gpu.py) can feed the reference's numbers straight to Engine._vit_blocks / _vit_backward with the same masks injected.
Run in the build container only:  python tools/gen_golden_drop_path.py
The fixture holds data (weights, inputs, masks, expected outputs / gradients) - no reference source.  Matrices and inputs are bf16 values.
Three compressed files, each below 1 MiB: enc_prenorm_droppath_mfma.npz (weights, x, gy, keep, rates, hidden states, last, last_undropped, gx,
the gradients of the vectors), ..._wgrad_a.npz (the gradients of the fused q / k / v projections), ..._wgrad_b.npz (the gradients of the other matrices).

The reference gives a layer ONE StochasticDepth object for both branches (attention_dropout is feedforward_dropout); here each branch gets a
module of its own, y = x * keep[b] / (1 - p_l): what StochasticDepth(p_l, mode="row") computes for the drawn row mask `keep`."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import _ref_import  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "enc_prenorm_droppath_mfma")
L, D, H, FF, B, N, RATE = 3, 128, 2, 128, 4, 17, 0.3
# keep[l][site][b]; layer 0 has p = 0.  Layer 1: sample 1 dropped at both sites, 2 at the feed-forward site only, 3 at the attention site only;
# layer 2: sample 2 at both, 3 feed-forward only, 1 attention only; sample 0 is kept everywhere
KEEP = [[[1, 1, 1, 1], [1, 1, 1, 1]],
        [[1, 0, 1, 0], [1, 0, 0, 1]],
        [[1, 0, 0, 1], [1, 1, 0, 0]]]


class FixedRowMask(torch.nn.Module):
    def __init__(self, keep, p):
        super().__init__()
        self.register_buffer("scale", torch.tensor(keep, dtype=torch.float32) / (1.0 - p), persistent=False)

    def forward(self, x):
        return x * self.scale.view(-1, *([1] * (x.dim() - 1)))


def bf(t):
    return t.to(torch.bfloat16).float()


def main():
    R = _ref_import.load()
    nn = torch.nn
    torch.manual_seed(9015)
    enc = R.transformer.TransformerEncoder(L, D, H, FF, 0.0, nn.GELU, 1e-6, True, 1e-6, drop_path_rate=RATE)
    rates = [float(v) for v in torch.linspace(0, RATE, L)]
    for l, layer in enumerate(enc.layer):
        assert layer.attention_dropout is layer.feedforward_dropout and abs(layer.attention_dropout.p - rates[l]) < 1e-7
        layer.attention_dropout = FixedRowMask(KEEP[l][0], rates[l])
        layer.feedforward_dropout = FixedRowMask(KEEP[l][1], rates[l])
    for mod in enc.modules():
        if isinstance(mod, nn.LayerNorm):
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.uniform_(-0.2, 0.2)
        elif isinstance(mod, nn.Linear):
            mod.weight.data.mul_(2.0)
            mod.bias.data.uniform_(-0.1, 0.1)
    with torch.no_grad():
        for p in enc.parameters():
            if p.dim() >= 2:
                p.copy_(bf(p))
    x = bf(torch.randn(B, N, D)).requires_grad_(True)
    out = enc(x, attention_mask=None, return_hidden_states=True)
    gy = bf(torch.randn_like(out.last_hidden_state))
    (out.last_hidden_state * gy).sum().backward()
    d = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    d.update(x=x, gy=gy, last=out.last_hidden_state, gx=x.grad, keep=torch.tensor(KEEP, dtype=torch.float32),
             rates=torch.tensor(rates, dtype=torch.float64))
    for i, h in enumerate(out.hidden_states):
        d[f"hs{i}"] = h
    for k, v in enc.named_parameters():
        d["grad." + k] = v.grad
    # the same encoder with nothing dropped (every branch scaled by 1): what the dropped result must differ from
    for layer in enc.layer:
        layer.attention_dropout, layer.feedforward_dropout = torch.nn.Identity(), torch.nn.Identity()
    with torch.no_grad():
        d["last_undropped"] = enc(x, attention_mask=None).last_hidden_state
    # the mechanism: a sample dropped at both sites of a layer passes it unchanged
    hs = out.hidden_states
    assert torch.equal(hs[2][1], hs[1][1]) and torch.equal(hs[3][2], hs[2][2]) and not torch.equal(hs[2][0], hs[1][0])
    d = {k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in d.items()}
    wgrad = [k for k in d if k.startswith("grad.") and d[k].ndim >= 2]
    parts = {"": [k for k in d if k not in wgrad], "_wgrad_a": [k for k in wgrad if "input_proj" in k], "_wgrad_b": [k for k in wgrad if "input_proj" not in k]}
    for tag, keys in parts.items():
        fn = OUT + tag + ".npz"
        np.savez_compressed(fn, **{k: d[k] for k in keys})
        print(f"{fn}: {os.path.getsize(fn)} B, {len(keys)} arrays")
        assert os.path.getsize(fn) < 1 << 20


if __name__ == "__main__":
    main()
