"""The rule both engines share: ONE clip norm over all flat stores of a model (the sum of every store's `sumsq()`), then `adam_step(total, ...)`
on each - against `torch.optim.Adam` + `clip_grad_norm_` over the union of the stores' parameters."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def test_one_clip_norm_over_two_flat_stores_matches_torch_adam(monkeypatch):
    """Two FlatStores (3112 elements: a [64, 32] GEMM weight, a group of two [16, 32] GEMM weights, an odd-sized bias; 1008 elements: no
    GEMM weight), seeded gradients whose joint norm is far above the clip, three steps of total = a.sumsq() + b.sumsq(); adam_step(total) on
    both.  p32, m, v: 1e-6 relative L2 against torch (the bar of test_fused_clip_adam_matches_torch_adam); p16 is the rounded master bit
    for bit; p16t of the GEMM weight and of both group members are the transposes of their p16 views bit for bit; the store without a
    transpose table launches no transpose, the other exactly one per step."""
    from medmoe_amd import ops
    from medmoe_amd.flat import FlatStore
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g) * 0.05
    wa = {"lin.weight": rn(64, 32), "k.weight": rn(16, 32), "q.weight": rn(16, 32), "lin.bias": rn(37)}
    wb = {"table": rn(30, 11), "scale": rn(601), "gate": rn(7, 9)}
    a = FlatStore(wa, "cuda", groups=[("qk", ["q.weight", "k.weight"])], gemm=["lin.weight", "q.weight", "k.weight"])
    b = FlatStore(wb, "cuda")
    assert (a.numel, b.numel) == (3112, 1008) and b.tr_table is None and not a.has_adam_state() and not b.has_adam_state()
    assert a.offsets["q.weight"] == 0 and a.offsets["k.weight"] == 512 and a.shapes["qk"] == (32, 32)
    launched = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *args: (launched.append((name, args[0].data_ptr())), real(name, *args))[1])
    stores = ((a, wa), (b, wb))
    ref = {(i, n): torch.nn.Parameter(w.clone().cuda()) for i, (_, ws) in enumerate(stores) for n, w in ws.items()}
    clip, lr = 0.25, 1e-3
    opt = torch.optim.Adam(list(ref.values()), lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    for step in range(1, 4):
        for i, (st, ws) in enumerate(stores):
            st.zero_grad()                                          # the padding between entries carries no gradient
            for n in ws:
                gr = (torch.randn(ws[n].shape, generator=g) * (1.0 + step)).cuda()
                st.grad(n).copy_(gr)
                ref[(i, n)].grad = gr.clone()
        total = a.sumsq() + b.sumsq()
        tn = torch.nn.utils.clip_grad_norm_(list(ref.values()), clip)
        assert float(tn) > 10 * clip and abs(float(total.sqrt()) - float(tn)) < 1e-5 * float(tn)
        a.adam_step(total, lr, 0.0, clip)
        b.adam_step(total, lr, 0.0, clip)
        opt.step()
        for i, (st, ws) in enumerate(stores):
            assert st.step_count == step and st.has_adam_state()
            m, v = st.adam_state()
            cat = lambda f: torch.cat([f(n).reshape(-1) for n in ws])       # the store's parameters, as that test compares one flat tensor
            assert rel(cat(st.f32), cat(lambda n: ref[(i, n)])) < 1e-6, (step, i)
            assert rel(cat(lambda n: st.view(m, n)), cat(lambda n: opt.state[ref[(i, n)]]["exp_avg"])) < 1e-6, (step, i)
            assert rel(cat(lambda n: st.view(v, n)), cat(lambda n: opt.state[ref[(i, n)]]["exp_avg_sq"])) < 1e-6, (step, i)
            assert torch.equal(st.p16, st.p32.to(torch.bfloat16)), step
        for n in ("lin.weight", "q.weight", "k.weight"):
            assert torch.equal(a.w16t(n), a.w16(n).t()), (step, n)
    torch.cuda.synchronize()
    transposes = [p for name, p in launched if name == "transpose_many"]
    assert transposes == [a.p16.data_ptr()] * 3
    assert [name for name, p in launched if p == b.g32.data_ptr() or p == b.p32.data_ptr()] == ["sumsq_det", "adam_step"] * 3
