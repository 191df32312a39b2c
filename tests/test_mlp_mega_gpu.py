"""The one-launch MLP training step (csrc/kernels/mlp_fused.hip, models/mlp_mega.py) against the layer-by-layer
fused path (FusedMLP + the optimiser's own launch) and a plain fp32 PyTorch reference of the same step.
Element-level checks of every phase against float64: test_mlp_mega_exact_gpu.py (mlp_mega_exact.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _pair(make, opt_cls, gpu, **kw):
    torch.manual_seed(0)
    a = make().to(gpu)
    b = make().to(gpu)
    b.load_state_dict(a.state_dict())
    return a, opt_cls(a.parameters(), **kw), b, opt_cls(b.parameters(), **kw)


def _batch(gpu, B=128, seed=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.rand(B, 1, 28, 28, generator=g).to(gpu)
    y = torch.randint(0, 10, (B,), generator=g).to(gpu)
    return x, y


@pytest.mark.parametrize("cfg", ["reference_adam", "small_sgd_momentum"])
def test_mega_step_matches_layerwise_path(gpu, cfg):
    from pytorch_distributed_examples_amd import _native
    from pytorch_distributed_examples_amd.models.mlp import MLP, reference_mlp
    from pytorch_distributed_examples_amd.models.mlp_fused import FusedMLP
    from pytorch_distributed_examples_amd.models.mlp_mega import MegaMLP
    from pytorch_distributed_examples_amd.ops.optim import FusedAdam, FusedSGD

    assert _native.C().mlp_train_grid() > 0
    if cfg == "reference_adam":
        ma, oa, mb, ob = _pair(reference_mlp, FusedAdam, gpu, lr=1e-3)
    else:
        ma, oa, mb, ob = _pair(lambda: MLP(hidden_layers=1, features=256), FusedSGD, gpu, lr=0.05, momentum=0.9)
    fm = FusedMLP(ma)
    mega = MegaMLP(mb, ob)
    for step in range(3):
        x, y = _batch(gpu, seed=step + 1)
        la = fm.forward_backward(x, y)
        oa.step()
        lb = mega.step(x, y)
        torch.cuda.synchronize()
        assert abs(float(la) - float(lb)) < 2e-3 * max(1.0, abs(float(la))), (step, float(la), float(lb))
        for (n, pa), pb in zip(ma.named_parameters(), mb.parameters()):
            ga, gb = pa.grad.float(), pb.grad.float()
            scale = ga.abs().max().item() + 1e-12
            assert (ga - gb).abs().max().item() <= 3e-2 * scale, (step, n, (ga - gb).abs().max().item(), scale)
            # updates: identical math on (nearly) identical gradients; Adam's normalised step can differ by up to
            # 2 lr where a gradient component is ~0 and its sign flips between the two accumulation orders
            dp = (pa.detach() - pb.detach()).abs()
            # SGD: the same update of the same gradient up to summation order (a stale-gradient race showed up here
            # as 1e-4 differences in the first layer)
            tol = 2.5e-3 if cfg == "reference_adam" else 2e-5
            assert dp.max().item() <= tol, (step, n, dp.max().item())
            assert (dp > 1e-4).float().mean().item() < 0.02, (step, n)
    assert mega.errors() == 0
    # the device step counter advanced once per step, like the optimiser's own launch
    sa = oa._dev[0]["step"][0].item()
    sb = ob._dev[0]["step"][0].item()
    assert sa == sb == 3
    # the bf16 copies the layers read were refreshed: an eager forward of both models agrees
    x, _ = _batch(gpu, seed=9)
    with torch.no_grad():
        assert torch.allclose(ma(x).float(), mb(x).float(), atol=5e-2, rtol=5e-2)


def test_mega_gradients_match_fp32_reference(gpu):
    """One step's loss and gradients against plain fp32 autograd on the same (bf16-rounded) weights and inputs.
    Seven layers of bf16 activations and gradients leave a few per cent of relative error in the first layers'
    gradients on ANY bf16 path: the one-launch step must be as close to fp32 as the layer-by-layer path is."""
    from pytorch_distributed_examples_amd.models.mlp import reference_mlp
    from pytorch_distributed_examples_amd.models.mlp_fused import FusedMLP
    from pytorch_distributed_examples_amd.models.mlp_mega import MegaMLP
    from pytorch_distributed_examples_amd.ops.optim import FusedSGD

    torch.manual_seed(3)
    m = reference_mlp().to(gpu)
    m2 = reference_mlp().to(gpu)
    m2.load_state_dict(m.state_dict())
    ref = [(L.weight.detach().to(torch.bfloat16).float().clone(), L.bias.detach().clone())
           for L in [m.input_layer, *m.hidden_layers, m.final_layer]]
    opt = FusedSGD(m.parameters(), lr=0.0)  # lr 0: the weights stay, the step still runs end to end
    x, y = _batch(gpu, seed=5)
    loss = MegaMLP(m, opt).step(x, y)
    loss2 = FusedMLP(m2).forward_backward(x, y)
    torch.cuda.synchronize()
    h = x.reshape(x.shape[0], -1).to(torch.bfloat16).float()
    ws = [torch.nn.Parameter(w) for w, _ in ref]
    bs = [torch.nn.Parameter(b) for _, b in ref]
    for i, (w, b) in enumerate(zip(ws, bs)):
        h = h @ w.t() + b
        if i < len(ws) - 1:
            h = torch.relu(h)
    lref = torch.nn.functional.cross_entropy(h, y)
    lref.backward()
    assert abs(float(loss) - float(lref)) < 1e-2 * max(1.0, float(lref)), (float(loss), float(lref))
    assert abs(float(loss2) - float(lref)) < 1e-2 * max(1.0, float(lref)), (float(loss2), float(lref))

    def rel(got, want):
        return (got - want).norm().item() / (want.norm().item() + 1e-12)

    layers = [m.input_layer, *m.hidden_layers, m.final_layer]
    layers2 = [m2.input_layer, *m2.hidden_layers, m2.final_layer]
    for i, (L, L2, w, b) in enumerate(zip(layers, layers2, ws, bs)):
        for got, other, want in ((L.weight.grad, L2.weight.grad, w.grad), (L.bias.grad, L2.bias.grad, b.grad)):
            e_mega, e_layer = rel(got, want), rel(other, want)
            assert e_mega < 0.15 and e_mega <= max(1.25 * e_layer, 0.02), (i, e_mega, e_layer)


def test_mega_step_captures_into_a_graph(gpu):
    from pytorch_distributed_examples_amd.models.mlp import reference_mlp
    from pytorch_distributed_examples_amd.models.mlp_mega import MegaMLP
    from pytorch_distributed_examples_amd.ops.optim import FusedAdam
    from pytorch_distributed_examples_amd.utils.graph import CapturedStep

    torch.manual_seed(4)
    m = reference_mlp().to(gpu)
    opt = FusedAdam(m.parameters(), lr=1e-3)
    mega = MegaMLP(m, opt)
    x, y = _batch(gpu, seed=7)
    g = CapturedStep(mega.step, [x, y], warmup=1).capture()
    first = float(g(x, y))
    for _ in range(30):
        last = g(x, y)
    torch.cuda.synchronize()
    assert float(last) < first, (first, float(last))  # the same batch: the loss falls
    assert mega.errors() == 0
    assert opt._dev[0]["step"][0].item() == 1 + 31  # the eager warm-up step + 31 replays (capture runs nothing)


def test_fused_update_is_bitwise_the_unfused_one(gpu, monkeypatch):
    """The fused backward window (each weight tile updated straight from its gradient accumulators, its W^T tile
    parked in LDS until the next window) against the unfused form (update one window later, gradient read back):
    the same fp32 values through the same update -- weights, their optimiser state, all gradients and both bf16
    copies bitwise equal after three Adam steps (biases to an ulp)."""
    from pytorch_distributed_examples_amd.models.mlp import reference_mlp
    from pytorch_distributed_examples_amd.models.mlp_mega import MegaMLP
    from pytorch_distributed_examples_amd.ops import functional as OF
    from pytorch_distributed_examples_amd.ops.optim import FusedAdam

    ma, oa, mb, ob = _pair(reference_mlp, FusedAdam, gpu, lr=1e-3)
    fa, fb = MegaMLP(ma, oa), MegaMLP(mb, ob)
    assert fa.fused_update()
    for step in range(3):
        x, y = _batch(gpu, seed=step + 11)
        monkeypatch.setenv("PDE_MLP_FUSE", "1")
        la = fa.step(x, y)
        monkeypatch.setenv("PDE_MLP_FUSE", "0")
        lb = fb.step(x, y)
        torch.cuda.synchronize()
        assert float(la) == float(lb), step
    assert fa.errors() == 0 and fb.errors() == 0
    bad = []
    for (n, pa), pb in zip(ma.named_parameters(), mb.parameters()):
        for what, ta, tb in (("param", pa, pb), ("grad", pa.grad, pb.grad), ("m", oa.state[pa]["exp_avg"],
                             ob.state[pb]["exp_avg"]), ("v", oa.state[pa]["exp_avg_sq"], ob.state[pb]["exp_avg_sq"])):
            # biases: the same update, but its scalar instance may be contracted to FMAs differently by the
            # compiler in the two code paths (r5za: 1-ulp differences, gradients bitwise equal)
            same = torch.equal(ta, tb) if ta.dim() > 1 or what == "grad" else \
                torch.allclose(ta, tb, rtol=1e-5, atol=1e-9)
            if not same:
                d = (ta - tb).abs()
                bad.append((n, what, d.max().item(), int((d > 0).sum().item()), int(d.flatten().argmax().item())))
    assert not bad, bad
    layers_a = [ma.input_layer, *ma.hidden_layers, ma.final_layer]
    layers_b = [mb.input_layer, *mb.hidden_layers, mb.final_layer]
    for i, (La, Lb) in enumerate(zip(layers_a, layers_b)):
        assert torch.equal(OF._maintained(La.weight, "bf16"), OF._maintained(Lb.weight, "bf16")), i
        if i > 0:
            ld = 32 if i == len(layers_a) - 1 else La.out_features
            ta = OF.maintain_transposed_copy(La.weight, ld)
            tb = OF.maintain_transposed_copy(Lb.weight, ld)
            assert torch.equal(ta, tb), i
            # and it IS the transpose of the updated weights
            assert torch.equal(ta[:, :La.out_features], La.weight.detach().to(torch.bfloat16).t()), i


def test_mega_in_launch_exchange_loopback_is_bitwise(gpu):
    """World > 1 form of the one-launch step (every weight-gradient tile exchanged over xGMI inside the launch,
    mlp_fused.hip xchg_tile) armed on a ONE-rank view: staging, flags and the rank-order read all run, the sum of
    one rank x 1.0 must reproduce the plain step bit for bit (losses, weights, Adam state), and the in-launch
    exchange epochs advance once per launch."""
    from pytorch_distributed_examples_amd.models.mlp import reference_mlp
    from pytorch_distributed_examples_amd.models.mlp_mega import MegaMLP
    from pytorch_distributed_examples_amd.ops.optim import FusedAdam

    ma, oa, mb, ob = _pair(reference_mlp, FusedAdam, gpu, lr=1e-3)
    plain = MegaMLP(ma, oa)
    xa = MegaMLP.exchange(mb, gpu)
    armed = MegaMLP(mb, ob, xgmi=xa)
    for step in range(3):
        x, y = _batch(gpu, seed=step + 11)
        la = plain.step(x, y)
        lb = armed.step(x, y)
        torch.cuda.synchronize()
        assert la.item() == lb.item(), (step, la.item(), lb.item())
    for pa, pb in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(pa, pb)
        assert torch.equal(pa.grad, pb.grad)
        sa, sb = oa.state[pa], ob.state[pb]
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
    armed.check()
    plain.check()
    xa.close()
