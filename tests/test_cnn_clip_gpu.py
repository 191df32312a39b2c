"""The fused CNN's post-all-reduce update with global-norm gradient clipping in ONE launch (k_cnn_opt_clip<MODE>,
csrc/kernels/cnn_fused.hip): ``forward_backward(x, y, grad_out=flat)`` then ``opt_step`` with ``max_grad_norm``,
against the float64 clip-then-update applied to the same flat gradient buffer read back from the device.

Weights and state: the bound scheme of the optimiser tests (test_optim_trust_gpu.held over the flat vectors), e32
being the error of the class's own fp32 ``_cpu_step`` with clipping.

The reported norm.  Every workgroup sums the 21,840 squares in one order: 22 float4 per thread = 88 fused
multiply-adds in a chain, 6 butterfly levels, 3 adds over the four waves: depth 97.  Every term is non-negative, so
the sum is within (1 + 2^-24)^97 - 1 < 97.001 x 2^-24 relative of the exact one; the square root halves that and adds
its own rounding, the multiplication by |grad_scale| one more: NORM_RTOL = (97 / 2 + 2.01) x 2^-24 = 3.0e-6.  The
coefficient adds the sum with 1e-6 and the quotient: two more roundings.  Measured on an MI355X: at most 0.05 of the
tolerance, and at most 0.24 of any L2 bound of weights and state.

Eval mode (no dropout), batches 6 (two workgroups) and 130 (33), as tests/test_cnn_fused_optim_gpu.py.
"""
import pytest
import torch
from test_optim_clip_gpu import fused, ref64
from test_optim_trust_gpu import held

pytestmark = pytest.mark.gpu

NORM_RTOL = (97 / 2 + 2.01) * 2.0 ** -24
CASES = {  # the four CnnUpdateModes
    "sgd": ("sgd", dict(lr=0.05)),
    "sgd_mom_wd": ("sgd", dict(lr=0.05, momentum=0.9, weight_decay=1e-2)),
    "adam": ("adam", dict(lr=0.01, weight_decay=1e-2)),
    "adamw": ("adamw", dict(lr=0.01, weight_decay=1e-2)),
}
FACTORS = (0.5, 2.0, 0.5)  # max_grad_norm / the step's norm: two steps clip, one does not


def net_and_batches(gpu, B, steps=3):
    from pytorch_distributed_examples_amd.models.cnn import Net

    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(11 + B)
    return Net().to(gpu).eval(), [(torch.randn(B, 1, 28, 28, generator=gen).to(gpu),
                                   torch.randint(0, 10, (B,), generator=gen).to(gpu)) for _ in range(steps)]


def cat(ts):
    return torch.cat([t.detach().reshape(-1).cpu().double() for t in ts])


@pytest.mark.parametrize("B", [6, 130])
@pytest.mark.parametrize("case", list(CASES))
def test_clipped_opt_step_follows_float64(gpu, case, B):
    from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN

    kind, hyper = CASES[case]
    net, data = net_and_batches(gpu, B)
    f = FusedCNN(net)
    g = f.grad_buffer()
    params = list(net.parameters())
    opt = fused(kind)(params, **hyper, max_grad_norm=1.0)
    p32 = [p.detach().cpu().clone().requires_grad_() for p in params]
    o32 = fused(kind)(p32, **hyper, max_grad_norm=1.0)
    p64, s64 = [p.detach().cpu().double() for p in params], [{} for _ in params]
    worst = 0.0
    for t, ((x, y), fac) in enumerate(zip(data, FACTORS), 1):
        f.forward_backward(x, y, grad_out=g)
        flat = g.detach().cpu().clone()
        total = float(flat.double().norm())
        coef = min(1.0, fac * total / (total + 1e-6))
        off = 0
        for q in p32:
            q.grad = flat[off:off + q.numel()].view_as(q).clone()
            off += q.numel()
        for o in (opt, o32):
            o.param_groups[0]["max_grad_norm"] = fac * total
        kb, b32, b64 = f.flat.detach().clone(), cat(p32), cat(p64)
        f.opt_step(opt, g)
        o32.step()
        p64 = [ref64(kind, o32.param_groups[0], p, q.grad.double() * coef, s, t) for p, q, s in zip(p64, p32, s64)]
        got = opt.last_grad_norm.tolist()
        frac = max(abs(got[0] - total) / (NORM_RTOL * total), abs(got[1] - coef) / ((NORM_RTOL + 2.0 ** -23) * coef))
        worst = max(worst, frac)
        assert frac <= 1.0 and (got[1] == 1.0) == (fac > 1), (got, total, coef)
        held(f"cnn clip {case} B{B} step{t} update", f.flat - kb, cat(p32) - b32, cat(p64) - b64, cat(p64))
        for key in s64[0]:
            want = cat([s[key] for s in s64])
            held(f"cnn clip {case} B{B} step{t} {key}", cat([opt.state[p][key] for p in params]),
                 cat([o32.state[q][key] for q in p32]), want, want)
        assert {k for k in opt.state[params[0]] if k != "step"} == set(s64[0])
    print(f"CNN_CLIP_NORM {case} B{B}: worst error {worst:.3f} of the tolerance {NORM_RTOL:.2e}")
    assert opt._dev[0]["step"].tolist() == [len(FACTORS), 0]
    # the fragment image the updates wrote is current: the same evaluation after a forced k_cnn_prep
    x, y = data[0]
    _, logp = f.evaluate(x, y, logprobs=True)
    f.invalidate()
    _, logp2 = f.evaluate(x, y, logprobs=True)
    assert torch.equal(logp, logp2)


def test_update_inside_the_reduction_refuses_a_clipping_optimiser(gpu):
    from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN

    net, data = net_and_batches(gpu, 6, 1)
    f = FusedCNN(net)
    with pytest.raises(ValueError, match="max_grad_norm"):
        f.forward_backward(*data[0], opt=fused("sgd")(net.parameters(), lr=0.05, max_grad_norm=1.0))


def test_hvd_step_routes_a_clipping_sgd_to_opt_step_at_world_1(gpu):
    """FusedHvdStep at world 1 with a clipping FusedSGD: route ``opt_step`` (three launches), and over three steps
    the bits of the eager composition forward_backward + opt_step."""
    from pytorch_distributed_examples_amd import hvd
    from pytorch_distributed_examples_amd.hvd.cnn_step import FusedHvdStep
    from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN

    hvd.init()
    net, data = net_and_batches(gpu, 130)
    ref, _ = net_and_batches(gpu, 130)
    hyper = dict(lr=0.05, momentum=0.9, max_grad_norm=1e-3)  # (far below the gradient norm of these batches)
    opt = hvd.DistributedOptimizer(fused("sgd")(net.parameters(), **hyper), named_parameters=net.named_parameters())
    step = FusedHvdStep(net, opt, 130, graph=False)
    assert step.route == "opt_step" and step.kernel_launches_per_step() == 3
    f, o = FusedCNN(ref), fused("sgd")(ref.parameters(), **hyper)
    g = f.grad_buffer()
    for x, y in data:
        la = step(x, y)
        lb = f.forward_backward(x, y, grad_out=g)
        f.opt_step(o, g)
        assert torch.equal(la, lb) and torch.equal(opt.last_grad_norm, o.last_grad_norm)
    assert torch.equal(step.fused.flat, f.flat) and (o.last_grad_norm[1] < 1).item()
