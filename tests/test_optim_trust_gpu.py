"""FusedLAMB / FusedLARS (csrc/kernels/optim_trust.hip: k_trust_norms + k_trust_apply) against the float64 formulas,
update by update, in the scheme of tests/test_optim_gpu.py.

After every step the update ``p_after - p_before`` and every state tensor are compared per tensor.  The same inputs
go through the classes' fp32 ``_cpu_step``; with e32 its error against float64 the kernel is held to

    L2           |k - r64|_2 <= 4 |e32|_2 + |ulp|_2
    per element  |k - r64|_i <= 4 max_j(|e32| / |r64|)_j |r64|_i + ulp_i

(``ulp``: one fp32 ulp of p_after, or of the state value).  No bound is taken from the kernel's output and the
factor 4 was NOT widened by a summation-length term.  Tensors: below / at / above one thread group, exactly one chunk,
one chunk plus one, three chunks (one ratio for all of them), a 4-D tensor, a view at storage offset 1 (scalar path),
an all-zero tensor and a zero-gradient tensor (ratio 1), a parameter without gradient.  |p| <= 0.75, |g| >= 0.1, one
sign per element.  LR halved after step 2.

Measured on an MI355X (worst tensor and step of each case; relative L2 error against float64 of kernel | fp32
reference | the bound the kernel is held to).  The update's worst tensors are the 1- and 5-element ones, where the
rounding of p_after is largest against the update; ``-gscale`` rows equal their unscaled case (a power of two):

  case           update                        exp_avg / momentum_buffer     exp_avg_sq
  lamb           6.2e-06 | 6.2e-06 | 4.5e-05   4.9e-08 | 4.0e-08 | 2.6e-07   9.4e-08 | 9.4e-08 | 4.6e-07
  lamb-wd0       6.2e-06 | 6.2e-06 | 4.5e-05   4.9e-08 | 4.0e-08 | 2.6e-07   9.4e-08 | 9.4e-08 | 4.6e-07
  lars           2.8e-05 | 2.8e-05 | 2.0e-04   1.3e-07 | 1.8e-07 | 8.3e-07
  lars-wd        4.2e-05 | 4.2e-05 | 2.7e-04   1.3e-07 | 1.8e-07 | 8.0e-07
  lars-mom0-wd   6.4e-05 | 6.4e-05 | 4.3e-04

The kernel used at most 0.36 of any L2 bound (momentum_buffer, lars); the 8194-element tensor needed no widening.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (5,), (1023,), (4096,), (4097,), (2 * 4096 + 2,), (7, 3, 5, 5), (1025,), (1025,), (1025,), (9,)]
VIEW, ZERO_P, ZERO_G, FROZEN = 7, 8, 9, 10  # indices into SHAPES
CASES = {
    "lamb": ("lamb", dict(lr=1e-2, weight_decay=0.1)),
    "lamb-wd0": ("lamb", dict(lr=1e-2, weight_decay=0.0)),
    "lamb-gscale": ("lamb", dict(lr=1e-2, weight_decay=0.1, grad_scale=0.125)),
    "lars": ("lars", dict(lr=1.0, momentum=0.9)),
    "lars-wd": ("lars", dict(lr=1.0, momentum=0.9, weight_decay=0.1)),
    "lars-mom0-wd": ("lars", dict(lr=1.0, momentum=0.0, weight_decay=0.1)),
    "lars-gscale": ("lars", dict(lr=1.0, momentum=0.9, weight_decay=0.1, grad_scale=0.125)),
}


def fused(kind):
    from pytorch_distributed_examples_amd.ops import optim as O

    return {"lamb": O.FusedLAMB, "lars": O.FusedLARS}[kind]


def ref64(kind, h, p, g, st, t):
    """The issue's formulas in float64 on one tensor; returns the new p, updates ``st``."""
    g, wd, eps, pn = g * h["grad_scale"], h["weight_decay"], h["eps"], p.norm()
    if kind == "lamb":
        b1, b2 = h["betas"]
        st["exp_avg"] = m = b1 * st.get("exp_avg", 0.0) + (1 - b1) * g
        st["exp_avg_sq"] = v = b2 * st.get("exp_avg_sq", 0.0) + (1 - b2) * g * g
        u = (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt() + eps) + wd * p
        r = pn / u.norm() if pn > 0 and u.norm() > 0 else 1.0
        return p - h["lr"] * r * u
    gn = g.norm()
    r = h["trust_coefficient"] * pn / (gn + wd * pn + eps) if pn > 0 and gn > 0 else 1.0
    d = r * (g + wd * p)
    if h["momentum"] != 0:
        st["momentum_buffer"] = d = d if t == 1 else h["momentum"] * st["momentum_buffer"] + d
    return p - h["lr"] * d


def held(tag, k, r32, r64, at):
    """The module docstring's bound for one tensor; ``at``: the values whose fp32 ulp is granted."""
    k, r32, r64 = (x.detach().cpu().double().reshape(-1) for x in (k, r32, r64))
    a = at.detach().cpu().double().reshape(-1).abs().float()
    ulp = (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()
    ek, e32, nz = (k - r64).abs(), (r32 - r64).abs(), r64 != 0
    rel32 = (e32[nz] / r64[nz].abs()).max().item() if nz.any() else 0.0
    print(f"TRUST_ERR {tag}: l2 kernel {ek.norm().item():.2e} fp32 {e32.norm().item():.2e} "
          f"bound {4 * e32.norm().item() + ulp.norm().item():.2e} of {r64.norm().item():.2e}")
    assert torch.isfinite(k).all() and ek.norm() <= 4 * e32.norm() + ulp.norm(), tag
    worst = (ek - (4 * rel32 * r64.abs() + ulp)).max().item()
    assert worst <= 0, f"{tag}: an element is {worst:.3e} past its bound (fp32 max-rel {rel32:.2e})"


def inputs(dev, seed=7):
    """(GPU leaves, CPU fp32 leaves, float64 values, gradient signs)."""
    gen = torch.Generator().manual_seed(seed)
    vals = [(0.25 * torch.randn(*s, generator=gen)).clamp_(-0.75, 0.75) for s in SHAPES]
    vals[ZERO_P].zero_()
    signs = [torch.where(torch.rand(*s, generator=gen) < 0.5, -1.0, 1.0) for s in SHAPES]
    signs[ZERO_G].zero_()
    kp = [v.clone().to(dev) for v in vals]
    flat = torch.zeros(SHAPES[VIEW][0] + 1, device=dev)
    kp[VIEW] = flat[1:].copy_(vals[VIEW])  # storage offset 1: no pointer of it is 16-byte aligned
    assert kp[VIEW].data_ptr() % 16 != 0
    return ([p.requires_grad_() for p in kp], [v.clone().requires_grad_() for v in vals],
            [v.double() for v in vals], signs)


def grads_of(gen, signs, unscale):
    gs = [s * (0.1 + torch.randn(s.shape, generator=gen).abs()) * unscale for s in signs]
    gs[FROZEN] = None
    return gs


def drive(tag, kind, hyper, dev, compare=True, steps=3):
    kp, p32, p64, signs = inputs(dev)
    opt, o32 = fused(kind)(kp, **hyper), fused(kind)(p32, **hyper)
    s64 = [{} for _ in p64]
    gen = torch.Generator().manual_seed(8)
    for t in range(1, steps + 1):
        gs = grads_of(gen, signs, 1.0 / hyper.get("grad_scale", 1.0))  # (a power of two: |g'| >= 0.1 still)
        for p, q, g in zip(kp, p32, gs):
            p.grad, q.grad = (None, None) if g is None else (g.to(dev), g.clone())
        kb, b32 = [p.detach().clone() for p in kp], [q.detach().clone() for q in p32]
        opt.step()
        o32.step()
        for i, g in enumerate(gs):
            if g is None:
                assert torch.equal(kp[i], kb[i]) and not opt.state[kp[i]], "a parameter without gradient changed"
                continue
            new = ref64(kind, o32.param_groups[0], p64[i], g.double(), s64[i], t)
            if compare:
                held(f"{tag} step{t} t{i} update", kp[i] - kb[i], p32[i] - b32[i], new - p64[i], new)
                for key, want in s64[i].items():
                    held(f"{tag} step{t} t{i} {key}", opt.state[kp[i]][key], o32.state[p32[i]][key], want, want)
                assert set(opt.state[kp[i]]) - {"step"} == set(s64[i])
            p64[i] = new
        if t == 2:
            for o in (opt, o32):
                o.param_groups[0]["lr"] *= 0.5
    assert opt._dev[0]["step"].tolist() == [steps, 0] and opt.state_dict()["state"][0]["step"] == steps
    return kp, opt


@pytest.mark.parametrize("case", list(CASES))
def test_updates_and_state_follow_float64(gpu, case):
    drive(case, *CASES[case], gpu)


@pytest.mark.parametrize("case", ["lamb", "lars-wd"])
def test_equal_runs_give_equal_bits(gpu, case):
    (pa, oa), (pb, ob) = (drive(case, *CASES[case], gpu, compare=False) for _ in range(2))
    for a, b in zip(pa, pb):
        assert torch.equal(a, b) and all(torch.equal(oa.state[a][k], ob.state[b][k]) for k in oa.state[a]
                                         if k != "step")


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_maintained_bf16_copy_is_the_rounded_weight(gpu, kind):
    from pytorch_distributed_examples_amd.ops import functional as OF
    from pytorch_distributed_examples_amd.ops import layers as L

    torch.manual_seed(61)
    fcs = [L.Linear(4097, 1).to(gpu), L.Linear(5, 8).to(gpu)]
    params = [p for fc in fcs for p in fc.parameters()]
    opt = fused(kind)(params, lr=1.0 if kind == "lars" else 1e-2)
    for p in params:
        p.grad = torch.randn_like(p)
    opt.step()
    for fc in fcs:
        assert torch.equal(OF._maintained(fc.weight, "bf16"), fc.weight.detach().bfloat16())


@pytest.mark.parametrize("case", ["lamb", "lars-wd"])
def test_graph_replays_equal_eager_steps(gpu, case):
    """step() captured once and replayed 3 times, LR halved between replays 2 and 3: the weights of three eager
    steps bit for bit, and the device step counter read back by state_dict()."""
    kind, hyper = CASES[case]
    eager, _ = drive(case, kind, hyper, gpu, compare=False)
    kp, _, _, signs = inputs(gpu)
    gen = torch.Generator().manual_seed(8)
    gs = [grads_of(gen, signs, 1.0) for _ in range(3)]
    live = [i for i in range(len(kp)) if i != FROZEN]
    for i in live:
        kp[i].grad = torch.zeros_like(kp[i])
    opt = fused(kind)(kp, **hyper)
    opt._group_dev(0, opt.param_groups[0], [kp[i] for i in live])  # tables and state exist before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for t in range(3):
        for i in live:
            kp[i].grad.copy_(gs[t][i])
        if t == 2:
            opt.param_groups[0]["lr"] *= 0.5
            opt.sync_hyper_to_device()
        graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(kp, eager))
    assert opt.state_dict()["state"][0]["step"] == 3
