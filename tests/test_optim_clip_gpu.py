"""Global-norm gradient clipping (``max_grad_norm``, csrc/kernels/optim_clip.hip: k_grad_clip + the unchanged update
kernels on hp_eff) of all five fused optimisers, against float64.

Tensors: those of tests/test_optim_trust_gpu.py (1 .. three chunks, a 4-D tensor, a view at storage offset 1, a
zero-gradient tensor, a parameter without gradient) plus one of 70 * 4096 + 3 elements (71 chunks: the final sum's
lane stride wraps past 64 entries).  The ``stride`` case is one tensor of 769 chunks, one more than the grid cap, so
a block walks two chunks through the pipelined loop.

Exact regime: integer gradients with sum g^2 < 2^21 and a power-of-two grad_scale, so every fp32 partial sum is exact
in any order and the reported norm is one correctly rounded sqrtf (and one exact scaling) away from float64: 1 ulp.
Under sum g^2 = S < 2^21 one dropped or doubled element of magnitude 1 moves the norm by 1 / (2 sqrt S) = 2^22 / S
ulps of sqrt S, more than 2.

Random regime: the bound scheme of the optimiser tests (test_optim_trust_gpu.held), e32 being the error of the
class's own fp32 ``_cpu_step`` with clipping; the factor 4 is not widened.  Measured on an MI355X: the exact norms
are 0.09 ulp (0.23 ulp in the ``stride`` case) from float64, and the kernel used at most 0.33 of any L2 bound
(momentum_buffer, lars; updates at most 0.19).
"""
import math

import pytest
import torch
from test_optim_trust_gpu import FROZEN, SHAPES, VIEW, ZERO_G, held
from test_optim_trust_gpu import ref64 as trust_ref64

pytestmark = pytest.mark.gpu

ALL = SHAPES + [(70 * 4096 + 3,)]
KINDS = {
    "sgd": dict(lr=0.05, momentum=0.9, weight_decay=0.1),
    "adam": dict(lr=1e-2, weight_decay=0.1),
    "adamw": dict(lr=1e-2, weight_decay=0.1),
    "lamb": dict(lr=1e-2, weight_decay=0.1),
    "lars": dict(lr=1.0, momentum=0.9, weight_decay=0.1),
}


def fused(kind):
    from pytorch_distributed_examples_amd.ops import optim as O

    return {"sgd": O.FusedSGD, "adam": O.FusedAdam, "adamw": O.FusedAdamW, "lamb": O.FusedLAMB, "lars": O.FusedLARS}[kind]


def ref64(kind, h, p, g, st, t):
    """One tensor's float64 update on the (already clipped) gradient ``g``; returns the new p, updates ``st``."""
    if kind in ("lamb", "lars"):
        return trust_ref64(kind, h, p, g, st, t)
    g, lr, wd = g * h["grad_scale"], h["lr"], h["weight_decay"]
    if kind == "adamw":
        p = p * (1 - lr * wd)
    elif wd != 0:
        g = g + wd * p
    if kind == "sgd":
        if h["momentum"] != 0:
            st["momentum_buffer"] = g = g if t == 1 else h["momentum"] * st["momentum_buffer"] + g
        return p - lr * g
    b1, b2 = h["betas"]
    st["exp_avg"] = m = b1 * st.get("exp_avg", 0.0) + (1 - b1) * g
    st["exp_avg_sq"] = v = b2 * st.get("exp_avg_sq", 0.0) + (1 - b2) * g * g
    return p - lr / (1 - b1 ** t) * m / (v.sqrt() / math.sqrt(1 - b2 ** t) + h["eps"])


def leaves(dev, shapes=ALL, seed=7):
    """(GPU leaves, their values on the CPU); tensor VIEW sits at storage offset 1 (no 16-byte aligned pointer)."""
    gen = torch.Generator().manual_seed(seed)
    vals = [(0.25 * torch.randn(*s, generator=gen)).clamp_(-0.75, 0.75) for s in shapes]
    kp = [v.clone().to(dev) for v in vals]
    if len(shapes) > VIEW:
        kp[VIEW] = torch.zeros(shapes[VIEW][0] + 1, device=dev)[1:].copy_(vals[VIEW])
        assert kp[VIEW].data_ptr() % 16 != 0
    return [p.requires_grad_() for p in kp], vals


def set_grads(ps, gs, dev):
    for p, g in zip(ps, gs):
        p.grad = None if g is None else g.to(dev).clone()


def norm64(gs, scales):
    return math.sqrt(sum(float((g.double() * s).pow(2).sum()) for g, s in zip(gs, scales) if g is not None))


def ulps(x, want):
    w = torch.tensor(want, dtype=torch.float32)
    return abs(float(x) - want) / float(torch.nextafter(w, torch.tensor(float("inf"))) - w)


@pytest.mark.parametrize("kind", list(KINDS) + ["stride"])
def test_norm_is_exact_on_integer_gradients(gpu, kind):
    shapes = [(769 * 4096 + 5,)] if kind == "stride" else ALL
    kind = "sgd" if kind == "stride" else kind
    kp, _ = leaves(gpu, shapes)
    gen = torch.Generator().manual_seed(3)
    if len(shapes) == 1:  # one element in seven is +-1: S = 450,000
        gs = [torch.where(torch.arange(shapes[0][0]) % 7 == 0, 1.0, 0.0) * torch.randint(0, 2, shapes[0], generator=gen)
              .mul(2).sub(1)]
    else:
        gs = [torch.randint(-2, 3, s, generator=gen).float() for s in shapes]
        gs[ZERO_G].zero_()
        gs[FROZEN] = None
    s = sum(float(g.double().pow(2).sum()) for g in gs if g is not None)
    assert 0 < s < 2 ** 21, s  # the premise of the 1-ulp bound
    set_grads(kp, gs, gpu)
    opt = fused(kind)(kp, **KINDS[kind], grad_scale=0.25, max_grad_norm=1.0)
    opt.step()
    total, coef = opt.last_grad_norm.tolist()
    want = norm64(gs, [0.25] * len(gs))
    print(f"CLIP_EXACT {kind} n={len(shapes)}: S {s:.0f} norm {total!r} float64 {want!r} ({ulps(total, want):.2f} ulp)")
    assert ulps(total, want) <= 1.0
    assert ulps(coef, min(1.0, 1.0 / (want + 1e-6))) <= 3.0  # total, the sum and the quotient: one rounding each


def drive(kind, dev, factors=(0.5, 2.0, 0.5), compare=True):
    """Three steps, max_grad_norm = factor x the float64 norm of the step's gradients.  On the step that does not
    clip (coef == 1, hp_eff == hp) a twin without max_grad_norm, set to the same weights and state, must end on
    the same bits."""
    hyper = KINDS[kind]
    (kp, vals), (tw, _) = leaves(dev), leaves(dev)
    p32, p64 = [v.clone().requires_grad_() for v in vals], [v.double() for v in vals]
    opt, o32, twin = fused(kind)(kp, **hyper, max_grad_norm=1.0), fused(kind)(p32, **hyper, max_grad_norm=1.0), \
        fused(kind)(tw, **hyper)
    s64 = [{} for _ in p64]
    gen = torch.Generator().manual_seed(8)
    for t, f in enumerate(factors, 1):
        gs = [torch.where(torch.rand(*s, generator=gen) < 0.5, -1.0, 1.0) *
              (0.1 + torch.randn(*s, generator=gen).abs()) for s in ALL]
        gs[ZERO_G].zero_()
        gs[FROZEN] = None
        total = norm64(gs, [1.0] * len(gs))
        coef = min(1.0, f * total / (total + 1e-6))
        for o in (opt, o32):
            o.param_groups[0]["max_grad_norm"] = f * total
        for ps, d in ((kp, dev), (p32, "cpu"), (tw, dev)):
            set_grads(ps, gs, d)
        if f > 1:
            for a, b in zip(tw, kp):
                a.data.copy_(b.data)
                for k, v in opt.state[b].items():
                    if torch.is_tensor(v):
                        twin.state[a][k].copy_(v)
        kb, b32 = [p.detach().clone() for p in kp], [q.detach().clone() for q in p32]
        for o in (opt, o32, twin):
            o.step()
        got = opt.last_grad_norm.tolist()
        assert abs(got[0] - total) <= 1e-5 * total and (got[1] == 1.0 if f > 1 else abs(got[1] - coef) <= 1e-5)
        for i, g in enumerate(gs):
            if g is None:
                assert torch.equal(kp[i], kb[i]) and not opt.state[kp[i]]
                continue
            if f > 1:
                assert torch.equal(kp[i], tw[i]) and all(
                    torch.equal(v, twin.state[tw[i]][k]) for k, v in opt.state[kp[i]].items() if torch.is_tensor(v)), \
                    f"{kind} t{i}: the step that does not clip differs from the optimiser without max_grad_norm"
            new = ref64(kind, o32.param_groups[0], p64[i], g.double() * coef, s64[i], t)
            if compare:
                held(f"clip {kind} step{t} t{i} update", kp[i] - kb[i], p32[i] - b32[i], new - p64[i], new)
                for key, want in s64[i].items():
                    held(f"clip {kind} step{t} t{i} {key}", opt.state[kp[i]][key], o32.state[p32[i]][key], want, want)
            p64[i] = new
    assert opt._dev[0]["step"].tolist() == [len(factors), 0]
    return kp, opt


@pytest.mark.parametrize("kind", list(KINDS))
def test_clipped_updates_and_state_follow_float64(gpu, kind):
    drive(kind, gpu)


def test_two_param_groups_share_one_norm_and_coefficient(gpu):
    """grad_scale 1 and 0.25 (exact regime): one norm over both, one coefficient in both groups' hp_eff, and the
    plain-SGD update -lr coef gs g.  Five roundings separate it from float64 (the total, the sum with 1e-6, the
    quotient, gs x coef, g x that; the fmaf is the ulp of p_after): (1 + 2^-24)^5 - 1 < 5.5 x 2^-24 relative."""
    kp, _ = leaves(gpu, [(4097,), (70 * 4096 + 3,), (5,)])
    gen = torch.Generator().manual_seed(4)
    gs = [torch.randint(-2, 3, p.shape, generator=gen).float() for p in kp]
    set_grads(kp, gs, gpu)
    scales, lr = [1.0, 0.25, 0.25], 0.5
    opt = fused("sgd")([dict(params=kp[:1]), dict(params=kp[1:], grad_scale=0.25)], lr=lr, max_grad_norm=8.0)
    before = [p.detach().clone() for p in kp]
    opt.step()
    total, coef = opt.last_grad_norm.tolist()
    want = norm64(gs, scales)
    assert want > 8.0 and ulps(total, want) <= 1.0 and ulps(coef, 8.0 / (want + 1e-6)) <= 3.0
    eff = [opt._hp_eff(opt._clip, slot)[6].item() for slot in range(2)]  # HP_GRAD_SCALE
    assert eff == [coef, torch.tensor(0.25 * coef, dtype=torch.float32).item()]
    for p, b, g, s in zip(kp, before, gs, scales):
        d64 = -lr * (8.0 / (want + 1e-6)) * s * g.double()
        a = p.detach().cpu().abs()
        ulp = (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()
        assert ((p.detach() - b).cpu().double() - d64).abs().le(5.5 * 2.0 ** -24 * d64.abs() + ulp).all()


@pytest.mark.parametrize("kind", ["sgd", "lamb"])
def test_graph_replays_equal_eager_steps(gpu, kind):
    """step() captured once, replayed three times on fresh gradients (the ticket is left 0 by every launch), then
    max_grad_norm changed + sync_hyper_to_device() and one more replay: four eager steps, bit for bit."""
    gen = torch.Generator().manual_seed(9)
    gs = [[torch.randn(*s, generator=gen) for s in ALL] for _ in range(4)]
    live = [i for i in range(len(ALL)) if i != FROZEN]
    runs = []
    for graph in (False, True):
        kp, _ = leaves(gpu)
        for i in live:
            kp[i].grad = torch.zeros_like(kp[i])
        opt = fused(kind)(kp, **KINDS[kind], max_grad_norm=40.0)
        if graph:  # tables, state and the clip workspace exist before the capture
            st = opt._group_dev(0, opt.param_groups[0], [kp[i] for i in live])
            opt._clip_dev(gpu, st["nchunks"])
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                opt.step()
        norms = []
        for t in range(4):
            for i in live:
                kp[i].grad.copy_(gs[t][i])
            if t == 3:
                opt.param_groups[0]["max_grad_norm"] = 1000.0
                opt.sync_hyper_to_device()
            g.replay() if graph else opt.step()
            norms.append(opt.last_grad_norm.clone())
        torch.cuda.synchronize()
        runs.append((kp, torch.stack(norms)))
    (ea, na), (gr, nb) = runs
    assert torch.equal(na, nb) and (na[:3, 1] < 1).all() and na[3, 1] == 1, (na, nb)
    assert all(torch.equal(a, b) for a, b in zip(ea, gr))

