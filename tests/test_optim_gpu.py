"""The fused multi-tensor optimiser kernel (csrc/kernels/optim_device.h, optim.hip) against a float64 reference,
update by update.

What is compared, after every step: the update ``p_after - p_before`` (both sides in float64) and every state
tensor, as a relative L2 error against :class:`Ref64` and per element.

Where the tolerance comes from.  Next to the float64 reference the same inputs go through an fp32 optimiser on
the CPU: ``torch.optim``'s own, or the fused optimisers' ``_cpu_step`` (torch's operation sequence) where
``torch.optim`` has no such option (``grad_scale``).  With e32 = that run's error against float64:

    L2           |k - r64|_2   <= 4 |e32|_2            + |ulp|_2
    per element  |k - r64|_i   <= 4 max_j(|e32|/|r64|)_j |r64|_i + ulp_i

``ulp`` is one fp32 ulp of the parameter (for the update: p_after is rounded to fp32 whatever the update's own
error) or of the state value itself.  The factor 4 covers what the kernel legitimately does differently
(operation order, FMA contraction, ``rsqrtf``, ``expm1f`` / ``log1pf`` in the bias correction); a wrong formula
is off by orders of magnitude more.  No bound is taken from the kernel's output.

Conditioning.  |p| <= 0.75, |g| >= 0.1 with one sign per element over the steps, so that no update or momentum
cancels to nothing and the rounding of p_after (<= 4.5e-8) stays far below the smallest update: the fp32
reference's per-element update error is asserted to stay under 1e-4 relative, and no element is excluded.

Measured on an MI355X (worst step of each case, aligned tensors and unaligned views together; relative L2
error against float64 of kernel | fp32 reference | the bound the kernel is held to).  The update's error is
the rounding of p_after in both runs; ``-lr``: lr halved after step 2; ``-late``: steps 999 and 1000:

  case             update                        momentum_buffer / exp_avg        exp_avg_sq
  sgd              1.5e-07 | 1.5e-07 | 1.1e-06
  sgd-wd           1.3e-07 | 1.3e-07 | 9.6e-07
  sgd-mom          1.0e-07 | 1.1e-07 | 7.3e-07   6.1e-08 | 6.7e-08 | 3.6e-07
  sgd-mom-wd       1.0e-07 | 1.1e-07 | 7.4e-07   6.2e-08 | 6.8e-08 | 3.6e-07
  adam             7.5e-07 | 7.5e-07 | 5.6e-06   5.0e-08 | 3.9e-08 | 2.4e-07      8.6e-08 | 9.0e-08 | 4.5e-07
  adam-wd          7.5e-07 | 7.5e-07 | 5.6e-06   5.1e-08 | 4.2e-08 | 2.5e-07      8.4e-08 | 8.5e-08 | 4.3e-07
  adamw-wd0        7.5e-07 | 7.5e-07 | 5.6e-06   5.0e-08 | 3.9e-08 | 2.4e-07      8.6e-08 | 9.0e-08 | 4.5e-07
  adamw            1.1e-06 | 1.1e-06 | 6.8e-06   5.0e-08 | 3.9e-08 | 2.4e-07      8.6e-08 | 9.0e-08 | 4.5e-07
  adam-betas-eps   7.5e-07 | 7.5e-07 | 5.6e-06   5.4e-08 | 3.5e-08 | 2.3e-07      4.2e-08 | 4.2e-08 | 2.5e-07
  adamw-betas-eps  1.1e-06 | 1.1e-06 | 7.1e-06   5.4e-08 | 3.5e-08 | 2.3e-07      4.2e-08 | 4.2e-08 | 2.5e-07
  sgd-mom-gscale   1.0e-07 | 1.1e-07 | 7.4e-07   6.2e-08 | 6.8e-08 | 3.6e-07
  adam-gscale      7.5e-07 | 7.5e-07 | 5.6e-06   5.1e-08 | 4.2e-08 | 2.5e-07      8.4e-08 | 8.5e-08 | 4.3e-07
  sgd-mom-wd-lr    8.4e-08 | 8.6e-08 | 6.1e-07   5.3e-08 | 5.9e-08 | 3.2e-07
  adam-wd-lr       1.4e-06 | 1.4e-06 | 1.1e-05   4.4e-08 | 4.0e-08 | 2.5e-07      8.4e-08 | 8.5e-08 | 4.3e-07
  adamw-lr         2.4e-06 | 2.4e-06 | 1.5e-05   4.2e-08 | 3.8e-08 | 2.4e-07      8.0e-08 | 8.3e-08 | 4.2e-07
  adam-late        2.8e-07 | 2.8e-07 | 2.0e-06   3.9e-08 | 3.9e-08 | 2.4e-07      7.9e-08 | 7.9e-08 | 4.0e-07
  adamw-late       3.9e-07 | 3.9e-07 | 2.4e-06   3.0e-08 | 3.0e-08 | 2.1e-07      6.7e-08 | 6.6e-08 | 3.5e-07

Before the bias correction and the (1 - beta) factors were made accurate (HP_OMB1 / HP_OMB2, bias_correction()
in optim_device.h) the kernel's fp32 ``1.f - 0.999f`` put exp_avg_sq 1.3e-5 off at every step (30x this bound),
exp_avg 2.4e-7, and the step-999 update 3e-6: the arithmetic of that kernel, replayed in fp32 on the CPU.
"""
import copy
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

# chunk = 4096 elements; a thread owns 4 groups of 4 elements; 256 threads x 4 = 1024
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 2 * 4096 + 2]
SHAPE4D = (7, 3, 5, 5)
KEYS = {"sgd": ("momentum_buffer",), "adam": ("exp_avg", "exp_avg_sq"), "adamw": ("exp_avg", "exp_avg_sq")}
TORCH = {"sgd": torch.optim.SGD, "adam": torch.optim.Adam, "adamw": torch.optim.AdamW}


def _fused(kind):
    from pytorch_distributed_examples_amd.ops import optim as O

    return {"sgd": O.FusedSGD, "adam": O.FusedAdam, "adamw": O.FusedAdamW}[kind]


# ---------------------------------------------------------------------------------------------------------------
# float64 reference (torch.optim semantics)
# ---------------------------------------------------------------------------------------------------------------
class Ref64:
    """SGD (momentum, L2), Adam (L2) and AdamW in float64 over the same fp32 parameters and gradients."""

    def __init__(self, kind, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, momentum=0.0,
                 grad_scale=1.0, step=0):
        self.kind, self.lr, self.betas, self.eps = kind, lr, betas, eps
        self.wd, self.mom, self.gs, self.t = weight_decay, momentum, grad_scale, step
        self.p = [p.detach().cpu().double().clone() for p in params]
        self.state = [{} for _ in params]

    def step(self, grads):
        self.t += 1
        b1, b2 = self.betas
        for i, g in enumerate(grads):
            if g is None:
                continue
            p, st = self.p[i], self.state[i]
            g = g.detach().cpu().double() * self.gs
            if self.kind == "sgd":
                if self.wd != 0:
                    g = g + self.wd * p
                if self.mom != 0:
                    buf = st.get("momentum_buffer")
                    st["momentum_buffer"] = g.clone() if buf is None else self.mom * buf + g
                    g = st["momentum_buffer"]
                p -= self.lr * g
                continue
            if self.kind == "adamw":
                p *= 1.0 - self.lr * self.wd
            elif self.wd != 0:
                g = g + self.wd * p
            m = st.get("exp_avg", torch.zeros_like(p))
            v = st.get("exp_avg_sq", torch.zeros_like(p))
            st["exp_avg"] = m = b1 * m + (1.0 - b1) * g
            st["exp_avg_sq"] = v = b2 * v + (1.0 - b2) * g * g
            bc1, bc2 = 1.0 - b1 ** self.t, 1.0 - b2 ** self.t
            p -= (self.lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + self.eps)


def ulp32(x64):
    """One fp32 ulp at each value of a float64 tensor."""
    a = x64.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def cat(ts):
    return torch.cat([t.detach().cpu().double().reshape(-1) for t in ts])


def check(tag, what, k, r32, r64, ulp, conditioned=False):
    """Hold the kernel's ``k`` to the bound derived from the fp32 reference ``r32`` (module docstring); all
    float64 vectors.  Prints the measured figures before it asserts."""
    assert torch.isfinite(k).all() and r64.abs().min().item() > 0
    ek, e32 = (k - r64).abs(), (r32 - r64).abs()
    n64 = r64.norm().item()
    l2k, l232 = ek.norm().item() / n64, e32.norm().item() / n64
    l2_bound = 4 * l232 + ulp.norm().item() / n64
    rel32 = (e32 / r64.abs()).max().item()
    relk = (ek / r64.abs()).max().item()
    print(f"OPTIM_ERR {tag} {what}: l2 kernel {l2k:.2e} fp32 {l232:.2e} bound {l2_bound:.2e} | "
          f"max-rel kernel {relk:.2e} fp32 {rel32:.2e}")
    if conditioned:
        assert rel32 < 1e-4, f"{tag} {what}: fp32 reference itself is off by {rel32:.2e} on one element"
    assert l2k <= l2_bound, f"{tag} {what}: relative L2 error {l2k:.3e} > {l2_bound:.3e} (fp32 ref {l232:.3e})"
    worst = (ek - (4 * rel32 * r64.abs() + ulp)).max().item()
    assert worst <= 0, f"{tag} {what}: an element is {worst:.3e} past its bound (max rel {relk:.3e}, fp32 {rel32:.3e})"


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def tensor_values(seed, shapes):
    """(parameter values, per-element gradient signs) on the CPU; |p| <= 0.75."""
    gen = torch.Generator().manual_seed(seed)
    ps = [(0.25 * torch.randn(*s, generator=gen)).clamp_(-0.75, 0.75) for s in shapes]
    sg = [torch.where(torch.rand(*s, generator=gen) < 0.5, -1.0, 1.0) for s in shapes]
    return ps, sg


def draw_grads(gen, signs):
    return [s * (0.1 + torch.randn(s.shape, generator=gen).abs()) for s in signs]


def leaf(v, dev):
    return v.detach().clone().to(dev).requires_grad_()


def edge_tensor_set(dev, seed=21):
    """The sizes on the kernel's edges, twice with the SAME values: as tensors of their own (16-byte aligned,
    vector path) and as views of one flat buffer at offsets that are no multiple of 4 elements (scalar path).
    Returns (device leaves, CPU values, gradient signs, number of aligned tensors)."""
    shapes = [(n,) for n in SIZES] + [SHAPE4D]
    vals, signs = tensor_values(seed, shapes)
    aligned = [leaf(v, dev) for v in vals]
    flat = torch.zeros(sum(v.numel() for v in vals) + 4 * len(vals) + 1, device=dev)
    views, off = [], 1
    for v in vals:
        if off % 4 == 0:
            off += 1
        w = flat[off:off + v.numel()].view(v.shape)
        w.copy_(v)
        assert w.data_ptr() % 16 != 0
        views.append(w.requires_grad_())
        off += v.numel()
    return aligned + views, vals + vals, signs + signs, len(vals)


def set_grads(ps, gs, dev):
    for p, g in zip(ps, gs):
        p.grad = None if g is None else g.to(dev)


def make_ref32(kind, params, hyper):
    """The fp32 reference run on the CPU: torch.optim, or the fused optimiser's CPU path for grad_scale."""
    ps = [p.detach().cpu().clone().requires_grad_() for p in params]
    if hyper.get("grad_scale", 1.0) != 1.0:
        return ps, _fused(kind)(ps, **hyper)
    return ps, TORCH[kind](ps, **hyper)


def states(opt, ps, key):
    return cat([opt.state[p][key] for p in ps])


class Trio:
    """One parameter group driven three ways: the kernel (fused, GPU), fp32 on the CPU, float64."""

    def __init__(self, kind, gpu_params, cpu_values, hyper, opt=None, group=None, step=0):
        self.kind, self.kp = kind, gpu_params
        self.opt = opt if opt is not None else _fused(kind)(gpu_params, **hyper)
        self.group = group if group is not None else self.opt.param_groups[0]
        self.p32, self.o32 = make_ref32(kind, cpu_values, hyper)
        self.r64 = Ref64(kind, cpu_values, step=step, **hyper)
        self.before = None

    def give(self, grads, dev):
        set_grads(self.kp, grads, dev)
        set_grads(self.p32, grads, "cpu")
        self.before = tuple([t.detach().cpu().double().clone() for t in ts] for ts in (self.kp, self.p32, self.r64.p))
        self.grads = grads

    def step_refs(self):
        self.o32.step()
        self.r64.step(self.grads)

    def compare(self, tag, parts):
        """``parts``: name -> index list (aligned tensors / unaligned views): each is held to the bound alone."""
        for name, idx in parts.items():
            def sel(ts):
                return cat([ts[i] for i in idx])

            kb, b32, b64 = (sel(b) for b in self.before)
            p64 = sel(self.r64.p)
            check(f"{tag} {name}", "update", sel(self.kp) - kb, sel(self.p32) - b32, p64 - b64, ulp32(p64),
                  conditioned=True)
            for key in KEYS[self.kind]:
                if key == "momentum_buffer" and self.r64.mom == 0:  # use_m == false: no state tensor at all
                    assert all(key not in self.opt.state[self.kp[i]] for i in idx)
                    continue
                s64 = sel([s.get(key) for s in self.r64.state])
                check(f"{tag} {name}", key, sel([self.opt.state[p].get(key) for p in self.kp]),
                      sel([self.o32.state[p].get(key) for p in self.p32]), s64, ulp32(s64))


def drive(tag, kind, hyper, dev, steps=5, after_step=None, seed=21):
    """``steps`` steps of one group over the edge tensor set with every comparison; ``after_step(trio, i)`` may
    change hyper-parameters between steps.  Returns the trio."""
    kp, vals, signs, na = edge_tensor_set(dev, seed)
    trio = Trio(kind, kp, vals, hyper)
    parts = {"aligned": list(range(na)), "views": list(range(na, 2 * na))}
    gen = torch.Generator().manual_seed(seed + 1)
    unscale = 1.0 / hyper.get("grad_scale", 1.0)  # (a power of two: the scaled gradient keeps |g| >= 0.1)
    for i in range(1, steps + 1):
        g = [x * unscale for x in draw_grads(gen, signs[:na])]
        trio.give(g + g, dev)
        trio.opt.step()
        trio.step_refs()
        trio.compare(f"{tag} step{i}", parts)
        # the scalar path (unaligned views) is the same arithmetic as the vector path
        for a, b in zip(kp[:na], kp[na:]):
            assert torch.equal(a.detach(), b.detach()), f"{tag} step {i}: vec and non-vec paths differ, n={a.numel()}"
        if after_step is not None:
            after_step(trio, i)
    assert int(trio.opt._dev[0]["step"][0].item()) == steps and int(trio.opt._dev[0]["step"][1].item()) == 0
    return trio


CASES = {
    "sgd": ("sgd", dict(lr=0.05)),
    "sgd-wd": ("sgd", dict(lr=0.05, weight_decay=0.1)),
    "sgd-mom": ("sgd", dict(lr=0.05, momentum=0.9)),
    "sgd-mom-wd": ("sgd", dict(lr=0.05, momentum=0.9, weight_decay=0.1)),
    "adam": ("adam", dict(lr=1e-2)),
    "adam-wd": ("adam", dict(lr=1e-2, weight_decay=0.1)),
    "adamw-wd0": ("adamw", dict(lr=1e-2, weight_decay=0.0)),
    "adamw": ("adamw", dict(lr=1e-2, weight_decay=0.1)),
    "adam-betas-eps": ("adam", dict(lr=1e-2, betas=(0.8, 0.95), eps=1e-3)),
    "adamw-betas-eps": ("adamw", dict(lr=1e-2, betas=(0.8, 0.95), eps=1e-3, weight_decay=0.1)),
    "sgd-mom-gscale": ("sgd", dict(lr=0.05, momentum=0.9, weight_decay=0.1, grad_scale=0.125)),
    "adam-gscale": ("adam", dict(lr=1e-2, weight_decay=0.1, grad_scale=0.125)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_updates_and_state_follow_float64(gpu, case):
    kind, hyper = CASES[case]
    drive(case, kind, hyper, gpu)


@pytest.mark.parametrize("case", ["sgd-mom-wd", "adam-wd", "adamw"])
def test_lr_change_between_steps(gpu, case):
    """``group["lr"]`` halved after step 2 (the hp_key re-upload): steps 3 and 4 follow the reference at the new
    rate."""
    kind, hyper = CASES[case]

    def halve(trio, i):
        if i == 2:
            trio.group["lr"] *= 0.5
            trio.o32.param_groups[0]["lr"] *= 0.5
            trio.r64.lr *= 0.5

    trio = drive(case + "-lr", kind, hyper, gpu, steps=4, after_step=halve)
    assert trio.group["lr"] == hyper["lr"] * 0.5


@pytest.mark.parametrize("kind", ["adam", "adamw"])
def test_bias_correction_at_step_1000(gpu, kind):
    """Steps 999 and 1000 without taking 998 steps: a state dict with ``step`` = 998 is loaded, which seeds the
    device step counter; the references' counters are set to match."""
    hyper = CASES[kind][1] if kind == "adamw" else CASES["adam-wd"][1]
    kp, vals, signs, na = edge_tensor_set(gpu, seed=31)
    trio = Trio(kind, kp, vals, hyper, step=998)
    gen = torch.Generator().manual_seed(32)
    # one throw-away step gives every optimiser its state tensors; then parameters and state are put back
    g = draw_grads(gen, signs[:na])
    trio.give(g + g, gpu)
    trio.opt.step()
    trio.o32.step()
    sd = copy.deepcopy(trio.opt.state_dict())
    for s in sd["state"].values():
        s["step"] = 998
        s["exp_avg"].zero_()
        s["exp_avg_sq"].zero_()
    trio.opt.load_state_dict(sd)
    with torch.no_grad():
        for p, q, v in zip(trio.kp, trio.p32, vals):
            p.copy_(v)
            q.copy_(v)
            st = trio.o32.state[q]
            st["step"] = torch.tensor(998.0)
            st["exp_avg"].zero_()
            st["exp_avg_sq"].zero_()
    parts = {"aligned": list(range(na)), "views": list(range(na, 2 * na))}
    for i in (999, 1000):
        g = draw_grads(gen, signs[:na])
        trio.give(g + g, gpu)
        trio.opt.step()
        trio.step_refs()
        trio.compare(f"{kind}-late step{i}", parts)
    assert int(trio.opt._dev[0]["step"][0].item()) == 1000 and trio.r64.t == 1000
    assert int(trio.o32.state[trio.p32[0]]["step"]) == 1000
    assert trio.opt.state_dict()["state"][0]["step"] == 1000


@pytest.mark.parametrize("kind", ["sgd", "adam", "adamw"])
def test_two_param_groups(gpu, kind):
    """Two groups with their own lr and weight decay: each follows its own reference and its own device counter."""
    shapes = [(4097,), (5,), (1025,)]
    hypers = [dict(lr=0.05, weight_decay=0.1), dict(lr=0.0125, weight_decay=0.0)]
    if kind == "sgd":
        hypers = [dict(h, momentum=0.9) for h in hypers]
    sets = [tensor_values(41 + gi, shapes) for gi in range(2)]
    kps = [[leaf(v, gpu) for v in vals] for vals, _ in sets]
    opt = _fused(kind)([dict(params=kps[gi], lr=hypers[gi]["lr"], weight_decay=hypers[gi]["weight_decay"])
                        for gi in range(2)], **{k: v for k, v in hypers[0].items() if k == "momentum"}, lr=1.0)
    trios = [Trio(kind, kps[gi], sets[gi][0], hypers[gi], opt=opt, group=opt.param_groups[gi]) for gi in range(2)]
    gen = torch.Generator().manual_seed(43)
    for i in range(1, 4):
        for gi, t in enumerate(trios):
            t.give(draw_grads(gen, sets[gi][1]), gpu)
        opt.step()
        for gi, t in enumerate(trios):
            t.step_refs()
            t.compare(f"{kind}-group{gi} step{i}", {"all": list(range(len(shapes)))})
        for gi in range(2):
            assert int(opt._dev[gi]["step"][0].item()) == i and int(opt._dev[gi]["step"][1].item()) == 0


@pytest.mark.parametrize("kind", ["sgd", "adam", "adamw"])
def test_param_without_grad_is_untouched(gpu, kind):
    """``.grad is None``: not a bit of the parameter changes, weight decay or not; its neighbours still follow
    the reference."""
    shapes = [(4097,), (1025,), (5,), (4096,)]
    hyper = dict(lr=0.05, weight_decay=0.1, **({"momentum": 0.9} if kind == "sgd" else {}))
    vals, signs = tensor_values(51, shapes)
    kp = [leaf(v, gpu) for v in vals]
    trio = Trio(kind, kp, vals, hyper)
    gen = torch.Generator().manual_seed(52)
    frozen = (1, 2)
    for i in range(1, 4):
        g = draw_grads(gen, signs)
        for j in frozen:
            g[j] = None
        trio.give(g, gpu)
        trio.opt.step()
        trio.step_refs()
        trio.compare(f"{kind}-nograd step{i}", {"live": [0, 3]})
        for j in frozen:
            assert torch.equal(kp[j].detach().cpu(), vals[j]), f"step {i}: parameter {j} without a gradient changed"
            assert not trio.opt.state[kp[j]], "state was created for a parameter that never had a gradient"


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_maintained_bf16_copy_is_the_rounded_weight(gpu, kind):
    """The bf16 compute copy the update launch writes next to a linear weight equals ``w.bfloat16()`` bit for bit
    after every step (4097 elements: a full chunk and a one-element tail; 5: one partial group)."""
    from pytorch_distributed_examples_amd.ops import functional as OF
    from pytorch_distributed_examples_amd.ops import layers as L

    torch.manual_seed(61)
    fcs = [L.Linear(4097, 1).to(gpu), L.Linear(5, 1).to(gpu), L.Linear(5, 8).to(gpu)]
    params = [p for fc in fcs for p in fc.parameters()]
    opt = _fused(kind)(params, lr=0.05, **({"momentum": 0.9} if kind == "sgd" else {}))
    for _ in range(3):
        for p in params:
            p.grad = torch.randn_like(p)
        opt.step()
        for fc in fcs:
            copy_ = OF._maintained(fc.weight, "bf16")
            assert copy_ is not None and copy_.shape == fc.weight.shape
            assert torch.equal(copy_, fc.weight.detach().bfloat16())


# ---------------------------------------------------------------------------------------------------------------
# the pipelined chunk loop and the non-temporal / write-through accesses, in child processes
# ---------------------------------------------------------------------------------------------------------------
PIPE_SHAPES = [(2 * 4096 + 2,), (4097,), (4096,), (5,)]  # 3 + 2 + 1 + 1 = 7 chunks
PIPE_CASES = [("sgd", dict(lr=0.05, momentum=0.9, weight_decay=0.1)), ("adam", dict(lr=1e-2, weight_decay=0.1))]

_CHILD = r"""
import sys
import torch
from pytorch_distributed_examples_amd.ops import optim as O
blob = torch.load(sys.argv[1])
make = {"sgd": O.FusedSGD, "adam": O.FusedAdam}
for case in blob:
    ps = [v.cuda().requires_grad_() for v in case["params"]]
    opt = make[case["kind"]](ps, **case["hyper"])
    for gs in case["grads"]:
        for p, g in zip(ps, gs):
            p.grad = g.cuda()
        opt.step()
    torch.cuda.synchronize()
    for i, p in enumerate(ps):
        assert torch.equal(p.detach().cpu(), case["want"][i]), (case["kind"], "param", i)
        for key, want in case["state"][i].items():
            assert torch.equal(opt.state[p][key].cpu(), want), (case["kind"], key, i)
    assert int(opt._dev[0]["step"][0].item()) == len(case["grads"])
print("OPTIM_PIPE_OK")
"""


def test_pipelined_loop_and_nt_modes_subprocess(gpu, tmp_path):
    """PDE_OPTIM_BLOCKS=2 makes each block walk 3-4 chunks (``cur = nxt`` in run_chunks), PDE_OPTIM_NT = 0 / 1 / 2
    selects plain / non-temporal / write-through state accesses; both are read once per process.  Same
    arithmetic, so the children must reproduce the parent's default-path results bit for bit."""
    blob = []
    for kind, hyper in PIPE_CASES:
        vals, signs = tensor_values(71, PIPE_SHAPES)
        gen = torch.Generator().manual_seed(72)
        grads = [draw_grads(gen, signs) for _ in range(3)]
        ps = [leaf(v, gpu) for v in vals]
        opt = _fused(kind)(ps, **hyper)
        for gs in grads:
            set_grads(ps, gs, gpu)
            opt.step()
        blob.append(dict(kind=kind, hyper=hyper, params=vals, grads=grads, want=[p.detach().cpu() for p in ps],
                         state=[{k: opt.state[p][k].cpu() for k in KEYS[kind]} for p in ps]))
    path = tmp_path / "optim_pipe.pt"
    torch.save(blob, path)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for nt in ("0", "1", "2"):
        env = dict(os.environ, PDE_OPTIM_BLOCKS="2", PDE_OPTIM_NT=nt)
        res = subprocess.run([sys.executable, "-c", _CHILD, str(path)], env=env, capture_output=True, text=True,
                             timeout=120, cwd=repo)
        assert res.returncode == 0 and "OPTIM_PIPE_OK" in res.stdout, f"PDE_OPTIM_NT={nt}: " + res.stderr[-3000:]
