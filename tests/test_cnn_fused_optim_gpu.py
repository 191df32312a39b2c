"""Momentum SGD, L2 weight decay, Adam and AdamW inside the fused CNN's slab reduction (cnn_reduce_role<OPT>) and
in the one-launch update behind an all-reduce (k_cnn_opt<MODE>): against the generic route (forward_backward +
``opt.step()``, a fragment prep every step), against ``torch.optim``, and for step counting, state binding, the
fragment image and hipGraph replay.  Eval mode throughout (no dropout), so the routes can be compared.

Shapes: the update epilogue does not depend on the batch; B = 6 is two workgroups, the last one partial (fewer
slabs than reduce lanes), B = 130 is 33 workgroups, the last one partial (one more than RED_LANES)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = {
    "sgd_mom": ("sgd", dict(lr=0.05, momentum=0.9)),
    "sgd_wd": ("sgd", dict(lr=0.05, weight_decay=1e-2)),
    "sgd_mom_wd": ("sgd", dict(lr=0.05, momentum=0.9, weight_decay=1e-2)),
    "adam": ("adam", dict(lr=0.01, weight_decay=1e-2)),
    "adamw": ("adamw", dict(lr=0.01, weight_decay=1e-2)),
}
BATCHES = [6, 130]
STEPS = 5
# Adam / AdamW: the bounds of test_fused_cnn_adamw_step_matches_multi_tensor_adamw
W_TOL = dict(rtol=1e-5, atol=1e-6)
M_TOL = dict(rtol=1e-5, atol=1e-7)
V_TOL = dict(rtol=1e-5, atol=1e-9)
STATE_KEYS = {"sgd": ("momentum_buffer",), "adam": ("exp_avg", "exp_avg_sq"), "adamw": ("exp_avg", "exp_avg_sq")}


def _make_opt(case, params):
    from pytorch_distributed_examples_amd.ops.optim import FusedAdam, FusedAdamW, FusedSGD

    kind, kw = CASES[case]
    return {"sgd": FusedSGD, "adam": FusedAdam, "adamw": FusedAdamW}[kind](params, **kw)


def _torch_opt(case, params):
    kind, kw = CASES[case]
    return {"sgd": torch.optim.SGD, "adam": torch.optim.Adam, "adamw": torch.optim.AdamW}[kind](params, **kw)


def _net(gpu):
    from pytorch_distributed_examples_amd.models.cnn import Net

    torch.manual_seed(0)
    return Net().to(gpu).eval()


_DATA = {}


def _batches(gpu, B):
    if B not in _DATA:
        gen = torch.Generator().manual_seed(11 + B)
        _DATA[B] = [(torch.randn(B, 1, 28, 28, generator=gen).to(gpu), torch.randint(0, 10, (B,), generator=gen).to(gpu))
                    for _ in range(STEPS)]
    return _DATA[B]


def _state(opt):
    """{param index: {key: tensor}} of the optimiser's state tensors, plus the step counts."""
    sd = opt.state_dict()["state"]
    return {k: {n: (t.detach().clone() if torch.is_tensor(t) else t) for n, t in v.items()} for k, v in sd.items()}


_GENERIC = {}


def _generic(gpu, case, B):
    """The generic route, computed once per (case, B): forward_backward, then the multi-tensor ``opt.step()``, which
    bumps the weight generation, so every step preps the fragment image from the fp32 weights."""
    from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN

    if (case, B) not in _GENERIC:
        net = _net(gpu)
        f = FusedCNN(net)
        g = f.grad_buffer()
        opt = _make_opt(case, net.parameters())
        losses = []
        for x, y in _batches(gpu, B):
            losses.append(f.forward_backward(x, y, grad_out=g).item())
            opt.step()
        torch.cuda.synchronize()
        _GENERIC[(case, B)] = (losses, f.flat.detach().clone(), _state(opt))
    return _GENERIC[(case, B)]


def _fused_step(f, opt, g, x, y, route):
    if route == "reduce":
        return f.forward_backward(x, y, grad_out=g, sgd=opt)
    loss = f.forward_backward(x, y, grad_out=g)
    f.opt_step(opt, g)
    return loss


def _compare(case, ref, losses, flat, state, report):
    kind = CASES[case][0]
    r_losses, r_flat, r_state = ref
    keys = [k for k in STATE_KEYS[kind] if any(k in v for v in r_state.values())]
    assert len(state) == len(r_state) == 8
    if kind == "sgd":
        assert losses == r_losses, (losses, r_losses)
        assert torch.equal(flat, r_flat)
        for k in r_state:
            for key in keys:
                assert torch.equal(state[k][key], r_state[k][key]), (k, key)
    else:
        dw = (flat - r_flat).abs().max().item()
        dm = max((state[k]["exp_avg"] - r_state[k]["exp_avg"]).abs().max().item() for k in r_state)
        dv = max((state[k]["exp_avg_sq"] - r_state[k]["exp_avg_sq"]).abs().max().item() for k in r_state)
        print(f"{report}: max |dw| {dw:.3e}  max |d exp_avg| {dm:.3e}  max |d exp_avg_sq| {dv:.3e}")
        torch.testing.assert_close(flat, r_flat, **W_TOL)
        torch.testing.assert_close(torch.tensor(losses), torch.tensor(r_losses), rtol=1e-4, atol=1e-5)
        for k in r_state:
            torch.testing.assert_close(state[k]["exp_avg"], r_state[k]["exp_avg"], **M_TOL)
            torch.testing.assert_close(state[k]["exp_avg_sq"], r_state[k]["exp_avg_sq"], **V_TOL)
    for k in r_state:
        assert int(state[k]["step"]) == int(r_state[k]["step"]) == STEPS


def _run_route(gpu, case, B, route):
    """STEPS fused steps by ``route`` ("reduce": the update inside the slab reduction; "post": forward_backward, then
    the one-launch update), checked every step against an fp32 torch.optim step on the same weights and gradient, and
    at the end against the generic route."""
    from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN
    from pytorch_distributed_examples_amd.ops import functional as OF

    ref = _generic(gpu, case, B)  # first: its optimiser steps bump the (global) weight generation, which would
    net = _net(gpu)               # otherwise make the fused model re-prep and hide the fragment refresh under test
    f = FusedCNN(net)
    g = f.grad_buffer()
    opt = _make_opt(case, net.parameters())
    p_t = f.flat.detach().clone().requires_grad_(True)
    o_t = _torch_opt(case, [p_t])
    losses = []
    for i, (x, y) in enumerate(_batches(gpu, B)):
        if i > 0:
            assert f._frag_gen == OF.weight_generation()  # no prep launch: the update refreshed the fragments
        with torch.no_grad():
            p_t.copy_(f.flat)
        losses.append(_fused_step(f, opt, g, x, y, route).item())
        p_t.grad = g.detach().clone()
        o_t.step()
        torch.cuda.synchronize()
        # torch's unfused multiply-add differs from fmaf by rounding only
        torch.testing.assert_close(f.flat, p_t.detach(), **W_TOL)
    _compare(case, ref, losses, f.flat, _state(opt), f"{case} B={B} {route} vs generic")
    return f, opt


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("case", list(CASES))
def test_update_in_reduction_matches_generic_route_and_torch(gpu, case, B):
    """Tests 1 and 2 of the feature: the update inside cnn_reduce_role against forward_backward + opt.step() (SGD:
    losses, weights and momentum buffers bit for bit -- one update function; Adam / AdamW: the existing AdamW test's
    tolerances) and, every step, against torch.optim at rtol 1e-5 / atol 1e-6.  Measured on gfx950, Adam and AdamW,
    both batches: max |dw| 0, max |d exp_avg| 0, max |d exp_avg_sq| 0 against the generic route."""
    _run_route(gpu, case, B, "reduce")


@pytest.mark.parametrize("case", list(CASES))
def test_post_allreduce_update_matches_generic_route_and_torch(gpu, case):
    """opt_step (k_cnn_sgd / k_cnn_opt<MODE>): the update after an all-reduce that ran outside the reduction kernel,
    same two comparisons; sgd_step / adam_step / adamw_step reach the same launch and refuse the other optimisers."""
    from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN

    f, opt = _run_route(gpu, case, 6, "post")
    # the named entry points route to the same launch
    net = _net(gpu)
    f2 = FusedCNN(net)
    g2 = f2.grad_buffer()
    opt2 = _make_opt(case, net.parameters())
    named = {"sgd": f2.sgd_step, "adam": f2.adam_step, "adamw": f2.adamw_step}
    step = named.pop(CASES[case][0])
    before = f2.flat.detach().clone()
    for other in named.values():  # the other optimisers' entry points refuse this one before any launch
        with pytest.raises(AssertionError):
            other(opt2, g2)
    torch.cuda.synchronize()
    assert torch.equal(f2.flat, before) and getattr(f2, "_opt_m", None) is None
    for x, y in _batches(gpu, 6):
        f2.forward_backward(x, y, grad_out=g2)
        step(opt2, g2)
    torch.cuda.synchronize()
    assert torch.equal(f.flat, f2.flat)


@pytest.mark.parametrize("case", ["sgd_mom_wd", "adam", "adamw"])
def test_step_count_state_views_and_resume(gpu, case):
    """After n fused steps every state ``step`` is n and the arrival ticket is back at 0; the state tensors are views
    of the flat buffers; a state_dict taken after 3 steps and loaded into a fresh net + optimiser + FusedCNN (the
    optimiser loads before FusedCNN exists, as in the trainer) continues to the result of 5 uninterrupted steps."""
    from pytorch_distributed_examples_amd.models.cnn import Net
    from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN

    kind = CASES[case][0]
    data = _batches(gpu, 6)
    net = _net(gpu)
    f = FusedCNN(net)
    g = f.grad_buffer()
    opt = _make_opt(case, net.parameters())
    for n, (x, y) in enumerate(data[:3], 1):
        f.forward_backward(x, y, grad_out=g, sgd=opt)
        sd = opt.state_dict()
        assert all(int(s["step"]) == n for s in sd["state"].values())
        assert len(sd["state"]) == 8
    assert int(opt._dev[0]["step"][1].item()) == 0
    flats = {"momentum_buffer": f._opt_m, "exp_avg": f._opt_m, "exp_avg_sq": f._opt_v}
    off = 0
    for k, p in enumerate(f.params):
        for key in STATE_KEYS[kind]:
            t = sd["state"][k][key]
            assert t.data_ptr() == flats[key][off:].data_ptr() and t.shape == p.shape, (k, key)
        off += p.numel()
    saved = copy.deepcopy(sd)
    weights = copy.deepcopy(net.state_dict())
    # resume in fresh objects
    net2 = Net().to(gpu).eval()
    net2.load_state_dict(weights)
    opt2 = _make_opt(case, net2.parameters())
    opt2.load_state_dict(saved)
    f2 = FusedCNN(net2)
    g2 = f2.grad_buffer()
    for x, y in data[3:]:
        f.forward_backward(x, y, grad_out=g, sgd=opt)
    for x, y in data[3:]:
        f2.forward_backward(x, y, grad_out=g2, sgd=opt2)
    torch.cuda.synchronize()
    s1, s2 = _state(opt), _state(opt2)
    assert all(int(s["step"]) == STEPS for s in s2.values())
    if kind == "sgd":
        assert torch.equal(f.flat, f2.flat)
        for k in s1:
            assert torch.equal(s1[k]["momentum_buffer"], s2[k]["momentum_buffer"])
    else:
        torch.testing.assert_close(f.flat, f2.flat, **W_TOL)
        for k in s1:
            torch.testing.assert_close(s1[k]["exp_avg"], s2[k]["exp_avg"], **M_TOL)
            torch.testing.assert_close(s1[k]["exp_avg_sq"], s2[k]["exp_avg_sq"], **V_TOL)


@pytest.mark.parametrize("case", list(CASES))
def test_fragment_image_after_updates_in_reduction(gpu, case):
    """write_frag under the new modes (conv1 and both conv2 layouts): after in-reduction updates the fused forward,
    which reads the refreshed fragment image, equals exactly a fresh FusedCNN's over a copy of the weights, which
    preps its image from fp32."""
    from pytorch_distributed_examples_amd.models.cnn import Net
    from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN
    from pytorch_distributed_examples_amd.ops import functional as OF

    data = _batches(gpu, 130)
    net = _net(gpu)
    f = FusedCNN(net)
    g = f.grad_buffer()
    opt = _make_opt(case, net.parameters())
    before = f.flat.detach().clone()
    for x, y in data[:3]:
        f.forward_backward(x, y, grad_out=g, sgd=opt)
    assert f._frag_gen == OF.weight_generation()  # predict below runs on the image the updates wrote
    pred, logp = f.predict(data[3][0], logprobs=True)
    fresh = Net().to(gpu).eval()
    fresh.load_state_dict(copy.deepcopy(net.state_dict()))
    pred2, logp2 = FusedCNN(fresh).predict(data[3][0], logprobs=True)
    torch.cuda.synchronize()
    assert (f.flat - before).abs().max().item() > 1e-4  # the weights moved
    assert torch.equal(logp, logp2) and torch.equal(pred, pred2)


def test_momentum_step_replays_in_a_hipgraph(gpu):
    """One captured momentum step replayed four times on new batches equals five eager steps: weights, momentum and
    the step count (the kernel reads the count from device memory, so momentum's first-step rule and the published
    count follow the replays)."""
    from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN
    from pytorch_distributed_examples_amd.utils.graph import CapturedStep

    case = "sgd_mom_wd"
    data = _batches(gpu, 130)
    eager_net = _net(gpu)
    fe = FusedCNN(eager_net)
    ge = fe.grad_buffer()
    oe = _make_opt(case, eager_net.parameters())
    for x, y in data:
        fe.forward_backward(x, y, grad_out=ge, sgd=oe)
    net = _net(gpu)
    f = FusedCNN(net)
    g = f.grad_buffer()
    opt = _make_opt(case, net.parameters())

    def step(x, y):
        return f.forward_backward(x, y, grad_out=g, sgd=opt)

    step(*data[0])  # eager: step 1 (tables and hyper-parameters reach the device outside the capture)
    graph = CapturedStep(step, list(data[1]), warmup=0).capture()
    for x, y in data[1:]:
        graph(x, y)
    torch.cuda.synchronize()
    assert torch.equal(f.flat, fe.flat)
    s, se = _state(opt), _state(oe)
    for k in se:
        assert torch.equal(s[k]["momentum_buffer"], se[k]["momentum_buffer"])
        assert int(s[k]["step"]) == int(se[k]["step"]) == STEPS


def test_plain_sgd_keeps_mode_0_and_its_bits(gpu):
    """momentum = 0 and weight_decay = 0 select mode 0 -- today's kernel -- and three steps equal the generic
    route bit for bit (the existing guarantee, through the new argument)."""
    from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN, fused_update_mode
    from pytorch_distributed_examples_amd.ops.optim import FusedSGD

    data = _batches(gpu, 130)[:3]
    n_ref, n_fus = _net(gpu), _net(gpu)
    f_ref, f_fus = FusedCNN(n_ref), FusedCNN(n_fus)
    g_ref, g_fus = f_ref.grad_buffer(), f_fus.grad_buffer()
    o_ref, o_fus = FusedSGD(n_ref.parameters(), lr=0.05), FusedSGD(n_fus.parameters(), lr=0.05)
    assert fused_update_mode(o_fus) == 0
    l_ref = []
    for x, y in data:
        l_ref.append(f_ref.forward_backward(x, y, grad_out=g_ref).item())
        o_ref.step()
    l_fus = [f_fus.forward_backward(x, y, grad_out=g_fus, opt=o_fus).item() for x, y in data]
    torch.cuda.synchronize()
    assert l_ref == l_fus
    assert torch.equal(f_ref.flat, f_fus.flat)
    assert getattr(f_fus, "_opt_m", None) is None  # no state was bound
    assert all(int(s["step"]) == 3 for s in o_fus.state_dict()["state"].values())


def test_invalid_combinations_raise(gpu):
    from pytorch_distributed_examples_amd import _native
    from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN
    from pytorch_distributed_examples_amd.ops import functional as OF

    C = _native.C()
    x, y = _batches(gpu, 6)[0]
    net = _net(gpu)
    f = FusedCNN(net)
    g = f.grad_buffer()
    opt = _make_opt("sgd_mom", net.parameters())
    before = f.flat.detach().clone()

    class TwoRanks:  # an exchange view of two ranks: the binding refuses accumulation before anything is launched
        size = 2

        def view(self):
            v = [0] * 17
            v[13] = 2
            return v

    with pytest.raises(RuntimeError, match="accumulation"):
        f.forward_backward(x, y, grad_out=g, accumulate=True, sgd=opt, xgmi=TwoRanks())
    with pytest.raises(ValueError):
        f.forward_backward(x, y, grad_out=g, sgd=opt, opt=opt)
    # a stateful mode without its state, straight at the binding
    st = opt._group_dev(0, opt.param_groups[0], list(net.parameters()))
    rng = OF._rng_counter(gpu)
    m = torch.zeros_like(f.flat)

    def train(mode, m, v, hp=st["hp"], step=st["step"]):
        return C.cnn_train(x, y, f.flat, rng, 0.5, 0.5, False, g, False, frag=f.frag, prep=True, hp=hp, step=step,
                           mode=mode, m=m, v=v)

    with pytest.raises(RuntimeError, match="needs m "):
        train(1, None, None)
    with pytest.raises(RuntimeError, match="need v "):
        train(3, m, None)
    with pytest.raises(RuntimeError, match="needs hp and step"):
        train(1, m, None, step=None)
    with pytest.raises(RuntimeError, match="shaped like params"):
        train(1, m[:-4], None)
    with pytest.raises(RuntimeError, match="mode must be"):
        train(4, m, m)

    def update(mode, m, v, frag=f.frag):
        return C.cnn_opt(f.flat, g, frag, st["hp"], st["step"], mode=mode, m=m, v=v)

    with pytest.raises(RuntimeError, match="need v "):
        update(3, m, None)  # AdamW without exp_avg_sq
    # the refusals the one checker makes uniform
    unaligned = torch.empty(f.frag.numel() + 16, dtype=torch.uint8, device=gpu)[1:]
    assert unaligned.data_ptr() % 16 == 1 and unaligned.nbytes >= C.cnn_frag_bytes()
    with pytest.raises(RuntimeError, match="frag must be a 16-B aligned"):
        update(1, m, None, frag=unaligned)
    with pytest.raises(RuntimeError, match="shaped like params"):
        update(1, m.cpu(), None)
    with pytest.raises(RuntimeError, match="mode must be"):
        update(4, m, m)
    torch.cuda.synchronize()
    assert torch.equal(f.flat, before)  # nothing was launched
