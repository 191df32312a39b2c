"""k_cnn_train / k_cnn_eval / k_cnn_reduce at the smallest batches at which the entry phases' clamped loads and
predicated LDS stores can go wrong: a workgroup with empty image slots, a workgroup with one image, one and two
workgroups in the reduction's tail loops.  Every load of the entry phase is unconditional from a clamped address, so
a value that leaks from a clamped slot shows up as a batch that is not the sum of its parts.  Fixture weights and
images: cnn_eval_fixture.py."""
import copy

import pytest
import torch

import cnn_eval_fixture as fx

pytestmark = pytest.mark.gpu

# the project's bound for two fused paths computing one quantity (test_eval_loss_equals_training_kernel_loss)
RTOL, ATOL = 1e-4, 1e-5


def _net(gpu):
    from pytorch_distributed_examples_amd.models.cnn import Net
    from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN

    net = Net().to(gpu)
    net.load_state_dict(fx.fixture()[0])
    return net, FusedCNN(net)


@pytest.fixture(scope="module")
def trained(gpu):
    """(net in eval mode, fused, images, labels) with the fixture weights; tests that write weights build their own."""
    net, fused = _net(gpu)
    x, y = fx.fixture()[1]["random"]
    return net.eval(), fused, x[:16].to(gpu), y[:16].to(gpu)


def _step(fused, x, y):
    """(loss, flat gradients) of one fused eval-mode step into a zeroed buffer."""
    g = torch.zeros_like(fused.flat)
    loss = fused.forward_backward(x, y, grad_out=g)
    torch.cuda.synchronize()
    return loss.clone(), g


def _check_additive(net, fused, parts, whole):
    """sum_i B_i * (loss_i, g_i) over the parts against B * (loss, g) of their concatenation, per parameter tensor.
    Every figure is printed before the first assertion.

    The kernel keeps every image's output gradient unscaled up to the reduction, which applies 1 / B in fp32, so an
    image contributes the same bf16 operands (dH, d2, e1) whatever batch it comes in and the two sides differ by
    fp32 summation order only: measured on MI355X, max |difference| 1.5e-8 .. 4.8e-7 per tensor at values of
    0.2 .. 4.3.  (While the operands held v / B, bf16(v / 5) * 5 was not bf16(v / 8) * 8 and conv1.weight,
    conv1.bias, conv2.weight and fc1.weight missed this bound by 1.6e-3 .. 4.6e-3.)"""
    (xw, yw), Bw = whole, whole[0].shape[0]
    assert sum(x.shape[0] for x, _ in parts) == Bw
    lw, gw = _step(fused, xw, yw)
    ls, gs = torch.zeros_like(lw), torch.zeros_like(gw)
    for x, y in parts:
        l, g = _step(fused, x, y)
        ls += x.shape[0] * l
        gs += x.shape[0] * g
    lw, gw = Bw * lw, Bw * gw
    print(f"B={Bw} from {[x.shape[0] for x, _ in parts]}: loss {ls.item():.9g} against {lw.item():.9g}, "
          f"difference {abs(ls.item() - lw.item()):.3e}")
    bad, off = [], 0
    for name, p in net.named_parameters():
        a, b = gs[off:off + p.numel()], gw[off:off + p.numel()]
        off += p.numel()
        d = (a - b).abs()
        excess = (d - (ATOL + RTOL * b.abs())).max().item()
        print(f"  {name}: max |difference| {d.max().item():.3e}, max |value| {b.abs().max().item():.3e}, "
              f"worst excess over atol + rtol |value| {excess:.3e}")
        if excess > 0:
            bad.append(name)
    assert off == gw.numel()
    torch.testing.assert_close(ls, lw, rtol=RTOL, atol=ATOL)
    assert not bad, bad


def test_batches_add_up_5_3_8(trained):
    """5 g5 + 3 g3 == 8 g8 (and the losses likewise) within rtol 1e-4, atol 1e-5, where the 8 images are the 5
    followed by the 3: B = 5 is a full workgroup plus one with a single image, B = 3 one workgroup with an empty
    slot, B = 8 two full ones -- nwg of 1 and 2 in the reduction's tail loops."""
    net, fused, x, y = trained
    _check_additive(net, fused, [(x[:5], y[:5]), (x[5:8], y[5:8])], (x[:8], y[:8]))


def test_batches_add_up_1_3_4(trained):
    """B = 1 (one workgroup, three empty slots) plus the three other images of a B = 4 workgroup, in the same way."""
    net, fused, x, y = trained
    _check_additive(net, fused, [(x[:1], y[:1]), (x[1:4], y[1:4])], (x[:4], y[:4]))


@pytest.mark.parametrize("B", [1, 5, 7])
def test_train_kernel_loss_equals_eval_kernel(trained, B):
    """k_cnn_train in eval mode against k_cnn_eval at partial workgroups: the batch-mean loss equals loss_sum / B
    within rtol 1e-4, atol 1e-5 (both kernels run the one shared entry phase)."""
    _, fused, x, y = trained
    loss = fused.forward_backward(x[:B], y[:B])
    loss_sum, _, count = fused.evaluate(x[:B], y[:B]).result()
    got = torch.tensor(loss_sum / count, dtype=torch.float32)
    print(f"B={B}: training-kernel loss {loss.item():.9g}, eval loss_sum / B {got.item():.9g}, "
          f"difference {abs(loss.item() - got.item()):.3e}")
    assert count == B
    torch.testing.assert_close(got, loss.cpu(), rtol=RTOL, atol=ATOL)


def test_dropout_replays_from_the_counter(gpu):
    """Dropout on at B = 5: two steps from the same counter value give bitwise-equal loss and gradients, the counter
    advances by one per step, and the next counter value draws other masks."""
    from pytorch_distributed_examples_amd.ops import functional as OF

    net, fused = _net(gpu)
    net.train()
    x, y = fx.fixture()[1]["random"]
    x, y = x[:5].to(gpu), y[:5].to(gpu)
    rng = OF._rng_counter(x.device)
    rng0 = rng.clone()
    try:
        runs = []
        for _ in range(2):
            rng.fill_(777)
            runs.append(_step(fused, x, y))
            assert int(rng.item()) == 778
        other = _step(fused, x, y)
        assert int(rng.item()) == 779
    finally:
        rng.copy_(rng0)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.isfinite(runs[0][1]).all() and not torch.equal(runs[0][1], other[1])


def test_fused_sgd_in_reduction_partial_workgroup(gpu):
    """B = 5, two steps: the SGD update inside the reduction against forward_backward + sgd_step -- bitwise-equal
    flat parameters (test_fused_cnn_sgd_matches_optimizer's relation at a partly filled workgroup)."""
    from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN
    from pytorch_distributed_examples_amd.ops.optim import FusedSGD

    m_ref, f_ref = _net(gpu)
    m_ref.eval()
    m_fus = copy.deepcopy(m_ref)
    f_fus = FusedCNN(m_fus)
    g_ref, g_fus = f_ref.grad_buffer(), f_fus.grad_buffer()
    o_ref, o_fus = FusedSGD(m_ref.parameters(), lr=0.05), FusedSGD(m_fus.parameters(), lr=0.05)
    xs, ys = fx.fixture()[1]["random"]
    xs, ys = xs[:10].to(gpu), ys[:10].to(gpu)
    start = f_ref.flat.clone()
    l_ref = []
    for i in range(2):  # (the reference first: its steps bump the global weight generation)
        l_ref.append(f_ref.forward_backward(xs[5 * i:5 * i + 5], ys[5 * i:5 * i + 5], grad_out=g_ref).item())
        f_ref.sgd_step(o_ref, g_ref)
    for i in range(2):
        l_fus = f_fus.forward_backward(xs[5 * i:5 * i + 5], ys[5 * i:5 * i + 5], grad_out=g_fus, sgd=o_fus)
        assert l_ref[i] == l_fus.item(), (i, l_ref[i], l_fus.item())
    torch.cuda.synchronize()
    assert torch.equal(f_ref.flat, f_fus.flat) and torch.equal(g_ref, g_fus)
    assert not torch.equal(f_fus.flat, start)
