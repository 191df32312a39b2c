"""The fused CNN step (k_cnn_train) fills several LDS regions of its backward ahead of the phase that used to write
them: the conv2-output gradient planes d2 / d2n are zeroed at kernel entry and P6 stores only the argmax tap of a live
cell; the conv2 data-gradient fragments w2d and the [ci][cell] planes r1 are written inside P4 by the waves that have
no image there (r1 as a transpose of the channel-last r1n).  The checks: nothing a previous kernel left in those
regions reaches a result, every dgrad tile of every image slot is visible in the gradients, and so is every 16 x 16
block of conv2's weight gradient.  Batch 4 is one full workgroup; batch 7 adds a second one with an empty image
slot."""
import copy

import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_examples_amd.models.cnn import Net
from pytorch_distributed_examples_amd.ops import functional as OF

pytestmark = pytest.mark.gpu

BOUND = 3e-2  # relative error against the bf16-operand fp32 reference (test_cnn_dgrad_ranges_gpu.py)


def rel_err(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _reference_grads(m, x, y, dr1_zeroed=None):
    """Loss and parameter gradients of a CPU fp32 model whose conv operands are rounded to bf16 (identity
    gradient), as the fused kernel's are (the helper of test_cnn_dgrad_ranges_gpu.py).  ``dr1_zeroed`` = (image,
    first position, one past the last): row-major positions of that image's 12x12 dr1 plane (conv2's input
    gradient, all channels) forced to zero on the way back -- what a lost dgrad tile would hand to conv1."""
    m = copy.deepcopy(m)

    def st(t):  # bf16-rounded value, identity gradient
        return t + (t.detach().to(torch.bfloat16).float() - t.detach())

    c1 = F.conv2d(st(x), st(m.conv1.weight), m.conv1.bias)
    r1 = st(F.relu(F.max_pool2d(c1, 2)))
    if dr1_zeroed is not None:
        s, p0, p1 = dr1_zeroed
        keep = torch.ones(x.shape[0], 1, 144)
        keep[s, 0, p0:p1] = 0.0
        keep = keep.view(x.shape[0], 1, 12, 12)
        r1.register_hook(lambda grad: grad * keep)
    c2 = F.conv2d(r1, st(m.conv2.weight), m.conv2.bias)
    r2 = F.relu(F.max_pool2d(c2, 2)).flatten(1)
    h = F.relu(F.linear(r2, m.fc1.weight, m.fc1.bias))
    loss = F.nll_loss(F.log_softmax(F.linear(h, m.fc2.weight, m.fc2.bias), 1), y)
    loss.backward()
    return loss.item(), {n: p.grad.clone() for n, p in m.named_parameters()}


@pytest.fixture(scope="module")
def nets(gpu):
    """One set of weights for the module: the CPU model (the reference's) and its fused GPU twin, eval mode."""
    from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN

    torch.manual_seed(0)
    m_cpu = Net().eval()
    m_gpu = copy.deepcopy(m_cpu).to(gpu).eval()
    return m_cpu, FusedCNN(m_gpu)


def _fused_grads(fused, m_cpu, x, y, gpu):
    g = torch.zeros(fused.flat.numel(), device=gpu)
    loss = fused.forward_backward(x.to(gpu), y.to(gpu), grad_out=g)
    torch.cuda.synchronize()
    out, off = {}, 0
    g = g.cpu()
    for n, p in m_cpu.named_parameters():
        out[n] = g[off:off + p.numel()].view_as(p)
        off += p.numel()
    return loss.item(), out


@pytest.mark.parametrize("batch", [4, 7])
def test_fused_cnn_stale_lds_cannot_leak_in(gpu, batch):
    """A training step (dropout on), then one step of a throwaway copy over 1024 images of +inf -- every CU's LDS is
    left holding inf / NaN in r1, d2, d2n and the fragment regions -- then the first step again from the same weights
    and dropout counter: finite and bit for bit the first.  A zero-fill that misses one slot P7a / P7b read, or an r1
    / w2d word nobody wrote, shows as NaN or as a difference."""
    from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN

    torch.manual_seed(1)
    m = Net().to(gpu).train()
    fused = FusedCNN(m)
    x = torch.randn(batch, 1, 28, 28, device=gpu)
    y = torch.randint(0, 10, (batch,), device=gpu)
    rng = OF._rng_counter(x.device)
    rng0 = rng.clone()

    def step():
        rng.copy_(rng0)
        g = torch.zeros(fused.flat.numel(), device=gpu)
        loss = fused.forward_backward(x, y, grad_out=g)
        torch.cuda.synchronize()
        return loss.item(), g

    l0, g0 = step()
    poison = FusedCNN(copy.deepcopy(m))
    gp = torch.zeros(poison.flat.numel(), device=gpu)
    poison.forward_backward(torch.full((1024, 1, 28, 28), float("inf"), device=gpu),
                            torch.zeros(1024, dtype=torch.long, device=gpu), grad_out=gp)
    torch.cuda.synchronize()
    l1, g1 = step()
    print("loss", l0, l1, "|g|", g0.norm().item(), g1.norm().item())
    assert torch.isfinite(torch.tensor([l0, l1])).all() and g0.abs().sum().item() > 0
    assert torch.isfinite(g0).all() and torch.isfinite(g1).all()
    assert l0 == l1, (l0, l1)
    assert torch.equal(g0, g1)


@pytest.mark.parametrize("batch", [4, 7])
def test_fused_cnn_every_dgrad_tile_of_every_image_is_visible(gpu, nets, batch):
    """For every image slot s and dgrad tile class c (16 row-major positions 16c .. 16c + 15 of the 12x12 plane, rows
    Y0 .. Y1): image s is non-zero only in the image rows 2 Y0 .. 2 Y1 + 5 that conv1 reads for those rows, every
    other image is zero.  All eight parameter gradients against the reference; the control shows on the reference
    alone that dr1 of image s without exactly that tile puts conv1.weight outside the bound."""
    m_cpu, fused = nets
    gen = torch.Generator().manual_seed(100 + batch)
    worst, worst_ctl, bad = 0.0, float("inf"), []
    for s in range(batch):
        for c in range(9):
            y0, y1 = (16 * c) // 12, (16 * c + 15) // 12
            x = torch.zeros(batch, 1, 28, 28)
            rows = slice(2 * y0, min(2 * y1 + 5, 27) + 1)
            x[s, 0, rows, :] = torch.randn(x[s, 0, rows, :].shape, generator=gen)
            y = torch.randint(0, 10, (batch,), generator=gen)
            l_ref, g_ref = _reference_grads(m_cpu, x, y)
            _, g_cut = _reference_grads(m_cpu, x, y, dr1_zeroed=(s, 16 * c, 16 * c + 16))
            e_cut = rel_err(g_cut["conv1.weight"], g_ref["conv1.weight"])
            loss, g = _fused_grads(fused, m_cpu, x, y, gpu)
            errs = {n: rel_err(g[n], g_ref[n]) for n in g_ref}
            worst, worst_ctl = max(worst, max(errs.values())), min(worst_ctl, e_cut)
            if e_cut <= BOUND:
                bad.append(("control", s, c, e_cut))
            if not (abs(loss - l_ref) < 1e-2 and len(errs) == 8 and all(v < BOUND for v in errs.values())):
                bad.append(("fused", s, c, loss, l_ref, errs))
    print("batch", batch, "largest rel err", worst, "smallest control err", worst_ctl)
    assert not bad, bad


@pytest.mark.parametrize("batch", [4, 7])
def test_fused_cnn_every_conv2_wgrad_block_is_visible(gpu, nets, batch):
    """Random full images: conv2.weight's gradient per block of (co 0..15 | 16..19) x 16 consecutive kidx = (ci, ky,
    kx) -- the tiles of the wgrad GEMM, 32 blocks -- each within the bound.  A lost or misplaced d2 / r1 value gives a
    block error of order 1; the bf16 rounding of the gradients, which the reference does not model, at most 3.5e-3."""
    m_cpu, fused = nets
    gen = torch.Generator().manual_seed(200 + batch)
    x = torch.randn(batch, 1, 28, 28, generator=gen)
    y = torch.randint(0, 10, (batch,), generator=gen)
    l_ref, g_ref = _reference_grads(m_cpu, x, y)
    loss, g = _fused_grads(fused, m_cpu, x, y, gpu)
    a, b = g["conv2.weight"].reshape(20, 250), g_ref["conv2.weight"].reshape(20, 250)
    errs = {}
    for co0, co1 in ((0, 16), (16, 20)):
        for k0 in range(0, 250, 16):
            errs[(co0, k0)] = rel_err(a[co0:co1, k0:k0 + 16], b[co0:co1, k0:k0 + 16])
    print("batch", batch, "loss", loss, l_ref, "largest block err", max(errs.values()))
    assert abs(loss - l_ref) < 1e-2, (loss, l_ref)
    assert len(errs) == 32 and all(v < BOUND for v in errs.values()), errs
