"""conv2's data gradient in the fused CNN step (k_cnn_train, phase P7b) runs, for every 16-position tile of the
12x12 plane, only the k-steps in which some tap of the tile has a source inside the 8x8 conv2 output; the other
k-steps multiply the zero block.  The checks: the step is bit for bit what it is with every k-step run
(PDE_CNN_P7B_FULLK=1), and the gradients that depend on the border tiles agree with an fp32 reference that can
tell a wrong border from a right one."""
import copy

import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_examples_amd.models.cnn import Net
from pytorch_distributed_examples_amd.ops import functional as OF

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


@pytest.mark.parametrize("batch", [4, 7])
def test_fused_cnn_dgrad_ranges_match_full_range_bitwise(gpu, monkeypatch, batch):
    """Three training steps (dropout on, fused SGD) with the per-class k-step ranges and with the full range, from
    the same weights and the same dropout stream: losses, gradients and weights must be equal bit for bit (the
    skipped k-steps add +-0).  batch 4 is one full workgroup (all 36 tiles, every class); batch 7 adds a second
    workgroup with an empty image slot."""
    from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN
    from pytorch_distributed_examples_amd.ops.optim import FusedSGD

    torch.manual_seed(0)
    base = Net().to(gpu).train()
    x = torch.randn(3, batch, 1, 28, 28, device=gpu)
    y = torch.randint(0, 10, (3, batch), device=gpu)
    rng = OF._rng_counter(x.device)
    rng0 = rng.clone()
    runs = []
    for fullk in ("0", "1"):
        monkeypatch.setenv("PDE_CNN_P7B_FULLK", fullk)
        rng.copy_(rng0)  # the same dropout stream for both runs
        m = copy.deepcopy(base)
        f = FusedCNN(m)
        g = f.grad_buffer()
        opt = FusedSGD(m.parameters(), lr=0.05)
        losses = [f.forward_backward(x[i], y[i], grad_out=g, sgd=opt).item() for i in range(3)]
        torch.cuda.synchronize()
        runs.append((losses, g.clone(), f.flat.clone()))
    (l0, g0, w0), (l1, g1, w1) = runs
    assert all(torch.isfinite(torch.tensor(l0))) and g0.abs().sum().item() > 0
    assert l0 == l1, (l0, l1)
    assert torch.equal(g0, g1)
    assert torch.equal(w0, w1)


def _reference_grads(m, x, y, dr1_rows_zeroed=()):
    """Loss and parameter gradients of a CPU fp32 model whose conv operands are rounded to bf16 (identity
    gradient), as the fused kernel's are.  ``dr1_rows_zeroed``: rows Y of conv2's input gradient (the 12x12 dr1
    plane) forced to zero on the way back -- what a data gradient with a broken border would hand to conv1."""
    m = copy.deepcopy(m)

    def st(t):  # bf16-rounded value, identity gradient
        return t + (t.detach().to(torch.bfloat16).float() - t.detach())

    c1 = F.conv2d(st(x), st(m.conv1.weight), m.conv1.bias)
    r1 = st(F.relu(F.max_pool2d(c1, 2)))
    if dr1_rows_zeroed:
        keep = torch.ones(12)
        keep[list(dr1_rows_zeroed)] = 0.0
        r1.register_hook(lambda grad: grad * keep[None, None, :, None])
    c2 = F.conv2d(r1, st(m.conv2.weight), m.conv2.bias)
    r2 = F.relu(F.max_pool2d(c2, 2)).flatten(1)
    h = F.relu(F.linear(r2, m.fc1.weight, m.fc1.bias))
    loss = F.nll_loss(F.log_softmax(F.linear(h, m.fc2.weight, m.fc2.bias), 1), y)
    loss.backward()
    return loss.item(), {n: p.grad.clone() for n, p in m.named_parameters()}


def test_fused_cnn_dgrad_borders_match_fp32_reference(gpu):
    """One full workgroup (4 images, eval mode: no dropout); image i is non-zero only in a 7x7 patch at corner i,
    so conv1's weight gradient takes dr1 from the first / last four rows and columns of the plane only -- the tiles
    whose k-step ranges are cut -- and from nothing in the centre.  All eight parameter gradients against the
    bf16-operand fp32 reference at the bounds of test_fused_cnn_matches_reference; the control shows on the
    reference alone that a data gradient missing its rows 0, 1, 10, 11 fails that bound on conv1.weight."""
    from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN

    torch.manual_seed(0)
    m_cpu = Net().eval()
    m_gpu = copy.deepcopy(m_cpu).to(gpu).eval()
    fused = FusedCNN(m_gpu)
    patch = 7
    x = torch.zeros(4, 1, 28, 28)
    for i in range(4):
        r0 = 0 if i < 2 else 28 - patch
        c0 = 0 if i % 2 == 0 else 28 - patch
        x[i, 0, r0:r0 + patch, c0:c0 + patch] = torch.randn(patch, patch)
    y = torch.randint(0, 10, (4,))

    l_ref, g_ref = _reference_grads(m_cpu, x, y)
    # control: the reference itself, with the border rows of dr1 dropped, is outside the bound
    _, g_cut = _reference_grads(m_cpu, x, y, dr1_rows_zeroed=(0, 1, 10, 11))
    e_cut = rel_err(g_cut["conv1.weight"], g_ref["conv1.weight"])
    print("control: conv1.weight rel err with dr1 rows 0, 1, 10, 11 zeroed:", e_cut)
    assert e_cut > 3e-2, e_cut

    g = torch.zeros(fused.flat.numel(), device=gpu)
    loss = fused.forward_backward(x.to(gpu), y.to(gpu), grad_out=g)
    torch.cuda.synchronize()
    off, errs = 0, {}
    for n, p in m_cpu.named_parameters():
        k = p.numel()
        errs[n] = rel_err(g[off:off + k].cpu().view_as(p), g_ref[n])
        off += k
    print("loss", loss.item(), "reference", l_ref, "rel errs", errs)
    assert abs(loss.item() - l_ref) < 1e-2, (loss.item(), l_ref)
    assert len(errs) == 8 and all(v < 3e-2 for v in errs.values()), errs
