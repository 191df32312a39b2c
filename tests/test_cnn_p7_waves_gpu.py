"""conv2's backward in the fused CNN step (k_cnn_train, phase P7) runs its two gradients on separate waves: eight
waves take the data gradient, one tile class for ALL FOUR image slots of the workgroup each (classes 0 and 8 share
a wave), and the other eight the weight gradient, two of the 16 kidx column blocks (N-tiles) each.  The checks: the
gradients that pass through those waves agree with the fp32 reference on bf16-rounded operands at batches that fill
a workgroup partly, exactly, and with one image over; every image slot and every pair of N-tiles is visible in them;
a second run of a step repeats its bits; and the step with every k-step run (PDE_CNN_P7B_FULLK=1, in a child
process) has the same bits at batches where one and all four tiles of a dgrad wave are live.

The bound is the one of test_cnn_idle_windows_gpu.py / test_cnn_dgrad_ranges_gpu.py: relative error 3e-2 of the
tensor (or block) against the reference, ||a - b|| / ||b||, which holds every element's error under 3e-2 ||b||."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_examples_amd.models.cnn import Net
from pytorch_distributed_examples_amd.ops import functional as OF

pytestmark = pytest.mark.gpu

BOUND = 3e-2  # test_fused_cnn_every_dgrad_tile_of_every_image_is_visible's
P7_NAMES = ("conv2.weight", "conv1.weight", "conv1.bias")  # what P7a writes and what P7b's e1 feeds (P9)
COUNTER = 4242  # the fixed dropout counter
P2 = P1 = 0.5


def rel_err(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _hash_u01(seed: int, ids):
    """Host copy of cnn_fused.hip's counter hash (splitmix64 finaliser over seed + golden * (id + 1))."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (np.asarray(ids, dtype=np.uint64) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float64) / 16777216.0


def _masks(counter: int, n: int):
    """The training kernel's Dropout2d [n, 20] and dropout [n, 50] multipliers for RNG counter ``counter``."""
    seed = (counter * 0xD1B54A32D192ED03) % (1 << 64)
    u2 = _hash_u01(seed ^ 0x5BD1E995, np.arange(n * 20)).reshape(n, 20)
    u1 = _hash_u01(seed ^ 0x27D4EB2F, np.arange(n * 50)).reshape(n, 50)
    m2 = np.where(u2 >= np.float32(P2), np.float32(1.0) / np.float32(1.0 - P2), 0.0).astype(np.float32)
    m1 = np.where(u1 >= np.float32(P1), np.float32(1.0) / np.float32(1.0 - P1), 0.0).astype(np.float32)
    return torch.from_numpy(m2), torch.from_numpy(m1)


def _reference_grads(m, x, y, masks=None, dr1_zeroed=None):
    """Loss and parameter gradients of a CPU fp32 model whose conv operands are rounded to bf16 (identity
    gradient), as the fused kernel's are.  ``masks`` = (Dropout2d [n, 20], dropout [n, 50]) multipliers.
    ``dr1_zeroed`` = (image, first position, one past the last): row-major positions of that image's 12x12 dr1 plane
    forced to zero on the way back -- what a lost dgrad tile would hand to conv1."""
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
    if masks is not None:
        c2 = c2 * masks[0][:, :, None, None]
    r2 = F.relu(F.max_pool2d(c2, 2)).flatten(1)
    h = F.relu(F.linear(r2, m.fc1.weight, m.fc1.bias))
    if masks is not None:
        h = h * masks[1]
    loss = F.nll_loss(F.log_softmax(F.linear(h, m.fc2.weight, m.fc2.bias), 1), y)
    loss.backward()
    return loss.item(), {n: p.grad.clone() for n, p in m.named_parameters()}


@pytest.fixture(scope="module")
def nets(gpu):
    """One set of weights for the module: the CPU model (the reference's) and its fused GPU twin."""
    from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN

    torch.manual_seed(0)
    m_cpu = Net().eval()
    m_gpu = copy.deepcopy(m_cpu).to(gpu).eval()
    return m_cpu, m_gpu, FusedCNN(m_gpu)


def _fused_step(nets, x, y, gpu, dropout):
    """(loss, flat gradient on the CPU) of one fused step; with ``dropout`` in training mode from COUNTER."""
    _, m_gpu, fused = nets
    m_gpu.train(dropout)
    try:
        if dropout:
            OF._rng_counter(gpu).fill_(COUNTER)
        g = torch.zeros(fused.flat.numel(), device=gpu)
        loss = fused.forward_backward(x.to(gpu), y.to(gpu), grad_out=g, p_drop2=P2, p_drop1=P1)
        torch.cuda.synchronize()
    finally:
        m_gpu.eval()
    return loss.item(), g.cpu()


def _named(m_cpu, g):
    out, off = {}, 0
    for n, p in m_cpu.named_parameters():
        out[n] = g[off:off + p.numel()].view_as(p)
        off += p.numel()
    return out


@pytest.mark.parametrize("dropout", [False, True], ids=["eval", "dropout"])
@pytest.mark.parametrize("batch", [1, 4, 5, 8])
def test_fused_cnn_p7_gradients_match_reference_and_repeat(gpu, nets, batch, dropout):
    """Batch 1: one workgroup with three empty slots (three of a dgrad wave's four tiles see only zeros); 4: one
    full workgroup; 5: a full one and one image; 8: two full ones.  conv2.weight (P7a), conv1.weight and conv1.bias
    (P7b through e1 and P9) against the reference, the loss too; the same step again is bit for bit the first."""
    m_cpu = nets[0]
    gen = torch.Generator().manual_seed(300 + batch)
    x = torch.randn(batch, 1, 28, 28, generator=gen)
    y = torch.randint(0, 10, (batch,), generator=gen)
    l_ref, g_ref = _reference_grads(m_cpu, x, y, masks=_masks(COUNTER, batch) if dropout else None)
    loss, flat = _fused_step(nets, x, y, gpu, dropout)
    loss2, flat2 = _fused_step(nets, x, y, gpu, dropout)
    g = _named(m_cpu, flat)
    errs = {n: rel_err(g[n], g_ref[n]) for n in P7_NAMES}
    worst = {n: ((g[n] - g_ref[n]).abs().max() / (g_ref[n].norm() + 1e-12)).item() for n in P7_NAMES}
    print("batch", batch, "dropout", dropout, "loss", loss, l_ref, "rel errs", errs, "largest element error / norm",
          worst)
    assert torch.isfinite(flat).all() and flat.abs().sum().item() > 0
    assert abs(loss - l_ref) < 1e-2, (loss, l_ref)
    assert all(v < BOUND for v in errs.values()), errs
    assert all(v < BOUND for v in worst.values()), worst  # per element (implied by the norm bound)
    assert loss2 == loss and torch.equal(flat2, flat)


@pytest.fixture(scope="module")
def zero_run(gpu, nets):
    """The step over four all-zero images (labels 0..3): what a slot's image must change."""
    loss, flat = _fused_step(nets, torch.zeros(4, 1, 28, 28), torch.arange(4), gpu, False)
    return _named(nets[0], flat)


@pytest.mark.parametrize("slot", [0, 1, 2, 3])
def test_fused_cnn_p7_every_slot_and_tile_pair_is_visible(gpu, nets, zero_run, slot):
    """One full workgroup in which only image ``slot`` is non-zero (labels as in the all-zero run).  conv1.weight's
    gradient then comes from that slot's dr1 alone, through all nine dgrad classes: it matches the reference, differs
    from the all-zero run, and the control shows on the reference alone that dr1 without any one class is outside
    the bound.  conv1.bias likewise against the reference and the all-zero run.  conv2.weight per wgrad wave = pair
    of 16-column kidx blocks, each block for both co tiles: inside the bound and different from the all-zero run."""
    m_cpu = nets[0]
    gen = torch.Generator().manual_seed(400 + slot)
    x = torch.zeros(4, 1, 28, 28)
    x[slot] = torch.randn(1, 28, 28, generator=gen)
    y = torch.arange(4)
    l_ref, g_ref = _reference_grads(m_cpu, x, y)
    ctl = []
    for c in range(9):
        _, g_cut = _reference_grads(m_cpu, x, y, dr1_zeroed=(slot, 16 * c, 16 * c + 16))
        ctl.append(rel_err(g_cut["conv1.weight"], g_ref["conv1.weight"]))
    loss, flat = _fused_step(nets, x, y, gpu, False)
    g = _named(m_cpu, flat)
    e1 = {n: rel_err(g[n], g_ref[n]) for n in ("conv1.weight", "conv1.bias")}
    a, b, z = (t["conv2.weight"].reshape(20, 250) for t in (g, g_ref, zero_run))
    blocks, same = {}, []
    for pair in range(8):  # wgrad wave `pair`: N-tiles 2 pair, 2 pair + 1
        for nt in (2 * pair, 2 * pair + 1):
            for co0, co1 in ((0, 16), (16, 20)):
                cols = slice(16 * nt, min(16 * nt + 16, 250))
                blocks[(pair, nt, co0)] = rel_err(a[co0:co1, cols], b[co0:co1, cols])
                if torch.equal(a[co0:co1, cols], z[co0:co1, cols]):
                    same.append((pair, nt, co0))
    print("slot", slot, "loss", loss, l_ref, "conv1 errs", e1, "control (dr1 without class c)", ctl,
          "largest conv2.weight block err", max(blocks.values()))
    assert min(ctl) > BOUND, ctl
    assert abs(loss - l_ref) < 1e-2, (loss, l_ref)
    assert all(v < BOUND for v in e1.values()), e1
    assert zero_run["conv1.weight"].abs().sum().item() == 0 and g["conv1.weight"].abs().sum().item() > 0
    assert not torch.equal(g["conv1.bias"], zero_run["conv1.bias"])
    assert len(blocks) == 32 and all(v < BOUND for v in blocks.values()), blocks
    assert not same, same


_CHILD = r"""
import sys, torch
from pytorch_distributed_examples_amd.models.cnn import Net
from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN
from pytorch_distributed_examples_amd.ops import functional as OF
blob = torch.load(sys.argv[1])
dev = torch.device("cuda:0")
m = Net().to(dev).train()
m.load_state_dict(blob["state"])
fused = FusedCNN(m)
for case in blob["cases"]:
    OF._rng_counter(dev).fill_(blob["counter"])
    g = torch.zeros(fused.flat.numel(), device=dev)
    loss = fused.forward_backward(case["x"].to(dev), case["y"].to(dev), grad_out=g)
    torch.cuda.synchronize()
    n = case["x"].shape[0]
    assert loss.item() == case["loss"], (n, loss.item(), case["loss"])
    assert torch.equal(g.cpu(), case["grads"]), ("gradients", n)
print("P7_FULLK_OK")
"""


def test_fused_cnn_p7_full_range_child_is_bit_identical(gpu, nets, tmp_path):
    """PDE_CNN_P7B_FULLK=1 in a child process: the dgrad k-loops run all 19 k-steps of every class.  The skipped
    k-steps add exact zeros, so losses and flat gradients of a training step (dropout from COUNTER) equal this
    process's bit for bit -- at batch 5 (second workgroup: one live tile per dgrad wave) and at batch 8 (all four
    tiles of every dgrad wave live in both workgroups)."""
    m_cpu = nets[0]
    cases = []
    for batch in (5, 8):
        gen = torch.Generator().manual_seed(500 + batch)
        x = torch.randn(batch, 1, 28, 28, generator=gen)
        y = torch.randint(0, 10, (batch,), generator=gen)
        loss, flat = _fused_step(nets, x, y, gpu, True)
        assert torch.isfinite(flat).all() and flat.abs().sum().item() > 0
        cases.append(dict(x=x, y=y, loss=loss, grads=flat))
    path = tmp_path / "p7_fullk.pt"
    torch.save(dict(state=m_cpu.state_dict(), counter=COUNTER, cases=cases), path)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PDE_CNN_P7B_FULLK="1")
    res = subprocess.run([sys.executable, "-c", _CHILD, str(path)], env=env, capture_output=True, text=True,
                         timeout=120, cwd=repo)
    assert res.returncode == 0 and "P7_FULLK_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]
