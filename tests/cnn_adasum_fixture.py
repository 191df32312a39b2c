"""Inputs, CPU references and the emulation shared by the fused-CNN Adasum tests (test_cnn_adasum_cpu.py,
test_cnn_adasum_gpu.py).

Rank ``r`` of ``N`` takes the next ``70 + 60 r`` images of ``mnist_splits(train=4096)`` in order, with their labels,
dropout off: a partial 4-image tile and unequal ranks (70 and 130 at two ranks), the ragged sizes of
test_cnn_fused_optim_xgmi_gpu.py.  Weights come from ``torch.manual_seed(0)``.

The deltas of these batches are correlated (they share the weights and the class templates), so their per-tensor
Adasum tree is far from both their sum and their average -- `conditions` asserts that on the fp64 reference alone --
and every tensor's squared delta norm is at least 10 x kAdasumEps on every rank, so the device and the fp64 reference
cannot take different branches of ``adasum_weights``.  That holds at lr 0.05 for SGD (at 0.01 the bias tensors' norms
land ON the threshold) and at lr 0.01 for Adam / AdamW, whose deltas are about lr per element."""
import functools

import torch
import torch.nn.functional as F

from adasum_fixture import CNN_SEGS, assert_not_sum_or_average, bound, reference
from cnn_eval_fixture import PlainNet

from pytorch_distributed_examples_amd.hvd import adasum

NPARAM = sum(CNN_SEGS)
CHUNK = 256  # elements per workgroup of the two Adasum launches (one parameter per thread)
SGD_LR, ADAM_LR, WD = 0.05, 0.01, 1e-2


def sizes(n_ranks):
    return [70 + 60 * r for r in range(n_ranks)]


def batch_range(r, n_ranks, step=0):
    """[lo, hi) of rank r's images at `step`: the ranks take consecutive runs, the steps consecutive rounds."""
    sz = sizes(n_ranks)
    lo = step * sum(sz) + sum(sz[:r])
    return lo, lo + sz[r]


@functools.lru_cache(maxsize=None)
def images():
    from pytorch_distributed_examples_amd.data.synthetic import mnist_splits

    train, _ = mnist_splits(train=4096, test=16)
    return train.images.float().reshape(-1, 1, 28, 28).cpu(), train.labels.long().cpu()


def batch(r, n_ranks, step=0):
    xs, ys = images()
    lo, hi = batch_range(r, n_ranks, step)
    assert hi <= xs.shape[0]
    return xs[lo:hi], ys[lo:hi]


def flat(tensors):
    return torch.cat([t.detach().reshape(-1) for t in tensors])


def _net():
    torch.manual_seed(0)
    return PlainNet()


@functools.lru_cache(maxsize=None)
def cpu_case(n_ranks):
    """``(start, grads, sgd_deltas, adamw_deltas)`` of step 0 in fp32 on the CPU: the shared weights, every rank's
    mean gradient, its plain-SGD delta at lr 0.05 and its AdamW delta (lr 0.01, weight decay 1e-2), each delta as
    ``local_update(start) - start`` in fp32 -- what launch A stages."""
    start = flat(_net().parameters())
    grads, sgd, adamw = [], [], []
    for r in range(n_ranks):
        x, y = batch(r, n_ranks)
        for kind in ("sgd", "adamw"):
            net = _net()
            opt = (torch.optim.SGD(net.parameters(), lr=SGD_LR) if kind == "sgd" else
                   torch.optim.AdamW(net.parameters(), lr=ADAM_LR, weight_decay=WD))
            F.nll_loss(net(x), y).backward()
            if kind == "sgd":
                grads.append(flat(p.grad for p in net.parameters()))
            opt.step()
            (sgd if kind == "sgd" else adamw).append(flat(net.parameters()) - start)
    return start, grads, sgd, adamw


def conditions(deltas):
    """The two conditions on the reference deltas alone: the fp64 per-tensor tree is at least 10 % (relative norm)
    from the plain sum and from the average, and every tensor's squared norm on every rank is at least
    10 x kAdasumEps.  Returns (distance from the sum, distance from the average, smallest squared norm)."""
    ref = reference(deltas, CNN_SEGS)
    assert_not_sum_or_average(deltas, ref)
    s = sum(d.double() for d in deltas)
    smallest, off = float("inf"), 0
    for n in CNN_SEGS:
        for d in deltas:
            smallest = min(smallest, float(d[off:off + n].double().pow(2).sum()))
        off += n
    assert smallest >= 10 * adasum.eps(), smallest
    return (float((ref - s).norm() / ref.norm()), float((ref - s / len(deltas)).norm() / ref.norm()), smallest)


def want_and_bound(start, deltas, adam=False):
    """fp64 ``start + reference(deltas)`` and the elementwise bound of a device result against it:
    ``adasum_fixture.bound`` on the delta plus the fp32 rounding of ``start + delta``; for Adam / AdamW also
    ``1e-5 sum_r |w_r| |delta_r|`` -- the rtol of these updates between two kernels, carried through the combine."""
    want = start.double() + reference(deltas, CNN_SEGS)
    bnd = bound(deltas, CNN_SEGS) + 2.0 ** -24 * want.abs()
    if adam:
        out, off = [], 0
        for n in CNN_SEGS:
            X = torch.stack([d[off:off + n].double() for d in deltas])
            w = adasum.adasum_weights(X @ X.T)
            out.append(1e-5 * (w.abs()[:, None] * X.abs()).sum(0))
            off += n
        bnd = bnd + torch.cat(out)
    return want, bnd


def worst_fraction(got, want, bnd):
    return float(((got.double() - want).abs() / bnd).max())


def _fma(a, b, c):
    """fp32 fma(a, b, c): the product of two fp32 values is exact in fp64."""
    return (a.double() * b.double() + c.double()).float()


def pieces(segs=CNN_SEGS, chunk=CHUNK):
    """(tensor s, chunk b, lo, hi) of every piece, in order: chunks of `chunk` elements split at tensor ends."""
    out, lo_s = [], 0
    for s, n in enumerate(segs):
        hi_s = lo_s + n
        for b in range(lo_s // chunk, (hi_s - 1) // chunk + 1):
            out.append((s, b, max(lo_s, b * chunk), min(hi_s, (b + 1) * chunk)))
        lo_s = hi_s
    return out


def emulate(start, deltas, segs=CNN_SEGS, chunk=CHUNK, order=None):
    """Launches A and B on the CPU: fp64 piece Grams in workspace rows b + s, each tensor's rows summed in row
    order, fp32 weights, ``w_0 x_0`` then the rank-order fma, ``start + acc`` in fp32.
    ``order``: a permutation the tree is built on (a mutation; the combine stays in rank order)."""
    N = len(deltas)
    X = torch.stack([d.float() for d in deltas])
    rows = {}
    for s, b, lo, hi in pieces(segs, chunk):
        P = X[:, lo:hi].double()
        assert b + s not in rows
        rows[b + s] = P @ P.T
    out = start.float().clone()
    lo_s = 0
    for s, n in enumerate(segs):
        hi_s = lo_s + n
        row0, row1 = lo_s // chunk + s, (hi_s - 1) // chunk + s
        G = rows[row0].clone()
        for row in range(row0 + 1, row1 + 1):
            G = G + rows[row]
        if order is None:
            w = adasum.adasum_weights(G)
        else:
            idx = torch.tensor(order)
            w = torch.empty(N, dtype=torch.float64)
            w[idx] = adasum.adasum_weights(G[idx][:, idx])
        wf = w.float()
        acc = wf[0] * X[0, lo_s:hi_s]
        for r in range(1, N):
            acc = _fma(wf[r].expand_as(acc), X[r, lo_s:hi_s], acc)
        out[lo_s:hi_s] = start[lo_s:hi_s].float() + acc
        lo_s = hi_s
    return out
