"""Inputs, reference and error bound shared by the Adasum tests (tests/test_adasum_cpu.py, tests/test_adasum_gpu.py).

Inputs are CORRELATED, x_r = g + 0.5 noise_r (seeded CPU generators): independent random vectors have near-zero dot
products, Adasum then equals the plain sum and a test on them would pass on an ordinary all-reduce.  For N = 2 these
give coefficients near 1 - 1/2.5 = 0.6: about 0.6 (a + b), 67 % from the sum and 17 % from the average.

Vectors of ONE element are collinear, and for collinear vectors Adasum IS the average (adasum(a, b) = (a + b) / 2 for
scalars of one sign), so `assert_not_sum_or_average` asks for the distance to the average only from 2 elements up."""
import torch

from pytorch_distributed_examples_amd.hvd import adasum

CNN_SEGS = [250, 10, 5000, 20, 16000, 50, 500, 10]  # the MNIST CNN's 21,840 parameters, tensor by tensor


def rank_data(r, n, seed, noise=0.5):
    g = torch.randn(n, generator=torch.Generator().manual_seed(seed * 1000 + 999))
    e = torch.randn(n, generator=torch.Generator().manual_seed(seed * 1000 + r))
    return g + noise * e


def reference(xs, segs):
    """fp64 sequential tree, segment by segment, of the ranks' fused buffers ``xs``."""
    out, off = [], 0
    for n in segs:
        out.append(adasum.adasum_tree([x[off:off + n] for x in xs]))
        off += n
    assert off == xs[0].numel()
    return torch.cat(out)


def bound(xs, segs):
    """Elementwise bound for a device result (fp64 Gram, fp32 weights, fp32 rank-order combine) against
    `reference`: 4 N 2^-24 sum_r |w_r| |x_r| + 1e-30, w from the fp64 Gram of each segment.  Derived, not measured:
    N fp32 roundings of the weights, N of the products and N - 1 of the running sum, each relative 2^-24 of a term
    bounded by sum_r |w_r| |x_r|, is under 3 N 2^-24; 4 N leaves room for the Gram's own rounding."""
    N = len(xs)
    out, off = [], 0
    for n in segs:
        X = torch.stack([x[off:off + n].double() for x in xs])
        w = adasum.adasum_weights(X @ X.T)
        out.append(4 * N * 2.0 ** -24 * (w.abs()[:, None] * X.abs()).sum(0) + 1e-30)
        off += n
    return torch.cat(out)


def assert_not_sum_or_average(xs, ref):
    """On the reference alone: a plain sum or average of these inputs is at least 10 % (relative norm) away."""
    s = sum(x.double() for x in xs)
    d_sum = float((ref - s).norm() / ref.norm())
    assert d_sum >= 0.1, d_sum
    if ref.numel() > 1:  # (one element: collinear vectors, Adasum is the average -- see the module docstring)
        d_avg = float((ref - s / len(xs)).norm() / ref.norm())
        assert d_avg >= 0.1, d_avg
