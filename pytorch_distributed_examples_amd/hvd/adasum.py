"""``hvd.Adasum`` in torch float64: the CPU data plane and the reference the tests compare the kernels against.

Two gradients combine as

    adasum(a, b) = (1 - a.b / (2 |a|^2)) a + (1 - a.b / (2 |b|^2)) b

(a coefficient is 1 when its vector's squared norm is below ``eps()``), and N = 2^k ranks as the tree over
contiguous halves, ``A(lo, hi) = adasum(A(lo, mid), A(mid, hi))`` -- Horovod's distance-doubling pairs (0,1),
(2,3), then (01, 23), ...  Dot products and norms are per tensor, never over a fused buffer as a whole.  A uniform
scale passes straight through: ``adasum(s a, s b) = s adasum(a, b)``.

Every tree node is a linear combination of the rank vectors, so the tree is ``sum_r w_r x_r`` with the weights a
function of the Gram matrix ``G[i][j] = x_i . x_j`` alone (:func:`adasum_weights`): the form the GPU kernels
compute (csrc/comm/adasum_weights.h, ``XgmiAllreduce::adasum``).
"""
from __future__ import annotations

import torch

from .. import _native


def eps() -> float:
    """The squared-norm threshold below which a coefficient is 1 (kAdasumEps, csrc/comm/adasum_weights.h)."""
    return float(_native.comm().ADASUM_EPS)


def is_power_of_two(n: int) -> bool:
    return n >= 1 and (n & (n - 1)) == 0


def adasum_pair(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """adasum(a, b) in float64 (inputs of any float dtype and shape; the result is float64, shaped like ``a``)."""
    a64, b64 = a.double(), b.double()
    dot = torch.dot(a64.reshape(-1), b64.reshape(-1))
    na = torch.dot(a64.reshape(-1), a64.reshape(-1))
    nb = torch.dot(b64.reshape(-1), b64.reshape(-1))
    e = eps()
    ca = 1.0 if float(na) < e else 1.0 - float(dot) / (2.0 * float(na))
    cb = 1.0 if float(nb) < e else 1.0 - float(dot) / (2.0 * float(nb))
    return ca * a64 + cb * b64


def adasum_tree(tensors) -> torch.Tensor:
    """The sequential tree over contiguous halves of ``tensors`` (one per rank, a power of two of them)."""
    xs = [t.double() for t in tensors]
    if not is_power_of_two(len(xs)):
        raise ValueError(f"Adasum needs a power-of-two number of ranks, not {len(xs)}")
    while len(xs) > 1:
        xs = [adasum_pair(xs[i], xs[i + 1]) for i in range(0, len(xs), 2)]
    return xs[0]


def adasum_weights(gram: torch.Tensor) -> torch.Tensor:
    """The N weights of the tree from the [N, N] Gram matrix: ``adasum_tree(xs) == sum_r w[r] * xs[r]``."""
    G = gram.double()
    n = G.shape[0]
    if G.dim() != 2 or G.shape[1] != n or not is_power_of_two(n):
        raise ValueError("adasum_weights expects an [N, N] Gram matrix, N a power of two")
    e = eps()
    w = torch.ones(n, dtype=torch.float64)
    span = 1
    while span < n:
        for lo in range(0, n, 2 * span):
            mid, hi = lo + span, lo + 2 * span
            wa, wb = w[lo:mid], w[mid:hi]
            na = float(wa @ G[lo:mid, lo:mid] @ wa)
            nb = float(wb @ G[mid:hi, mid:hi] @ wb)
            dot = float(wa @ G[lo:mid, mid:hi] @ wb)
            ca = 1.0 if na < e else 1.0 - dot / (2.0 * na)
            cb = 1.0 if nb < e else 1.0 - dot / (2.0 * nb)
            w[lo:mid] *= ca
            w[mid:hi] *= cb
        span *= 2
    return w


def adasum_segments_(gathered: torch.Tensor, out: torch.Tensor, seg_lengths) -> torch.Tensor:
    """``gathered``: [N, n], every rank's fused buffer; ``out`` [n] gets the per-segment tree (cast to its dtype).
    The same arithmetic on the same values on every rank, so every rank holds the same bits."""
    off = 0
    for n in seg_lengths:
        n = int(n)
        if n:
            out[off:off + n] = adasum_tree([gathered[r, off:off + n] for r in range(gathered.shape[0])]).to(out.dtype)
        off += n
    if off != out.numel():
        raise ValueError("Adasum: the segment lengths do not cover the fused buffer")
    return out
