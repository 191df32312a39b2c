"""Max pooling, global average pooling and dropout (csrc/kernels/norm_pool.hip), exact where the arithmetic allows.

Max pooling: integer inputs in [-3, 3] -- ties everywhere, exact zeros under ``relu`` -- against a reference written
here from ``unfold`` with the tie rule stated: the FIRST tap in (ky, kx) scan order that holds the window's maximum
(taps outside the image never win).  y, the saved argmax and dx (integer dy; at most 9 overlapping windows sum small
integers, exact in fp32 and in bf16) are compared with ``torch.equal``.
Average pooling: forward within 2^-8 |ref| + HW u mean|x| (the bf16 half-ulp and HW sequential fp32 adds); the
backward equals bf16(dy * (1.f / HW)) bit for bit; integer inputs at HW = 16 are exact.
Dropout: kept outputs equal bf16(x * (1.f / (1.f - p))), gradients bf16(dy * scale) * mask, bit for bit; keep counts
within 5 sigma of the binomial; the channel mode's mask is constant over H x W and differs between images, calls and
replays of one captured graph."""
import math

import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_examples_amd.ops import functional as OF

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF = 2.0 ** -8


# ---- max pooling ----------------------------------------------------------------------------------------------------


def _ints(g, shape, lim=3):
    return torch.randint(-lim, lim + 1, shape, generator=g).double()


def maxpool_reference(x, dy, k, s, p, relu):
    """x [N, H, W, C], dy [N, Ho, Wo, C], float64 -> (y, argmax tap ky * k + kx, dx) in the same layout."""
    n, h, w, c = x.shape
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    xp = F.pad(x.permute(0, 3, 1, 2), (p, p, p, p), value=-math.inf)
    cols = F.unfold(xp, k, stride=s).view(n, c, k * k, ho * wo)             # taps in (ky, kx) order
    best = cols.max(2, keepdim=True).values
    is_max = cols == best
    first = is_max & (is_max.cumsum(2) == 1)                                 # the first tap holding the maximum
    assert (first.sum(2) == 1).all()
    idx = first.double().argmax(2)
    y = best.squeeze(2)
    if relu:
        y = y.clamp_min(0)
    d = dy.permute(0, 3, 1, 2).reshape(n, c, 1, ho * wo)
    if relu:
        d = d * (y > 0).unsqueeze(2)
    dx = F.fold((first * d).reshape(n, c * k * k, ho * wo), (h + 2 * p, w + 2 * p), k, stride=s)
    dx = dx[:, :, p:p + h, p:p + w]

    def nhwc(t):
        return t.view(n, c, ho, wo).permute(0, 2, 3, 1).contiguous()
    return nhwc(y), nhwc(idx).to(torch.uint8), dx.permute(0, 2, 3, 1).contiguous()


def _run_maxpool(gpu, x, dy, k, s, p, relu):
    xd = x.bfloat16().to(gpu).requires_grad_()
    y = OF.max_pool2d(xd, k, s, p, relu)
    y.backward(dy.bfloat16().to(gpu))
    _, idx = OF._C().maxpool_fwd(xd.detach(), k, s, p, relu)
    torch.cuda.synchronize()
    return y.detach().cpu(), idx.cpu(), xd.grad.cpu()


def _where(got, want):
    bad = (got.double() != want.double()).nonzero()
    n, i, j, c = bad[0].tolist()
    return (f"{len(bad)} of {want.numel()} differ -- first (image {n}, y {i}, x {j}, channel {c}): got "
            f"{got[n, i, j, c].item()!r} want {want[n, i, j, c].item()!r}")


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("k,s,p", [(3, 2, 1), (2, 2, 0), (3, 1, 1)])
@pytest.mark.parametrize("c", [16, 64, 10])
@pytest.mark.parametrize("h,w", [(12, 12), (7, 9)])
def test_maxpool_exact(gpu, h, w, c, k, s, p, relu):
    g = torch.Generator().manual_seed(1000 * h + 10 * c + k + s + p)
    x = _ints(g, (3, h, w, c))
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    dy = _ints(g, (3, ho, wo, c))
    ry, ridx, rdx = maxpool_reference(x, dy, k, s, p, relu)
    y, idx, dx = _run_maxpool(gpu, x, dy, k, s, p, relu)
    assert torch.equal(y, ry.bfloat16()), "y: " + _where(y, ry)
    assert torch.equal(idx, ridx), "argmax: " + _where(idx, ridx)
    assert torch.equal(dx, rdx.bfloat16()), "dx: " + _where(dx, rdx)
    # the data has what the test is for: ties in most windows, exact zeros under relu
    xp = F.pad(x.permute(0, 3, 1, 2), (p, p, p, p), value=-math.inf)
    cols = F.unfold(xp, k, stride=s).view(3, c, k * k, -1)
    assert ((cols == cols.max(2, keepdim=True).values).sum(2) > 1).double().mean().item() > 0.2
    assert not relu or (ry == 0).any()


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("k,s,p", [(3, 2, 1), (2, 2, 0), (3, 1, 1)])
@pytest.mark.parametrize("h,w", [(12, 12), (7, 9)])
def test_maxpool_vector_and_scalar_kernels_agree(gpu, h, w, k, s, p, relu):
    """C = 16 takes the 8-channel kernels, the same tensor padded to C = 17 the scalar ones: same y, argmax, dx."""
    g = torch.Generator().manual_seed(77 + h + k + s)
    x = _ints(g, (3, h, w, 16))
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    dy = _ints(g, (3, ho, wo, 16))
    a = _run_maxpool(gpu, x, dy, k, s, p, relu)
    b = _run_maxpool(gpu, torch.cat([x, _ints(g, (3, h, w, 1))], -1), torch.cat([dy, _ints(g, (3, ho, wo, 1))], -1),
                     k, s, p, relu)
    for name, u, v in zip(("y", "argmax", "dx"), a, b):
        assert torch.equal(u, v[..., :16].contiguous()), f"{name}: " + _where(u, v[..., :16])


# ---- global average pooling -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("c", [8, 200])
@pytest.mark.parametrize("h,w", [(1, 1), (4, 4), (7, 7)])
def test_avgpool_exact(gpu, h, w, c):
    hw = h * w
    g = torch.Generator().manual_seed(hw + c)
    x = torch.randn(5, h, w, c, generator=g).bfloat16()
    dy = torch.randn(5, c, generator=g).bfloat16()
    xd = x.to(gpu).requires_grad_()
    y = OF.global_avg_pool_flat(xd)
    y.backward(dy.to(gpu))
    torch.cuda.synchronize()
    ref = x.double().mean((1, 2))
    err = (y.detach().cpu().double() - ref).abs()
    bound = BF * ref.abs() + hw * U * x.double().abs().mean((1, 2))
    print("avgpool forward: worst fraction of the bound", (err / bound).max().item())
    assert (err <= bound).all(), (int((err > bound).sum()), (err > bound).nonzero()[0].tolist())
    inv = torch.tensor(1.0, dtype=torch.float32) / hw
    want = (dy.float() * inv).bfloat16().view(5, 1, 1, c).expand(5, h, w, c)
    assert torch.equal(xd.grad.cpu(), want), _where(xd.grad.cpu(), want)


def test_avgpool_integers_exact(gpu):
    g = torch.Generator().manual_seed(16)
    x = _ints(g, (5, 4, 4, 200))
    y = OF.global_avg_pool_flat(x.bfloat16().to(gpu))
    ref = x.mean((1, 2))   # a multiple of 1/16 below 4: six significant bits
    assert torch.equal(ref.bfloat16().double(), ref)
    assert torch.equal(y.cpu(), ref.bfloat16())


# ---- dropout ----------------------------------------------------------------------------------------------------------


def _nonzero_randn(g, shape):
    x = torch.randn(shape, generator=g)
    return (torch.sign(x) + (x == 0)) * x.abs().clamp_min(2.0 ** -10)   # a kept output is never zero


def _scale(p):
    one = torch.tensor(1.0, dtype=torch.float32)
    return one / (one - torch.tensor(p, dtype=torch.float32))


def _five_sigma(keep, draws, p):
    mean, sigma = draws * (1 - p), math.sqrt(draws * p * (1 - p))
    assert abs(keep - mean) <= 5 * sigma, (keep, draws, p)


ELEMENT_SHAPES = [(1,), (255,), (257,), (3, 5, 5, 10)]
CHANNEL_SHAPES = [(1, 1, 1, 1), (1, 5, 17, 3), (1, 1, 257, 1), (3, 5, 5, 10)]   # 1, 255, 257 and 750 elements


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("channel,shape", [(False, s) for s in ELEMENT_SHAPES] + [(True, s) for s in CHANNEL_SHAPES],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("channel" if v else "element"))
def test_dropout_exact(gpu, channel, shape, p):
    g = torch.Generator().manual_seed(len(shape) * 1000 + shape[-1] + int(p * 10))
    x, dy = _nonzero_randn(g, shape).bfloat16(), _nonzero_randn(g, shape).bfloat16()
    xd = x.to(gpu).requires_grad_()
    y = OF.dropout(xd, p, True, channel=channel)
    assert y is not xd and y.dtype == torch.bfloat16
    y.backward(dy.to(gpu))
    torch.cuda.synchronize()
    y, dx = y.detach().cpu(), xd.grad.cpu()
    keep = y != 0
    sc = _scale(p)
    zero = torch.zeros((), dtype=torch.bfloat16)
    assert torch.equal(y, torch.where(keep, (x.float() * sc).bfloat16(), zero))
    assert torch.equal(dx, torch.where(keep, (dy.float() * sc).bfloat16(), zero))
    # The 5-sigma window is as wide as these few draws make it.  At 1 draw it admits both outcomes, so it
    # cannot fail there; channel mode has 1, 3, 1 and 30 draws; at 255 draws and p = 0.1 it is 206..253 kept.  At
    # these sizes it rejects only gross mistakes (everything kept or dropped, p and 1 - p exchanged); the keep RATE is held
    # by test_dropout_keep_rate_on_many_draws.
    if channel:
        assert torch.equal(keep, keep[:, :1, :1, :].expand_as(keep))        # constant over H x W
        _five_sigma(int(keep[:, 0, 0, :].sum()), shape[0] * shape[-1], p)
    else:
        _five_sigma(int(keep.sum()), x.numel(), p)


def test_dropout_keep_rate_on_many_draws(gpu):
    """The 5-sigma window on enough draws to mean something, and p's rounding: 2^24-level uniforms against fp32 p."""
    x = torch.ones(1 << 20, device=gpu).bfloat16()
    for p in (0.1, 0.5, 0.9):
        _five_sigma(int((OF.dropout(x, p, True) != 0).sum()), 1 << 20, p)
        _five_sigma(int((OF.dropout(x.view(1 << 10, 1, 1, 1 << 10), p, True, channel=True) != 0).sum()), 1 << 20, p)


def test_dropout_channel_masks_differ(gpu):
    """Between the images of one call, between two calls, and between two replays of one captured graph."""
    x = torch.ones(4, 3, 3, 64, device=gpu).bfloat16()
    a = OF.dropout(x, 0.5, True, channel=True) != 0     # (also creates the device RNG counter before the capture)
    b = OF.dropout(x, 0.5, True, channel=True) != 0
    assert torch.equal(a, a[:, :1, :1, :].expand_as(a))
    for i in range(4):
        for j in range(i):
            assert not torch.equal(a[i], a[j]), (i, j)
    assert not torch.equal(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(graph):
        y = OF.dropout(x, 0.5, True, channel=True)
    torch.cuda.current_stream().wait_stream(s)
    masks = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        masks.append((y != 0).clone())
    assert torch.equal(masks[0], masks[0][:, :1, :1, :].expand_as(masks[0]))
    assert not torch.equal(masks[0], masks[1])
    kept = torch.where(masks[1], torch.full_like(y, 2.0), torch.zeros_like(y))
    assert torch.equal(y, kept)


def test_dropout_off_returns_the_input(gpu):
    x = torch.randn(3, 5, 5, 16, device=gpu).bfloat16()
    assert OF.dropout(x, 0.5, training=False) is x
    assert OF.dropout(x, 0.0, training=True) is x
    assert OF.dropout(x, 0.0, training=True, channel=True) is x
