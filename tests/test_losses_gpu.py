"""Every path of csrc/kernels/loss.hip against float64 ``torch.nn.functional`` on the CPU, given the same
already-rounded inputs (bf16 logits go in as ``.double()``).

Tolerances come from the output format, not from the kernel:
  loss value   relative 1e-5 (a one-block fp32 tree over at most a few thousand rows is far below that);
  fp32 dx      relative L2 1e-5;
  bf16 dx      per element |d - ref| <= 2^-8 |ref| (one bf16 ulp) + 1e-5 * scale, the fp32 term, where ``scale``
               is the magnitude of the operands before they cancel: g / B for (softmax - onehot) g / B,
               |dy| + softmax |sum dy| for the log_softmax backward, |ref| itself for MSE.
The fused / unfused cross-entropy pair is held to twice these bounds against each other (each side once).

(2^-8 |ref| is also the largest error round-to-nearest can make, just above a power of two: the bf16 bound has
no slack for a truncating or double-rounding conversion.)

Measured on an MI355X (worst case of each group; loss relative error | fp32 dx relative L2 | bf16 dx worst
|d - ref| / bound):

  cross_entropy         1.2e-07 (300x10)        2.3e-07 (5x1000)     0.989 (2500x8)
  nll_loss              8.2e-08 (300x10)        4.4e-08 (2500x8)     0.755 (5x1000)
  ce, logits ~ 80+-30   7.4e-08 (37x64)         2.1e-06 (37x64)
  ce, row of -1e4       3.6e-08                 1.1e-07
  log_softmax           5.9e-08 (y, rel L2)     6.0e-07 (5x1000)     0.994 (259x1000)
  mse_loss              5.9e-08 (n = 1)         5.6e-08 (n = 8193)   0.989 (n = 8192)
  ce_fused              9.4e-08 (1500x10)                            0.988 (1500x16)
  ce_fwd + ce_bwd       9.4e-08 (1500x10)                            0.988 (1500x16)

``__expf`` / ``__logf`` stay two orders of magnitude inside the loss and fp32 bounds.
"""
import zlib

import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_examples_amd.ops import functional as OF

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5
DX_L2 = 1e-5
BF16_ULP = 2.0 ** -8
DTYPES = [torch.float32, torch.bfloat16]
IDS = {torch.float32: "fp32", torch.bfloat16: "bf16"}


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def make_targets(gen, B, V):
    """Unique targets where B <= V (an off-by-one in the one-hot then lands on another row's class)."""
    if B <= V:
        return torch.randperm(V, generator=gen)[:B]
    return torch.randint(0, V, (B,), generator=gen)


def check_loss(tag, loss, ref):
    got, want = float(loss.item()), float(ref.item())
    err = abs(got - want) / abs(want)
    print(f"LOSS_ERR {tag} loss: rel {err:.2e} (ref {want:.6g})")
    assert got == got and abs(got) != float("inf"), f"{tag}: loss {got}"
    assert err <= LOSS_RTOL, f"{tag}: loss {got!r} vs {want!r}, relative error {err:.3e}"


def check_dx(tag, dx, ref, scale, want_dtype):
    """``ref`` float64; ``scale``: float64 tensor or number, the uncancelled operand magnitude (module docstring)."""
    assert dx.dtype == want_dtype and dx.shape == ref.shape, (dx.dtype, dx.shape)
    d = dx.detach().cpu().double()
    assert torch.isfinite(d).all(), f"{tag}: non-finite gradient"
    if want_dtype == torch.float32:
        err = ((d - ref).norm() / ref.norm()).item()
        print(f"LOSS_ERR {tag} dx fp32: rel l2 {err:.2e}")
        assert err <= DX_L2, f"{tag}: fp32 dx relative L2 error {err:.3e}"
    else:
        bound = BF16_ULP * ref.abs() + 1e-5 * scale
        ratio = ((d - ref).abs() / bound).max().item()
        print(f"LOSS_ERR {tag} dx bf16: worst |d - ref| / bound {ratio:.3f}")
        assert ratio <= 1.0, f"{tag}: a bf16 dx element is {ratio:.3f}x its bound"


def ce_case(gpu, tag, x_cpu, tgt, mode, gup):
    """cross_entropy (mode 0) / nll_loss (mode 1) forward, determinism and backward on ``x_cpu`` (fp32 or bf16)."""
    fn, ref_fn = ((OF.cross_entropy, F.cross_entropy), (OF.nll_loss, F.nll_loss))[mode]
    x = x_cpu.to(gpu).requires_grad_()
    t = tgt.to(gpu)
    loss = fn(x, t)
    x64 = x_cpu.detach().double().requires_grad_()
    ref = ref_fn(x64, tgt)
    check_loss(tag, loss, ref)
    assert torch.equal(loss.detach(), fn(x.detach(), t)), f"{tag}: loss differs between two launches"
    (loss * gup).backward()
    (ref * gup).backward()
    check_dx(tag, x.grad, x64.grad, abs(gup) / x_cpu.shape[0], x_cpu.dtype)


CE_SHAPES = [(1, 10), (300, 10), (1025, 10), (2500, 8), (64, 17), (37, 64), (33, 65), (5, 1000)]


@pytest.mark.parametrize("gup", [1.0, 0.37])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("B,V", CE_SHAPES)
def test_cross_entropy(gpu, B, V, dtype, gup):
    gen = _gen("ce", B, V)
    x = (torch.randn(B, V, generator=gen) * 3).to(dtype)
    ce_case(gpu, f"ce {B}x{V} {IDS[dtype]} g{gup}", x, make_targets(gen, B, V), 0, gup)


@pytest.mark.parametrize("gup", [1.0, 0.37])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("B,V", CE_SHAPES)
def test_nll_loss(gpu, B, V, dtype, gup):
    gen = _gen("nll", B, V)
    lp = F.log_softmax(torch.randn(B, V, generator=gen) * 3, 1).to(dtype)
    ce_case(gpu, f"nll {B}x{V} {IDS[dtype]} g{gup}", lp, make_targets(gen, B, V), 1, gup)


@pytest.mark.parametrize("B,V", [(300, 10), (37, 64)])
def test_cross_entropy_large_logits(gpu, B, V):
    """exp() of these logits overflows fp32 unless the row maximum is subtracted first."""
    gen = _gen("ce-large", B, V)
    x = torch.randn(B, V, generator=gen) * 30 + 80
    ce_case(gpu, f"ce-large {B}x{V}", x, make_targets(gen, B, V), 0, 1.0)


def test_cross_entropy_row_of_minus_1e4(gpu):
    """One row whose non-target entries are all -1e4: its softmax is the one-hot exactly, loss and gradient
    stay finite."""
    gen = _gen("ce-1e4")
    B, V = 64, 10
    x = torch.randn(B, V, generator=gen) * 3
    tgt = make_targets(gen, B, V)
    keep = x[5, tgt[5]].clone()
    x[5] = -1e4
    x[5, tgt[5]] = keep
    ce_case(gpu, "ce-1e4", x, tgt, 0, 1.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("B", [1, 5, 259])
@pytest.mark.parametrize("V", [10, 64, 65, 130, 1000])
def test_log_softmax(gpu, V, B, dtype):
    """Thread-per-row (V <= 64) and wave-per-row forward; backward with a random dy, fp32 dx for fp32 input and
    bf16 dx for bf16 input."""
    gen = _gen("lsm", B, V)
    x_cpu = (torch.randn(B, V, generator=gen) * 3).to(dtype)
    dy = torch.randn(B, V, generator=gen)
    x = x_cpu.to(gpu).requires_grad_()
    y = OF.log_softmax(x)
    x64 = x_cpu.detach().double().requires_grad_()
    y64 = F.log_softmax(x64, 1)
    tag = f"log_softmax {B}x{V} {IDS[dtype]}"
    assert y.dtype == torch.float32
    err = ((y.detach().cpu().double() - y64.detach()).norm() / y64.detach().norm()).item()
    print(f"LOSS_ERR {tag} y: rel l2 {err:.2e}")
    assert err <= DX_L2, f"{tag}: forward relative L2 error {err:.3e}"
    assert torch.equal(y.detach(), OF.log_softmax(x.detach()))
    y.backward(dy.to(gpu))
    y64.backward(dy.double())
    scale = dy.double().abs() + y64.detach().exp() * dy.double().sum(1, keepdim=True).abs()
    check_dx(tag, x.grad, x64.grad, scale, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("shape", [(1,), (1023,), (8191,), (8192,), (8193,), (32, 1000)], ids=str)
def test_mse_loss(gpu, shape, dtype):
    """8 x 1024 elements per unrolled trip of the one block: below, at and past one trip, and the ResNet shape."""
    gen = _gen("mse", *shape)
    p_cpu = torch.randn(*shape, generator=gen).to(dtype)
    t_cpu = torch.randn(*shape, generator=gen)
    p = p_cpu.to(gpu).requires_grad_()
    t = t_cpu.to(gpu)
    loss = OF.mse_loss(p, t)
    p64 = p_cpu.detach().double().requires_grad_()
    ref = F.mse_loss(p64, t_cpu.double())
    tag = f"mse {tuple(shape)} {IDS[dtype]}"
    check_loss(tag, loss, ref)
    assert torch.equal(loss.detach(), OF.mse_loss(p.detach(), t)), f"{tag}: loss differs between two launches"
    (loss * 0.37).backward()
    (ref * 0.37).backward()
    check_dx(tag, p.grad, p64.grad, p64.grad.abs(), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("B", [1, 128, 1500])
@pytest.mark.parametrize("V", [8, 10, 16, 17, 40])
def test_ce_fused(gpu, V, B, dtype):
    """Loss and bf16 d logits in one launch: the row-in-registers path (V <= 16) and the general one; a strided
    ``dx_out`` keeps its padding columns; the result agrees with ce_fwd + ce_bwd."""
    C = OF._C()
    gen = _gen("fused", B, V)
    x_cpu = (torch.randn(B, V, generator=gen) * 3).to(dtype)
    tgt = make_targets(gen, B, V)
    x, t = x_cpu.to(gpu), tgt.to(gpu)
    x64 = x_cpu.detach().double().requires_grad_()
    ref = F.cross_entropy(x64, tgt)
    ref.backward()
    dref = x64.grad
    tag = f"ce_fused {B}x{V} {IDS[dtype]}"

    loss, dx = C.ce_fused(x, t)
    check_loss(tag, loss, ref)
    check_dx(tag, dx, dref, 1.0 / B, torch.bfloat16)
    assert torch.equal(loss, C.ce_fused(x, t)[0]), f"{tag}: loss differs between two launches"

    # a [B, V] view of a wider buffer: the columns past V are not the kernel's to write
    ld = 24 if V <= 16 else 48
    sentinel = torch.full((B, ld), -7.0, dtype=torch.bfloat16, device=gpu)
    buf = sentinel.clone()
    loss_v, dx_v = C.ce_fused(x, t, buf[:, :V])
    assert torch.equal(loss_v, loss) and torch.equal(buf[:, :V], dx) and dx_v.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[:, V:].view(torch.int16), sentinel[:, V:].view(torch.int16)), f"{tag}: padding written"

    # ce_fwd + ce_bwd on the same input: within the same bounds, and within twice them of the fused result
    loss2, lse = C.ce_fwd(x, t, 0)
    dx2 = C.ce_bwd(x, t, lse, torch.ones(1, device=gpu), 0, False)
    check_loss(tag + " unfused", loss2, ref)
    check_dx(tag + " unfused", dx2, dref, 1.0 / B, torch.bfloat16)
    assert abs(loss.item() - loss2.item()) <= 2 * LOSS_RTOL * abs(ref.item())
    bound = 2 * (BF16_ULP * dref.abs() + 1e-5 / B)
    assert ((dx.double() - dx2.double()).abs().cpu() <= bound).all(), f"{tag}: fused and unfused dx disagree"


@pytest.mark.parametrize("op", ["ce_fwd", "ce_bwd", "ce_fused", "log_softmax_fwd", "mse_fwd", "mse_bwd"])
def test_fp16_input_is_refused(gpu, op):
    """The kernels read fp32 or bf16 through one flag: any other dtype would be read as bf16."""
    C = OF._C()
    x = torch.randn(4, 10, device=gpu).half()
    t = torch.randint(0, 10, (4,), device=gpu)
    one = torch.ones(1, device=gpu)
    calls = {
        "ce_fwd": lambda: C.ce_fwd(x, t, 0),
        "ce_bwd": lambda: C.ce_bwd(x, t, torch.zeros(4, device=gpu), one, 0, True),
        "ce_fused": lambda: C.ce_fused(x, t),
        "log_softmax_fwd": lambda: C.log_softmax_fwd(x),
        "mse_fwd": lambda: C.mse_fwd(x, torch.zeros(4, 10, device=gpu)),
        "mse_bwd": lambda: C.mse_bwd(x, torch.zeros(4, 10, device=gpu), one, True),
    }
    with pytest.raises(RuntimeError, match="fp32 or bf16"):
        calls[op]()
