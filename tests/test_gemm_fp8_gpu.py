"""The FP8 path (csrc/kernels/gemm_fp8.hip): k_gemm_fp8 exact on integer operands in all three roles, k_fp8_quant and
k_fp8_scales against torch's float8 casts, and one FusedMLP(precision="fp8") step against a float64 emulation."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# test_step_matches_emulation: four times the largest figure seen on an MI355X over seeds 0, 1, 2 and both batches
# (profiles/fp8_linear.md holds every figure); a tie of the fp32 sum can quantise one FP8 step off the float64 one.
# The smallest distance between the emulation and the unquantised float64 gradient was 5.35e-2 (checked in the test).
BOUND = 4 * 3.411e-3  # max over tensors of |g - g_ref| / |g_ref|
LOSS_BOUND = 4 * 4.5e-6  # |loss - loss_ref| / loss_ref


def _fp8():
    from pytorch_distributed_examples_amd import _native
    from pytorch_distributed_examples_amd.ops import fp8

    return _native.C(), fp8


def _rule_scale(fmax, amax):
    return 2.0 ** (math.frexp(torch.tensor(fmax / amax, dtype=torch.float32).item())[1] - 1)


# (520, 1024, 256): 144 tiles of 64 x 64, so the 64-row tile (from 128 tiles up), with M off it; the others run the 32-row one
@pytest.mark.parametrize("M,N,K", [(16, 16, 128), (80, 48, 384), (128, 1024, 784), (32, 10, 1024), (520, 1024, 256)])
@pytest.mark.parametrize("role", ["fwd", "dgrad", "wgrad"])
def test_gemm_exact(gpu, role, M, N, K):
    """Integer operands every format holds exactly (|v| <= 16 in e4m3, <= 8 in e5m2), unit scales: every fp32 partial
    sum is an integer below 2^24, so the output equals the float64 product bit for bit.  Operands reach the GEMM in
    their role's layout: dgrad reads the quantiser's transposed weight copy, wgrad both transposed copies."""
    C, fp8 = _fp8()
    g = torch.Generator().manual_seed(M + N + K)
    fa = fp8.E4M3 if role == "fwd" else fp8.E5M2
    a = torch.randint(-8 if fa else -16, (8 if fa else 16) + 1, (M, K), generator=g).float()
    b = torch.randint(-16, 17, (N, K), generator=g).float()
    rec = fp8.ScaleRecords([fa, fp8.E4M3], gpu)
    ops = []
    for x, fmt, transposed, r in ((a, fa, role == "wgrad", 0), (b, fp8.E4M3, role != "fwd", 1)):
        src = (x.T if transposed else x).contiguous().to(gpu)
        dst, dst_t = fp8.buffer(*src.shape, gpu), fp8.buffer(*src.shape[::-1], gpu)
        fp8.QuantPlan(rec, fmt, [src], [dst], [dst_t], [r]).run()
        ops.append(dst_t if transposed else dst)
    ref = a.double() @ b.double().T
    out = torch.full((M, N), float("nan"), device=gpu)
    if role != "wgrad":
        C.fp8_gemm(role, ops[0], ops[1], M, N, rec.t, 0, 1, out=out)
    else:
        gb = torch.full((M,), float("nan"), device=gpu)
        C.fp8_gemm(role, ops[0], ops[1], M, N, rec.t, 0, 1, out=out, gbias=gb)
        assert torch.equal(gb.cpu().double(), a.double().sum(1))
        C.fp8_gemm(role, ops[0], ops[1], M, N, rec.t, 0, 1, out=out, gbias=gb, accumulate=True)
        assert torch.equal(gb.cpu().double(), 2 * a.double().sum(1))
        ref = 2 * ref
    assert torch.equal(out.cpu().double(), ref)


@pytest.mark.parametrize("mag", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("shape", [(33, 784), (10, 1024)])
@pytest.mark.parametrize("fmt", [0, 1])
def test_quantiser(gpu, fmt, shape, mag):
    C, fp8 = _fp8()
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1)) * mag
    fmax, amax = fp8.FMT_MAX[fmt], x.abs().max().item()
    scale = _rule_scale(fmax, amax)
    rec = fp8.ScaleRecords([fmt], gpu)
    rec.t[0, :2] = torch.tensor([scale, 1.0 / scale])
    dst, dst_t = fp8.buffer(*shape, gpu), fp8.buffer(*shape[::-1], gpu)
    fp8.QuantPlan(rec, fmt, [x.to(gpu)], [dst], [dst_t], [0]).run()
    want = (x * scale).to(fp8.TORCH_DTYPE[fmt]).float()  # round to nearest even; never overflows at this scale
    rows, cols = shape
    assert torch.equal(fp8.decode(dst.cpu(), fmt)[:, :cols], want)
    assert torch.equal(fp8.decode(dst_t.cpu(), fmt)[:, :rows], want.T)
    assert not dst[:, cols:].any() and not dst_t[:, rows:].any()
    assert rec.t[0, 2].item() == amax
    rec.t[0, :2] = 1.0
    rec.update()
    assert rec.t[0].tolist() == [scale, 1.0 / scale, 0.0, fmax]


@pytest.mark.parametrize("fmt", [0, 1])
def test_quantiser_clamps(gpu, fmt):
    """Beyond max / scale the output is +-max, finite (torch's own e4m3 cast would give NaN)."""
    C, fp8 = _fp8()
    x = torch.tensor([[1e6, -1e6, 1.0, float("inf")]], device=gpu)
    rec = fp8.ScaleRecords([fmt], gpu)
    dst = fp8.buffer(1, 4, gpu)
    fp8.quantise(rec, fmt, x, dst, None, 0)
    with pytest.raises(RuntimeError, match="scale record"):
        fp8.quantise(rec, fmt, x, dst, None, 1)
    fmax = fp8.FMT_MAX[fmt]
    assert fp8.decode(dst.cpu(), fmt)[0, :4].tolist() == [fmax, -fmax, 1.0, fmax]
    rec.update()  # amax is not finite: the scale stays
    assert rec.t[0].tolist() == [1.0, 1.0, 0.0, fmax]


@pytest.mark.parametrize("M,N,K", [(50, 70, 256), (520, 1000, 128)])  # 32-row and 64-row tiles, M and N off both
@pytest.mark.parametrize("role", ["fwd", "dgrad"])
def test_quantising_epilogues(gpu, role, M, N, K):
    """Integer operands make the fp32 value in front of the quantiser exact, so both copies must decode to torch's
    round-to-nearest-even cast of relu(C + bias) * scale (forward) or C * mask * scale (dgrad), the padding of both
    must be zero bytes, rows past M / N must stay untouched, and amax is the exact maximum."""
    C, fp8 = _fp8()
    g = torch.Generator().manual_seed(M + K)
    fa = fp8.E4M3 if role == "fwd" else fp8.E5M2
    a = torch.randint(-8 if fa else -16, (8 if fa else 16) + 1, (M, K), generator=g).float()
    b = torch.randint(-16, 17, (N, K), generator=g).float()
    A, Bq = fp8.buffer(M, K, gpu), fp8.buffer(N, K, gpu)
    A[:, :K] = a.to(fp8.TORCH_DTYPE[fa]).view(torch.uint8).to(gpu)
    Bq[:, :K] = b.to(fp8.TORCH_DTYPE[fp8.E4M3]).view(torch.uint8).to(gpu)
    scale = 2.0 ** -8 if role == "fwd" else 0.25  # |C| <= 16 * 16 * 256 and 8 * 16 * 256: inside both formats
    rec = fp8.ScaleRecords([fa, fp8.E4M3, fa], gpu)
    rec.t[2, :2] = torch.tensor([scale, 1.0 / scale])
    y = a.double() @ b.double().T
    if role == "fwd":
        bias = torch.randint(-50, 51, (N,), generator=g).float()
        y, extra = torch.relu(y + bias.double()), dict(bias=bias.to(gpu))
    else:
        kind = torch.randint(0, 3, (M, N), generator=g)  # the producer's activation byte: +0, -0 or 1.0
        mask = fp8.buffer(M, N, gpu)
        mask[:, :N] = torch.tensor([0x00, 0x80, 0x38], dtype=torch.uint8)[kind].to(gpu)
        y, extra = y * (kind == 2), dict(mask=mask)
    want = (y * scale).float().to(fp8.TORCH_DTYPE[fa]).float()
    q, qt = fp8.buffer(M + 4, N, gpu), fp8.buffer(N + 4, M, gpu)
    q[M:], qt[N:] = 0xFF, 0xFF
    C.fp8_gemm(role, A, Bq, M, N, rec.t, 0, 1, q=q, qt=qt, rec_out=2, **extra)
    assert torch.equal(fp8.decode(q.cpu(), fa)[:M, :N], want)
    assert torch.equal(fp8.decode(qt.cpu(), fa)[:N, :M], want.T)
    assert not q[:M, N:].any() and not qt[:N, M:].any()
    assert (q[M:] == 0xFF).all() and (qt[N:] == 0xFF).all()
    assert rec.t[2, 2].item() == y.abs().max().item()


def _reference_step(ws, bs, x, y, s, quant):
    """One step in float64; with `quant`, cast through torch.float8_* where the kernels quantise, with scales s
    (e4m3 inputs, weights and activations; bf16 then e5m2 d logits; e5m2 data gradients).  Returns (loss, grads)."""
    def q(t, sc, dt, fmax):
        return ((t * sc).clamp(-fmax, fmax).float().to(dt).double() / sc) if quant else t

    e4, e5 = (torch.float8_e4m3fn, 448.0), (torch.float8_e5m2, 57344.0)
    n = len(ws)
    wq = [q(w.double(), s["weight"][i], *e4) for i, w in enumerate(ws)]
    h = [q(x.double(), s["act"][0], *e4)]
    for i in range(n - 1):
        h.append(q(torch.relu(h[i] @ wq[i].T + bs[i].double()), s["act"][i + 1], *e4))
    logits = h[-1] @ wq[-1].T + bs[-1].double()
    loss = torch.nn.functional.cross_entropy(logits, y)
    d = (torch.softmax(logits, 1) - torch.nn.functional.one_hot(y, logits.shape[1])) / len(y)
    d = q(d.float().to(torch.bfloat16).double() if quant else d, s["grad"][-1], *e5)
    grads = [None] * n
    for i in range(n - 1, -1, -1):
        grads[i] = (d.T @ h[i], d.sum(0))
        if i > 0:
            d = q((d @ wq[i]) * (h[i] != 0), s["grad"][i - 1], *e5)
    return loss.item(), [t for pair in grads for t in pair]


@pytest.mark.parametrize("batch", [32, 160])
def test_step_matches_emulation(gpu, batch):
    from pytorch_distributed_examples_amd.models.mlp import MLP
    from pytorch_distributed_examples_amd.models.mlp_fused import FusedMLP

    for seed in range(3):
        torch.manual_seed(seed)
        net = MLP(1, 64).to(gpu)
        x, y = torch.randn(batch, 784, device=gpu), torch.randint(0, 10, (batch,), device=gpu)
        fm = FusedMLP(net, precision="fp8")
        fm.calibrate(x, y)
        s = fm.fp8_scales()
        loss = fm.forward_backward(x, y).item()
        params = [p for L in fm.layers for p in (L.weight, L.bias)]
        ws, bs = [p.detach().cpu() for p in params[0::2]], [p.detach().cpu() for p in params[1::2]]
        ref_loss, ref = _reference_step(ws, bs, x.cpu(), y.cpu(), s, True)
        _, exact = _reference_step(ws, bs, x.cpu(), y.cpu(), s, False)
        err = [((p.grad.cpu().double() - r).norm() / r.norm()).item() for p, r in zip(params, ref)]
        noise = [((e - r).norm() / r.norm()).item() for e, r in zip(exact, ref)]
        dloss = abs(loss - ref_loss) / ref_loss
        print(f"batch {batch} seed {seed}: loss rel {dloss:.2e}  err {max(err):.3e}  noise min {min(noise):.3e}")
        assert dloss <= LOSS_BOUND
        assert max(err) <= BOUND < 0.5 * min(noise), (err, noise)
    # the default precision is untouched: same gradients, bit for bit, with and without the argument
    grads = []
    for fm in (FusedMLP(net), FusedMLP(net, precision="bf16")):
        fm.forward_backward(x, y)
        grads.append([p.grad.clone() for p in params])
    assert all(torch.equal(a, b) for a, b in zip(*grads))
