"""hvd.Adasum on the GPU: the weights function the combine kernel runs, the two xGMI kernels (csrc/comm/
xgmi_allreduce.hip: Gram pass + weights and combine) rehearsed with 2 and 4 processes sharing ONE card, and the hvd
API on that plane at 2 ranks (engine, graph-mode inline call, DistributedOptimizer's deltas, the MNIST example).

Device results are compared elementwise with the fp64 tree (hvd/adasum.py) under the derived bound of
tests/adasum_fixture.py::bound -- on correlated inputs whose tree is far from both their sum and their average."""
import os
import re
import subprocess
import sys
import tempfile

import pytest
import torch

from adasum_fixture import rank_data

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n_ranks", [2, 4, 8])
def test_adasum_weights_binding(gpu, n_ranks):
    """The host side of the shared host/device function against the Python one -- the N = 8 tree without eight
    processes -- including a rank whose norm is zero.  fp64 on both sides: a few hundred operations, 1e-12."""
    from pytorch_distributed_examples_amd import _native
    from pytorch_distributed_examples_amd.hvd import adasum

    C = _native.comm()
    for zero in (None, 0, n_ranks - 1):
        X = torch.stack([rank_data(r, 500, 40 + n_ranks).double() for r in range(n_ranks)])
        if zero is not None:
            X[zero] = 0
        G = X @ X.T
        w = C.adasum_weights(G)
        want = adasum.adasum_weights(G)
        assert w.dtype == torch.float64 and torch.allclose(w, want, rtol=1e-12, atol=0), (zero, w, want)
        assert torch.allclose((w[:, None] * X).sum(0), adasum.adasum_tree(list(X)), rtol=1e-11, atol=1e-13)
    with pytest.raises(RuntimeError):
        C.adasum_weights(torch.eye(3, dtype=torch.float64))


def test_adasum_world1_is_the_scale(gpu):
    from pytorch_distributed_examples_amd import _native

    C = _native.comm()
    xa = C.XgmiAllreduce(0, 1, gpu.index, 1 << 20)
    t = torch.arange(1000, dtype=torch.float32, device=gpu)
    xa.adasum_(t, [250, 750], 0.5)
    torch.cuda.synchronize()
    assert torch.equal(t.cpu(), torch.arange(1000, dtype=torch.float32) * 0.5)
    with pytest.raises(Exception):
        xa.adasum_(t, [250, 700], 1.0)  # the segments must cover the tensor
    assert xa.error() == 0
    xa.close()


_REHEARSAL = r"""
import os, sys, time, torch, torch.distributed as dist
sys.path.insert(0, os.environ["REPO"]); sys.path.insert(0, os.path.join(os.environ["REPO"], "tests"))
from adasum_fixture import CNN_SEGS, assert_not_sum_or_average, bound, rank_data, reference
from pytorch_distributed_examples_amd.parallel import dist as pdist
from pytorch_distributed_examples_amd.parallel.xgmi_allreduce import XgmiAllreduce
ctx = pdist.init_distributed()          # PDE_BACKEND=gloo: several ranks on one GPU
N, r, dev = ctx.world_size, ctx.rank, ctx.device
xa = XgmiAllreduce(dev, max_bytes=4 << 20, blocks=8, timeout_s=20.0)
_cache = {}

def case(segs, seed):
    # inputs, fp64 reference and bound of one case: computed once, shared by the checks below
    key = (tuple(segs), seed)
    if key not in _cache:
        n = sum(segs)
        xs = [rank_data(k, n, seed) for k in range(N)]
        ref = reference(xs, segs)
        assert_not_sum_or_average(xs, ref)
        _cache[key] = (xs, ref, bound(xs, segs))
    return _cache[key]

def within(out, ref, bnd, what):
    err = (out.double() - ref).abs()
    worst = float((err / bnd).max())
    print("ADASUM_RATIO", what, N, f"{worst:.3f}", flush=True)
    assert torch.isfinite(out).all() and worst <= 1.0, (what, worst)

def same_on_all_ranks(out, what):
    outs = [torch.empty_like(out) for _ in range(N)]
    dist.all_gather(outs, out)
    assert all(torch.equal(o, outs[0]) for o in outs), what

def run(x, segs, offset=0, scale=1.0):
    buf = torch.empty(x.numel() + offset, device=dev)
    t = buf[offset:]
    t.copy_(x)
    xa.adasum_(t, segs, scale)
    torch.cuda.synchronize()
    return t.cpu()

LISTS = [([1], 0), ([7], 0), ([10, 20, 50, 10], 0), (CNN_SEGS, 0), ([262144], 0), (CNN_SEGS, 1)]
for li, (segs, offset) in enumerate(LISTS):
    what = f"list{li}"
    n = sum(segs)
    xs, ref, bnd = case(segs, 61 + li)
    out = run(xs[r], segs, offset)
    within(out, ref, bnd, what)
    same_on_all_ranks(out, what)
    # disjoint supports: every dot product is exactly zero, every coefficient exactly 1 -- the sum, exactly
    ys = [torch.where(torch.arange(n) % N == k, xs[k], torch.zeros(n)) for k in range(N)]
    out = run(ys[r], segs, offset)
    assert torch.equal(out, sum(ys)), what
    # a rank with a zero gradient: no NaN, and the tree of the others
    zs = list(xs); zs[N - 1] = torch.zeros(n)
    out = run(zs[r], segs, offset)
    within(out, reference(zs, segs), bound(zs, segs), what + ".zero")
    same_on_all_ranks(out, what + ".zero")
# the scale is applied once, at the end
xs, ref, bnd = case(CNN_SEGS, 61 + 3)
within(run(xs[r], CNN_SEGS, 0, 0.25), 0.25 * ref, 0.25 * bnd, "scale")   # (a power of two: the product is exact)
# a sum, an Adasum and a sum on one instance with no host sync in between: epochs and slot parity
a = rank_data(r, 21840, 71).to(dev); b = xs[r].to(dev); c = rank_data(r, 7000, 72).to(dev)
xa.allreduce_(a); xa.adasum_(b, CNN_SEGS); xa.allreduce_(c)
torch.cuda.synchronize()
assert torch.allclose(a.cpu(), sum(rank_data(k, 21840, 71) for k in range(N)), rtol=1e-5, atol=1e-5)
within(b.cpu(), ref, bnd, "mixed")
assert torch.allclose(c.cpu(), sum(rank_data(k, 7000, 72) for k in range(N)), rtol=1e-5, atol=1e-5)
# three captured calls (different sizes: grids of 8, 8 and 1 workgroups), replayed three times on fresh inputs
shapes = [CNN_SEGS, [262144], [7]]
ts = [torch.zeros(sum(s), device=dev) for s in shapes]
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g):
    for t, s in zip(ts, shapes):
        xa.adasum_(t, s)
for rep in range(3):
    # (seven elements are few: with some seeds their tree lies within 10 % of the average, which `case` refuses;
    # seeds 62 and 72-74 do not)
    cases = [case(s, 72 + rep if s == [7] else 80 + 3 * rep + i) for i, s in enumerate(shapes)]
    for t, cs in zip(ts, cases):
        t.copy_(cs[0][r])
    g.replay()
    torch.cuda.synchronize()
    for i, (t, cs) in enumerate(zip(ts, cases)):
        within(t.cpu(), cs[1], cs[2], f"graph{rep}.{i}")
        same_on_all_ranks(t.cpu(), f"graph{rep}.{i}")
# a late peer: the others spin (bounded) until it arrives
if r == N - 1:
    time.sleep(0.3)
within(run(xs[r], CNN_SEGS), ref, bnd, "late")
xa.check()
# a two-shot instance refuses
x2 = XgmiAllreduce(dev, max_bytes=1 << 20, blocks=8, two_shot=True)
try:
    x2.adasum_(torch.zeros(8, device=dev))
    raise AssertionError("a two-shot instance ran Adasum")
except RuntimeError:
    pass
dist.barrier()
x2.close(); xa.close()
dist.destroy_process_group()
print("ADASUM_OK", r)
"""

_HVD = r"""
import os, sys, torch
sys.path.insert(0, os.environ["REPO"]); sys.path.insert(0, os.path.join(os.environ["REPO"], "tests"))
from adasum_fixture import assert_not_sum_or_average, bound, rank_data, reference
from pytorch_distributed_examples_amd import hvd
from pytorch_distributed_examples_amd.hvd import adasum
os.environ["PDE_HVD_DATA_PLANE"] = "xgmi"
os.environ["HOROVOD_CYCLE_TIME"] = "20"   # ms: the enqueues of one burst land in one negotiation cycle
hvd.init()
N, r = hvd.size(), hvd.rank()
dev = torch.device("cuda", torch.cuda.current_device())

def within(out, ref, bnd, what):
    worst = float(((out.double() - ref).abs() / bnd).max())
    print("ADASUM_RATIO", what, f"{worst:.3f}", flush=True)
    assert torch.isfinite(out).all() and worst <= 1.0, (what, worst)

# named tensors fused by the engine, with different correlations: per-tensor coefficients
sizes, noises = [300, 41, 7000], [0.1, 0.5, 2.0]
ts = [[rank_data(k, n, 20 + i, noise=z) for i, (n, z) in enumerate(zip(sizes, noises))] for k in range(N)]
fused = [torch.cat(t) for t in ts]
ref, bnd = reference(fused, sizes), bound(fused, sizes)
assert_not_sum_or_average(fused, ref)
assert float((ref - reference(fused, [sum(sizes)])).norm() / ref.norm()) > 0.05
mine = [t.to(dev) for t in ts[r]]
before = hvd.engine_stats()
hs = [hvd.allreduce_async_(t, name=f"f{i}", op=hvd.Adasum) for i, t in enumerate(mine)]
for h in hs:
    hvd.synchronize(h)
torch.cuda.synchronize()
st = hvd.engine_stats()
assert st["xgmi_batches"] > before["xgmi_batches"] and st["fused_requests"] >= before["fused_requests"] + 2, st
got = torch.cat([t.cpu() for t in mine])
within(got, ref, bnd, "engine")
every = hvd.allgather(got[None].to(dev)).cpu()
assert all(torch.equal(every[0], every[k]) for k in range(N))
# out of place, with scales
out = hvd.allreduce(ts[r][2].to(dev), op=hvd.Adasum, name="oop", prescale_factor=0.5, postscale_factor=4.0)
within(out.cpu(), 2.0 * ref[341:], 2.0 * bnd[341:], "scaled")   # (a power of two: the product is exact)
# the inline (graph-mode) call: same tensors, caller's stream, adjacent views reduced in place
flat = fused[r].to(dev)
views = list(flat.split(sizes))
hvd.core.set_graph_mode(True, views)
hvd.core.allreduce_inline_(views, op=hvd.Adasum)
torch.cuda.synchronize()
within(flat.cpu(), ref, bnd, "inline.span")
sep = [t.to(dev) for t in ts[r]]
hvd.core.allreduce_inline_(sep, op=hvd.Adasum)
torch.cuda.synchronize()
within(torch.cat([t.cpu() for t in sep]), ref, bnd, "inline.pack")
hvd.core.set_graph_mode(False)
hvd.core.check_health()
# what the exchange cannot take is an error, never a sum
for bad, kw in ((torch.zeros(8, device=dev, dtype=torch.float64), {}),
                (torch.zeros(hvd.core._ctx.xgmi.max_bytes // 4 + 4, device=dev), {})):
    try:
        hvd.allreduce_(bad, op=hvd.Adasum, **kw)
        raise AssertionError("accepted")
    except ValueError:
        pass

# DistributedOptimizer(op=Adasum): 3 eager steps and one in graph mode against the fp64 emulation of both ranks
def model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(12, 16), torch.nn.Tanh(), torch.nn.Linear(16, 3)).to(dev)

def batch(k, step):
    c = torch.Generator().manual_seed(100 + step)
    g = torch.Generator().manual_seed(1000 + 10 * step + k)
    return ((torch.randn(8, 12, generator=c) + 0.3 * torch.randn(8, 12, generator=g)).to(dev),
            (torch.randn(8, 3, generator=c) + 0.3 * torch.randn(8, 3, generator=g)).to(dev))

m = model()
opt = hvd.DistributedOptimizer(torch.optim.SGD(m.parameters(), lr=0.05, momentum=0.9),
                               named_parameters=m.named_parameters(), op=hvd.Adasum)
assert not opt._hooks
reps = [model() for _ in range(N)]
ropts = [torch.optim.SGD(q.parameters(), lr=0.05, momentum=0.9) for q in reps]
for step in range(4):
    if step == 3:   # a fourth step in graph mode: one stream-ordered inline call over the flat delta buffer
        opt.enable_graph_mode()
    start = [p.detach().clone() for p in m.parameters()]
    x, y = batch(r, step)
    opt.zero_grad()
    torch.nn.functional.mse_loss(m(x), y).backward()
    opt.step()
    torch.cuda.synchronize()
    deltas = []
    for k, (q, ro) in enumerate(zip(reps, ropts)):   # rank k's local step from the shared weights
        with torch.no_grad():
            for p, s in zip(q.parameters(), start):
                p.copy_(s)
        xk, yk = batch(k, step)
        ro.zero_grad()
        torch.nn.functional.mse_loss(q(xk), yk).backward()
        ro.step()
        deltas.append([(p.detach() - s).reshape(-1).cpu() for p, s in zip(q.parameters(), start)])
    for i, (p, s) in enumerate(zip(m.parameters(), start)):
        ds = [deltas[k][i] for k in range(N)]
        want = s.cpu().double().reshape(-1) + adasum.adasum_tree(ds)
        if step == 0 and p.dim() == 2:
            assert_not_sum_or_average(ds, adasum.adasum_tree(ds))
        # the bound on the delta, plus the fp32 rounding of start + delta
        tol = bound(ds, [ds[0].numel()]) + 2.0 ** -24 * want.abs()
        within(p.detach().cpu().reshape(-1), want, tol, f"opt{step}.{i}")
    flat = torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    every = hvd.allgather(flat[None]).cpu()
    assert all(torch.equal(every[0], every[k]) for k in range(N)), step
opt.disable_graph_mode()
hvd.shutdown()
print("ADASUM_HVD_OK", r)
"""

_MNIST = r"""
import hashlib, os, sys, torch
sys.path.insert(0, os.environ["REPO"])
os.environ["PDE_HVD_DATA_PLANE"] = "xgmi"
sys.argv = [os.path.join(os.environ["REPO"], "horovod_examples", "mnist_horovod.py"), "--use-adasum", "--epochs", "1",
            "--train-size", "2048", "--batch-size", "256", "--layers"]
from pytorch_distributed_examples_amd.apps.mnist_hvd import main
model = main()
w = torch.cat([p.detach().reshape(-1).cpu() for p in model.parameters()])
assert torch.isfinite(w).all()
print("ADASUM_WEIGHTS", hashlib.sha256(w.numpy().tobytes()).hexdigest(), flush=True)
"""


def _run(script, n, timeout=240):
    from pytorch_distributed_examples_amd.parallel.dist import free_port

    env = dict(os.environ, REPO=REPO, PDE_BACKEND="gloo")
    with tempfile.NamedTemporaryFile("w", suffix=".py", delete=False) as f:
        f.write(script)
        path = f.name
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), path]
    try:
        return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    finally:
        os.unlink(path)


def _report(res, name):
    if res.returncode != 0:  # full logs for the post-mortem (pytest truncates long assertion messages, not its
        print(f"---- {name}: stdout ----\n{res.stdout}\n---- {name}: stderr ----\n{res.stderr}")  # captured output)
    print("\n".join(l for l in res.stdout.splitlines() if l.startswith("ADASUM_RATIO")))
    return (res.stdout[-2000:], "\n".join(l for l in res.stderr.splitlines() if l.startswith("[rank"))[-6000:],
            res.stderr[-3000:])


@pytest.mark.parametrize("n", [2, 4])
def test_adasum_rehearsal_one_gpu(gpu, n):
    res = _run(_REHEARSAL, n)
    tail = _report(res, f"adasum_rehearsal_{n}")
    assert res.returncode == 0 and res.stdout.count("ADASUM_OK") == n, tail


def test_adasum_hvd_xgmi_world2(gpu):
    res = _run(_HVD, 2)
    tail = _report(res, "adasum_hvd")
    assert res.returncode == 0 and res.stdout.count("ADASUM_HVD_OK") == 2, tail


def test_adasum_mnist_example_world2(gpu):
    res = _run(_MNIST, 2)
    tail = _report(res, "adasum_mnist")
    assert res.returncode == 0, tail
    # (the ranks' lines may interleave without a newline: match the number's own format, %.4f)
    losses = [float(v) for v in re.findall(r"Loss: (-?\d+\.\d{4}|-?inf|nan)", res.stdout)]
    assert len(losses) >= 2 and all(torch.isfinite(torch.tensor(losses))), losses
    hashes = re.findall(r"ADASUM_WEIGHTS ([0-9a-f]{64})", res.stdout)
    assert len(hashes) == 2 and hashes[0] == hashes[1], hashes
