"""hvd.Adasum of the fused CNN's weight deltas on the GPU: the two launches behind ``forward_backward``
(k_cnn_adasum_delta, k_cnn_adasum_apply; csrc/kernels/cnn_fused.hip) rehearsed with 2 and 4 processes sharing ONE card
as in tests/test_adasum_gpu.py, and the Horovod layer on that plane at 2 ranks (FusedHvdStep, the MNIST example).

Results are compared elementwise with ``start + `` the fp64 per-tensor tree of the ranks' reference deltas (a second
FusedCNN per rank that takes the existing ``forward_backward`` + ``opt_step`` from the same weights) under the
derived bound of tests/cnn_adasum_fixture.py::want_and_bound.  One rehearsal per world size runs every check of its
world; the tests below read its markers."""
import functools
import os
import re
import subprocess
import sys
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_PRELUDE = r"""
import os, sys, time, torch, torch.distributed as dist
sys.path.insert(0, os.environ["REPO"]); sys.path.insert(0, os.path.join(os.environ["REPO"], "tests"))
import cnn_adasum_fixture as fx
from adasum_fixture import CNN_SEGS, assert_not_sum_or_average, bound, rank_data, reference
from pytorch_distributed_examples_amd.models.cnn import Net
from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN
from pytorch_distributed_examples_amd.ops import functional as OF
from pytorch_distributed_examples_amd.ops.optim import FusedAdam, FusedAdamW, FusedSGD

MODES = {"sgd": (lambda p: FusedSGD(p, lr=fx.SGD_LR), False),
         "sgd_momentum_wd": (lambda p: FusedSGD(p, lr=fx.SGD_LR, momentum=0.9, weight_decay=fx.WD), False),
         "adam": (lambda p: FusedAdam(p, lr=fx.ADAM_LR), True),
         "adamw": (lambda p: FusedAdamW(p, lr=fx.ADAM_LR, weight_decay=fx.WD), True)}

def say(*words):
    # one write() per line: the ranks share the pipe, and a print() of several words may interleave with a peer's
    sys.stdout.flush()
    os.write(1, (" ".join(str(w) for w in words) + "\n").encode())

def fresh(make, dev):
    # a Net from torch.manual_seed(0), its fused step, optimiser and flat gradient buffer
    torch.manual_seed(0)
    f = FusedCNN(Net().to(dev))
    return f, make(f.net.parameters()), f.grad_buffer()

def local_step(f, o, g, x, y):
    # the existing route: this rank's own step, no exchange
    f.forward_backward(x, y, grad_out=g, p_drop2=0.0, p_drop1=0.0)
    f.opt_step(o, g)

def within(got, want, bnd, what):
    worst = fx.worst_fraction(got, want, bnd)
    say("CNN_ADASUM_RATIO", what, f"{worst:.3f}")
    assert torch.isfinite(got).all() and worst <= 1.0, (what, worst)
    return worst
"""

_REHEARSAL = _PRELUDE + r"""
from pytorch_distributed_examples_amd.parallel import dist as pdist
from pytorch_distributed_examples_amd.parallel.xgmi_allreduce import XgmiAllreduce
from pytorch_distributed_examples_amd.utils.graph import CapturedStep
ctx = pdist.init_distributed()          # PDE_BACKEND=gloo: several ranks on one GPU
N, r, dev = ctx.world_size, ctx.rank, ctx.device
xa = XgmiAllreduce(dev, max_bytes=4 << 20, timeout_s=20.0)

def gather(t):
    ts = [torch.empty_like(t.cpu()) for _ in range(N)]
    dist.all_gather(ts, t.cpu().contiguous())
    return ts

def same_on_all_ranks(t):
    ts = gather(t)
    return all(torch.equal(v, ts[0]) for v in ts)

def data(it):
    x, y = fx.batch(r, N, it)
    return x.to(dev), y.to(dev)

def adasum_step(f, o, g, x, y):
    f.forward_backward(x, y, grad_out=g, p_drop2=0.0, p_drop1=0.0)
    f.adasum_step(o, g, xa)

def state_of(f):
    return [t.clone() for t in (getattr(f, "_opt_m", None), getattr(f, "_opt_v", None)) if t is not None]

def steps_of(o):
    return o._dev[0]["step"].cpu().tolist()

# ---- 1. the kernels: four update modes, three steps, against the fp64 tree of the ranks' reference deltas ----------
for name, (make, adam) in MODES.items():
    fa, oa, ga = fresh(make, dev)
    fb, ob, gb = fresh(make, dev)
    worst = 0.0
    for it in range(3):
        x, y = data(it)
        start = fa.flat.clone()
        with torch.no_grad():
            fb.flat.copy_(start)
        fb.invalidate()
        adasum_step(fa, oa, ga, x, y)
        if it == 2:
            # fragment currency: the image launch B refreshed (no prep launch is due) against one rebuilt from a
            # copy of the weights
            assert fa._frag_gen == OF.weight_generation() and not fa.always_prep
            pa, la = fa.predict(x, logprobs=True)
            fc = FusedCNN(Net().to(dev))
            with torch.no_grad():
                fc.flat.copy_(fa.flat)
            pc, lc = fc.predict(x, logprobs=True)
            assert torch.equal(pa, pc) and torch.equal(la, lc), (name, "fragment image", float((la - lc).abs().max()))
        local_step(fb, ob, gb, x, y)
        torch.cuda.synchronize()
        deltas = gather(fb.flat - start)
        want, bnd = fx.want_and_bound(start.cpu(), deltas, adam=adam)
        if it == 0 and name == "sgd":
            assert_not_sum_or_average(deltas, reference(deltas, CNN_SEGS))
        worst = max(worst, within(fa.flat.cpu(), want, bnd, f"{name}.step{it} N={N}"))
        assert same_on_all_ranks(fa.flat), (name, it)   # every replica holds bit-identical weights
        for sa, sb in zip(state_of(fa), state_of(fb)):  # the state stays local and advances on the local gradient
            assert torch.allclose(sa, sb, rtol=1e-5, atol=0) if adam else torch.equal(sa, sb), (name, it)
    assert steps_of(oa) == [3, 0] and steps_of(ob) == [3, 0], (steps_of(oa), steps_of(ob))  # count, ticket cleared
    xa.check()
    say("CNN_ADASUM_WORST", name, N, f"{worst:.3f}")
    dist.barrier()
say("CNN_ADASUM_KERNELS_OK", r)

if N == 2:
    # ---- 2. a zero-delta rank: rank 1 runs lr 0 -- its delta is exactly 0, rank 0's coefficient exactly 1 and
    # fmaf(w, 0, acc) = acc, so every rank holds start + fl(local_0 - start) bit for bit: rank 0's local step
    # wherever that fp32 subtraction is exact, one rounding of the delta away elsewhere (Horovod's delta form)
    make = lambda p: FusedSGD(p, lr=fx.SGD_LR if r == 0 else 0.0)
    fa, oa, ga = fresh(make, dev)
    fb, ob, gb = fresh(make, dev)
    x, y = data(0)
    start = fa.flat.clone()
    adasum_step(fa, oa, ga, x, y)
    local_step(fb, ob, gb, x, y)
    torch.cuda.synchronize()
    local0 = gather(fb.flat)[0]
    if r == 1:
        assert torch.equal(fb.flat, start)
    expect = start.cpu() + (local0 - start.cpu())
    assert torch.equal(fa.flat.cpu(), expect), float((fa.flat.cpu() - expect).abs().max())
    off = fa.flat.cpu() != local0
    # (two roundings: of the delta, 2^-24 |local_0 - start|, and of start + delta, 2^-24 |result|)
    got64, loc64 = fa.flat.cpu().double(), local0.double()
    assert ((got64 - loc64).abs() <= 2.0 ** -24 * ((loc64 - start.cpu().double()).abs() + got64.abs())).all()
    say("CNN_ADASUM_ZERO_DELTA inexact deltas", int(off.sum()), "of", off.numel())
    assert int(off.sum()) <= off.numel() // 100
    xa.check()
    dist.barrier()
    say("CNN_ADASUM_ZERO_OK", r)

    # ---- 3. one captured step, replayed on three batches, against three eager steps from the same start; a
    # stand-alone Adasum on the same instance before and after (shared epoch / slot parity)
    def standalone(seed):
        xs = [rank_data(k, fx.NPARAM, seed) for k in range(N)]
        t = xs[r].to(dev)
        xa.adasum_(t, CNN_SEGS)
        torch.cuda.synchronize()
        within(t.cpu(), reference(xs, CNN_SEGS), bound(xs, CNN_SEGS), f"standalone{seed}")
    make = MODES["sgd_momentum_wd"][0]
    fe, oe, ge = fresh(make, dev)
    fg, og, gg = fresh(make, dev)
    standalone(91)
    x, y = data(0)
    adasum_step(fe, oe, ge, x, y)
    adasum_step(fg, og, gg, x, y)    # everything lazy is initialised, the fragment image is current
    torch.cuda.synchronize()
    assert fg._frag_gen == OF.weight_generation()   # the captured step carries no prep launch
    graph = CapturedStep(lambda a, b: adasum_step(fg, og, gg, a, b), [x, y], warmup=0).capture()
    for it in (1, 2, 3):
        x, y = data(it)
        graph(x, y)
        adasum_step(fe, oe, ge, x, y)
    torch.cuda.synchronize()
    assert torch.equal(fg.flat, fe.flat) and torch.equal(fg._opt_m, fe._opt_m)
    assert steps_of(og) == [4, 0] and steps_of(oe) == [4, 0], (steps_of(og), steps_of(oe))
    assert same_on_all_ranks(fg.flat)
    standalone(92)
    xa.check()
    dist.barrier()
    say("CNN_ADASUM_GRAPH_OK", r)

    # ---- 4. a late peer: the others spin (bounded) until it arrives; same bits, no error
    make = MODES["sgd_momentum_wd"][0]
    fl, ol, gl = fresh(make, dev)
    fn, on, gn = fresh(make, dev)
    for it in range(2):
        x, y = data(it)
        torch.cuda.synchronize()
        if it == 1 and r == 1:
            time.sleep(0.5)
        adasum_step(fl, ol, gl, x, y)
        torch.cuda.synchronize()
        adasum_step(fn, on, gn, x, y)
    torch.cuda.synchronize()
    assert torch.equal(fl.flat, fn.flat) and torch.equal(fl._opt_m, fn._opt_m) and same_on_all_ranks(fl.flat)
    xa.check()
    say("CNN_ADASUM_LATE_OK", r)

# ---- what the launcher refuses
fa, oa, ga = fresh(MODES["sgd"][0], dev)
fa.forward_backward(*data(0), grad_out=ga, p_drop2=0.0, p_drop1=0.0)
small = XgmiAllreduce(dev, max_bytes=4 << 20, blocks=8, timeout_s=20.0)   # 8 flag rows: fewer than the workgroups
try:
    fa.adasum_step(oa, ga, small)
    raise AssertionError("a view with too few flag rows was accepted")
except RuntimeError:
    pass
torch.cuda.synchronize()
dist.barrier()
small.close(); xa.close()
dist.destroy_process_group()
say("CNN_ADASUM_OK", r)
"""

_HVD = _PRELUDE + r"""
from pytorch_distributed_examples_amd import hvd
from pytorch_distributed_examples_amd.hvd.cnn_step import FusedHvdStep
os.environ["PDE_HVD_DATA_PLANE"] = "xgmi"
os.environ["HOROVOD_CYCLE_TIME"] = "20"   # ms: the enqueues of one burst land in one negotiation cycle
hvd.init()
N, r = hvd.size(), hvd.rank()
dev = torch.device("cuda", torch.cuda.current_device())
fused_route = os.environ.get("PDE_CNN_ADASUM_FUSED", "1") != "0"

make = lambda p: FusedSGD(p, lr=fx.SGD_LR, momentum=0.9)
torch.manual_seed(0)
model = Net().to(dev)
model.eval()    # (the fused step follows net.training: no dropout, so the emulation below sees the same gradients)
opt = hvd.DistributedOptimizer(make(model.parameters()), named_parameters=model.named_parameters(), op=hvd.Adasum)
step = FusedHvdStep(model, opt, fx.sizes(N)[r])
assert step.route == ("adasum_fused" if fused_route else "adasum_fallback"), step.route
assert step.kernel_launches_per_step() == (4 if fused_route else None), step.kernel_launches_per_step()
reps = [fresh(make, dev) for _ in range(N)]   # rank k's local step from the shared weights, emulated on every rank
for f, _, _ in reps:
    f.net.eval()
for it in range(3):
    start = step.fused.flat.clone()
    x, y = fx.batch(r, N, it)
    step(x.to(dev), y.to(dev))
    torch.cuda.synchronize()
    deltas = []
    for k, (f, o, g) in enumerate(reps):
        with torch.no_grad():
            f.flat.copy_(start)
        f.invalidate()
        xk, yk = fx.batch(k, N, it)
        local_step(f, o, g, xk.to(dev), yk.to(dev))
        deltas.append((f.flat - start).cpu())
    want, bnd = fx.want_and_bound(start.cpu(), deltas)
    within(step.fused.flat.cpu(), want, bnd, f"hvd.step{it}")
    every = hvd.allgather(step.fused.flat[None]).cpu()
    assert all(torch.equal(every[0], every[k]) for k in range(N)), it
# the third step was a graph replay (the fused route spends the second, eager, on making the fragment image current)
assert step.replays == (1 if fused_route else 2) and step.graph is not None
assert step.adasum_steps == (2 if fused_route else 0), step.adasum_steps
assert int(opt._dev[0]["step"][0].item()) == 3 and int(opt._dev[0]["step"][1].item()) == 0
hvd.core.check_health()
opt.disable_graph_mode()
hvd.shutdown()
say("CNN_ADASUM_HVD_OK", r)
"""

_MNIST = r"""
import hashlib, os, sys, torch
sys.path.insert(0, os.environ["REPO"])
os.environ["PDE_HVD_DATA_PLANE"] = "xgmi"
# (--log-interval 1: every batch's loss is printed, so the first and the last printed loss are four steps apart)
sys.argv = [os.path.join(os.environ["REPO"], "horovod_examples", "mnist_horovod.py"), "--use-adasum", "--epochs", "1",
            "--train-size", "2048", "--batch-size", "256", "--lr", "0.05", "--log-interval", "1"]
from pytorch_distributed_examples_amd.apps.mnist_hvd import main
model = main()
w = torch.cat([p.detach().reshape(-1).cpu() for p in model.parameters()])
assert torch.isfinite(w).all()
sys.stdout.flush()   # one write() per line: the ranks share the pipe, and the words of a print() may interleave
os.write(1, f"CNN_ADASUM_ROUTE {model.train_route}\n".encode())
os.write(1, f"CNN_ADASUM_WEIGHTS {hashlib.sha256(w.numpy().tobytes()).hexdigest()}\n".encode())
"""


def _run(script, n, timeout=240, **env_extra):
    from pytorch_distributed_examples_amd.parallel.dist import free_port

    env = dict(os.environ, REPO=REPO, PDE_BACKEND="gloo", **env_extra)
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
    if res.returncode != 0:  # full logs for the post-mortem (pytest truncates long assertion messages)
        print(f"---- {name}: stdout ----\n{res.stdout}\n---- {name}: stderr ----\n{res.stderr}")
    print("\n".join(l for l in res.stdout.splitlines() if l.startswith("CNN_ADASUM_")))
    return (res.stdout[-2000:], "\n".join(l for l in res.stderr.splitlines() if l.startswith("[rank"))[-6000:],
            res.stderr[-3000:])


@functools.lru_cache(maxsize=None)
def _rehearsal(n):
    """One run per world size, shared by the tests that read its markers."""
    return _run(_REHEARSAL, n)


@pytest.mark.parametrize("n", [2, 4])
def test_cnn_adasum_kernels(gpu, n):
    """Plain SGD, momentum + weight decay, Adam and AdamW, three steps each: within the bound of the fp64 tree,
    bit-identical weights on all ranks, local state, step count 3 with a cleared ticket, no exchange error, a current
    fragment image; and a view with too few flag rows is refused."""
    res = _rehearsal(n)
    tail = _report(res, f"cnn_adasum_{n}")
    assert res.stdout.count("CNN_ADASUM_KERNELS_OK") == n, tail
    assert res.returncode == 0 and res.stdout.count("CNN_ADASUM_OK") == n, tail
    worst = {m: float(v) for m, v in re.findall(rf"CNN_ADASUM_WORST (\w+) {n} (\d+\.\d+)", res.stdout)}
    assert set(worst) == {"sgd", "sgd_momentum_wd", "adam", "adamw"} and max(worst.values()) <= 1.0, worst


def test_cnn_adasum_zero_delta_rank(gpu):
    """Rank 1 runs lr 0: every rank holds ``start + fl(local_0 - start)`` bit for bit (a coefficient of exactly 1,
    ``fmaf(w, 0, acc)``).  That IS rank 0's local step wherever the fp32 delta is exact; on the CPU fixture 16 to 22
    of the 21,840 deltas are not (a weight much smaller than its update), and there the delta form is one rounding of
    the delta away -- the script prints the count and bounds it by 1 % of the elements, and each difference by the two
    roundings of the delta form."""
    res = _rehearsal(2)
    assert res.stdout.count("CNN_ADASUM_ZERO_OK") == 2, _report(res, "cnn_adasum_zero")


def test_cnn_adasum_graph_replays(gpu):
    res = _rehearsal(2)
    assert res.stdout.count("CNN_ADASUM_GRAPH_OK") == 2, _report(res, "cnn_adasum_graph")


def test_cnn_adasum_late_peer(gpu):
    res = _rehearsal(2)
    assert res.stdout.count("CNN_ADASUM_LATE_OK") == 2, _report(res, "cnn_adasum_late")


@pytest.mark.parametrize("fused", ["1", "0"])
def test_cnn_adasum_hvd_step_world2(gpu, fused):
    """FusedHvdStep around an Adasum DistributedOptimizer: 4 launches per step on the fused route, three steps (the
    third a graph replay) within the bound of the fp64 emulation of both ranks; PDE_CNN_ADASUM_FUSED=0: the same
    script on forward_backward + opt.step()."""
    res = _run(_HVD, 2, PDE_CNN_ADASUM_FUSED=fused)
    tail = _report(res, f"cnn_adasum_hvd_{fused}")
    assert res.returncode == 0 and res.stdout.count("CNN_ADASUM_HVD_OK") == 2, tail


def test_cnn_adasum_mnist_example_world2(gpu):
    res = _run(_MNIST, 2)
    tail = _report(res, "cnn_adasum_mnist")
    assert res.returncode == 0, tail
    assert re.findall(r"CNN_ADASUM_ROUTE (\w+)", res.stdout) == ["adasum_fused"] * 2, tail
    # (the ranks' lines may interleave without a newline: match the number's own format, %.4f)
    losses = [float(v) for v in re.findall(r"Loss: (-?\d+\.\d{4}|-?inf|nan)", res.stdout)]
    assert len(losses) >= 4 and all(torch.isfinite(torch.tensor(losses))), losses
    assert losses[-1] < losses[0], losses
    hashes = re.findall(r"CNN_ADASUM_WEIGHTS ([0-9a-f]{64})", res.stdout)
    assert len(hashes) == 2 and hashes[0] == hashes[1], hashes
