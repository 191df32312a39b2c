"""The stateful updates over the in-kernel xGMI gradient exchange, rehearsed on ONE GPU as in tests/test_xgmi_gpu.py:
two processes share the card and map each other's IPC-exported staging buffers.  SGD with momentum + weight decay
and AdamW inside the slab reduction (exchange, then update) against local gradients all-reduced over gloo plus the
one-launch update (k_cnn_opt<MODE>); weights and optimiser state bit-identical across the two ranks."""
import os
import subprocess
import sys
import tempfile

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SCRIPT = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ["REPO"])
from pytorch_distributed_examples_amd.parallel import dist as pdist
from pytorch_distributed_examples_amd.parallel.xgmi_allreduce import XgmiAllreduce
ctx = pdist.init_distributed()          # PDE_BACKEND=gloo: several ranks on one GPU
N, r, dev = ctx.world_size, ctx.rank, ctx.device
xa = XgmiAllreduce(dev, max_bytes=4 << 20, timeout_s=20.0)
from pytorch_distributed_examples_amd.models.cnn import Net
from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN
from pytorch_distributed_examples_amd.ops.optim import FusedAdamW, FusedSGD

def same_on_all_ranks(t):
    ts = [torch.empty_like(t.cpu()) for _ in range(N)]
    dist.all_gather(ts, t.cpu())
    return all(torch.equal(v, ts[0]) for v in ts)

cases = [("sgd", lambda p: FusedSGD(p, lr=0.05, momentum=0.9, weight_decay=1e-2), ("momentum_buffer",)),
         ("adamw", lambda p: FusedAdamW(p, lr=0.01, weight_decay=1e-2), ("exp_avg", "exp_avg_sq"))]
for name, make, keys in cases:
    torch.manual_seed(0)
    net_a, net_b = Net().to(dev), Net().to(dev)
    net_b.load_state_dict(net_a.state_dict())
    fa, fb = FusedCNN(net_a), FusedCNN(net_b)
    oa, ob = make(net_a.parameters()), make(net_b.parameters())
    ga, gb = fa.grad_buffer(), fb.grad_buffer()  # installs the p.grad views the optimisers step
    gen = torch.Generator().manual_seed(100 + r)
    for it in range(3):
        x = torch.randn(70 + 60 * r, 1, 28, 28, generator=gen).to(dev)   # ranks hold different batch sizes
        y = torch.randint(0, 10, (x.shape[0],), generator=gen).to(dev)
        fa.forward_backward(x, y, grad_out=ga, sgd=oa, xgmi=xa, p_drop2=0.0, p_drop1=0.0)
        fb.forward_backward(x, y, grad_out=gb, p_drop2=0.0, p_drop1=0.0)
        h = gb.cpu(); dist.all_reduce(h); gb.copy_(h / N)
        fb.opt_step(ob, gb)
    torch.cuda.synchronize()
    xa.check()
    assert torch.allclose(ga, gb, rtol=1e-5, atol=1e-7), (name, (ga - gb).abs().max())
    assert torch.allclose(fa.flat, fb.flat, rtol=1e-5, atol=1e-7), (name, (fa.flat - fb.flat).abs().max())
    print("XGMI_OPT", name, r, "max |dw|", float((fa.flat - fb.flat).abs().max()), flush=True)
    sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
    assert all(int(s["step"]) == 3 for s in sa.values()) and all(int(s["step"]) == 3 for s in sb.values())
    assert int(oa._dev[0]["step"][1].item()) == 0  # the arrival ticket cleared
    assert same_on_all_ranks(fa.flat), name      # every replica holds bit-identical weights
    for k in sa:
        for key in keys:
            assert same_on_all_ranks(sa[k][key]), (name, k, key)
    dist.barrier()
dist.barrier()
xa.close()
dist.destroy_process_group()
print("XGMI_OPT_OK", r)
"""


def test_stateful_updates_over_the_xgmi_exchange(gpu):
    from pytorch_distributed_examples_amd.parallel.dist import free_port

    env = dict(os.environ, REPO=REPO, PDE_BACKEND="gloo")
    with tempfile.NamedTemporaryFile("w", suffix=".py", delete=False) as f:
        f.write(_SCRIPT)
        path = f.name
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), path]
    try:
        res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    finally:
        os.unlink(path)
    ranks = "\n".join(l for l in res.stderr.splitlines() if l.startswith("[rank"))  # the ranks' tracebacks
    print(res.stdout[-2000:])
    assert res.returncode == 0 and res.stdout.count("XGMI_OPT_OK") == 2, (res.stdout[-2000:], ranks[-6000:])
