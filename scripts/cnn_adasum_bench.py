#!/usr/bin/env python3
"""Step time of the fused MNIST CNN under hvd.Adasum: the two Adasum launches behind the fused kernel (FusedHvdStep's
``adasum_fused`` route, 4 launches per step) against ``forward_backward`` + the Adasum optimizer's own ``step()``
(``PDE_CNN_ADASUM_FUSED=0``: _foreach copies, the local multi-tensor update, a subtract, the stand-alone exchange's two
launches and an add), with the averaged all-reduce step for scale.

    python scripts/cnn_adasum_bench.py [--out profiles/cnn_fused_adasum.jsonl]

Starts ``--ranks`` (2) processes that SHARE one GPU -- a rehearsal: the numbers show launch and protocol cost, not xGMI
link time; every "peer" read is a local HBM read.  Every variant is ``--steps`` (64) training steps on one batch captured
into a hipGraph; a run is ``--replays`` (200) replays, each ended by a device synchronise, and its figure is the median
time per step.  The variants take turns, ``--rounds`` (7) runs each, so drift of the machine hits all alike.  Batch 1024
and 128 per rank.  Rank 0 appends one JSON row per (batch, variant) to ``--out`` and prints it.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

# (name, optimiser, hvd op, PDE_CNN_ADASUM_FUSED)
VARIANTS = [("adasum_fused_sgd_momentum", "sgd", "adasum", "1"), ("adasum_fused_adamw", "adamw", "adasum", "1"),
            ("adasum_fallback_sgd_momentum", "sgd", "adasum", "0"), ("adasum_fallback_adamw", "adamw", "adasum", "0"),
            ("average_sgd_momentum", "sgd", "average", "1")]


def worker(args):
    import torch

    os.environ["PDE_HVD_DATA_PLANE"] = "xgmi"
    from pytorch_distributed_examples_amd import hvd
    from pytorch_distributed_examples_amd.data.synthetic import mnist_splits
    from pytorch_distributed_examples_amd.hvd.cnn_step import FusedHvdStep
    from pytorch_distributed_examples_amd.models.cnn import Net
    from pytorch_distributed_examples_amd.ops.optim import FusedAdamW, FusedSGD
    from pytorch_distributed_examples_amd.utils.graph import CapturedSteps

    hvd.init()
    r, n_ranks = hvd.rank(), hvd.size()
    dev = torch.device("cuda", torch.cuda.current_device())
    train, _ = mnist_splits(device=dev, train=1024 * n_ranks, test=16)
    rows = []
    for batch in (1024, 128):
        x = train.images[r * batch:(r + 1) * batch].float().reshape(-1, 1, 28, 28).contiguous()
        y = train.labels[r * batch:(r + 1) * batch].long().contiguous()
        steps, graphs = {}, {}
        for name, kind, op, switch in VARIANTS:
            os.environ["PDE_CNN_ADASUM_FUSED"] = switch
            torch.manual_seed(0)
            model = Net().to(dev)
            model.train()
            # small rates: tens of thousands of steps on one batch stay finite
            opt = (FusedSGD(model.parameters(), lr=1e-3, momentum=0.9) if kind == "sgd" else
                   FusedAdamW(model.parameters(), lr=1e-4, weight_decay=1e-2))
            named = [(f"{name}.b{batch}.{n}", p) for n, p in model.named_parameters()]
            opt = hvd.DistributedOptimizer(opt, named_parameters=named,
                                           op=hvd.Adasum if op == "adasum" else hvd.Average)
            step = FusedHvdStep(model, opt, batch, graph=False)
            for _ in range(3):  # negotiation, graph mode on, the fragment image current
                step.eager_step(x, y)
            torch.cuda.synchronize()
            g = CapturedSteps(step.eager_step, [(x, y)] * args.steps, warmup=0).capture()
            for _ in range(3):
                g.replay()
            torch.cuda.synchronize()
            steps[name], graphs[name] = step, g
        med = {name: [] for name in graphs}
        low = {name: [] for name in graphs}
        for _ in range(args.rounds):
            for name in graphs:
                hvd.barrier()
                per_step = []
                for _ in range(args.replays):
                    t0 = time.perf_counter()
                    graphs[name].replay()
                    torch.cuda.synchronize()
                    per_step.append((time.perf_counter() - t0) * 1e6 / args.steps)
                med[name].append(statistics.median(per_step))
                low[name].append(min(per_step))
        hvd.core.check_health()
        for name, kind, op, switch in VARIANTS:
            w = steps[name].fused.flat
            rows.append({"script": "cnn_adasum_bench", "device": torch.cuda.get_device_name(0),
                         "what": "shared_card_rehearsal", "ranks": n_ranks, "batch_per_rank": batch, "variant": name,
                         "route": steps[name].route, "kernel_launches_per_step": steps[name].kernel_launches_per_step(),
                         "steps_per_graph": args.steps, "replays_per_run": args.replays, "runs": args.rounds,
                         "us_per_step_run_medians": [round(t, 3) for t in med[name]],
                         "us_per_step_median": round(statistics.median(med[name]), 3),
                         "us_per_step_range": [round(min(med[name]), 3), round(max(med[name]), 3)],
                         "us_per_step_min": round(min(low[name]), 3), "finite": bool(torch.isfinite(w).all().item())})
        for name in list(graphs):
            steps[name].opt.disable_graph_mode()
        del graphs, steps
    hvd.shutdown()
    if r == 0:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for row in rows:
                print(json.dumps(row), flush=True)
                f.write(json.dumps(row) + "\n")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cnn_fused_adasum.jsonl"))
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--steps", type=int, default=64, help="training steps per hipGraph")
    ap.add_argument("--replays", type=int, default=200, help="replays per run")
    ap.add_argument("--rounds", type=int, default=7, help="alternating runs per variant")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.worker:
        worker(args)
        return 0
    from pytorch_distributed_examples_amd.parallel.dist import free_port

    env = dict(os.environ, PDE_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.ranks}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__), "--worker",
           "--out", args.out, "--steps", str(args.steps), "--replays", str(args.replays), "--rounds", str(args.rounds)]
    return subprocess.run(cmd, env=env, timeout=900).returncode


if __name__ == "__main__":
    sys.exit(main())
