#!/usr/bin/env python3
"""Timing of the xGMI Adasum (XgmiAllreduce.adasum_: Gram launch + combine launch) against the one-shot sum
(XgmiAllreduce.allreduce_: one launch) on the same instance.

    python scripts/adasum_bench.py [--out profiles/adasum_xgmi.jsonl]

Starts ``--ranks`` (2) processes that SHARE one GPU -- a rehearsal: the numbers show launch and protocol cost (flag
round trips, the second launch, the fp64 Gram arithmetic), not xGMI link time; every "peer" read is a local HBM read.
Every variant is ``--calls`` (64) calls captured into a hipGraph; a run is ``--replays`` (200) replays, each ended by a
device synchronise, and its figure is the median time per call.  The variants take turns, ``--rounds`` (7) runs each,
so drift of the machine hits both alike.  Sizes: 21,840 elements (the MNIST CNN's gradients, as its 8 tensors) and
262,144 (one tensor).  Rank 0 appends one JSON row per (size, variant) to ``--out`` and prints it.
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

CNN_SEGS = [250, 10, 5000, 20, 16000, 50, 500, 10]
SIZES = {21840: CNN_SEGS, 262144: [262144]}


def worker(args):
    import torch
    import torch.distributed as dist

    from pytorch_distributed_examples_amd.parallel import dist as pdist
    from pytorch_distributed_examples_amd.parallel.xgmi_allreduce import XgmiAllreduce

    ctx = pdist.init_distributed()
    r, dev = ctx.rank, ctx.device
    xa = XgmiAllreduce(dev, max_bytes=4 << 20, blocks=args.blocks, timeout_s=30.0)
    rows = []
    for n, segs in SIZES.items():
        g = torch.Generator().manual_seed(n)
        base = torch.randn(n, generator=g)
        x = (base + 0.5 * torch.randn(n, generator=torch.Generator().manual_seed(n + 1 + r))).to(dev)
        bufs = {"allreduce": x.clone(), "adasum": x.clone()}
        # every call rewrites its buffer in place: a scale that keeps 90,000 repeated calls finite (the sum
        # doubles correlated inputs, Adasum of equal vectors returns them)
        calls = {"allreduce": lambda t: xa.impl.allreduce_(t, 0.5, False),
                 "adasum": lambda t: xa.adasum_(t, segs, 1.0)}
        graphs = {}
        for v, fn in calls.items():
            for _ in range(3):
                fn(bufs[v])
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s), torch.cuda.graph(graph):
                for _ in range(args.calls):
                    fn(bufs[v])
            torch.cuda.current_stream().wait_stream(s)
            for _ in range(5):
                graph.replay()
            torch.cuda.synchronize()
            graphs[v] = graph
        med = {v: [] for v in calls}
        low = {v: [] for v in calls}
        for _ in range(args.rounds):
            for v in calls:
                dist.barrier()
                per_call = []
                for _ in range(args.replays):
                    t0 = time.perf_counter()
                    graphs[v].replay()
                    torch.cuda.synchronize()
                    per_call.append((time.perf_counter() - t0) * 1e6 / args.calls)
                med[v].append(statistics.median(per_call))
                low[v].append(min(per_call))
        xa.check()
        for v in calls:
            rows.append({"script": "adasum_bench", "device": torch.cuda.get_device_name(0),
                         "what": "shared_card_rehearsal", "ranks": ctx.world_size, "blocks": args.blocks,
                         "variant": v, "elements": n, "segments": len(segs) if v == "adasum" else 1,
                         "launches_per_call": 2 if v == "adasum" else 1, "calls_per_graph": args.calls,
                         "replays_per_run": args.replays, "runs": args.rounds,
                         "us_per_call_run_medians": [round(t, 3) for t in med[v]],
                         "us_per_call_median": round(statistics.median(med[v]), 3),
                         "us_per_call_range": [round(min(med[v]), 3), round(max(med[v]), 3)],
                         "us_per_call_min": round(min(low[v]), 3),
                         "finite": bool(torch.isfinite(bufs[v]).all().item())})
        del graphs
    dist.barrier()
    xa.close()
    dist.destroy_process_group()
    if r == 0:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for row in rows:
                print(json.dumps(row), flush=True)
                f.write(json.dumps(row) + "\n")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "adasum_xgmi.jsonl"))
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=8, help="workgroups per call (ranks sharing a card: few)")
    ap.add_argument("--calls", type=int, default=64, help="calls per hipGraph")
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
           "--out", args.out, "--blocks", str(args.blocks), "--calls", str(args.calls), "--replays",
           str(args.replays), "--rounds", str(args.rounds)]
    return subprocess.run(cmd, env=env, timeout=900).returncode


if __name__ == "__main__":
    sys.exit(main())
