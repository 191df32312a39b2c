#!/usr/bin/env python3
"""Step time of ``FusedMLP.forward_backward`` + ``FusedAdam.step()`` on the reference 5x1024 MLP, bf16 or fp8.

    python scripts/fp8_step_bench.py --precision fp8 [--out profiles/fp8_linear.jsonl]

One precision per process (alternate fresh processes to compare).  For each batch in 128, 1024, 8192: ``--steps`` steps
inside one hipGraph, ``--replays`` replays each ended by a device synchronise; median and minimum per step.  The
last replay's loss is checked to be finite.  Needs a GPU; one JSON row per batch is printed and appended to ``--out``.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--precision", required=True, choices=["bf16", "fp8"])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fp8_linear.jsonl"))
    ap.add_argument("--steps", type=int, default=20, help="training steps per hipGraph")
    ap.add_argument("--replays", type=int, default=30)
    args = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("fp8_step_bench: needs a GPU (a CPU run says nothing about these times)")
    from pytorch_distributed_examples_amd.models.mlp import reference_mlp
    from pytorch_distributed_examples_amd.models.mlp_fused import FusedMLP
    from pytorch_distributed_examples_amd.ops.optim import FusedAdam

    dev = torch.device("cuda:0")
    rows = []
    for B in (128, 1024, 8192):
        torch.manual_seed(0)
        model = reference_mlp().to(dev)
        opt = FusedAdam(model.parameters(), lr=1e-3)
        fm = FusedMLP(model, precision=args.precision)
        x, y = torch.randn(B, 784, device=dev), torch.randint(0, 10, (B,), device=dev)
        if args.precision == "fp8":
            fm.calibrate(x, y)
        for _ in range(3):
            loss = fm.forward_backward(x, y)
            opt.step()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.cuda.graph(graph):
            for _ in range(args.steps):
                loss = fm.forward_backward(x, y)
                opt.step()
        torch.cuda.current_stream().wait_stream(s)
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        per_step = []
        for _ in range(args.replays):
            t0 = time.perf_counter()
            graph.replay()
            torch.cuda.synchronize()
            per_step.append((time.perf_counter() - t0) * 1e6 / args.steps)
        assert torch.isfinite(loss).item(), "non-finite loss"
        row = {"script": "fp8_step_bench", "device": torch.cuda.get_device_name(0), "precision": args.precision,
               "batch": B, "steps_per_graph": args.steps, "replays": args.replays,
               "launches_per_step": fm.launches_per_step(), "us_per_step_median": round(statistics.median(per_step), 2),
               "us_per_step_min": round(min(per_step), 2), "last_loss": round(loss.item(), 5)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
