#!/usr/bin/env python3
"""Timing of the two-launch trust-ratio step (csrc/kernels/optim_trust.hip) against the one-launch step it extends.

    python scripts/optim_trust_bench.py [--out profiles/optim_trust.jsonl]

One process.  Every variant is ``--steps`` (64) optimiser steps on fixed gradients captured into a hipGraph; a run is
``--replays`` (200) replays, each ended by a device synchronise, and its figure is the median time per step.  The
variants of a parameter set take turns, ``--rounds`` (7) runs each, so drift of the machine hits both alike.

Parameter sets and pairs:
  mlp       the 5x1024 MLP              FusedLAMB             against FusedAdamW
  cnn       the MNIST CNN               FusedLARS (mom 0.9)   against FusedSGD (momentum 0.9)
  resnet2   ResNet-50 stage 2           FusedLARS (mom 0.9)   against FusedSGD (momentum 0.9)

The parameters are detached copies (no layer keeps compute copies of them), so a step is the update launches alone:
1 for AdamW / SGD, 2 for LAMB / LARS.  Needs a GPU; one JSON row per (set, variant) and one ratio row per set are
appended to ``--out`` and printed.
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "optim_trust.jsonl"))
    ap.add_argument("--steps", type=int, default=64, help="optimiser steps per hipGraph")
    ap.add_argument("--replays", type=int, default=200, help="replays per run")
    ap.add_argument("--rounds", type=int, default=7, help="alternating runs per variant")
    ap.add_argument("--sets", nargs="+", default=["mlp", "cnn", "resnet2"])
    args = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("optim_trust_bench: needs a GPU (a CPU run says nothing about these times)")
    from pytorch_distributed_examples_amd.models.cnn import Net
    from pytorch_distributed_examples_amd.models.mlp import reference_mlp
    from pytorch_distributed_examples_amd.models.resnet import ResNetShard2
    from pytorch_distributed_examples_amd.ops.optim import FusedAdamW, FusedLAMB, FusedLARS, FusedSGD

    dev = torch.device("cuda:0")
    models = {"mlp": reference_mlp, "cnn": Net, "resnet2": ResNetShard2}
    # tiny learning rates: 90,000 steps on one gradient must stay finite (the time does not depend on the values)
    pairs = {
        "mlp": {"adamw": lambda ps: FusedAdamW(ps, lr=1e-7), "lamb": lambda ps: FusedLAMB(ps, lr=1e-7)},
        "cnn": {"sgd_mom": lambda ps: FusedSGD(ps, lr=1e-7, momentum=0.9),
                "lars": lambda ps: FusedLARS(ps, lr=1e-4, momentum=0.9)},
    }
    pairs["resnet2"] = pairs["cnn"]
    launches = {"adamw": 1, "sgd_mom": 1, "lamb": 2, "lars": 2}
    rows = []

    def emit(row):
        row = {"script": "optim_trust_bench", "device": torch.cuda.get_device_name(0), **row}
        rows.append(row)
        print(json.dumps(row), flush=True)

    def build(shapes, make):
        gen = torch.Generator().manual_seed(0)
        ps = [(0.1 * torch.randn(s, generator=gen)).to(dev).requires_grad_() for s in shapes]
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen).to(dev)
        opt = make(ps)
        for _ in range(3):
            opt.step()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(args.steps):
                opt.step()
        for _ in range(5):
            graph.replay()
        torch.cuda.synchronize()
        return graph, opt, ps

    def run(graph):
        per_step = []
        for _ in range(args.replays):
            t0 = time.perf_counter()
            graph.replay()
            torch.cuda.synchronize()
            per_step.append((time.perf_counter() - t0) * 1e6 / args.steps)
        return statistics.median(per_step), min(per_step)

    for name in args.sets:
        shapes = [tuple(p.shape) for p in models[name]().parameters()]
        elems = sum(torch.Size(s).numel() for s in shapes)
        built = {v: build(shapes, make) for v, make in pairs[name].items()}
        med = {v: [] for v in built}
        low = {v: [] for v in built}
        for _ in range(args.rounds):
            for v in built:
                m, lo = run(built[v][0])
                med[v].append(m)
                low[v].append(lo)
        summary = {}
        for v, (graph, opt, ps) in built.items():
            steps = int(opt.state_dict()["state"][0]["step"])
            expect = 3 + args.steps * (5 + args.rounds * args.replays)
            assert steps == expect, (name, v, steps, expect, "the graph did not run every step")
            summary[v] = statistics.median(med[v])
            emit({"what": "graph_optim_step", "set": name, "variant": v, "tensors": len(shapes), "elements": elems,
                  "launches_per_step": launches[v], "steps_per_graph": args.steps, "replays_per_run": args.replays,
                  "runs": args.rounds, "us_per_step_run_medians": [round(t, 3) for t in med[v]],
                  "us_per_step_median": round(summary[v], 3), "us_per_step_min": round(min(low[v]), 3),
                  "weights_finite": all(bool(torch.isfinite(p).all().item()) for p in ps)})
        base, trust = list(built)
        emit({"what": "ratio", "set": name, "trust": trust, "baseline": base,
              "trust_over_baseline": round(summary[trust] / summary[base], 3)})
        del built
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
