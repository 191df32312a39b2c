#!/usr/bin/env python3
"""Timing of the fused CNN step with the optimiser update inside the slab reduction (cnn_reduce_role<OPT>) against the
routes it replaces.

    python scripts/cnn_optim_bench.py [--out profiles/cnn_fused_optim.jsonl]

One process.  Every variant is ``--steps`` (64) training steps of one batch captured into a hipGraph; a run is
``--replays`` (200) replays, each ended by a device synchronise, and its figure is the median time per step.  The
variants take turns, ``--rounds`` (7) runs each, so drift of the machine hits all of them alike.  Batch 1024 (the
benchmark's) and 128 (the elastic scripts').

Variants:
  sgd_plain_reduce   plain SGD inside the reduction (the benchmark's step; the reference point)      2 launches
  sgd_mom_reduce     SGD momentum 0.9 inside the reduction                                           2 launches
  sgd_mom_generic    the same optimiser through forward_backward + opt.step(): train, reduce, the multi-tensor
                     update and the next step's fragment prep -- the only route before this one       4 launches
  adamw_reduce       AdamW inside the reduction                                                      2 launches
  adamw_step         forward_backward + FusedCNN.adamw_step (k_cnn_opt<2>)                            3 launches

Needs a GPU; one JSON row per (batch, variant) plus one verdict row per batch is appended to ``--out`` and printed.
Exit status 1 when momentum inside the reduction measured slower than the generic route.
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

VARIANTS = ("sgd_plain_reduce", "sgd_mom_reduce", "sgd_mom_generic", "adamw_reduce", "adamw_step")
LAUNCHES = {"sgd_plain_reduce": 2, "sgd_mom_reduce": 2, "sgd_mom_generic": 4, "adamw_reduce": 2, "adamw_step": 3}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cnn_fused_optim.jsonl"))
    ap.add_argument("--steps", type=int, default=64, help="training steps per hipGraph")
    ap.add_argument("--replays", type=int, default=200, help="replays per run")
    ap.add_argument("--rounds", type=int, default=7, help="alternating runs per variant")
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 128])
    args = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("cnn_optim_bench: needs a GPU (a CPU run says nothing about these times)")
    from pytorch_distributed_examples_amd.models.cnn import Net
    from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN
    from pytorch_distributed_examples_amd.ops import functional as OF
    from pytorch_distributed_examples_amd.ops.optim import FusedAdamW, FusedSGD

    dev = torch.device("cuda:0")
    rows = []

    def emit(row):
        row = {"script": "cnn_optim_bench", "device": torch.cuda.get_device_name(0), **row}
        rows.append(row)
        print(json.dumps(row), flush=True)

    def build(variant, x, y):
        """(graph of --steps steps, the loss tensor of its last step, the optimiser)."""
        torch.manual_seed(0)
        net = Net().to(dev).train()
        fused = FusedCNN(net)
        grads = fused.grad_buffer()
        # tiny learning rates: 90,000 steps on one batch must stay finite (the time does not depend on the values)
        if variant.startswith("sgd"):
            opt = FusedSGD(net.parameters(), lr=1e-5, momentum=0.0 if variant == "sgd_plain_reduce" else 0.9)
        else:
            opt = FusedAdamW(net.parameters(), lr=1e-6)
        if variant == "sgd_mom_generic":
            # the fused kernel keeps its own fragment image: the multi-tensor update need not refresh the layer
            # path's conv layouts (a fifth launch) -- the generic route at its four launches
            for p in net.parameters():
                p.__dict__["_pde_own_copies"] = True
                OF.release_compute_copies(p)

        def step():
            if variant.endswith("_reduce"):
                return fused.forward_backward(x, y, grad_out=grads, opt=opt)
            loss = fused.forward_backward(x, y, grad_out=grads)
            if variant == "adamw_step":
                fused.adamw_step(opt, grads)
            else:
                opt.step()
            return loss

        for _ in range(3):
            step()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.cuda.graph(graph):
            for _ in range(args.steps):
                loss = step()
        torch.cuda.current_stream().wait_stream(s)
        for _ in range(5):
            graph.replay()
        torch.cuda.synchronize()
        return graph, loss, opt

    def run(graph):
        per_step = []
        for _ in range(args.replays):
            t0 = time.perf_counter()
            graph.replay()
            torch.cuda.synchronize()
            per_step.append((time.perf_counter() - t0) * 1e3 / args.steps)
        return statistics.median(per_step), min(per_step)

    ok = True
    for batch in args.batches:
        gen = torch.Generator().manual_seed(batch)
        x = torch.randn(batch, 1, 28, 28, generator=gen).to(dev)
        y = torch.randint(0, 10, (batch,), generator=gen).to(dev)
        built = {v: build(v, x, y) for v in VARIANTS}
        med = {v: [] for v in VARIANTS}
        low = {v: [] for v in VARIANTS}
        for _ in range(args.rounds):
            for v in VARIANTS:
                m, lo = run(built[v][0])
                med[v].append(m)
                low[v].append(lo)
        summary = {}
        for v in VARIANTS:
            graph, loss, opt = built[v]
            steps = int(next(iter(opt.state_dict()["state"].values()))["step"])
            expect = 3 + args.steps * (5 + args.rounds * args.replays)
            assert steps == expect, (v, steps, expect, "the graph did not run every step")
            finite = bool(torch.isfinite(loss).item())
            summary[v] = statistics.median(med[v])
            emit({"what": "graph_train_step", "variant": v, "batch": batch, "launches_per_step": LAUNCHES[v],
                  "steps_per_graph": args.steps, "replays_per_run": args.replays, "runs": args.rounds,
                  "ms_per_step_run_medians": [round(t, 5) for t in med[v]],
                  "ms_per_step_median": round(summary[v], 5), "ms_per_step_min": round(min(low[v]), 5),
                  "images_per_s_median": round(batch / summary[v] * 1e3), "final_loss": float(loss.item()),
                  "final_loss_finite": finite})
        mom_ok = summary["sgd_mom_reduce"] <= summary["sgd_mom_generic"]
        ok = ok and mom_ok
        emit({"what": "verdict", "batch": batch,
              "momentum_in_reduce_not_slower_than_generic": mom_ok,
              "momentum_generic_over_in_reduce": round(summary["sgd_mom_generic"] / summary["sgd_mom_reduce"], 3),
              "momentum_in_reduce_over_plain": round(summary["sgd_mom_reduce"] / summary["sgd_plain_reduce"], 3),
              "adamw_faster_route": "reduce" if summary["adamw_reduce"] <= summary["adamw_step"] else "adamw_step",
              "adamw_step_over_in_reduce": round(summary["adamw_step"] / summary["adamw_reduce"], 3)})
        del built
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
