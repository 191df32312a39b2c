#!/usr/bin/env python3
"""Step cost of global-norm gradient clipping (``max_grad_norm``; csrc/kernels/optim_clip.hip, k_cnn_opt_clip)
against the same step without it.

    python scripts/optim_clip_bench.py [--out profiles/optim_clip.jsonl] [--sets mlp cnn1024 cnn128]

One process per call; call it several times for fresh processes.  Every variant is ``--steps`` steps captured into a
hipGraph; a run is ``--replays`` replays, each ended by a device synchronise, and its figure is the median time per
step.  The variants of a set take turns, ``--rounds`` runs each, so drift of the machine hits all alike.

  mlp       the 5x1024 MLP's parameters, optimiser step alone on fixed gradients:
            adamw (1 launch) | adamw_clip (2) | lamb (2) | lamb_clip (3)
  cnnB      the fused CNN at batch B, forward_backward + opt_step (momentum SGD):
            plain (3 launches) | clip_fused (3: k_cnn_opt_clip) | clip_two (4: k_grad_clip + k_cnn_opt on hp_eff)
  cnn_upd   the CNN's opt_step alone on a fixed gradient, the same three variants (1 | 1 | 2 launches)

Needs a GPU; one JSON row per (set, variant) is appended to ``--out`` and printed.
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "optim_clip.jsonl"))
    ap.add_argument("--steps", type=int, default=32, help="steps per hipGraph")
    ap.add_argument("--replays", type=int, default=100, help="replays per run")
    ap.add_argument("--rounds", type=int, default=5, help="alternating runs per variant")
    ap.add_argument("--sets", nargs="+", default=["mlp", "cnn1024", "cnn128", "cnn_upd"])
    args = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("optim_clip_bench: needs a GPU (a CPU run says nothing about these times)")
    from pytorch_distributed_examples_amd.models.cnn import Net
    from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN
    from pytorch_distributed_examples_amd.models.mlp import reference_mlp
    from pytorch_distributed_examples_amd.ops.optim import FusedAdamW, FusedLAMB, FusedSGD

    dev = torch.device("cuda:0")
    clip = dict(max_grad_norm=1.0)

    def mlp_step(make):
        gen = torch.Generator().manual_seed(0)
        ps = [(0.1 * torch.randn(p.shape, generator=gen)).to(dev).requires_grad_() for p in reference_mlp().parameters()]
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen).to(dev)
        opt = make(ps)
        return opt.step

    def cnn_step(B, fused_clip, update_only=False, **kw):
        def build():
            torch.manual_seed(0)
            f = FusedCNN(Net().to(dev).eval())
            g = f.grad_buffer()
            opt = FusedSGD(f.params, lr=1e-7, momentum=0.9, **kw)
            x, y = torch.randn(B, 1, 28, 28, device=dev), torch.randint(0, 10, (B,), device=dev)
            f.forward_backward(x, y, grad_out=g)

            def step():
                os.environ["PDE_CNN_CLIP_FUSED"] = "1" if fused_clip else "0"  # read by opt_step at capture
                if not update_only:
                    f.forward_backward(x, y, grad_out=g)
                f.opt_step(opt, g)
            return step
        return build

    sets = {"mlp": {"adamw": lambda: mlp_step(lambda ps: FusedAdamW(ps, lr=1e-7)),
                    "adamw_clip": lambda: mlp_step(lambda ps: FusedAdamW(ps, lr=1e-7, **clip)),
                    "lamb": lambda: mlp_step(lambda ps: FusedLAMB(ps, lr=1e-7)),
                    "lamb_clip": lambda: mlp_step(lambda ps: FusedLAMB(ps, lr=1e-7, **clip))}}
    for name, B, upd in (("cnn1024", 1024, False), ("cnn128", 128, False), ("cnn_upd", 128, True)):
        sets[name] = {"plain": cnn_step(B, True, upd), "clip_fused": cnn_step(B, True, upd, **clip),
                      "clip_two": cnn_step(B, False, upd, **clip)}

    def capture(step):
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(args.steps):
                step()
        for _ in range(5):
            graph.replay()
        torch.cuda.synchronize()
        return graph

    def run(graph):
        per_step = []
        for _ in range(args.replays):
            t0 = time.perf_counter()
            graph.replay()
            torch.cuda.synchronize()
            per_step.append((time.perf_counter() - t0) * 1e6 / args.steps)
        return statistics.median(per_step)

    rows = []
    for name in args.sets:
        # (the step callables stay referenced: they own the optimiser, its device tables and the tensors whose
        # addresses the captured launches hold)
        steps = {v: build() for v, build in sets[name].items()}
        graphs = {v: capture(step) for v, step in steps.items()}
        med = {v: [] for v in graphs}
        for _ in range(args.rounds):
            for v, graph in graphs.items():
                med[v].append(run(graph))
        for v in graphs:
            rows.append({"script": "optim_clip_bench", "device": torch.cuda.get_device_name(0), "pid": os.getpid(),
                         "set": name, "variant": v, "steps_per_graph": args.steps, "replays_per_run": args.replays,
                         "us_per_step_run_medians": [round(t, 3) for t in med[v]],
                         "us_per_step_median": round(statistics.median(med[v]), 3)})
            print(json.dumps(rows[-1]), flush=True)
        torch.cuda.synchronize()
        del graphs, steps
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
