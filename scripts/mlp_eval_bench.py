#!/usr/bin/env python3
"""Timing of the one-launch MLP evaluation (FusedMLPEval, k_mlp_eval) against the layer-by-layer test pass.

    python scripts/mlp_eval_bench.py [--out profiles/mlp_eval.jsonl]

(i)  ``graph_eval_call``: time per ``evaluate`` call of the reference MLP at B = 128, 1024 and 10,000 inside a hipGraph
     of ``--calls`` calls (one stats buffer), every replay ended by a device synchronise; median and minimum over
     ``--replays`` replays.  The replays' totals are checked against the same number of eager calls.
(ii) ``test_pass``: one full test pass of 10,000 rows at the scripts' batch (128) through the entry scripts' own pass
     (``elastic/rewire.py::_test``), ``--rounds`` times each way in one process, alternating the fused route with the
     layer pass (``PDE_MLP_EVAL=0``, the behaviour before this route existed).  Each pass ends in the device-to-host
     copy of its counts.

Needs a GPU; one JSON row per measurement is appended to ``--out`` and printed.  The exit status is 0 when every
fused pass was below every layer pass (the rule for the scripts' default).
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


class _World1:
    size = 1


class _Quiet:
    def __init__(self):
        self.lines = []

    def print(self, msg, **_):
        self.lines.append(msg)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mlp_eval.jsonl"))
    ap.add_argument("--calls", type=int, default=20, help="evaluate calls per hipGraph")
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--test-size", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=128)
    args = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("mlp_eval_bench: needs a GPU (a CPU run says nothing about these times)")
    from pytorch_distributed_examples_amd import _native
    from pytorch_distributed_examples_amd.data.loader import ShardedLoader
    from pytorch_distributed_examples_amd.data.synthetic import mnist_splits
    from pytorch_distributed_examples_amd.elastic.rewire import _test
    from pytorch_distributed_examples_amd.models.cnn_fused import CnnEvalStats
    from pytorch_distributed_examples_amd.models.mlp import reference_mlp
    from pytorch_distributed_examples_amd.models.mlp_eval import FusedMLPEval

    C = _native.C()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = reference_mlp().to(dev)
    ev = FusedMLPEval(model)
    _, test_set = mnist_splits(device=dev, train=args.batch, test=args.test_size)
    loader = ShardedLoader(test_set, args.batch, 1, 0, shuffle=False)
    rows = []

    def emit(row):
        row = {"script": "mlp_eval_bench", "device": torch.cuda.get_device_name(0),
               "rows_per_workgroup": C.mlp_eval_rows_per_workgroup(), **row}
        rows.append(row)
        print(json.dumps(row), flush=True)

    # ---- (i) evaluate calls inside one hipGraph -------------------------------------------------------------
    weight_bytes = sum(L.weight.numel() * 2 for L in ev.layers)
    flop_per_row = sum(2 * L.weight.numel() for L in ev.layers)
    for B in (128, 1024, args.test_size):
        x, y = test_set.images[:B].reshape(B, -1), test_set.labels[:B]
        eager = CnnEvalStats(dev)
        for _ in range(3):
            ev.evaluate(x, y, eager)
        torch.cuda.synchronize()
        correct1 = eager.result()[1] // 3
        stats = CnnEvalStats(dev)
        graph = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.cuda.graph(graph):
            for _ in range(args.calls):
                ev.evaluate(x, y, stats)
        torch.cuda.current_stream().wait_stream(s)
        for _ in range(5):
            graph.replay()
        torch.cuda.synchronize()
        stats.zero_()
        torch.cuda.synchronize()
        per_call = []
        for _ in range(args.replays):
            t0 = time.perf_counter()
            graph.replay()
            torch.cuda.synchronize()
            per_call.append((time.perf_counter() - t0) * 1e3 / args.calls)
        _, correct, count = stats.result()
        n = args.replays * args.calls
        assert (correct, count) == (n * correct1, n * B), (correct, count, "the graph did not repeat the eager call")
        med = statistics.median(per_call)
        emit({"what": "graph_eval_call", "batch": B, "workgroups": -(-B // C.mlp_eval_rows_per_workgroup()),
              "calls_per_graph": args.calls, "replays": args.replays, "ms_per_call_median": round(med, 5),
              "ms_per_call_min": round(min(per_call), 5), "rows_per_s_median": round(B / med * 1e3),
              "tflops_median": round(flop_per_row * B / med / 1e9, 2),
              "weight_bytes_streamed_per_workgroup": weight_bytes})

    # ---- (ii) the entry scripts' test pass, fused route and layer pass alternating ------------------------------
    comm, log = _World1(), _Quiet()

    def one_pass(mode):
        os.environ["PDE_MLP_EVAL"] = mode
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _test(model, loader, dev, comm, log)  # ends in the device-to-host copy of the counts
        return (time.perf_counter() - t0) * 1e3

    for mode in ("1", "0", "1", "0"):  # warm up both ways (code objects, allocator, bf16 weight copies)
        one_pass(mode)
    fused_ms, layer_ms = [], []
    for _ in range(args.rounds):
        fused_ms.append(one_pass("1"))
        layer_ms.append(one_pass("0"))
    os.environ.pop("PDE_MLP_EVAL", None)
    emit({"what": "test_pass", "rows": args.test_size, "batch": args.batch, "rounds": args.rounds,
          "fused_ms": [round(v, 4) for v in fused_ms], "layer_ms": [round(v, 4) for v in layer_ms],
          "fused_ms_median": round(statistics.median(fused_ms), 4),
          "layer_ms_median": round(statistics.median(layer_ms), 4),
          "layer_over_fused_median": round(statistics.median(layer_ms) / statistics.median(fused_ms), 2),
          "every_fused_below_every_layer": max(fused_ms) < min(layer_ms), "printed": sorted(set(log.lines))})

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    return 0 if rows[-1]["every_fused_below_every_layer"] else 1


if __name__ == "__main__":
    sys.exit(main())
