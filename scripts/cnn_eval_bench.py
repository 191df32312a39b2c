#!/usr/bin/env python3
"""Timing of the fused CNN evaluation path (FusedCNN.evaluate, k_cnn_eval) against the layer-by-layer test pass.

    python scripts/cnn_eval_bench.py [--out profiles/r7_cnn_eval.jsonl] [--train-json FILE]

(i)  ``graph_eval_call``: time per 1024-image ``evaluate`` call inside a hipGraph of ``--calls`` calls (one stats
     buffer), every replay ended by a device synchronise; median and minimum over ``--replays`` replays.
(ii) ``test_pass``: one full test pass of 10,000 images at batch 1024 through the entry scripts' own pass
     (``elastic/rewire.py::_test``), ``--rounds`` times each way in one process, alternating the fused path with
     the layer path (``PDE_CNN_EVAL=0``, the behaviour before this path existed).  Each pass ends in the
     device-to-host copy of its counts.

``--train-json FILE``: a file holding bench.py's JSON result line from the same session; its ``ms_per_step`` (fused
training step of the same 1024-image batch) is written beside (i) with the verdict ``eval_below_train_step``.
Needs a GPU; one JSON row per measurement is appended to ``--out`` and printed.
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r7_cnn_eval.jsonl"))
    ap.add_argument("--train-json", default=None)
    ap.add_argument("--calls", type=int, default=64, help="evaluate calls per hipGraph (>= 50)")
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--test-size", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=1024)
    args = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("cnn_eval_bench: needs a GPU (a CPU run says nothing about these times)")
    from pytorch_distributed_examples_amd import _native
    from pytorch_distributed_examples_amd.data.loader import ShardedLoader
    from pytorch_distributed_examples_amd.data.synthetic import mnist_splits
    from pytorch_distributed_examples_amd.elastic.rewire import _test
    from pytorch_distributed_examples_amd.models.cnn import Net
    from pytorch_distributed_examples_amd.models.cnn_fused import CnnEvalStats, FusedCNN

    C = _native.C()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = Net().to(dev)
    fused = FusedCNN(model)
    _, test_set = mnist_splits(device=dev, train=args.batch, test=args.test_size)
    loader = ShardedLoader(test_set, args.batch, 1, 0, shuffle=False)
    rows = []

    def emit(row):
        row = {"script": "cnn_eval_bench", "device": torch.cuda.get_device_name(0),
               "images_per_workgroup": C.cnn_eval_images_per_workgroup(), **row}
        rows.append(row)
        print(json.dumps(row), flush=True)

    # ---- (i) evaluate calls inside one hipGraph -------------------------------------------------------------
    x, y = test_set.images[:args.batch], test_set.labels[:args.batch]
    stats = CnnEvalStats(dev)
    for _ in range(3):
        fused.evaluate(x, y, stats)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.cuda.graph(graph):
        for _ in range(args.calls):
            fused.evaluate(x, y, stats)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(10):
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
    loss_sum, correct, count = stats.result()
    assert count == args.replays * args.calls * args.batch, (count, "the graph did not run every call")
    row = {"what": "graph_eval_call", "batch": args.batch, "calls_per_graph": args.calls, "replays": args.replays,
           "ms_per_call_median": round(statistics.median(per_call), 5), "ms_per_call_min": round(min(per_call), 5),
           "images_per_s_median": round(args.batch / statistics.median(per_call) * 1e3)}
    if args.train_json:
        with open(args.train_json) as f:
            train = [json.loads(line) for line in f if line.lstrip().startswith("{")][-1]
        assert train["config"]["global_batch"] == args.batch, "bench.py ran another batch size"
        row["train_ms_per_step"] = train["ms_per_step"]
        row["train_steps"] = train["steps"]
        row["eval_below_train_step"] = row["ms_per_call_median"] < train["ms_per_step"]
    emit(row)

    # ---- (ii) the entry scripts' test pass, fused and layer path alternating ----------------------------------
    comm, log = _World1(), _Quiet()

    def one_pass(mode):
        os.environ["PDE_CNN_EVAL"] = mode
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _test(model, loader, dev, comm, log, fused=fused)  # ends in the device-to-host copy of the counts
        return (time.perf_counter() - t0) * 1e3

    for mode in ("1", "0", "1", "0"):  # warm up both ways (code objects, allocator, bf16 weight copies)
        one_pass(mode)
    fused_ms, layer_ms = [], []
    for _ in range(args.rounds):
        fused_ms.append(one_pass("1"))
        layer_ms.append(one_pass("0"))
    os.environ.pop("PDE_CNN_EVAL", None)
    acc = sorted(set(log.lines))
    emit({"what": "test_pass", "images": args.test_size, "batch": args.batch, "rounds": args.rounds,
          "fused_ms": [round(v, 4) for v in fused_ms], "layer_ms": [round(v, 4) for v in layer_ms],
          "fused_ms_median": round(statistics.median(fused_ms), 4),
          "layer_ms_median": round(statistics.median(layer_ms), 4),
          "layer_over_fused_median": round(statistics.median(layer_ms) / statistics.median(fused_ms), 2),
          "every_fused_below_every_layer": max(fused_ms) < min(layer_ms), "printed": acc})

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    ok = rows[-1]["every_fused_below_every_layer"] and rows[0].get("eval_below_train_step", True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
