"""What the uint8 MNIST path costs next to the fp32 one (profiles/mnist_u8_gather.md), in one process on one GPU,
the two sides alternating round by round:

* ``EpochBatches.fill`` of a 60,000-row shard: the uint8 gather + normalise kernel (data/mnist.py) against the two
  ``index_select`` calls on the fp32 twin -- the device work alone (``fill_*``: index list already on the device)
  and the whole call with its host-side permutation and upload (``fillcall_*``: host clock, ends in a synchronise);
* the captured elastic prologue at ``rows = 10 * 1024``: one hipGraph holding ``gather_rows_u8_counter`` against one
  holding ``gather_rows_counter`` (``node_*``, per replay).

Device times are events around ``--reps`` back-to-back calls (after a warm-up of the same calls), the median over
``--rounds`` rounds; bytes are what the algorithm has to move (source rows + fp32 rows + labels + indices).

    python scripts/mnist_u8_gather_bench.py [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60000)
    ap.add_argument("--rows", type=int, default=10 * 1024)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the GPU")
    from pytorch_distributed_examples_amd import _native
    from pytorch_distributed_examples_amd.data.loader import ShardedLoader
    from pytorch_distributed_examples_amd.data.mnist import MNIST, export
    from pytorch_distributed_examples_amd.utils.epoch_graph import EpochBatches, sampler_indices

    C = _native.C()
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as d:
        export(d, train=args.n, test=16)
        ds = MNIST(d, train=True, device=dev)

    class Twin:
        images = ds.table[ds.images_u8.long()].view(-1, 1, 28, 28)
        labels = ds.labels

        def __len__(self):
            return args.n

    twin = Twin()
    eb_u8 = EpochBatches(ShardedLoader(ds, 128, 1, 0, shuffle=True))
    eb_f32 = EpochBatches(ShardedLoader(twin, 128, 1, 0, shuffle=True))
    # fill() as the trainers call it, minus the host's permutation and its upload (the same on both sides): the
    # device work of one fill on an index list already on the device
    idx = sampler_indices(eb_u8.loader.sampler).to(dev)

    def fill_u8():
        ds.gather(idx, out=(eb_u8.x, eb_u8.y))

    def fill_f32():
        torch.index_select(twin.images, 0, idx, out=eb_f32.x)
        torch.index_select(twin.labels, 0, idx, out=eb_f32.y)

    fill_u8()
    fill_f32()
    assert torch.equal(eb_u8.x, eb_f32.x) and torch.equal(eb_u8.y, eb_f32.y)

    rows = args.rows
    xb = torch.empty(rows, 1, 28, 28, device=dev)
    yb = torch.empty(rows, dtype=torch.long, device=dev)
    counter = torch.zeros(2, dtype=torch.int32, device=dev)

    def capture(fn):
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.cuda.graph(g):
            fn()
        torch.cuda.current_stream().wait_stream(s)
        return g

    g_u8 = capture(lambda: C.gather_rows_u8_counter(ds.images_u8, ds.labels, idx, ds.table, counter, xb, yb))
    g_f32 = capture(lambda: C.gather_rows_counter(twin.images, twin.labels, idx, counter, xb, yb))
    # (the counter runs past the list during the timing: the clamped slices then all read the list's last row --
    # so it is rewound before every call batch to keep every replay on distinct rows)
    per_list = args.n // rows

    def node(g):
        def run():
            counter.zero_()
            for _ in range(per_list):
                g.replay()
        return run

    def fill_call(eb):  # the whole EpochBatches.fill(epoch): permutation on the host, upload, gather; host clock
        import time

        epoch = [0]

        def run(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                epoch[0] += 1
                eb.fill(epoch[0])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6 / reps
        return run

    calls = {"fillcall_u8": fill_call(eb_u8), "fillcall_f32": fill_call(eb_f32)}
    sides = {"fill_u8": fill_u8, "fill_f32": fill_f32, "node_u8": node(g_u8), "node_f32": node(g_f32)}
    for fn in sides.values():  # warm-up of every timed shape
        timed(fn, 10)
    for fn in calls.values():
        fn(3)
    samples = {k: [] for k in list(sides) + list(calls)}
    for _ in range(args.rounds):
        for k, fn in sides.items():  # alternating
            samples[k].append(timed(fn, args.reps if k.startswith("fill") else max(1, args.reps // per_list)))
        for k, fn in calls.items():
            samples[k].append(fn(10))
    for k in ("node_u8", "node_f32"):  # per replay (the counter reset is one tiny memset per per_list replays)
        samples[k] = [v / per_list for v in samples[k]]
    R = 784
    moved = {"fill_u8": args.n * (R + 4 * R + 16 + 8), "fill_f32": args.n * (8 * R + 16 + 8 + 8),
             "node_u8": rows * (R + 4 * R + 16 + 8), "node_f32": rows * (8 * R + 16 + 8)}
    res = {"device": torch.cuda.get_device_name(0), "n": args.n, "rows": rows, "reps": args.reps,
           "rounds": args.rounds}
    for k, v in samples.items():
        med = statistics.median(v)
        res[k] = {"us_median": round(med, 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2)}
        if k in moved:  # (a whole fill() call is mostly host work: no rate)
            res[k].update(bytes=moved[k], GB_per_s=round(moved[k] / med / 1e3, 1))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
