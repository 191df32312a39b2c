"""The uint8 gather + normalise kernel (csrc/kernels/elementwise.hip k_gather_rows_u8) and what runs on it: the
byte dataset (data/mnist.py), the loaders, the epoch graphs of the fused CNN path and the entry scripts on an
exported directory.  Everything the kernel writes is compared bitwise: a normalised pixel is table[byte]."""
import json
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def _table():
    from pytorch_distributed_examples_amd.data.mnist import pixel_table

    return pixel_table()


def _source(N, R, seed):
    """uint8 [N, R] with every byte value, labels [N]."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, 256, (N, R), generator=g, dtype=torch.uint8)
    src.view(-1)[torch.randperm(N * R, generator=g)[:256]] = torch.arange(256, dtype=torch.uint8)
    assert src.unique().numel() == 256
    return src, torch.randint(0, 10, (N,), generator=g)


@pytest.fixture(scope="module")
def exported(tmp_path_factory):
    from pytorch_distributed_examples_amd.data.mnist import export

    d = tmp_path_factory.mktemp("mnist_idx")
    export(d, train=2048, test=512)
    return d


@pytest.mark.parametrize("R,rows", [(R, rows) for R in (16, 48, 784) for rows in (1, 3, 255, 257, 1003)] +
                         [(784, 10700)])
def test_gather_rows_u8_matches_table_lookup(gpu, R, rows):
    """rows x R / 16 chunks: one lane, one wave, part of a workgroup, several workgroups; 10,700 rows of 784 are
    524,300 chunks, the first count above the launch's 2048 x 256 lanes (the grid-stride loop runs)."""
    from pytorch_distributed_examples_amd import _native

    C = _native.C()
    N = 301
    src, labels = _source(N, R, seed=R + rows)
    g = torch.Generator().manual_seed(7)
    K = rows + 5
    idx = torch.randint(0, N, (K,), generator=g)
    idx[0], idx[K // 2], idx[-1] = 0, N - 1, N - 1
    if K > 8:
        idx[3], idx[4], idx[5] = N - 1, 7, 7  # repeated rows
    table = _table()
    expanded = table[src.long()]  # the reference, computed once on the host: [N, R] fp32
    d_src, d_labels, d_idx, d_table = src.to(gpu), labels.to(gpu), idx.to(gpu), table.to(gpu)
    for start in (0, 5, 9):  # 9: start + rows runs 4 past the list; those rows repeat idx[K - 1]
        pos = (torch.arange(rows) + start).clamp(max=K - 1)
        x = torch.full((rows, R), float("nan"), device=gpu)
        y = torch.full((rows,), -1, dtype=torch.long, device=gpu)
        C.gather_rows_u8(d_src, d_labels, d_idx, d_table, x, y, start)
        assert torch.equal(x.cpu(), expanded.index_select(0, idx[pos])), (R, rows, start)
        assert torch.equal(y.cpu(), labels.index_select(0, idx[pos])), (R, rows, start)


def test_gather_rows_u8_counter_eager_and_replayed(gpu):
    """tests/test_gather_counter_gpu.py's scenario on the byte kernel."""
    from pytorch_distributed_examples_amd import _native

    C = _native.C()
    N, rows, R = 5000, 3 * 128, 784
    src, labels = _source(N, R, seed=0)
    g = torch.Generator().manual_seed(0)
    table = _table().to(gpu)
    src, labels = src.to(gpu), labels.to(gpu)
    idx = torch.randperm(N, generator=g)[:4 * rows].to(gpu)
    counter = torch.zeros(2, dtype=torch.int32, device=gpu)
    x = torch.empty(rows, 1, 28, 28, device=gpu)
    y = torch.empty(rows, dtype=torch.long, device=gpu)

    def want(c):
        sl = idx[c * rows:(c + 1) * rows]
        return table[src.index_select(0, sl).long()].view(rows, 1, 28, 28), labels.index_select(0, sl)

    for c in range(2):  # eager: the counter advances once per launch
        C.gather_rows_u8_counter(src, labels, idx, table, counter, x, y)
        wx, wy = want(c)
        assert torch.equal(x, wx) and torch.equal(y, wy), c
    assert counter.tolist() == [2, 0]
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.cuda.graph(graph):
        C.gather_rows_u8_counter(src, labels, idx, table, counter, x, y)
    torch.cuda.current_stream().wait_stream(s)
    counter.copy_(torch.tensor([1, 0], dtype=torch.int32))  # the host repositions (epoch start / resume)
    for c in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        wx, wy = want(c)
        assert torch.equal(x, wx) and torch.equal(y, wy), c
    assert counter.tolist() == [4, 0]


def test_gather_rows_u8_rejects_before_launch(gpu):
    from pytorch_distributed_examples_amd import _native

    C = _native.C()
    table = _table().to(gpu)
    labels = torch.zeros(8, dtype=torch.long, device=gpu)
    idx = torch.zeros(4, dtype=torch.long, device=gpu)
    y = torch.full((4,), -1, dtype=torch.long, device=gpu)

    def untouched(x):
        torch.cuda.synchronize()
        assert bool((x == -1).all()) and bool((y == -1).all())

    x = torch.full((4, 20), -1.0, device=gpu)
    with pytest.raises(RuntimeError, match="multiple of 16"):  # R = 20
        C.gather_rows_u8(torch.zeros(8, 20, dtype=torch.uint8, device=gpu), labels, idx, table, x, y, 0)
    untouched(x)
    src = torch.zeros(8, 16, dtype=torch.uint8, device=gpu)
    flat = torch.full((4 * 16 + 4,), -1.0, device=gpu)
    view = flat[1:1 + 4 * 16].view(4, 16)  # contiguous, 4 bytes off a 16-byte boundary
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        C.gather_rows_u8(src, labels, idx, table, view, y, 0)
    untouched(flat)
    x = torch.full((4, 16), -1.0, device=gpu)
    with pytest.raises(RuntimeError, match="uint8"):
        C.gather_rows_u8(src.to(torch.int8), labels, idx, table, x, y, 0)
    with pytest.raises(RuntimeError, match="uint8"):
        C.gather_rows_u8_counter(src.float(), labels, idx, table, torch.zeros(2, dtype=torch.int32, device=gpu), x, y)
    untouched(x)
    C.gather_rows_u8(src, labels, idx, table, x, y, 0)  # (the same arguments with a good src pass)
    assert torch.equal(x.cpu(), _table()[0].expand(4, 16)) and y.tolist() == [0] * 4


def test_dataset_gather_gpu_equals_cpu(gpu, exported):
    from pytorch_distributed_examples_amd.data.mnist import MNIST

    cpu, dev = MNIST(exported, train=True, limit=1000), MNIST(exported, train=True, device=gpu, limit=1000)
    assert dev.images_u8.is_cuda and dev.images_u8.dtype == torch.uint8 and dev.table.is_cuda and dev.labels.is_cuda
    assert not hasattr(dev, "images")
    g = torch.Generator().manual_seed(2)
    idx = torch.cat([torch.tensor([0, 999, 999, 0]), torch.randint(0, 1000, (333,), generator=g)])
    wx, wy = cpu.gather(idx)
    x, y = dev.gather(idx.to(gpu))
    assert x.shape == (337, 1, 28, 28) and torch.equal(x.cpu(), wx) and torch.equal(y.cpu(), wy)
    xo, yo = torch.empty(100, 1, 28, 28, device=gpu), torch.empty(100, dtype=torch.long, device=gpu)
    dev.gather(idx.to(gpu), out=(xo, yo), start=37, rows=100)
    assert torch.equal(xo.cpu(), wx[37:137]) and torch.equal(yo.cpu(), wy[37:137])
    xi, yi = dev[999]
    assert torch.equal(xi.cpu(), wx[1]) and int(yi) == int(wy[1])


class Twin:
    """The fp32 form of a byte dataset, as the loaders have always taken it (``images`` / ``labels``)."""

    def __init__(self, ds):
        self.images = ds.table[ds.images_u8.long()].view(-1, 1, 28, 28)
        self.labels = ds.labels.clone()

    def __len__(self):
        return self.labels.shape[0]


@pytest.fixture(scope="module")
def pair(gpu, exported):
    from pytorch_distributed_examples_amd.data.mnist import MNIST

    ds = MNIST(exported, train=True, device=gpu, limit=1000)
    twin = Twin(ds)
    assert torch.equal(twin.images.cpu().view(-1, 784),
                       ds.images_u8.cpu().float().div(255).sub(0.1307).div(0.3081))  # the twin is the definition
    return ds, twin


@pytest.mark.parametrize("rank", [0, 1])
def test_loaders_equal_fp32_twin_gpu(pair, rank):
    from pytorch_distributed_examples_amd.data.loader import ShardedLoader
    from pytorch_distributed_examples_amd.utils.epoch_graph import EpochBatches

    ds, twin = pair
    la, lb = (ShardedLoader(d, 64, 2, rank, shuffle=True) for d in (ds, twin))
    ea, eb = (EpochBatches(ShardedLoader(d, 64, 2, rank, shuffle=True)) for d in (ds, twin))
    assert ea.x.is_cuda and ea.x.dtype == torch.float32 and ea.x.shape == (500, 1, 28, 28)
    for epoch in (0, 1):
        la.set_epoch(epoch)
        lb.set_epoch(epoch)
        a, b = list(la), list(lb)
        assert len(a) == len(b) == 8 and [x.shape[0] for x, _ in a] == [64] * 7 + [52]
        ea.fill(epoch)
        eb.fill(epoch)
        for i, ((xa, ya), (xb, yb)) in enumerate(zip(a, b)):
            assert xa.is_cuda and torch.equal(xa, xb) and torch.equal(ya, yb)
            (fa, ga), (fb, gb) = ea.batch(i), eb.batch(i)
            assert torch.equal(fa, fb) and torch.equal(ga, gb) and torch.equal(fa, xa) and torch.equal(ga, ya)


def test_chunked_graphs_feed_equal_batches(gpu, exported):
    """The fused CNN path's data flow (ChunkedGraphs over EpochBatches) on the byte dataset and on its fp32 twin:
    the step function sees bitwise-equal (x, y) sequences.  The step only clones its inputs, so no training
    kernel's determinism is involved."""
    from pytorch_distributed_examples_amd.data.loader import ShardedLoader
    from pytorch_distributed_examples_amd.data.mnist import MNIST
    from pytorch_distributed_examples_amd.utils.epoch_graph import ChunkedGraphs, EpochBatches

    ds = MNIST(exported, train=True, device=gpu, limit=1024 + 40)
    runs = []
    for d in (ds, Twin(ds)):
        eb = EpochBatches(ShardedLoader(d, 128, 1, 0, shuffle=True))
        seen = []

        def step(x, y):
            loss = torch.zeros((), device=x.device)
            loss.inputs = (x.clone(), y.clone())  # static buffers of the graph when captured: copied out below
            return loss

        def on_steps(idxs, outs):
            seen.extend((b, o.inputs[0].clone(), o.inputs[1].clone()) for b, o in zip(idxs, outs))

        runner = ChunkedGraphs(step, eb, chunk=3, eager_first=1)
        for epoch in (0, 1):
            eb.fill(epoch)
            runner.run(on_steps=on_steps)
        torch.cuda.synchronize()
        assert runner.replays >= 5 and [b for b, _, _ in seen] == list(range(9)) * 2
        assert [x.shape[0] for _, x, _ in seen] == ([128] * 8 + [40]) * 2
        runs.append(seen)
    for (_, xa, ya), (_, xb, yb) in zip(*runs):
        assert torch.equal(xa, xb) and torch.equal(ya, yb)
    assert not torch.equal(runs[0][0][1], runs[0][9][1])  # (the two epochs differ: the replays read refilled data)


def test_mnist_ddp_entry_on_exported_dir(gpu, exported, tmp_path, capsys):
    from pytorch_distributed_examples_amd.apps import mnist_ddp

    mnist_ddp.main(["2", "1", "--model", "cnn", "--batch_size", "64", "--train_size", "2048", "--test_size", "512",
                    "--data_dir", str(exported), "--snapshot_path", str(tmp_path / "snapshot.pt"),
                    "--metrics", str(tmp_path / "m.jsonl")])
    out = capsys.readouterr().out
    assert "Batchsize: 64 | Steps: 32" in out and "images/s (node)" in out and "Execution time" in out
    accs = [float(s.split("%")[0]) for s in out.split("Test accuracy: ")[1:]]  # (one per epoch)
    rows = [json.loads(l) for l in open(tmp_path / "m.jsonl")]
    print("ddp losses", [r["loss"] for r in rows], "accuracies", accs)
    assert len(accs) == 2 and all(0.0 <= a <= 100.0 for a in accs)
    assert len(rows) == 2 and all(math.isfinite(r["loss"]) for r in rows)
    assert rows[1]["loss"] < rows[0]["loss"] + 0.5


def test_mnist_hvd_entry_on_exported_dir(gpu, exported, capsys):
    from pytorch_distributed_examples_amd.apps import mnist_hvd

    mnist_hvd.main(["--epochs", "2", "--batch-size", "64", "--train-size", "2048", "--log-interval", "5",
                    "--graph-chunk", "4", "--data-dir", str(exported)])
    out = capsys.readouterr().out
    losses = []
    for epoch in (0, 1):
        lines = [l for l in out.splitlines() if l.startswith(f"Worker: 0 | Epoch: {epoch} | Batch:")]
        assert [int(l.split("Batch: ")[1].split("/")[0]) for l in lines] == list(range(0, 32, 5))
        assert all(l.split("Batch: ")[1].split(" ")[0].endswith("/32") for l in lines)
        losses.append([float(l.rsplit("Loss: ", 1)[1]) for l in lines])
    print("hvd losses", losses)
    assert all(math.isfinite(v) for ep in losses for v in ep)
    assert losses[1][-1] < losses[0][-1] + 0.5
    assert "images/s (node)" in out and "images/s (this worker)" in out
