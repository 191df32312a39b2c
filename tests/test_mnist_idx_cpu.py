"""The MNIST IDX path on the CPU (data/mnist.py): the file format and its errors, the search for the four files,
the byte dataset's gather against the definition of a normalised pixel, the loaders against an fp32 twin, the
export command and an entry script on an exported directory."""
import gzip
import os
import struct

import pytest
import torch

from pytorch_distributed_examples_amd.data import mnist as M
from pytorch_distributed_examples_amd.data.synthetic import MNIST_MEAN, MNIST_STD

NAMES = ["train-images-idx3-ubyte", "train-labels-idx1-ubyte", "t10k-images-idx3-ubyte", "t10k-labels-idx1-ubyte"]


def _normalise(u8):
    """ToTensor + Normalize on bytes: the definition of a normalised pixel."""
    return u8.to(torch.float32).div(255).sub(MNIST_MEAN).div(MNIST_STD)


class Twin:
    """The fp32 form of a byte dataset, as the loaders have always taken it (``images`` / ``labels``)."""

    def __init__(self, ds):
        self.images = _normalise(ds.images_u8).view(-1, 1, 28, 28)
        self.labels = ds.labels.clone()

    def __len__(self):
        return self.labels.shape[0]


@pytest.fixture(scope="module")
def exported(tmp_path_factory):
    d = tmp_path_factory.mktemp("mnist_idx")
    M.export(d, train=1000, test=256)
    return d


# -- the IDX container ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", ["", ".gz"])
def test_idx_round_trip(tmp_path, ext):
    g = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (37, 28, 28), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 10, (37,), generator=g, dtype=torch.uint8)
    pi, pl = tmp_path / ("images-idx3-ubyte" + ext), tmp_path / ("labels-idx1-ubyte" + ext)
    M.write_idx(pi, images)
    M.write_idx(pl, labels)
    raw = (gzip.open if ext else open)(pi, "rb").read()
    assert raw[:16] == struct.pack(">IIII", 0x00000803, 37, 28, 28) and len(raw) == 16 + 37 * 784
    assert (gzip.open if ext else open)(pl, "rb").read()[:8] == struct.pack(">II", 0x00000801, 37)
    if ext:
        assert open(pi, "rb").read(2) == b"\x1f\x8b"  # really compressed
    ri, rl = M.read_idx(pi), M.read_idx(pl)
    assert ri.dtype == torch.uint8 and ri.shape == (37, 28, 28) and torch.equal(ri, images)
    assert rl.dtype == torch.uint8 and rl.shape == (37,) and torch.equal(rl, labels)


@pytest.mark.parametrize("case,blob", [
    ("wrong-magic", struct.pack(">II", 0x00000D01, 4) + bytes(4)),
    ("one-short", struct.pack(">IIII", 0x00000803, 2, 28, 28) + bytes(2 * 784 - 1)),
    ("one-long", struct.pack(">IIII", 0x00000803, 2, 28, 28) + bytes(2 * 784 + 1)),
    ("rank-2", struct.pack(">III", 0x00000802, 3, 5) + bytes(15)),
])
def test_read_idx_rejects(tmp_path, case, blob):
    p = tmp_path / f"{case}-idx"
    p.write_bytes(blob)
    with pytest.raises(ValueError) as e:
        M.read_idx(p)
    assert str(p) in str(e.value)


# -- find_mnist ----------------------------------------------------------------------------------------------------
def _touch_all(d, ext=""):
    os.makedirs(d, exist_ok=True)
    for n in NAMES:
        open(os.path.join(d, n + ext), "wb").close()


@pytest.mark.parametrize("sub", ["", os.path.join("MNIST", "raw"), "raw"])
def test_find_mnist_layouts(tmp_path, sub):
    d = os.path.join(tmp_path, sub)
    _touch_all(d)
    found = M.find_mnist(tmp_path)
    assert sorted(found.values()) == sorted(os.path.join(d, n) for n in NAMES)
    assert found[(True, "images")].endswith(NAMES[0]) and found[(False, "labels")].endswith(NAMES[3])


def test_find_mnist_order_and_gz(tmp_path):
    _touch_all(os.path.join(tmp_path, "raw"))
    _touch_all(os.path.join(tmp_path, "MNIST", "raw"), ".gz")
    assert all(os.path.dirname(p) == os.path.join(tmp_path, "MNIST", "raw") and p.endswith(".gz")
               for p in M.find_mnist(tmp_path).values())  # MNIST/raw before raw; .gz when no plain file is there
    _touch_all(tmp_path, ".gz")
    open(os.path.join(tmp_path, NAMES[0]), "wb").close()
    found = M.find_mnist(tmp_path)
    assert found[(True, "images")] == os.path.join(tmp_path, NAMES[0])  # plain preferred over .gz
    assert found[(True, "labels")] == os.path.join(tmp_path, NAMES[1] + ".gz")


def test_find_mnist_missing_lists_paths(tmp_path):
    _touch_all(tmp_path)
    os.remove(os.path.join(tmp_path, NAMES[2]))
    with pytest.raises(FileNotFoundError) as e:
        M.find_mnist(tmp_path)
    for d in (str(tmp_path), os.path.join(tmp_path, "MNIST", "raw"), os.path.join(tmp_path, "raw")):
        for ext in ("", ".gz"):
            assert os.path.join(d, NAMES[2] + ext) in str(e.value)


# -- the dataset ---------------------------------------------------------------------------------------------------
def _write_set(d, images, labels, train=True):
    pre = "train" if train else "t10k"
    M.write_idx(os.path.join(d, f"{pre}-images-idx3-ubyte"), images)
    M.write_idx(os.path.join(d, f"{pre}-labels-idx1-ubyte"), labels)


def test_dataset_gather_is_the_definition_bitwise(tmp_path):
    g = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (40, 28, 28), generator=g, dtype=torch.uint8)
    images.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)  # every byte value
    labels = torch.randint(0, 10, (40,), generator=g, dtype=torch.uint8)
    _write_set(tmp_path, images, labels)
    _write_set(tmp_path, images[:8], labels[:8], train=False)
    ds = M.MNIST(tmp_path, train=True)
    assert not hasattr(ds, "images") and ds.sample_shape == (1, 28, 28) and len(ds) == 40
    assert ds.images_u8.dtype == torch.uint8 and ds.images_u8.shape == (40, 784) and ds.images_u8.is_contiguous()
    assert ds.labels.dtype == torch.int64 and torch.equal(ds.labels, labels.long())
    assert torch.equal(ds.table, _normalise(torch.arange(256, dtype=torch.uint8)))
    idx = torch.tensor([39, 0, 0, 17, 5, 39, 1])
    x, y = ds.gather(idx)
    assert x.dtype == torch.float32 and x.shape == (7, 1, 28, 28)
    assert torch.equal(x, _normalise(images[idx]).view(7, 1, 28, 28)) and torch.equal(y, labels[idx].long())
    assert ds.images_u8[0, :256].tolist() == list(range(256))
    xo, yo = torch.empty(3, 1, 28, 28), torch.empty(3, dtype=torch.long)
    rx, ry = ds.gather(idx, out=(xo, yo), start=2, rows=3)
    assert rx is xo and ry is yo and torch.equal(xo, x[2:5]) and torch.equal(yo, y[2:5])
    for k, i in enumerate(idx.tolist()):  # __getitem__ agrees with gather
        xi, yi = ds[i]
        assert xi.shape == (1, 28, 28) and torch.equal(xi, x[k]) and int(yi) == int(y[k])
    assert len(M.MNIST(tmp_path, train=False)) == 8 and len(M.MNIST(tmp_path, train=True, limit=11)) == 11
    with pytest.raises(ValueError):
        M.MNIST(tmp_path, train=True, limit=41)


def test_dataset_rejects_label_count(tmp_path):
    images = torch.zeros(5, 28, 28, dtype=torch.uint8)
    _write_set(tmp_path, images, torch.zeros(4, dtype=torch.uint8))
    _write_set(tmp_path, images, torch.zeros(5, dtype=torch.uint8), train=False)
    with pytest.raises(ValueError):
        M.MNIST(tmp_path, train=True)
    assert len(M.MNIST(tmp_path, train=False)) == 5


# -- loaders against the fp32 twin ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair(exported):
    ds = M.MNIST(exported, train=True)
    return ds, Twin(ds)


def test_exported_set_covers_every_byte(pair):
    assert len(pair[0]) == 1000 and pair[0].images_u8.unique().numel() == 256


@pytest.mark.parametrize("rank", [0, 1])
def test_sharded_loader_equals_fp32_twin(pair, rank):
    from pytorch_distributed_examples_amd.data.loader import ShardedLoader

    ds, twin = pair
    la, lb = (ShardedLoader(d, 64, 2, rank, shuffle=True) for d in (ds, twin))
    for epoch in (0, 1):
        la.set_epoch(epoch)
        lb.set_epoch(epoch)
        a, b = list(la), list(lb)
        assert len(a) == len(b) == 8 and [x.shape[0] for x, _ in a] == [64] * 7 + [52]
        for (xa, ya), (xb, yb) in zip(a, b):
            assert xa.dtype == torch.float32 and torch.equal(xa, xb) and torch.equal(ya, yb)


@pytest.mark.parametrize("rank", [0, 1])
def test_epoch_batches_equal_fp32_twin(pair, rank):
    from pytorch_distributed_examples_amd.data.loader import ShardedLoader
    from pytorch_distributed_examples_amd.utils.epoch_graph import EpochBatches

    ds, twin = pair
    ea, eb = (EpochBatches(ShardedLoader(d, 64, 2, rank, shuffle=True)) for d in (ds, twin))
    assert ea.x.dtype == torch.float32 and ea.x.shape == (500, 1, 28, 28)
    for epoch in (0, 1):
        ea.fill(epoch)
        eb.fill(epoch)
        assert len(ea) == len(eb) == 8
        for b in range(8):
            (xa, ya), (xb, yb) = ea.batch(b), eb.batch(b)
            assert xa.shape[0] == (64 if b < 7 else 52) and torch.equal(xa, xb) and torch.equal(ya, yb)


def test_mnist_datasets_switch(exported):
    from pytorch_distributed_examples_amd.data.synthetic import SyntheticMNIST

    tr, te = M.mnist_datasets("cpu", 64, 32)
    assert isinstance(tr, SyntheticMNIST) and len(tr) == 64 and len(te) == 32 and tr.images.shape == (64, 1, 28, 28)
    tr, te = M.mnist_datasets("cpu", 640, 200, data_dir=exported)
    assert isinstance(tr, M.MNIST) and len(tr) == 640 and len(te) == 200


# -- the export command and an entry script ------------------------------------------------------------------------
@pytest.mark.parametrize("gz", [False, True])
def test_export_command(tmp_path, capsys, gz):
    from pytorch_distributed_examples_amd.data.synthetic import mnist_splits

    M.main(["export", str(tmp_path), "--train", "96", "--test", "32"] + (["--gz"] if gz else []))
    assert sorted(os.listdir(tmp_path)) == sorted(n + (".gz" if gz else "") for n in NAMES)
    assert len(capsys.readouterr().out.split()) == 4
    tr, te = M.MNIST(tmp_path, train=True), M.MNIST(tmp_path, train=False)
    assert len(tr) == 96 and len(te) == 32
    s_tr, s_te = mnist_splits(train=96, test=32)
    for ds, syn in ((tr, s_tr), (te, s_te)):
        want = ((syn.images * MNIST_STD + MNIST_MEAN) * 255).round().clamp(0, 255).to(torch.uint8)
        assert torch.equal(ds.images_u8, want.view(-1, 784)) and torch.equal(ds.labels, syn.labels)
        # the bytes are the synthetic pixels to within half a quantisation step (1 / 255 / std = 0.0127)
        assert (ds.gather(torch.arange(len(ds)))[0] - syn.images).abs().max() < 0.5 / 255 / MNIST_STD + 1e-5


def test_mnist_ddp_entry_on_exported_dir_cpu(tmp_path, capsys):
    from pytorch_distributed_examples_amd.apps import mnist_ddp

    M.export(tmp_path / "data", train=512, test=256)
    mnist_ddp.main(["1", "1", "--device", "cpu", "--data_dir", str(tmp_path / "data"), "--train_size", "512",
                    "--test_size", "256", "--snapshot_path", str(tmp_path / "snapshot.pt")])
    out = capsys.readouterr().out
    assert "Batchsize: 128 | Steps: 4" in out and "Execution time" in out
    acc = float(out.split("Test accuracy: ")[1].split("%")[0])
    assert 0.0 <= acc <= 100.0
