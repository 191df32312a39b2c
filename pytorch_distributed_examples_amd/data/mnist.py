"""The real MNIST files (reference: ``datasets.MNIST`` + ``ToTensor`` + ``Normalize((0.1307,), (0.3081,))``,
mnist_ddp_elastic.py:166-169, mnist_horovod.py:34-38, horovod_mnist_elastic.py:44-50).

* :func:`read_idx` / :func:`write_idx` -- the IDX container (big-endian magic ``0x00000803`` uint8 images
  ``[N, 28, 28]`` / ``0x00000801`` uint8 labels ``[N]``, dimension words, payload), plain or ``.gz``.
* :func:`find_mnist` -- the four standard file names under ``root``, ``root/MNIST/raw`` (torchvision's layout) or
  ``root/raw``.  Nothing is ever downloaded.
* :class:`MNIST` -- the split as BYTES on the device: ``images_u8`` uint8 ``[N, 784]`` (47 MB for the train split
  against 188 MB in fp32) and the 256 possible normalised pixels as ``table``.  A batch is expanded to fp32 inside
  the gather that builds it (:meth:`MNIST.gather`: on a GPU one launch of csrc/kernels/elementwise.hip
  ``k_gather_rows_u8``, ``x = table[images_u8[idx]]``).  There is deliberately no fp32 ``images`` tensor.
* :func:`mnist_datasets` -- what the entry scripts call: the synthetic splits without a data directory, two
  :class:`MNIST` objects with one.
* ``python -m pytorch_distributed_examples_amd.data.mnist export DIR [--train N] [--test M] [--gz]`` writes the
  synthetic set as the four IDX files (for tests, and for anyone without the real files).
"""
from __future__ import annotations

import gzip
import os
import struct
import sys

import torch
from torch.utils.data import Dataset

from .synthetic import MNIST_MEAN, MNIST_STD

MAGIC_IMAGES, MAGIC_LABELS = 0x00000803, 0x00000801
FILES = {
    (True, "images"): "train-images-idx3-ubyte",
    (True, "labels"): "train-labels-idx1-ubyte",
    (False, "images"): "t10k-images-idx3-ubyte",
    (False, "labels"): "t10k-labels-idx1-ubyte",
}


def _open(path, mode):
    return gzip.open(path, mode) if str(path).endswith(".gz") else open(path, mode)


def read_idx(path) -> torch.Tensor:
    """The uint8 tensor of an IDX file: ``[N, 28, 28]``-style images (rank 3) or labels (rank 1)."""
    with _open(path, "rb") as f:
        data = f.read()
    if len(data) < 4:
        raise ValueError(f"{path}: not an IDX file (only {len(data)} bytes)")
    magic = struct.unpack(">I", data[:4])[0]
    if magic >> 8 != MAGIC_IMAGES >> 8:  # two zero bytes, then the element type: 0x08 = uint8
        raise ValueError(f"{path}: bad IDX magic 0x{magic:08x} (expected 0x{MAGIC_IMAGES:08x} uint8 images or "
                         f"0x{MAGIC_LABELS:08x} uint8 labels)")
    rank = magic & 0xFF
    if rank not in (1, 3):
        raise ValueError(f"{path}: IDX rank {rank} is not supported (1: labels, 3: images)")
    if len(data) < 4 + 4 * rank:
        raise ValueError(f"{path}: truncated IDX header")
    dims = struct.unpack(f">{rank}I", data[4:4 + 4 * rank])
    count = 1
    for d in dims:
        count *= d
    payload = len(data) - 4 - 4 * rank
    if payload != count:
        raise ValueError(f"{path}: dimensions {list(dims)} need {count} payload bytes, the file has {payload}")
    if count == 0:
        return torch.empty(dims, dtype=torch.uint8)
    return torch.frombuffer(bytearray(data[4 + 4 * rank:]), dtype=torch.uint8).reshape(dims)


def write_idx(path, tensor: torch.Tensor) -> None:
    """Write a uint8 tensor of rank 1 (labels) or 3 (images) as an IDX file (``.gz`` name: compressed)."""
    t = torch.as_tensor(tensor)
    if t.dtype != torch.uint8 or t.dim() not in (1, 3):
        raise ValueError(f"{path}: write_idx takes a uint8 tensor of rank 1 or 3, got {t.dtype} rank {t.dim()}")
    t = t.detach().cpu().contiguous()
    head = struct.pack(">I", 0x00000800 | t.dim()) + struct.pack(f">{t.dim()}I", *t.shape)
    with _open(path, "wb") as f:
        f.write(head)
        f.write(t.numpy().tobytes())


def find_mnist(root) -> dict:
    """Paths of the four MNIST files: ``{(train, "images" | "labels"): path}``.  Each name is tried plain, then
    ``.gz``, in ``root``, ``root/MNIST/raw``, ``root/raw``.  Never downloads: a missing file is an error."""
    root = os.fspath(root)
    dirs = [root, os.path.join(root, "MNIST", "raw"), os.path.join(root, "raw")]
    found = {}
    for key, name in FILES.items():
        tried = [os.path.join(d, name + ext) for d in dirs for ext in ("", ".gz")]
        hit = next((p for p in tried if os.path.isfile(p)), None)
        if hit is None:
            raise FileNotFoundError(f"MNIST file {name} not found (nothing is downloaded); tried: " + ", ".join(tried))
        found[key] = hit
    return found


def pixel_table(device="cpu") -> torch.Tensor:
    """The normalised value of each of the 256 pixel bytes: ``ToTensor`` (``/ 255``) then ``Normalize`` -- this
    arithmetic, in this order, is the definition of a normalised pixel (the fused form
    ``x * (1 / 255 / std) - mean / std`` differs from it in most of the 256 values)."""
    return torch.arange(256, dtype=torch.float32).div(255).sub(MNIST_MEAN).div(MNIST_STD).to(device)


class MNIST(Dataset):
    """One MNIST split held as bytes on ``device``; see the module docstring."""

    sample_shape = (1, 28, 28)

    def __init__(self, root, train: bool = True, device="cpu", limit: int | None = None):
        files = find_mnist(root)
        images, labels = read_idx(files[(train, "images")]), read_idx(files[(train, "labels")])
        if images.dim() != 3 or tuple(images.shape[1:]) != self.sample_shape[1:]:
            raise ValueError(f"{files[(train, 'images')]}: expected [N, 28, 28] images, got {list(images.shape)}")
        if labels.dim() != 1 or labels.shape[0] != images.shape[0]:
            raise ValueError(f"{files[(train, 'labels')]}: {list(labels.shape)} labels for {images.shape[0]} images "
                             f"({files[(train, 'images')]})")
        if limit is not None:
            if limit > images.shape[0]:
                raise ValueError(f"{files[(train, 'images')]}: {limit} samples asked for, the file has "
                                 f"{images.shape[0]}")
            images, labels = images[:limit], labels[:limit]
        self.images_u8 = images.reshape(images.shape[0], -1).contiguous().to(device)
        self.labels = labels.to(torch.int64).to(device)
        self.table = pixel_table(device)

    @property
    def device(self):
        return self.images_u8.device

    def __len__(self):
        return self.labels.shape[0]

    def __getitem__(self, i):
        return self.table[self.images_u8[i].long()].view(self.sample_shape), self.labels[i]

    def gather(self, idx, out=None, start: int = 0, rows: int | None = None):
        """``x[k] = table[images_u8[idx[start + k]]]`` (fp32 ``[rows, 1, 28, 28]``), ``y[k] = labels[idx[start + k]]``
        for ``k < rows`` (default: the rest of ``idx``), written into ``out = (x, y)`` when given.  On a GPU: one
        launch of the uint8 gather kernel; on the CPU plain indexing."""
        rows = idx.numel() - start if rows is None else rows
        if rows < 0 or start < 0 or start + rows > idx.numel():
            raise ValueError(f"gather: rows [{start}, {start + rows}) of {idx.numel()} indices")
        if out is None:
            out = (torch.empty((rows,) + self.sample_shape, dtype=torch.float32, device=self.device),
                   torch.empty(rows, dtype=torch.int64, device=self.device))
        x, y = out
        if tuple(x.shape) != (rows,) + self.sample_shape or tuple(y.shape) != (rows,):
            raise ValueError(f"gather: out must be ([{rows}, 1, 28, 28], [{rows}]), got {list(x.shape)}, {list(y.shape)}")
        if rows == 0:
            return x, y
        if self.images_u8.is_cuda:
            from .. import _native

            _native.C().gather_rows_u8(self.images_u8, self.labels, idx, self.table, x, y, start)
        else:
            sl = idx[start:start + rows]
            x.copy_(self.table[self.images_u8.index_select(0, sl).long()].view(x.shape))
            y.copy_(self.labels.index_select(0, sl))
        return x, y


def mnist_datasets(device, train: int, test: int, data_dir=None):
    """(train set, test set) of the MNIST entry scripts: the synthetic splits, or with ``data_dir`` the first
    ``train`` / ``test`` samples of the IDX files found there."""
    if data_dir is None:
        from .synthetic import mnist_splits

        return mnist_splits(device=device, train=train, test=test)
    return (MNIST(data_dir, train=True, device=device, limit=train),
            MNIST(data_dir, train=False, device=device, limit=test))


def quantise(x: torch.Tensor) -> torch.Tensor:
    """Normalised fp32 pixels back to bytes (the export's rounding)."""
    return ((x * MNIST_STD + MNIST_MEAN) * 255).round().clamp(0, 255).to(torch.uint8)


def export(out_dir, train: int = 60000, test: int = 10000, gz: bool = False) -> dict:
    """Write the synthetic set as the four IDX files into ``out_dir``; returns their paths (keys as FILES)."""
    from .synthetic import mnist_splits

    os.makedirs(out_dir, exist_ok=True)
    tr, te = mnist_splits(device="cpu", train=train, test=test)
    paths = {}
    for is_train, ds in ((True, tr), (False, te)):
        for kind, t in (("images", quantise(ds.images).view(-1, 28, 28)), ("labels", ds.labels.to(torch.uint8))):
            p = os.path.join(os.fspath(out_dir), FILES[(is_train, kind)] + (".gz" if gz else ""))
            write_idx(p, t)
            paths[(is_train, kind)] = p
    return paths


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(prog="python -m pytorch_distributed_examples_amd.data.mnist",
                                 description="MNIST IDX tools (nothing is ever downloaded)")
    sub = ap.add_subparsers(dest="cmd", required=True)
    ex = sub.add_parser("export", help="write the synthetic set as the four MNIST IDX files")
    ex.add_argument("dir")
    ex.add_argument("--train", type=int, default=60000)
    ex.add_argument("--test", type=int, default=10000)
    ex.add_argument("--gz", action="store_true", help="gzip the files")
    args = ap.parse_args(argv)
    for p in export(args.dir, args.train, args.test, args.gz).values():
        print(p)


if __name__ == "__main__":
    main(sys.argv[1:])
