"""FP8 (OCP e4m3 / e5m2) plumbing for the HIP kernels of ``csrc/kernels/gemm_fp8.hip``: the format constants, the
zero-padded byte buffers the GEMM reads, the per-tensor scale records and the quantiser's launch tables.

Scaling is per tensor, a power of two, delayed by one step: a tensor is quantised with the scale its record holds,
the kernels fold its unscaled ``max |x|`` into the record's ``amax`` word, and ``ScaleRecords.update()`` (one tiny
launch at the end of the step) turns that into the next step's scale.  Everything lives in device memory, so a step
can be captured in a hipGraph.
"""
from __future__ import annotations

import torch

from .. import _native

E4M3, E5M2 = 0, 1  # the MFMA's operand-format codes
FMT_MAX = {E4M3: 448.0, E5M2: 57344.0}
TORCH_DTYPE = {E4M3: torch.float8_e4m3fn, E5M2: torch.float8_e5m2}


def pad128(n: int) -> int:
    return (n + 127) // 128 * 128


def buffer(rows: int, cols: int, dev) -> torch.Tensor:
    """FP8 bytes [rows][cols padded to 128], zero (0x00 is +0 in both formats): a GEMM operand with K = cols."""
    return torch.zeros(rows, pad128(cols), dtype=torch.uint8, device=dev)


def decode(buf: torch.Tensor, fmt: int) -> torch.Tensor:
    """The values an FP8 byte buffer holds, as fp32 (for tests and inspection)."""
    return buf.view(TORCH_DTYPE[fmt]).float()


class ScaleRecords:
    """``[T][4]`` fp32 on the device: {scale, 1 / scale, amax, format max} per tensor; scales start at 1."""

    def __init__(self, formats, dev):
        rec = torch.tensor([[1.0, 1.0, 0.0, FMT_MAX[f]] for f in formats], dtype=torch.float32)
        self.t = rec.to(dev)
        self.formats = list(formats)

    def update(self) -> None:
        """scale = 2^floor(log2(format max / amax)) where amax is finite and not 0; amax = 0."""
        _native.C().fp8_scales(self.t)

    def scales(self) -> list:
        return self.t[:, 0].tolist()


def quantise(records: ScaleRecords, fmt: int, src, dst, dst_t, rec: int) -> None:
    """One tensor, one launch, no state: ``src`` (fp32 or bf16 ``[rows][cols]`` row view, any address) -> ``dst`` and,
    unless ``dst_t`` is None, the transposed ``dst_t``, with the scale of record ``rec``."""
    none = torch.empty(0, dtype=torch.uint8, device=src.device) if dst_t is None else dst_t
    _native.C().fp8_quant_one(src, dst, none, records.t, rec, fmt)


class QuantPlan:
    """Several tensors in one launch (the weights of a model): ``srcs[i]`` -> ``dsts[i]`` and, where given, the
    transposed ``dsts_t[i]``, all in format ``fmt`` with the scales of records ``rec[i]``.  The device table is
    built once, for tensors whose addresses stay (parameters); it keeps them alive."""

    def __init__(self, records: ScaleRecords, fmt: int, srcs, dsts, dsts_t, rec):
        self.records, self.fmt, self.n = records, fmt, len(srcs)
        self.keep = (list(srcs), list(dsts), list(dsts_t))
        none = torch.empty(0, dtype=torch.uint8, device=srcs[0].device)
        self.table, self.blocks_x = _native.C().fp8_quant_table(
            list(srcs), list(dsts), [none if t is None else t for t in dsts_t], list(rec), records.t)

    def run(self) -> None:
        t = self.records.t
        _native.C().fp8_quant(self.table, self.n, self.blocks_x, t, self.fmt, t.shape[0])
