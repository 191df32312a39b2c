"""Evaluation of the elastic-DDP MLP in ONE launch per call (csrc/kernels/mlp_eval.hip, ``k_mlp_eval``).

Reference: the per-epoch test pass of pytorch_elastic/mnist_ddp_elastic.py:117-130 over the ``Model`` of :133-159;
model of :mod:`.mlp`::

    ev = FusedMLPEval(model)
    pred = ev.predict(x)                          # int64 [B]; logits=True / logprobs=True add the fp32 [B, 10] tensors
    stats = CnnEvalStats(dev)
    for x, y in loader:
        ev.evaluate(x, y, stats)                  # totals accumulate on the device, no host synchronisation
    loss_sum, correct, count = stats.result()     # one device-to-host copy per pass

A workgroup carries 32 batch rows through every layer with the activations in LDS and the weights streamed straight
into MFMA fragments; log-softmax, argmax, the hit count and the summed NLL are taken in the same launch.  Numbers
are those of the layer path (``model(x)``): bf16 operands and hand-offs, fp32 accumulation and bias.  The weights
are the layers' own bf16 copies (``ops.functional._bf16_weight``), looked up on every call -- the tensors
``k_mlp_train`` refreshes in place -- so a replayed training graph or a ``load_state_dict`` is seen exactly as
``model(x)`` sees it.  ``evaluate`` / ``predict`` write nothing but their outputs.

A small batch is latency-bound here (every workgroup streams all weights: 4 workgroups at B = 128), so
:func:`mlp_eval_pass`, the entry scripts' test pass, evaluates a rank's shard in chunks of up to 16,384 rows when
the dataset holds whole tensors.
"""
from __future__ import annotations

import os

import torch

from .. import _native
from ..ops import functional as OF
from .cnn_fused import CnnEvalStats

PASS_CHUNK = 16384  # rows per launch of mlp_eval_pass


def mlp_eval_enabled() -> bool:
    """The entry scripts' MLP test passes run through :meth:`FusedMLPEval.evaluate`; ``PDE_MLP_EVAL=0`` keeps the
    layer-by-layer pass (A/B runs)."""
    return os.environ.get("PDE_MLP_EVAL", "1") != "0"


class FusedMLPEval:
    def __init__(self, net):
        self.net = net
        self.layers = [net.input_layer, *net.hidden_layers, net.final_layer]
        for i, L in enumerate(self.layers):
            assert L.bias is not None and L.relu == (i < len(self.layers) - 1), "Linear+ReLU stack, plain last layer"
        self._part: dict = {}  # the totals' per-workgroup partials, one buffer per (grid, device): no allocation later

    def _eval(self, x, y, stats, want_pred, want_logits, want_logp):
        C = _native.C()
        x = x.reshape(x.shape[0], -1).float().contiguous()
        part = None
        if stats is not None:
            y = y.long().contiguous()
            grid = -(-x.shape[0] // C.mlp_eval_rows_per_workgroup())
            key = (grid, str(x.device))
            if key not in self._part:
                self._part[key] = torch.empty(grid, dtype=torch.float32, device=x.device)
            part = self._part[key]
        return C.mlp_eval(x, y, [OF._bf16_weight(L.weight) for L in self.layers],
                          [L.bias.detach() for L in self.layers], want_pred, want_logits, want_logp,
                          None if stats is None else stats.buf, part)

    @torch.no_grad()
    def predict(self, x: torch.Tensor, logits: bool = False, logprobs: bool = False):
        """Predicted class of every row (int64 ``[B]``, lowest index on a tie); with ``logits`` / ``logprobs`` also
        the fp32 ``[B, classes]`` last-layer outputs / log-probabilities, in that order: ``(pred, logits, logp)``."""
        pred, lg, lp = self._eval(x, None, None, True, logits, logprobs)
        out = (pred,) + ((lg,) if logits else ()) + ((lp,) if logprobs else ())
        return out if len(out) > 1 else pred

    @torch.no_grad()
    def evaluate(self, x: torch.Tensor, y: torch.Tensor, stats: CnnEvalStats | None = None, logprobs: bool = False):
        """Add the batch's summed NLL, correct predictions and row count to ``stats`` (a new :class:`CnnEvalStats`
        when ``None``) without any host synchronisation; returns ``stats``, or ``(stats, logp)`` with ``logprobs``."""
        if stats is None:
            stats = CnnEvalStats(x.device)
        _, _, lp = self._eval(x, y, stats, False, False, logprobs)
        return (stats, lp) if logprobs else stats


@torch.no_grad()
def mlp_eval_pass(evaluator_or_model, loader, device):
    """One test pass over ``loader`` (a :class:`..data.loader.ShardedLoader`): ``(correct, total, loss_sum)``.

    On the GPU (``PDE_MLP_EVAL`` not 0) through :class:`FusedMLPEval`: when the dataset holds whole tensors
    (``images`` or ``images_u8``) the rank's shard, in sampler order, in chunks of up to ``PASS_CHUNK`` rows -- one
    gather and one launch each -- otherwise one launch per loader batch; the counts stay on the device until the pass
    ends.  Else the layer pass (``model(images)`` per batch, the count through ATen), which takes no loss:
    ``loss_sum`` is ``None``."""
    ev = evaluator_or_model if isinstance(evaluator_or_model, FusedMLPEval) else None
    model = ev.net if ev is not None else evaluator_or_model
    device = torch.device(device)
    if device.type != "cuda" or not mlp_eval_enabled():
        total = 0
        correct = torch.zeros((), dtype=torch.long, device=device)
        for images, labels in loader:
            predicted = model(images).float().argmax(1)
            total += labels.size(0)
            correct += (predicted == labels).sum()
        return int(correct.item()), total, None
    if ev is None:
        ev = FusedMLPEval(getattr(model, "module", model))
    stats = CnnEvalStats(device)
    ds = loader.dataset
    images, u8 = getattr(ds, "images", None), getattr(ds, "images_u8", None)
    if u8 is not None or images is not None:
        idx = torch.tensor(list(iter(loader.sampler)), dtype=torch.long).to(u8.device if u8 is not None
                                                                            else images.device)
        total = idx.numel()
        for i in range(0, total, PASS_CHUNK):
            sl = idx[i:i + PASS_CHUNK]
            x, y = ds.gather(sl) if u8 is not None else (images.index_select(0, sl), ds.labels.index_select(0, sl))
            ev.evaluate(x.to(device), y.to(device), stats)
    else:
        total = 0
        for x, y in loader:
            ev.evaluate(x.to(device), y.to(device), stats)
            total += y.size(0)
    loss_sum, correct, count = stats.result()
    assert count == total, (count, total)
    return correct, total, loss_sum
