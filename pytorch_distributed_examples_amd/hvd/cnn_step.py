"""GPU training step of the Horovod MNIST CNN scripts with ANY wrapped optimiser (horovod_mnist_elastic.py uses
AdamW, :41-42), captured into a hipGraph.

    step = FusedHvdStep(model, optimizer, batch)   # optimizer = hvd.DistributedOptimizer(FusedAdamW(...))
    loss = step(x, y)                              # forward + backward + all-reduce + AdamW
    step.reset()                                   # after an elastic reset (new engine / world size)

* forward + backward: the whole-network fused kernel (:class:`..models.cnn_fused.FusedCNN`), gradients written
  into ``p.grad`` views of ONE flat buffer -- so the fusion engine reduces the batch in place (one xGMI one-shot
  exchange, no pack / unpack) -- with the bf16 weight-fragment image rebuilt from the fp32 weights inside the
  kernel every step (``always_prep``: the optimiser is not the fused SGD);
* ``optimizer.step()``: ``synchronize()`` (the engine; in graph mode stream-ordered on the caller's stream) then the
  wrapped multi-tensor optimiser (FusedAdamW: hyper-parameters and step count in device memory);
* the first call after construction or :meth:`reset` runs eagerly through the engine -- it negotiates the gradient
  names into the response cache -- then ``enable_graph_mode`` and the step is captured: every later full-batch call
  is ONE graph replay (the batch copied into the graph's static slots).  A short last batch runs eagerly.
  :meth:`reset` drops the graph (the xGMI view, the world size and the learning rate are baked into it).
* ``hvd.DistributedOptimizer(opt, op=hvd.Adasum)`` around a one-group FusedSGD / FusedAdam / FusedAdamW on the xGMI
  plane: the step is ``forward_backward(grad_out)`` + :meth:`FusedCNN.adasum_step` on the engine's xGMI instance, on
  the caller's stream -- FOUR launches (``k_cnn_train``, ``k_cnn_reduce<0>``, ``k_cnn_adasum_delta``,
  ``k_cnn_adasum_apply``), under the rule of ``allreduce_inline_``: graph mode, engine parked.  So the first call
  still takes ``forward_backward`` + ``opt.step()`` through the engine (it negotiates the delta names) and turns
  graph mode on, the second is the first fused one (it makes the fragment image current) and the third is captured.
  Without an xGMI plane, with an optimiser :func:`fused_update_mode` rejects, or with ``PDE_CNN_ADASUM_FUSED=0`` (the
  A/B switch), every step is ``forward_backward`` + ``opt.step()``: the same numbers through the optimiser's
  ``_foreach`` copies and the stand-alone exchange.
"""
from __future__ import annotations

import os

import torch

from ..models.cnn_fused import FusedCNN, fused_update_mode


def adasum_update_mode(opt) -> int | None:
    """The fused update mode (:func:`..models.cnn_fused.fused_update_mode`) of an ``hvd.DistributedOptimizer(...,
    op=hvd.Adasum)`` whose local step the Adasum launches of the fused CNN can take; ``None`` for an optimiser that
    is not an Adasum wrapper or wraps anything else.  Pure: needs no native module."""
    return fused_update_mode(opt) if getattr(opt, "_adasum", False) else None


def adasum_fused_enabled() -> bool:
    """``PDE_CNN_ADASUM_FUSED=0`` keeps an Adasum optimiser on ``forward_backward`` + ``opt.step()`` (A/B runs)."""
    return os.environ.get("PDE_CNN_ADASUM_FUSED", "1") != "0"


class FusedHvdStep:
    def __init__(self, model, optimizer, batch: int, graph: bool = True):
        self.model, self.opt, self.batch = model, optimizer, int(batch)
        self.fused = FusedCNN(model)
        from ..models.cnn_fused import opt_in_reduce_enabled

        # a one-group FusedSGD (the DP script, mnist_horovod.py:50; any momentum / weight decay), FusedAdamW (the
        # elastic script) or FusedAdam: the update rides in the fused kernel's slab reduction at world 1, else it is
        # ONE launch after the engine's synchronize that also refreshes the bf16 fragment image (FusedCNN.opt_step)
        # -- the bench's hvd_cnn step.  PDE_CNN_OPT_IN_REDUCE=0 keeps Adam / AdamW on the launch of their own at
        # world 1 too.  Anything else: the wrapped optimiser's own step, fragments rebuilt in-kernel.
        self.mode = fused_update_mode(optimizer)
        # an Adasum wrapper reduces weight deltas in step(), never gradients: the routes below that all-reduce
        # gradients are not its; adasum_mode: the local update its fused route takes
        self.adasum = bool(getattr(optimizer, "_adasum", False))
        self.adasum_mode = adasum_update_mode(optimizer) if adasum_fused_enabled() else None
        self.adasum_steps = 0  # steps taken by the two Adasum launches
        sgd = self.mode in (0, 1) and not self.adasum
        self.in_reduce = self.mode in (0, 1) or (self.mode is not None and opt_in_reduce_enabled())
        self.fused.always_prep = self.mode is None
        if not sgd:
            from ..ops import functional as OF

            # the kernel rebuilds its fragment image from the fp32 weights every step: the optimiser need not keep
            # the layer path's bf16 conv / linear layouts current (an eager model(x) falls back to cached copies)
            for p in model.parameters():
                p.__dict__["_pde_own_copies"] = True
                OF.release_compute_copies(p)
        self.grads = self.fused.grad_buffer()  # p.grad: views of one flat buffer (never set to None)
        self.use_graph = graph
        self.graph = None
        self.negotiated = False
        self.replays = 0

    def _eager(self, x, y):
        if self.mode is None:
            loss = self.fused.forward_backward(x, y, grad_out=self.grads)
            self.opt.step()
            return loss
        from . import core

        if self.in_reduce and core.size() == 1:  # all-reduce = identity: the update inside the reduction kernel
            self.opt.synchronize()
            return self.fused.forward_backward(x, y, grad_out=self.grads, opt=self.opt)
        if self.adasum:
            # the fallback's opt.step() writes the weights with _foreach kernels: where it is every step, the
            # kernel rebuilds its fragment image every step too
            self.fused.always_prep = not self._adasum_capable()
            loss = self.fused.forward_backward(x, y, grad_out=self.grads)
            if self.negotiated and self._adasum_capable():  # graph mode: the engine is parked, its xGMI instance ours
                self.fused.adasum_step(self.opt, self.grads, core._ctx.xgmi)
                self.adasum_steps += 1
            else:
                self.opt.step()
            return loss
        loss = self.fused.forward_backward(x, y, grad_out=self.grads)
        self.opt.synchronize()  # the engine (graph mode: stream-ordered on this stream)
        with self.opt.skip_synchronize():
            self.fused.opt_step(self.opt, self.grads)
        return loss

    def _adasum_capable(self) -> bool:
        """The two Adasum launches can take this optimiser's step: a fused update mode, the switch on, and the
        engine's xGMI plane over more than one rank."""
        from . import core

        return self.adasum_mode is not None and core.size() > 1 and core._ctx.xgmi is not None

    @property
    def route(self) -> str:
        """Where a full step goes once negotiated: ``adasum_fused`` (the two Adasum launches), ``adasum_fallback``
        (``forward_backward`` + the Adasum optimiser's own ``step()``), ``in_reduce`` (world 1: the update inside
        the reduction kernel), ``opt_step`` (engine all-reduce + the one-launch update) or ``optimizer``."""
        from . import core

        if self.mode is not None and self.in_reduce and core.size() == 1:
            return "in_reduce"
        if self.adasum:
            return "adasum_fused" if self._adasum_capable() else "adasum_fallback"
        return "optimizer" if self.mode is None else "opt_step"

    def kernel_launches_per_step(self) -> int | None:
        """Kernel launches of one negotiated step with a current fragment image: 4 on the fused Adasum route
        (training, reduction, delta + exchange + Gram, apply), 2 with the update inside the reduction, 3 plus the
        engine's exchange with the one-launch update; ``None`` where the wrapped optimiser's own step decides."""
        return {"adasum_fused": 4, "in_reduce": 2, "opt_step": 3}.get(self.route)

    def eager_step(self, x, y):
        """One eager step; the first one negotiates through the engine and turns graph mode on, so every later call
        is capturable (an epoch-graph runner, utils/epoch_graph.py, captures this function)."""
        loss = self._eager(x, y)
        if not self.negotiated:
            torch.cuda.synchronize()
            self.opt.enable_graph_mode()
            self.negotiated = True
        return loss

    def __call__(self, x, y):
        if not self.use_graph or x.shape[0] != self.batch:
            return self._eager(x, y)
        if self.graph is None:
            if not self.negotiated:  # one step through the engine: every gradient enters the response cache
                loss = self._eager(x, y)
                torch.cuda.synchronize()
                self.opt.enable_graph_mode()
                self.negotiated = True
                return loss
            if self.adasum and self._adasum_capable() and self.adasum_steps == 0:
                # the negotiated step went through opt.step(): one eager step on the Adasum launches makes the
                # fragment image current, so the captured step carries no prep launch
                return self._eager(x, y)
            from ..utils.graph import CapturedStep

            # no warm-up steps: the negotiated eager step already initialised everything (a warm-up would train
            # one extra step on this batch)
            self.graph = CapturedStep(self._eager, [x, y], warmup=0).capture()
        self.replays += 1
        return self.graph(x, y)

    def reset(self):
        """After an elastic reset: drop the graph and negotiate again through the new engine."""
        self.graph = None
        self.negotiated = False
        self.adasum_steps = 0
        if hasattr(self.opt, "disable_graph_mode"):
            self.opt.disable_graph_mode()
        self.fused.invalidate()
