"""Fused training step for the MNIST CNN (csrc/kernels/cnn_fused.hip).

:class:`FusedCNN` flattens a :class:`~.cnn.Net`'s parameters into ONE contiguous fp32 buffer in torch
parameter order (the ``nn.Parameter`` objects stay the same, their storage becomes views of the flat
buffer, so optimizers / ``state_dict`` / DDP keep working) and runs forward + NLL + backward of the
whole batch in one kernel launch plus one deterministic slab-reduction that writes the gradients
straight into a flat gradient buffer -- the DDP wrapper's, when it is laid out in forward order.

    fused = FusedCNN(net)
    ddp = DistributedDataParallel(net, overlap=False, param_order="forward")
    loss = fused.forward_backward(x, y, grad_out=ddp.flat_grad)   # grads written, no autograd
    ddp.sync_gradients(); opt.step()

Semantics match ``nll_loss(net(x), y)`` + ``backward()`` in train mode, including Dropout2d(p=0.5) on
conv2's output and dropout(p=0.5) on fc1's (fresh masks every call; dropout disabled in eval mode).

Fused optimiser step: the training kernel reads the conv weights as a bf16 MFMA fragment image that a prep
kernel writes from the fp32 parameters.  With ``sgd=opt`` (or ``opt=opt``) the slab reduction also applies the
optimiser update and rewrites the fragment slots of the weights it updates; :meth:`opt_step`, after a gradient
all-reduce that ran elsewhere, is the same update as one launch (:meth:`sgd_step` / :meth:`adam_step` /
:meth:`adamw_step` are :meth:`opt_step` behind a check of the optimiser's type).  Either way the next step skips
the prep launch.  Both go through one update descriptor of the native layer (``CnnUpdate``: mode, hyper-parameters,
step words, state) with one mode numbering.  ``opt`` is a one-group ``FusedSGD`` (plain -- the
reference's ``optim.SGD(lr=0.01)``, mnist_horovod.py:50 -- or with momentum and / or weight decay),
``FusedAdam`` or ``FusedAdamW`` (:func:`fused_update_mode`); the stateful ones keep ``momentum_buffer`` /
``exp_avg`` / ``exp_avg_sq`` as views of flat buffers, so ``state_dict()`` and ``opt.step()`` see the same state::

    opt = FusedSGD(net.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    loss = fused.forward_backward(x, y, grad_out=buf, sgd=opt)          # world 1: 2 launches per step
    loss = fused.forward_backward(x, y, grad_out=g, sgd=opt, xgmi=xa)   # world > 1 on one node: 2 launches
    loss = fused.forward_backward(x, y, grad_out=ddp.flat_grad)         # world > 1, any data plane:
    ddp.sync_gradients(); fused.opt_step(opt, ddp.flat_grad)            #   3 launches + all-reduce
    loss = fused.forward_backward(x, y, opt=adamw)                      # a FusedAdamW: AdamW in the reduction
    loss = fused.forward_backward(x, y, grad_out=g)                     # world 2 / 4 / 8 on one node, hvd.Adasum of
    fused.adasum_step(opt, g, xa)                                       #   the weight deltas: 4 launches

With ``xgmi`` (a :class:`..parallel.xgmi_allreduce.XgmiAllreduce` over the data-parallel ranks) the slab
reduction exchanges every workgroup's gradient chunk with all peers over xGMI inside the same kernel and
sums the ranks' chunks in rank order (``avg``: x 1/world), so ``grad_out`` receives the all-reduced
gradients, identical on every rank, and the update stays fused -- the all-reduce costs no launch.

The fragment image is re-derived (prep launch) whenever anything other than these fused updates may have
written the weights: any other optimiser step bumps the weight generation (:func:`.functional.
bump_weight_generation`); direct writes (``load_state_dict``, broadcasts) must call :meth:`invalidate`.

Evaluation runs on the same path (``k_cnn_eval``: the training kernel's forward, eval mode, one launch)::

    pred = fused.predict(x)                          # int64 [B]; logprobs=True: (pred, logp [B, 10])
    stats = CnnEvalStats(dev)
    for x, y in test_loader:
        fused.evaluate(x, y, stats)                  # no host synchronisation
    loss_sum, correct, count = stats.result()        # one device-to-host copy per pass
"""
from __future__ import annotations

import os

import torch

from .. import _native
from ..ops import functional as OF


class FusedCNN:
    def __init__(self, net, workgroups: int | None = None):
        C = _native.C()
        self.net = net
        self.params = list(net.parameters())
        n = sum(p.numel() for p in self.params)
        assert n == C.cnn_num_params(), f"not the reference Net ({n} params)"
        dev = self.params[0].device
        flat = torch.empty(n, dtype=torch.float32, device=dev)
        off = 0
        with torch.no_grad():
            for p in self.params:
                k = p.numel()
                flat[off:off + k].copy_(p.detach().reshape(-1))
                p.data = flat[off:off + k].view_as(p)
                off += k
        self.flat = flat
        OF.bump_weight_generation()  # parameter storage moved: drop cached compute copies
        self.own_grad = None
        self.workgroups = workgroups
        self.stamps = None  # diagnostic: int64 [nwg, 16] tensor of per-phase wall-clock stamps
        self.stop_after = -1  # diagnostic: end the training kernel after phase stamp k (counter attribution)
        self.frag = torch.empty(C.cnn_frag_bytes(), dtype=torch.uint8, device=dev)
        self._frag_gen = None  # weight generation at which the fragment image was last made current
        # an optimiser other than the fused SGD updates the weights every step (AdamW, hipGraph-replayed): the
        # kernel rebuilds its bf16 fragment image from the fp32 weights at every step (k_cnn_prep fused in)
        self.always_prep = False

    def invalidate(self):
        """The fp32 weights were written behind our back: rebuild the fragment image next step."""
        self._frag_gen = None

    def _bind_state(self, opt, mode: int):
        """The optimiser's per-parameter state -- ``momentum_buffer`` (SGD with momentum) or ``exp_avg`` /
        ``exp_avg_sq`` (Adam, AdamW) -- becomes views of two flat buffers indexed like ``self.flat`` (state_dict keeps
        working, and the multi-tensor ``opt.step()`` and the fused updates share one state); a state tensor replaced
        behind our back (``load_state_dict``, an elastic restore) is copied in and re-bound."""
        if mode == 0:
            return
        if getattr(self, "_opt_m", None) is None:
            self._opt_m = torch.zeros_like(self.flat)
            self._opt_v = torch.zeros_like(self.flat)
        if mode == 1:
            keys = (("momentum_buffer", self._opt_m),) if opt.param_groups[0]["momentum"] != 0.0 else ()
        else:
            keys = (("exp_avg", self._opt_m), ("exp_avg_sq", self._opt_v))
        off = 0
        for p in self.params:
            k = p.numel()
            st = opt.state[p]
            for key, flat in keys:
                view = flat[off:off + k].view_as(p)
                cur = st.get(key)
                if cur is None or cur.data_ptr() != view.data_ptr():
                    with torch.no_grad():
                        if cur is None:
                            view.zero_()
                        else:
                            view.copy_(cur.reshape(p.shape))
                    st[key] = view
            off += k

    def _update_args(self, opt):
        """``(mode, device state, params, m, v)`` of an optimiser the fused update can apply
        (:func:`fused_update_mode`): its state bound to the flat buffers BEFORE the optimiser builds its device table,
        so both see one state; ``m`` / ``v``: the flat state buffers the mode uses, else ``None``."""
        mode = fused_update_mode(opt)
        assert mode is not None, "fused update needs a one-group FusedSGD, FusedAdam or FusedAdamW"
        self._bind_state(opt, mode)
        group = opt.param_groups[0]
        params = [p for p in group["params"] if p.grad is not None]
        st = opt._group_dev(0, group, params)
        for p in params:  # the fused update writes the fp32 weights only (plus its own fragment image)
            OF.release_compute_copies(p)
        return mode, st, params, (self._opt_m if mode >= 1 else None), (self._opt_v if mode >= 2 else None)

    def _after_update(self, opt, params):
        # the step count lives in the optimizer's device counter (advanced by the fused kernels, so hipGraph
        # replays count too); the optimiser's state_dict() reads it back
        OF.bump_weight_generation()
        self._frag_gen = OF.weight_generation()

    @torch.no_grad()
    def opt_step(self, opt, grads: torch.Tensor):
        """``opt.step()`` for the flat parameters fused with the fragment-image refresh, ONE launch: plain SGD
        (``k_cnn_sgd``), SGD with momentum / weight decay, Adam or AdamW (``k_cnn_opt<MODE>``) -- the update after
        a gradient all-reduce that ran outside the reduction kernel.  The update math and the device step counter are
        the optimiser's own (optim_device.h)."""
        mode, st, params, m, v = self._update_args(opt)
        _native.C().cnn_opt(self.flat, grads, self.frag, st["hp"], st["step"], mode=mode, m=m, v=v)
        self._after_update(opt, params)

    @torch.no_grad()
    def adasum_step(self, opt, grads: torch.Tensor, xgmi):
        """``hvd.Adasum`` of the ranks' weight deltas (``hvd/optimizer.py`` ``_adasum_step``) behind
        ``forward_backward(x, y, grad_out=grads)``, TWO launches on the current stream: ``k_cnn_adasum_delta`` takes
        ``opt``'s LOCAL step on ``grads`` (its state and device step counter advance; the weights keep the shared
        starting values), exchanges the deltas over ``xgmi`` (a one-shot :class:`..parallel.xgmi_allreduce.
        XgmiAllreduce` over a power-of-two world) and writes every tensor's Gram; ``k_cnn_adasum_apply`` sets
        ``w = start + adasum_r(delta_r)``, one set of coefficients per parameter tensor, bit-identical on every rank,
        and refreshes the fragment image.  ``xgmi`` must be idle on every other stream (the hvd engine: graph mode)."""
        mode, st, params, m, v = self._update_args(opt)
        gram, rows = xgmi.gram_workspace()
        _native.C().cnn_adasum_step(self.flat, grads, self.frag, st["hp"], st["step"], mode, m, v,
                                    xgmi_view=xgmi.view(), gram=gram, gram_rows=rows)
        self._after_update(opt, params)

    def sgd_step(self, opt, grads: torch.Tensor):
        """:meth:`opt_step` of a one-group FusedSGD (any momentum / weight decay)."""
        from ..ops.optim import FusedSGD

        assert isinstance(opt, FusedSGD), "sgd_step needs a FusedSGD"
        self.opt_step(opt, grads)

    def adam_step(self, opt, grads: torch.Tensor):
        """:meth:`opt_step` of a one-group FusedAdam (L2 weight decay)."""
        from ..ops.optim import FusedAdam

        assert isinstance(opt, FusedAdam), "adam_step needs a FusedAdam"
        self.opt_step(opt, grads)

    def adamw_step(self, opt, grads: torch.Tensor):
        """:meth:`opt_step` of a one-group FusedAdamW: one launch instead of the multi-tensor update plus the next
        step's prep launch."""
        from ..ops.optim import FusedAdamW

        assert isinstance(opt, FusedAdamW), "adamw_step needs a FusedAdamW"
        self.opt_step(opt, grads)

    def _nwg(self, B: int) -> int:
        if self.workgroups:
            return self.workgroups
        # ~4 images per workgroup, one workgroup per CU (256 CUs); 2 fit per CU by LDS
        return max(1, min(512, (B + 3) // 4))

    def grad_buffer(self) -> torch.Tensor:
        """A flat gradient buffer whose views are installed as ``p.grad`` (when no DDP buffer is used)."""
        if self.own_grad is None:
            self.own_grad = torch.zeros_like(self.flat)
            off = 0
            for p in self.params:
                k = p.numel()
                p.grad = self.own_grad[off:off + k].view_as(p)
                off += k
        return self.own_grad

    def forward_backward(self, x: torch.Tensor, y: torch.Tensor, grad_out: torch.Tensor | None = None,
                         accumulate: bool = False, p_drop2: float = 0.5, p_drop1: float = 0.5,
                         sgd=None, xgmi=None, avg: bool = True, opt=None) -> torch.Tensor:
        """Loss (device scalar) of the local batch; gradients of the mean loss written to ``grad_out``.

        ``sgd`` / ``opt`` (synonyms; pass one): a one-group FusedSGD (any momentum / weight decay), FusedAdam or
        FusedAdamW over these parameters -- also take the optimiser step, inside the reduction kernel.
        ``xgmi``: an XgmiAllreduce over the data-parallel ranks -- ``grad_out`` receives the all-reduced
        gradients (``avg``: averaged), exchanged inside the reduction kernel."""
        C = _native.C()
        if sgd is not None and opt is not None:
            raise ValueError("forward_backward: pass the optimiser as sgd= or opt=, not both")
        opt = sgd if opt is None else opt
        if grad_out is None:
            grad_out = self.grad_buffer()
        x = x.float().contiguous()
        y = y.long().contiguous()
        training = self.net.training
        prep = self.always_prep or self._frag_gen is None or self._frag_gen != OF.weight_generation()
        update = {}
        if opt is not None:
            mode, st, params, m, v = self._update_args(opt)
            update = dict(hp=st["hp"], step=st["step"], mode=mode, m=m, v=v)
        view, xscale = None, 1.0
        if xgmi is not None and xgmi.size > 1:
            view, xscale = xgmi.view(), (1.0 / xgmi.size if avg else 1.0)
        loss = C.cnn_train(x, y, self.flat, OF._rng_counter(x.device), p_drop2, p_drop1, training, grad_out,
                           accumulate, stamps=self.stamps, frag=self.frag, prep=prep, stop_after=self.stop_after,
                           xgmi_view=view, xscale=xscale, **update)
        if opt is not None:
            self._after_update(opt, params)
        else:
            # the weights did not change: the image stays current until someone writes them
            self._frag_gen = OF.weight_generation()
        return loss

    # ---- forward-only evaluation (k_cnn_eval): eval mode whatever net.training says ---------------------------
    def _eval(self, x, y, stats, want_pred, want_logp):
        x = x.float().contiguous()
        if y is not None:
            y = y.long().contiguous()
        # the fragment-currency rule of forward_backward; the weights do not change, so the generation stays
        prep = self.always_prep or self._frag_gen is None or self._frag_gen != OF.weight_generation()
        pred, logp = _native.C().cnn_eval(x, y, self.flat, self.frag, prep, want_pred, want_logp,
                                          None if stats is None else stats.buf)
        self._frag_gen = OF.weight_generation()
        return pred, logp

    @torch.no_grad()
    def predict(self, x: torch.Tensor, logprobs: bool = False):
        """Predicted class of every image (int64 ``[B]``, lowest index on a tie) on the fused path; with
        ``logprobs`` also the fp32 ``[B, 10]`` log-probabilities: ``(pred, logp)``."""
        pred, logp = self._eval(x, None, None, True, logprobs)
        return (pred, logp) if logprobs else pred

    @torch.no_grad()
    def evaluate(self, x: torch.Tensor, y: torch.Tensor, stats: "CnnEvalStats | None" = None,
                 logprobs: bool = False):
        """Add the batch's summed NLL, correct predictions and image count to ``stats`` (a new
        :class:`CnnEvalStats` when ``None``) without any host synchronisation; returns ``stats``, or
        ``(stats, logp)`` with ``logprobs``.  Read the totals once per pass with ``stats.result()``."""
        if stats is None:
            stats = CnnEvalStats(self.flat.device)
        _, logp = self._eval(x, y, stats, False, logprobs)
        return (stats, logp) if logprobs else stats


def fused_update_mode(opt) -> int | None:
    """The update mode of the fused CNN kernels for ``opt``: 0 plain SGD, 1 SGD with momentum and / or L2 weight
    decay, 2 Adam (L2), 3 AdamW -- for a one-group FusedSGD / FusedAdam / FusedAdamW (a ``hvd.DistributedOptimizer``
    around one too); ``None`` for anything else, which keeps ``opt.step()``.  Pure: needs no native module."""
    from ..ops.optim import FusedAdam, FusedAdamW, FusedSGD

    if not isinstance(opt, (FusedSGD, FusedAdam, FusedAdamW)) or len(opt.param_groups) != 1:
        return None
    if isinstance(opt, FusedSGD):
        group = opt.param_groups[0]
        return 0 if group["momentum"] == 0.0 and group["weight_decay"] == 0.0 else 1
    return 2 if isinstance(opt, FusedAdam) else 3


def opt_in_reduce_enabled() -> bool:
    """Single process, FusedAdam / FusedAdamW: take the update inside the reduction kernel (two launches per step)
    instead of the one-launch update behind it (three); ``PDE_CNN_OPT_IN_REDUCE=0|1`` is the A/B switch."""
    return os.environ.get("PDE_CNN_OPT_IN_REDUCE", "1") != "0"


def fused_eval_enabled() -> bool:
    """The entry scripts' test passes run through :meth:`FusedCNN.evaluate`; ``PDE_CNN_EVAL=0`` keeps the
    layer-by-layer pass (A/B runs)."""
    return os.environ.get("PDE_CNN_EVAL", "1") != "0"


class CnnEvalStats:
    """Running totals of :meth:`FusedCNN.evaluate` on the device: summed NLL (float64), correct predictions and
    images.  The sum over a batch is combined in a fixed order, so equal calls give bitwise-equal totals.  Calls that
    share one buffer must be ordered on the device (one stream, or one captured graph): a launch owns the arrival
    ticket in the buffer until it ends."""

    def __init__(self, device):
        # {loss_sum as float64 bits, correct, count, the kernel's arrival ticket (0 between launches)}
        self.buf = torch.zeros(4, dtype=torch.int64, device=device)

    def zero_(self):
        self.buf.zero_()
        return self

    def result(self):
        """``(loss_sum, correct, count)`` -- one device-to-host copy."""
        host = self.buf.cpu()
        return float(host[:1].view(torch.float64).item()), int(host[1].item()), int(host[2].item())
