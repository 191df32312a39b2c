"""Fused multi-tensor optimisers: SGD, Adam, AdamW, and the trust-ratio pair LAMB and LARS.

GPU parameters are updated by ONE ``multi_tensor_optim`` launch per param group (csrc/kernels/optim.hip)
whose hyper-parameters and step counter live in device memory, so the update is hipGraph-capturable
and an LR change between replays (Horovod-elastic ``on_state_reset``, horovod_mnist_elastic.py:80-82)
is honoured.  The same launch refreshes the bf16 compute copies of the weights it updates (linear and
1x1-conv weights, whose compute layout is a plain cast), so those layers never re-derive them per step
(:func:`.functional.maintain_compute_copies`).  CPU parameters use the same math in plain torch (the
reference's CPU configuration).

:class:`FusedLAMB` and :class:`FusedLARS` scale every tensor's update by a ratio of two L2 norms over the whole
tensor, so their step is TWO launches (csrc/kernels/optim_trust.hip): the chunks' squared norms, then the update.
Same device-resident hyper-parameters and step counter, same bf16 copy refresh, no host read and no allocation
in ``step()``: capturable like the others.

The per-parameter state uses torch's key names (``step``, ``exp_avg``, ``exp_avg_sq``,
``momentum_buffer``) so ``state_dict()`` round-trips with ``torch.optim`` and with the elastic
``TorchState`` commit/restore.

``max_grad_norm=X`` on any of the five classes clips the gradient to a global L2 norm first, with
``torch.nn.utils.clip_grad_norm_``'s semantics and ``grad_scale`` folded in: ``g' = grad_scale g``, ``total =
sqrt(sum g'^2)`` over every parameter of every group that has a gradient, ``coef = min(1, X / (total + 1e-6))``, and
the update runs on ``coef g'``.  On the GPU that is ONE more launch per step (csrc/kernels/optim_clip.hip): it
reduces the norm and writes, per group, a second hyper-parameter table whose ``grad_scale`` carries ``coef``; the
unchanged update kernels then run on that table.  ``last_grad_norm`` is the device tensor ``{total, coef}``; no host
read, so the step stays capturable, and ``max_grad_norm`` lives in device memory like the other hyper-parameters.
"""
from __future__ import annotations

import torch

from .. import _native
from . import functional as OF
from . import streams

_MODES = {"sgd": 0, "adam": 1, "adamw": 2}
_TRUST = {"lamb": 0, "lars": 1}  # kinds of the two-launch trust-ratio step (multi_tensor_trust)
_ADAM_STATE = ("adam", "adamw", "lamb")  # exp_avg + exp_avg_sq; the others: momentum_buffer with momentum != 0


class _FusedBase(torch.optim.Optimizer):
    KIND = "adam"

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, momentum=0.0,
                 grad_scale=1.0, max_grad_norm=None, **extra):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, momentum=momentum,
                        grad_scale=grad_scale, max_grad_norm=max_grad_norm, **extra)
        super().__init__(params, defaults)
        self._dev = {}  # id(group) -> dict(table, sig, hp, hp_key, step)
        self._clip = None  # dict(ws, key, nchunks): the clip workspace (pde_kernels.h ClipWs), made on first use

    # -- global-norm clipping --------------------------------------------------------------------
    def clip_max_norm(self):
        """The optimiser's ``max_grad_norm``, or ``None`` when it does not clip.  One norm spans all groups, so the
        groups must agree (``.get``: a param group saved before the option existed has no such key)."""
        vals = {g.get("max_grad_norm") for g in self.param_groups}
        if len(vals) > 1:
            raise ValueError(f"max_grad_norm must be the same in every param group (one global norm), not {vals}")
        return next(iter(vals)) if vals else None

    def _clip_dev(self, device, nchunks: int):
        """The clip workspace, sized for ``nchunks`` chunks, with ``max_grad_norm`` uploaded when it changed."""
        C = _native.C()
        cl = self._clip
        if cl is None or "ws" not in cl or cl["nchunks"] < nchunks or cl["ws"].device != device:
            ws = torch.zeros(C.optim_clip_ws_floats(nchunks), dtype=torch.float32, device=device)
            cl = self._clip = {"ws": ws, "nchunks": nchunks, "key": None, "layout": C.optim_clip_layout()}
        self._upload_clip(cl)
        return cl

    def _upload_clip(self, cl):
        key = float(self.clip_max_norm())
        if cl["key"] != key:
            o = cl["layout"][0]
            cl["ws"][o:o + 1].copy_(torch.tensor([key], dtype=torch.float32), non_blocking=False)
            cl["key"] = key

    def _hp_eff(self, cl, slot: int):
        _, _, o, n = cl["layout"]
        return cl["ws"][o + slot * n:o + (slot + 1) * n]

    @property
    def last_grad_norm(self):
        """Device tensor ``{total, coef}`` of the last clipped GPU step -- the norm before clipping, as
        ``clip_grad_norm_`` returns it, and the coefficient applied -- without a synchronisation; ``None`` before
        the first one.  (CPU parameters: a host tensor of the same two numbers.)"""
        if self._clip is None:
            return None
        if "host" in self._clip:
            return self._clip["host"]
        o = self._clip["layout"][1]
        return self._clip["ws"][o:o + 2]

    # -- GPU -----------------------------------------------------------------------------------
    def _group_dev(self, gi, group, params):
        C = _native.C()
        st = self._dev.get(gi)
        dev = params[0].device
        if st is None:
            st = {"sig": None, "hp_key": None,
                  "hp": torch.zeros(9, dtype=torch.float32, device=dev),  # float[HP_COUNT], pde_kernels.h
                  # {steps taken, arrival counter of the update kernel}
                  "step": torch.zeros(2, dtype=torch.int32, device=dev)}
            # a new group state (new optimizer, or after load_state_dict): the host step is authoritative once
            s0 = self.state[params[0]].get("step") if params else None
            st["step"][0].fill_(int(s0) if s0 is not None else 0)
            self._dev[gi] = st
        need_avg = self.KIND in _ADAM_STATE or group["momentum"] != 0.0
        for p in params:
            state = self.state[p]
            if self.KIND in _ADAM_STATE:
                if "exp_avg" not in state:
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            elif need_avg and "momentum_buffer" not in state:
                state["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        grads = [p.grad for p in params]
        if self.KIND in _ADAM_STATE:
            m = [self.state[p]["exp_avg"] for p in params]
            v = [self.state[p]["exp_avg_sq"] for p in params]
        else:
            m = [self.state[p]["momentum_buffer"] for p in params] if need_avg else []
            v = []
        sig = tuple((p.data_ptr(), g.data_ptr(), g.is_contiguous()) for p, g in zip(params, grads)) + \
            tuple(t.data_ptr() for t in m) + tuple(t.data_ptr() for t in v)
        if st["sig"] != sig:
            # (re)build the tables; the device step counter carries on
            grads_c = [g if g.is_contiguous() else g.contiguous() for g in grads]
            copies = [OF.maintain_compute_copies(p) or {} for p in params]
            none = torch.empty(0, device=params[0].device)
            bf = [c.get("bf16", none) for c in copies]
            table, chunks, nchunks = C.optim_table([p.data for p in params], grads_c, m, v, bf)
            st.update(sig=sig, table=table, chunks=chunks, nchunks=nchunks, grads_keep=grads_c)
            if self.KIND in _TRUST:  # per-tensor chunk spans + the float2[nchunks] norm workspace, made once
                st["spans"], st["norms"], n = C.optim_trust_table([p.data for p in params])
                assert n == nchunks
            # KxK conv weights: both bf16 GEMM layouts refreshed by one launch after the update
            kxk = [(p, c) for p, c in zip(params, copies) if "kxk" in c]
            st["conv_table"], st["nconv"], st["conv_blocks"] = None, 0, 0
            if kxk:
                st["conv_table"] = C.conv_layout_table([p.data for p, _ in kxk], [c["conv_fwd"] for _, c in kxk],
                                                       [c["conv_dgrad"] for _, c in kxk],
                                                       [c["kxk"][0] for _, c in kxk], [c["kxk"][1] for _, c in kxk])
                st["nconv"] = len(kxk)
                # x blocks per entry: the largest weight's 32x32 (co, ci) tiles (3x3 path) / 256-pair chunks
                tiles = max(-(-c["kxk"][0] // 32) * -(-c["kxk"][1] // 32) for _, c in kxk)
                st["conv_blocks"] = max(1, min(1024, tiles))
        self._upload_hyper(st, group)
        return st

    def _upload_hyper(self, st, group):
        b1, b2 = group["betas"]
        if self.KIND == "lars":
            b1 = group["trust_coefficient"]  # HP_TRUST: the slot of beta1, which LARS has no use for
        hp_key = (group["lr"], b1, b2, group["eps"], group["weight_decay"], group["momentum"], group["grad_scale"])
        if st["hp_key"] != hp_key:
            # + HP_OMB1 / HP_OMB2: 1 - beta in double, then rounded (the kernel's 1.f - 0.999f is 1.3e-5 off)
            st["hp"].copy_(torch.tensor(list(hp_key) + [1.0 - b1, 1.0 - b2], dtype=torch.float32), non_blocking=False)
            st["hp_key"] = hp_key

    def sync_hyper_to_device(self):
        """Upload hyper-parameters changed through ``param_groups`` to the device tables the update kernels read:
        what a captured ``step()`` needs between hipGraph replays (an eager ``step()`` does it itself)."""
        for gi, group in enumerate(self.param_groups):
            if gi in self._dev:
                self._upload_hyper(self._dev[gi], group)
        if self._clip is not None and "ws" in self._clip and self.clip_max_norm() is not None:
            self._upload_clip(self._clip)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        C = None
        live = [(gi, group, [p for p in group["params"] if p.grad is not None])
                for gi, group in enumerate(self.param_groups)]
        live = [t for t in live if t[2]]
        hp_eff, cpu_coef = self._clip_step(live) if live and self.clip_max_norm() is not None else ({}, None)
        for gi, group, params in live:
            if params[0].is_cuda:
                C = C or _native.C()
                streams.join(params[0].device)  # gradients written on the wgrad side stream
                st = self._group_dev(gi, group, params)
                hp = hp_eff.get(gi, st["hp"])  # clipping: the group's table with coef in its grad scale
                if self.KIND in _TRUST:
                    C.optim_trust_step(st["table"], st["chunks"], st["nchunks"], st["spans"], st["norms"],
                                       _TRUST[self.KIND], hp, st["step"])
                else:
                    C.optim_step(st["table"], st["chunks"], st["nchunks"], _MODES[self.KIND], hp, st["step"])
                if st["nconv"]:
                    C.conv_layouts_step(st["conv_table"], st["nconv"], st["conv_blocks"])
                # host ``step`` is synchronised from the device counter by state_dict() (graph replays)
            else:
                self._cpu_step(group, params, cpu_coef)
        OF.bump_weight_generation()
        return loss

    def _clip_step(self, live):
        """The clipping half of ``step()`` over ``live`` = [(group index, group, params with a gradient)].  GPU: ONE
        ``optim_clip`` launch over all groups' tables; returns ({group index: hp_eff}, None).  CPU: the coefficient
        in torch, ``clip_grad_norm_``'s own operations; returns ({}, coef)."""
        max_norm = self.clip_max_norm()
        if not live[0][2][0].is_cuda:
            norms = []
            for _, group, params in live:
                gs = group["grad_scale"]
                norms += [torch.linalg.vector_norm(p.grad if gs == 1.0 else p.grad * gs) for p in params]
            total = torch.linalg.vector_norm(torch.stack(norms))
            coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
            self._clip = {"host": torch.stack([total, coef])}
            return {}, coef
        C = _native.C()
        if len(live) > 8:
            raise ValueError(f"max_grad_norm: at most 8 param groups with a gradient, not {len(live)}")
        dev = live[0][2][0].device
        if any(not p.is_cuda or p.device != dev for _, _, ps in live for p in ps):
            raise ValueError("max_grad_norm: one norm spans all parameters, which must be on one device")
        streams.join(dev)
        sts = [self._group_dev(gi, group, params) for gi, group, params in live]
        cl = self._clip_dev(dev, sum(st["nchunks"] for st in sts))
        C.optim_clip([st["table"] for st in sts], [st["chunks"] for st in sts], [st["nchunks"] for st in sts],
                     [st["hp"] for st in sts], cl["ws"])
        return {gi: self._hp_eff(cl, slot) for slot, (gi, _, _) in enumerate(live)}, None

    # -- update segments: one layer's update appended to a later backward GEMM launch ------------
    def _segment(self, subset):
        """(table, chunks, c0, c1, mode, hp, step) of ``subset`` -- parameters contiguous in the (single, GPU)
        param group's order -- for ``optim_attach`` / ``optim_step_range``."""
        assert len(self.param_groups) == 1, "update segments: one parameter group"
        if self.clip_max_norm() is not None:
            raise ValueError("update segments run before the global gradient norm exists: not with max_grad_norm")
        group = self.param_groups[0]
        params = [p for p in group["params"] if p.grad is not None]
        st = self._group_dev(0, group, params)
        chunk = _native.C().optim_chunk_elems()
        starts, c = {}, 0
        for p in params:
            starts[id(p)] = c
            c += -(-p.numel() // chunk)
        ids = [id(p) for p in subset]
        c0 = min(starts[i] for i in ids)
        c1 = max(starts[id(p)] + -(-p.numel() // chunk) for p in subset)
        assert c1 - c0 == sum(-(-p.numel() // chunk) for p in subset), "segment parameters must be contiguous"
        return st["table"], st["chunks"], c0, c1, _MODES[self.KIND], st["hp"], st["step"]

    def supports_segments(self, params) -> bool:
        """True when :meth:`attach_update` / :meth:`step_range` can run this optimiser's update piecewise:
        one GPU parameter group, no KxK conv layout copies to refresh, not a trust-ratio kind (its update
        needs the whole tensor's norms first) and no ``max_grad_norm`` (a segment would run before the global norm
        exists)."""
        # (inspects the maintained copies without re-allocating them: maintain_compute_copies would replace the
        # copies the optimiser table writes)
        return (self.KIND in _MODES and len(self.param_groups) == 1 and self.clip_max_norm() is None and
                all(p.is_cuda for p in params) and
                not any(getattr(p, "_pde_conv", False) and p.dim() == 4 and p.shape[2] * p.shape[3] > 1
                        for p in params) and
                not any("kxk" in p.__dict__.get("_pde_maint", {}) for p in params))

    @torch.no_grad()
    def attach_update(self, subset):
        """Append the update of ``subset`` (whose gradients are final) to the NEXT paired backward GEMM launch
        as extra blocks (``OF.gemm_pair``): the HBM-bound update overlaps the latency-bound GEMMs."""
        t, ch, c0, c1, mode, hp, step = self._segment(subset)
        _native.C().optim_attach(t, ch, c0, c1, mode, hp, step, False)

    @torch.no_grad()
    def step_range(self, subset, last: bool = True):
        """The update of ``subset`` as its own launch; ``last``: the step's final segment (advances the device
        step counter -- every parameter must have been updated by a segment of this step)."""
        t, ch, c0, c1, mode, hp, step = self._segment(subset)
        _native.C().optim_step_range(t, ch, c0, c1, mode, hp, step, last)
        if last:
            OF.bump_weight_generation()

    # -- CPU reference math (torch.optim semantics) ---------------------------------------------
    def _cpu_step(self, group, params, coef=None):
        lr, (b1, b2), eps = group["lr"], group["betas"], group["eps"]
        wd, mom, gs = group["weight_decay"], group["momentum"], group["grad_scale"]
        for p in params:
            g = p.grad if gs == 1.0 else p.grad * gs
            if coef is not None:  # max_grad_norm: the clip coefficient of _clip_step (a 0-dim tensor)
                g = g * coef
            state = self.state[p]
            state["step"] = state.get("step", 0) + 1
            t = state["step"]
            if self.KIND in _TRUST:
                self._cpu_trust(group, p, g, state, t)
                continue
            if self.KIND == "sgd":
                if wd != 0:
                    g = g.add(p, alpha=wd)
                if mom != 0:
                    buf = state.get("momentum_buffer")
                    if buf is None or t == 1:
                        buf = g.clone()
                    else:
                        buf.mul_(mom).add_(g)
                    state["momentum_buffer"] = buf
                    g = buf
                p.add_(g, alpha=-lr)
                continue
            if self.KIND == "adamw":
                p.mul_(1 - lr * wd)
            elif wd != 0:
                g = g.add(p, alpha=wd)
            if "exp_avg" not in state:
                state["exp_avg"] = torch.zeros_like(p)
                state["exp_avg_sq"] = torch.zeros_like(p)
            m, v = state["exp_avg"], state["exp_avg_sq"]
            m.lerp_(g, 1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            bc1 = 1 - b1 ** t
            bc2 = 1 - b2 ** t
            denom = (v.sqrt() / (bc2 ** 0.5)).add_(eps)
            p.addcdiv_(m, denom, value=-lr / bc1)

    def _cpu_trust(self, group, p, g, state, t):
        """LAMB / LARS on one CPU tensor (``g`` already scaled by ``grad_scale``)."""
        lr, (b1, b2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
        pn = p.norm()
        if self.KIND == "lamb":
            if "exp_avg" not in state:
                state["exp_avg"] = torch.zeros_like(p)
                state["exp_avg_sq"] = torch.zeros_like(p)
            m, v = state["exp_avg"], state["exp_avg_sq"]
            m.lerp_(g, 1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            u = (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt_().add_(eps))
            if wd != 0:
                u.add_(p, alpha=wd)
            un = u.norm()
            r = float(pn / un) if pn > 0 and un > 0 else 1.0
            p.add_(u, alpha=-lr * r)
            return
        mom, gn = group["momentum"], g.norm()
        r = float(group["trust_coefficient"] * pn / (gn + wd * pn + eps)) if pn > 0 and gn > 0 else 1.0
        d = (g.add(p, alpha=wd) if wd != 0 else g) * r
        if mom != 0:
            buf = state.get("momentum_buffer")
            if buf is None or t == 1:
                buf = d.clone()
            else:
                buf.mul_(mom).add_(d)
            state["momentum_buffer"] = buf
            d = buf
        p.add_(d, alpha=-lr)

    def sync_step_from_device(self):
        """Copy each GPU group's device step counter into the per-parameter host ``step``.  The device counter
        is authoritative: hipGraph replays of a captured training step (and the fused CNN update kernels)
        advance it without running this Python code."""
        for gi, group in enumerate(self.param_groups):
            st = self._dev.get(gi)
            if st is None:
                continue
            steps = int(st["step"][0].item())
            for p in group["params"]:
                if p in self.state:
                    self.state[p]["step"] = steps

    def state_dict(self):
        self.sync_step_from_device()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._dev = {}
        self._clip = None


class FusedSGD(_FusedBase):
    KIND = "sgd"

    def __init__(self, params, lr, momentum=0.0, weight_decay=0.0, grad_scale=1.0, max_grad_norm=None):
        super().__init__(params, lr=lr, momentum=momentum, weight_decay=weight_decay, grad_scale=grad_scale,
                         max_grad_norm=max_grad_norm)


class FusedAdam(_FusedBase):
    KIND = "adam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0,
                 max_grad_norm=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, grad_scale=grad_scale,
                         max_grad_norm=max_grad_norm)


class FusedAdamW(_FusedBase):
    KIND = "adamw"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0,
                 max_grad_norm=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, grad_scale=grad_scale,
                         max_grad_norm=max_grad_norm)


class FusedLAMB(_FusedBase):
    """LAMB (You et al. 2020): Adam's direction with a per-tensor trust ratio, two launches per step.

        m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;  u = (m / bc1) / (sqrt(v / bc2) + eps) + wd p
        r = |p| / |u| if both norms are positive, else 1;  p -= lr r u          (g' = grad_scale g)

    Norms are L2 norms over each parameter tensor as handed over.  ``max_grad_norm`` clips the gradient to a
    global norm before everything else (apex ``FusedLAMB(max_grad_norm=...)``), one more launch.  Not done here:
    excluding 1-D tensors (biases, norm scales) from the adaptation, update segments attached to GEMM launches
    (``supports_segments`` is False), and the in-kernel update of ``FusedCNN`` / ``MegaMLP``."""
    KIND = "lamb"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, grad_scale=1.0,
                 max_grad_norm=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, grad_scale=grad_scale,
                         max_grad_norm=max_grad_norm)


class FusedLARS(_FusedBase):
    """LARS (You et al. 2017): momentum SGD with a per-tensor trust ratio, two launches per step.

        r = trust_coefficient |p| / (|g'| + wd |p| + eps) if |p| and |g'| are positive, else 1
        d = r (g' + wd p);  m = d at step 1 or with momentum 0, else momentum m + d;  p -= lr m

    ``momentum_buffer`` exists only with momentum != 0.  ``max_grad_norm``: global-norm gradient clipping first,
    one more launch.  Not done here: excluding 1-D tensors from the adaptation, Nesterov momentum, update segments
    attached to GEMM launches (``supports_segments`` is False), and the in-kernel update of ``FusedCNN`` /
    ``MegaMLP``."""
    KIND = "lars"

    def __init__(self, params, lr, momentum=0.9, weight_decay=0.0, trust_coefficient=1e-3, eps=1e-8,
                 grad_scale=1.0, max_grad_norm=None):
        super().__init__(params, lr=lr, momentum=momentum, weight_decay=weight_decay, eps=eps,
                         grad_scale=grad_scale, max_grad_norm=max_grad_norm, trust_coefficient=trust_coefficient)
