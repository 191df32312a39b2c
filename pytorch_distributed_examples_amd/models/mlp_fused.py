"""Fused training step for the elastic-DDP MLP (pytorch_elastic/mnist_ddp_elastic.py:133-173; the model of
:mod:`.mlp`), without autograd: one explicit launch sequence over preallocated activation buffers.

Per step, for L linear layers (7 for the reference 5x1024 model):

* 1 cast of the fp32 images into a bf16 activation buffer that carries a trailing ONES column;
* L forward GEMMs (bias + ReLU in the epilogue) writing straight into the next layer's padded buffer,
  whose ones column is set once at allocation;
* 1 fused cross-entropy launch: mean loss + d logits (bf16);
* L weight-gradient GEMMs that also produce the bias gradient: the GEMM runs over the input's ones
  column, and that output column (= the batch sum of dY) is routed to the bias gradient in the epilogue
  (``linear_wgrad_bias``) -- no column-sum kernel; weight and bias gradients land directly in the
  parameters' ``.grad`` (the DDP flat buffer), no zeroing, no accumulation copies;
* L-1 data-gradient GEMMs with the producer's ReLU mask applied in the epilogue (threshold_backward
  fused); the first layer's input gradient is never computed.  Each layer's dgrad and weight-gradient
  GEMMs go out as ONE paired launch (``OF.gemm_pair``), so the two small grids fill the chip together.

The layer-by-layer autograd path (``MLP.forward`` + ``backward()``) runs the same GEMMs plus autograd's
grad-zeroing, copies, casts and one bias column-sum per layer (≈60 launches per step vs ≈30 here).

    fmlp = FusedMLP(model)                       # model: MLP on the GPU
    ddp = DistributedDataParallel(model, overlap=False)
    loss = fmlp.forward_backward(x, y)           # grads written into p.grad (the DDP flat buffer)
    ddp.sync_gradients(); opt.step()
"""
from __future__ import annotations

import torch

from .. import _native
from ..ops import functional as OF
from ..ops import streams


def _pad8(n: int) -> int:
    return (n + 7) // 8 * 8


class FusedMLP:
    """``precision="fp8"`` (opt-in, GPU only): the same step on the FP8 GEMM of ``csrc/kernels/gemm_fp8.hip`` --
    e4m3 weights and activations, e5m2 gradients, per-tensor power-of-two scales from the previous step's maxima
    (:mod:`..ops.fp8`), fp32 accumulation, fp32 master weights and fp32 gradients in ``p.grad``.  Per step: one
    weight-quantise launch, one input-quantise launch, L forward GEMMs (bias + ReLU + quantise + transpose in the
    epilogue), ``ce_fused``, one d-logits quantise launch, L weight-gradient GEMMs (bias gradient inside) and L-1
    data-gradient GEMMs (ReLU mask + quantise + transpose in the epilogue), one scale-update launch."""

    def __init__(self, net, precision: str = "bf16"):
        if precision not in ("bf16", "fp8"):
            raise ValueError(f"precision must be 'bf16' or 'fp8', not {precision!r}")
        self.net = net
        self.precision = precision
        self.layers = [net.input_layer, *net.hidden_layers, net.final_layer]
        for i, L in enumerate(self.layers):
            assert L.bias is not None, "the fused step routes every bias gradient through the ones column"
            assert L.relu == (i < len(self.layers) - 1), "ReLU after every layer but the last"
        self._bufs: dict = {}
        self._fp8: dict = {}

    # ---- FP8 path ------------------------------------------------------------------------------------------
    def _fp8_state(self, B: int, dev: torch.device):
        """Records (shared by every batch size), weight buffers and table, and the per-batch-size buffers.  Nothing
        here depends on the input tensor: the input and d logits are quantised by table-free launches."""
        from ..ops import fp8

        n = len(self.layers)
        st = self._fp8
        if "rec" not in st:
            # record i: input of layer i; n + i: weight i; 2n + i: gradient of layer i's output
            st["rec"] = fp8.ScaleRecords([fp8.E4M3] * (2 * n) + [fp8.E5M2] * n, dev)
            st["wq"] = [fp8.buffer(L.out_features, L.in_features, dev) for L in self.layers]
            st["wqt"] = [fp8.buffer(L.in_features, L.out_features, dev) for L in self.layers]
        wkey = tuple(L.weight.data_ptr() for L in self.layers)
        if st.get("wkey") != wkey:  # first use, or the parameters moved: the weight quantiser's table is rebuilt
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FusedMLP(precision='fp8'): the weights moved since the last eager step; run one "
                                   "step (or calibrate) before graph capture")
            st["wkey"] = wkey
            st["wplan"] = fp8.QuantPlan(st["rec"], fp8.E4M3, [L.weight.detach() for L in self.layers], st["wq"],
                                        st["wqt"], [n + i for i in range(n)])
        if B not in st:
            feats = [self.layers[0].in_features] + [L.out_features for L in self.layers]
            st[B] = dict(
                aq=[fp8.buffer(B, f, dev) for f in feats[:-1]], aqt=[fp8.buffer(f, B, dev) for f in feats[:-1]],
                dq=[fp8.buffer(B, f, dev) for f in feats[1:]], dqt=[fp8.buffer(f, B, dev) for f in feats[1:]],
                logits=torch.empty(B, feats[-1], dtype=torch.float32, device=dev),
                dlog=torch.zeros(B, _pad8(feats[-1]), dtype=torch.bfloat16, device=dev))
        return st, st[B]

    def _forward_backward_fp8(self, x, y, accumulate):
        from ..ops import fp8

        if not x.is_cuda:
            raise ValueError("precision='fp8' runs on the GPU only (the FP8 GEMM is a gfx950 kernel)")
        C = _native.C()
        B, n = x.shape[0], len(self.layers)
        xs = x.reshape(B, -1)  # the quantiser reads fp32 or bf16 rows of any pitch, wherever they are
        if xs.dtype not in (torch.float32, torch.bfloat16):
            xs = xs.float()
        if xs.stride(1) != 1:
            xs = xs.contiguous()
        st, b = self._fp8_state(B, x.device)
        rec, last = st["rec"].t, n - 1
        st["wplan"].run()
        fp8.quantise(st["rec"], fp8.E4M3, xs, b["aq"][0], b["aqt"][0], 0)
        for i, L in enumerate(self.layers):
            if i < last:
                C.fp8_gemm("fwd", b["aq"][i], st["wq"][i], B, L.out_features, rec, i, n + i, bias=L.bias.detach(),
                           q=b["aq"][i + 1], qt=b["aqt"][i + 1], rec_out=i + 1)
            else:
                C.fp8_gemm("fwd", b["aq"][i], st["wq"][i], B, L.out_features, rec, i, n + i, bias=L.bias.detach(),
                           out=b["logits"])
        loss, _ = C.ce_fused(b["logits"], y.long().contiguous(), b["dlog"])
        fp8.quantise(st["rec"], fp8.E5M2, b["dlog"][:, :self.layers[-1].out_features], b["dq"][-1], b["dqt"][-1],
                     3 * n - 1)
        for i in range(last, -1, -1):
            L = self.layers[i]
            gw, gb = self._grads(L)
            C.fp8_gemm("wgrad", b["dqt"][i], b["aqt"][i], L.out_features, L.in_features, rec, 2 * n + i, i,
                       out=gw, gbias=gb, accumulate=accumulate)
            if i > 0:
                C.fp8_gemm("dgrad", b["dq"][i], st["wqt"][i], B, L.in_features, rec, 2 * n + i, n + i,
                           q=b["dq"][i - 1], qt=b["dqt"][i - 1], rec_out=2 * n + i - 1, mask=b["aq"][i])
        st["rec"].update()
        return loss

    @torch.no_grad()
    def calibrate(self, x: torch.Tensor, y: torch.Tensor) -> None:
        """One FP8 pass that only sets the scales (the first real step then does not run on the initial scales
        of 1); the gradients it leaves are overwritten by the next step."""
        if self.precision != "fp8":
            raise ValueError("calibrate() belongs to precision='fp8'")
        self._forward_backward_fp8(x, y, False)

    def fp8_scales(self) -> dict:
        """The current scales: {'act': [...], 'weight': [...], 'grad': [...]}, one per layer (after a step)."""
        s, n = self._fp8["rec"].scales(), len(self.layers)
        return {"act": s[:n], "weight": s[n:2 * n], "grad": s[2 * n:]}

    def _buffers(self, B: int, dev: torch.device):
        key = (B, str(dev))
        if key not in self._bufs:
            bf = dict(dtype=torch.bfloat16, device=dev)
            acts = [torch.zeros(B, _pad8(self.layers[0].in_features + 1), **bf)]  # ones column: per-step cast
            for L in self.layers[:-1]:
                h = torch.zeros(B, _pad8(L.out_features + 1), **bf)
                h[:, L.out_features] = 1.0  # the GEMMs write [:, :out_features] only
                acts.append(h)
            logits = torch.empty(B, self.layers[-1].out_features, dtype=torch.float32, device=dev)
            dys = [torch.empty(B, L.out_features, **bf) for L in self.layers[:-1]]
            # d logits with its row padded to a multiple of 8 (zero columns, never written): the last layer's
            # dgrad then has K = 16 instead of 10 and runs on the FAST GEMM path with the zero-padded weight copy
            dlog = torch.zeros(B, _pad8(self.layers[-1].out_features), **bf)
            self._bufs[key] = (acts, logits, dys, dlog)
        return self._bufs[key]

    def _grads(self, L):
        for p in (L.weight, L.bias):
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        return L.weight.grad, L.bias.grad

    @torch.no_grad()
    def forward_backward(self, x: torch.Tensor, y: torch.Tensor, accumulate: bool = False, opt=None) -> torch.Tensor:
        """Mean cross-entropy of the batch (device scalar); parameter gradients written (``accumulate``:
        added) into each parameter's ``.grad``.

        ``opt`` (a fused optimiser, single process -- no gradient all-reduce between backward and update):
        the optimiser step is folded into the backward: layer i+1's update runs as extra blocks of layer i's
        paired dgrad + wgrad launch (its gradients are final by then, and no GEMM of that launch touches its
        weights), layers 1 and 0 in one closing launch.  Replaces ``opt.step()``; same update math, same
        kernels' device code.  Not available with ``precision="fp8"`` (ValueError)."""
        if self.precision == "fp8":
            if opt is not None:
                raise ValueError("precision='fp8' does not fold the optimiser into the backward: call opt.step()")
            return self._forward_backward_fp8(x, y, accumulate)
        C = _native.C()
        params_of = [[L.weight, L.bias] for L in self.layers]
        fuse_opt = (opt is not None and not streams.active_for(x) and
                    opt.supports_segments([p for ps in params_of for p in ps]))
        if fuse_opt:
            for L in self.layers:  # every gradient exists up front: ONE optimiser table for the whole step
                self._grads(L)
        B = x.shape[0]
        acts, logits, dys, dlog = self._buffers(B, x.device)
        C.cast_rows_ones(x.reshape(B, -1).float().contiguous(), acts[0])
        last = len(self.layers) - 1
        for i, L in enumerate(self.layers):
            w = OF._bf16_weight(L.weight)
            out = acts[i + 1][:, :L.out_features] if i < last else logits
            C.linear_fwd_out(acts[i][:, :L.in_features], w, L.bias.detach(), i < last, out)
        nout = self.layers[-1].out_features
        loss, dy = C.ce_fused(logits, y.long().contiguous(), dlog)
        dy = dlog[:, :nout]
        side = streams.active_for(x)
        for i in range(last, -1, -1):
            L = self.layers[i]
            gw, gb = self._grads(L)
            if side:
                # (opt-in, ops/streams.py) weight + bias gradient on the side stream, concurrent with the dgrad
                # chain (forked before the dgrad is enqueued so the fork point does not wait for it)
                with streams.fork(dy, join_at_backward_end=False):
                    C.linear_wgrad_bias(dy, acts[i][:, :L.in_features + 1], gw, gb, accumulate)
            elif i > 0:
                # dgrad + weight/bias gradient as ONE paired GEMM launch (dgrad tiles first), carrying the update
                # of layer i + 1 when the optimiser is folded in
                wpad = OF._maintained(L.weight, "bf16_pad") if i == last else None
                if fuse_opt and i < last:
                    opt.attach_update(params_of[i + 1])
                with OF.gemm_pair(defer_second=True, flush_by_caller=True):
                    if wpad is not None:  # K padded to 16: zero columns of d logits x zero rows of the weight
                        C.linear_dgrad_out(dlog, wpad, acts[i][:, :L.in_features], dys[i - 1])
                    else:
                        C.linear_dgrad_out(dy, OF._bf16_weight(L.weight), acts[i][:, :L.in_features], dys[i - 1])
                    C.linear_wgrad_bias(dy, acts[i][:, :L.in_features + 1], gw, gb, accumulate)
                dy = dys[i - 1]
                continue
            else:
                C.linear_wgrad_bias(dy, acts[i][:, :L.in_features + 1], gw, gb, accumulate)
            if i > 0:
                C.linear_dgrad_out(dy, OF._bf16_weight(L.weight), acts[i][:, :L.in_features], dys[i - 1])
                dy = dys[i - 1]
        # the deferred weight-gradient reductions: one batched launch (and the side stream, if used)
        streams.join(x.device)
        if fuse_opt:  # the updates no backward launch could carry: layers 0 and 1 (1 only if it exists)
            opt.step_range([p for ps in params_of[:min(2, last + 1)] for p in ps], last=True)
        return loss

    def launches_per_step(self) -> int:
        """Kernel launches of one forward_backward (split-K GEMMs add their reduce launch on top)."""
        n = len(self.layers)
        if self.precision == "fp8":  # + weight quantise, d-logits quantise and the scale update
            return 2 + n + 2 + n + (n - 1) + 1
        return 1 + n + 1 + n + (n - 1)
