"""Phase replay of the one-launch MLP training step (test_mlp_mega_exact_cpu.py, test_mlp_mega_exact_gpu.py):
``k_mlp_train`` (csrc/kernels/mlp_fused.hip, models/mlp_mega.py) against float64, phase by phase and element by
element.  Every phase is recomputed from the kernel's OWN inputs to that phase -- the buffers it left in memory --
so an error never compounds and a failure names the phase that made it.  u = 2^-24 throughout.

Before a step: copies of the fp32 weights and biases, both bf16 weight copies (``wbf`` [out][in], ``wtbf`` [in][ld],
ld = out, 32 for the last layer), the optimiser state, the step count, x and y; every ``p.grad`` is filled with NaN
and ``act[1:]``, ``actT``, ``d[1:]``, ``dT[1:]`` with the bf16 NaN pattern: none may remain (every element written).

  phase     inputs (as left in memory)                         output checked
  F_l       act[l] (l = 0: bf16(x)), pre-step wbf[l], bias     act[l+1] = bf16(relu(.))
  CE        act[nl-1], wbf[nl-1], bias, y                      dlog[:, :out] = bf16((softmax - onehot) / B), the loss
  dgrad_j   dlog or d[j+1], pre-step wtbf[j], act[j]           d[j] = bf16((G . W^T) [act_j > 0])          (j >= 1)
  wgrad_j   dlogT[:out] / dT[j+1], actT[j]                     p.grad: weight (fp32), bias = row sums of G^T
  update_l  pre-step p and state, the kernel's own p.grad,     p, exp_avg / exp_avg_sq / momentum_buffer
            the hyper-parameters, the step count

Bounds -- each from the operands of the float64 replay, none from the kernel's output.
  GEMM phases.  bf16 x bf16 products are exact in fp32, so only the accumulation rounds: K products take at most
  K rounded additions (the bias included), each within u of a partial sum that |A| . |W|^T (+ |bias|) = S bounds.
  With g = K u S an fp32 output is held to |got - r64| <= g; a bf16 output to g + h(|r64| + g), h(v) half a bf16
  ulp AT v: 2^(floor(log2 v) - 8), between 2^-9 v and 2^-8 v (bf16 keeps 8 significant bits, so a correctly rounded
  1.0039 is 2^-8 off: a flat 2^-9 |r64| would refuse correct roundings in the lower half of every binade).  K = in
  for the forward, the G operand's width for dgrad (32 for the last layer), B for wgrad and the bias row sums.  No
  element is excluded: a forward value within g of zero is covered by the absolute term; the ReLU mask of dgrad is
  read from the kernel's own act[j], so it is never ambiguous, and a masked element must be zero (bound 0).
  dlog.  r64 = (p - onehot) / B from the float64 logits.  The kernel's logits are within dz = K u max_n S of them,
  which moves p by at most p (e^(2 dz) - 1).  ``__expf`` / ``__logf`` get 2^-9 |r64|: about a thousand times the few
  fp32 ulps of an argument below 32 that they cost, while a wrong label, a wrong row maximum or a missing 1 / B is
  off by order one.  With e = 2^-9 |r64| + p (e^(2 dz) - 1) / B the bound is e + h(|r64| + e).
  Loss.  The one figure that is measured, not derived (it depends on the fast intrinsics' error): |loss - r64| / r64
  against the float64 replay (logits from the kernel's own act[nl-1]) on an MI355X over every case and step of
  test_mlp_mega_exact_gpu.py, LOSS_REL = 4 x the largest seen (profiles/mlp_mega_exact.md).  It must stay under
  1e-4: one dropped row at B = 1024 moves the mean by about 1e-3.
  Update.  ``Ref64``, ``ulp32`` and ``check`` of test_optim_gpu.py on the kernel's own gradient, per tensor: 4 x the
  fp32 CPU optimiser's error plus one fp32 ulp, as an L2 norm and per element.  ``check`` measures the per-element
  error relative to the result, which its own data is conditioned for (one gradient sign per element: "no update
  or momentum cancels to nothing").  The kernel's own gradients of fresh batches are not: in exp_avg = b1 m +
  (1 - b1) g (momentum_buffer = mom m + g) the terms cancel on some elements, and there ANY fp32 evaluation is off by
  an ulp of the operands, not of the result -- relative to the result the error has a 1 / x tail, and its largest
  sample differs between two correct evaluations by more than 4 every so often (measured on an MI355X: 8 of 10
  cases had such an element, each within one fp32 ulp of its operands, the L2 criterion passing).  So
  for these two sums (``held``) the per-element relative errors are taken against the summed magnitudes of the
  operands, b1 |m| + (1 - b1) |g| (mom |m| + |g| + wd |p|): the same criterion wherever nothing cancels, and the
  L2 criterion unchanged.  A unit that is inactive over the whole
  batch has gradients of exactly zero; where the float64 update or state is exactly zero (``check`` divides by it)
  its formula gives a bound of zero, which is what is asserted there: the kernel's value must be zero too.

Exact (``torch.equal``): actT[l] = act[l]^T, dT[l] = d[l]^T, actT[0] = bf16(x)^T, dlogT[:16] = dlog[:, :16]^T,
dlog[:, out:] and dlogT[out:] all zero bytes, d[j] = 0 wherever act[j] = 0, after the step wbf = bf16(w),
wtbf[:, :out] = wbf^T with zero pad columns, the step counter one further, ``errors() == 0``.  The update is replayed
from p.grad as stored, so the fused form (updated from the accumulators) is held to the gradient it published.

Tiles (the report names them): a row-GEMM output (F, CE, dgrad) is cut into 32 x 16 tiles, tile t = (column // 16)
(B / 32) + row // 32; a weight gradient into 64 x 64 tiles, t = (in // 64) ceil(out / 64) + out // 64, each summed in
ceil(B / 128) passes of 128 batch columns; tile t runs on workgroup t mod grid in round t // grid.

  case  model (hidden, features, classes)  B     optimiser            grid  reaches
  A     5, 1024, 10                        160   Adam                 nat.  320 forward tiles > grid (later tiles load
                                                                            their own weights), 256 gradient tiles = grid
                                                                            (fused), 2 wgrad passes, bias span 40
  B     1, 72, 10                          1024  AdamW wd 0.1         nat.  8 wgrad passes, span 256; 72 = 64 + 8 =
                                                                            4.5 x 16 = 2 x 32 + 8: partial tiles, the
                                                                            scalar tail of wt_flush
  C     2, 264, 16                         32    SGD mom 0.9 wd 1e-2  nat.  one row tile, the read-back update form,
                                                                            every class column valid
  D     0, 1024, 10                        96    SGD, no momentum     nat.  nl = 2, use_m == false, span 24
  E     1, 72, 10                          96    Adam                 8     15 forward, 15 dgrad, 26 gradient tiles on 8
                                                                            workgroups: every += gridDim.x loop, Adam in
                                                                            the read-back form
  Fp    as E, PDE_MLP_PRELOAD=0            96    Adam                 8     flag bit 0
  Ff    as E, PDE_MLP_FUSE=0               96    Adam                 nat.  flag bit 1
  G     6, 64, 10                          64    AdamW                nat.  nl = 8 = kMlpMaxLayers
  H3    1, 64, 3                           64    Adam                 3     fewer workgroups than barrier groups
  H1    1, 64, 3                           64    Adam                 1     one workgroup doing everything
  A128  as A                               128   Adam                 nat.  the shape the agreement tests use (1 step)
nl = 1 (``ce_phase<true>``) cannot be reached through MegaMLP (input and final layer always exist).
"""
import math
import os
import sys
import time
import zlib
from typing import NamedTuple, Optional

import torch

from test_optim_gpu import KEYS, TORCH, Ref64, check, ulp32

U = 2.0 ** -24
NAT = 256            # workgroups of the natural grid: one per CU of an MI355X
IN0 = 784
# 4 x the largest |loss - r64| / r64 seen on an MI355X over every case and step (profiles/mlp_mega_exact.md)
LOSS_REL = 4 * 1.21e-7
assert LOSS_REL < 1e-4


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    hidden: int
    feat: int
    classes: int
    B: int
    kind: str                  # "sgd" | "adam" | "adamw"
    hyper: dict
    grid: Optional[int] = None  # None: the natural grid
    steps: int = 3
    env: tuple = ()            # ((name, value), ...) set while the case runs
    reach: dict = {}           # premises asserted against ``Geo.reach()``

    @property
    def dims(self):
        return [IN0] + [self.feat] * (self.hidden + 1) + [self.classes]


ADAM = dict(lr=1e-3)
_E = dict(fwd_tiles=15, dgrad_tiles=15, grad_tiles=26, fused=False, multi_fwd=True, multi_dgrad=True,
          multi_grad=True, multi_ce=False, passes=1, span=24)
CASES = {c.name: c for c in [
    Case("A", 5, 1024, 10, 160, "adam", ADAM, steps=2,
         reach=dict(fwd_tiles=320, grad_tiles=256, fused=True, multi_fwd=True, multi_dgrad=True, multi_grad=False,
                    passes=2, span=40)),
    Case("B", 1, 72, 10, 1024, "adamw", dict(lr=1e-3, weight_decay=0.1),
         reach=dict(fused=True, passes=8, span=256, partial=True, multi_fwd=False)),
    Case("C", 2, 264, 16, 32, "sgd", dict(lr=0.05, momentum=0.9, weight_decay=1e-2),
         reach=dict(fused=False, ce_tiles=1, passes=1, span=8, partial=True, use_m=True)),
    Case("D", 0, 1024, 10, 96, "sgd", dict(lr=0.05), reach=dict(nl=2, fused=False, use_m=False, span=24)),
    Case("E", 1, 72, 10, 96, "adam", ADAM, grid=8, reach=_E),
    Case("Fp", 1, 72, 10, 96, "adam", ADAM, grid=8, env=(("PDE_MLP_PRELOAD", "0"),), reach=_E),
    Case("Ff", 1, 72, 10, 96, "adam", ADAM, env=(("PDE_MLP_FUSE", "0"),), reach=dict(fused=False, multi_grad=False)),
    Case("G", 6, 64, 10, 64, "adamw", dict(lr=1e-3, weight_decay=1e-2), reach=dict(nl=8, fused=True)),
    Case("H3", 1, 64, 3, 64, "adam", ADAM, grid=3,
         reach=dict(fused=False, multi_fwd=True, multi_grad=True, multi_ce=False, fwd_tiles=8)),
    Case("H1", 1, 64, 3, 64, "adam", ADAM, grid=1,
         reach=dict(fused=False, multi_fwd=True, multi_grad=True, multi_ce=True)),
    Case("A128", 5, 1024, 10, 128, "adam", ADAM, steps=1,
         reach=dict(fwd_tiles=256, multi_fwd=False, fused=True, passes=1, span=32)),
]}
TABLE = ["A", "B", "C", "D", "E", "Fp", "Ff", "G", "H3", "H1"]


class Geo:
    """Tile geometry of one case on ``grid`` workgroups, mirrored from mlp_fused.hip."""

    def __init__(self, case, grid=None, fuse_env=None):
        self.case, self.dims, self.B = case, case.dims, case.B
        self.nl = len(self.dims) - 1
        self.grid = grid if grid is not None else (case.grid or NAT)
        env = dict(case.env)
        nofuse = (env.get("PDE_MLP_FUSE", "1") if fuse_env is None else fuse_env)[:1] == "0"
        self.grad_tiles = [cdiv(self.dims[l + 1], 64) * cdiv(self.dims[l], 64) for l in range(self.nl)]
        self.fused = case.kind != "sgd" and not nofuse and max(self.grad_tiles) <= self.grid
        self.mt = self.B // 32

    def row_tiles(self, n):
        return self.mt * cdiv(n, 16)

    def reach(self):
        d, g = self.dims, self.grid
        fwd = max(self.row_tiles(d[l + 1]) for l in range(self.nl - 1))
        dgr = max([self.row_tiles(d[j]) for j in range(1, self.nl)])
        return dict(nl=self.nl, fwd_tiles=fwd, dgrad_tiles=dgr, grad_tiles=max(self.grad_tiles), ce_tiles=self.mt,
                    fused=self.fused, multi_fwd=fwd > g, multi_dgrad=dgr > g, multi_grad=max(self.grad_tiles) > g,
                    multi_ce=self.mt > g, passes=cdiv(self.B, 128), span=self.B // 4,
                    partial=any(x % 64 for x in d[1:-1]) and any(x % 16 for x in d[1:-1]),
                    use_m=self.case.kind != "sgd" or self.case.hyper.get("momentum", 0.0) != 0.0)

    def row_tile(self, row, col):
        t = (col // 16) * self.mt + row // 32
        return (f"32x16 row tile {t} (rows {row // 32 * 32}.., columns {col // 16 * 16}..), workgroup {t % self.grid}, "
                f"round {t // self.grid}")

    def grad_tile(self, layer):
        ot = cdiv(self.dims[layer + 1], 64)

        def where(o, i):
            t = (i // 64) * ot + o // 64
            return (f"64x64 gradient tile {t} (outputs {o // 64 * 64}.., inputs {i // 64 * 64}.., {cdiv(self.B, 128)} "
                    f"pass(es) of 128 batch columns), workgroup {t % self.grid}, round {t // self.grid}")
        return where


def batch(case, step):
    """x standard normal, y uniform with label 0 and label classes - 1 forced into the batch."""
    g = torch.Generator().manual_seed(zlib.crc32(case.name[:1].encode()) + 1000 * step)
    x = torch.randn(case.B, IN0, generator=g)
    y = torch.randint(0, case.classes, (case.B,), generator=g)
    y[0], y[1] = 0, case.classes - 1
    return x, y


def state_keys(case):
    if case.kind == "sgd":
        return KEYS["sgd"] if case.hyper.get("momentum", 0.0) != 0.0 else ()
    return KEYS[case.kind]


# ---------------------------------------------------------------------------------------------------------------
# the report
# ---------------------------------------------------------------------------------------------------------------
def hulp_bf16(v):
    """Half a bf16 ulp at the magnitude ``v`` (float64, >= 0): 2^(floor(log2 v) - 8); 0 at 0."""
    _, e = torch.frexp(v)
    return torch.where(v > 0, torch.ldexp(torch.ones_like(v), e - 9), torch.zeros_like(v))


class Report:
    def __init__(self, geo, step):
        self.geo, self.step = geo, step
        self.fails = []
        self.frac = {}
        self.loss_rel = None

    def elements(self, phase, layer, what, got, want, bound, where):
        """2-d ``got`` within ``bound`` of ``want`` (bound None: equal); ``where(row, col)`` names the owning tile."""
        g64 = got.double()
        err = (g64 - want).abs()
        err = torch.where(torch.isfinite(g64), err, torch.full_like(err, math.inf))
        if bound is None:
            bound = torch.zeros_like(err)
        else:
            ok = bound > 0
            f = (err[ok] / bound[ok]).max().item() if ok.any() else 0.0
            if (~ok & (err > 0)).any():
                f = math.inf
            self.frac[phase] = max(self.frac.get(phase, 0.0), f)
        bad = (err > bound).nonzero()
        if len(bad):
            r, c = bad[0].tolist()
            self.fails.append(f"step {self.step} phase {phase} layer {layer} {what}: {len(bad)} of {err.numel()} "
                              f"elements out of bound -- first (row {r}, column {c}), {where(r, c)}: got "
                              f"{g64[r, c].item()!r} want {want[r, c].item()!r} |d| {err[r, c].item():.3e} > "
                              f"{bound[r, c].item():.3e}")

    def exact(self, phase, layer, what, got, want, where):
        if got.shape != want.shape:
            self.fails.append(f"step {self.step} phase {phase} layer {layer} {what}: shape {tuple(got.shape)} for "
                              f"{tuple(want.shape)}")
        elif not torch.equal(got, want):
            self.elements(phase, layer, what, got.reshape(got.shape[0], -1), want.double().reshape(got.shape[0], -1),
                          None, where)
            if not self.fails or what not in self.fails[-1]:   # (differs only in the sign of a zero or a NaN)
                self.fails.append(f"step {self.step} phase {phase} layer {layer} {what}: not bit-identical")

    def fail(self, phase, layer, text):
        self.fails.append(f"step {self.step} phase {phase} layer {layer} {text}")


# ---------------------------------------------------------------------------------------------------------------
# the replay
# ---------------------------------------------------------------------------------------------------------------
def _params(d):
    """[w0, b0, w1, b1, ...] of a snapshot."""
    return [t for w, b in zip(d["w"], d["b"]) for t in (w, b)]


def replay_forward(geo, pre, post, rep, exact=False):
    """F_0 .. F_(nl-2) and the transposed copies; ``exact``: bit for bit (the integer fixture).  Returns the
    activations the later phases read ([bf16(x), act[1], ...]) and the largest S."""
    dims, nl = geo.dims, geo.nl
    xb = pre["x"].bfloat16()
    acts = [xb] + list(post["act"][1:])
    top = 0.0
    for l in range(nl - 1):
        A, W, b = acts[l].double(), pre["wbf"][l].double(), pre["b"][l].double()
        S = A.abs() @ W.abs().T + b.abs()
        top = max(top, S.max().item())
        r = torch.relu(A @ W.T + b)
        g = dims[l] * U * S
        if exact:   # S < 2^24: the fp32 sum IS the float64 one, whatever the order; the hand-off rounds it once
            r = r.float().bfloat16().double()
        rep.elements(f"F{l}", l, f"act[{l + 1}]", post["act"][l + 1], r, None if exact else g + hulp_bf16(r + g),
                     geo.row_tile)
    rep.exact("F0", 0, "actT[0] = bf16(x)^T", post["actT"][0], xb.T.contiguous(),
              lambda r, c: f"x^T row (input) {r}, batch column {c}")
    for l in range(1, nl):
        rep.exact(f"F{l - 1}", l - 1, f"actT[{l}] = act[{l}]^T", post["actT"][l], acts[l].T.contiguous(),
                  lambda r, c: "transposed copy of " + geo.row_tile(c, r))
    return acts, top


def verify(geo, pre, post, step=0):
    """Every phase of one step; returns the Report."""
    case, dims, nl, B = geo.case, geo.dims, geo.nl, geo.B
    rep = Report(geo, step)
    out = dims[nl]
    for name, ts in (("act", post["act"][1:]), ("actT", post["actT"]), ("d", post["d"][1:]), ("dT", post["dT"][1:]),
                     ("grad", post["gw"] + post["gb"])):
        for i, t in enumerate(ts):
            n = int(torch.isnan(t.float()).sum())
            if n:
                rep.fail("written", i, f"{name}: {n} of {t.numel()} elements still hold the NaN fill")
    acts, _ = replay_forward(geo, pre, post, rep)
    # ---- CE ---------------------------------------------------------------------------------------------------
    l = nl - 1
    A, W, b = acts[l].double(), pre["wbf"][l].double(), pre["b"][l].double()
    z = A @ W.T + b
    S = A.abs() @ W.abs().T + b.abs()
    dz = dims[l] * U * S.max(1, keepdim=True).values
    lse = torch.logsumexp(z, 1)
    p = torch.exp(z - lse[:, None])
    onehot = torch.nn.functional.one_hot(pre["y"], out).double()
    r = (p - onehot) / B
    e = 2.0 ** -9 * r.abs() + p * torch.expm1(2 * dz) / B
    dlog, dlogT = post["dlog"], post["dlogT"]
    ce_tile = lambda row, col: geo.row_tile(row, 0)  # noqa: E731
    rep.elements("CE", l, "dlog", dlog[:, :out], r, e + hulp_bf16(r.abs() + e), ce_tile)
    zero = torch.zeros((), dtype=torch.int16)
    rep.exact("CE", l, "dlog pad columns (zero bytes)", dlog[:, out:].contiguous().view(torch.int16),
              zero.expand(B, 32 - out), ce_tile)
    rep.exact("CE", l, "dlogT[:16] = dlog[:, :16]^T", dlogT[:16], dlog[:, :16].T.contiguous(),
              lambda rr, cc: "transposed copy of " + geo.row_tile(cc, 0))
    rep.exact("CE", l, "dlogT pad rows (zero bytes)", dlogT[out:].contiguous().view(torch.int16),
              zero.expand(32 - out, B), lambda rr, cc: "transposed copy of " + geo.row_tile(cc, 0))
    want = (lse - z.gather(1, pre["y"][:, None])[:, 0]).mean().item()
    rep.loss_rel = abs(post["loss"] - want) / want if math.isfinite(post["loss"]) else math.inf
    if not rep.loss_rel <= LOSS_REL:
        rep.fail("CE", l, f"loss: got {post['loss']!r} want {want!r}: relative error {rep.loss_rel:.3e} > "
                          f"{LOSS_REL:.3e}")
    # ---- backward ---------------------------------------------------------------------------------------------
    for j in range(nl - 1, -1, -1):
        last = j == nl - 1
        if j >= 1:
            G = (dlog if last else post["d"][j + 1]).double()
            Wt = pre["wtbf"][j].double()
            mask = acts[j] > 0
            r = (G @ Wt.T) * mask
            g = G.shape[1] * U * (G.abs() @ Wt.abs().T) * mask
            dj = post["d"][j]
            rep.exact(f"dgrad{j}", j, f"d[{j}] = 0 where act[{j}] = 0", torch.where(mask, torch.zeros_like(dj), dj),
                      torch.zeros_like(dj), geo.row_tile)
            rep.elements(f"dgrad{j}", j, f"d[{j}]", dj, r, g + hulp_bf16(r.abs() + g), geo.row_tile)
            rep.exact(f"dgrad{j}", j, f"dT[{j}] = d[{j}]^T", post["dT"][j], dj.T.contiguous(),
                      lambda rr, cc: "transposed copy of " + geo.row_tile(cc, rr))
        GT = (dlogT[:out] if last else post["dT"][j + 1]).double()
        AT = post["actT"][j].double()
        where = geo.grad_tile(j)
        rep.elements(f"wgrad{j}", j, "weight gradient", post["gw"][j], GT @ AT.T, B * U * (GT.abs() @ AT.abs().T),
                     where)
        rep.elements(f"wgrad{j}", j, "bias gradient", post["gb"][j][:, None], GT.sum(1, keepdim=True),
                     B * U * GT.abs().sum(1, keepdim=True), lambda o, _: "bias row of " + where(o, 0))
    # ---- update -----------------------------------------------------------------------------------------------
    verify_update(geo, pre, post, rep)
    for l in range(nl):
        wb = post["w"][l].bfloat16()
        where = geo.grad_tile(l)
        rep.exact(f"update{l}", l, "wbf = bf16(w)", post["wbf"][l], wb, where)
        if l >= 1:
            o = dims[l + 1]
            wt = post["wtbf"][l]
            rep.exact(f"update{l}", l, "wtbf[:, :out] = wbf^T", wt[:, :o].contiguous(), wb.T.contiguous(),
                      lambda i, oo: "transposed copy in " + where(oo, i))
            if wt.shape[1] > o:
                rep.exact(f"update{l}", l, "wtbf pad columns (zero bytes)", wt[:, o:].contiguous().view(torch.int16),
                          zero.expand(wt.shape[0], wt.shape[1] - o), lambda i, oo: f"input row {i}")
    if post["t"] != pre["t"] + 1:
        rep.fail("update", "-", f"the device step counter went from {pre['t']} to {post['t']}")
    if post["errors"] != 0:
        rep.fail("barrier", "-", f"errors() == {post['errors']}")
    return rep


def held(tag, what, k, r32, r64, ulp, scale):
    """test_optim_gpu.check's two criteria for a momentum sum, the per-element relative errors taken against
    ``scale`` >= |r64|, the summed magnitudes of the sum's operands (module docstring).  Without cancellation scale
    is |r64| and this is ``check`` itself."""
    assert torch.isfinite(k).all() and scale.min().item() > 0
    ek, e32 = (k - r64).abs(), (r32 - r64).abs()
    n64 = r64.norm().item()
    l2k, l232 = ek.norm().item() / n64, e32.norm().item() / n64
    l2_bound = 4 * l232 + ulp.norm().item() / n64
    rel32, relk = (e32 / scale).max().item(), (ek / scale).max().item()
    print(f"OPTIM_ERR {tag} {what}: l2 kernel {l2k:.2e} fp32 {l232:.2e} bound {l2_bound:.2e} | "
          f"max-rel-to-operands kernel {relk:.2e} fp32 {rel32:.2e}")
    assert l2k <= l2_bound, f"{tag} {what}: relative L2 error {l2k:.3e} > {l2_bound:.3e} (fp32 ref {l232:.3e})"
    worst = (ek - (4 * rel32 * scale + ulp)).max().item()
    assert worst <= 0, f"{tag} {what}: an element is {worst:.3e} past its bound (max rel {relk:.3e}, fp32 {rel32:.3e})"


def verify_update(geo, pre, post, rep, t=None):
    """update_l: the kernel's p and state after the step against Ref64 stepped from the pre-step snapshot with the
    kernel's own gradient; the bound from the fp32 CPU optimiser on the same inputs (test_optim_gpu.check)."""
    case = geo.case
    t = pre["t"] if t is None else t
    keys = state_keys(case)
    p0, grads = _params(pre), [g for w, b in zip(post["gw"], post["gb"]) for g in (w, b)]
    if not all(torch.isfinite(g).all() for g in grads):
        rep.fail("update", "-", "a gradient is not finite: the update is not replayed")
        return
    r64 = Ref64(case.kind, p0, step=t, **case.hyper)
    p32 = [p.clone().requires_grad_() for p in p0]
    o32 = TORCH[case.kind](p32, **case.hyper)
    for i, p in enumerate(p32):
        p.grad = grads[i].clone()
        st = {k: pre["state"][i][k].clone() for k in keys}
        r64.state[i] = {k: v.double() for k, v in st.items()}
        if case.kind != "sgd":
            st["step"] = torch.tensor(float(t))
        o32.state[p] = st
    o32.step()
    r64.step(grads)
    pk, sk = _params(post), post["state"]
    # the operands of the momentum sum (module docstring): what its fp32 error is relative to
    wd, scales = case.hyper.get("weight_decay", 0.0), []
    for i, p in enumerate(p0):
        g = grads[i].double().abs() + (wd * p.double().abs() if case.kind != "adamw" else 0.0)
        if case.kind == "sgd":
            scales.append(g + case.hyper.get("momentum", 0.0) * pre["state"][i]["momentum_buffer"].double().abs()
                          if keys else g)
        else:
            b1 = case.hyper.get("betas", (0.9, 0.999))[0]
            scales.append((1.0 - b1) * g + b1 * pre["state"][i]["exp_avg"].double().abs())
    for i in range(len(p0)):
        layer, name = i // 2, "weight" if i % 2 == 0 else "bias"
        b64 = p0[i].double()
        todo = [("update", pk[i].double() - b64, p32[i].detach().double() - b64, r64.p[i] - b64, ulp32(r64.p[i]))]
        for k in keys:
            s64 = r64.state[i][k]
            todo.append((k, sk[i][k].double(), o32.state[p32[i]][k].double(), s64, ulp32(s64)))
        for what, k, r32, ref, ulp in todo:
            k, r32, ref, ulp = (t.reshape(-1) for t in (k, r32, ref, ulp))
            nz = ref != 0
            if not nz.all():   # check()'s formula at a reference of exactly zero: a bound of zero
                bad = (~nz & ~(k == 0)).nonzero()
                if len(bad):
                    e = int(bad[0])
                    rep.fail(f"update{layer}", layer, f"{name} {what}: {len(bad)} elements whose float64 value is "
                                                      f"exactly zero are not -- first flat index {e}: {k[e].item()!r}")
                k, r32, ref, ulp = k[nz], r32[nz], ref[nz], ulp[nz]
            tag = f"{case.name} step {rep.step} layer {layer} {name}"
            try:
                if what in ("exp_avg", "momentum_buffer"):
                    held(tag, what, k, r32, ref, ulp, scales[i].reshape(-1)[nz])
                else:
                    check(tag, what, k, r32, ref, ulp)
            except AssertionError as exc:
                rep.fail(f"update{layer}", layer, f"{name} {what}: " + str(exc).splitlines()[0])
            ek = (k - ref).abs()
            n64 = ref.norm().item()
            if n64 > 0:
                bound = 4 * (r32 - ref).norm().item() / n64 + ulp.norm().item() / n64
                f = ek.norm().item() / n64 / bound if bound > 0 else math.inf
                rep.frac[f"update {what}"] = max(rep.frac.get(f"update {what}", 0.0), f)


# ---------------------------------------------------------------------------------------------------------------
# the step's arithmetic on the CPU (fp32 torch), with the mistakes test_mlp_mega_exact_cpu.py plants in it
# ---------------------------------------------------------------------------------------------------------------
class Mut(NamedTuple):
    """A planted mistake: ``name`` at ``layer``, element / tile origin (``a``, ``b``) and k-step ``k``.

    ulp      act[layer + 1][a, b] one bf16 ulp off, away from the value it was rounded from (towards it, an element
             that rounding left 0.49 ulp off would land 0.51 ulp off on the other side: no bound that admits a
             correct rounding of an fp32 sum with accumulation error can see that)
    swapT    actT[layer][a, b] and actT[layer][a, b + 1] exchanged (layer 0: x^T; layer >= 1 also a wgrad operand)
    swapdT   the same in dT[layer]
    kstep    the 32 x 16 forward tile of layer ``layer`` at (a, b) computed without k-step ``k`` (32 inputs)
    pass     the 64 x 64 weight-gradient tile of ``layer`` at (a, b) without its second pass (batch columns 128..255)
    bias8    bias gradient ``a`` of ``layer`` without batch columns b .. b + 7
    ge       >= for > in the ReLU mask of every dgrad
    noB      d logits without the 1 / B
    label    row ``a`` of the CE phase takes the label of row a + 1
    stale    the 64 x 64 tile at (outputs a, inputs b) of wtbf[layer] left at the pre-step weights
    count    the update runs with the previous step's count
    """
    name: str
    layer: int = 0
    a: int = 0
    b: int = 0
    k: int = 0


def _mm4(a, w):
    """a [M, K] . w [N, K]^T in fp32 with K split over the four waves (k-step ks of 32 belongs to wave ks mod 4),
    the quarters added in wave order."""
    owner = torch.arange(a.shape[1]) // 32 % 4
    acc = None
    for q in range(4):
        sel = owner == q
        if sel.any():
            part = a[:, sel] @ w[:, sel].T
            acc = part if acc is None else acc + part
    return acc


def init_pre(case, seed=0):
    """A pre-step snapshot of a freshly initialised model (uniform +-1 / sqrt(in), like nn.Linear), step count 0."""
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()) + seed)
    dims = case.dims
    w, b = [], []
    for l in range(len(dims) - 1):
        k = 1.0 / math.sqrt(dims[l])
        w.append((torch.rand(dims[l + 1], dims[l], generator=g) * 2 - 1) * k)
        b.append((torch.rand(dims[l + 1], generator=g) * 2 - 1) * k)
    pre = dict(w=w, b=b, t=0)
    derive_copies(pre)
    pre["state"] = [{k: torch.zeros_like(p) for k in state_keys(case)} for p in _params(pre)]
    return pre


def derive_copies(d):
    nl = len(d["w"])
    d["wbf"] = [w.bfloat16() for w in d["w"]]
    d["wtbf"] = [None] * nl
    for l in range(1, nl):
        o, i = d["w"][l].shape
        wt = torch.zeros(i, 32 if l == nl - 1 else o, dtype=torch.bfloat16)
        wt[:, :o] = d["wbf"][l].T
        d["wtbf"][l] = wt


def emulate(geo, pre, mut=None):
    """One step from ``pre`` (with ``x`` and ``y``): the buffers and tensors the kernel leaves, as ``post``."""
    case, dims, nl, B = geo.case, geo.dims, geo.nl, geo.B
    m = mut.name if mut else None
    out = dims[nl]
    act = [pre["x"].bfloat16()]
    for l in range(nl - 1):
        A, W = act[l].float(), pre["wbf"][l].float()
        c = _mm4(A, W)
        if m == "kstep" and mut.layer == l:
            A2 = A[mut.a:mut.a + 32].clone()
            A2[:, 32 * mut.k:32 * mut.k + 32] = 0
            c[mut.a:mut.a + 32, mut.b:mut.b + 16] = _mm4(A2, W[mut.b:mut.b + 16])
        v = torch.relu(c + pre["b"][l])
        h = v.bfloat16()
        if m == "ulp" and mut.layer == l:
            assert h[mut.a, mut.b] > 0
            h.view(torch.int16)[mut.a, mut.b] += 1 if h[mut.a, mut.b].float() >= v[mut.a, mut.b] else -1
        act.append(h)
    actT = [a.T.contiguous() for a in act]

    def swap(t):
        t[mut.a, mut.b], t[mut.a, mut.b + 1] = t[mut.a, mut.b + 1].clone(), t[mut.a, mut.b].clone()
        assert t[mut.a, mut.b] != t[mut.a, mut.b + 1]

    if m == "swapT":
        swap(actT[mut.layer])
    # ---- CE ---------------------------------------------------------------------------------------------------
    l = nl - 1
    z = _mm4(act[l].float(), pre["wbf"][l].float()) + pre["b"][l]
    y = pre["y"].clone()
    if m == "label":
        assert y[mut.a] != y[mut.a + 1]
        y[mut.a] = y[mut.a + 1]
    lse = torch.logsumexp(z, 1)
    dl = (torch.exp(z - lse[:, None]) - torch.nn.functional.one_hot(y, out).float()) * \
        (1.0 if m == "noB" else 1.0 / B)
    dlog = torch.zeros(B, 32, dtype=torch.bfloat16)
    dlog[:, :out] = dl.bfloat16()
    dlogT = torch.zeros(32, B, dtype=torch.bfloat16)
    dlogT[:16] = dlog[:, :16].T
    rows = lse - z.gather(1, y[:, None])[:, 0]
    loss = (rows.view(B // 32, 32).sum(1).sum() / B).item()   # one partial per 32-row tile, then their sum / B
    # ---- backward ---------------------------------------------------------------------------------------------
    d, dT, gw, gb = [None] * nl, [None] * nl, [None] * nl, [None] * nl
    for j in range(nl - 1, -1, -1):
        last = j == nl - 1
        if j >= 1:
            c = _mm4((dlog if last else d[j + 1]).float(), pre["wtbf"][j].float())
            a = act[j].float()
            d[j] = (c * ((a >= 0) if m == "ge" else (a > 0))).bfloat16()
            dT[j] = d[j].T.contiguous()
            if m == "swapdT" and mut.layer == j:
                swap(dT[j])
        GT, AT = (dlogT[:out] if last else dT[j + 1]).float(), actT[j].float()
        acc = torch.zeros(dims[j + 1], dims[j])
        for kb in range(0, B, 128):   # 128 batch columns per pass
            part = GT[:, kb:kb + 128] @ AT[:, kb:kb + 128].T
            if m == "pass" and mut.layer == j and kb == 128:
                part[mut.a:mut.a + 64, mut.b:mut.b + 64] = 0
            acc += part
        gw[j], gb[j] = acc, GT.sum(1)
        if m == "bias8" and mut.layer == j:
            gb[j][mut.a] = GT[mut.a].sum() - GT[mut.a, mut.b:mut.b + 8].sum()
    # ---- update: fp32 torch.optim ---------------------------------------------------------------------------
    t = pre["t"] - 1 if m == "count" else pre["t"]
    ps = [p.clone().requires_grad_() for p in _params(pre)]
    opt = TORCH[case.kind](ps, **case.hyper)
    grads = [g for pair in zip(gw, gb) for g in pair]
    for i, p in enumerate(ps):
        p.grad = grads[i].clone()
        st = {k: pre["state"][i][k].clone() for k in state_keys(case)}
        if case.kind != "sgd":
            st["step"] = torch.tensor(float(t))
        opt.state[p] = st
    opt.step()
    post = dict(act=[None] + act[1:], actT=actT, d=d, dT=dT, dlog=dlog, dlogT=dlogT, gw=gw, gb=gb, loss=loss,
                w=[p.detach() for p in ps[0::2]], b=[p.detach() for p in ps[1::2]],
                state=[{k: opt.state[p][k] for k in state_keys(case)} for p in ps], t=pre["t"] + 1, errors=0)
    derive_copies(post)
    if m == "stale":
        o0, i0 = mut.a, mut.b
        post["wtbf"][mut.layer][i0:i0 + 64, o0:o0 + 64] = pre["wtbf"][mut.layer][i0:i0 + 64, o0:o0 + 64]
    return post


def next_pre(post):
    return {k: post[k] for k in ("w", "b", "wbf", "wtbf", "state", "t")}


def emulate_case(case, steps, mut=None, mut_step=None):
    """``steps`` emulated steps of ``case``, every one replayed; the mistake planted in step ``mut_step`` (default:
    the last).  Returns the reports."""
    geo = Geo(case)
    pre = init_pre(case)
    mut_step = steps - 1 if mut_step is None else mut_step
    reps = []
    for s in range(steps):
        pre["x"], pre["y"] = batch(case, s)
        post = emulate(geo, pre, mut if s == mut_step else None)
        reps.append(verify(geo, pre, post, s))
        pre = next_pre(post)
    return reps


# ---------------------------------------------------------------------------------------------------------------
# running on the GPU: only through MegaMLP(net, opt).step(x, y)
# ---------------------------------------------------------------------------------------------------------------
def _cpu(t):
    return t.detach().cpu().clone()


class Runner:
    """A fresh model, optimiser and MegaMLP (fresh barrier words) for ``case``; ``step(s)`` takes the snapshot,
    plants the NaN fill, runs one step and returns (pre, post)."""

    def __init__(self, case, dev, grid=None, seed=0):
        from pytorch_distributed_examples_amd.models.mlp import MLP
        from pytorch_distributed_examples_amd.models.mlp_mega import MegaMLP
        from pytorch_distributed_examples_amd.ops import optim as O

        self.case, self.dev = case, dev
        torch.manual_seed(zlib.crc32(case.name[:1].encode()) + seed)
        self.net = MLP(case.hidden, case.feat, IN0, case.classes).to(dev)
        self.opt = {"sgd": O.FusedSGD, "adam": O.FusedAdam, "adamw": O.FusedAdamW}[case.kind](
            self.net.parameters(), **case.hyper)
        self.mega = MegaMLP(self.net, self.opt)
        grid = grid if grid is not None else case.grid
        if grid is not None:
            self.mega._grid = grid          # before the first launch: the barrier counts derive from gridDim.x
        self.layers = self.mega.layers
        self.bufs = self.mega._buffers(case.B, dev)

    def geo(self):
        geo = Geo(self.case, self.mega.grid(), os.environ.get("PDE_MLP_FUSE", "1"))
        assert geo.fused == self.mega.fused_update(), (geo.fused, self.mega.fused_update())
        return geo

    def _weights(self):
        from pytorch_distributed_examples_amd.ops import functional as OF

        nl = len(self.layers)
        d = dict(w=[_cpu(L.weight) for L in self.layers], b=[_cpu(L.bias) for L in self.layers])
        derive_copies(d)   # before the first step no maintained copy exists yet: it is derived as bf16(w)
        for i, L in enumerate(self.layers):
            if L.weight.__dict__.get("_pde_maint") is None:
                continue
            d["wbf"][i] = _cpu(OF._maintained(L.weight, "bf16"))
            if i > 0:
                d["wtbf"][i] = _cpu(OF.maintain_transposed_copy(L.weight, 32 if i == nl - 1 else L.out_features))
        keys = state_keys(self.case)
        d["state"] = [{k: _cpu(self.opt.state[p][k]) if k in self.opt.state[p] else torch.zeros_like(p, device="cpu")
                       for k in keys} for p in self.mega.params]
        dv = self.opt._dev.get(0)
        d["t"] = int(dv["step"][0].item()) if dv is not None else 0
        return d

    def step(self, s, xy=None):
        x, y = batch(self.case, s) if xy is None else xy
        pre = self._weights()
        pre["x"], pre["y"] = x, y
        nan = float("nan")
        for p in self.mega.params:
            if p.grad is None:
                p.grad = torch.full_like(p, nan)
            else:
                p.grad.fill_(nan)           # in place: the optimiser's tables keep the gradient's address
        b = self.bufs
        for t in b["act"][1:] + b["actT"] + b["d"][1:] + b["dT"][1:]:
            t.fill_(nan)
        loss = self.mega.step(x.to(self.dev), y.to(self.dev))
        torch.cuda.synchronize()
        post = self._weights()
        none = [None]
        post.update(act=none + [_cpu(t) for t in b["act"][1:]], actT=[_cpu(t) for t in b["actT"]],
                    d=none + [_cpu(t) for t in b["d"][1:]], dT=none + [_cpu(t) for t in b["dT"][1:]],
                    dlog=_cpu(b["dlog"]), dlogT=_cpu(b["dlogT"]), gw=[_cpu(L.weight.grad) for L in self.layers],
                    gb=[_cpu(L.bias.grad) for L in self.layers], loss=float(loss), errors=self.mega.errors())
        return pre, post


def run_case(case, dev, steps=None, grid=None):
    """Every step of ``case`` on the GPU, replayed; returns (reports, geometry, wall seconds, last post)."""
    t0 = time.perf_counter()
    old = {k: os.environ.get(k) for k, _ in case.env}
    os.environ.update(dict(case.env))
    try:
        run = Runner(case, dev, grid)
        geo = run.geo()
        reps, post = [], None
        for s in range(case.steps if steps is None else steps):
            pre, post = run.step(s)
            reps.append(verify(geo, pre, post, s))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return reps, geo, time.perf_counter() - t0, post


def describe(name, reps, geo, secs):
    """The profile lines of one case: per step, the worst ratio of error to bound of every phase, the loss figure."""
    lines = [f"case {name}: grid {geo.grid}, {'fused' if geo.fused else 'read-back'} update, {secs:.2f} s"]
    for rep in reps:
        fr = " ".join(f"{k}={v:.3f}" for k, v in rep.frac.items())
        lines.append(f"  step {rep.step}: loss_rel={rep.loss_rel:.3e} {fr}")
    return lines


def main(argv):
    """Run the named cases (none: all) on the GPU; prints the profile lines and every failure; exit 1 on a failure."""
    names = [a for a in argv if not a.startswith("--")] or list(CASES)
    dev = torch.device("cuda:0")
    failed, worst = 0, 0.0
    for n in names:
        reps, geo, secs, _ = run_case(CASES[n], dev)
        print("\n".join(describe(n, reps, geo, secs)), flush=True)
        for rep in reps:
            worst = max(worst, rep.loss_rel)
            for f in rep.fails:
                print(f"MISMATCH {n} {f}", flush=True)
            failed += bool(rep.fails)
    print(f"largest loss_rel {worst:.3e}; LOSS_REL {LOSS_REL:.3e}")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.exit(main(sys.argv[1:]))
