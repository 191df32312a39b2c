"""BatchNorm cases that can see one wrong element (test_norm_exact_cpu.py, test_norm_exact_gpu.py): the kernels of
csrc/kernels/norm_pool.hip against float64, with three separate checks per case, so that an error in the statistics
cannot hide (or cause) an error in the apply stage and the other way round.  u = 2^-24 throughout.

Data regimes
  int   x holds integers in [-lim, lim] (bf16 holds them exactly), the pivot row x[0] of every group included, and
        sum_rows (x - x[0])^2 < 2^24 per channel and group (asserted: ``premise``): every shifted partial sum the
        kernels form -- sum (x - x[0]) and sum (x - x[0])^2 -- is an integer below 2^24, exact in fp32 in ANY order.
        dy and the residual hold integers in [-3, 3], so sum dy*mask is exact too.
  rand  x ~ 3 N(0, 1) + 1, residual and dy ~ N(0, 1), all rounded to bf16: magnitudes and rounding.

Check 1, statistics against float64, per channel (and group): save_mean, save_invstd, scale, shift and the running
statistics after one and after two calls.
  int:   |d mean| <= 2u max(|mean|, |x[0]|)       (float(mean_s) and the add of the pivot: two roundings)
         |d invstd| <= 4u invstd                  (float(var), + eps, rsqrtf of <= 1 ulp: u + u/2 + 2u)
  rand:  the same plus the reduction-depth terms, D = ceil(rpb / 64) + 64 + nrb a sequential upper bound of the
         lane / LDS / chunk reduction (geometry below):
         |d mean| += D u mean|x - x[0]|,  |d var| <= 2 D u mean (x - x[0])^2 carried to invstd as
         1/2 |d var| / (var + eps) (relative) -- the pivot term is what makes a pivot outlier cost accuracy.
         This D holds for the one-launch and the two-launch form (``rpb`` / ``nrb`` of the grid that runs).
         The three-pass form (PDE_BN_3PASS) reduces in another shape, so its D is counted from k_bn_stats /
         k_bn_finalize (k_bn_bwd_reduce / k_bn_bwd_finalize are built alike): a block of 256 threads covers
         rpi = 256 / min(C / 8, 256) rows per trip, nblk blocks of rpb rows each (bn_blocks).  A summand passes
         through at most ceil(rpb / rpi) - 1 rounded additions in its thread (the first, to zero, is exact),
         rpi - 1 when thread row 0 adds the other thread rows from LDS in sequence, ceil(nblk / 64) - 1 in the
         finalizing lane's loop over the blocks' partials (first exact again) and 6 in the wave butterfly; forming
         a summand costs up to 3 roundings (d (x - mean) invstd; one for (x - x[0])^2):
         D = ceil(rpb / rpi) + rpi + ceil(nblk / 64) + 6.
  scale = gamma * invstd:        |d scale| <= (|d invstd| / invstd + 2u) |scale|
  shift = beta - mean * gamma * invstd:
         |d shift| <= |scale| |d mean| + |mean gamma| |d invstd| + 3u |mean scale| + 2u |shift|
  running_mean, per momentum update:  4u (|(1 - m) rm| + |m mean|) + m |d mean|   ((1 - m), two products, one sum)
  running_var,  per momentum update:  4u ((1 - m) rv + m unbiased) + m |d var| n / (n - 1): "within 4u relative,
         using the unbiased variance".  A grouped call makes ``groups`` updates in slice order; an earlier update's
         allowance is carried through the later ones times (1 - m).  The second call's reference starts from the
         state the kernel itself left after the first, so the allowance does not grow with the call count.
  m is the fp32 value of 0.1 and eps the fp32 value of 1e-5: what the kernels receive.

Check 2, the apply stage, every element: the float64 reference of y is built from the kernel's OWN returned
scale / shift:  ref = relu?(x scale + shift + res),  |y - ref| <= 2^-8 |ref| + 8u (|x scale| + |shift| + |res|)
(2^-8: the worst relative half-ulp of bf16; the second term: the fp32 product, the sums and their cancellation,
with or without a fused multiply-add).  dres equals the masked dy bit for bit.

Check 3, the backward, mask = (kernel y > 0) -- check 2 has pinned y --, d = dy mask, xhat = (x - mean) invstd
with the kernel's own mean / invstd:
  dbeta   int:  equals the float64 sum bit for bit (written, not accumulated); rand: |.| <= D u sum|d|
  dgamma  |.| <= D u sum|d xhat|
          A grouped call returns the sum over the groups: each group's sum has depth D, and both forms then add
          the ``groups`` sums one after another in group order (the last group's finalizer of k_bn_bwd_fused; the
          accumulating per-group calls of the multi-launch form), groups - 1 rounded additions more.  So for
          dbeta / dgamma of a grouped case, and for nothing else, D + groups - 1 stands in place of D.
  dx      ref = a d - a t1 / P - (a t2 / P) xhat,  a = gamma invstd, t1 / t2 the kernel's returned dbeta / dgamma;
          |dx - ref| <= 2^-8 |ref| + 8u (|a d| + |a t1 / P| + |a t2 / P xhat|).  Grouped calls return only the
          group SUMS of t1 / t2: there the per-group float64 sums stand in, and their own allowance
          (a / P) D u (sum|d| + |xhat| sum|d xhat|) is added.
The backward of a BatchNorm without residual recomputes the ReLU mask from x scale + shift, so an element whose
float64 pre-activation lies within check 2's fp32 term is ambiguous:
``ambiguous`` counts them and the seeds are chosen so that every case has none (asserted on the reference alone).
A second identical call must be bit-identical; the device error word must stay 0.

Geometry (bn_fin_grid): ncg = ceil(C / 64); nrb = min(chunks, target // (ncg groups), max(1, P // 64)) (>= 1),
target = min(resident cap, blocks); rpb = ceil(P / nrb); grid = ceil(P / rpb) ncg groups; rows per thread
= ceil(rpb / 64): <= 4 takes <4>, <= 8 <8>, <= 16 <16> only with PDE_BN_RC16=1, else <0>.

  name              C     N x H x W      exercises                                          variant  form
  full              64    2 x 16 x 16    one row per thread, full chunks (8 x 64 rows)      <4>      one launch
  ragged            64    10 x 10 x 10   15 chunks of 67 rows, ragged last chunk (62 rows), <4>      one launch
                                         second register row partly empty
  partial_cg        24    4 x 10 x 10    partial channel group (3 of 8 lanes)               <4>      one launch
  four_cg           200   2 x 9 x 9      4 channel groups, the last 8 channels wide, 2 x 81 <4>      one launch
  few_rows          2048  2 x 4 x 4      32 rows: fewer rows than row lanes                 <4>      one launch
  two_rows          64    2 x 1 x 1      P = 2                                              <4>      one launch
  rc8               64    4 x 100 x 100  128 chunks of 313 rows: 5 rows per thread          <8>      one launch
  stream_16 / _17   64    4 x 25 x 40/41 BnHeadroom(cap - 4) held: 4 chunks of 1000 / 1025  <0>      one launch
                                         rows, 16 / 17 rows per thread: the 8-row trips (4-row
                                         in the backward) without / with a tail
  pivot             64    10 x 10 x 10   int, x[0] += 24: a pivot outlier                   <4>      one launch
  grouped           64    8 x 8 x 8      bn_groups(4): 4 x 128 rows, 2 chunks per group     <4>      one launch
  refused           64 / 200             BnHeadroom(cap) held: the one-launch form refused  --       two launches
                                         (a refusal means target < ncg groups, so bn_fin_grid gives ONE row chunk
                                         per channel group: the refused cases run k_bn_stats_fin / k_bn_bwd_reduce_fin
                                         without a cross-chunk hand-off; that hand-off runs with several chunks only
                                         under PDE_BN_FUSED=0, in the child process of that policy)
suffixes: _i / _r the regime; p plain, a ReLU (mask from x), ra residual + ReLU (mask from y, dres).
"""
import functools
import json
import math
import os
import sys
import zlib
from typing import NamedTuple

import torch

U = 2.0 ** -24
BF = 2.0 ** -8
EPS = torch.tensor(1e-5, dtype=torch.float32).item()
MOM = torch.tensor(0.1, dtype=torch.float32).item()
EXACT_LIMIT = float(1 << 24)
TOKEN = "NORM_EXACT_OK"
ROWS, CG = 64, 64       # row lanes of a block, channels of a channel group (kBnRows, kBnCG)


# ---------------------------------------------------------------------------------------------------------------
# geometry and dispatch, mirrored from norm_pool.hip
# ---------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


class Policy(NamedTuple):
    """The PDE_BN_* switches that change the grid, the kernel variant or the launch form."""
    chunks: int = 128
    blocks: int = 256
    single_rows: int = 0
    fused: bool = True
    threepass: bool = False
    fwd_rc: bool = True
    rc8: bool = True
    rc16: bool = False

    @classmethod
    def from_env(cls, env):
        def off(k):
            return env.get(k, "")[:1] == "0"
        return cls(int(env.get("PDE_BN_CHUNKS", 128)), int(env.get("PDE_BN_BLOCKS", 256)),
                   int(env.get("PDE_BN_SINGLE_ROWS", 0)), not off("PDE_BN_FUSED"), "PDE_BN_3PASS" in env,
                   not off("PDE_BN_FWD_RC"), not off("PDE_BN_RC8"), env.get("PDE_BN_RC16", "")[:1] == "1")


class Grid(NamedTuple):
    ncg: int
    nrb: int    # row chunks actually launched: ceil(P / rpb)
    rpb: int
    grid: int   # nrb * ncg * groups

    @property
    def rows_per_thread(self):
        return cdiv(self.rpb, ROWS)


def fin_grid(P, C, groups=1, cap=256, pol=Policy()):
    """bn_fin_grid for ``P`` rows PER GROUP."""
    ncg = cdiv(C, CG)
    target = min(cap, pol.blocks)
    nrb = max(1, min(pol.chunks, target // (ncg * groups)))
    nrb = min(nrb, max(1, P // ROWS))
    if P <= pol.single_rows:
        nrb = 1
    rpb = cdiv(P, nrb)
    nrb = cdiv(P, rpb)
    return Grid(ncg, nrb, rpb, nrb * ncg * groups)


def variants(rows_per_thread, pol=Policy()):
    """(forward, backward) register variant of the one-launch kernels."""
    def pick(rc_on):
        if rc_on and rows_per_thread <= 4:
            return "<4>"
        if rc_on and pol.rc8 and rows_per_thread <= 8:
            return "<8>"
        if rc_on and pol.rc16 and rows_per_thread <= 16:
            return "<16>"
        return "<0>"
    return pick(pol.fwd_rc), pick(True)


def blocks_3pass(P, C):
    """bn_blocks: (blocks, rows per block, rows per trip) of the three-pass statistics kernels."""
    g8 = C // 8
    nb = max(1, min(cdiv(P * g8, 2048), 1024, P))
    rpb = cdiv(P, nb)
    return cdiv(P, rpb), rpb, 256 // min(g8, 256)


class Plan(NamedTuple):
    form: str       # "one" | "multi" | "3pass"
    grid: Grid      # of the form that runs
    depth: int      # D
    one: int        # what ONE bn_fwd_train / bn_bwd call adds to the one_launch counter,
    multi: int      # ... to the multi_launch counter,
    last_grid: int  # and leaves in last_grid (0: does not touch it)


def plan(case, cap=256, pol=Policy()):
    """What runs for ``case`` with ``cap`` resident blocks (before the case's own headroom) under ``pol``.

    The counters follow bn_one_launch, which counts a grid as one-launch when PDE_BN_FUSED is on and the grid fits
    the resident cap -- BEFORE bn_fwd_train / bn_bwd ask for the ticket window, which PDE_BN_3PASS withholds.  So
    under PDE_BN_3PASS a call still counts as one_launch, and a grouped call, which then falls through to one
    ungrouped call per group, counts 1 + groups times where the one-launch form counts once."""
    eff = {"": cap, "four": min(cap, 4), "all": 0}[case.headroom]
    G = case.groups
    pg = case.P // G
    top = fin_grid(pg, case.C, G, eff, pol)
    sub = fin_grid(pg, case.C, 1, eff, pol)     # the grouped recursion: one ungrouped BatchNorm per group
    fits = pol.fused and top.grid <= eff
    if fits and not pol.threepass:
        return Plan("one", top, top.rows_per_thread + ROWS + top.nrb, 1, 0, top.grid)
    one, multi, last = (1, 0, top.grid) if fits else (0, 1, 0)
    if G > 1:
        if pol.fused and sub.grid <= eff:
            one, last = one + G, sub.grid
        else:
            multi += G
    if pol.threepass:
        nblk, rpb, rpi = blocks_3pass(pg, case.C)
        return Plan("3pass", top, cdiv(rpb, rpi) + rpi + cdiv(nblk, 64) + 6, one, multi, last)
    # (a refused grouped call whose groups fit on their own would run the one-launch kernel per group: no case of
    # the table, the counters above still say what bn_one_launch counts)
    return Plan("multi", sub, sub.rows_per_thread + ROWS + sub.nrb, one, multi, last)


# ---------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    C: int
    shape: tuple            # (N, H, W)
    regime: str             # "int" | "rand"
    res: bool
    relu: bool
    groups: int = 1
    variant: str = "<4>"    # of both directions, default policy
    form: str = "one"       # default policy
    headroom: str = ""      # "" | "four" (BnHeadroom(cap - 4)) | "all" (BnHeadroom(cap))
    lim: int = 3
    pivot: int = 0
    seed: int = 0

    @property
    def P(self):
        n, h, w = self.shape
        return n * h * w


def _table():
    t = []
    modes = {"p": (False, False), "a": (False, True), "ra": (True, True)}

    def add(stem, C, shape, combos, **kw):
        for regime, mode in combos:
            res, relu = modes[mode]
            t.append(Case(f"{stem}_{regime[0]}_{mode}", C, shape, regime, res, relu, **kw))

    I, R = "int", "rand"
    add("full", 64, (2, 16, 16), [(I, "p"), (I, "a"), (I, "ra"), (R, "ra")])
    add("ragged", 64, (10, 10, 10), [(I, "a"), (I, "ra"), (R, "p"), (R, "a"), (R, "ra")])
    add("partial_cg", 24, (4, 10, 10), [(I, "a"), (R, "ra")])
    add("four_cg", 200, (2, 9, 9), [(I, "ra"), (R, "a")])
    add("few_rows", 2048, (2, 4, 4), [(I, "ra"), (R, "a")])
    add("two_rows", 64, (2, 1, 1), [(I, "p"), (R, "ra")])
    add("rc8", 64, (4, 100, 100), [(I, "a"), (R, "ra")], variant="<8>", lim=2)
    add("stream_16", 64, (4, 25, 40), [(I, "a"), (R, "ra")], variant="<0>", headroom="four")
    add("stream_17", 64, (4, 25, 41), [(I, "ra"), (R, "a")], variant="<0>", headroom="four")
    add("pivot", 64, (10, 10, 10), [(I, "a"), (I, "ra")], pivot=24)
    add("grouped", 64, (8, 8, 8), [(I, "a"), (I, "ra"), (R, "a"), (R, "ra")], groups=4)
    add("refused", 64, (10, 10, 10), [(R, "ra")], form="multi", headroom="all")
    add("refused200", 200, (2, 9, 9), [(I, "a")], form="multi", headroom="all")
    return t


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]


# ---------------------------------------------------------------------------------------------------------------
# operands and the float64 reference
# ---------------------------------------------------------------------------------------------------------------
class Ref:
    """Operands (float64, [groups, rows per group, C]) and float64 statistics of one case."""


@functools.lru_cache(maxsize=4)
def reference(name):
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) + c.seed)
    G, P, C = c.groups, c.P, c.C
    pg = P // G
    r = Ref()
    r.case = c
    if c.regime == "int":
        x = torch.randint(-c.lim, c.lim + 1, (G, pg, C), generator=g).double()
        x[:, 0, :] += c.pivot
        res = torch.randint(-3, 4, (G, pg, C), generator=g).double()
        dy = torch.randint(-3, 4, (G, pg, C), generator=g).double()
    else:
        x = (3 * torch.randn(G, pg, C, generator=g) + 1).bfloat16().double()
        res = torch.randn(G, pg, C, generator=g).bfloat16().double()
        dy = torch.randn(G, pg, C, generator=g).bfloat16().double()
    r.x, r.res, r.dy = x, (res if c.res else None), dy
    r.gamma = (torch.rand(C, generator=g) + 0.5).float().double()
    r.beta = torch.randn(C, generator=g).float().double()
    r.rm0 = (0.1 * torch.randn(C, generator=g)).float().double()
    r.rv0 = (torch.rand(C, generator=g) + 0.5).float().double()
    r.x0 = x[:, 0, :]
    r.d = x - r.x0[:, None, :]
    r.premise = r.d.pow(2).sum(1).max().item()
    r.mean = x.mean(1)
    r.var = (x - r.mean[:, None, :]).pow(2).mean(1)
    r.invstd = (r.var + EPS).rsqrt()
    r.unbiased = r.var * (pg / (pg - 1.0)) if pg > 1 else r.var
    r.scale = r.gamma * r.invstd
    r.shift = r.beta - r.mean * r.scale
    return r


def stat_bounds(r, D):
    """Check 1's allowances on mean, invstd, var, scale and shift ([groups, C] each)."""
    bm = 2 * U * torch.maximum(r.mean.abs(), r.x0.abs())
    bv = torch.zeros_like(bm)
    if r.case.regime == "rand":
        bm = bm + D * U * r.d.abs().mean(1)
        bv = 2 * D * U * r.d.pow(2).mean(1)
    bi = 4 * U * r.invstd + r.invstd * 0.5 * bv / (r.var + EPS)
    bs = (bi / r.invstd + 2 * U) * r.scale.abs()
    bh = r.scale.abs() * bm + (r.mean * r.gamma).abs() * bi + 3 * U * (r.mean * r.scale).abs() + 2 * U * r.shift.abs()
    return dict(mean=bm, invstd=bi, var=bv, scale=bs, shift=bh)


def running(r, rm, rv, means, unbiased, bm, bv, order=None):
    """The ``groups`` momentum updates in slice order from the state (rm, rv), float64, and their allowances."""
    pg = r.case.P // r.case.groups
    k = pg / (pg - 1.0) if pg > 1 else 1.0
    am, av = torch.zeros_like(rm), torch.zeros_like(rv)
    for g in (range(r.case.groups) if order is None else order):
        am = (1 - MOM) * am + 4 * U * (((1 - MOM) * rm).abs() + (MOM * means[g]).abs()) + MOM * bm[g]
        av = (1 - MOM) * av + 4 * U * ((1 - MOM) * rv + MOM * unbiased[g]) + MOM * bv[g] * k
        rm = (1 - MOM) * rm + MOM * means[g]
        rv = (1 - MOM) * rv + MOM * unbiased[g]
    return rm, rv, am, av


def ambiguous(r):
    """Elements of a ReLU case without residual whose float64 pre-activation lies within check 2's fp32 term
    8u (|x scale| + |shift|): the forward and the backward's recomputation (one with, one without a fused
    multiply-add, say) could put them on different sides of zero."""
    c = r.case
    if not c.relu or c.res:
        return 0
    xs = r.x * r.scale[:, None, :]
    pre = xs + r.shift[:, None, :]
    return int((pre.abs() <= 8 * U * (xs.abs() + r.shift.abs()[:, None, :])).sum())


# ---------------------------------------------------------------------------------------------------------------
# verification
# ---------------------------------------------------------------------------------------------------------------
class Report:
    def __init__(self, case, grid):
        self.case, self.grid = case, grid
        self.fails = []
        self.frac = {}

    def _note(self, key, err, bound):
        ok = bound > 0
        f = (err[ok] / bound[ok]).max().item() if ok.any() else 0.0
        if (~ok & (err > 0)).any():
            f = math.inf
        self.frac[key] = max(self.frac.get(key, 0.0), f)

    def channels(self, what, key, got, want, bound):
        """Per-channel [groups, C] output within ``bound`` of ``want``."""
        err = (got - want).abs()
        err = torch.where(torch.isfinite(got), err, torch.full_like(err, math.inf))
        if key:
            self._note(key, err, bound)
        bad = (err > bound).nonzero()
        if len(bad):
            g, ch = bad[0].tolist()
            self.fails.append(f"{what}: {len(bad)} of {err.numel()} channels out of bound -- first group {g} channel "
                              f"{ch} (channel group {ch // CG}): got {got[g, ch].item()!r} want {want[g, ch].item()!r} "
                              f"|d| {err[g, ch].item():.3e} > {bound[g, ch].item():.3e}")

    def elements(self, what, key, got, want, bound=None):
        """Elementwise [groups, rows, C] output within ``bound`` of ``want`` (None: equal)."""
        err = (got - want).abs()
        err = torch.where(torch.isfinite(got), err, torch.full_like(err, math.inf))
        if bound is None:
            bound = torch.zeros_like(err)
        if key:
            self._note(key, err, bound)
        bad = (err > bound).nonzero()
        if len(bad):
            g, row, ch = bad[0].tolist()
            self.fails.append(f"{what}: {len(bad)} of {err.numel()} elements out of bound -- first (row {row}, channel "
                              f"{ch}) of group {g}: row chunk {row // self.grid.rpb}, channel group {ch // CG}, lane "
                              f"{ch % CG // 8}: got {got[g, row, ch].item()!r} want {want[g, row, ch].item()!r} "
                              f"|d| {err[g, row, ch].item():.3e} > {bound[g, row, ch].item():.3e}")


def verify(name, out, pl):
    """Checks 1-3 of case ``name`` on ``out`` (CPU tensors as the bindings return them: y, mean, invstd, ss, rm1,
    rv1, rm2, rv2, dx, dgamma, dbeta, dres) for the plan ``pl`` that ran; returns the Report."""
    r = reference(name)
    c = r.case
    G, C, D = c.groups, c.C, pl.depth
    pg = c.P // G
    rep = Report(c, pl.grid)
    mean_k = out["mean"].double().view(G, C)
    inv_k = out["invstd"].double().view(G, C)
    ss = out["ss"].double().view(G, 2, C)
    scale_k, shift_k = ss[:, 0], ss[:, 1]
    # ---- check 1 ------------------------------------------------------------------------------------------------
    b = stat_bounds(r, D)
    rep.channels("save_mean", "stats", mean_k, r.mean, b["mean"])
    rep.channels("save_invstd", "stats", inv_k, r.invstd, b["invstd"])
    rep.channels("scale", "stats", scale_k, r.scale, b["scale"])
    rep.channels("shift", "stats", shift_k, r.shift, b["shift"])
    rm, rv = r.rm0, r.rv0
    for call in ("1", "2"):
        rm, rv, am, av = running(r, rm, rv, r.mean, r.unbiased, b["mean"], b["var"])
        rep.channels(f"running_mean after call {call}", "stats", out["rm" + call].double()[None], rm[None], am[None])
        rep.channels(f"running_var after call {call}", "stats", out["rv" + call].double()[None], rv[None], av[None])
        rm, rv = out["rm" + call].double(), out["rv" + call].double()   # the next call starts from the kernel's state
    if c.regime == "int":
        # the device's rsqrtf, measured: float(var) + eps as the kernel forms it, then 1 / sqrt in float64
        arg = (r.var.float() + torch.tensor(EPS, dtype=torch.float32)).double()
        rep.frac["rsqrt_u"] = ((inv_k - arg.rsqrt()).abs() / (arg.rsqrt() * U)).max().item()
    # ---- check 2 ------------------------------------------------------------------------------------------------
    xs = r.x * scale_k[:, None, :]
    pre = xs + shift_k[:, None, :]
    mag = xs.abs() + shift_k.abs()[:, None, :]
    if c.res:
        pre, mag = pre + r.res, mag + r.res.abs()
    ref = pre.clamp_min(0) if c.relu else pre
    y_k = out["y"].double().view(G, pg, C)
    rep.elements("y", "y", y_k, ref, BF * ref.abs() + 8 * U * mag)
    # ---- check 3 ------------------------------------------------------------------------------------------------
    d = r.dy * (y_k > 0) if c.relu else r.dy
    if c.res:
        rep.elements("dres", None, out["dres"].double().view(G, pg, C), d)
    xh = (r.x - mean_k[:, None, :]) * inv_k[:, None, :]
    t1, t2 = d.sum(1), (d * xh).sum(1)
    a1, a2 = d.abs().sum(1), (d * xh).abs().sum(1)
    db_k, dg_k = out["dbeta"].double(), out["dgamma"].double()
    Dg = D + G - 1      # the sum over the groups: groups - 1 additions behind each group's own reduction
    if c.regime == "int":
        assert a1.sum(0).max().item() < EXACT_LIMIT
        rep.channels("dbeta (exact)", None, db_k[None], t1.sum(0).float().double()[None],
                     torch.zeros(1, C, dtype=torch.float64))
    else:
        rep.channels("dbeta", "dbeta", db_k[None], t1.sum(0)[None], Dg * U * a1.sum(0)[None])
    rep.channels("dgamma", "dgamma", dg_k[None], t2.sum(0)[None], Dg * U * a2.sum(0)[None])
    a = r.gamma * inv_k
    extra = 0.0
    if G == 1:
        t1k, t2k = db_k[None], dg_k[None]
    else:
        t1k, t2k = t1, t2
        extra = (a.abs() / pg)[:, None, :] * D * U * (a1[:, None, :] + xh.abs() * a2[:, None, :])
    A = a[:, None, :] * d
    B = (a * t1k / pg)[:, None, :].expand_as(A)
    Cc = (a * t2k / pg)[:, None, :] * xh
    ref = A - B - Cc
    rep.elements("dx", "dx", out["dx"].double().view(G, pg, C), ref,
                 BF * ref.abs() + 8 * U * (A.abs() + B.abs() + Cc.abs()) + extra)
    return rep


# ---------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic on the CPU (fp32 torch), with the mistakes test_norm_exact_cpu.py plants in it
# ---------------------------------------------------------------------------------------------------------------
def emulate(name, mut=None, row=0, pl=None):
    """What the bindings return for case ``name``, computed on the CPU the way the kernels compute it: shifted sums
    (float64 here: exact in the int regime, better than any fp32 order in the rand regime), the finalize in
    double then fp32, the apply stages in fp32.  ``mut``: "drop" / "twice" (row ``row`` of group 0 left out of /
    counted twice in the statistics), "unwritten" (row ``row`` of y left as allocated: zeros), "biased"
    (running_var from the biased variance), "reverse" (group momentum updates in reverse order), "lanes" (two
    8-channel lanes of y exchanged within the row chunk of ``row``), "ge" (>= for > in the ReLU mask)."""
    r = reference(name)
    c = r.case
    G, C = c.groups, c.C
    pg = c.P // G
    f32 = torch.float32
    w = torch.ones(G, pg, 1, dtype=torch.float64)
    if mut == "drop":
        w[0, row] = 0
    if mut == "twice":
        w[0, row] = 2
    s1, s2 = (r.d * w).sum(1), (r.d * r.d * w).sum(1)
    mean_s = s1 / pg
    var = (s2 / pg - mean_s * mean_s).clamp_min(0)
    mean = mean_s.to(f32) + r.x0.to(f32)
    invstd = torch.rsqrt(var.to(f32) + torch.tensor(EPS, dtype=f32))
    gam, bet = r.gamma.to(f32), r.beta.to(f32)
    scale = gam * invstd
    shift = bet - mean * gam * invstd
    x32 = r.x.to(f32)
    t = x32 * scale[:, None, :] + shift[:, None, :]
    if c.res:
        t = t + r.res.to(f32)
    y = (t.clamp_min(0) if c.relu else t).bfloat16()
    if mut == "unwritten":
        y[0, row] = 0
    if mut == "lanes":
        rpb = pl.grid.rpb
        lo = row // rpb * rpb
        y[0, lo:lo + rpb, 0:16] = torch.cat([y[0, lo:lo + rpb, 8:16], y[0, lo:lo + rpb, 0:8]], -1)
    out = dict(y=y.view(c.P, C), mean=mean.reshape(-1), invstd=invstd.reshape(-1),
               ss=torch.stack([scale, shift], 1).reshape(-1))
    unb = (var if mut == "biased" or pg == 1 else var * (pg / (pg - 1.0))).to(f32)
    m = torch.tensor(MOM, dtype=f32)
    rm, rv = r.rm0.to(f32), r.rv0.to(f32)
    for call in ("1", "2"):
        for g in (reversed(range(G)) if mut == "reverse" else range(G)):
            rm = (1 - m) * rm + m * mean[g]
            rv = (1 - m) * rv + m * unb[g]
        out["rm" + call], out["rv" + call] = rm, rv
    d = r.dy.to(f32)
    if c.relu:
        d = d * ((y.float() >= 0) if mut == "ge" else (y.float() > 0))
    if c.res:
        out["dres"] = d.bfloat16().view(c.P, C)
    xh = (x32 - mean[:, None, :]) * invstd[:, None, :]
    t1 = d.double().sum(1).to(f32)
    t2 = (d * xh).double().sum(1).to(f32)
    out["dbeta"], out["dgamma"] = t1.double().sum(0).to(f32), t2.double().sum(0).to(f32)
    a = gam * invstd
    dx = a[:, None, :] * d - (a * t1 / pg)[:, None, :] - (a * t2 / pg)[:, None, :] * xh
    out["dx"] = dx.bfloat16().view(c.P, C)
    return out


# ---------------------------------------------------------------------------------------------------------------
# running on the GPU
# ---------------------------------------------------------------------------------------------------------------
def _ops():
    from pytorch_distributed_examples_amd.ops import functional as OF

    return OF._C(), OF


def run_case(name, dev="cuda", pol=Policy()):
    """Run case ``name`` twice (forward + backward through the bindings, parameter gradients written, not
    accumulated); returns (Report, stats) -- the report also holds a second call that is not bit-identical, the
    launch form or grid that ``plan`` does not predict, and a named variant the geometry does not give."""
    Cx, OF = _ops()
    r = reference(name)
    c = r.case
    dev = torch.device(dev)
    n, h, w = c.shape
    bf = torch.bfloat16

    def to(t, dt):
        return t.to(dt).to(dev).contiguous()

    x = to(r.x.view(n, h, w, c.C), bf)
    res = to(r.res.view(n, h, w, c.C), bf) if c.res else None
    dy = to(r.dy.view(n, h, w, c.C), bf)
    gamma, beta = to(r.gamma, torch.float32), to(r.beta, torch.float32)
    rm, rv = to(r.rm0, torch.float32), to(r.rv0, torch.float32)
    cap = OF.bn_launch_stats()["cap"]
    assert cap >= 8, cap
    pl = plan(c, cap, pol)
    hold = OF.BnHeadroom(cap - 4) if c.headroom == "four" else (OF.BnHeadroom(cap) if c.headroom == "all" else None)
    try:
        s0 = OF.bn_launch_stats()
        runs = []
        for _ in range(2):
            y, mean, invstd, ss = Cx.bn_fwd(x, gamma, beta, rm, rv, EPS, MOM, res, c.relu, c.groups)
            dx, dg, db, dres = Cx.bn_bwd(dy, x, y, mean, invstd, gamma, c.relu, c.res, None, None,
                                         None if c.res else ss, c.groups, False)
            o = dict(y=y, mean=mean, invstd=invstd, ss=ss, dx=dx, dgamma=dg, dbeta=db, rm=rm.clone(), rv=rv.clone())
            if c.res:
                o["dres"] = dres
            runs.append(o)
        torch.cuda.synchronize()
        s1 = OF.bn_launch_stats()
    finally:
        if hold is not None:
            hold.release()
    held_after, cap_after = Cx.bn_headroom_reserved(), OF.bn_launch_stats()["cap"]
    err = Cx.bn_error(True)
    a, b = runs
    out = {k: v.cpu().view(-1, c.C) if v.dim() == 4 else v.cpu() for k, v in a.items() if k not in ("rm", "rv")}
    out.update(rm1=a["rm"].cpu(), rv1=a["rv"].cpu(), rm2=b["rm"].cpu(), rv2=b["rv"].cpu())
    rep = verify(name, out, pl)
    if err != 0:
        rep.fails.append(f"device error word {err}")
    for k in a:
        if k not in ("rm", "rv") and not torch.equal(a[k], b[k]):
            rep.fails.append(f"{k}: the second identical call differs in {int((a[k] != b[k]).sum())} elements")
    one, multi = s1["one_launch"] - s0["one_launch"], s1["multi_launch"] - s0["multi_launch"]
    # two forward and two backward calls, each counted as ``plan`` reads bn_one_launch
    if (one, multi) != (4 * pl.one, 4 * pl.multi) or (pl.last_grid and s1["last_grid"] != pl.last_grid):
        rep.fails.append(f"expected the {pl.form} form to count one_launch +{4 * pl.one}, multi_launch "
                         f"+{4 * pl.multi}, last_grid {pl.last_grid or 'untouched'}: one_launch +{one}, multi_launch "
                         f"+{multi}, last_grid {s1['last_grid']}")
    if (held_after, cap_after) != (0, cap):
        rep.fails.append(f"after the case {held_after} blocks of headroom are still reserved, resident cap "
                         f"{cap_after} (was {cap})")
    if pol == Policy():
        fv, bv = variants(pl.grid.rows_per_thread, pol)
        if pl.form != c.form or (pl.form == "one" and (fv, bv) != (c.variant, c.variant)):
            rep.fails.append(f"the table names {c.variant} / {c.form}, the geometry gives {fv} {bv} / {pl.form} "
                             f"({pl.grid})")
    return rep, pl


# ---------------------------------------------------------------------------------------------------------------
# eval mode (bn_apply): Python-built fp32 scale / shift, check 2's bound
# ---------------------------------------------------------------------------------------------------------------
EVAL_CASES = {"eval_four_cg_ra": (200, 162, True, True), "eval_ragged_p": (64, 1000, False, False),
              "eval_few_rows_a": (2048, 32, False, True)}


def run_eval(name, dev="cuda"):
    Cx, _ = _ops()
    C, P, has_res, relu = EVAL_CASES[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    x = (3 * torch.randn(P, C, generator=g) + 1).bfloat16()
    res = torch.randn(P, C, generator=g).bfloat16() if has_res else None
    scale = ((torch.rand(C, generator=g) + 0.5) * torch.rsqrt(torch.rand(C, generator=g) + 0.5)).float()
    shift = torch.randn(C, generator=g).float()
    dev = torch.device(dev)
    y = Cx.bn_apply(x.view(1, 1, P, C).to(dev), scale.to(dev), shift.to(dev),
                    res.view(1, 1, P, C).to(dev) if has_res else None, relu)
    torch.cuda.synchronize()
    xs = x.double() * scale.double()
    pre, mag = xs + shift.double(), xs.abs() + shift.double().abs()
    if has_res:
        pre, mag = pre + res.double(), mag + res.double().abs()
    ref = pre.clamp_min(0) if relu else pre
    rep = Report(None, Grid(cdiv(C, CG), 1, P, 1))
    rep.elements("y (eval)", "y", y.cpu().double().view(1, P, C), ref[None], (BF * ref.abs() + 8 * U * mag)[None])
    return rep


# ---------------------------------------------------------------------------------------------------------------
# child-process entry
# ---------------------------------------------------------------------------------------------------------------
def main(argv):
    """Run the named cases (none named: the whole table and the eval cases) under the PDE_BN_* policy of the
    environment; failures go to stdout, then a ``FRACTIONS`` line (worst observed fraction of each bound, the
    measured rsqrtf error in u, the launch forms and variants that ran) and ``NORM_EXACT_OK <count>`` (exit 0) if
    there were none, exit 1 otherwise."""
    _, OF = _ops()
    pol = Policy.from_env(os.environ)
    names = [a for a in argv if not a.startswith("--")] or NAMES + list(EVAL_CASES)
    failed, frac, seen = 0, {}, set()
    for n in names:
        sys.stderr.write(f"[case] {n}\n")
        sys.stderr.flush()
        if n in EVAL_CASES:
            rep = run_eval(n)
        else:
            rep, pl = run_case(n, "cuda", pol)
            fv, bv = variants(pl.grid.rows_per_thread, pol)
            seen.add(f"{pl.form}{fv}{bv}" if pl.form == "one" else pl.form)
            if n.startswith("stream_") and pl.form == "one" and pol.rc16 and pol.single_rows == 0:
                want = "<16>" if n.startswith("stream_16") else "<0>"
                if (fv, bv) != (want, want) or pl.grid.nrb != 4:
                    rep.fails.append(f"PDE_BN_RC16=1: expected {want} on 4 chunks, the geometry gives {fv} {bv} "
                                     f"{pl.grid}")
        OF.check_device_errors(n)
        for f in rep.fails:
            print(f"MISMATCH {n} {f}")
        failed += bool(rep.fails)
        for k, v in rep.frac.items():
            frac[k] = max(frac.get(k, 0.0), v)
    print("FRACTIONS " + json.dumps(dict(frac=frac, forms=sorted(seen))))
    if failed:
        print(f"{failed} of {len(names)} cases fail")
        return 1
    print(f"{TOKEN} {len(names)}")
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.exit(main(sys.argv[1:]))
