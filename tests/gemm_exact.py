"""Exact GEMM / implicit-GEMM convolution cases (test_gemm_exact_cpu.py, test_gemm_exact_gpu.py): bf16 operands
filled with small integers, so every product is an integer and -- while sum_k |a||b| < 2^24 -- every fp32 partial
sum is exact in ANY order: any tile, split-K, slab-reduction order or MFMA accumulation order must reproduce the
float64 reference bit for bit.  The compare is ``torch.equal``; there is no tolerance.

Operands: bf16-output ops take entries uniform in {-1, 0, 1} (bias / added ``aux`` integers in [-3, 3], a DReLU
mask of any bf16 with random signs), so every reference value stays <= 256 and is a bf16 number; fp32-output ops
take entries in [-3, 3] (9 K < 2^24), accumulating ones start from an integer fp32 base.  Every op that takes
``out`` gets it pre-filled with a sentinel (0.5: no integer result equals it), as a row view of a wider pitch
where the binding allows views and between guard zones otherwise, and the WHOLE buffer is compared: every
element inside written, nothing outside touched.  Operand row views carry 7s in their pad columns.

Shapes are in linear form (x [M, K], w [N, K]); ``gemm`` is what the kernel sees as M x N x K.  The path column
is what PDE_GEMM_LOG shows under the default policy (asserted by test_gemm_exact_gpu.py's logging child):

  name                     binding call                                    gemm M x N x K      default path
  fwd_64_fast              linear_fwd 130x40x70, bias                      130 x 70 x 40       64x64 (FAST loaders)
  fwd_64_generic_k         linear_fwd 130x50x70, bias + ReLU               130 x 70 x 50       64x64 (K % 8 != 0: generic)
  fwd_64_generic_pitch     linear_fwd_out 130x48x70, x pitch 52, out 75    130 x 70 x 48       64x64 (pitch % 8 != 0: generic)
  fwd_out_f32_pitch        linear_fwd_out 130x40x70 fp32, out pitch 72     130 x 70 x 40       64x64
  dgrad_out_pitch          linear_dgrad_out 130x72x40, mask, pitches       130 x 40 x 72       64x64
  fwd_128x32               linear_fwd 200x72x10, bias                      200 x 10 x 72       128x32
  fwd_128x32_generic       linear_fwd 200x50x10 fp32                       200 x 10 x 50       128x32 (generic)
  fwd_32x128               linear_fwd 8x64x130, ReLU                       8 x 130 x 64        32x128
  skinny_fwd_a / _b        linear_fwd 72x2056x40 / 200x4096x96, bias+ReLU  as written          skinny (K-contiguous B)
  skinny_dgrad_a / _b      linear_dgrad of the same shapes, DReLU mask     as written          skinny (row-contiguous B)
  lowk_64 / lowk_128       linear_fwd 4100x40x200 bias / 4096x32x128 ReLU  as written          lowk, 64- / 128-wide strip
  wgrad_lanes1 / 4 / 16    linear_wgrad dy [rows, 70], x [rows, 132];      70 x 132 x rows     64x64 split-K + vector reduce with
                           rows 512 / 2048 / 16384                                             1 / 4 / 16 slab lanes (split 2 / 8 / 64)
  wgrad_scalar_reduce      linear_wgrad dy [2048, 70], x [2048, 130]       70 x 130 x 2048     64x64 split-K + scalar reduce (N % 4)
  wgrad_accum              linear_wgrad(out, accumulate=True), 2048 rows   70 x 132 x 2048     64x64 split-K, 4 lanes
  wgrad_out_unsplit        linear_wgrad(out), 200 rows                     70 x 132 x 200      64x64
  wgrad_bias_split(+_acc)  linear_wgrad_bias, 2048 rows, K = 131           70 x 132 x 2048     64x64 split-K, 4 lanes
  wgrad_bias_unsplit(+_acc) linear_wgrad_bias, 200 rows, K = 50            70 x 51 x 200       64x64
  pair_dense               linear_dgrad (mask) + linear_wgrad in gemm_pair 264x136x72 + 72x136x264   pair
  pair_skinny              skinny dgrad + tile wgrad in gemm_pair          72x40x264 + 264x40x72     pair-skinny
  pair_both_split          dgrad + wgrad, both split-K                     1032x72x1024 + 1024x72x1032  pair, both split (4 lanes)
  pair_conv_s1 / _s2       conv dgrad (kind 3) + wgrad (kind 2), 3x2       see the case        pair
  pair_conv1x1_s1 / _s2    1x1 conv_dgrad(w_fwd_layout=True) + wgrad       see the case        pair
  pair_conv_deferred       3x3 40 -> 40 channels, 9 x 12 x 10, defer_second, 1080x40x360 + 40x360x1080  pair; second split, reduced by
                           OIHW + accumulate, then the deferred flush                          gemm_reduce_jobs
  conv40_fwd               the same conv forward, unpaired                 1080 x 40 x 360     64x64 (kind 1 gather)
  conv_<g>_fwd/dgrad/wgrad N=3, H=7 (8 for g = rows), W=10, Ci=5 (8), Co=12 (16): (R,S) = (3,2), (1,3), stride 1 / 2, pad 0 / 1;
                           forward (bias + ReLU; fp32 + bias), dgrad (plain, DReLU, add_aux), wgrad (written,
                           accumulated): narrow tiles (N <= 32: 128x32; else M <= 32: 32x128)
  mnist2_fwd/dgrad/wgrad   8 x 12 x 12 x 16 -> 24, 5x5 (K = 400)           512x24x400 ...      128x32, 128x32 split-K, 32x128 split-K
  layout_<g>               nchw_to_nhwc, conv_w_fwd, conv_w_dgrad against permute / pad, bitwise
  forced_fwd_skinny        linear_fwd 200x520x136, bias                    200 x 136 x 520     skinny
  forced_fwd               linear_fwd 200x200x136, bias + ReLU             200 x 136 x 200     64x64
  forced_wgrad             linear_wgrad dy [2048, 136], x [2048, 264]      136 x 264 x 2048    64x64 split-K, 4 lanes

``forced``: every GEMM of the case has M, N >= 128 -- the cases the forced 128-tile DMA children run.
"""
import functools
import re
import sys
import zlib
from typing import Callable, NamedTuple, Optional

import torch
import torch.nn.functional as F

SENT = 0.5          # sentinel of pre-filled outputs and guard zones: no integer result equals it
PADV = 7.0          # pad columns of operand row views: read as data they would change every output
GUARD = 64          # elements before / after a contiguous ``out``
TOKEN = "GEMM_EXACT_OK"
EXACT_LIMIT = float(1 << 24)
BF16_LIMIT = 256.0


def pad8(c):
    return (c + 7) // 8 * 8


class E(NamedTuple):
    """One expected PDE_GEMM_LOG line: ``what`` (prefix), the GEMM's M, N, K, the tile (None: not compared), and
    the split: None unsplit; 1 / 4 / 16 split-K with that many slab lanes in the vector reduce; 0 split-K with the
    scalar reduce (N % 4 != 0)."""
    what: str
    M: int
    N: int
    K: int
    tile: Optional[str] = "64x64"
    lanes: Optional[int] = None


class Prepared:
    """Operands, references and the launch of one case; everything but ``launch`` lives on the CPU in float64.
    refs / dtypes / bounds are keyed by output name; a ref is the expected content of the WHOLE output buffer."""

    def __init__(self):
        self.refs = {}      # name -> float64 tensor
        self.dtypes = {}    # name -> dtype the kernel writes
        self.bounds = {}    # name -> max over outputs of sum_k |a||b| + |epilogue terms|
        self.values = {}    # name -> the computed values inside the buffer (what the bf16 limit applies to)
        self.gemms = []     # (A [M, K], B [K, N]) of every dense product: the linear controls
        self.convs = []     # dict(x, w, dy, stride, pad) of every convolution: the conv controls
        self.launch = None  # dev -> {name: device tensor}

    def add(self, name, ref, dtype, bound, values=None):
        self.refs[name] = ref.double()
        self.dtypes[name] = dtype
        self.bounds[name] = float(bound)
        self.values[name] = (ref if values is None else values).double()


class Case(NamedTuple):
    name: str
    build: Callable[[], Prepared]
    expect: tuple      # of E
    forced: bool = False


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def ints(g, shape, lim):
    """Integers uniform in [-lim, lim], float64."""
    return torch.randint(-lim, lim + 1, tuple(shape), generator=g).double()


def signs(g, shape):
    """A DReLU mask operand: random normals rounded to bf16 (any magnitude, random signs)."""
    return torch.randn(tuple(shape), generator=g).bfloat16().double()


def _dev(t, dtype, dev):
    return t.to(dtype).to(dev).contiguous()


def _row_view(t, pitch, dtype, dev, fill=PADV):
    """t [rows, cols] as a view of a [rows, pitch] device buffer whose pad columns hold ``fill``."""
    buf = torch.full((t.shape[0], pitch), fill, dtype=dtype, device=dev)
    buf[:, :t.shape[1]] = t.to(dtype).to(dev)
    return buf[:, :t.shape[1]]


def _pitched(ref, pitch, base=None):
    """Expected whole buffer of an output written through a [rows, pitch] row view."""
    full = torch.full((ref.shape[0], pitch), SENT, dtype=torch.float64)
    full[:, :ref.shape[1]] = ref if base is None else base + ref
    return full


def _guarded(ref, base=None):
    """Expected whole buffer of a contiguous output between two guard zones."""
    full = torch.full((GUARD + ref.numel() + GUARD,), SENT, dtype=torch.float64)
    full[GUARD:GUARD + ref.numel()] = (ref if base is None else base + ref).reshape(-1)
    return full


def _guard_buf(shape, dtype, dev, base=None):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((GUARD + n + GUARD,), SENT, dtype=dtype, device=dev)
    out = buf[GUARD:GUARD + n].view(*shape)
    if base is not None:
        out.copy_(base.to(dtype).to(dev))
    return buf, out


def _ops():
    from pytorch_distributed_examples_amd.ops import functional as OF

    return OF._C(), OF


# ---------------------------------------------------------------------------------------------------------------
# dense cases
# ---------------------------------------------------------------------------------------------------------------
def _fwd(name, M, K, N, bias=False, relu=False, f32=False, out_pitch=None, x_pitch=None):
    def build():
        g = _gen(name)
        lim = 3 if f32 else 1
        x, w = ints(g, (M, K), lim), ints(g, (N, K), lim)
        b = ints(g, (N,), 3) if bias else None
        ref = x @ w.t() + (b if bias else 0)
        if relu:
            ref = ref.clamp_min(0)
        p = Prepared()
        dt = torch.float32 if f32 else torch.bfloat16
        bound = (x.abs() @ w.abs().t()).max() + (3 if bias else 0)
        p.add("y", ref if out_pitch is None else _pitched(ref, out_pitch), dt, bound, ref)
        p.gemms.append((x, w.t()))

        def launch(dev):
            C, _ = _ops()
            wd = _dev(w, torch.bfloat16, dev)
            bd = _dev(b, torch.float32, dev) if bias else None
            xd = _dev(x, torch.bfloat16, dev) if x_pitch is None else _row_view(x, x_pitch, torch.bfloat16, dev)
            if out_pitch is None and x_pitch is None:
                return {"y": C.linear_fwd(xd, wd, bd, relu, f32)}
            pitch = N if out_pitch is None else out_pitch
            buf = torch.full((M, pitch), SENT, dtype=dt, device=dev)
            C.linear_fwd_out(xd, wd, bd, relu, buf[:, :N])
            return {"y": buf}

        p.launch = launch
        return p

    return build


def _dgrad(name, M, K, N, mask=False, out_pitch=None, dy_pitch=None, aux_pitch=None):
    """dx [M, N] = dy [M, K] . w [K, N] (* (aux > 0))."""
    def build():
        g = _gen(name)
        dy, w = ints(g, (M, K), 1), ints(g, (K, N), 1)
        aux = signs(g, (M, N)) if mask else None
        ref = dy @ w
        if mask:
            ref = ref * (aux > 0)
        p = Prepared()
        p.add("dx", ref if out_pitch is None else _pitched(ref, out_pitch), torch.bfloat16,
              (dy.abs() @ w.abs()).max(), ref)
        p.gemms.append((dy, w))

        def launch(dev):
            C, _ = _ops()
            wd = _dev(w, torch.bfloat16, dev)
            if out_pitch is None:
                return {"dx": C.linear_dgrad(_dev(dy, torch.bfloat16, dev), wd,
                                             _dev(aux, torch.bfloat16, dev) if mask else None)}
            dyd = _row_view(dy, dy_pitch or K, torch.bfloat16, dev)
            auxd = _row_view(aux, aux_pitch or N, torch.bfloat16, dev, fill=-1.0) if mask else None
            buf = torch.full((M, out_pitch), SENT, dtype=torch.bfloat16, device=dev)
            C.linear_dgrad_out(dyd, wd, auxd, buf[:, :N])
            return {"dx": buf}

        p.launch = launch
        return p

    return build


def _wgrad(name, rows, N, K, out=False, accumulate=False):
    """dW [N, K] = dy [rows, N]^T . x [rows, K], fp32."""
    def build():
        g = _gen(name)
        dy, x = ints(g, (rows, N), 3), ints(g, (rows, K), 3)
        base = ints(g, (N, K), 50) if accumulate else None
        ref = dy.t() @ x
        p = Prepared()
        bound = (dy.abs().t() @ x.abs()).max() + (50 if accumulate else 0)
        p.add("dw", _guarded(ref, base) if out else ref, torch.float32, bound, ref if base is None else ref + base)
        p.gemms.append((dy.t(), x))

        def launch(dev):
            C, _ = _ops()
            dyd, xd = _dev(dy, torch.bfloat16, dev), _dev(x, torch.bfloat16, dev)
            if not out:
                return {"dw": C.linear_wgrad(dyd, xd)}
            buf, o = _guard_buf((N, K), torch.float32, dev, base)
            C.linear_wgrad(dyd, xd, o, accumulate)
            return {"dw": buf}

        p.launch = launch
        return p

    return build


def _wgrad_bias(name, rows, N, K, dy_pitch, x_pitch, accumulate=False):
    """dW [N, K] and db [N] from ONE GEMM over x_ext = [x | 1] (linear_wgrad_bias), operands as row views."""
    def build():
        g = _gen(name)
        dy, x = ints(g, (rows, N), 3), ints(g, (rows, K), 3)
        xe = torch.cat([x, torch.ones(rows, 1, dtype=torch.float64)], 1)
        bw = ints(g, (N, K), 50) if accumulate else None
        bb = ints(g, (N,), 50) if accumulate else None
        rw, rb = dy.t() @ x, dy.sum(0)
        p = Prepared()
        bound = (dy.abs().t() @ xe.abs()).max() + (50 if accumulate else 0)
        p.add("dw", _guarded(rw, bw), torch.float32, bound, rw if bw is None else rw + bw)
        p.add("db", _guarded(rb, bb), torch.float32, bound, rb if bb is None else rb + bb)
        p.gemms.append((dy.t(), xe))

        def launch(dev):
            C, _ = _ops()
            dyd = _row_view(dy, dy_pitch, torch.bfloat16, dev)
            xd = _row_view(xe, x_pitch, torch.bfloat16, dev)
            wbuf, ow = _guard_buf((N, K), torch.float32, dev, bw)
            bbuf, ob = _guard_buf((N,), torch.float32, dev, bb)
            C.linear_wgrad_bias(dyd, xd, ow, ob, accumulate)
            return {"dw": wbuf, "db": bbuf}

        p.launch = launch
        return p

    return build


def _pair_linear(name, B, Nl, Kl, mask=True, accumulate=False):
    """A linear layer's backward in one paired launch: dx [B, Kl] = dy [B, Nl] . w [Nl, Kl] (* mask) and
    dW [Nl, Kl] = dy^T . x."""
    def build():
        g = _gen(name)
        dy, w, x = ints(g, (B, Nl), 1), ints(g, (Nl, Kl), 1), ints(g, (B, Kl), 1)
        aux = signs(g, (B, Kl)) if mask else None
        base = ints(g, (Nl, Kl), 50) if accumulate else None
        rdx = dy @ w
        if mask:
            rdx = rdx * (aux > 0)
        rdw = dy.t() @ x
        p = Prepared()
        p.add("dx", rdx, torch.bfloat16, (dy.abs() @ w.abs()).max())
        p.add("dw", _guarded(rdw, base), torch.float32, (dy.abs().t() @ x.abs()).max() + (50 if accumulate else 0),
              rdw if base is None else rdw + base)
        p.gemms += [(dy, w), (dy.t(), x)]

        def launch(dev):
            C, OF = _ops()
            dyd, wd, xd = (_dev(t, torch.bfloat16, dev) for t in (dy, w, x))
            auxd = _dev(aux, torch.bfloat16, dev) if mask else None
            buf, o = _guard_buf((Nl, Kl), torch.float32, dev, base)
            with OF.gemm_pair():
                dx = C.linear_dgrad(dyd, wd, auxd)
                C.linear_wgrad(dyd, xd, o, accumulate)
            return {"dx": dx, "dw": buf}

        p.launch = launch
        return p

    return build


# ---------------------------------------------------------------------------------------------------------------
# convolution cases
# ---------------------------------------------------------------------------------------------------------------
class Geom(NamedTuple):
    n: int
    h: int
    w: int
    ci: int
    co: int
    r: int
    s: int
    stride: int
    pad: int

    @property
    def ho(self):
        return (self.h + 2 * self.pad - self.r) // self.stride + 1

    @property
    def wo(self):
        return (self.w + 2 * self.pad - self.s) // self.stride + 1

    @property
    def cp(self):
        return pad8(self.ci)

    @property
    def cop(self):
        return pad8(self.co)


def conv_all(x, w, dy, stride, pad):
    """float64 CPU convolution of NCHW x with OIHW w, and its autograd: (y, dx, dw) for the output gradient dy."""
    xr, wr = x.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
    y = F.conv2d(xr, wr, None, stride=stride, padding=pad)
    y.backward(dy)
    return y.detach(), xr.grad, wr.grad


def nhwc(t, cpad, fill=None, g=None):
    """NCHW -> NHWC with the channels padded to ``cpad``: zeros, or integers in [-fill, fill] (what a kernel
    must never let through: the matching weight columns are zero, the OIHW remap drops them)."""
    t = t.permute(0, 2, 3, 1)
    c = t.shape[-1]
    if cpad == c:
        return t.contiguous()
    tail = torch.zeros(*t.shape[:-1], cpad - c, dtype=t.dtype) if fill is None else ints(g, (*t.shape[:-1], cpad - c),
                                                                                          fill)
    return torch.cat([t, tail], -1).contiguous()


def w_fwd_layout(w, cp, cop):
    """[Co, Ci, R, S] -> [Cop, R*S*Cp], k = (kh, kw, c), zero padded."""
    co, ci, r, s = w.shape
    t = F.pad(w.permute(0, 2, 3, 1), (0, cp - ci, 0, 0, 0, 0, 0, cop - co))
    return t.reshape(cop, r * s * cp).contiguous()


def w_dgrad_layout(w, cp, cop):
    """[Co, Ci, R, S] -> [Cip, R*S*Cop], k = (kh, kw, co), zero padded."""
    co, ci, r, s = w.shape
    t = F.pad(w.permute(1, 2, 3, 0), (0, cop - co, 0, 0, 0, 0, 0, cp - ci))
    return t.reshape(cp, r * s * cop).contiguous()


def _conv_operands(name, G, lim):
    g = _gen(name)
    x = ints(g, (G.n, G.ci, G.h, G.w), lim)
    w = ints(g, (G.co, G.ci, G.r, G.s), lim)
    dy = ints(g, (G.n, G.co, G.ho, G.wo), lim)
    return g, x, w, dy


def _conv_fwd(name, G):
    def build():
        g, x, w, dy = _conv_operands(name, G, 1)
        b = ints(g, (G.co,), 3)
        y, _, _ = conv_all(x, w, dy, G.stride, G.pad)
        bound = conv_all(x.abs(), w.abs(), dy, G.stride, G.pad)[0].max() + 3
        yb = y + b.view(1, -1, 1, 1)
        p = Prepared()
        p.add("y_bias_relu", nhwc(yb.clamp_min(0), G.cop), torch.bfloat16, bound)
        p.add("y_f32", nhwc(yb, G.cop), torch.float32, bound)
        p.convs.append(dict(x=x, w=w, dy=dy, stride=G.stride, pad=G.pad))

        def launch(dev):
            C, _ = _ops()
            xd = _dev(nhwc(x, G.cp), torch.bfloat16, dev)
            wf = _dev(w_fwd_layout(w, G.cp, G.cop), torch.bfloat16, dev)
            bd = _dev(b, torch.float32, dev)
            return {"y_bias_relu": C.conv_fwd(xd, wf, bd, G.r, G.s, G.stride, G.pad, True, False),
                    "y_f32": C.conv_fwd(xd, wf, bd, G.r, G.s, G.stride, G.pad, False, True)}

        p.launch = launch
        return p

    return build


def _conv_dgrad(name, G, fwd_layout=False):
    def build():
        g, x, w, dy = _conv_operands(name, G, 1)
        _, dx, _ = conv_all(x, w, dy, G.stride, G.pad)
        bound = conv_all(x, w.abs(), dy.abs(), G.stride, G.pad)[1].max() + 3
        mask = signs(g, (G.n, G.h, G.w, G.cp))
        add = ints(g, (G.n, G.h, G.w, G.cp), 3)
        dxn = nhwc(dx, G.cp)
        p = Prepared()
        p.add("dx", dxn, torch.bfloat16, bound)
        p.add("dx_drelu", dxn * (mask > 0), torch.bfloat16, bound)
        p.add("dx_add_aux", dxn + add, torch.bfloat16, bound)
        p.convs.append(dict(x=x, w=w, dy=dy, stride=G.stride, pad=G.pad))

        def launch(dev):
            C, _ = _ops()
            dyd = _dev(nhwc(dy, G.cop, 1, g), torch.bfloat16, dev)
            wl = w_fwd_layout(w, G.cp, G.cop) if fwd_layout else w_dgrad_layout(w, G.cp, G.cop)
            wd = _dev(wl, torch.bfloat16, dev)
            a = (G.h, G.w, G.r, G.s, G.stride, G.pad)
            return {"dx": C.conv_dgrad(dyd, wd, *a, None, fwd_layout),
                    "dx_drelu": C.conv_dgrad(dyd, wd, *a, _dev(mask, torch.bfloat16, dev), fwd_layout),
                    "dx_add_aux": C.conv_dgrad(dyd, wd, *a, _dev(add, torch.bfloat16, dev), fwd_layout, True)}

        p.launch = launch
        return p

    return build


def _conv_wgrad(name, G):
    def build():
        g, x, w, dy = _conv_operands(name, G, 3)
        _, _, dw = conv_all(x, w, dy, G.stride, G.pad)
        bound = conv_all(x.abs(), w, dy.abs(), G.stride, G.pad)[2].max() + 50
        base = ints(g, tuple(w.shape), 50)
        p = Prepared()
        p.add("dw", _guarded(dw), torch.float32, bound, dw)
        p.add("dw_accum", _guarded(dw, base), torch.float32, bound, dw + base)
        p.convs.append(dict(x=x, w=w, dy=dy, stride=G.stride, pad=G.pad))

        def launch(dev):
            C, _ = _ops()
            xd = _dev(nhwc(x, G.cp, 3, g), torch.bfloat16, dev)
            dyd = _dev(nhwc(dy, G.cop, 3, g), torch.bfloat16, dev)
            a = (G.r, G.s, G.stride, G.pad, G.co, G.ci)
            b0, o0 = _guard_buf(tuple(w.shape), torch.float32, dev)
            b1, o1 = _guard_buf(tuple(w.shape), torch.float32, dev, base)
            C.conv_wgrad(dyd, xd, *a, o0, False)
            C.conv_wgrad(dyd, xd, *a, o1, True)
            return {"dw": b0, "dw_accum": b1}

        p.launch = launch
        return p

    return build


def _pair_conv(name, G, fwd_layout=False, defer=False, accumulate=False, aux="drelu"):
    """A conv layer's backward in one paired launch: conv_dgrad + conv_wgrad(out, accumulate) inside gemm_pair;
    defer: the wgrad's slabs are left to the batched deferred reduction, flushed right after."""
    def build():
        g, x, w, dy = _conv_operands(name, G, 1)
        _, dx, dw = conv_all(x, w, dy, G.stride, G.pad)
        ab = conv_all(x.abs(), w.abs(), dy.abs(), G.stride, G.pad)
        mask = signs(g, (G.n, G.h, G.w, G.cp)) if aux == "drelu" else None
        base = ints(g, tuple(w.shape), 50) if accumulate else None
        dxn = nhwc(dx, G.cp)
        p = Prepared()
        p.add("dx", dxn * (mask > 0) if mask is not None else dxn, torch.bfloat16, ab[1].max())
        p.add("dw", _guarded(dw, base), torch.float32, ab[2].max() + 50, dw if base is None else dw + base)
        p.convs.append(dict(x=x, w=w, dy=dy, stride=G.stride, pad=G.pad))

        def launch(dev):
            C, OF = _ops()
            from pytorch_distributed_examples_amd.ops import streams

            xd = _dev(nhwc(x, G.cp), torch.bfloat16, dev)
            dyd = _dev(nhwc(dy, G.cop), torch.bfloat16, dev)
            wl = w_fwd_layout(w, G.cp, G.cop) if fwd_layout else w_dgrad_layout(w, G.cp, G.cop)
            wd = _dev(wl, torch.bfloat16, dev)
            md = _dev(mask, torch.bfloat16, dev) if mask is not None else None
            buf, o = _guard_buf(tuple(w.shape), torch.float32, dev, base)
            with OF.gemm_pair(defer_second=defer, flush_by_caller=True):
                dxd = C.conv_dgrad(dyd, wd, G.h, G.w, G.r, G.s, G.stride, G.pad, md, fwd_layout)
                C.conv_wgrad(dyd, xd, G.r, G.s, G.stride, G.pad, G.co, G.ci, o, accumulate)
            if defer:
                streams.flush_deferred()
                assert C.gemm_deferred_count() == 0
            return {"dx": dxd, "dw": buf}

        p.launch = launch
        return p

    return build


def _layout(name, G):
    def build():
        g = _gen(name)
        x = ints(g, (G.n, G.ci, G.h, G.w), 100)
        w = ints(g, (G.co, G.ci, G.r, G.s), 100)
        p = Prepared()
        p.add("nhwc", nhwc(x, G.cp), torch.bfloat16, 0)
        p.add("w_fwd", w_fwd_layout(w, G.cp, G.cop), torch.bfloat16, 0)
        p.add("w_dgrad", w_dgrad_layout(w, G.cp, G.cop), torch.bfloat16, 0)

        def launch(dev):
            C, _ = _ops()
            wd = _dev(w, torch.float32, dev)
            return {"nhwc": C.nchw_to_nhwc(_dev(x, torch.float32, dev), G.cp),
                    "w_fwd": C.conv_w_fwd(wd, G.cp, G.cop), "w_dgrad": C.conv_w_dgrad(wd, G.cp, G.cop)}

        p.launch = launch
        return p

    return build


# ---------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------
def _tile(M, N):
    """Tile of an unpaired GEMM the 128x128 threshold does not reach: narrow problems take narrow tiles."""
    return "128x32" if N <= 32 else ("32x128" if M <= 32 else "64x64")


def _conv_expect(G, part):
    m_out, k_fwd = G.n * G.ho * G.wo, G.r * G.s * G.cp
    if part == "fwd":
        return (E("single", m_out, G.cop, k_fwd, _tile(m_out, G.cop)),)
    if part == "dgrad":
        m = G.n * G.h * G.w
        return (E("single", m, G.cp, G.r * G.s * G.cop, _tile(m, G.cp)),)
    return (E("single", G.co, k_fwd, m_out, _tile(G.co, k_fwd)),)


# N = 3 images of 7 x 10: the 64-row tiles straddle image boundaries at odd offsets; `rows`: H = 8 with a 3-high
# window at stride 2 leaves (8 - 3) % 2 = 1 input row no window owns (exactly zero gradient); 1x3 at stride 2
# leaves the last input column ownerless in the same way ((10 - 3) % 2 = 1).
GEOMS = {}
for _rs, (_r, _s) in (("3x2", (3, 2)), ("1x3", (1, 3))):
    for _st in (1, 2):
        for _pd in (0, 1):
            GEOMS[f"{_rs}_s{_st}_p{_pd}"] = Geom(3, 7, 10, 5, 12, _r, _s, _st, _pd)
GEOMS["rows"] = Geom(3, 8, 10, 5, 12, 3, 2, 2, 0)
MNIST2 = Geom(8, 12, 12, 16, 24, 5, 5, 1, 0)
CONV40 = Geom(9, 12, 10, 40, 40, 3, 3, 1, 1)
PAIR_S1 = Geom(3, 7, 10, 5, 12, 3, 2, 1, 1)
PAIR_S2 = Geom(3, 7, 10, 5, 12, 3, 2, 2, 1)
PW_S1 = Geom(3, 7, 10, 24, 40, 1, 1, 1, 0)
PW_S2 = Geom(3, 7, 10, 24, 40, 1, 1, 2, 0)


def _pair_conv_expect(G):
    return (E("pair.0", G.n * G.h * G.w, G.cp, G.r * G.s * G.cop), E("pair.1", G.co, G.r * G.s * G.cp,
                                                                     G.n * G.ho * G.wo))


def _table():
    t = []

    def add(name, build, expect, forced=False):
        t.append(Case(name, build, tuple(expect), forced))

    S = "single"
    add("fwd_64_fast", _fwd("fwd_64_fast", 130, 40, 70, bias=True), [E(S, 130, 70, 40)])
    add("fwd_64_generic_k", _fwd("fwd_64_generic_k", 130, 50, 70, bias=True, relu=True), [E(S, 130, 70, 50)])
    add("fwd_64_generic_pitch", _fwd("fwd_64_generic_pitch", 130, 48, 70, bias=True, out_pitch=75, x_pitch=52),
        [E(S, 130, 70, 48)])
    add("fwd_out_f32_pitch", _fwd("fwd_out_f32_pitch", 130, 40, 70, bias=True, relu=True, f32=True, out_pitch=72),
        [E(S, 130, 70, 40)])
    add("dgrad_out_pitch", _dgrad("dgrad_out_pitch", 130, 72, 40, mask=True, out_pitch=48, dy_pitch=80, aux_pitch=56),
        [E(S, 130, 40, 72)])
    add("fwd_128x32", _fwd("fwd_128x32", 200, 72, 10, bias=True), [E(S, 200, 10, 72, "128x32")])
    add("fwd_128x32_generic", _fwd("fwd_128x32_generic", 200, 50, 10, f32=True), [E(S, 200, 10, 50, "128x32")])
    add("fwd_32x128", _fwd("fwd_32x128", 8, 64, 130, relu=True), [E(S, 8, 130, 64, "32x128")])
    for tag, (M, K, N) in (("a", (72, 2056, 40)), ("b", (200, 4096, 96))):
        add(f"skinny_fwd_{tag}", _fwd(f"skinny_fwd_{tag}", M, K, N, bias=True, relu=True),
            [E("skinny", M, N, K, None)])
        add(f"skinny_dgrad_{tag}", _dgrad(f"skinny_dgrad_{tag}", M, K, N, mask=True), [E("skinny", M, N, K, None)])
    add("lowk_64", _fwd("lowk_64", 4100, 40, 200, bias=True), [E("lowk", 4100, 200, 40, "x64")])
    add("lowk_128", _fwd("lowk_128", 4096, 32, 128, relu=True), [E("lowk", 4096, 128, 32, "x128")], forced=True)
    for rows, lanes in ((512, 1), (2048, 4), (16384, 16)):
        add(f"wgrad_lanes{lanes}", _wgrad(f"wgrad_lanes{lanes}", rows, 70, 132),
            [E(S, 70, 132, rows, "64x64", lanes)])
    add("wgrad_scalar_reduce", _wgrad("wgrad_scalar_reduce", 2048, 70, 130), [E(S, 70, 130, 2048, "64x64", 0)])
    add("wgrad_accum", _wgrad("wgrad_accum", 2048, 70, 132, out=True, accumulate=True),
        [E(S, 70, 132, 2048, "64x64", 4)])
    add("wgrad_out_unsplit", _wgrad("wgrad_out_unsplit", 200, 70, 132, out=True), [E(S, 70, 132, 200)])
    for acc in (False, True):
        sfx = "_acc" if acc else ""
        add("wgrad_bias_split" + sfx, _wgrad_bias("wgrad_bias_split" + sfx, 2048, 70, 131, 72, 136, acc),
            [E(S, 70, 132, 2048, "64x64", 4)])
        add("wgrad_bias_unsplit" + sfx, _wgrad_bias("wgrad_bias_unsplit" + sfx, 200, 70, 50, 72, 56, acc),
            [E(S, 70, 51, 200)])
    add("pair_dense", _pair_linear("pair_dense", 264, 72, 136), [E("pair.0", 264, 136, 72), E("pair.1", 72, 136, 264)])
    add("pair_skinny", _pair_linear("pair_skinny", 72, 264, 40, accumulate=True),
        [E("pair-skinny.0", 72, 40, 264, None), E("pair-skinny.1", 264, 40, 72)])
    add("pair_both_split", _pair_linear("pair_both_split", 1032, 1024, 72),
        [E("pair.0", 1032, 72, 1024, "64x64", 4), E("pair.1", 1024, 72, 1032, "64x64", 4)])
    add("pair_conv_s1", _pair_conv("pair_conv_s1", PAIR_S1), _pair_conv_expect(PAIR_S1))
    add("pair_conv_s2", _pair_conv("pair_conv_s2", PAIR_S2, accumulate=True, aux=None), _pair_conv_expect(PAIR_S2))
    add("pair_conv1x1_s1", _pair_conv("pair_conv1x1_s1", PW_S1, fwd_layout=True), _pair_conv_expect(PW_S1))
    add("pair_conv1x1_s2", _pair_conv("pair_conv1x1_s2", PW_S2, fwd_layout=True, accumulate=True),
        _pair_conv_expect(PW_S2))
    add("pair_conv_deferred", _pair_conv("pair_conv_deferred", CONV40, defer=True, accumulate=True, aux=None),
        [E("pair.0", 1080, 40, 360), E("pair.1", 40, 360, 1080, "64x64", 4)])
    add("conv40_fwd", _conv_fwd("conv40_fwd", CONV40), [E(S, 1080, 40, 360)])
    for gname, G in list(GEOMS.items()) + [("mnist2", MNIST2)]:
        pre = "mnist2" if gname == "mnist2" else f"conv_{gname}"
        add(f"{pre}_fwd", _conv_fwd(f"{pre}_fwd", G), _conv_expect(G, "fwd"))
        ed, ew = _conv_expect(G, "dgrad"), _conv_expect(G, "wgrad")
        if gname == "mnist2":  # K = 600 and 512: the only unpaired conv gradients here long enough to split (in 2)
            ed, ew = (ed[0]._replace(lanes=1),), (ew[0]._replace(lanes=1),)
        add(f"{pre}_dgrad", _conv_dgrad(f"{pre}_dgrad", G), ed)
        add(f"{pre}_wgrad", _conv_wgrad(f"{pre}_wgrad", G), ew)
    for gname in ("3x2_s1_p0", "1x3_s1_p0"):
        add(f"layout_{gname}", _layout(f"layout_{gname}", GEOMS[gname]), [])
    add("forced_fwd_skinny", _fwd("forced_fwd_skinny", 200, 520, 136, bias=True), [E("skinny", 200, 136, 520, None)],
        forced=True)
    add("forced_fwd", _fwd("forced_fwd", 200, 200, 136, bias=True, relu=True), [E(S, 200, 136, 200)], forced=True)
    add("forced_wgrad", _wgrad("forced_wgrad", 2048, 136, 264), [E(S, 136, 264, 2048, "64x64", 4)], forced=True)
    return t


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
FORCED_NAMES = [c.name for c in CASES if c.forced]


@functools.lru_cache(maxsize=2)
def prepare(name):
    return BY_NAME[name].build()


# ---------------------------------------------------------------------------------------------------------------
# running and reporting
# ---------------------------------------------------------------------------------------------------------------
class Mismatch(NamedTuple):
    output: str
    count: int
    total: int
    first: tuple    # of ((m, n), (tile_m, tile_n), got, want)

    def __str__(self):
        where = "; ".join(f"(m={m}, n={n}) tile ({tm}, {tn}): got {g!r} want {w!r}" for (m, n), (tm, tn), g, w
                          in self.first)
        return f"{self.output}: {self.count} of {self.total} elements differ -- {where}"


def compare(name, got, want, dtype):
    """None if ``got`` is bitwise ``want`` (float64 reference cast to the output dtype: exact, it holds small
    integers and the sentinel), else the Mismatch: outputs are viewed as [rows, last dim]."""
    want = want.to(dtype)
    got = got.detach().cpu()
    if got.dtype != dtype or got.shape != want.shape:
        return Mismatch(f"{name} (dtype / shape {got.dtype} {tuple(got.shape)}, want {dtype} {tuple(want.shape)})",
                        want.numel(), want.numel(), ())
    if torch.equal(got, want):
        return None
    g2 = got.reshape(-1, got.shape[-1]) if got.dim() > 1 else got.reshape(1, -1)
    w2 = want.reshape(g2.shape)
    bad = (g2 != w2) | (g2.isnan() != w2.isnan())
    idx = bad.nonzero()
    first = tuple(((int(m), int(n)), (int(m) // 64, int(n) // 64), g2[m, n].item(), w2[m, n].item())
                  for m, n in idx[:6].tolist())
    return Mismatch(name, int(bad.sum()), bad.numel(), first)


def run_case(name, dev="cuda"):
    """Run one case on ``dev``; the list of its Mismatches (empty: every output buffer is bitwise the reference)."""
    p = prepare(name)
    got = p.launch(torch.device(dev))
    torch.cuda.synchronize()
    assert set(got) == set(p.refs), (sorted(got), sorted(p.refs))
    out = []
    for k in sorted(p.refs):
        m = compare(k, got[k], p.refs[k], p.dtypes[k])
        if m is not None:
            out.append(m)
    return out


def main(argv):
    """Child-process entry: run the named cases (none named: the whole table; ``--forced``: the forced-tile
    set), a ``[case] NAME`` line on stderr before each so PDE_GEMM_LOG lines can be attributed; mismatches go to
    stdout, then ``GEMM_EXACT_OK`` (exit 0) if there were none, exit 1 otherwise."""
    from pytorch_distributed_examples_amd.ops import functional as OF

    names = [a for a in argv if not a.startswith("--")]
    if "--forced" in argv:
        names += FORCED_NAMES
    names = names or NAMES
    failed = 0
    for n in names:
        sys.stderr.write(f"[case] {n}\n")
        sys.stderr.flush()
        bad = run_case(n)
        OF.check_device_errors(n)
        for m in bad:
            print(f"MISMATCH {n} {m}")
        failed += bool(bad)
    sys.stderr.write("[case] -\n")
    sys.stderr.flush()
    if failed:
        print(f"{failed} of {len(names)} cases differ")
        return 1
    print(f"{TOKEN} {len(names)}")
    return 0


# ---------------------------------------------------------------------------------------------------------------
# PDE_GEMM_LOG
# ---------------------------------------------------------------------------------------------------------------
_LOG = re.compile(r"\[gemm\] (\S+) M=(\d+) N=(\d+) K=(\d+) akind=(\d) bkind=(\d) tile=(\d+x\d+) tiles=(\d+) split=(\d+)")


def parse_log(stderr):
    """{case name: [dict(what, M, N, K, tile, split)]} from a child's stderr."""
    out, cur = {}, None
    for line in stderr.splitlines():
        if line.startswith("[case] "):
            cur = out.setdefault(line[7:].strip(), [])
            continue
        m = _LOG.search(line)
        if m and cur is not None:
            cur.append(dict(what=m.group(1), M=int(m.group(2)), N=int(m.group(3)), K=int(m.group(4)),
                            tile=m.group(7), split=int(m.group(9))))
    return out


def slab_lanes(split):
    """Slab lanes of the vector reduce for a split count (gemm.hip reduce_lanes)."""
    return 1 if split <= 2 else (4 if split <= 16 else 16)


def path_errors(case, entries):
    """What of ``case.expect`` the logged launches do not show."""
    errs = []
    for e in case.expect:
        hit = [x for x in entries if x["what"].startswith(e.what) and (x["M"], x["N"], x["K"]) == (e.M, e.N, e.K)]
        if not hit:
            errs.append(f"{case.name}: no '{e.what}' launch of {e.M}x{e.N}x{e.K} (logged: {entries})")
            continue
        for x in hit:
            if e.tile is not None and not x["tile"].endswith(e.tile):
                errs.append(f"{case.name}: {e.what} {e.M}x{e.N}x{e.K} on tile {x['tile']}, table says {e.tile}")
            if e.lanes is None and x["split"] != 1:
                errs.append(f"{case.name}: {e.what} {e.M}x{e.N}x{e.K} split {x['split']}, table says unsplit")
            if e.lanes is not None and x["split"] <= 1:
                errs.append(f"{case.name}: {e.what} {e.M}x{e.N}x{e.K} unsplit, table says split-K")
            if e.lanes and x["split"] > 1 and slab_lanes(x["split"]) != e.lanes:
                errs.append(f"{case.name}: {e.what} {e.M}x{e.N}x{e.K} split {x['split']} = "
                            f"{slab_lanes(x['split'])} slab lanes, table says {e.lanes}")
    return errs


if __name__ == "__main__":
    import os

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.exit(main(sys.argv[1:]))
