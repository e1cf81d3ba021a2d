"""Autograd front ends of the training-side HIP kernels (``csrc/conv_wgrad*.hip``, ``csrc/pack_weights.hip``, ``csrc/elementwise_bwd.hip``, ``csrc/bn_train.hip`` + the forward conv).

Training does not go through launch plans: modules build an ordinary autograd graph out of
the two Functions below, on ``torch.channels_last`` tensors (logical NCHW, physical NHWC --
exactly the layout the kernels use, so nothing is converted).  What they replace in the
reference: the autograd of mmcv ``ConvModule`` in train mode (cuDNN conv fwd / backward-data /
backward-filter, ATen batch_norm with batch statistics, ``MishCudaFunction``,
mmdet/models/backbones/darknetcsp.py:15-64, mmdet/ops/mish_cuda/mish.py:18-36).

  ConvFunction    y = conv(x, w)                       fwd: fused conv kernel with an identity
                                                       epilogue; bwd: dX = the same kernel on dY
                                                       (zero-dilated for stride 2) with flipped,
                                                       transposed weights, dW = yv4_conv_wgrad
  BNActFunction   y = act(BN_batchstats(x)) (+ res)    saves only x and the batch statistics; the
                                                       activation is recomputed in backward (the
                                                       reference keeps conv-out, BN-out and the Mish
                                                       input: SURVEY Q17)
"""
import contextlib
import ctypes as C
import os

import torch

from . import _lib
from ._lib import DTYPE_CODE as _DCODE, ConvDesc, check
from .direct_grad import (_DIRECT_WGRAD, _ParamRef, _direct_grad_listeners, _direct_grad_target, _flat_f32, _side,
                          _wgrad_workspace)
from .ops import _need_cuda, stream_ptr
from .packed_weights import _chunk, _rowpair_weights, packed_weight
# the public names of the two modules above stay reachable as ``train_ops.<name>`` (package modules, tests and tools say so)
from .direct_grad import add_direct_grad_listener, join_side_streams, remove_direct_grad_listener, wgrad_side_stream  # noqa: F401
from .packed_weights import _PACK_CACHES, clear_pack_cache, invalidate_packed_weights  # noqa: F401

# ---- A/B switches, read once at import (YV4_PACK_CACHE: packed_weights; YV4_DIRECT_WGRAD, YV4_WGRAD_STREAM: direct_grad) ----
_SLICE_GRADS = os.environ.get('YV4_SLICE_GRADS', '1') != '0'      # off: a channel-slice gradient is copied to dense NHWC
_GRAD_SINK_ON = os.environ.get('YV4_GRAD_SINK', '1') != '0'       # off: autograd adds a shortcut's gradient (see GradSink)
_ROWPAIR_ON = os.environ.get('YV4_DGRAD_ROWPAIR', '1') != '0'     # off: every 3x3 / stride 2 data gradient takes the parity form
# YV4_WGRAD_ATOMIC=1: the round-1 weight gradient (split-M partials added with float atomics: not run-to-run
# deterministic); default (off): partials in a workspace + ordered reduction (yv4_conv_wgrad_det)
_WGRAD_ATOMIC = os.environ.get('YV4_WGRAD_ATOMIC', '0') == '1'


def to_nhwc(x):
    """Logical NCHW tensor whose storage is dense NHWC."""
    return x.contiguous(memory_format=torch.channels_last)


def image_to_nhwc16(x, dtype, channels):
    """fp32 NCHW image batch -> dense 16-bit NHWC with ``channels`` per pixel (the real ones, then zeros) in ONE pass
    (``yv4_nchw_to_nhwc_h16``); returned as the logical (N, channels, H, W) channels_last tensor the conv ops take.
    ATen needs a zero fill, a padded copy, a cast and a layout copy for the same result (0.66 ms at 64 x 3 x 608 x 608)."""
    N, C_, H, W = x.shape
    out = torch.empty((N, channels, H, W), device=x.device, dtype=dtype, memory_format=torch.channels_last)
    check(_lib.lib().yv4_nchw_to_nhwc_h16(x.data_ptr(), out.data_ptr(), N, C_, H, W, channels, 0, channels - C_,
                                          _DCODE[dtype], stream_ptr()), 'yv4_nchw_to_nhwc_h16')
    return out


def nhwc_or_slice(t, dtype):
    """(tensor, pixel stride in elements): ``t`` itself when it already is ``dtype`` and either dense NHWC or a
    channel slice of a dense NHWC tensor (what ``torch.cat``'s backward hands to each branch: every kernel takes
    a pixel stride, so the slice needs no copy); else a dense NHWC copy."""
    if _SLICE_GRADS and t.dtype == dtype and t.dim() == 4:
        N, C_, H, W = t.shape
        sn, sc, sh, sw = t.stride()
        if (sc == 1 or C_ == 1) and sw >= C_ and sh == W * sw and sn == H * W * sw and sw % _chunk(dtype) == 0 \
                and t.data_ptr() % 16 == 0:
            return t, sw
    t = to_nhwc(t.to(dtype))
    return t, t.shape[1]


def _kernel_map(x):
    """``x`` as the elementwise kernels take it: on the GPU, dense NHWC, fp32 or a 16-bit type (anything else -> fp32)."""
    _need_cuda(x, 'x')
    return to_nhwc(x if x.dtype in _DCODE else x.float())


def _is_nhwc(t):
    return t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)


_IDENTITY = {}


def _identity_affine(device, C_):
    """(ones, zeros) of length C_, cached per device: the identity epilogue of a training conv."""
    key = (str(device), C_)
    if key not in _IDENTITY:
        _IDENTITY[key] = (torch.ones(C_, device=device), torch.zeros(C_, device=device))
    return _IDENTITY[key]


def _ptr(t, offset=0):
    """Address of ``t`` (plus ``offset`` bytes) for an optional pointer argument: None stays None."""
    return t.data_ptr() + offset if t is not None else None


def _kept_clean(buf):
    """1 for a statistics buffer whose owner keeps it zeroed between uses (``conv_stats_buffer(persistent=True)``)."""
    return 1 if getattr(buf, '_yv4_kept_clean', False) else 0


def _desc(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, x_cs, y_cs, y_co=0):
    """A ``ConvDesc`` from the geometry and the pixel strides of input and output (``y_co``: the output's first channel)."""
    d = ConvDesc()
    d.N, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout = N, H, W, Cin, Ho, Wo, Cout
    d.KH, d.KW, d.stride, d.pad = KH, KW, stride, pad
    d.x_cstride, d.y_cstride, d.y_coff = x_cs, y_cs, y_co
    return d


# One helper per kernel family with an fp32 and a 16-bit entry point: the fp32 entry for fp32 operands, else ``_h16``
# with the element code.  (The ``yv4_bn_*_h16`` entries take fp32 maps themselves and are called directly.)
def _conv_fwd(d, dtype, x, w, ones, zeros, res, out):
    if dtype == torch.float32:
        check(_lib.lib().yv4_conv_bn_act_fwd(C.byref(d), x, w, ones, zeros, None, None, res, out, stream_ptr()),
              'yv4_conv_bn_act_fwd')
    else:
        code = _DCODE[dtype]
        check(_lib.lib().yv4_conv_bn_act_fwd_h16(C.byref(d), code, code, x, w, ones, zeros, None, None, res, out, stream_ptr()),
              'yv4_conv_bn_act_fwd_h16')


def _conv_scatter(d, dtype, dy, w, dx, Hd, Wd, sh, sw, a, b):
    """Identity-epilogue correlation of ``dy`` whose output pixel (i, j) goes to dx[:, :, sh * i + a, sw * j + b] of a
    (Hd, Wd) map."""
    ones, zeros = _identity_affine(dy.device, d.Cout)
    if dtype == torch.float32:
        check(_lib.lib().yv4_conv_scatter_fwd(C.byref(d), dy.data_ptr(), w.data_ptr(), ones.data_ptr(), zeros.data_ptr(),
                                     dx.data_ptr(), Hd, Wd, sh, sw, a, b, stream_ptr()), 'yv4_conv_scatter_fwd')
    else:
        check(_lib.lib().yv4_conv_scatter_fwd_h16(C.byref(d), _DCODE[dtype], dy.data_ptr(), w.data_ptr(), ones.data_ptr(),
                                         zeros.data_ptr(), dx.data_ptr(), Hd, Wd, sh, sw, a, b, stream_ptr()),
              'yv4_conv_scatter_fwd_h16')


def _wgrad_atomic(d, dtype, x, dy, dw):
    if dtype == torch.float32:
        check(_lib.lib().yv4_conv_wgrad(C.byref(d), x.data_ptr(), dy.data_ptr(), dw.data_ptr(), stream_ptr()), 'yv4_conv_wgrad')
    else:
        check(_lib.lib().yv4_conv_wgrad_h16(C.byref(d), _DCODE[dtype], x.data_ptr(), dy.data_ptr(), dw.data_ptr(), stream_ptr()),
              'yv4_conv_wgrad_h16')


def _spp_pool_fwd(out, N, H, W, Cc):
    if out.dtype == torch.float32:
        check(_lib.lib().yv4_spp_pool_fwd(out.data_ptr(), N, H, W, Cc, 4 * Cc, 0, stream_ptr()), 'yv4_spp_pool_fwd')
    else:
        check(_lib.lib().yv4_spp_pool_fwd_h16(out.data_ptr(), N, H, W, Cc, 4 * Cc, 0, _DCODE[out.dtype], stream_ptr()),
              'yv4_spp_pool_fwd_h16')


def _conv_launch(x, w_packed, Cin_p, Cout, KH, KW, stride, pad, out, stats=None, x_cs=None, residual=None, res_cs=None,
                 y_cs=None, y_co=0):
    """Identity-epilogue conv of a channels_last tensor; fp32, or fp16 / bf16 operands (fp32 accumulate).
    ``stats``: a float64 buffer of ``STATS_REPLICAS * 2 * Cout`` entries that receives the BatchNorm sums of the
    output (``yv4_conv_fwd_stats``: accumulated in the conv kernel's epilogue)."""
    N, _, H, W = x.shape
    d = _desc(N, H, W, Cin_p, out.shape[2], out.shape[3], Cout, KH, KW, stride, pad,
              x_cs if x_cs is not None else Cin_p, y_cs if y_cs is not None else Cout, y_co)
    if residual is not None:        # out = conv + residual (a gradient that joins this one: see GradSink)
        assert stats is None and residual.dtype == x.dtype
        d.r_cstride, d.r_coff = (res_cs if res_cs is not None else Cout), 0
    ones, zeros = _identity_affine(x.device, Cout)
    if stats is not None:
        assert stats.dtype == torch.float64 and stats.numel() >= _lib.STATS_REPLICAS * 2 * Cout
        check(_lib.lib().yv4_conv_fwd_stats(C.byref(d), _DCODE[x.dtype], x.data_ptr(), w_packed.data_ptr(),
                                            ones.data_ptr(), zeros.data_ptr(), out.data_ptr(), stats.data_ptr(),
                                            _kept_clean(stats), stream_ptr()), 'yv4_conv_fwd_stats')
        return d
    _conv_fwd(d, x.dtype, x.data_ptr(), w_packed.data_ptr(), ones.data_ptr(), zeros.data_ptr(), _ptr(residual),
              out.data_ptr())
    return d


class GradSink:
    """Joins two gradient paths of one tensor without autograd's add kernel.  For  out = x + f(x)  (a Bottleneck
    with shortcut, darknetcsp.py:60-64) the gradient of x is  d_out + f'(d_out): the BN + act + residual Function at
    the end of f parks d_out here instead of returning it for the residual, and the FIRST convolution of f -- whose
    backward runs last -- adds it in the epilogue of its data-gradient launch (``residual=`` of the conv kernels).
    Saves one read-read-write pass over the activation per bottleneck and step.  YV4_GRAD_SINK=0 switches it off."""
    __slots__ = ('value', 'cs')

    def __init__(self):
        self.value = None
        self.cs = None


def grad_sink_for(x):
    """A sink for the residual path of ``x``, or None when the fusion does not apply (no gradient wanted)."""
    if _GRAD_SINK_ON and torch.is_grad_enabled() and x.requires_grad:
        return GradSink()
    return None


def _dgrad_dilated(dy, weight, xshape, stride, pad, dtype, dy_cs=None, residual=None, res_cs=None, owner=None):
    """dX = correlate(dY zero-dilated by `stride`, W flipped in (kh,kw) and transposed in (co,ci)), pad k-1-p."""
    N, Cin, H, W = xshape
    Cout, _, KH, KW = weight.shape
    Ho, Wo = dy.shape[2], dy.shape[3]
    h16 = dtype != torch.float32
    L = _lib.lib()
    wtp, _ = packed_weight(weight, dtype, transpose_flip=True, owner=owner)     # rows = Cin, taps mirrored, cast: one launch
    src_cs = None
    if stride == 1:
        src, src_cs = dy, dy_cs
    elif stride == 2:
        if dy_cs is not None and dy_cs != Cout:
            dy = to_nhwc(dy)
        src = torch.empty((N, Cout, 2 * Ho, 2 * Wo), device=dy.device, dtype=dtype, memory_format=torch.channels_last)
        k = 2 if h16 else 1     # a 16-bit map with C % 8 == 0 is an fp32 map with C/2 channels
        check(L.yv4_dilate2_fwd(dy.data_ptr(), src.data_ptr(), N, Ho, Wo, Cout // k, Cout // k, 0, stream_ptr()),
              'yv4_dilate2_fwd')
    else:
        raise NotImplementedError('conv backward: stride must be 1 or 2')
    p2 = KH - 1 - pad
    Hs, Ws = src.shape[2], src.shape[3]
    Hx = Hs + 2 * p2 - KH + 1
    Wx = Ws + 2 * p2 - KW + 1
    dxf = torch.empty((N, Cin, Hx, Wx), device=dy.device, dtype=dtype, memory_format=torch.channels_last)
    if residual is not None:
        assert (Hx, Wx) == (H, W)
    _conv_launch(src, wtp, Cout, Cin, KH, KW, 1, p2, dxf, x_cs=src_cs, residual=residual, res_cs=res_cs)
    if (Hx, Wx) != (H, W):
        # stride 2 with odd input size: the dilated grid is one row/column larger or smaller
        dx = torch.empty((N, Cin, H, W), device=dy.device, dtype=dtype, memory_format=torch.channels_last).zero_()
        hh, ww = min(H, Hx), min(W, Wx)
        dx[:, :, :hh, :ww] = dxf[:, :, :hh, :ww]
        return dx
    return dxf


def _dgrad_s2_parity(dy, weight, xshape, dtype, dy_cs=None, owner=None):
    """Data gradient of a 3x3 / stride 2 / pad 1 convolution as four parity classes: with
    hi = 2*ho - 1 + kh, the input rows hi = 2i + a receive only the taps kh with (a + 1 - kh) even
    (a = 0: kh = 1 from dY row i;  a = 1: kh = 2 from row i and kh = 0 from row i + 1), likewise in x.
    Each class is a stride-1 correlation of dY with 1, 2, 2 or 4 taps whose result is scattered to
    dX[:, :, a::2, b::2] (``yv4_conv_scatter_fwd``): the forward FLOPs exactly, no dilated copy."""
    N, Cin, H, W = xshape
    Cout = weight.shape[0]
    Ho, Wo = dy.shape[2], dy.shape[3]
    dx = torch.empty((N, Cin, H, W), device=dy.device, dtype=dtype, memory_format=torch.channels_last)
    taps = {0: (1, 1, 1), 1: (2, -2, 2)}          # (first source tap, step, count): [1] and [2, 0]
    wd = weight.detach()
    for a in (0, 1):
        Ha = (H - a + 1) // 2
        for b in (0, 1):
            Wb = (W - b + 1) // 2
            if Ha == 0 or Wb == 0:
                continue
            wp, _ = packed_weight(wd, dtype, taps=(taps[a], taps[b]), owner=owner if owner is not None else weight)
            d = _desc(N, Ho, Wo, Cout, Ha, Wb, Cin, taps[a][2], taps[b][2], 1, 0, dy_cs if dy_cs is not None else Cout, Cin)
            _conv_scatter(d, dtype, dy, wp, dx, H, W, 2, 2, a, b)
    return dx


def _dgrad_s2_rowpair(dy, weight, xshape, dtype, dy_cs=None, owner=None):
    """The same data gradient for FEW input channels (2 * Cin <= 64), even H and W: the two column parities of an input
    row pair are ONE output pixel of 2 * Cin channels -- dX viewed as (N, H, W / 2, 2 Cin) -- so each row parity a is a
    single stride-1 correlation of dY with a (1 + a) x 2 kernel into 2 Cin channels, scattered to the rows 2 i + a
    (``yv4_conv_scatter_fwd``, sh = 2, sw = 1).  Two launches instead of four, each with a full 64-column tile and whole
    128-byte lines per output pixel; a third more FLOPs (the zero blocks) on a layer that is bound by its bytes:
    conv1 of CSPDarknet (32 -> 64 at 608 -> 304, batch 64): 1.61 -> 0.8 ms."""
    N, Cin, H, W = xshape
    Cout = weight.shape[0]
    Ho, Wo = dy.shape[2], dy.shape[3]
    dx = torch.empty((N, Cin, H, W), device=dy.device, dtype=dtype, memory_format=torch.channels_last)
    w2 = _rowpair_weights(weight, dtype, owner)
    for a in (0, 1):
        d = _desc(N, Ho, Wo, Cout, H // 2, W // 2, 2 * Cin, 1 + a, 2, 1, 0, dy_cs if dy_cs is not None else Cout, 2 * Cin)
        _conv_scatter(d, dtype, dy, w2[a], dx, H, W // 2, 2, 1, a, 0)
    return dx


def _cat_output(ctx, cat_buf, cat_total, cat_off, N, C_, H, W, dtype, device):
    """(y, pixel stride, channel offset): where a Function writes its (N, C_, H, W) result.  ``cat_total`` == 0: a dense
    tensor of its own.  Else channels [cat_off, cat_off + C_) of a (N, cat_total, H, W) concat buffer (``CatSlot``):
    ``cat_buf`` if given (written in place, marked dirty and returned), else a fresh one.  ``ctx.cat`` remembers the
    slice for ``_cat_grad``."""
    ctx.cat = None
    if not cat_total:
        return torch.empty((N, C_, H, W), device=device, dtype=dtype, memory_format=torch.channels_last), C_, 0
    assert cat_off % _chunk(dtype) == 0 and cat_off + C_ <= cat_total
    if cat_buf is None:
        y = torch.empty((N, cat_total, H, W), device=device, dtype=dtype, memory_format=torch.channels_last)
    else:
        assert tuple(cat_buf.shape) == (N, cat_total, H, W) and cat_buf.dtype == dtype and _is_nhwc(cat_buf)
        y = cat_buf
        ctx.mark_dirty(cat_buf)
    ctx.cat = (cat_off, cat_buf is not None)
    return y, cat_total, cat_off


def _cat_grad(ctx, dy, C_):
    """(this Function's slice of ``dy``, the gradient to return for ``cat_buf``): with a concat output, dy is the
    gradient of the whole buffer -- this producer's channel slice of it, and the buffer's gradient handed on to the
    producer of the other channels (the one whose buffer was passed in)."""
    if ctx.cat is None:
        return dy, None
    off, passed = ctx.cat
    return dy[:, off:off + C_], (dy if passed else None)


class ConvFunction(torch.autograd.Function):
    """``dtype``: torch.float32, or torch.float16 / torch.bfloat16 -- then x, y and their gradients are
    that type (fp32 accumulation in every kernel) while ``weight`` and its gradient stay fp32 (the
    master copy the optimizer steps; autocast semantics of the reference's Fp16 hook)."""

    @staticmethod
    def forward(ctx, x, weight, stride, pad, dtype, stats=None, direct=None, sink=None, cat_buf=None, cat_total=0,
                cat_off=0, park=None):
        """``direct``: a ``_ParamRef`` to the parameter whose ``.grad`` receives dW in place (then ``weight`` is the
        detached parameter: autograd does not track it through this Function, see ``conv2d``).
        ``cat_total`` > 0: the output is channels [cat_off, cat_off + Cout) of a (N, cat_total, Ho, Wo) concat buffer --
        ``cat_buf`` if given (written in place and returned), else a fresh one whose other channels a later producer
        fills (see ``CatSlot``).  ``park``: a ``GradSink`` that receives this conv's data gradient instead of autograd
        (x also feeds a conv whose backward runs LATER and adds the parked gradient in its own launch)."""
        _need_cuda(x, 'x')
        if _side.join_pending or _side.dirty:
            # a forward pass while a join is still "pending": the backward that queued it never finished (its callback was
            # dropped with the exception) -- join now, so the one-shot flag cannot stay stuck for the rest of the process
            # (known, kept as it is: a forward INSIDE a running backward -- checkpoint recomputation, a double backward --
            # also lands here, joins early and clears the flag, so that backward queues a second callback)
            _side.join()
        ctx.direct = direct
        ctx.park = park
        ctx.sink = sink if stride == 1 else None     # (the stride-2 parity form has no residual input)
        Cout, Cin, KH, KW = weight.shape
        al = _chunk(dtype)
        xc = x.shape[1]
        # ``x`` may carry MORE channels than the weight (zeros: the image stored with a whole number of 16-byte chunks
        # per pixel, ``image_to_nhwc16``): the forward operand is packed to x's width, the weight gradient is taken
        # over the weight's own (padded) channels with x's pixel stride; such an x has no gradient
        assert xc >= Cin and Cout % al == 0 and xc % al == 0 and (xc == Cin or not ctx.needs_input_grad[0]), \
            f'training conv needs channel counts that are multiples of {al} (got {xc}/{Cin}->{Cout})'
        ctx.x_dtype = x.dtype
        x = to_nhwc(x.to(dtype))
        N, _, H, W = x.shape
        Ho = (H + 2 * pad - KH) // stride + 1
        Wo = (W + 2 * pad - KW) // stride + 1
        wp, cp = packed_weight(weight, dtype, owner=direct.p if direct is not None else None,
                               pad_to=xc if xc != Cin else None)
        assert cp == xc
        y, y_cs, y_co = _cat_output(ctx, cat_buf, cat_total, cat_off, N, Cout, Ho, Wo, dtype, x.device)
        _conv_launch(x, wp, cp, Cout, KH, KW, stride, pad, y, stats, y_cs=y_cs, y_co=y_co)
        ctx.save_for_backward(x, weight)
        ctx.geom = (stride, pad, dtype, (Cin + al - 1) // al * al)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        stride, pad, dtype, cp = ctx.geom
        Cout, Cin, KH, KW = weight.shape
        N, _, H, W = x.shape
        dy, dcat = _cat_grad(ctx, dy, Cout)
        dy, dy_cs = nhwc_or_slice(dy, dtype)
        Ho, Wo = dy.shape[2], dy.shape[3]
        L = _lib.lib()
        h16 = dtype != torch.float32
        code = _DCODE[dtype]
        dx = dw = None
        own = ctx.direct.p if ctx.direct is not None else None       # the parameter whose detached alias ``weight`` is
        if ctx.needs_input_grad[1] or own is not None:
            target = _direct_grad_target(own, cp) if own is not None else None
            dwp = target if target is not None else torch.zeros((Cout, KH * KW * cp), device=x.device,
                                                                dtype=torch.float32)
            d = _desc(N, H, W, cp, Ho, Wo, Cout, KH, KW, stride, pad, x.shape[1], dy_cs)
            if _WGRAD_ATOMIC:
                _wgrad_atomic(d, dtype, x, dy, dwp)
            else:
                # deterministic form: partial sums of the reduction chunks in a workspace, added in chunk order
                need = int(L.yv4_conv_wgrad_workspace(C.byref(d), code))
                side = _side.for_launch(x.device) if target is not None else None
                ws = _wgrad_workspace(need, x.device, 'side' if side is not None else None)
                if side is not None:
                    side.wait_stream(torch.cuda.current_stream(x.device))
                with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
                    check(L.yv4_conv_wgrad_det(C.byref(d), code, x.data_ptr(), dy.data_ptr(), dwp.data_ptr(), _ptr(ws), need,
                                               stream_ptr()), 'yv4_conv_wgrad_det')
                if side is not None:     # (ws too: a grown one frees its predecessor while the side stream may still read it)
                    _side.issued(side, x, dy, ws)
            if target is None:
                dw = dwp.view(Cout, KH, KW, cp)[..., :Cin].permute(0, 3, 1, 2)
                if cp != Cin:
                    dw = dw.contiguous()
            if own is not None:              # autograd does not track the weight here: hand the gradient over
                if target is None:           # (.grad went away between forward and backward)
                    own.grad = dw.clone() if own.grad is None else own.grad.add_(dw)
                dw = None
                for cb in _direct_grad_listeners:
                    cb(own)
        if ctx.needs_input_grad[0]:
            joined = jcs = None
            if ctx.sink is not None and ctx.sink.value is not None:
                joined, jcs = ctx.sink.value, ctx.sink.cs
                ctx.sink.value = None
                if joined.dtype != dtype or tuple(joined.shape) != (N, Cin, H, W):
                    joined = to_nhwc(joined.to(dtype))
                    jcs = None
            if stride == 2 and (KH, KW, pad) == (3, 3, 1) and Cout % (8 if h16 else 32) == 0:
                if _ROWPAIR_ON and 2 * Cin <= 64 and H % 2 == 0 and W % 2 == 0 and Cin % (4 if h16 else 2) == 0:
                    dx = _dgrad_s2_rowpair(dy, weight, (N, Cin, H, W), dtype, dy_cs, owner=own)
                else:
                    dx = _dgrad_s2_parity(dy, weight, (N, Cin, H, W), dtype, dy_cs, owner=own)
            else:
                dx = _dgrad_dilated(dy, weight, (N, Cin, H, W), stride, pad, dtype, dy_cs, residual=joined, res_cs=jcs,
                                    owner=own)
                joined = None
            if joined is not None:
                dx = dx + joined
            dx = dx.to(ctx.x_dtype)
        elif ctx.sink is not None and ctx.sink.value is not None:
            dx, ctx.sink.value = ctx.sink.value, None       # nobody wants this conv's share: hand the parked one on
        if ctx.park is not None and dx is not None:
            ctx.park.value, ctx.park.cs = dx, None          # joins the other consumer's data gradient (GradSink)
            dx = None
        return dx, dw, None, None, None, None, None, None, dcat, None, None, None


def train_dtype(module, x):
    """Operand type of a training-mode conv: the module's ``compute_dtype`` (``wrap_fp16_model``) if
    it is a 16-bit type, else the type ``x`` already has (16-bit activations stay 16-bit), else fp32."""
    dt = getattr(module, 'compute_dtype', None)
    if dt in (torch.float16, torch.bfloat16):
        return dt
    return x.dtype if x.dtype in (torch.float16, torch.bfloat16) else torch.float32


class CatSlot:
    """Where a producer writes inside a channel-concat buffer instead of returning a tensor of its own that
    ``torch.cat`` would copy: ``CatSlot(total, offset)`` for the FIRST producer (it allocates the (N, total, H, W)
    buffer and returns it), ``CatSlot(total, offset, buf)`` for every further one (``buf`` = what the previous producer
    returned; it is written in place and returned again).  The gradient of the buffer reaches every producer's
    backward whole; each takes its own channel slice (a strided view, no copy)."""
    __slots__ = ('total', 'off', 'buf')

    def __init__(self, total, off, buf=None):
        self.total, self.off, self.buf = int(total), int(off), buf

    def args(self):
        return self.buf, self.total, self.off


def conv2d(x, weight, stride=1, pad=0, dtype=None, stats=None, sink=None, cat=None, park=None):
    """``dtype`` None: follow ``x`` (a 16-bit activation keeps the path 16-bit, anything else is fp32).
    ``stats``: see ``_conv_launch`` / ``conv_stats_buffer``; pass the same buffer to ``bn_act(..., sums=)``.
    ``cat``: a ``CatSlot`` -- the result is the concat buffer with this conv's channels written."""
    if dtype is None:
        dtype = x.dtype if x.dtype in (torch.float16, torch.bfloat16) else torch.float32
    cargs = cat.args() if cat is not None else (None, 0, 0)
    if (_DIRECT_WGRAD and weight.requires_grad and weight.is_leaf and x.requires_grad and torch.is_grad_enabled()
            and _direct_grad_target(weight, weight.shape[1]) is not None
            and weight.shape[1] % _chunk(dtype) == 0):
        # dW goes straight into weight.grad (see the note above ConvFunction): the Function sees the detached weight
        return ConvFunction.apply(x, weight.detach(), stride, pad, dtype, stats, _ParamRef(weight), sink, *cargs, park)
    return ConvFunction.apply(x, weight, stride, pad, dtype, stats, None, sink, *cargs, park)


def stats_numel(cout):
    return _lib.STATS_REPLICAS * 2 * cout


def conv_stats_buffer(cout, device, persistent=False):
    """Scratch for the BatchNorm sums a training conv leaves for the BN that follows it.  ``persistent``: a zeroed
    buffer its owner keeps across steps; it is marked so that the conv skips the memset and ``bn_act`` has the
    finalize kernel clear it again as it reads it (the owner must pair every ``conv2d(stats=)`` with
    ``bn_act(sums=)``)."""
    if not persistent:
        return torch.empty(_lib.STATS_REPLICAS * 2 * cout, dtype=torch.float64, device=device)
    buf = torch.zeros(_lib.STATS_REPLICAS * 2 * cout, dtype=torch.float64, device=device)
    buf._yv4_kept_clean = True
    return buf


class BNActFunction(torch.autograd.Function):
    """Train-mode BatchNorm2d + activation (+ residual add) as one forward and one backward."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, act, slope, residual, training=True,
                sync_group=None, sums=None, direct=None, res_sink=None, cat_buf=None, cat_total=0, cat_off=0):
        """``sync_group``: None, or a (process group or 'world') to synchronise the batch statistics over
        (torch.nn.SyncBatchNorm semantics: statistics over all ranks' rows, local dgamma / dbeta).
        ``sums``: the replicated [sum | sum of squares] buffer the producing conv filled (``conv2d(stats=)``):
        the statistics pass over ``x`` is skipped."""
        x = _kernel_map(x)
        code = _DCODE[x.dtype]
        N, Cc, H, W = x.shape
        assert Cc % 4 == 0, 'BatchNorm kernels need a channel count that is a multiple of 4'
        M = N * H * W
        dev = x.device
        L = _lib.lib()
        work = torch.empty(4 * Cc, dtype=torch.float64, device=dev)     # (4*C: room for the deterministic mode's lo words)
        mean = torch.empty(Cc, dtype=torch.float32, device=dev)
        invstd = torch.empty(Cc, dtype=torch.float32, device=dev)
        rows = None
        bwd_work = None

        def finalize(buf, replicas, m, rows, c, off=0, clean=0, wk=None):
            """Mean / inverse deviation / running statistics of the channels [off, off + c) from the sums in ``buf``."""
            check(L.yv4_bn_finalize(buf.data_ptr(), replicas, m, rows, c, float(eps), float(momentum), _ptr(mean, 4 * off),
                                    _ptr(invstd, 4 * off), _ptr(running_mean, 4 * off), _ptr(running_var, 4 * off), clean,
                                    wk, stream_ptr()), 'yv4_bn_finalize')

        if training and sync_group is not None:
            import torch.distributed as dist
            group = None if sync_group == 'world' else sync_group
            pre = sums
            sums = torch.empty(4 * Cc + 1, dtype=torch.float64, device=dev)[:2 * Cc + 1]   # [sum | sum of squares | rows]
            if pre is not None:
                check(L.yv4_conv_stats_fold(pre.data_ptr(), Cc, _kept_clean(pre), sums.data_ptr(), stream_ptr()),
                      'yv4_conv_stats_fold')
            else:       # (works in 4*C doubles: the tensor above is a view of 4*C + 1)
                check(L.yv4_bn_partial_sums(x.data_ptr(), code, M, Cc, Cc, 0, sums.data_ptr(), stream_ptr()),
                      'yv4_bn_partial_sums')
            sums[2 * Cc:].fill_(float(M))
            dist.all_reduce(sums, group=group)
            rows = sums[2 * Cc:]
            finalize(sums, 1, 0, rows.data_ptr(), Cc)
            ctx.sync_group = group
        elif training and isinstance(sums, (list, tuple)):
            # x is a concat buffer whose channel ranges were produced by several convs, each leaving its own sums
            # (``CatSlot`` + ``conv2d(stats=)``): one finalize per range, on the ranges of mean / invstd / running stats
            # (the finalize kernel clears the 4*c words at the pointer it is handed: the ranges' pieces tile the 4*Cc words
            # of the backward's accumulator)
            bwd_work = torch.empty(4 * Cc, dtype=torch.float64, device=dev)
            off = 0
            for buf in sums:
                c = buf.numel() // (2 * _lib.STATS_REPLICAS)
                finalize(buf, _lib.STATS_REPLICAS, M, None, c, off, _kept_clean(buf), _ptr(bwd_work, 32 * off))
                off += c
            assert off == Cc, 'the statistics buffers do not cover the concat buffer'
        elif training and sums is not None:
            # the finalize kernel also clears the backward's reduction buffer (and a persistent statistics buffer)
            bwd_work = torch.empty(4 * Cc, dtype=torch.float64, device=dev)
            finalize(sums, _lib.STATS_REPLICAS, M, None, Cc, 0, _kept_clean(sums), bwd_work.data_ptr())
        elif training:
            check(L.yv4_bn_train_stats_h16(x.data_ptr(), code, M, Cc, Cc, 0, float(eps), float(momentum),
                                           work.data_ptr(), mean.data_ptr(), invstd.data_ptr(), _ptr(running_mean),
                                           _ptr(running_var), stream_ptr()), 'yv4_bn_train_stats')
        else:       # eval-mode BN inside a training graph: the running statistics are constants
            mean.copy_(running_mean.detach().float())
            torch.rsqrt(running_var.detach().float() + eps, out=invstd)
        res = to_nhwc(residual.to(x.dtype)) if residual is not None else None
        y, y_cs, y_co = _cat_output(ctx, cat_buf, cat_total, cat_off, N, Cc, H, W, x.dtype, dev)
        g = gamma.detach().float().contiguous()
        b = beta.detach().float().contiguous()
        check(L.yv4_bn_act_fwd_h16(x.data_ptr(), code, Cc, 0, mean.data_ptr(), invstd.data_ptr(), g.data_ptr(),
                                   b.data_ptr(), _ptr(res), Cc, 0, y.data_ptr(), y_cs,
                                   y_co, M, Cc, int(act), float(slope), stream_ptr()), 'yv4_bn_act_fwd')
        ctx.save_for_backward(x, mean, invstd, g, b)
        ctx.direct = direct      # (_ParamRef(weight), _ParamRef(bias)): dgamma / dbeta are added to their .grad in place
        ctx.bwd_work = bwd_work  # 2*C doubles already cleared by the finalize kernel, or None
        ctx.rows = rows
        ctx.act = (int(act), float(slope))
        ctx.training = bool(training)
        ctx.has_res = residual is not None
        ctx.res_sink = res_sink if residual is not None else None      # GradSink: the residual's gradient is parked
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, invstd, g, b = ctx.saved_tensors
        act, slope = ctx.act
        N, Cc, H, W = x.shape
        dy, dcat = _cat_grad(ctx, dy, Cc)
        dy, dcs = nhwc_or_slice(dy, x.dtype)
        code = _DCODE[x.dtype]
        M = N * H * W
        dev = x.device
        dx = torch.empty_like(x, memory_format=torch.channels_last)
        dgamma = torch.empty(Cc, dtype=torch.float32, device=dev)
        dbeta = torch.empty(Cc, dtype=torch.float32, device=dev)
        work = torch.empty(4 * Cc, dtype=torch.float64, device=dev)
        L = _lib.lib()
        gw = gb = None
        # what every backward entry point starts with: x, dy (pixel stride, channel offset), statistics, affine
        ops = (x.data_ptr(), code, Cc, 0, dy.data_ptr(), dcs, 0, mean.data_ptr(), invstd.data_ptr(), g.data_ptr(), b.data_ptr())
        if ctx.rows is not None:            # SyncBN: local sums -> all-reduce -> apply with the totals
            import torch.distributed as dist
            check(L.yv4_bn_act_bwd_sums(*ops, dgamma.data_ptr(), dbeta.data_ptr(), work.data_ptr(), M, Cc, act, slope,
                                        stream_ptr()), 'yv4_bn_act_bwd_sums')
            dist.all_reduce(work[:2 * Cc], group=ctx.sync_group)     # (the other half is the deterministic mode's scratch)
            check(L.yv4_bn_act_bwd_apply(*ops, dx.data_ptr(), Cc, 0, work.data_ptr(), M, 0, ctx.rows.data_ptr(), Cc, act,
                                         slope, stream_ptr()), 'yv4_bn_act_bwd_apply')
        else:
            if ctx.direct is not None:
                gw, gb = ctx.direct[0].p.grad, ctx.direct[1].p.grad
                if not (_flat_f32(gw, Cc) and _flat_f32(gb, Cc)):
                    gw = gb = None
            if gw is not None:       # dgamma / dbeta added to the parameters' gradients by the kernel itself
                flags = 0 if ctx.training else 1
                wk = work
                if ctx.bwd_work is not None:
                    wk, flags = ctx.bwd_work, flags | 2
                    ctx.bwd_work = None          # one use: a second backward through this node memsets again
                check(L.yv4_bn_act_bwd_accum(*ops, dx.data_ptr(), Cc, 0, gw.data_ptr(), gb.data_ptr(), wk.data_ptr(), M, Cc,
                                             act, slope, flags, stream_ptr()), 'yv4_bn_act_bwd_accum')
            else:
                fn = L.yv4_bn_act_bwd_h16 if ctx.training else L.yv4_bn_eval_act_bwd
                check(fn(*ops, dx.data_ptr(), Cc, 0, dgamma.data_ptr(), dbeta.data_ptr(), work.data_ptr(), M, Cc, act, slope,
                         stream_ptr()), 'yv4_bn_act_bwd')
        dres = dy if ctx.has_res else None
        if dres is not None and ctx.res_sink is not None:
            ctx.res_sink.value, ctx.res_sink.cs = dy, dcs       # added by the data-gradient launch that consumes the sink
            dres = None
        if ctx.direct is not None:   # autograd does not track gamma / beta through this Function
            if ctx.rows is not None or gw is None:
                for ref, gr in zip(ctx.direct, (dgamma, dbeta)):
                    ref.p.grad = gr.clone() if ref.p.grad is None else ref.p.grad.add_(gr)
            for ref in ctx.direct:
                for cb in _direct_grad_listeners:
                    cb(ref.p)
            dgamma = dbeta = None
        return dx, dgamma, dbeta, None, None, None, None, None, None, dres, None, None, None, None, None, dcat, None, None


def _sync_group(bn):
    """The group a ``torch.nn.SyncBatchNorm`` (norm_cfg type 'SyncBN', configs/yolov5_ddp) synchronises over:
    its ``process_group`` or the world; None for a plain BatchNorm2d or a single-process run (torch's
    SyncBatchNorm also falls back to local statistics when world_size == 1, batchnorm.py ``need_sync``)."""
    import torch.distributed as dist
    if not isinstance(bn, torch.nn.SyncBatchNorm) or not bn.training:
        return None
    if not (dist.is_available() and dist.is_initialized()):
        return None
    group = bn.process_group
    if dist.get_world_size(group) <= 1:
        return None
    return group if group is not None else 'world'


def bn_act(x, bn, act=(0, 0.0), residual=None, sums=None, res_sink=None, cat=None):
    """``bn``: a torch BatchNorm2d; in training mode it normalises with batch statistics and updates
    the running ones, in eval mode (``norm_eval`` / frozen stages inside a training graph) with the
    running statistics as constants.  act = (YV4_ACT_*, slope)."""
    mom = bn.momentum if bn.momentum is not None else 0.1
    use_batch = bn.training or not bn.track_running_stats
    gamma, beta, direct = bn.weight, bn.bias, None
    if (_DIRECT_WGRAD and x.requires_grad and torch.is_grad_enabled() and gamma.requires_grad and beta.requires_grad
            and getattr(gamma, '_yv4_grad_in_arena', False) and getattr(beta, '_yv4_grad_in_arena', False)
            and _flat_f32(gamma.grad, gamma.numel()) and _flat_f32(beta.grad, beta.numel())):
        # dgamma / dbeta go straight into the parameters' gradients (see the note above ConvFunction)
        direct = (_ParamRef(gamma), _ParamRef(beta))
        gamma, beta = gamma.detach(), beta.detach()
    out = BNActFunction.apply(x, gamma, beta, bn.running_mean if bn.track_running_stats else None,
                              bn.running_var if bn.track_running_stats else None, bn.eps, mom, act[0], act[1],
                              residual, use_batch, _sync_group(bn) if use_batch else None,
                              sums if use_batch else None, direct, res_sink,
                              *(cat.args() if cat is not None else (None, 0, 0)))
    if bn.training and bn.track_running_stats and bn.num_batches_tracked is not None:
        if _fwd_depth[0] > 0:        # inside a registered module's training forward: one multi-tensor add at its end
            _nbt_pending.append(bn.num_batches_tracked)
        else:
            bn.num_batches_tracked += 1
    return out


# ``num_batches_tracked += 1`` of every BatchNorm is a 5 us launch on a scalar (108 per YOLOv4-L forward): inside a
# registered module's training forward (``HipModule._dispatch`` keeps the depth) they are collected and applied by
# one ``torch._foreach_add_`` when the outermost forward returns.
_fwd_depth = [0]
_nbt_pending = []


def flush_batch_counters():
    if _nbt_pending:
        torch._foreach_add_(_nbt_pending, 1)
        _nbt_pending.clear()


class ResampleIntoFunction(torch.autograd.Function):
    """Nearest resample of ``x`` to (Hd, Wd) written into a channel range of a concat buffer (``CatSlot``) -- the
    ``F.interpolate(...)`` + ``torch.cat`` of necks/yolo_neck_csp.py:213-219,229 without the intermediate tensor; with
    Hd == Hs it is the plain copy of a saved tensor into its concat half.  Backward: the buffer's gradient slice, summed
    over the pixels that read each source pixel (``yv4_resample_nearest_bwd``; the slice itself for the copy)."""

    @staticmethod
    def forward(ctx, x, Hd, Wd, cat_buf, cat_total, cat_off):
        x = _kernel_map(x)
        N, Cc, Hs, Ws = x.shape
        al = _chunk(x.dtype)
        assert Cc % al == 0 and cat_total % al == 0 and cat_off + Cc <= cat_total
        out, _, _ = _cat_output(ctx, cat_buf, cat_total, cat_off, N, Cc, Hd, Wd, x.dtype, x.device)
        k = 1 if x.dtype == torch.float32 else 2      # a 16-bit map with C % 8 == 0 is an fp32 map with C / 2 channels
        check(_lib.lib().yv4_resample_nearest_fwd(x.data_ptr(), out.data_ptr(), N, Hs, Ws, Hd, Wd, Cc // k, Cc // k, 0,
                                                  cat_total // k, cat_off // k, stream_ptr()), 'yv4_resample_nearest_fwd')
        ctx.geom = (N, Cc, Hs, Ws, Hd, Wd, x.dtype)
        return out

    @staticmethod
    def backward(ctx, dz):
        N, Cc, Hs, Ws, Hd, Wd, dtype = ctx.geom
        dy, dcat = _cat_grad(ctx, dz, Cc)
        dy, dcs = nhwc_or_slice(dy, dtype)
        if (Hs, Ws) == (Hd, Wd):
            dx = dy                                   # the copy's gradient is the slice itself (a strided view)
        else:
            dx = torch.empty((N, Cc, Hs, Ws), device=dz.device, dtype=dtype, memory_format=torch.channels_last)
            check(_lib.lib().yv4_resample_nearest_bwd(dy.data_ptr(), dx.data_ptr(), N, Hs, Ws, Hd, Wd, Cc, dcs, 0,
                                                      _DCODE[dtype], stream_ptr()), 'yv4_resample_nearest_bwd')
        return dx, None, None, dcat, None, None


def resample_into(x, size, cat):
    """``x`` nearest-resampled to ``size`` (an integer multiple of its own, or the same) into ``cat`` (a ``CatSlot``)."""
    return ResampleIntoFunction.apply(x, int(size[0]), int(size[1]), *cat.args())


def resample_into_ok(x, size):
    """Integer scale factors (what the backward kernel sums over), 16-byte channel chunks."""
    Hs, Ws = x.shape[2], x.shape[3]
    return x.is_cuda and x.dtype in _DCODE and x.shape[1] % _chunk(x.dtype) == 0 and size[0] % Hs == 0 and size[1] % Ws == 0 \
        and size[0] // Hs <= 8 and size[1] // Ws <= 8


class SPPCatFunction(torch.autograd.Function):
    """``torch.cat([x, mp5(x), mp9(x), mp13(x)], 1)`` (darknetcsp.py:176-181,203-206,222-226) as one
    forward (slice copy + ``yv4_spp_pool_fwd``) and one backward launch (``yv4_spp_pool_bwd``); the
    concat buffer itself is what is saved."""

    @staticmethod
    def forward(ctx, x):
        x = _kernel_map(x)
        N, Cc, H, W = x.shape
        al = _chunk(x.dtype)
        assert Cc % al == 0, f'SPP kernels need a channel count that is a multiple of {al}'
        out = torch.empty((N, 4 * Cc, H, W), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        out[:, :Cc] = x
        _spp_pool_fwd(out, N, H, W, Cc)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, dcat):
        out, = ctx.saved_tensors
        N, C4_, H, W = out.shape
        Cc = C4_ // 4
        dcat = to_nhwc(dcat.to(out.dtype))
        dx = torch.zeros((N, Cc, H, W), dtype=torch.float32, device=out.device).contiguous(
            memory_format=torch.channels_last)
        check(_lib.lib().yv4_spp_pool_bwd(out.data_ptr(), 4 * Cc, 0, dcat.data_ptr(), 4 * Cc, 0, dx.data_ptr(), N, H, W,
                                          Cc, _DCODE[out.dtype], stream_ptr()), 'yv4_spp_pool_bwd')
        return dx.to(out.dtype)


def spp_cat(x):
    return SPPCatFunction.apply(x)
