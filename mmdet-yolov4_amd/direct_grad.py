"""Where the weight gradients of the training Functions go (``train_ops`` is the user): straight into the flat gradient
arena, with listeners for whoever must know that such a gradient is final, and on a side stream that is joined at the end
of every backward pass."""
import os

import torch

# ---- A/B switches, read once at import ---------------------------------------------------------------------------------
_DIRECT_WGRAD = os.environ.get('YV4_DIRECT_WGRAD', '1') != '0'    # off: dW / dgamma / dbeta are returned to autograd
_WGRAD_STREAM = os.environ.get('YV4_WGRAD_STREAM', '1') != '0'    # off: weight gradients run on the current stream

# ---- weight gradients straight into the gradient arena -----------------------------------------------------
# When a conv weight's ``.grad`` is a channels_last fp32 tensor that already exists at backward time (the flat
# gradient arena of ``flat_state.FlatState``, zeroed once per step), ``yv4_conv_wgrad*`` accumulates INTO it -- its
# (Cout, KH, KW, Cin) memory is exactly the kernel's dW layout and the kernels only ever atomicAdd -- and the
# Function returns no gradient for the weight.  That removes, per conv and step, the zero fill of a scratch dW and
# autograd's ``grad += dW`` (230 launches of the YOLOv4-L step).  autograd's post-accumulate hooks do not fire for
# such a weight (the Function is given the detached weight, so autograd never sees it), so whoever needs to know
# that a weight gradient is final registers a listener here
# (``dist.GradReducer`` does).  YV4_DIRECT_WGRAD=0 restores the autograd path.
_direct_grad_listeners = []
_listeners_need_main_stream = []     # listeners that assume the gradient was written on the CURRENT stream


def add_direct_grad_listener(cb, side_stream_ok=False):
    """``cb(weight)`` is called after a conv's backward accumulated dW into ``weight.grad`` directly.  ``side_stream_ok``:
    the listener knows that the weight gradient may have been launched on the side stream and orders itself behind
    ``wgrad_side_stream(device)`` (the gradient exchange does: ``GradReducer._launch``); a listener that does not say so
    switches the side stream off while it is registered."""
    _direct_grad_listeners.append(cb)
    if not side_stream_ok:
        _listeners_need_main_stream.append(cb)
    return cb


def remove_direct_grad_listener(cb):
    if cb in _direct_grad_listeners:
        _direct_grad_listeners.remove(cb)
    if cb in _listeners_need_main_stream:
        _listeners_need_main_stream.remove(cb)


def _flat_f32(g, n):
    return g is not None and g.dtype == torch.float32 and g.numel() == n and g.is_contiguous()


class _ParamRef:
    """Carries a parameter through ``Function.apply`` without autograd seeing a tensor argument."""
    __slots__ = ('p',)

    def __init__(self, p):
        self.p = p


def _direct_grad_target(weight, cp):
    g = weight.grad
    if not _DIRECT_WGRAD or g is None or g.dtype != torch.float32 or g.shape != weight.shape or cp != weight.shape[1]:
        return None
    if not getattr(weight, '_yv4_grad_in_arena', False) or not g.permute(0, 2, 3, 1).is_contiguous():
        return None
    return g


_WGRAD_WS = {}


def _wgrad_workspace(nbytes, device, stream_key=None):
    """One growing fp32 scratch per (device, stream), shared by all layers (kernels on one stream run in order)."""
    if not nbytes:
        return None
    key = (device, stream_key)
    ws = _WGRAD_WS.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
        _WGRAD_WS[key] = ws
    return ws


# The weight gradient of a layer is needed by nobody before the optimizer (or the gradient exchange), while the data gradient
# is on backward's critical path: with dW going straight into the gradient arena, ``yv4_conv_wgrad*`` is launched on a SIDE
# stream.  It then runs beside the BatchNorm backward passes of the layers in front of it -- matrix-pipe-bound work
# beside HBM-bound work -- instead of between them.  Ordering: the side stream waits for the current stream at every launch
# (dY, x and the zeroed arena are ready), the tensors are handed to the allocator with ``record_stream``, and the current
# stream waits for the side stream in a callback the autograd engine runs at the END of this backward pass (so every
# ``.backward()`` leaves finished gradients behind, whoever called it).  Gradient listeners: the multi-GPU exchange launches
# a bucket when its last weight gradient has been ISSUED, and orders the bucket's collective behind the side stream itself
# (``GradReducer._launch`` -> ``wgrad_side_stream``); any other listener switches the side stream off while registered.
# YV4_WGRAD_STREAM=0 keeps everything on one stream.
class _SideStream:
    def __init__(self):
        self.streams = {}           # device -> its side stream, made on first use
        self.join_pending = False   # a join callback is queued with the autograd engine for the backward pass in flight
        self.dirty = False          # a side stream holds weight gradients the current stream has not waited for

    def for_launch(self, device):
        """The stream to launch a weight gradient of ``device`` on, or None (switched off, or a listener needs the
        gradient on the current stream)."""
        if not _WGRAD_STREAM or _listeners_need_main_stream:
            return None
        st = self.streams.get(device)
        if st is None:
            st = self.streams[device] = torch.cuda.Stream(device=device)
        return st

    def issued(self, side, *tensors):
        """A weight gradient that reads ``tensors`` was launched on ``side``: the allocator learns of the second stream,
        and the join is queued for the end of the backward pass in flight (once per pass)."""
        for t in tensors:
            if t is not None:
                t.record_stream(side)
        self.dirty = True
        if not self.join_pending:
            self.join_pending = True
            torch.autograd.Variable._execution_engine.queue_callback(self.join)

    def join(self):
        """Make the current stream wait for every weight gradient launched on a side stream.  Idempotent and cheap (one event
        wait per device when something is pending, nothing otherwise).  The autograd callback does this at the end of every
        backward pass -- but the engine DROPS queued callbacks when a backward raises (an OOM retry, ``pytest.raises``, a failed
        check in a later node), so nothing may rely on the callback alone: the optimizer step, the gradient hooks, the gradient
        exchange, ``FlatState.zero_grad`` and the next forward pass all call this before they touch the gradient arena."""
        self.join_pending = False
        if self.dirty:
            self.dirty = False
            for dev, st in self.streams.items():
                torch.cuda.current_stream(dev).wait_stream(st)

    def unjoined(self, device):
        """The side stream that holds weight gradients not yet joined into the current stream of ``device``, or None."""
        return self.streams.get(torch.device(device)) if self.dirty else None


_side = _SideStream()
join_side_streams = _side.join
wgrad_side_stream = _side.unjoined
