"""Packed weight operands of the training convs (``csrc/pack_weights.hip``): the table that re-packs all of them in one
launch per optimizer step, and the row-pair operands of the few-channel stride-2 data gradient.  ``train_ops`` is the
user; the two caches are separate structures that share one staleness test (``_is_current``)."""
import os
import weakref

import torch

from . import _lib
from ._lib import DTYPE_CODE as _DCODE, check
from .ops import stream_ptr

# ---- A/B switch, read once at import -----------------------------------------------------------------------------------
_PACK_CACHE_ON = os.environ.get('YV4_PACK_CACHE', '1') != '0'     # off: every request packs with a launch of its own


def _chunk(dtype):
    """Channels in one 16-byte chunk: the alignment every kernel asks of channel counts, offsets and pixel strides."""
    return 4 if dtype == torch.float32 else 8


# Staleness is detected through torch's version counters; an update that bypasses them (``p.data.copy_()``, a
# raw-pointer kernel) must call ``invalidate_packed_weights()`` -- FlatSGD.step, load_state_dict of a FlatState model and
# the EMA swap do (they also bump the versions) -- which makes the next request re-pack everything.
_generation = 0


def invalidate_packed_weights():
    global _generation
    _generation += 1


def _is_current(wref, version, gen, owner):
    """A cached operand is still the packed form of ``owner``'s present values: the weak reference recorded with it is
    to this very object (not to a dead tensor whose address or id was handed on), torch's version counter has not moved
    since it was packed, and nobody called ``invalidate_packed_weights()`` since."""
    return wref() is owner and version == owner._version and gen == _generation


# ---- packed weight operands, replayed in one launch per optimizer step -----------------------------------------------
# A training step needs every conv weight twice as a packed 16-bit (or fp32) operand: (Cout, K) for the forward, the
# transposed / mirrored form for the data gradient (plus one per parity class of a stride-2 layer) -- 750 launches of
# ``yv4_pack_weight`` per YOLOv4-L step.  The operands only change when the weights do, so the requests of the first
# step are recorded in a table (``yv4_pack_desc``) and from then on ONE ``yv4_pack_weights_multi`` launch refreshes all
# of them the first time any operand is asked for after the weights' version counter moved.  The version is torch's
# (views of the flat arena share the arena's counter; ``FlatSGD.step`` bumps it for its raw-pointer kernel).
# YV4_PACK_CACHE=0 packs per call as before.
class _PackCache:
    ROWS_TARGET = 16384         # output elements per workgroup

    def __init__(self, device):
        self.device = device
        self.entries = {}       # key -> dict(weight=weakref, desc fields, dst, version)
        self.table = None       # device copy of the descriptor table (rebuilt when entries were added)
        self.dirty_table = True
        self.total_blocks = 0

    @staticmethod
    def key(weight, dtype, mode):
        return (weight.data_ptr(), tuple(weight.shape), tuple(weight.stride()), dtype, mode)

    def lookup(self, weight, dtype, mode):
        e = self.entries.get(self.key(weight, dtype, mode))
        if e is None:
            return None
        if e['wref']() is not weight:       # the owner died and the allocator handed its address to another tensor of the
            del self.entries[self.key(weight, dtype, mode)]     # same shape: a miss (the table is rebuilt on the next add)
            self.dirty_table = True
            return None
        if not _is_current(e['wref'], e['version'], e['gen'], weight):
            self.refresh(weight)
        return e

    def add(self, weight, dtype, mode, fields, dst, cp):
        """Only PERSISTENT weights come here (``packed_weight``: leaves of the autograd graph, i.e. parameters); the
        entry holds a weak reference, so a model that is dropped takes its entries with it at the next refresh."""
        e = dict(fields=fields, dst=dst, cp=cp, version=weight._version, gen=_generation, wref=weakref.ref(weight))
        self.entries[self.key(weight, dtype, mode)] = e
        self.dirty_table = True
        return e

    def _build(self):
        n = len(self.entries)
        tab = (_lib.PackDesc * n)()
        blk = 0
        for i, e in enumerate(self.entries.values()):
            d = tab[i]
            for k, v in e['fields'].items():
                setattr(d, k, v)
            d.dst = e['dst'].data_ptr()
            rows = (d.Cin if d.transpose else d.Cout) * d.KHo * d.KWo
            icp = ((d.Cout if d.transpose else d.Cin) + d.pad_to - 1) // d.pad_to * d.pad_to
            # whole rows r (all their taps) per workgroup; the data-gradient operand is read ACROSS r (the source is
            # contiguous along it), so its workgroups take groups of rows (pack_rows in csrc/pack_weights.hip)
            taps = d.KHo * d.KWo
            group = taps * (max(8, 64 // taps) if d.transpose else 1)
            d.rows_per_block = group * max(1, self.ROWS_TARGET // (icp * group))
            d.nblocks = (rows + d.rows_per_block - 1) // d.rows_per_block
            d.first_block = blk
            blk += d.nblocks
        self.total_blocks = blk
        raw = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8)
        self.table = raw.to(self.device)
        self.dirty_table = False

    def refresh(self, _weight):
        """Re-pack every recorded operand in one launch (the weights move together at an optimizer step)."""
        live = {}
        for k, e in self.entries.items():
            w = e['wref']()
            if w is not None and w.data_ptr() == k[0]:
                live[k] = e
        if len(live) != len(self.entries):
            self.entries = live
            self.dirty_table = True
        if not self.entries:
            return
        if self.dirty_table:
            self._build()
        check(_lib.lib().yv4_pack_weights_multi(self.table.data_ptr(), len(self.entries), self.total_blocks, stream_ptr()),
              'yv4_pack_weights_multi')
        for e in self.entries.values():
            e['version'] = e['wref']()._version
            e['gen'] = _generation


_PACK_CACHES = {}


def clear_pack_cache():
    _PACK_CACHES.clear()


def packed_weight(weight, dtype, transpose_flip=False, taps=None, owner=None, pad_to=None):
    """The conv kernels' weight operand from an fp32 (Cout, Cin, KH, KW) parameter in one launch (``yv4_pack_weight``):
    rows x (KH'*KW'*Cp), K ordered (kh, kw, channel), channels zero-padded to a 16-byte chunk, cast to ``dtype``.
    ``transpose_flip``: the data gradient's operand (rows = Cin, channels = Cout, taps mirrored).  ``taps``:
    ((kh0, kh_step, KH'), (kw0, kw_step, KW')) selects source taps explicitly (rows = Cin, channels = Cout): the
    operand of one parity class of a stride-2 data gradient.  Returns (w, Cp).  The result is a cached buffer that the
    next refresh overwrites: use it on the current stream before the weights change again (the conv launches do).
    ``owner``: the parameter ``weight`` is a detached alias of (``conv2d`` hands ``ConvFunction`` the detached weight
    when dW goes straight into ``weight.grad``): the table records and weakly references the OWNER, so a fresh alias
    per step still hits its entry.  ``pad_to``: pad the channels to a multiple of this instead of one 16-byte chunk (the
    stem: 3 input channels against an activation stored with 16)."""
    Cout, Cin, KH, KW = weight.shape
    al = _chunk(dtype)
    if pad_to is not None:
        assert pad_to % al == 0
        al = pad_to
    transpose = bool(transpose_flip or taps is not None)
    rows, ic = (Cin, Cout) if transpose else (Cout, Cin)
    cp = (ic + al - 1) // al * al
    if taps is not None:
        (kh0, khs, KHo), (kw0, kws, KWo) = taps
    elif transpose_flip:
        kh0, khs, KHo, kw0, kws, KWo = KH - 1, -1, KH, KW - 1, -1, KW
    else:
        kh0, khs, KHo, kw0, kws, KWo = 0, 1, KH, 0, 1, KW
    w = weight.detach()
    # temporaries (the stem weight zero-padded to a 16-byte chunk in every step, darknetcsp.Conv.fwd: a fresh non-leaf
    # tensor each time) take the per-call launch below: cached, each step would add an entry that is never hit again
    ident = owner if owner is not None else weight
    persistent = ident.is_leaf and (ident.requires_grad or isinstance(ident, torch.nn.Parameter)) and \
        ident.data_ptr() == weight.data_ptr()
    cacheable = _PACK_CACHE_ON and persistent and w.dtype == torch.float32 and w.is_cuda
    cache = None
    mode = (bool(transpose_flip), taps, al)
    if cacheable:
        cache = _PACK_CACHES.get(w.device)
        if cache is None:
            cache = _PACK_CACHES[w.device] = _PackCache(w.device)
        e = cache.lookup(ident, dtype, mode)
        if e is not None:
            return e['dst'], e['cp']
    if w.dtype != torch.float32:
        w = w.float()
    out = torch.empty((rows, KHo * KWo * cp), device=w.device, dtype=dtype)
    st = w.stride()
    check(_lib.lib().yv4_pack_weight(w.data_ptr(), st[0], st[1], st[2], st[3], Cout, Cin, KH, KW, KHo, KWo, kh0, khs, kw0,
                                     kws, int(transpose), al, out.data_ptr(), _DCODE[dtype], stream_ptr()),
          'yv4_pack_weight')
    if cacheable:
        cache.add(ident, dtype, mode, dict(w=w.data_ptr(), s_co=st[0], s_ci=st[1], s_kh=st[2], s_kw=st[3], Cout=Cout, Cin=Cin,
                                       KHo=KHo, KWo=KWo, kh0=kh0, kh_step=khs, kw0=kw0, kw_step=kws,
                                       transpose=int(transpose), pad_to=al, dtype=_DCODE[dtype]), out, cp)
    return out, cp


_ROWPAIR_W = {}     # id(owner) -> (weakref(owner), version, generation, dtype, (W2 for a = 0, W2 for a = 1))


def _rowpair_weights(weight, dtype, owner):
    """Operands of ``train_ops._dgrad_s2_rowpair``: for row parity a, rows = (b, c) -- column parity and input channel --,
    K ordered (di, dj, co) over the dY taps (i + di, j + dj); zero where the (parity, tap) pair has no source tap.
    Cached per parameter until its version (or the packed-weight generation) moves."""
    ident = owner if owner is not None else weight
    key = id(ident)
    hit = _ROWPAIR_W.get(key)
    if hit is not None and _is_current(hit[0], hit[1], hit[2], ident) and hit[3] == dtype:
        return hit[4]
    w = weight.detach().float()
    Co, Cx = w.shape[0], w.shape[1]
    out = []
    for khs in ((1,), (2, 0)):                       # a = 0: dY row i through kh = 1;  a = 1: row i (kh = 2), row i + 1 (kh = 0)
        t = w.new_zeros((2, Cx, len(khs), 2, Co))    # (b, c, di, dj, co)
        for di, kh in enumerate(khs):
            t[0, :, di, 0] = w[:, :, kh, 1].t()      # b = 0: column j through kw = 1
            t[1, :, di, 0] = w[:, :, kh, 2].t()      # b = 1: column j (kw = 2) ...
            t[1, :, di, 1] = w[:, :, kh, 0].t()      # ... and column j + 1 (kw = 0)
        out.append(t.reshape(2 * Cx, len(khs) * 2 * Co).to(dtype).contiguous())
    if len(_ROWPAIR_W) > 64:
        _ROWPAIR_W.clear()
    _ROWPAIR_W[key] = (weakref.ref(ident), ident._version, _generation, dtype, tuple(out))
    return tuple(out)
