"""Resident pre-split conv weights (include/ssv_hip.h, "Resident pre-split weights").

The split-bf16 conv kernels read weights as bf16 hi/lo planes in MFMA fragment order.  Splitting a weight is one
small launch per conv call (forward order for the forward, transposed order for the data gradient) -- about a
hundred launches per training step.  A ``ResidentWeights`` keeps one plane buffer per conv weight and refreshes
all of them with ONE launch (``ssv_conv_pack_multi``); ``FusedAdam`` does that right after its update, so the next
step's convolutions find current planes and skip their own split.

Each weight carries its entry (``_ssv_planes``, as activations carry ``ops.amax_of``'s scale lists): the planes, the pack
shape, the weight's address and autograd version (``Tensor._version``) at the last refresh, and a weak reference to the
owning ``ResidentWeights``.  ``lookup(w)`` resolves a view to its weight (``w._base``) and returns the planes only while the
weight keeps that address and version, ``w`` starts at that address with the pack shape, and the owner lives; anything
else is a miss and the conv splits the weight itself.  In-place torch ops (``load_state_dict``, ``init``) bump the
version; writers that go around it (``p.data`` writes, collectives) must call ``invalidate``.
"""
import ctypes
import weakref

import numpy as np
import torch

from . import _lib

_LIVE = weakref.WeakSet()                # every ResidentWeights (invalidate(None))
_INFER = weakref.WeakKeyDictionary()     # inference module -> its ResidentWeights (ensure)


class _Entry:
    __slots__ = ("planes", "shape", "version", "addr", "owner")

    def __reduce__(self):                # a pickled or deep-copied weight carries no planes
        return type(None), ()


def param_of(t):
    """The parameter that tensor ``t`` is, or is a view of: what ``lookup``, ``gradarena`` and ``ops`` hang a parameter's state on and
    find it by (never by address: another tensor may live there).  Relies on autograd handing a ``Function`` its caller's tensor
    OBJECTS, in ``forward`` and again from ``ctx.saved_tensors``, and on a view of a view naming the root as its ``_base``; a tensor
    that merely shares storage (``q.data = p.data``, ``p.detach()``) has no ``_base`` and is nobody's view."""
    return t if t._base is None else t._base


def lookup(w):
    """ctypes pointer to current planes of weight ``w`` (a (Cout, Cin, k) tensor or the packed view of one), or None."""
    p = param_of(w)
    e = getattr(p, "_ssv_planes", None)
    if (e is None or e.version != p._version or e.addr != p.data_ptr() or w.data_ptr() != e.addr or e.shape != tuple(w.shape)
            or e.owner() is None):
        return None
    return e.planes


def _owner(p):
    e = getattr(p, "_ssv_planes", None)
    return e.owner() if e is not None else None


def invalidate(params=None):
    """Forget the planes of ``params`` (all live ones when None); they are rebuilt by the next refresh."""
    for p in ([p for rw in _LIVE for p in rw.params] if params is None else params):
        e = getattr(p, "_ssv_planes", None)
        if e is not None:
            e.version = -1


def mark_transposed(p):
    """Declare ``p`` the (Cin, Cout, 2) weight of a ConvTranspose1d(k = 2, s = 2) (``tts.upsampling`` at construction, ``ops.deconv1d_k2s2`` on
    every call): its planes are kept for the 1x1 weight ``p.view(Cin, 2 Cout, 1)`` its data gradient is a forward convolution with.  A
    ``copy.deepcopy`` of a model loses the mark (a Python attribute) until the copy's first deconvolution; a plane set built before that leaves
    the weight out, and the copy splits it per call -- correct, slower.  The package itself never deep-copies a model."""
    p._ssv_transposed = True
    return p


def eligible(p):
    return (p.is_cuda and p.dtype == torch.float32 and p.dim() == 3 and p.is_contiguous()
            and p.shape[2] in ((2,) if getattr(p, "_ssv_transposed", False) else (1, 3)))


def pack_shape(p):
    """The (Cout, Cin, k) conv weight whose planes are kept for parameter ``p``: itself, or the 1x1 view of a ``mark_transposed`` weight."""
    return (p.shape[0], 2 * p.shape[1], 1) if getattr(p, "_ssv_transposed", False) else tuple(p.shape)


class ResidentWeights:
    """Plane buffers + the device job table for a fixed list of conv weights."""

    def __init__(self, params):
        self.params = [p for p in params if eligible(p)]
        self._key = None
        self._jobs = None
        self._nblocks = 0
        _LIVE.add(self)

    def _build(self):
        key = tuple(p.data_ptr() for p in self.params)
        if key == self._key:
            return
        n = len(self.params)
        dev = self.params[0].device
        sizes = [int(_lib.query("ssv_conv_pack_bytes", *pack_shape(p))) for p in self.params]
        self._planes = [torch.empty(s, dtype=torch.uint8, device=dev) for s in sizes]
        vp = ctypes.c_void_p
        w = (vp * n)(*[p.data_ptr() for p in self.params])
        pl = (vp * n)(*[t.data_ptr() for t in self._planes])
        ci = lambda k: (ctypes.c_int * n)(*[pack_shape(p)[k] for p in self.params])
        jobs = (_lib.PackJob * (2 * n))()
        nblocks = _lib.lib().ssv_conv_pack_plan(n, w, pl, ci(0), ci(1), ci(2), jobs)
        if nblocks < 0:
            raise RuntimeError("ssv_conv_pack_plan: " + _lib.lib().ssv_last_error().decode())
        raw = np.frombuffer(bytes(jobs), dtype=np.uint8).copy()
        host = torch.from_numpy(raw).pin_memory()
        self._jobs = torch.empty(raw.size, dtype=torch.uint8, device=dev)
        self._jobs.copy_(host, non_blocking=False)
        self._nblocks, self._njobs = nblocks, 2 * n
        self._ws_bytes = int(_lib.query("ssv_conv_pack_multi_workspace", 2 * n))
        self._ws = torch.empty(max(self._ws_bytes, 256), dtype=torch.uint8, device=dev)      # the weights' partial maxima (split-fp16)
        me = weakref.ref(self)                 # weak: the weights must not keep their planes alive once the owner is gone
        for p, t in zip(self.params, self._planes):
            e = p._ssv_planes = _Entry()
            e.planes, e.shape, e.version, e.addr, e.owner = ctypes.c_void_p(t.data_ptr()), pack_shape(p), -1, None, me
        self._key = key

    def refresh(self, stream):
        """Re-split every weight on ``stream`` (one launch) and mark the planes current."""
        if not self.params:
            return
        self._build()
        _lib.call("ssv_conv_pack_multi", ctypes.c_void_p(self._jobs.data_ptr()), self._njobs, self._nblocks,
                  ctypes.c_void_p(self._ws.data_ptr()), self._ws_bytes, stream)
        for p in self.params:
            if _owner(p) is self:
                p._ssv_planes.version, p._ssv_planes.addr = p._version, p.data_ptr()


def ensure(module, stream):
    """Inference helper: keep the conv weights of ``module`` resident.  The first call builds the planes; later calls cost
    one version check per weight and re-split (one launch) only if a weight was modified since (``load_state_dict``, init).
    The plane set lives as long as the module does."""
    # A weight has ONE set of planes.  When the module's weights already belong to a training optimizer's ResidentWeights
    # (FusedAdam re-splits those after every update -- inside the captured hipGraph when the step is replayed from one),
    # use and, if stale, refresh THOSE: a second set registered here would be written once and then go stale behind the
    # version check, because FusedAdam updates weights through raw pointers.
    mine = [p for p in module.parameters() if eligible(p)]
    rw = _INFER.get(module)
    owners = {id(o): o for o in map(_owner, mine)}
    if owners and not any(o is None or o is rw for o in owners.values()):
        if any(lookup(p) is None for p in mine):
            for o in owners.values():
                o.refresh(stream)
        return next(iter(owners.values()))
    if rw is None or [id(p) for p in rw.params] != [id(p) for p in mine]:
        rw = _INFER[module] = ResidentWeights(mine)
    if any(lookup(p) is None for p in rw.params):
        rw.refresh(stream)
    return rw
