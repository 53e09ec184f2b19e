"""Host-side mirror of the reference's GE2E speaker embedder (``GE2E/speech_embedder_net.py``).

``SpeechEmbedder().forward(x)``: (B, frames, n_mels) -> (B, proj) unit-norm d-vectors
(speech_embedder_net.py:27-33); ``GE2ELoss(device).forward(emb)``: (N, M, D) -> scalar loss
(:43-49 with GE2E/utils.py:16-55).  The LSTM stack, the projection and the loss run in libssv_hip.so, forward (what
BASELINE.json's north_star asks) and backward (one iteration of GE2E/train_speech_embedder.py:70-86
through ``train_iteration``, which ends in torch's own clip_grad_norm_ and SGD; ``GE2ETrainStep``, the iteration on a corpus held
on the device, runs those too in libssv_hip.so: ``ClipSGD``, and ``tisv_batch_gather`` for the batch).  State-dict keys equal the
reference's (``LSTM_stack.weight_ih_l0`` ... ``projection.bias``), so its checkpoints load unchanged.

The reference reads its sizes from a module-global ``hparam`` loaded from config/config.yaml; here they
are constructor arguments whose defaults are that file's values (nmels 40, hidden 768, 3 layers,
proj 256; GE2E/config/config.yaml:16,21-23).
"""
import ctypes
import weakref

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .ops import _c, _dev, _p, _stream, _ws


def _ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


# SpeechEmbedder -> its last inference call's workspace and what it was prepared for (see _EmbedderFn.forward).  Keyed by
# the module itself, weakly: an entry can only serve the module that wrote it and is freed with it.
_FWD_CACHE = weakref.WeakKeyDictionary()


class _EmbedderFn(torch.autograd.Function):
    """SpeechEmbedder.forward (speech_embedder_net.py:27-33) with its backward: LSTM stack -> last frame -> Linear -> x/|x|.
    Inputs: ``cache`` (None: training, every frame is kept for the backward; otherwise the calling module's dict that keeps
    the inference workspace), x, projection weight, projection bias, then per layer w_ih, w_hh, b_ih, b_hh."""

    @staticmethod
    def forward(ctx, cache, x, pw, pb, *lstm):
        train = cache is None
        layers = len(lstm) // 4
        Bn, T, F = x.shape
        H, P = lstm[1].shape[1], pw.shape[0]
        w_ih, w_hh = [_c(lstm[4 * l]) for l in range(layers)], [_c(lstm[4 * l + 1]) for l in range(layers)]
        b_ih, b_hh = [_c(lstm[4 * l + 2]) for l in range(layers)], [_c(lstm[4 * l + 3]) for l in range(layers)]
        pw, pb = _c(pw), _c(pb)
        h_last = torch.empty((Bn, H), dtype=torch.float32, device=x.device)
        args = (_ptr_array(w_ih), _ptr_array(w_hh), _ptr_array(b_ih), _ptr_array(b_hh))
        if train:
            saved = _ws(_lib.query("ssv_lstm_saved_bytes", Bn, T, F, H, layers), x.device)
            nb = _lib.query("ssv_lstm_train_fwd_workspace", Bn, T, F, H, layers)
            ws = _ws(nb, x.device)
            _lib.call("ssv_lstm_train_fwd", _p(x), *args, _p(h_last), _p(saved), Bn, T, F, H, layers, _p(ws), nb, _stream())
        else:
            # d-vector extraction runs batch after batch on fixed weights: the workspace (with the split weight planes and their scale) is kept
            # in the module's cache between calls and re-used as long as shape, arithmetic mode, stream and every weight's (address, version)
            # are the same
            nb = _lib.query("ssv_lstm_fwd_workspace", Bn, T, F, H, layers)
            key = (Bn, T, F, H, layers, _lib.precision(), x.device, _stream().value, tuple((t.data_ptr(), t._version) for t in lstm))
            hit = cache.get("key") == key
            ws = cache["ws"] if hit else _ws(nb, x.device)
            _lib.call("ssv_lstm_fwd_cached", _p(x), *args, _p(h_last), Bn, T, F, H, layers, _p(ws), nb, 1 if hit else 0, _stream())
            cache["key"], cache["ws"] = key, ws
        e = torch.empty((Bn, P), dtype=torch.float32, device=x.device)
        norms = torch.empty((Bn,), dtype=torch.float32, device=x.device) if train else None
        nb2 = _lib.query("ssv_proj_l2norm_fwd_workspace", Bn, P)
        ws2 = _ws(nb2, x.device)
        _lib.call("ssv_proj_l2norm_fwd", _p(h_last), _p(pw), _p(pb), _p(e), _p(norms), Bn, H, P, _p(ws2), nb2, _stream())
        if train:
            ctx.save_for_backward(saved, h_last, e, norms, pw, *w_ih, *w_hh)
            ctx.dims = (Bn, T, F, H, P, layers)
        return e

    @staticmethod
    def backward(ctx, de):
        Bn, T, F, H, P, layers = ctx.dims
        saved, h_last, e, norms, pw = ctx.saved_tensors[:5]
        w_ih = list(ctx.saved_tensors[5:5 + layers])
        w_hh = list(ctx.saved_tensors[5 + layers:5 + 2 * layers])
        dev = e.device
        de = _c(de)
        dh = torch.empty((Bn, H), dtype=torch.float32, device=dev)
        dpw = torch.empty_like(pw)
        dpb = torch.empty((P,), dtype=torch.float32, device=dev)
        nb = _lib.query("ssv_proj_l2norm_bwd_workspace", Bn, P)
        ws = _ws(nb, dev)
        _lib.call("ssv_proj_l2norm_bwd", _p(de), _p(e), _p(norms), _p(h_last), _p(pw), _p(dh), _p(dpw), _p(dpb), Bn, H, P,
                  _p(ws), nb, _stream())
        dw_ih = [torch.empty_like(w) for w in w_ih]
        dw_hh = [torch.empty_like(w) for w in w_hh]
        db_ih = [torch.empty((4 * H,), dtype=torch.float32, device=dev) for _ in range(layers)]
        db_hh = [torch.empty((4 * H,), dtype=torch.float32, device=dev) for _ in range(layers)]
        nb2 = _lib.query("ssv_lstm_bwd_workspace", Bn, T, F, H, layers)
        ws2 = _ws(nb2, dev)
        _lib.call("ssv_lstm_bwd", _p(dh), _p(saved), _ptr_array(w_ih), _ptr_array(w_hh), _ptr_array(dw_ih), _ptr_array(dw_hh),
                  _ptr_array(db_ih), _ptr_array(db_hh), Bn, T, F, H, layers, _p(ws2), nb2, _stream())
        grads = []
        for l in range(layers):
            grads += [dw_ih[l], dw_hh[l], db_ih[l], db_hh[l]]
        return (None, None, dpw, dpb) + tuple(grads)


class SpeechEmbedder(nn.Module):
    def __init__(self, nmels=40, hidden=768, num_layer=3, proj=256):
        super().__init__()
        self.LSTM_stack = nn.LSTM(nmels, hidden, num_layers=num_layer, batch_first=True)
        for name, param in self.LSTM_stack.named_parameters():      # speech_embedder_net.py:20-24
            if "bias" in name:
                nn.init.constant_(param, 0.0)
            elif "weight" in name:
                nn.init.xavier_normal_(param)
        self.projection = nn.Linear(hidden, proj)
        self.dims = (nmels, hidden, num_layer, proj)

    def forward(self, x):
        _dev(x, "utterance batch")
        x = _c(x)
        nmels, H, layers, P = self.dims
        if x.shape[2] != nmels:
            raise RuntimeError("SpeechEmbedder: input has %d mel bins, model expects %d" % (x.shape[2], nmels))
        lstm = self.LSTM_stack
        params = []
        for l in range(layers):
            params += [getattr(lstm, "%s_l%d" % (kind, l)) for kind in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        if self.training and torch.is_grad_enabled():
            # keeps every frame for backpropagation through time (ssv_lstm_saved_bytes: 5.8 GB at 880 x 120 frames)
            return _EmbedderFn.apply(None, x, self.projection.weight, self.projection.bias, *params)
        with torch.no_grad():       # d-vector extraction (GE2E/dvector_create.py:100): nothing is kept but the workspace
            return _EmbedderFn.apply(_FWD_CACHE.setdefault(self, {}), x, self.projection.weight, self.projection.bias, *params)

    def invalidate(self):
        """Drop the kept inference workspace (the split LSTM weight planes); the next call splits the weights again.  Calls
        notice in-place torch updates of the weights (version) and rebinds (address) by themselves; call this after writing
        weights through ``.data`` (``p.data.copy_(...)``), which leaves both unchanged."""
        _FWD_CACHE.pop(self, None)


class _GE2ELossFn(torch.autograd.Function):
    """GE2ELoss.forward (speech_embedder_net.py:43-49, utils.py:16-55) and its gradient w.r.t. embeddings, w, b."""

    @staticmethod
    def forward(ctx, emb, w, b):
        e = _c(emb)
        N, M, D = e.shape
        w1, b1 = _c(w.reshape(1)), _c(b.reshape(1))
        loss = torch.empty((1,), dtype=torch.float32, device=e.device)
        per = torch.empty((N, M), dtype=torch.float32, device=e.device)
        nb = _lib.query("ssv_ge2e_loss_fwd_workspace", N, M, D)
        ws = _ws(nb, e.device)
        _lib.call("ssv_ge2e_loss_fwd", _p(e), _p(w1), _p(b1), _p(loss), _p(per), N, M, D, _p(ws), nb, _stream())
        ctx.save_for_backward(e, w1, b1)
        ctx.mark_non_differentiable(per)
        return loss[0], per

    @staticmethod
    def backward(ctx, dloss, _dper):
        e, w1, b1 = ctx.saved_tensors
        N, M, D = e.shape
        demb = torch.empty_like(e)
        dw = torch.empty((1,), dtype=torch.float32, device=e.device)
        db = torch.empty((1,), dtype=torch.float32, device=e.device)
        g = _c(dloss.reshape(1).float())
        nb = _lib.query("ssv_ge2e_loss_bwd_workspace", N, M, D)
        ws = _ws(nb, e.device)
        _lib.call("ssv_ge2e_loss_bwd", _p(e), _p(w1), _p(b1), _p(g), _p(demb), _p(dw), _p(db), N, M, D, _p(ws), nb, _stream())
        return demb, dw.reshape(()), db.reshape(())


class GE2ELoss(nn.Module):
    def __init__(self, device):
        super().__init__()
        self.w = nn.Parameter(torch.tensor(10.0).to(device), requires_grad=True)
        self.b = nn.Parameter(torch.tensor(-5.0).to(device), requires_grad=True)
        self.device = device

    def forward(self, embeddings, return_per_embedding=False):
        _dev(embeddings, "embeddings")
        loss, per = _GE2ELossFn.apply(embeddings.float(), self.w, self.b)
        return (loss, per) if return_per_embedding else loss


def train_iteration(embedder_net, ge2e_loss, optimizer, mel_db_batch, N, M):
    """One iteration of GE2E/train_speech_embedder.py:70-86 (the batch permutation of :67-73 is undone at :78 before the
    loss and does not enter the arithmetic, so it is omitted): forward, loss, backward on the HIP path, then torch's own
    ``clip_grad_norm_`` (3.0 on the embedder, 1.0 on the loss parameters) and the optimizer step, as the reference does."""
    optimizer.zero_grad()
    x = mel_db_batch.reshape(N * M, mel_db_batch.size(-2), mel_db_batch.size(-1))
    embeddings = embedder_net(x).reshape(N, M, -1)
    loss = ge2e_loss(embeddings)
    loss.backward()
    torch.nn.utils.clip_grad_norm_(embedder_net.parameters(), 3.0)
    torch.nn.utils.clip_grad_norm_(ge2e_loss.parameters(), 1.0)
    optimizer.step()
    return loss.detach()


# --------------------------------------------------------------------------------------------- the iteration on a resident corpus
def tisv_batch_gather(corpus, rows, out):
    """``out[b, t, f] = corpus[rows[b], f, t]``: the batch of GE2E/data_load.py:77-85 (``utters[utter_index]``, transposed) from a corpus
    (U_total, nmels, frames) held on the device, for the int32 device table ``rows`` of global utterance rows (repeats allowed), into
    ``out`` (len(rows), frames, nmels).  The table is not checked here: the host that drew it validates it before the upload."""
    _dev(corpus, "corpus"), _dev(rows, "row table"), _dev(out, "batch")
    U, nmels, frames = corpus.shape
    if not (corpus.dtype == out.dtype == torch.float32 and rows.dtype == torch.int32 and corpus.is_contiguous() and rows.is_contiguous()
            and out.is_contiguous() and tuple(out.shape) == (rows.numel(), frames, nmels)):
        raise RuntimeError("tisv_batch_gather: need a dense float32 corpus (U, nmels, frames), a dense int32 row table (Bn,) and a dense "
                           "float32 output (Bn, frames, nmels); got %s, %s, %s" % (tuple(corpus.shape), tuple(rows.shape), tuple(out.shape)))
    _lib.call("ssv_tisv_batch_gather", _p(corpus), U, _p(rows), _p(out), rows.numel(), nmels, frames, _stream())
    return out


_SGD_PIECE = 16384


class ClipSGD:
    """``clip_grad_norm_`` per parameter group and the plain ``optim.SGD`` step (GE2E/train_speech_embedder.py:84-86) for every parameter
    in two launches (``ssv_clip_sgd_multi``).  ``groups``: ``[(params, max_norm), ...]``, at most 8.  ``step(loss=None)`` reads the
    parameters' ``.grad`` (whoever wrote them: autograd, or buffers bound by hand), updates the parameters and leaves each group's norm
    before clipping in ``norms`` (device floats; what ``clip_grad_norm_`` returns).  The gradients are NOT rescaled in memory.  With a
    device scalar ``loss`` the call also stores it in slot ``steps % hist_len`` of ``loss_hist`` and advances the device counter
    ``step_dev``, so a replayed hipGraph keeps the last ``hist_len`` losses without a read-back per iteration (``losses(n)``).

    The update does not bump the parameters' version counters: a ``SpeechEmbedder`` that has been stepped needs ``invalidate()``."""

    def __init__(self, groups, lr, hist_len=1024):
        self.groups = [([p for p in params], float(mn)) for params, mn in groups]
        if not 1 <= len(self.groups) <= 8:
            raise ValueError("ClipSGD: 1 to 8 groups, got %d" % len(self.groups))
        if hist_len < 1:
            raise ValueError("ClipSGD: hist_len must be positive")
        self.lr, self.hist_len = float(lr), int(hist_len)
        self._max_norm = (ctypes.c_float * len(self.groups))(*[mn for _, mn in self.groups])
        self._key = None
        self._table = None
        self._flip = 0

    def _alloc(self, device):
        assert ctypes.sizeof(_lib.ClipSgdChunk) == 32
        cap = sum((p.numel() + _SGD_PIECE - 1) // _SGD_PIECE for params, _ in self.groups for p in params)
        # Two pinned tables used alternately with an event after each copy, as FusedAdam keeps them: a rebuild (gradient addresses move
        # between eager iterations of the autograd path) must not overwrite a pinned table whose asynchronous copy has not run yet.
        self._host = [torch.empty((cap, 4), dtype=torch.int64).pin_memory() for _ in range(2)]
        self._copied = [None, None]
        self._table = torch.empty((cap, 4), dtype=torch.int64, device=device)
        self._nb = _lib.query("ssv_clip_sgd_workspace", cap)
        self._ws = _ws(self._nb, device)
        self.norms = torch.zeros((len(self.groups),), dtype=torch.float32, device=device)
        self.loss_hist = torch.zeros((self.hist_len,), dtype=torch.float32, device=device)
        self.step_dev = torch.zeros((1,), dtype=torch.int32, device=device)

    def _rows(self, live):
        rows = []
        for gi, p in live:
            g = p.grad
            if not (p.is_contiguous() and g.is_contiguous() and p.dtype == torch.float32 and g.dtype == torch.float32 and g.numel() == p.numel()):
                raise RuntimeError("ClipSGD needs dense float32 parameters and gradients")
            n = p.numel()
            for off in range(0, n, _SGD_PIECE):
                rows.append((p.data_ptr() + 4 * off, g.data_ptr() + 4 * off, min(_SGD_PIECE, n - off), gi))      # (group in the low half, pad_ = 0)
        return torch.from_numpy(np.array(rows, dtype=np.int64))

    def _build(self, live):
        """(device table, pieces) of this call's parameters and gradients."""
        key = tuple((p.data_ptr(), p.grad.data_ptr()) for _, p in live)
        if torch.cuda.is_current_stream_capturing() and key != self._key:
            # (a captured step keeps its gradients in static buffers, GE2ETrainStep's way: the table of the warm-up's last call is the capture's)
            raise RuntimeError("ClipSGD under capture: parameters or gradients are not those of the last eager call; bind static gradient buffers and warm up first")
        if key != self._key:
            arr = self._rows(live)
            self._flip ^= 1
            host, ev = self._host[self._flip], self._copied[self._flip]
            if ev is not None:
                ev.synchronize()
            host[:len(arr)].copy_(arr)
            self._table.copy_(host, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._copied[self._flip] = ev
            self._nchunks = len(arr)
            self._key = key
        return self._table, self._nchunks

    @torch.no_grad()
    def step(self, loss=None):
        live = [(gi, p) for gi, (params, _) in enumerate(self.groups) for p in params if p.grad is not None]
        if not live:
            return
        _dev(live[0][1], "parameter")
        if self._table is None:
            self._alloc(live[0][1].device)
        table, nchunks = self._build(live)
        if loss is not None:
            _dev(loss, "loss")
            if loss.dtype != torch.float32 or loss.numel() != 1:
                raise RuntimeError("ClipSGD.step: loss must be one float32 device scalar")
        _lib.call("ssv_clip_sgd_multi", _p(table), nchunks, self._max_norm, len(self.groups), self.lr, _p(self.norms),
                  _p(loss), _p(self.loss_hist) if loss is not None else None, self.hist_len, _p(self.step_dev), _p(self._ws), self._nb, _stream())

    @property
    def steps(self):
        """Calls so far (reads the device counter: a synchronisation)."""
        return 0 if self._table is None else int(self.step_dev.item())

    def losses(self, n):
        """The losses of the last ``n`` calls, oldest first (one read-back)."""
        if n == 0:
            return []
        steps = self.steps
        if not 0 < n <= min(steps, self.hist_len):
            raise ValueError("ClipSGD.losses(%d): %d steps taken, the history keeps %d" % (n, steps, self.hist_len))
        hist = self.loss_hist.cpu()
        return [float(hist[(steps - n + i) % self.hist_len]) for i in range(n)]


class GE2ETrainStep:
    """One iteration of GE2E/train_speech_embedder.py:65-86 on static device buffers, nothing of it on the host: the batch gathered from a
    corpus held on the device (``corpus``: a float32 device tensor (U_total, nmels, frames), or an object with ``data`` holding one, such
    as ``ge2e_harness.ResidentSpeakerCorpus``), the embedder's forward keeping every frame, the loss, the backward and ``ClipSGD`` (3.0 on
    the embedder, 1.0 on the loss's w and b).  Forward and backward are the C-ABI calls of ``_EmbedderFn`` and ``_GE2ELossFn``, in
    autograd's order, on buffers allocated once: activations, workspaces and one gradient buffer per parameter, bound as its ``.grad`` -- the
    same kernels on the same values, so the gradients are bitwise ``train_iteration``'s, and nothing is allocated per iteration.
    ``graph=True``: ``prepare()`` warms up, captures the iteration into one hipGraph (``train.PhasedStep``, one phase, one stream, a plain
    chain of launches) and undoes the warm-up's training (``train.TrainingSnapshot``, and the loss-history counter); ``run(rows)`` then
    uploads the (N*M,) int32 row table and replays.  ``graph=False`` makes the same calls eagerly.  ``losses(n)`` reads the last n losses
    back.  The buffers are sized for the arithmetic mode (``ssv_set_precision``) in force at construction; running in another raises."""

    def __init__(self, net, ge2e_loss, N, M, frames, lr, graph=True, corpus=None, hist_len=1024):
        from .train import PhasedStep
        data = getattr(corpus, "data", corpus)
        if data is None:
            raise ValueError("GE2ETrainStep: corpus (the resident (U_total, nmels, frames) tensor, or its holder) is required")
        _dev(data, "corpus")
        F, H, layers, P = net.dims
        if data.dim() != 3 or data.shape[1] != F or data.shape[2] != frames:
            raise ValueError("GE2ETrainStep: corpus is %s, expected (U_total, %d, %d)" % (tuple(data.shape), F, frames))
        if M < 2:
            raise ValueError("GE2ETrainStep: the GE2E loss needs M >= 2 utterances per speaker")
        self.net, self.ge2e_loss, self.N, self.M, self.frames, self.corpus = net, ge2e_loss, int(N), int(M), int(frames), data
        Bn, T, dev = self.N * self.M, self.frames, data.device
        lstm = net.LSTM_stack
        self._w = [[getattr(lstm, "%s_l%d" % (kind, l)) for l in range(layers)] for kind in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        self._pw, self._pb = net.projection.weight, net.projection.bias
        params = [p for kind in self._w for p in kind] + [self._pw, self._pb, ge2e_loss.w, ge2e_loss.b]
        for p in params:
            _dev(p, "parameter")
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("GE2ETrainStep needs dense float32 parameters")

        def f32(*shape):
            return torch.empty(shape, dtype=torch.float32, device=dev)
        self.rows = torch.zeros((Bn,), dtype=torch.int32, device=dev)
        self.x = f32(Bn, T, F)
        self._mode = _lib.precision()
        q = _lib.query
        self._dims = (Bn, T, F, H, layers)
        self._h_last, self._e, self._enorm = f32(Bn, H), f32(Bn, P), f32(Bn)
        self._saved = _ws(q("ssv_lstm_saved_bytes", *self._dims), dev)
        self._loss1, self._per, self._one = f32(1), f32(self.N, self.M), torch.ones((1,), dtype=torch.float32, device=dev)
        self._demb, self._dh, self._dw1, self._db1 = f32(Bn, P), f32(Bn, H), f32(1), f32(1)
        self._wsn = [q("ssv_lstm_train_fwd_workspace", *self._dims), q("ssv_proj_l2norm_fwd_workspace", Bn, P), q("ssv_ge2e_loss_fwd_workspace", self.N, self.M, P),
                     q("ssv_ge2e_loss_bwd_workspace", self.N, self.M, P), q("ssv_proj_l2norm_bwd_workspace", Bn, P), q("ssv_lstm_bwd_workspace", *self._dims)]
        self._wss = [_ws(nb, dev) for nb in self._wsn]
        # one gradient buffer per parameter, bound as its .grad (the loss's w and b are 0-dim: views of one-element buffers)
        self._g = [[torch.empty_like(p) for p in kind] for kind in self._w]
        self._dpw, self._dpb = torch.empty_like(self._pw), torch.empty_like(self._pb)
        for kind, grads in zip(self._w, self._g):
            for p, g in zip(kind, grads):
                p.grad = g
        self._pw.grad, self._pb.grad = self._dpw, self._dpb
        ge2e_loss.w.grad, ge2e_loss.b.grad = self._dw1.reshape(()), self._db1.reshape(())
        self._ptrs = [_ptr_array(kind) for kind in self._w] + [_ptr_array(grads) for grads in self._g]
        # two pinned staging slots and an event after each copy: the host must not overwrite a table that a copy in flight still reads
        self._rows_host = [torch.empty((Bn,), dtype=torch.int32).pin_memory() for _ in range(2)]
        self._rows_copied = [None, None]
        self._flip = 0
        self.sgd = ClipSGD([(list(net.parameters()), 3.0), (list(ge2e_loss.parameters()), 1.0)], lr, hist_len)
        self.loss = self._loss1[0]
        self.stepper = PhasedStep([("graph", self._iteration)], graph=graph)

    def _iteration(self):
        if _lib.precision() != self._mode:
            raise RuntimeError("GE2ETrainStep: built for arithmetic mode %d, now %d (build a new step after ssv_set_precision)" % (self._mode, _lib.precision()))
        Bn, T, F, H, layers = self._dims
        N, M, P = self.N, self.M, self._e.shape[1]
        w_ih, w_hh, b_ih, b_hh, dw_ih, dw_hh, db_ih, db_hh = self._ptrs
        ws, nb, st = self._wss, self._wsn, _stream()
        w1, b1 = self.ge2e_loss.w.detach().reshape(1), self.ge2e_loss.b.detach().reshape(1)
        tisv_batch_gather(self.corpus, self.rows, self.x)
        # _EmbedderFn.forward (training), _GE2ELossFn.forward
        _lib.call("ssv_lstm_train_fwd", _p(self.x), w_ih, w_hh, b_ih, b_hh, _p(self._h_last), _p(self._saved), Bn, T, F, H, layers, _p(ws[0]), nb[0], st)
        _lib.call("ssv_proj_l2norm_fwd", _p(self._h_last), _p(self._pw), _p(self._pb), _p(self._e), _p(self._enorm), Bn, H, P, _p(ws[1]), nb[1], st)
        _lib.call("ssv_ge2e_loss_fwd", _p(self._e), _p(w1), _p(b1), _p(self._loss1), _p(self._per), N, M, P, _p(ws[2]), nb[2], st)
        # loss.backward(): _GE2ELossFn.backward (seed 1.0), _EmbedderFn.backward
        _lib.call("ssv_ge2e_loss_bwd", _p(self._e), _p(w1), _p(b1), _p(self._one), _p(self._demb), _p(self._dw1), _p(self._db1), N, M, P, _p(ws[3]), nb[3], st)
        _lib.call("ssv_proj_l2norm_bwd", _p(self._demb), _p(self._e), _p(self._enorm), _p(self._h_last), _p(self._pw), _p(self._dh), _p(self._dpw), _p(self._dpb),
                  Bn, H, P, _p(ws[4]), nb[4], st)
        _lib.call("ssv_lstm_bwd", _p(self._dh), _p(self._saved), w_ih, w_hh, dw_ih, dw_hh, db_ih, db_hh, Bn, T, F, H, layers, _p(ws[5]), nb[5], st)
        self.sgd.step(self.loss)
        self.net.invalidate()                   # the kernels moved the weights behind the version counters (_FWD_CACHE's key)

    def prepare(self):
        """Warm up and capture (``graph=True``; one-shot): afterwards every parameter is what it was before and no loss is in the history."""
        from .train import TrainingSnapshot
        if not self.stepper.use_graph or self.stepper.plan is not None:
            return self
        snap = TrainingSnapshot([self.net, self.ge2e_loss], []).take()
        self.stepper.prepare()
        snap.restore()
        self.sgd.step_dev.zero_()               # the warm-up's iterations are not part of the history
        self.sgd.loss_hist.zero_()
        self.net.invalidate()
        torch.cuda.synchronize()
        return self

    def release(self):
        self.stepper.release()
        return self

    def load(self, rows_host):
        """Put the (N*M,) row table (host integers, validated here against the corpus) into the static device buffer."""
        rows = torch.as_tensor(rows_host).reshape(-1)
        if rows.numel() != self.rows.numel() or rows.is_floating_point():
            raise ValueError("GE2ETrainStep: the row table must hold N*M = %d integers, got %s %s" % (self.rows.numel(), rows.dtype, tuple(rows.shape)))
        if int(rows.min()) < 0 or int(rows.max()) >= self.corpus.shape[0]:
            raise ValueError("GE2ETrainStep: row table entries must lie in [0, %d), got [%d, %d]" % (self.corpus.shape[0], int(rows.min()), int(rows.max())))
        self._flip ^= 1
        host, ev = self._rows_host[self._flip], self._rows_copied[self._flip]
        if ev is not None:
            ev.synchronize()
        host.copy_(rows)
        self.rows.copy_(host, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._rows_copied[self._flip] = ev

    def run(self, rows_host=None):
        """One iteration on ``rows_host`` (None: on the table already in the device buffer).  Returns the loss as a device scalar, valid
        until the next iteration."""
        if rows_host is not None:
            self.load(rows_host)
        self.stepper.run()
        self.net.invalidate()
        return self.loss

    @property
    def norms(self):
        return self.sgd.norms

    def losses(self, n):
        return self.sgd.losses(n)


# --------------------------------------------------------------------------------------------- multi-GPU
# The embedder shards by utterance; the loss needs every embedding of a speaker and every centroid, so there is exactly one
# exchange: an all-gather of the (N_local*M, P) embeddings -- 113 KB per rank at 880 utterances over 8 ranks.  Every rank then
# evaluates the same full loss, so the gradient of a rank's own embeddings is its slice of d(loss)/d(embeddings) (no second
# collective for the activations); the embedder's weight gradients are partial sums over the local utterances and are summed
# over ranks, the loss parameters' gradients are already complete on every rank.
class _GatherEmbeddings(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e, group):
        import torch.distributed as dist
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        e = e.contiguous()
        parts = [torch.empty_like(e) for _ in range(world)]
        dist.all_gather(parts, e, group=group)
        ctx.rank, ctx.n = rank, e.shape[0]
        return torch.cat(parts, 0)

    @staticmethod
    def backward(ctx, g):
        return g[ctx.rank * ctx.n:(ctx.rank + 1) * ctx.n].contiguous(), None


def gather_embeddings(e, group=None):
    """All ranks' embeddings in rank order (differentiable); the identity without an initialised process group."""
    import torch.distributed as dist
    if not dist.is_available() or not dist.is_initialized() or dist.get_world_size(group) == 1:
        return e
    return _GatherEmbeddings.apply(e, group)


def sharded_train_iteration(embedder_net, ge2e_loss, optimizer, mel_db_local, N_local, M, group=None):
    """``train_iteration`` with the N speakers of the batch split over the ranks of ``group`` (rank r holds speakers
    [r*N_local, (r+1)*N_local), each with its M utterances): local embedder forward, one all-gather of the embeddings, the
    full loss on every rank, backward, one SUM all-reduce of the embedder's gradients, then the reference's clipping and
    optimizer step -- every rank ends with the weights the single-process iteration on the whole batch produces."""
    import torch.distributed as dist
    optimizer.zero_grad()
    x = mel_db_local.reshape(N_local * M, mel_db_local.size(-2), mel_db_local.size(-1))
    e_all = gather_embeddings(embedder_net(x), group)
    loss = ge2e_loss(e_all.reshape(-1, M, e_all.shape[-1]))
    loss.backward()
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        grads = [p.grad for p in embedder_net.parameters() if p.grad is not None]
        flat = torch.cat([g.reshape(-1) for g in grads])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
        off = 0
        for g in grads:
            g.copy_(flat[off:off + g.numel()].view_as(g))
            off += g.numel()
    torch.nn.utils.clip_grad_norm_(embedder_net.parameters(), 3.0)
    torch.nn.utils.clip_grad_norm_(ge2e_loss.parameters(), 1.0)
    optimizer.step()
    return loss.detach()
