"""Host-side mirror of the reference's GE2E speaker embedder (``GE2E/speech_embedder_net.py``).

``SpeechEmbedder().forward(x)``: (B, frames, n_mels) -> (B, proj) unit-norm d-vectors
(speech_embedder_net.py:27-33); ``GE2ELoss(device).forward(emb)``: (N, M, D) -> scalar loss
(:43-49 with GE2E/utils.py:16-55).  The LSTM stack, the projection and the loss run in libssv_hip.so, forward (what
BASELINE.json's north_star asks) and backward (one iteration of GE2E/train_speech_embedder.py:70-86
through ``train_iteration``, which ends in torch's own clip_grad_norm_ and SGD; ``GE2ETrainStep``, the iteration on a corpus held
on the device, runs those too in libssv_hip.so: ``ClipSGD``, and ``tisv_batch_gather`` for the batch).  The verification test around the
embedder (GE2E/train_speech_embedder.py:112-322: trial scores, threshold sweep, spoof rate) has device operators too -- ``sv_trial_scores``,
``sv_eer_sweep``, ``sv_accept_rate`` -- and ``SvEvalStep`` runs a batch of it on a resident corpus; ``sv_score_curve`` and
``score_list_curve`` count for the curves of curve.py (thousands of thresholds, one pass over the scores).  State-dict keys equal the
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
from .train import PhasedStep, StagedUpload, TrainingSnapshot


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

    def _alloc(self, device):
        assert ctypes.sizeof(_lib.ClipSgdChunk) == 32
        cap = sum((p.numel() + _SGD_PIECE - 1) // _SGD_PIECE for params, _ in self.groups for p in params)
        # (a rebuild refills the table: gradient addresses move between eager iterations of the autograd path)
        self._table = torch.empty((cap, 4), dtype=torch.int64, device=device)
        self._upload = StagedUpload(self._table)
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
            self._upload.host()[:len(arr)].copy_(arr)
            self._upload.send()
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


# What the steps on a resident corpus share (GE2ETrainStep, SvEvalStep; ``step``: the caller's name, for the messages).
def _resident_data(corpus, step):
    """The corpus tensor of ``corpus`` (the tensor itself, or an object with ``data`` holding it), on the device."""
    data = getattr(corpus, "data", corpus)
    if data is None:
        raise ValueError("%s: corpus (the resident (U_total, nmels, frames) tensor, or its holder) is required" % step)
    return _dev(data, "corpus")


def _lstm_weights(net, others, step):
    """The embedder's LSTM weights as lists per kind (w_ih, w_hh, b_ih, b_hh), layer by layer, and their pointer arrays -- built once: the
    weights stay where they are -- after checking that they, the projection's and ``others`` are dense float32 device parameters."""
    w = [[getattr(net.LSTM_stack, "%s_l%d" % (kind, l)) for l in range(net.dims[2])] for kind in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    for p in [p for kind in w for p in kind] + [net.projection.weight, net.projection.bias] + list(others):
        _dev(p, "parameter")
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise RuntimeError("%s needs dense float32 parameters" % step)
    return w, [_ptr_array(kind) for kind in w]


def _row_table(rows_host, n, n_corpus, step):
    """The (N*M,) row table ``rows_host`` (host integers) as a flat tensor, validated against a corpus of ``n_corpus`` rows."""
    rows = torch.as_tensor(rows_host).reshape(-1)
    if rows.numel() != n or rows.is_floating_point():
        raise ValueError("%s: the row table must hold N*M = %d integers, got %s %s" % (step, n, rows.dtype, tuple(rows.shape)))
    if int(rows.min()) < 0 or int(rows.max()) >= n_corpus:
        raise ValueError("%s: row table entries must lie in [0, %d), got [%d, %d]" % (step, n_corpus, int(rows.min()), int(rows.max())))
    return rows


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
        data = _resident_data(corpus, "GE2ETrainStep")
        F, H, layers, P = net.dims
        if data.dim() != 3 or data.shape[1] != F or data.shape[2] != frames:
            raise ValueError("GE2ETrainStep: corpus is %s, expected (U_total, %d, %d)" % (tuple(data.shape), F, frames))
        if M < 2:
            raise ValueError("GE2ETrainStep: the GE2E loss needs M >= 2 utterances per speaker")
        self.net, self.ge2e_loss, self.N, self.M, self.frames, self.corpus = net, ge2e_loss, int(N), int(M), int(frames), data
        Bn, T, dev = self.N * self.M, self.frames, data.device
        self._w, w_ptrs = _lstm_weights(net, [ge2e_loss.w, ge2e_loss.b], "GE2ETrainStep")
        self._pw, self._pb = net.projection.weight, net.projection.bias

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
        self._ptrs = w_ptrs + [_ptr_array(grads) for grads in self._g]
        self._rows_upload = StagedUpload(self.rows)
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
        if not self.stepper.use_graph or self.stepper.plan is not None:
            return self
        with TrainingSnapshot([self.net, self.ge2e_loss], []):
            self.stepper.prepare()
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
        rows = _row_table(rows_host, self.rows.numel(), self.corpus.shape[0], "GE2ETrainStep")
        self._rows_upload.host().copy_(rows)
        self._rows_upload.send()

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


# --------------------------------------------------------------------------------------------- the verification test on the device
SV_NTHR = 50
_SV_THR = {}


def _sv_thresholds(device):
    """The sweep's 50 thresholds as ``ge2e_harness.eer_sweep`` builds them for a float32 matrix (the same bits), uploaded once per device."""
    t = _SV_THR.get(device)
    if t is None:
        t = _SV_THR[device] = torch.tensor([0.01 * i + 0.5 for i in range(SV_NTHR)], dtype=torch.float32).to(device)
    return t


def sv_sweep_constants(size_1, es1, spoof=True):
    """(head, tail, den, pos, hden, hpos) of ``ge2e_harness.eer_sweep``: the host-side divisions of train_speech_embedder.py:174-194 /
    :264-284, float and integer where the reference has them."""
    hden, hpos = float(size_1 / 2 - es1 / 2), size_1 // 2 - es1 // 2
    if spoof:
        half = (size_1 - es1) // 2
        return half, half, float(size_1 - es1), size_1 - es1, hden, hpos
    return 0, 0, hden, hpos, hden, hpos


def sv_eval_shapes(N, M, enroll_num, eval_num=None):
    """(es1, V, V2) of the verification test on batches of N speakers x M utterances: 2*enroll_num enrolment rows, V = M - es1 verification
    rows, V2 = 2*eval_num of them in the no-spoof test (None without ``eval_num``).  Raises a ``ValueError`` for what the reference asserts
    (:141, M even) or fails on later: fewer than two speakers (FAR divides by N - 1), no verification half left."""
    N, M, enroll_num = int(N), int(M), int(enroll_num)
    if N < 2:
        raise ValueError("verification test: N = %d, needs at least 2 speakers per batch (FAR divides by N - 1)" % N)
    if M % 2 != 0:
        raise ValueError("verification test: M = %d must be even (train_speech_embedder.py:141)" % M)
    if enroll_num < 1 or 2 * enroll_num >= M:
        raise ValueError("verification test: 2 * enroll_num = %d enrolment rows of M = %d leave nothing to verify" % (2 * enroll_num, M))
    es1 = 2 * enroll_num
    V = M - es1
    if V < 2:
        raise ValueError("verification test: M - 2 * enroll_num = %d verification rows, the own-speaker score needs 2" % V)
    V2 = None
    if eval_num is not None:
        V2 = 2 * int(eval_num)
        if not 2 <= V2 <= V:
            raise ValueError("verification test: 2 * eval_num = %d must lie in [2, M - 2 * enroll_num = %d]" % (V2, V))
    return es1, V, V2


def _sv_row(row, spoof):
    best = int(row[1])
    out = dict(EER=float(row[0]), thres=0.01 * best + 0.5, FAR=float(row[2]), FRR=float(row[3]))
    if spoof:
        out["gt_FRR"], out["spoof_rate"] = float(row[4]), float(row[5])
    return out


def sv_trial_scores(e_enr, e_ver, V=None, out=None, cent=None):
    """``ge2e_harness.cossim_eval(e_ver[:, :V], e_enr.mean(1))`` in one launch (``ssv_sv_trial_scores``): e_enr (N, E, D), e_ver (N, Vs, D)
    float32 on the device, V (default Vs) rows of every speaker in use -> (N, V, N).  ``out`` / ``cent``: where to write the matrix and the
    (N, D) centroids (dense float32; the matrix is allocated when absent, the centroids are not kept)."""
    e_enr, e_ver = _c(e_enr), _c(e_ver)
    if e_enr.dim() != 3 or e_ver.dim() != 3 or e_enr.shape[0] != e_ver.shape[0] or e_enr.shape[2] != e_ver.shape[2]:
        raise RuntimeError("sv_trial_scores: need enrolment (N, E, D) and verification (N, V, D) embeddings, got %s and %s" % (tuple(e_enr.shape), tuple(e_ver.shape)))
    N, E, D = e_enr.shape
    Vs = e_ver.shape[1]
    V = Vs if V is None else int(V)
    if out is None:
        out = torch.empty((N, max(V, 0), N), dtype=torch.float32, device=e_ver.device)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (N, V, N)):
        raise RuntimeError("sv_trial_scores: out must be a dense float32 device tensor (%d, %d, %d)" % (N, V, N))
    if cent is not None and not (cent.is_cuda and cent.dtype == torch.float32 and cent.is_contiguous() and tuple(cent.shape) == (N, D)):
        raise RuntimeError("sv_trial_scores: cent must be a dense float32 device tensor (%d, %d)" % (N, D))
    _lib.call("ssv_sv_trial_scores", _p(e_enr), _p(e_ver), _p(out), _p(cent), N, E, V, Vs, D, _stream())
    return out


def _sv_sweep_call(sim, consts, counts, hist, hist_len, step_dev):
    N, V = sim.shape[0], sim.shape[1]
    head, tail, den, pos, hden, hpos = consts
    _lib.call("ssv_sv_eer_sweep", _p(sim), N, V, _p(_sv_thresholds(sim.device)), SV_NTHR, head, tail, den, float(pos), hden, float(hpos),
              _p(counts), _p(hist), hist_len, _p(step_dev), _stream())


def sv_eer_sweep(sim, size_1, es1, spoof=True, return_counts=False):
    """``ge2e_harness.eer_sweep`` on the device (``ssv_sv_eer_sweep``): the same dict (Python floats; ``thres`` = 0.01 * index + 0.5), one
    read-back.  ``return_counts``: also the (50, 4) int32 table of accepted trials (all, own column, its head rows, its tail rows)."""
    _dev(sim, "similarity matrix")
    if sim.dim() != 3 or sim.shape[0] != sim.shape[2] or sim.dtype != torch.float32:
        raise RuntimeError("sv_eer_sweep: need a float32 similarity matrix (N, V, N), got %s %s" % (sim.dtype, tuple(sim.shape)))
    sim = sim.contiguous()
    counts = torch.zeros((SV_NTHR, 4), dtype=torch.int32, device=sim.device)
    hist = torch.zeros((1, 6), dtype=torch.float64, device=sim.device)
    step_dev = torch.zeros((1,), dtype=torch.int32, device=sim.device)
    _sv_sweep_call(sim, sv_sweep_constants(size_1, es1, spoof), counts, hist, 1, step_dev)
    out = _sv_row(hist.cpu()[0], spoof)
    return (out, counts) if return_counts else out


def sv_accept_rate(sim_stack, thres, eval_num):
    """The body of ``ge2e_harness.spoof_rate_at`` over a device stack (nmat, N, V, N) of similarity matrices (``ssv_sv_accept_rate``): per
    matrix the fraction of own-speaker trials in the last 2*eval_num rows above ``thres``, as Python floats (one read-back)."""
    _dev(sim_stack, "similarity stack")
    if sim_stack.dim() != 4 or sim_stack.shape[1] != sim_stack.shape[3] or sim_stack.dtype != torch.float32:
        raise RuntimeError("sv_accept_rate: need a float32 stack (nmat, N, V, N), got %s %s" % (sim_stack.dtype, tuple(sim_stack.shape)))
    sim_stack = sim_stack.contiguous()
    nmat, N, V, _ = sim_stack.shape
    rates = torch.empty((max(nmat, 1),), dtype=torch.float32, device=sim_stack.device)
    _lib.call("ssv_sv_accept_rate", _p(sim_stack), nmat, N, V, 2 * int(eval_num), float(thres), _p(rates), _stream())
    return [float(r) for r in rates.cpu()]


def _curve_thresholds(thresholds, dtype, what):
    """A host sequence of thresholds -> numpy array in the scores' type.  Checked here, in that type and before anything touches the device,
    because the kernel does not: non-decreasing (duplicates pass) and no NaN."""
    t = np.asarray(thresholds, dtype=np.float64).astype(np.float32 if dtype == torch.float32 else np.float64)
    if t.ndim != 1 or t.size < 1:
        raise ValueError("%s: need a non-empty one-dimensional sequence of thresholds, got shape %s" % (what, tuple(t.shape)))
    if np.isnan(t).any() or (t[1:] < t[:-1]).any():
        raise ValueError("%s: the thresholds must be non-decreasing and free of NaN (the kernel searches them)" % what)
    return t


def sv_score_curve(sim_stack, thresholds, head, tail):
    """The counts behind curve.py's GE2E sweep for every matrix of a device stack (nmat, N, V, N) and every threshold of the host sequence
    ``thresholds`` (non-decreasing; compared as their float32 roundings, strictly, as ``sim > thres`` compares a float32 matrix with a Python
    float), in one launch (``ssv_sv_score_curve``): int32 (nmat, K, 4) on the device -- accepted trials of the whole matrix, the own-speaker
    column, its first ``head`` rows, its last ``tail`` rows, the columns of ``sv_eer_sweep(return_counts=True)``.  Nothing is read back."""
    thr = _curve_thresholds(thresholds, torch.float32, "sv_score_curve")
    _dev(sim_stack, "similarity stack")
    if sim_stack.dim() != 4 or sim_stack.shape[1] != sim_stack.shape[3] or sim_stack.dtype != torch.float32:
        raise RuntimeError("sv_score_curve: need a float32 stack (nmat, N, V, N), got %s %s" % (sim_stack.dtype, tuple(sim_stack.shape)))
    thr, K = torch.from_numpy(thr).to(sim_stack.device), int(thr.size)
    sim_stack = sim_stack.contiguous()
    nmat, N, V, _ = sim_stack.shape
    counts = torch.empty((max(nmat, 1), K, 4), dtype=torch.int32, device=sim_stack.device)
    _lib.call("ssv_sv_score_curve", _p(sim_stack), nmat, N, V, int(head), int(tail), _p(thr), K, _p(counts), _stream())
    return counts


def score_list_curve(scores, classes, thresholds, nclass):
    """Per threshold and class the items of a device score vector above the threshold (strict, in the scores' own type): ``scores`` (n,)
    float32 or float64 -- the dtype picks ``ssv_score_list_curve_f32`` / ``_f64`` --, ``classes`` (n,) uint8 codes (an item whose code is
    >= ``nclass`` is counted nowhere), ``thresholds`` a non-decreasing host sequence -> int32 (K, nclass) on the device."""
    thr = _curve_thresholds(thresholds, scores.dtype, "score_list_curve")
    _dev(scores, "scores")
    _dev(classes, "classes")
    if scores.dim() != 1 or scores.dtype not in (torch.float32, torch.float64) or classes.dtype != torch.uint8 or classes.shape != scores.shape:
        raise RuntimeError("score_list_curve: need float32 or float64 scores (n,) and uint8 classes (n,), got %s %s and %s %s"
                           % (scores.dtype, tuple(scores.shape), classes.dtype, tuple(classes.shape)))
    thr, K = torch.from_numpy(thr).to(scores.device), int(thr.size)
    scores, classes = scores.contiguous(), classes.contiguous()
    counts = torch.empty((K, max(int(nclass), 1)), dtype=torch.int32, device=scores.device)
    entry = "ssv_score_list_curve_f32" if scores.dtype == torch.float32 else "ssv_score_list_curve_f64"
    _lib.call(entry, _p(scores), _p(classes), scores.numel(), int(nclass), _p(thr), K, _p(counts), _stream())
    return counts


class SvEvalStep:
    """One batch of the verification test (GE2E/train_speech_embedder.py:131-199, and :225-289 when ``eval_num`` is given) on static device
    buffers: the enrolment and the verification utterances gathered from a corpus held on the device (``corpus`` as for ``GE2ETrainStep``),
    the embedder's inference forward on each -- the host path's two shapes, (N*es1, frames, nmels) and (N*V, frames, nmels), through the
    same two C-ABI calls as ``SpeechEmbedder.forward``, so the embeddings are bitwise ``net(enr)`` / ``net(ver)`` on the same rows -- the
    trial scores and the mixture sweep; with ``eval_num`` also the no-spoof scores (the first 2*eval_num verification rows) and their
    sweep, from the same embeddings.  Each shape keeps its own LSTM workspace for the life of the step: the weights are scanned and split
    once per shape (``invalidate()`` after changing them), not once per call as the two shapes alternating through the module's one-entry
    cache cost; ``SpeechEmbedder.forward`` and that cache are not touched.

    ``graph=True``: ``prepare()`` warms up, captures the batch into one hipGraph (``train.PhasedStep``: one phase, one stream, a plain chain
    of launches) and resets the history; ``run(rows)`` uploads the (N*M,) row table -- speaker after speaker, M rows each, split here into
    the two tables -- replays, and copies the mixture matrix into the next slot of ``stack`` (``stack_len`` slots, device to device).
    ``graph=False`` makes the same calls eagerly.  ``results(n)``: the sweeps' rows of the last n batches in one read-back;
    ``sims(n)``: their mixture matrices, on the device."""

    def __init__(self, net, corpus, N, M, enroll_num, eval_num=None, graph=True, hist_len=1024, stack_len=None):
        self.es1, self.V, self.V2 = sv_eval_shapes(N, M, enroll_num, eval_num)
        data = _resident_data(corpus, "SvEvalStep")
        F, H, layers, P = net.dims
        if data.dim() != 3 or data.shape[1] != F or data.dtype != torch.float32 or not data.is_contiguous():
            raise ValueError("SvEvalStep: corpus is %s %s, expected dense float32 (U_total, %d, frames)" % (data.dtype, tuple(data.shape), F))
        if hist_len < 1 or (stack_len is not None and stack_len < 1):
            raise ValueError("SvEvalStep: hist_len and stack_len must be positive")
        self.net, self.corpus, self.N, self.M, self.eval_num = net, data, int(N), int(M), eval_num
        self.hist_len, self.stack_len = int(hist_len), int(hist_len if stack_len is None else stack_len)
        T, dev, N = int(data.shape[2]), data.device, self.N
        self._w, self._ptrs = _lstm_weights(net, [], "SvEvalStep")
        self._pw, self._pb = net.projection.weight, net.projection.bias
        self._mode = _lib.precision()

        def f32(*shape):
            return torch.empty(shape, dtype=torch.float32, device=dev)
        q = _lib.query
        # the two sides of the batch: (row table, gathered batch, h_last, embeddings, LSTM dims, LSTM workspace, projection workspace)
        # (the row tables are views of ONE (N*M,) device table, enrolment rows first, verification rows after: one upload serves both)
        self._sides = []
        self.rows = torch.zeros((N * self.M,), dtype=torch.int32, device=dev)
        for rows in self.rows.split((N * self.es1, N * self.V)):
            Bn = rows.numel()
            dims = (Bn, T, F, H, layers)
            nb, nb2 = q("ssv_lstm_fwd_workspace", *dims), q("ssv_proj_l2norm_fwd_workspace", Bn, P)
            self._sides.append(dict(rows=rows, x=f32(Bn, T, F), h=f32(Bn, H), e=f32(Bn, P), dims=dims,
                                    ws=_ws(nb, dev), nb=nb, ws2=_ws(nb2, dev), nb2=nb2))
        self._packed = 0                                                # 1 once both workspaces hold the split weight planes
        self.e_enr, self.e_ver = self._sides[0]["e"].view(N, self.es1, P), self._sides[1]["e"].view(N, self.V, P)
        self.sim, self.cent = f32(N, self.V, N), f32(N, P)
        self.sim_nospoof = f32(N, self.V2, N) if self.V2 is not None else None
        self._consts = sv_sweep_constants(self.M, self.es1, True)
        self._consts2 = sv_sweep_constants(self.M, self.es1, False)
        # [0]: the mixture sweep's history, [1]: the no-spoof sweep's -- one tensor, so that results() is one copy
        self.hist = torch.zeros((2, self.hist_len, 6), dtype=torch.float64, device=dev)
        self.counts = torch.zeros((2, SV_NTHR, 4), dtype=torch.int32, device=dev)
        self.step_dev = torch.zeros((2,), dtype=torch.int32, device=dev)
        self.stack = f32(self.stack_len, N, self.V, N)
        self.batches = 0                                                # run() calls since prepare(): the host's copy of step_dev
        _sv_thresholds(dev)                                             # uploaded before any capture
        self._rows_upload = StagedUpload(self.rows)
        self.stepper = PhasedStep([("graph", self._batch)], graph=graph)

    def _batch(self):
        if _lib.precision() != self._mode:
            raise RuntimeError("SvEvalStep: built for arithmetic mode %d, now %d (build a new step after ssv_set_precision)" % (self._mode, _lib.precision()))
        st, P = _stream(), self._pw.shape[0]
        for s in self._sides:
            Bn, T, F, H, layers = s["dims"]
            tisv_batch_gather(self.corpus, s["rows"], s["x"])
            _lib.call("ssv_lstm_fwd_cached", _p(s["x"]), *self._ptrs, _p(s["h"]), Bn, T, F, H, layers, _p(s["ws"]), s["nb"], self._packed, st)
            _lib.call("ssv_proj_l2norm_fwd", _p(s["h"]), _p(self._pw), _p(self._pb), _p(s["e"]), None, Bn, H, P, _p(s["ws2"]), s["nb2"], st)
        self._packed = 1
        sv_trial_scores(self.e_enr, self.e_ver, out=self.sim, cent=self.cent)
        _sv_sweep_call(self.sim, self._consts, self.counts[0], self.hist[0], self.hist_len, self.step_dev[0:1])
        if self.sim_nospoof is not None:
            sv_trial_scores(self.e_enr, self.e_ver, V=self.V2, out=self.sim_nospoof)
            _sv_sweep_call(self.sim_nospoof, self._consts2, self.counts[1], self.hist[1], self.hist_len, self.step_dev[1:2])

    def _reset(self):
        self.step_dev.zero_()
        self.hist.zero_()
        self.batches = 0

    def prepare(self):
        """Warm up and capture (``graph=True``; one-shot).  Afterwards the history is empty and its counters are zero."""
        if not self.stepper.use_graph or self.stepper.plan is not None:
            return self
        self.stepper.prepare()
        self._reset()
        torch.cuda.synchronize()
        return self

    def release(self):
        self.stepper.release()
        return self

    def invalidate(self):
        """The embedder's weights changed: the next (eager) batch scans and splits them again.  A captured step must be released first."""
        if self.stepper.plan is not None:
            raise RuntimeError("SvEvalStep.invalidate: release() the captured batch first; its replay assumes the split weight planes it was captured with")
        self._packed = 0

    def load(self, rows_host):
        """Put the batch's (N*M,) row table (host integers, validated here against the corpus) into the two static device tables."""
        rows = _row_table(rows_host, self.N * self.M, self.corpus.shape[0], "SvEvalStep").reshape(self.N, self.M)
        host, n_enr = self._rows_upload.host(), self.N * self.es1
        host[:n_enr].view(self.N, self.es1).copy_(rows[:, :self.es1])
        host[n_enr:].view(self.N, self.V).copy_(rows[:, self.es1:])
        self._rows_upload.send()

    def run(self, rows_host=None):
        """One batch on ``rows_host`` (None: on the tables already on the device).  Returns the mixture matrix's slot in ``stack``."""
        if rows_host is not None:
            self.load(rows_host)
        self.stepper.run()
        slot = self.stack[self.batches % self.stack_len]
        slot.copy_(self.sim)
        self.batches += 1
        return slot

    def results(self, n):
        """The last ``n`` batches' sweeps, oldest first, in one read-back: a list of ``eer_sweep(spoof=True)`` dicts, each with the
        no-spoof sweep's dict under ``"nospoof"`` when the step has an ``eval_num``."""
        if n == 0:
            return []
        if not 0 < n <= min(self.batches, self.hist_len):
            raise ValueError("SvEvalStep.results(%d): %d batches run, the history keeps %d" % (n, self.batches, self.hist_len))
        hist = self.hist.cpu()
        out = []
        for k in range(self.batches - n, self.batches):
            r = _sv_row(hist[0, k % self.hist_len], True)
            if self.sim_nospoof is not None:
                r["nospoof"] = _sv_row(hist[1, k % self.hist_len], False)
            out.append(r)
        return out

    def sims(self, n=None):
        """The mixture matrices of the last ``n`` batches (default: all since ``prepare()``), oldest first: a device tensor (n, N, V, N)."""
        n = self.batches if n is None else n
        if not 0 < n <= min(self.batches, self.stack_len):
            raise ValueError("SvEvalStep.sims(%s): %d batches run, the stack keeps %d" % (n, self.batches, self.stack_len))
        if self.batches <= self.stack_len:
            return self.stack[self.batches - n:self.batches]
        idx = torch.tensor([k % self.stack_len for k in range(self.batches - n, self.batches)], device=self.stack.device)
        return self.stack.index_select(0, idx)


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
