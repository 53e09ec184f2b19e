"""The front half of the i-vector system on the device: cepstral features, a diagonal-covariance GMM-UBM trained by EM, and the
Baum-Welch statistics (zeroth and first order, per utterance) that i-vector training and extraction start from.

This is the bottom of the reference's ``kaldi_ivectors/run.sh`` (MFCC -> VAD -> diagonal UBM -> full UBM -> extractor -> PLDA), as far
as the diagonal UBM.  Kaldi's binaries are NOT reproduced: its MFCC (povey window, snip-edges, energy in C0), its energy VAD and the
recipe's ``conf/`` values are not pinned here; the algorithms are the ones stated at the entries in ``include/ssv_hip.h``, and a float64
restatement (``tests/_ivector_ref.py``) is the yardstick.  Ours, not Kaldi's: the initialisation of ``DiagUbm.from_frames`` and the
treatment of a starved Gaussian in the M-step.

Every FLOP of the hot path runs in ``csrc/ivector.hip``; torch is plumbing (memory, the stream).  Tensors must live on a ROCm device.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, ops
from .ops import _p

_F32, _F64, _I32, _I64 = torch.float32, torch.float64, torch.int32, torch.int64
MAX_D, MAX_C, MAX_NSEL = 128, 2048, 32
LL_ROW = 4096          # the per-frame log-likelihoods are summed as rows of this many columns (ssv_gmm_stats_reduce), then over the columns


# ------------------------------------------------------------------------------------------------------------ host tables
def dct_table(n_ceps, n_mels, lifter=22):
    """Rows 0 .. n_ceps-1 of the orthonormal DCT-II over ``n_mels`` bins, row k scaled by the cepstral lifter 1 + (Q/2) sin(pi k / Q),
    Q = ``lifter`` (0: none): float32 (n_ceps, n_mels), computed in double and rounded once."""
    n_ceps, n_mels = int(n_ceps), int(n_mels)
    if not 1 <= n_ceps <= n_mels:
        raise ValueError("dct_table: n_ceps=%d must lie in [1, n_mels=%d]" % (n_ceps, n_mels))
    if lifter < 0:
        raise ValueError("dct_table: lifter=%r must be >= 0" % (lifter,))
    k, m = np.arange(n_ceps, dtype=np.float64)[:, None], np.arange(n_mels, dtype=np.float64)[None, :]
    t = np.sqrt(2.0 / n_mels) * np.cos(np.pi * k * (2.0 * m + 1.0) / (2.0 * n_mels))
    t[0] = np.sqrt(1.0 / n_mels)
    if lifter:
        t *= 1.0 + 0.5 * lifter * np.sin(np.pi * k / lifter)
    return t.astype(np.float32)


def _offsets(off, name, device, total=None):
    """An offset table as (int64 device tensor, host int64 array or None).  A host sequence is validated here (ascending, inside
    [0, total]) and travels to the entry as well, which checks it again; a device tensor is taken as it is -- the kernels clamp what
    they read."""
    if isinstance(off, torch.Tensor) and off.is_cuda:
        if off.dtype != _I64 or off.dim() != 1 or off.numel() < 2:
            raise ValueError("%s: need an int64 vector of at least 2 offsets, got %s %s" % (name, off.dtype, tuple(off.shape)))
        return off.contiguous(), None
    if isinstance(off, torch.Tensor):
        off = off.numpy()
    host = np.ascontiguousarray(np.asarray(off, dtype=np.int64))
    if host.ndim != 1 or host.size < 2:
        raise ValueError("%s: need a vector of at least 2 offsets, got shape %s" % (name, host.shape))
    if np.any(np.diff(host) < 0) or host[0] < 0 or (total is not None and host[-1] > total):
        raise ValueError("%s: offsets must ascend inside [0, %s]" % (name, total))
    return torch.from_numpy(host).to(device), host


def _matrix(t, name, dtype=_F32, cols=None):
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s: need a torch tensor, got %s" % (name, type(t).__name__))
    ops._dev(t, name)
    if t.dtype != dtype or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1 or (cols is not None and t.shape[1] != cols):
        raise ValueError("%s: need a %s matrix (rows >= 1, %s columns), got %s %s" % (name, dtype, cols if cols is not None else ">= 1", t.dtype, tuple(t.shape)))
    return t.contiguous()


def cepstral_features(mel, utt_off, n_ceps=20, lifter=22, delta_window=3, delta_order=2, cmn_window=300):
    """``mel`` (G, M) float32, the compact frames-major log-mel array of ``DvectorExtractor.log_mel``; ``utt_off`` (U + 1) offsets, frames
    [utt_off[u], utt_off[u+1]) being utterance u (rows past utt_off[-1] are not written and come back 0).  ``n_ceps`` cepstra (DCT-II +
    lifter; ``n_ceps=None``: the mel frames themselves), deltas of ``delta_order`` with window ``delta_window`` on indices clamped to the
    utterance, then the centred sliding mean over ``cmn_window`` frames subtracted from all columns -- the order of
    ``sid/train_diag_ubm.sh``.  Returns (G, n * (delta_order + 1)) float32.  Defaults: the ``sid`` scripts' options, 60 columns."""
    mel = _matrix(mel, "cepstral_features: mel")
    G, M = mel.shape
    if delta_order not in (0, 1, 2) or (delta_order and delta_window < 1) or cmn_window < 1:
        raise ValueError("cepstral_features: delta_order=%r must be 0, 1 or 2, delta_window=%r and cmn_window=%r positive" % (delta_order, delta_window, cmn_window))
    off, _ = _offsets(utt_off, "cepstral_features: utt_off", mel.device, total=G)
    dct = None if n_ceps is None else torch.from_numpy(dct_table(n_ceps, M, lifter)).to(mel.device)
    Cc = M if dct is None else int(n_ceps)
    out = torch.zeros((G, Cc * (delta_order + 1)), dtype=_F32, device=mel.device)
    nws = _lib.query("ssv_ivec_features_workspace", G, Cc, int(delta_order))
    ws = ops._ws(nws, mel.device)
    _lib.call("ssv_ivec_features", _p(mel), _p(off), _p(dct), _p(out), G, M, off.numel() - 1, Cc, int(delta_window), int(delta_order), int(cmn_window),
              _p(ws), nws, ops._stream())
    return out


# ------------------------------------------------------------------------------------------------------------ the UBM
class DiagUbm:
    """A diagonal-covariance Gaussian mixture on one device: ``w`` (C,), ``mu`` and ``var`` (C, D) as float64 tensors -- the M-step
    runs in double -- and the float32 planes ``A = mu / var``, ``B = -1/2 / var``, ``g`` the kernels read, rounded once from them."""

    def __init__(self, w, mu, var):
        for t, name in ((w, "w"), (mu, "mu"), (var, "var")):
            if not isinstance(t, torch.Tensor):
                raise ValueError("DiagUbm: %s must be a torch tensor" % name)
        if mu.dim() != 2 or var.shape != mu.shape or w.shape != (mu.shape[0],) or any(t.dtype != _F64 for t in (w, mu, var)):
            raise ValueError("DiagUbm: need float64 w (C,), mu (C, D), var (C, D); got %s %s, %s %s, %s %s"
                             % (w.dtype, tuple(w.shape), mu.dtype, tuple(mu.shape), var.dtype, tuple(var.shape)))
        C, D = mu.shape
        if not (1 <= C <= MAX_C and 1 <= D <= MAX_D):
            raise ValueError("DiagUbm: C=%d must lie in [1, %d] and D=%d in [1, %d]" % (C, MAX_C, D, MAX_D))
        if w.device != mu.device or var.device != mu.device:
            raise ValueError("DiagUbm: w, mu and var must live on one device")
        self.w, self.mu, self.var = w.contiguous().clone(), mu.contiguous().clone(), var.contiguous().clone()
        self._planes = None

    def planes(self):
        """The float32 planes (A, B, g) of the current parameters: built on the device at first use (``ssv_gmm_diag_planes``), rewritten
        by every M-step.  The state itself may sit on the host (``load(path, device="cpu")``); every operation needs a ROCm device."""
        if self._planes is None:
            for t, name in ((self.w, "w"), (self.mu, "mu"), (self.var, "var")):
                ops._dev(t, "DiagUbm: " + name)
            C, D, dev = self.C, self.D, self.device
            A, B = torch.empty((C, D), dtype=_F32, device=dev), torch.empty((C, D), dtype=_F32, device=dev)
            g = torch.empty((C,), dtype=_F32, device=dev)
            _lib.call("ssv_gmm_diag_planes", _p(self.w), _p(self.mu), _p(self.var), _p(A), _p(B), _p(g), C, D, ops._stream())
            self._planes = (A, B, g)
        return self._planes

    A = property(lambda self: self.planes()[0])
    B = property(lambda self: self.planes()[1])
    g = property(lambda self: self.planes()[2])
    C = property(lambda self: self.mu.shape[0])
    D = property(lambda self: self.mu.shape[1])
    device = property(lambda self: self.mu.device)

    # ------------------------------------------------------------------ state
    def state_dict(self):
        return {"w": self.w.clone(), "mu": self.mu.clone(), "var": self.var.clone()}

    def load_state_dict(self, sd):
        new = DiagUbm(sd["w"].to(self.device), sd["mu"].to(self.device), sd["var"].to(self.device))
        self.__dict__.update(new.__dict__)
        return self

    def save(self, path):
        """``.npz`` with the float64 ``w``, ``mu``, ``var`` (the planes are derived)."""
        np.savez(path, w=self.w.cpu().numpy(), mu=self.mu.cpu().numpy(), var=self.var.cpu().numpy())

    @classmethod
    def load(cls, path, device="cuda"):
        """``device="cpu"`` gives a state holder only (to inspect or move); the operations need a ROCm device."""
        with np.load(path) as z:
            return cls(*(torch.from_numpy(np.asarray(z[k], dtype=np.float64)).to(device) for k in ("w", "mu", "var")))

    @classmethod
    def from_frames(cls, X, num_gauss, seed=0):
        """The starting point of EM -- OURS, not Kaldi's (``gmm-global-init-from-feats`` clusters): the means are ``num_gauss`` distinct
        frames drawn on the host by ``numpy.random.default_rng(seed)``, every variance is the frames' global variance per dimension
        (float64 on the device), the weights are uniform."""
        X = _matrix(X, "DiagUbm.from_frames: X")
        F, D = X.shape
        num_gauss = int(num_gauss)
        if not 1 <= num_gauss <= min(F, MAX_C):
            raise ValueError("DiagUbm.from_frames: num_gauss=%d must lie in [1, min(frames=%d, %d)]" % (num_gauss, F, MAX_C))
        rows = np.sort(np.random.default_rng(seed).choice(F, size=num_gauss, replace=False))
        mu = X[torch.from_numpy(rows).to(X.device)].double()
        var = X.double().var(dim=0, unbiased=False).clamp_min(1e-10).expand(num_gauss, D).contiguous()
        w = torch.full((num_gauss,), 1.0 / num_gauss, dtype=_F64, device=X.device)
        return cls(w, mu, var)

    # ------------------------------------------------------------------ operations
    def _frames(self, X, who):
        return _matrix(X, who + ": X", cols=self.D)

    def posteriors(self, X, nsel=20, min_post=0.0, loglik_out=None):
        """Per frame the ``nsel`` likeliest Gaussians (descending), their posteriors among themselves (those below ``min_post`` zeroed,
        the rest renormalised) and the log-likelihood over the selected: ``idx`` (F, nsel) int32, ``post`` (F, nsel), ``loglik`` (F,)."""
        X = self._frames(X, "DiagUbm.posteriors")
        nsel = int(nsel)
        if not 1 <= nsel <= min(self.C, MAX_NSEL):
            raise ValueError("DiagUbm.posteriors: nsel=%d must lie in [1, min(C=%d, %d)]" % (nsel, self.C, MAX_NSEL))
        if not 0.0 <= min_post < 1.0:
            raise ValueError("DiagUbm.posteriors: min_post=%r must lie in [0, 1)" % (min_post,))
        F = X.shape[0]
        idx = torch.empty((F, nsel), dtype=_I32, device=X.device)
        post = torch.empty((F, nsel), dtype=_F32, device=X.device)
        ll = loglik_out if loglik_out is not None else torch.empty((F,), dtype=_F32, device=X.device)
        _lib.call("ssv_gmm_diag_gselect", _p(X), _p(self.A), _p(self.B), _p(self.g), _p(idx), _p(post), _p(ll), F, self.D, self.C, nsel, float(min_post),
                  ops._stream())
        return idx, post, ll[:F]

    def stats(self, X, seg_off, order, idx=None, post=None, nsel=20, min_post=0.0):
        """``slab`` (S, C, 1 + order * D) float32: per segment [seg_off[s], seg_off[s+1]) and Gaussian the sums of gamma, gamma x and
        (order 2) gamma x^2.  ``idx`` / ``post``: the sparse posteriors (default: ``self.posteriors(X, nsel, min_post)``)."""
        X = self._frames(X, "DiagUbm.stats")
        F = X.shape[0]
        if order not in (1, 2):
            raise ValueError("DiagUbm.stats: order=%r must be 1 or 2" % (order,))
        off, host = _offsets(seg_off, "DiagUbm.stats: seg_off", X.device, total=F)
        if (idx is None) != (post is None):
            raise ValueError("DiagUbm.stats: idx and post come together")
        if idx is None:
            idx, post, _ = self.posteriors(X, nsel, min_post)
        idx = _matrix(idx, "DiagUbm.stats: idx", dtype=_I32)
        post = _matrix(post, "DiagUbm.stats: post", cols=idx.shape[1])
        if idx.shape[0] != F or post.shape[0] != F or idx.shape[1] > min(self.C, MAX_NSEL):
            raise ValueError("DiagUbm.stats: idx / post must be (%d, nsel <= %d), got %s and %s" % (F, min(self.C, MAX_NSEL), tuple(idx.shape), tuple(post.shape)))
        S = off.numel() - 1
        slab = torch.empty((S, self.C, 1 + order * self.D), dtype=_F32, device=X.device)
        hp = None if host is None else host.ctypes.data_as(ctypes.c_void_p)
        _lib.call("ssv_gmm_diag_stats", _p(X), _p(idx), _p(post), _p(off), hp, _p(slab), F, self.D, self.C, idx.shape[1], S, int(order), ops._stream())
        return slab

    @staticmethod
    def reduce(slab):
        """(S, ...) float32 -> (...) float64: the slabs added in ascending s, in double (``ssv_gmm_stats_reduce``)."""
        ops._dev(slab, "DiagUbm.reduce: slab")
        if slab.dtype != _F32 or slab.dim() < 2 or slab.numel() == 0:
            raise ValueError("DiagUbm.reduce: need a non-empty float32 (S, ...) tensor, got %s %s" % (slab.dtype, tuple(slab.shape)))
        slab = slab.contiguous()
        out = torch.empty(slab.shape[1:], dtype=_F64, device=slab.device)
        _lib.call("ssv_gmm_stats_reduce", _p(slab), _p(out), slab.shape[0], out.numel(), ops._stream())
        return out

    def update(self, stats, var_floor=1e-3, min_count=10.0, min_weight=1e-5):
        """The M-step from (C, 1 + 2 D) float64 statistics, in place (``ssv_gmm_diag_update``)."""
        stats = _matrix(stats, "DiagUbm.update: stats", dtype=_F64, cols=1 + 2 * self.D)
        if stats.shape[0] != self.C:
            raise ValueError("DiagUbm.update: stats must have C=%d rows, got %d" % (self.C, stats.shape[0]))
        _lib.call("ssv_gmm_diag_update", _p(stats), _p(self.w), _p(self.mu), _p(self.var), _p(self.A), _p(self.B), _p(self.g), self.C, self.D,
                  float(var_floor), float(min_count), float(min_weight), ops._stream())

    def em_step(self, X, nsel=20, chunk=2048, var_floor=1e-3, min_count=10.0, min_weight=1e-5):
        """One EM iteration over all frames: posteriors, order-2 statistics over runs of ``chunk`` frames (each an fp32 sum), their
        float64 reduction, the M-step.  Returns the mean log-likelihood per frame under the parameters BEFORE the update, a float64
        device scalar: the float32 per-frame values are added in double by the reduce entry (rows of LL_ROW), then over its columns."""
        X = self._frames(X, "DiagUbm.em_step")
        F = X.shape[0]
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError("DiagUbm.em_step: chunk=%d must be positive" % chunk)
        ll = torch.zeros((-(-F // LL_ROW), LL_ROW), dtype=_F32, device=X.device)
        idx, post, _ = self.posteriors(X, nsel, 0.0, loglik_out=ll.view(-1))
        seg = np.minimum(np.arange(0, F + chunk, chunk, dtype=np.int64), F)
        acc = self.reduce(self.stats(X, seg, 2, idx, post))
        self.update(acc, var_floor, min_count, min_weight)
        return self.reduce(ll).sum() / F

    def fit(self, X, iters=4, nsel=20, var_floor=1e-3, min_count=10.0, min_weight=1e-5, chunk=2048, log=print):
        """``iters`` EM iterations; returns the history of mean log-likelihoods per frame (each under the parameters its iteration
        started from), host floats.  ``log``: called with one line per iteration, or None."""
        hist = []
        for it in range(int(iters)):
            hist.append(float(self.em_step(X, nsel, chunk, var_floor, min_count, min_weight)))
            if log:
                log("diag-ubm EM %d/%d: mean log-likelihood per frame %.6f" % (it + 1, iters, hist[-1]))
        return hist


# ------------------------------------------------------------------------------------------------------------ Baum-Welch statistics
def plan_bw_passes(frames_per_utt, C, D, nsel, free):
    """Host planning of ``bw_stats``: the utterances go through in passes [u0, u1) whose temporaries -- the sparse posteriors of the
    pass's frames (nsel * 8 + 4 bytes a frame) and its slab (C * (1 + D) * 4 bytes an utterance) -- take at most half of what is left
    of ``free`` after the outputs N (U, C) and F (U, C, D).  Returns (passes, need): ``need`` = the outputs plus twice the costliest
    single utterance, the least ``free`` with which the plan exists (the caller refuses below it)."""
    n = [int(v) for v in frames_per_utt]
    if not n or min(n) < 0:
        raise ValueError("plan_bw_passes: need at least one utterance and no negative length")
    row = C * (1 + D) * 4
    cost = [f * (nsel * 8 + 4) + row for f in n]
    out_bytes = len(n) * row
    need = out_bytes + 2 * max(cost)
    budget = max((int(free) - out_bytes) // 2, max(cost))
    passes, u0, acc = [], 0, 0
    for u, c in enumerate(cost):
        if u > u0 and acc + c > budget:
            passes.append((u0, u))
            u0, acc = u, 0
        acc += c
    passes.append((u0, len(n)))
    return passes, need


def bw_stats(ubm, X, utt_off, nsel=20, min_post=0.025):
    """The per-utterance Baum-Welch statistics of ``X`` (F, D) under ``ubm``: ``N`` (U, C) and ``F`` (U, C, D) float32, from posteriors
    pruned at ``min_post`` and renormalised (Kaldi's posterior lists).  ``utt_off``: a HOST sequence of U + 1 ascending offsets."""
    X = ubm._frames(X, "bw_stats")
    if isinstance(utt_off, torch.Tensor):
        utt_off = utt_off.cpu().numpy()
    _, host = _offsets(np.asarray(utt_off), "bw_stats: utt_off", "cpu", total=X.shape[0])
    U, C, D = host.size - 1, ubm.C, ubm.D
    passes, need = plan_bw_passes(np.diff(host), C, D, int(nsel), ops.free_bytes(X.device))
    ops.require_free_bytes(need, X.device, "bw_stats: the statistics of %d utterances x %d Gaussians x %d dimensions need" % (U, C, D),
                           "fewer utterances per call, or a smaller UBM")
    N = torch.empty((U, C), dtype=_F32, device=X.device)
    Fs = torch.empty((U, C, D), dtype=_F32, device=X.device)
    for u0, u1 in passes:
        f0, f1 = int(host[u0]), int(host[u1])
        if f1 == f0:
            N[u0:u1].zero_()
            Fs[u0:u1].zero_()
            continue
        slab = ubm.stats(X[f0:f1], host[u0:u1 + 1] - f0, 1, nsel=nsel, min_post=min_post)
        N[u0:u1].copy_(slab[:, :, 0])
        Fs[u0:u1].copy_(slab[:, :, 1:])
    return N, Fs


# ------------------------------------------------------------------------------------------------------------ the whole chain
def frames_per_utterance(pl, B):
    """Compact frames of every row of a ``dvector.plan``: its tiles' frame counts added per row (a row without a window has none)."""
    n = np.zeros(B, dtype=np.int64)
    if len(pl.tiles):
        np.add.at(n, pl.tiles[:, 0].astype(np.int64), pl.tiles[:, 5].astype(np.int64))
    return n


def train_diag_ubm(front_end, y16, lengths, spans=None, num_gauss=1024, seed=0, n_ceps=20, lifter=22, delta_window=3, delta_order=2, cmn_window=300,
                   **fit_kw):
    """Waveforms to a trained diagonal UBM for a ragged device batch: the ``DvectorExtractor`` plan and ``log_mel`` (``front_end``: a
    ``DvectorExtractor``, or a ``TisvFrontEnd`` to build one around -- no embedder runs), ``cepstral_features``, ``DiagUbm.from_frames``
    and ``fit(**fit_kw)``.  Returns a namespace: ``ubm``, ``history``, ``features`` (G, cols), ``utt_off`` (host int64, B + 1)."""
    from .dvector import DvectorExtractor
    ex = front_end
    if not isinstance(ex, DvectorExtractor):
        ex = DvectorExtractor(front_end, SimpleNamespace(dims=(front_end.nmels,)))
    pl = ex.plan(y16, lengths, spans)
    if pl.n_frames < 1:
        raise ValueError("train_diag_ubm: no utterance of the batch gives a frame")
    utt_off = np.concatenate([[0], np.cumsum(frames_per_utterance(pl, y16.shape[0]))]).astype(np.int64)
    mel = ex.log_mel(y16, pl)
    X = cepstral_features(mel, utt_off, n_ceps, lifter, delta_window, delta_order, cmn_window)[:pl.n_frames]
    ubm = DiagUbm.from_frames(X, num_gauss, seed)
    return SimpleNamespace(ubm=ubm, history=ubm.fit(X, **fit_kw), features=X, utt_off=utt_off)
