"""The i-vector system on the device: cepstral features, a diagonal-covariance GMM-UBM trained by EM, the Baum-Welch statistics (zeroth
and first order, per utterance), the total-variability extractor trained by EM on them, i-vector extraction and cosine trial scores.

This is the bottom of the reference's ``kaldi_ivectors/run.sh`` (MFCC -> VAD -> diagonal UBM -> full UBM -> extractor -> PLDA), as far
as the full-covariance UBM (``FullUbm``, ``train_full_ubm``; yardstick ``tests/_fgmm_ref.py``).  Kaldi's binaries are NOT reproduced: its
MFCC (povey window, snip-edges, energy in C0), its energy VAD and the recipe's ``conf/`` values are not pinned here; the algorithms are
the ones stated at the entries in ``include/ssv_hip.h``, and a float64 restatement (``tests/_ivector_ref.py``) is the yardstick.  Ours,
not Kaldi's: the initialisation of ``DiagUbm.from_frames`` and the treatment of a starved or degenerate Gaussian in the M-steps.

The extractor (``TotalVariability``) is this project's model too, stated at the entries of ``include/ssv_hip.h`` ("I-vector extractor"):
no prior offset, no weight projection; the UBM under it is diagonal (``DiagUbm``) or full-covariance (``FullUbm``); scoring here is
cosine on length-normalised vectors (PLDA is ``plda.py``) -- and its yardstick is ``tests/_ivector_tv_ref.py``.

Every FLOP of the hot path runs in ``csrc/ivector.hip``, ``csrc/fgmm.hip`` and ``csrc/ivector_tv.hip``; torch is plumbing (memory, the
stream).  Tensors must live on a ROCm device.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, ops
from .ops import _p

_F32, _F64, _I32, _I64 = torch.float32, torch.float64, torch.int32, torch.int64
MAX_D, MAX_C, MAX_NSEL, MAX_R = 128, 2048, 32, 192
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


class FullUbm:
    """A full-covariance Gaussian mixture on one device (``include/ssv_hip.h``, "full-covariance UBM"): ``w`` (C,), ``mu`` (C, D) and
    ``cov`` (C, Pd) float64, ``cov`` the packed lower triangles of the covariances (``tri_pack``), with the planes the kernels read:
    the float32 whitening matrices ``Wt`` (C, D, D), ``muf`` (C, D), ``g`` (C,) and the float64 packed inverses ``icov`` (C, Pd).
    The Gaussians of a frame are selected by the diagonal mixture ``self.diag()``; the posteriors over the selected are the full ones."""

    def __init__(self, w, mu, cov):
        for t, name in ((w, "w"), (mu, "mu"), (cov, "cov")):
            if not isinstance(t, torch.Tensor):
                raise ValueError("FullUbm: %s must be a torch tensor" % name)
        if mu.dim() != 2 or cov.dim() != 2 or cov.shape != (mu.shape[0], tri_size(mu.shape[1])) or w.shape != (mu.shape[0],) \
                or any(t.dtype != _F64 for t in (w, mu, cov)):
            raise ValueError("FullUbm: need float64 w (C,), mu (C, D), cov (C, D (D + 1) / 2); got %s %s, %s %s, %s %s"
                             % (w.dtype, tuple(w.shape), mu.dtype, tuple(mu.shape), cov.dtype, tuple(cov.shape)))
        C, D = mu.shape
        if not (1 <= C <= MAX_C and 1 <= D <= MAX_D):
            raise ValueError("FullUbm: C=%d must lie in [1, %d] and D=%d in [1, %d]" % (C, MAX_C, D, MAX_D))
        if w.device != mu.device or cov.device != mu.device:
            raise ValueError("FullUbm: w, mu and cov must live on one device")
        self.w, self.mu, self.cov = w.contiguous().clone(), mu.contiguous().clone(), cov.contiguous().clone()
        self._planes = self._diag = None

    C = property(lambda self: self.mu.shape[0])
    D = property(lambda self: self.mu.shape[1])
    Pd = property(lambda self: self.cov.shape[1])
    device = property(lambda self: self.mu.device)

    def _alloc_planes(self):
        C, D, dev = self.C, self.D, self.device
        return (torch.empty((C, D, D), dtype=_F32, device=dev), torch.empty((C, D), dtype=_F32, device=dev), torch.empty((C,), dtype=_F32, device=dev),
                torch.empty((C, self.Pd), dtype=_F64, device=dev))

    def planes(self):
        """(Wt, muf, g, icov) of the current parameters: built on the device at first use (``ssv_fgmm_planes``), rewritten by every
        M-step.  The state itself may sit on the host; every operation needs a ROCm device."""
        if self._planes is None:
            for t, name in ((self.w, "w"), (self.mu, "mu"), (self.cov, "cov")):
                ops._dev(t, "FullUbm: " + name)
            pl = self._alloc_planes()
            _lib.call("ssv_fgmm_planes", _p(self.w), _p(self.mu), _p(self.cov), *(_p(t) for t in pl), self.C, self.D, ops._stream())
            self._planes = pl
        return self._planes

    Wt = property(lambda self: self.planes()[0])
    muf = property(lambda self: self.planes()[1])
    g = property(lambda self: self.planes()[2])
    icov = property(lambda self: self.planes()[3])

    @property
    def var(self):
        """diag(Sigma) (C, D) float64."""
        i = torch.arange(self.D, device=self.device)
        return self.cov[:, i * (i + 1) // 2 + i].contiguous()

    @classmethod
    def from_diag(cls, diag_ubm):
        """The full mixture whose covariances are ``diag_ubm``'s diagonals: where ``sid/train_full_ubm.sh`` starts."""
        C, D = diag_ubm.mu.shape
        cov = torch.zeros((C, tri_size(D)), dtype=_F64, device=diag_ubm.device)
        i = torch.arange(D, device=diag_ubm.device)
        cov[:, i * (i + 1) // 2 + i] = diag_ubm.var
        return cls(diag_ubm.w, diag_ubm.mu, cov)

    def diag(self):
        """The selector: a ``DiagUbm`` on diag(Sigma), rebuilt after every update."""
        if self._diag is None:
            self._diag = DiagUbm(self.w, self.mu, self.var)
        return self._diag

    # ------------------------------------------------------------------ state
    def state_dict(self):
        return {"w": self.w.clone(), "mu": self.mu.clone(), "cov": self.cov.clone()}

    def load_state_dict(self, sd):
        new = FullUbm(sd["w"].to(self.device), sd["mu"].to(self.device), sd["cov"].to(self.device))
        self.__dict__.update(new.__dict__)
        return self

    def save(self, path):
        """``.npz`` with the float64 ``w``, ``mu``, ``cov`` (the planes are derived)."""
        np.savez(path, w=self.w.cpu().numpy(), mu=self.mu.cpu().numpy(), cov=self.cov.cpu().numpy())

    @classmethod
    def load(cls, path, device="cuda"):
        """``device="cpu"`` gives a state holder only (to inspect or move); the operations need a ROCm device."""
        with np.load(path) as z:
            return cls(*(torch.from_numpy(np.asarray(z[k], dtype=np.float64)).to(device) for k in ("w", "mu", "cov")))

    # ------------------------------------------------------------------ operations
    def _frames(self, X, who):
        return _matrix(X, who + ": X", cols=self.D)

    def _idx(self, idx, F, who):
        idx = _matrix(idx, who + ": idx", dtype=_I32)
        if idx.shape[0] != F or idx.shape[1] > MAX_NSEL:
            raise ValueError("%s: idx must be (%d, nsel <= %d), got %s" % (who, F, MAX_NSEL, tuple(idx.shape)))
        return idx

    def group(self, idx):
        """The Gaussian-major lists of a selection ``idx`` (F, nsel) int32 (``ssv_fgmm_group_selection``): ``(start (C + 1,), pairs
        (F nsel,))`` int32, ``pairs[start[c]:start[c + 1]]`` the slots f * nsel + j whose Gaussian is c, ascending."""
        idx = _matrix(idx, "FullUbm.group: idx", dtype=_I32)
        F, nsel = idx.shape
        if nsel > MAX_NSEL:
            raise ValueError("FullUbm.group: idx has %d columns, at most %d" % (nsel, MAX_NSEL))
        start = torch.empty((self.C + 1,), dtype=_I32, device=idx.device)
        pairs = torch.empty((F * nsel,), dtype=_I32, device=idx.device)
        nws = _lib.query("ssv_fgmm_group_workspace", F, nsel, self.C)
        ws = ops._ws(nws, idx.device)
        _lib.call("ssv_fgmm_group_selection", _p(idx), _p(start), _p(pairs), F, nsel, self.C, _p(ws), ws.numel(), ops._stream())
        return start, pairs

    def posteriors(self, X, nsel=20, min_post=0.0, idx=None, groups=None, loglik_out=None):
        """``idx`` (F, nsel) int32 -- given, or the ``nsel`` likeliest Gaussians of ``self.diag()`` -- with the FULL-covariance posteriors
        among them (those below ``min_post`` zeroed, the rest renormalised) and the log-likelihood over the selected:
        ``(idx, post (F, nsel), loglik (F,))``.  ``groups``: ``self.group(idx)`` when the caller holds it already."""
        X = self._frames(X, "FullUbm.posteriors")
        F = X.shape[0]
        if not 0.0 <= min_post < 1.0:
            raise ValueError("FullUbm.posteriors: min_post=%r must lie in [0, 1)" % (min_post,))
        if idx is None:
            idx = self.diag().posteriors(X, nsel, 0.0)[0]
            groups = None
        idx = self._idx(idx, F, "FullUbm.posteriors")
        start, pairs = groups if groups is not None else self.group(idx)
        nsel = idx.shape[1]
        post = torch.empty((F, nsel), dtype=_F32, device=X.device)
        ll = loglik_out if loglik_out is not None else torch.empty((F,), dtype=_F32, device=X.device)
        nws = _lib.query("ssv_fgmm_post_workspace", F, nsel)
        ws = ops._ws(nws, X.device)
        Wt, muf, g, _ = self.planes()
        _lib.call("ssv_fgmm_select_post", _p(X), _p(Wt), _p(muf), _p(g), _p(idx), _p(start), _p(pairs), _p(post), _p(ll), F, self.D, self.C, nsel,
                  float(min_post), _p(ws), ws.numel(), ops._stream())
        return idx, post, ll[:F]

    def stats(self, X, seg_off, order=1, idx=None, post=None, nsel=20, min_post=0.0):
        """``slab`` (S, C, 1 + order * D) float32 as ``DiagUbm.stats``, from the full posteriors: what ``bw_stats`` and
        ``extract_ivectors`` call, so they work on either mixture."""
        X = self._frames(X, "FullUbm.stats")
        if (idx is None) != (post is None):
            raise ValueError("FullUbm.stats: idx and post come together")
        if idx is None:
            idx, post, _ = self.posteriors(X, nsel, min_post)
        return self.diag().stats(X, seg_off, order, idx, post)

    def full_stats(self, X, idx, post, groups=None):
        """(C, 1 + D + Pd) float64: N, S1, S2 centred on the current means, over each Gaussian's list (``ssv_fgmm_stats``)."""
        X = self._frames(X, "FullUbm.full_stats")
        F = X.shape[0]
        idx = self._idx(idx, F, "FullUbm.full_stats")
        post = _matrix(post, "FullUbm.full_stats: post", cols=idx.shape[1])
        if post.shape[0] != F:
            raise ValueError("FullUbm.full_stats: post must have %d rows, got %d" % (F, post.shape[0]))
        start, pairs = groups if groups is not None else self.group(idx)
        nsel = idx.shape[1]
        out = torch.empty((self.C, 1 + self.D + self.Pd), dtype=_F64, device=X.device)
        nws = _lib.query("ssv_fgmm_stats_workspace", F, nsel, self.C, self.D)
        ops.require_free_bytes(nws, X.device, "FullUbm.full_stats: the run sums of C=%d, D=%d need" % (self.C, self.D), "a smaller mixture")
        ws = ops._ws(nws, X.device)
        _lib.call("ssv_fgmm_stats", _p(X), _p(self.muf), _p(post), _p(start), _p(pairs), _p(out), F, self.D, self.C, nsel, _p(ws), ws.numel(), ops._stream())
        return out

    def update(self, stats, var_floor=1e-3, min_count=10.0, min_weight=1e-5):
        """The M-step from ``full_stats``, in place (``ssv_fgmm_update``).  Returns ``kept`` (C,) int32: 1 where the Gaussian kept its
        mean and covariance (starved, or a conditional variance below ``var_floor``)."""
        stats = _matrix(stats, "FullUbm.update: stats", dtype=_F64, cols=1 + self.D + self.Pd)
        if stats.shape[0] != self.C:
            raise ValueError("FullUbm.update: stats must have C=%d rows, got %d" % (self.C, stats.shape[0]))
        pl = self._planes if self._planes is not None else self._alloc_planes()
        for t, name in ((self.w, "w"), (self.mu, "mu"), (self.cov, "cov")):
            ops._dev(t, "FullUbm: " + name)
        kept = torch.empty((self.C,), dtype=_I32, device=self.device)
        _lib.call("ssv_fgmm_update", _p(stats), _p(self.w), _p(self.mu), _p(self.cov), *(_p(t) for t in pl), _p(kept), self.C, self.D,
                  float(var_floor), float(min_count), float(min_weight), ops._stream())
        self._planes, self._diag = pl, None
        return kept

    def em_step(self, X, idx, groups=None, var_floor=1e-3, min_count=10.0, min_weight=1e-5):
        """One EM iteration on the selection ``idx``: posteriors (no pruning), centred statistics, the M-step.  Returns the mean
        log-likelihood per frame over the selected under the parameters BEFORE the update (a float64 device scalar, summed as in
        ``DiagUbm.em_step``) and ``kept``."""
        X = self._frames(X, "FullUbm.em_step")
        F = X.shape[0]
        if groups is None:
            groups = self.group(self._idx(idx, F, "FullUbm.em_step"))
        ll = torch.zeros((-(-F // LL_ROW), LL_ROW), dtype=_F32, device=X.device)
        idx, post, _ = self.posteriors(X, idx=idx, groups=groups, loglik_out=ll.view(-1))
        kept = self.update(self.full_stats(X, idx, post, groups), var_floor, min_count, min_weight)
        return DiagUbm.reduce(ll).sum() / F, kept

    def fit(self, X, iters=4, nsel=20, var_floor=1e-3, min_count=10.0, min_weight=1e-5, log=print):
        """``iters`` EM iterations on ONE selection, taken from ``self.diag()`` at the start and held (``sid/train_full_ubm.sh`` selects
        once, with the diagonal UBM): exact EM on the truncated objective, whose history -- the mean log-likelihoods over the selected,
        each under the parameters its iteration started from, host floats -- cannot decrease unless a Gaussian is kept or a weight floored."""
        X = self._frames(X, "FullUbm.fit")
        nsel = int(nsel)
        if not 1 <= nsel <= min(self.C, MAX_NSEL):
            raise ValueError("FullUbm.fit: nsel=%d must lie in [1, min(C=%d, %d)]" % (nsel, self.C, MAX_NSEL))
        idx = self.diag().posteriors(X, nsel, 0.0)[0]
        groups = self.group(idx)
        hist = []
        for it in range(int(iters)):
            ll, kept = self.em_step(X, idx, groups, var_floor, min_count, min_weight)
            hist.append(float(ll))
            if log:
                log("full-ubm EM %d/%d: mean log-likelihood per frame %.6f, %d Gaussians kept" % (it + 1, iters, hist[-1], int(kept.sum())))
        return hist


def train_full_ubm(diag_ubm, X, iters=4, nsel=20, **fit_kw):
    """``sid/train_full_ubm.sh``: ``FullUbm.from_diag(diag_ubm)`` and ``fit(X, iters, nsel, **fit_kw)``.  Returns a namespace: ``ubm``, ``history``."""
    ubm = FullUbm.from_diag(diag_ubm)
    return SimpleNamespace(ubm=ubm, history=ubm.fit(X, iters, nsel, **fit_kw))


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


# ------------------------------------------------------------------------------------------------------------ the packed triangle
def tri_size(R):
    return R * (R + 1) // 2


def tri_pack(S):
    """(..., R, R) -> (..., P): the lower triangle row-major, element (i, j), j <= i, at i (i + 1) / 2 + j (host arrays)."""
    S = np.asarray(S)
    i, j = np.tril_indices(S.shape[-1])
    return np.ascontiguousarray(S[..., i, j])


def tri_unpack(p, R=None):
    """(..., P) -> (..., R, R) symmetric (host arrays); P must be a triangular number (and R's, when R is given)."""
    p = np.asarray(p)
    n = int(round((np.sqrt(8.0 * p.shape[-1] + 1.0) - 1.0) / 2.0))
    if tri_size(n) != p.shape[-1] or (R is not None and n != R):
        raise ValueError("tri_unpack: %d entries are not the lower triangle of a %s x %s matrix" % (p.shape[-1], R or "R", R or "R"))
    i, j = np.tril_indices(n)
    S = np.zeros(p.shape[:-1] + (n, n), dtype=p.dtype)
    S[..., i, j] = p
    S[..., j, i] = p
    return S


# ------------------------------------------------------------------------------------------------------------ the extractor
def _stats_pair(N, Ft, C, D, who):
    N = _matrix(N, who + ": N", cols=C)
    if not isinstance(Ft, torch.Tensor):
        raise ValueError("%s: Ft: need a torch tensor, got %s" % (who, type(Ft).__name__))
    ops._dev(Ft, who + ": Ft")
    if Ft.dtype != _F32 or Ft.numel() != N.shape[0] * C * D or Ft.shape[0] != N.shape[0]:
        raise ValueError("%s: Ft: need float32 (%d, %d, %d), got %s %s" % (who, N.shape[0], C, D, Ft.dtype, tuple(Ft.shape)))
    return N, Ft.contiguous().view(N.shape[0], C * D)


def centre_stats(ubm, N, F, out=None):
    """``Ft`` (U, C, D) = ``F`` - ``N`` mu, one float32 fused multiply-add per element (``ssv_ivec_centre_stats``): the first-order
    statistics centred on the UBM's means BEFORE any product, so that the big product does not cancel.  ``out``: where to write (``F``
    itself is allowed); default a new tensor.  ``ubm``: a ``DiagUbm`` or a ``TotalVariability``."""
    C, D = ubm.mu.shape
    N, F2 = _stats_pair(N, F, C, D, "centre_stats")
    ops._dev(ubm.mu, "centre_stats: mu")
    if out is None:
        out = torch.empty((N.shape[0], C, D), dtype=_F32, device=N.device)
    elif out.dtype != _F32 or out.numel() != F2.numel() or not out.is_contiguous() or not out.is_cuda:
        raise ValueError("centre_stats: out must be a contiguous float32 device tensor of F's size")
    _lib.call("ssv_ivec_centre_stats", _p(N), _p(F2), _p(ubm.mu), _p(out), N.shape[0], C, D, ops._stream())
    return out.view(N.shape[0], C, D)


def product(A, B, out=None):
    """``out`` (m, n) float32 = ``A`` (m, K) ``B`` (K, n) on the exact-fp32 MFMA, K in runs added in double (``ssv_ivec_product``)."""
    A, B = _matrix(A, "product: A"), _matrix(B, "product: B")
    if A.shape[1] != B.shape[0]:
        raise ValueError("product: A is %s and B is %s" % (tuple(A.shape), tuple(B.shape)))
    if out is None:
        out = torch.empty((A.shape[0], B.shape[1]), dtype=_F32, device=A.device)
    elif out.dtype != _F32 or tuple(out.shape) != (A.shape[0], B.shape[1]) or not out.is_contiguous() or not out.is_cuda:
        raise ValueError("product: out must be a contiguous float32 device tensor (%d, %d)" % (A.shape[0], B.shape[1]))
    _lib.call("ssv_ivec_product", _p(A), _p(B), _p(out), A.shape[0], B.shape[1], A.shape[1], ops._stream())
    return out


def product_tn(A, B, acc):
    """``acc`` (m, n) float64 += ``A`` (U, m)^T ``B`` (U, n), in place (``ssv_ivec_product_tn``)."""
    A, B = _matrix(A, "product_tn: A"), _matrix(B, "product_tn: B")
    if not isinstance(acc, torch.Tensor) or not acc.is_cuda or acc.dtype != _F64 or not acc.is_contiguous() or A.shape[0] != B.shape[0] \
            or acc.numel() != A.shape[1] * B.shape[1]:
        raise ValueError("product_tn: A %s, B %s need a contiguous float64 device accumulator of %d x %d" % (tuple(A.shape), tuple(B.shape), A.shape[1], B.shape[1]))
    _lib.call("ssv_ivec_product_tn", _p(A), _p(B), _p(acc), A.shape[0], A.shape[1], B.shape[1], ops._stream())
    return acc


def plan_tv_passes(U, C, D, R, free, train, full=False):
    """Host planning of the extractor's passes over ``U`` utterances whose statistics are resident: a pass [u0, u1) holds per utterance
    Lp (P floats; training: M as well), b and w (R floats each), obj (a double) and, training, a one -- at most half of what is left of
    ``free`` after the fixed part: training, the float64 accumulators A (C, P), Cm (C D, R), Nc (C) and sum M (P); extraction, the
    output w (U, R); ``full`` (a full-covariance UBM): the float64 packed inverses icov (C, D (D + 1) / 2) as well, either way.
    Returns (passes, need): ``need`` = the fixed part plus one utterance, the least ``free`` with which a plan exists."""
    U, P = int(U), tri_size(int(R))
    if U < 1:
        raise ValueError("plan_tv_passes: need at least one utterance")
    per = P * 4 * (2 if train else 1) + R * 8 + 8 + (4 if train else 0)
    fixed = (C * P + C * D * R + C + P) * 8 if train else U * R * 4
    if full:
        fixed += C * tri_size(int(D)) * 8
    n = max(1, min(U, ((int(free) - fixed) // 2) // per))
    return [(u0, min(u0 + n, U)) for u0 in range(0, U, n)], fixed + per


def plan_extract_passes(frames_per_utt, C, D, R, nsel, free):
    """Host planning of ``extract_ivectors``: a pass [u0, u1) holds the sparse posteriors of its frames (nsel * 8 + 4 bytes a frame) and per
    utterance the slab, N and Ft (2 C (1 + D) floats), Lp (P floats), b (R floats) and obj -- at most half of what is left of ``free``
    after the output w (U, R).  Returns (passes, need), ``need`` = the output plus twice the costliest single utterance."""
    n = [int(v) for v in frames_per_utt]
    if not n or min(n) < 0:
        raise ValueError("plan_extract_passes: need at least one utterance and no negative length")
    row = 2 * C * (1 + D) * 4 + tri_size(int(R)) * 4 + R * 4 + 8
    cost = [f * (nsel * 8 + 4) + row for f in n]
    out_bytes = len(n) * R * 4
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


class TotalVariability:
    """A total-variability model on one device: ``T`` (C, D, R) float64 and the UBM it stands on (``w`` (C,), ``mu``, ``var`` (C, D)
    float64), with the float32 planes ``G`` (C D, R) and ``Pk`` (C, P) the products read, rebuilt after every update.  ``cov`` (C, Pd)
    float64, optional: the packed full covariances of a ``FullUbm``; the planes then hold Sigma^-1 in place of 1 / var
    (``ssv_ivec_tv_planes_full``), ``var`` is their diagonal, and nothing below the planes knows the difference."""

    def __init__(self, T, w, mu, var, cov=None):
        for t, name in ((T, "T"), (w, "w"), (mu, "mu"), (var, "var")):
            if not isinstance(t, torch.Tensor):
                raise ValueError("TotalVariability: %s must be a torch tensor" % name)
        if T.dim() != 3 or mu.dim() != 2 or tuple(T.shape[:2]) != tuple(mu.shape) or var.shape != mu.shape or w.shape != (mu.shape[0],) \
                or any(t.dtype != _F64 for t in (T, w, mu, var)):
            raise ValueError("TotalVariability: need float64 T (C, D, R), w (C,), mu (C, D), var (C, D); got %s %s, %s %s, %s %s, %s %s"
                             % (T.dtype, tuple(T.shape), w.dtype, tuple(w.shape), mu.dtype, tuple(mu.shape), var.dtype, tuple(var.shape)))
        C, D, R = T.shape
        if not (1 <= C <= MAX_C and 1 <= D <= MAX_D and 1 <= R <= MAX_R):
            raise ValueError("TotalVariability: C=%d must lie in [1, %d], D=%d in [1, %d] and R=%d in [1, %d]" % (C, MAX_C, D, MAX_D, R, MAX_R))
        if any(t.device != T.device for t in (w, mu, var)):
            raise ValueError("TotalVariability: T, w, mu and var must live on one device")
        if cov is not None and (not isinstance(cov, torch.Tensor) or cov.dtype != _F64 or tuple(cov.shape) != (C, tri_size(D)) or cov.device != T.device):
            raise ValueError("TotalVariability: cov must be a float64 (C, D (D + 1) / 2) tensor on T's device")
        self.T, self.w, self.mu, self.var = (t.contiguous().clone() for t in (T, w, mu, var))
        self.cov = None if cov is None else cov.contiguous().clone()
        self._planes = self._ubm = None

    C = property(lambda self: self.T.shape[0])
    D = property(lambda self: self.T.shape[1])
    R = property(lambda self: self.T.shape[2])
    P = property(lambda self: tri_size(self.T.shape[2]))
    device = property(lambda self: self.T.device)

    def planes(self):
        """(G, Pk) of the current ``T`` (``ssv_ivec_tv_planes``; with ``cov``, ``ssv_ivec_tv_planes_full`` on the UBM's ``icov``): built at
        first use, rebuilt by every update."""
        if self._planes is None:
            for t, name in ((self.T, "T"), (self.var, "var")):
                ops._dev(t, "TotalVariability: " + name)
            G = torch.empty((self.C * self.D, self.R), dtype=_F32, device=self.device)
            Pk = torch.empty((self.C, self.P), dtype=_F32, device=self.device)
            if self.cov is None:
                _lib.call("ssv_ivec_tv_planes", _p(self.T), _p(self.var), _p(G), _p(Pk), self.C, self.D, self.R, ops._stream())
            else:
                _lib.call("ssv_ivec_tv_planes_full", _p(self.T), _p(self.ubm().icov), _p(G), _p(Pk), self.C, self.D, self.R, ops._stream())
            self._planes = (G, Pk)
        return self._planes

    G = property(lambda self: self.planes()[0])
    Pk = property(lambda self: self.planes()[1])

    def ubm(self):
        if self._ubm is None:
            self._ubm = DiagUbm(self.w, self.mu, self.var) if self.cov is None else FullUbm(self.w, self.mu, self.cov)
        return self._ubm

    # ------------------------------------------------------------------ state
    def state_dict(self):
        sd = {"T": self.T.clone(), "w": self.w.clone(), "mu": self.mu.clone(), "var": self.var.clone()}
        if self.cov is not None:
            sd["cov"] = self.cov.clone()
        return sd

    def save(self, path):
        """``.npz`` with the float64 ``T``, ``w``, ``mu``, ``var`` and, when set, ``cov`` (the planes are derived)."""
        np.savez(path, **{k: v.cpu().numpy() for k, v in self.state_dict().items()})

    @classmethod
    def load(cls, path, device="cuda"):
        """``device="cpu"`` gives a state holder only; the operations need a ROCm device."""
        with np.load(path) as z:
            keys = ("T", "w", "mu", "var") + (("cov",) if "cov" in z.files else ())
            return cls(*(torch.from_numpy(np.asarray(z[k], dtype=np.float64)).to(device) for k in keys))

    @classmethod
    def from_ubm(cls, ubm, R, seed=0):
        """The starting point of EM -- OURS: T_cdr = 0.1 sqrt(var_cd) z, z standard normal drawn on the host by
        ``numpy.random.default_rng(seed)`` in (C, D, R) order.  ``ubm``: a ``DiagUbm``, or a ``FullUbm`` (var = diag Sigma; its ``cov`` is kept)."""
        R = int(R)
        if not 1 <= R <= MAX_R:
            raise ValueError("TotalVariability.from_ubm: R=%d must lie in [1, %d]" % (R, MAX_R))
        z = np.random.default_rng(seed).standard_normal((ubm.C, ubm.D, R))
        T = 0.1 * np.sqrt(ubm.var.cpu().numpy())[:, :, None] * z
        return cls(torch.from_numpy(T).to(ubm.device), ubm.w, ubm.mu, ubm.var, cov=getattr(ubm, "cov", None))

    # ------------------------------------------------------------------ operations
    def estep(self, N, Ft, want_M=False, w_out=None):
        """One pass, no planning: ``Lp`` = N Pk and ``b`` = Ft G (``ssv_ivec_product``), then ``ssv_ivec_estep``.  Returns a namespace: ``w``
        (U, R) float32, ``obj`` (U,) float64, ``M`` (U, P) float32 or None, and the device's own ``Lp`` (U, P), ``b`` (U, R)."""
        N, Ft = _stats_pair(N, Ft, self.C, self.D, "TotalVariability.estep")
        U, dev = N.shape[0], N.device
        G, Pk = self.planes()
        Lp, b = product(N, Pk), product(Ft, G)
        w = w_out if w_out is not None else torch.empty((U, self.R), dtype=_F32, device=dev)
        M = torch.empty((U, self.P), dtype=_F32, device=dev) if want_M else None
        obj = torch.empty((U,), dtype=_F64, device=dev)
        _lib.call("ssv_ivec_estep", _p(Lp), _p(b), _p(w), _p(M), _p(obj), U, self.R, ops._stream())
        return SimpleNamespace(w=w, obj=obj, M=M, Lp=Lp, b=b)

    def _passes(self, U, dev, train, who):
        passes, need = plan_tv_passes(U, self.C, self.D, self.R, ops.free_bytes(dev), train, full=self.cov is not None)
        ops.require_free_bytes(need, dev, "%s: %d utterances at C=%d, D=%d, R=%d need" % (who, U, self.C, self.D, self.R), "a smaller rank or UBM")
        return passes

    def em_step(self, N, Ft, min_div=True, min_count=10.0):
        """One EM iteration over all utterances, in planned passes: per pass the E-step with M, then A += N^T M, Cm += Ft^T w, Nc += N^T 1
        into float64 accumulators (``ssv_ivec_product_tn``) and sum M by ``ssv_gmm_stats_reduce``; then ``ssv_ivec_tv_update`` -- with
        ``min_div`` after J = chol_lower(mean M), an R x R float64 factorisation on the host -- and the planes of the new ``T``.  Returns the
        mean objective per utterance under the parameters BEFORE the update, a float64 device scalar."""
        N, Ft = _stats_pair(N, Ft, self.C, self.D, "TotalVariability.em_step")
        U, dev, C, D, R, P = N.shape[0], N.device, self.C, self.D, self.R, self.P
        A = torch.zeros((C, P), dtype=_F64, device=dev)
        Cm = torch.zeros((C * D, R), dtype=_F64, device=dev)
        Nc = torch.zeros((C, 1), dtype=_F64, device=dev)
        Msum = torch.zeros((P,), dtype=_F64, device=dev)
        obj = torch.zeros((), dtype=_F64, device=dev)
        for u0, u1 in self._passes(U, dev, True, "TotalVariability.em_step"):
            e = self.estep(N[u0:u1], Ft[u0:u1], want_M=True)
            product_tn(N[u0:u1], e.M, A)
            product_tn(Ft[u0:u1], e.w, Cm)
            product_tn(N[u0:u1], torch.ones((u1 - u0, 1), dtype=_F32, device=dev), Nc)
            Msum += DiagUbm.reduce(e.M)
            obj += e.obj.sum()
        J = None
        if min_div:
            J = torch.from_numpy(np.linalg.cholesky(tri_unpack(Msum.cpu().numpy() / U, R))).to(dev).contiguous()
        _lib.call("ssv_ivec_tv_update", _p(A), _p(Cm), _p(Nc), _p(J), _p(self.T), C, D, R, float(min_count), ops._stream())
        self._planes = None
        self.planes()
        return obj / U

    def fit(self, N, Ft, iters=5, min_div=True, min_count=10.0, log=print):
        """``iters`` EM iterations (the recipe's --num-iters is 5); returns the history of mean objectives (each under the parameters its
        iteration started from), host floats."""
        hist = []
        for it in range(int(iters)):
            hist.append(float(self.em_step(N, Ft, min_div, min_count)))
            if log:
                log("ivector-extractor EM %d/%d: mean objective per utterance %.6f" % (it + 1, iters, hist[-1]))
        return hist

    def extract(self, N, Ft):
        """The i-vectors ``w`` (U, R) float32 of resident statistics, in planned passes; every row is the bits of a one-pass E-step."""
        N, Ft = _stats_pair(N, Ft, self.C, self.D, "TotalVariability.extract")
        U, dev = N.shape[0], N.device
        w = torch.empty((U, self.R), dtype=_F32, device=dev)
        for u0, u1 in self._passes(U, dev, False, "TotalVariability.extract"):
            self.estep(N[u0:u1], Ft[u0:u1], w_out=w[u0:u1])
        return w


def train_ivector_extractor(ubm, X, utt_off, R, iters=5, nsel=20, min_post=0.025, seed=0, min_div=True, min_count=10.0, log=print):
    """Frames to a trained extractor: ``bw_stats``, ``centre_stats`` in place, ``TotalVariability.from_ubm(ubm, R, seed)`` and ``fit``.
    Returns a namespace: ``tv``, ``history``, ``N`` (U, C), ``Ft`` (U, C, D)."""
    N, F = bw_stats(ubm, X, utt_off, nsel, min_post)
    Ft = centre_stats(ubm, N, F, out=F)
    tv = TotalVariability.from_ubm(ubm, R, seed)
    return SimpleNamespace(tv=tv, history=tv.fit(N, Ft, iters, min_div, min_count, log), N=N, Ft=Ft)


def extract_ivectors(tv, X, utt_off, nsel=20, min_post=0.025):
    """Frames to i-vectors (U, R) float32 under ``tv`` and its UBM, in passes planned by ``plan_extract_passes``: per pass the Baum-Welch
    statistics of its utterances, centred in place, then the E-step; the statistics of all utterances are never resident at once.
    ``utt_off``: a HOST sequence of U + 1 ascending offsets.  A row does not depend on the pass it went through."""
    ubm = tv.ubm()
    X = ubm._frames(X, "extract_ivectors")
    if isinstance(utt_off, torch.Tensor):
        utt_off = utt_off.cpu().numpy()
    _, host = _offsets(np.asarray(utt_off), "extract_ivectors: utt_off", "cpu", total=X.shape[0])
    U, C, D = host.size - 1, tv.C, tv.D
    passes, need = plan_extract_passes(np.diff(host), C, D, tv.R, int(nsel), ops.free_bytes(X.device))
    ops.require_free_bytes(need, X.device, "extract_ivectors: %d utterances at C=%d, D=%d, R=%d need" % (U, C, D, tv.R), "fewer utterances per call")
    w = torch.empty((U, tv.R), dtype=_F32, device=X.device)
    for u0, u1 in passes:
        f0, f1 = int(host[u0]), int(host[u1])
        if f1 == f0:
            w[u0:u1].zero_()            # no frames: zero statistics, whose E-step is w = 0 exactly
            continue
        slab = ubm.stats(X[f0:f1], host[u0:u1 + 1] - f0, 1, nsel=nsel, min_post=min_post)
        N, F = slab[:, :, 0].contiguous(), slab[:, :, 1:].contiguous()
        tv.estep(N, centre_stats(tv, N, F, out=F), w_out=w[u0:u1])
    return w


# ------------------------------------------------------------------------------------------------------------ trials
def cosine_trials(enroll, spk_off, evalv):
    """``scores`` (E, S) float32: eval vector e against the model of speaker s, the re-normalised mean of the length-normalised enrolment
    rows [spk_off[s], spk_off[s+1]) (``ssv_ivec_cosine_trials``).  A zero vector scores 0."""
    enroll = _matrix(enroll, "cosine_trials: enroll")
    evalv = _matrix(evalv, "cosine_trials: evalv", cols=enroll.shape[1])
    off, host = _offsets(spk_off, "cosine_trials: spk_off", enroll.device, total=enroll.shape[0])
    S = off.numel() - 1
    scores = torch.empty((evalv.shape[0], S), dtype=_F32, device=enroll.device)
    hp = None if host is None else host.ctypes.data_as(ctypes.c_void_p)
    _lib.call("ssv_ivec_cosine_trials", _p(enroll), _p(off), hp, _p(evalv), _p(scores), enroll.shape[0], S, evalv.shape[0], enroll.shape[1], ops._stream())
    return scores


def _utt2spk(lines, who):
    out = []
    for line in lines:
        line = line.rstrip("\r\t\n ")
        parts = line.split(" ")
        if len(parts) != 2:
            raise ValueError("%s: %r is not '<utterance> <speaker>'" % (who, line))
        out.append((parts[0], parts[1]))
    return out


def split_enroll_eval(utt2spk_lines, enroll_num=3):
    """local/split_data_enroll_eval.py: per speaker, in the order speakers first appear, the first ``enroll_num`` utterances in file order
    enrol and the rest are eval (the script's shuffle is commented out).  Returns (enroll_lines, eval_lines), '<utterance> <speaker>'."""
    by_spk = {}
    for utt, spk in _utt2spk(utt2spk_lines, "split_enroll_eval"):
        by_spk.setdefault(spk, []).append(utt)
    enroll, ev = [], []
    for spk, utts in by_spk.items():
        for i, utt in enumerate(utts):
            (enroll if i < enroll_num else ev).append(utt + " " + spk)
    return enroll, ev


def trial_list(eval_utt2spk):
    """local/produce_trials.py: every eval utterance, in file order, against every speaker of the file, in order of first appearance:
    '<utterance> <speaker> target|nontarget'."""
    pairs = _utt2spk(eval_utt2spk, "trial_list")
    speakers = list(dict.fromkeys(spk for _, spk in pairs))
    return ["%s %s %s" % (utt, target, "target" if target == spk else "nontarget") for utt, spk in pairs for target in speakers]


def write_trial_scores(path, speakers, utterances, scores):
    """The score file ``parse_ivector_scores`` reads: '<speaker> <utterance> <score>' per trial, utterance-major as ``trial_list`` orders
    them; ``scores`` (len(utterances), len(speakers)), written with 9 significant digits (a float32 survives them)."""
    scores = np.asarray(scores.detach().cpu() if isinstance(scores, torch.Tensor) else scores)
    if scores.shape != (len(utterances), len(speakers)):
        raise ValueError("write_trial_scores: scores are %s for %d utterances x %d speakers" % (scores.shape, len(utterances), len(speakers)))
    with open(path, "w") as f:
        for e, utt in enumerate(utterances):
            for s, spk in enumerate(speakers):
                f.write("%s %s %.9g\n" % (spk, utt, scores[e, s]))
