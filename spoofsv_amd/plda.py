"""The back end of the i-vector system on the device: two-covariance PLDA trained by EM on length-normalised i-vectors, log-likelihood-ratio
trial scores, and the equal error rate.

This is the last third of the reference's ``kaldi_ivectors/run.sh`` (``ivector-compute-plda``, ``ivector-plda-scoring --num-utts``,
``compute-eer``).  Kaldi's binaries are NOT reproduced bit for bit: the model is this project's, stated in ``include/ssv_hip.h`` ("I-vector
back end: PLDA"), and a float64 numpy restatement (``tests/_plda_ref.py``) is the yardstick.

Every FLOP of training and scoring runs in ``csrc/plda.hip`` (and the product family of ``csrc/ivector_tv.hip``); torch is plumbing (memory,
the stream).  Two things run on the host in float64 numpy, once per model or per score list: ``PldaEstimator.finalize`` (an R x R
factorisation and eigen-decomposition, as the extractor's minimum-divergence factor) and ``compute_eer``.  Tensors must live on a ROCm
device.
"""
import ctypes

import numpy as np
import torch

from . import _lib, ops
from .ivector import MAX_R, _matrix, _offsets, product_tn, tri_pack, tri_size, tri_unpack
from .ops import _p

_F32, _F64, _I32 = torch.float32, torch.float64, torch.int32


def _host_ptr(host):
    return None if host is None else host.ctypes.data_as(ctypes.c_void_p)


def class_stats(X, spk_off, length_norm=True, residuals=True, means=True, model=False):
    """``ssv_plda_class_stats`` on ``X`` (n, R) float32 and the offsets of S speakers: returns (Xd, means, mu, model) -- the float32
    residual rows, the float64 speaker means (rows of speakers without rows: zero, as allocated), their unweighted mean, and the float32
    speaker models (the mean, normalised again) -- each None unless asked for."""
    X = _matrix(X, "class_stats: X")
    n, R = X.shape
    off, host = _offsets(spk_off, "class_stats: spk_off", X.device, total=n)
    S = off.numel() - 1
    Xd = torch.empty_like(X) if residuals else None
    m = torch.zeros((S, R), dtype=_F64, device=X.device) if means else None
    mu = torch.empty((R,), dtype=_F64, device=X.device) if means else None
    mod = torch.empty((S, R), dtype=_F32, device=X.device) if model else None
    if Xd is not None:
        Xd.zero_()                  # rows no speaker owns
    _lib.call("ssv_plda_class_stats", _p(X), _p(off), _host_ptr(host), _p(Xd), _p(m), _p(mu), _p(mod), n, S, R, int(bool(length_norm)), ops._stream())
    return Xd, m, mu, mod


def mixed_inverse(a, b, coef=None, want_logdet=True):
    """``out`` (J, P) = (a + coef_j b)^-1 and ``logdet`` (J) = log|a + coef_j b| (``ssv_plda_mixed_inverse``); ``a`` None: (coef_j b)^-1.
    ``b`` (P,) with ``coef`` (J,), or ``b`` (J, P) -- a matrix per row -- with ``coef`` None (ones).  Packed float64 device tensors."""
    many = b.dim() == 2
    if many and coef is not None:
        raise ValueError("mixed_inverse: a stack of b comes without coefficients")
    P = b.shape[-1]
    R = int(round((np.sqrt(8.0 * P + 1.0) - 1.0) / 2.0))
    if tri_size(R) != P or b.dtype != _F64 or not b.is_cuda or not b.is_contiguous() or (a is not None and (a.dtype != _F64 or a.numel() != P)) \
            or (coef is not None and (coef.dtype != _F64 or coef.dim() != 1 or coef.numel() < 1)):
        raise ValueError("mixed_inverse: need packed float64 device triangles of one size and a float64 coefficient vector")
    J = b.shape[0] if many else (1 if coef is None else coef.numel())
    out = torch.empty((J, P), dtype=_F64, device=b.device)
    ld = torch.empty((J,), dtype=_F64, device=b.device) if want_logdet else None
    _lib.call("ssv_plda_mixed_inverse", _p(a), _p(b), P if many else 0, _p(coef), _p(out), _p(ld), J, R, ops._stream())
    return out, ld


def compute_eer(target, nontarget):
    """The walk of Kaldi's ``compute-eer`` on the host in float64: both lists sorted ascending; for p = 0, 1, ... while p + 1 < |target|,
    q = |non| - 1 - floor(|non| p / |target|) floored at 0, stopping at the first p with non[q] < target[p].  Returns (eer, threshold) =
    (p / |target|, target[p]).  An empty list is a ``ValueError``."""
    t = np.sort(np.asarray(target, dtype=np.float64).ravel())
    non = np.sort(np.asarray(nontarget, dtype=np.float64).ravel())
    if t.size == 0 or non.size == 0:
        raise ValueError("compute_eer: %d target and %d nontarget scores; both lists must hold some" % (t.size, non.size))
    p = 0
    while p + 1 < t.size:
        q = max(non.size - 1 - (non.size * p) // t.size, 0)
        if non[q] < t[p]:
            break
        p += 1
    return p / t.size, float(t[p])


class Plda:
    """A PLDA model on one device: ``mean`` (R,), ``transform`` A (R, R) and ``psi`` (R,) as float64 tensors, with the float32 plane
    ``At`` = A^T the transform's product reads, rounded once from double."""

    def __init__(self, mean, transform, psi):
        for t, name in ((mean, "mean"), (transform, "transform"), (psi, "psi")):
            if not isinstance(t, torch.Tensor):
                raise ValueError("Plda: %s must be a torch tensor" % name)
        R = mean.numel()
        if mean.dim() != 1 or tuple(transform.shape) != (R, R) or tuple(psi.shape) != (R,) or any(t.dtype != _F64 for t in (mean, transform, psi)):
            raise ValueError("Plda: need float64 mean (R,), transform (R, R), psi (R,); got %s %s, %s %s, %s %s"
                             % (mean.dtype, tuple(mean.shape), transform.dtype, tuple(transform.shape), psi.dtype, tuple(psi.shape)))
        if not 1 <= R <= MAX_R:
            raise ValueError("Plda: R=%d must lie in [1, %d]" % (R, MAX_R))
        if transform.device != mean.device or psi.device != mean.device:
            raise ValueError("Plda: mean, transform and psi must live on one device")
        self.mean, self.A, self.psi = (t.contiguous().clone() for t in (mean, transform, psi))
        self.At = self.A.t().contiguous().to(_F32)

    R = property(lambda self: self.mean.numel())
    device = property(lambda self: self.mean.device)

    # ------------------------------------------------------------------ state
    def state_dict(self):
        return {"mean": self.mean.clone(), "transform": self.A.clone(), "psi": self.psi.clone()}

    def load_state_dict(self, sd):
        other = Plda(*(torch.as_tensor(sd[k]).to(self.device) for k in ("mean", "transform", "psi")))
        if other.R != self.R:
            raise ValueError("Plda.load_state_dict: the state has R=%d, the model R=%d" % (other.R, self.R))
        self.mean, self.A, self.psi, self.At = other.mean, other.A, other.psi, other.At

    def save(self, path):
        """``.npz`` with the float64 ``mean``, ``transform``, ``psi`` (the plane is derived)."""
        np.savez(path, **{k: v.cpu().numpy() for k, v in self.state_dict().items()})

    @classmethod
    def load(cls, path, device="cuda"):
        """``device="cpu"`` gives a state holder only; the operations need a ROCm device."""
        with np.load(path) as z:
            return cls(*(torch.from_numpy(np.asarray(z[k], dtype=np.float64)).to(device) for k in ("mean", "transform", "psi")))

    # ------------------------------------------------------------------ operations
    def transform(self, X, num_examples=1, length_norm=True):
        """``u`` (n, R) float32 of ``X`` (n, R) float32 (``ssv_plda_transform``).  ``num_examples``: one count for all rows, or an int32 device
        vector (a host sequence is uploaded) of the utterances behind each row."""
        ops._dev(self.mean, "Plda.transform: mean")
        X = _matrix(X, "Plda.transform: X", cols=self.R)
        n = X.shape[0]
        nex, nall = None, 0
        if isinstance(num_examples, (int, np.integer)):
            nall = int(num_examples)
            if nall < 1:
                raise ValueError("Plda.transform: num_examples=%d must be at least 1" % nall)
        else:
            nex = torch.as_tensor(num_examples).to(device=X.device, dtype=_I32).contiguous()
            if nex.dim() != 1 or nex.numel() != n:
                raise ValueError("Plda.transform: num_examples must hold one count per row (%d), got %s" % (n, tuple(nex.shape)))
        Xc, U = torch.empty_like(X), torch.empty_like(X)
        _lib.call("ssv_plda_transform", _p(X), _p(self.mean), _p(self.At), _p(self.psi), _p(nex), nall, _p(Xc), _p(U), n, self.R, int(bool(length_norm)), ops._stream())
        return U

    def speaker_models(self, enroll, spk_off):
        """(``y`` (S, R) float32, ``n`` (S,) int32 device): per speaker the mean of its normalised enrolment rows, normalised again
        (``ssv_plda_class_stats``) and transformed with n = the number of its rows."""
        enroll = _matrix(enroll, "Plda.speaker_models: enroll", cols=self.R)
        off, host = _offsets(spk_off, "Plda.speaker_models: spk_off", enroll.device, total=enroll.shape[0])
        _, _, _, model = class_stats(enroll, off if host is None else host, True, residuals=False, means=False, model=True)
        n = (off[1:] - off[:-1]).clamp_(min=0).to(_I32)
        return self.transform(model, n, length_norm=False), n

    def planes(self, y, n):
        """(``H`` (S, 2R) float32, ``k`` (S,) float64) of transformed speaker models (``ssv_plda_speaker_planes``)."""
        y = _matrix(y, "Plda.planes: y", cols=self.R)
        S = y.shape[0]
        n = torch.as_tensor(n).to(device=y.device, dtype=_I32).contiguous()
        if n.dim() != 1 or n.numel() != S:
            raise ValueError("Plda.planes: n must hold one count per speaker (%d), got %s" % (S, tuple(n.shape)))
        H = torch.empty((S, 2 * self.R), dtype=_F32, device=y.device)
        k = torch.empty((S,), dtype=_F64, device=y.device)
        _lib.call("ssv_plda_speaker_planes", _p(y), _p(n), _p(self.psi), _p(H), _p(k), S, self.R, ops._stream())
        return H, k

    def score_planes(self, H, k, evalv_transformed, out=None):
        """``scores`` (E, S) float32 = [t^2, t] H^T + k (``ssv_plda_score``)."""
        T = _matrix(evalv_transformed, "Plda.score: eval vectors", cols=self.R)
        E, S = T.shape[0], H.shape[0]
        if out is None:
            out = torch.empty((E, S), dtype=_F32, device=T.device)
        _lib.call("ssv_plda_score", _p(T), _p(H), _p(k), _p(out), E, S, self.R, ops._stream())
        return out

    def score(self, y, n, evalv_transformed):
        """``scores`` (E, S) float32: the log-likelihood ratio of every transformed eval vector against every speaker model (y, n)."""
        H, k = self.planes(y, n)
        return self.score_planes(H, k, evalv_transformed)

    def trials(self, enroll, spk_off, evalv):
        """The whole scoring chain: speaker models of ``enroll`` (n, R) by ``spk_off``, ``evalv`` (E, R) normalised and transformed with
        n = 1, scores (E, S) float32."""
        y, n = self.speaker_models(enroll, spk_off)
        return self.score(y, n, self.transform(evalv, 1, True))


class PldaEstimator:
    """EM for the two-covariance model on ``X`` (n, R) float32 device vectors of S speakers (``spk_off``: S + 1 ascending offsets).  The
    statistics are taken once: residual rows, means, mu (``ssv_plda_class_stats``) and the scatter of the residuals
    (``ssv_ivec_product_tn``).  ``W`` and ``B`` are packed float64 device triangles, starting from the identity: views of one (2, P) tensor,
    to be written in place (``W.copy_``)."""

    def __init__(self, X, spk_off, length_norm=True):
        X = _matrix(X, "PldaEstimator: X")
        n, R = X.shape
        if not 1 <= R <= MAX_R:
            raise ValueError("PldaEstimator: R=%d must lie in [1, %d]" % (R, MAX_R))
        off, host = _offsets(spk_off, "PldaEstimator: spk_off", X.device, total=n)
        if host is None:
            host = off.cpu().numpy()
        counts = np.clip(np.diff(np.clip(host, 0, n)), 0, None)
        if not (counts > 0).any():
            raise ValueError("PldaEstimator: no speaker has rows")
        dev = X.device
        self.R, self.P, self.S, self.dev = R, tri_size(R), counts.size, dev
        self.Sn, self.N = int((counts > 0).sum()), int(counts.sum())
        distinct = np.unique(counts[counts > 0])
        self.J = distinct.size
        cls = np.searchsorted(distinct, counts).astype(np.int32)
        cls[counts == 0] = -1
        nspk = np.array([(counts == c).sum() for c in distinct], dtype=np.float64)
        self.cnt, self.cls = torch.from_numpy(counts.astype(np.int32)).to(dev), torch.from_numpy(cls).to(dev)
        self.coef = torch.from_numpy(distinct.astype(np.float64)).to(dev)
        self.nspk, self.nrow = torch.from_numpy(nspk).to(dev), torch.from_numpy(nspk * distinct).to(dev)
        self.cw = torch.from_numpy(counts.astype(np.float64)).to(dev)           # wsyrk weights of the r rows (0 for a speaker without rows)
        Xd, self.means, self.mu, _ = class_stats(X, off if host is None else host, length_norm)
        self.Sigma = torch.zeros((R, R), dtype=_F64, device=dev)
        product_tn(Xd, Xd, self.Sigma)
        eye = torch.from_numpy(tri_pack(np.eye(R))).to(dev)
        self.WB = torch.stack([eye, eye])                                      # W and B side by side: one launch inverts both
        self.W, self.B = self.WB[0], self.WB[1]
        self.w = torch.empty((self.S, R), dtype=_F64, device=dev)
        self.r = torch.empty((self.S, R), dtype=_F64, device=dev)
        self.quad = torch.empty((self.S,), dtype=_F64, device=dev)

    def _estep(self):
        """Everything an iteration needs under the current W, B: W^-1, B^-1 and their log-determinants, the mixed inverses per distinct
        count, and per speaker w, r and the quadratic form.  Three launches."""
        st = ops._stream()
        inv, ld = mixed_inverse(None, self.WB)
        self.Winv, self.Binv, self.ldW, self.ldB = inv[0], inv[1], ld[0:1], ld[1:2]
        self.Mx, self.ldMx = mixed_inverse(self.Binv, self.Winv, self.coef)
        _lib.call("ssv_plda_em_classes", _p(self.means), _p(self.mu), _p(self.cnt), _p(self.cls), _p(self.Mx), _p(self.Winv), _p(self.w), _p(self.r), _p(self.quad),
                  self.S, self.J, self.R, st)

    def _update(self, update, obj):
        _lib.call("ssv_plda_em_update", _p(self.Mx), _p(self.ldMx), _p(self.nspk), _p(self.nrow), _p(self.WW if update else None), _p(self.RR if update else None),
                  _p(self.Sigma), _p(self.Winv), _p(self.ldW), _p(self.ldB), _p(self.cnt), _p(self.cls), _p(self.quad), _p(self.W if update else None),
                  _p(self.B if update else None), _p(obj), self.J, self.S, self.R, float(self.Sn), float(self.N), ops._stream())

    def objective(self):
        """The objective under the current W and B, a float64 device scalar."""
        self._estep()
        obj = torch.empty((1,), dtype=_F64, device=self.dev)
        self._update(False, obj)
        return obj[0]

    def em_step(self):
        """One EM iteration; returns the objective under the parameters BEFORE the update, a float64 device scalar.  Nothing is read on the
        host."""
        self._estep()
        st = ops._stream()
        self.WW = torch.zeros((self.R, self.R), dtype=_F64, device=self.dev)
        self.RR = torch.zeros((self.R, self.R), dtype=_F64, device=self.dev)
        _lib.call("ssv_plda_wsyrk_f64", _p(self.w), None, _p(self.WW), self.S, self.R, st)
        _lib.call("ssv_plda_wsyrk_f64", _p(self.r), _p(self.cw), _p(self.RR), self.S, self.R, st)
        obj = torch.empty((1,), dtype=_F64, device=self.dev)
        self._update(True, obj)
        return obj[0]

    def finalize(self):
        """(mu, A, psi) from the current W and B, on the host in float64: W = C C^T, C^-1 B C^-T = U diag(psi) U^T, psi floored at 0 and sorted
        descending, A = U^T C^-1, each row's sign fixed so that its entry of largest magnitude is positive."""
        A, psi = finalize_host(tri_unpack(self.W.cpu().numpy(), self.R), tri_unpack(self.B.cpu().numpy(), self.R))
        return Plda(self.mu.clone(), torch.from_numpy(A).to(self.dev), torch.from_numpy(psi).to(self.dev))


def finalize_host(W, B):
    """The simultaneous diagonalisation of float64 host matrices W and B: returns (A, psi) with A W A^T = I and A B A^T = diag(psi)."""
    C = np.linalg.cholesky(W)
    Ci = np.linalg.inv(C)
    M = Ci @ B @ Ci.T
    psi, U = np.linalg.eigh(0.5 * (M + M.T))
    order = np.argsort(-psi, kind="stable")
    psi, U = np.maximum(psi[order], 0.0), U[:, order]
    A = U.T @ Ci
    big = np.abs(A).argmax(axis=1)
    A = A * np.where(A[np.arange(A.shape[0]), big] < 0, -1.0, 1.0)[:, None]
    return np.ascontiguousarray(A), np.ascontiguousarray(psi)


def train_plda(X, spk_off, iters=10, length_norm=True, log=print):
    """``iters`` EM iterations from W = B = I (``ivector-compute-plda``'s --num-em-iters is 10), then ``finalize``.  Returns (``Plda``, history):
    ``iters + 1`` objectives, one before each update and one after the last, host floats -- read as they come when ``log`` is given, at the
    end otherwise."""
    est = PldaEstimator(X, spk_off, length_norm)
    hist = []
    for it in range(int(iters)):
        hist.append(est.em_step())
        if log:
            hist[-1] = float(hist[-1])
            log("plda EM %d/%d: objective per vector %.6f" % (it + 1, iters, hist[-1]))
    hist.append(est.objective())
    hist = [float(h) for h in hist]
    if log:
        log("plda EM: final objective per vector %.6f" % hist[-1])
    return est.finalize(), hist
