"""The PLDA back end on the device against the float64 restatement (tests/_plda_ref.py): class statistics, the mixed inverse, one EM
iteration piece by piece and ten whole, the transform, the speaker planes and the score, the model's round trip through a file, and the
whole chain to the spoof-rate curve and the equal error rate.  Every bar is recorded or derived in _plda_ref.py.  Outputs are poisoned
(NaN) and sit between guard zones that must come back whole."""
import functools

import numpy as np
import pytest
import torch

import _plda_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64


def _pl():
    from spoofsv_amd import plda
    return plda


def _call(name, *args):
    from spoofsv_amd import _lib
    _lib.call(name, *args)


def _p(t):
    from spoofsv_amd import ops
    return ops._p(t)


def _st():
    from spoofsv_amd import ops
    return ops._stream()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pack(M):
    i, j = np.tril_indices(M.shape[-1])
    return np.ascontiguousarray(M[..., i, j])


def _unpack(p):
    from spoofsv_amd.ivector import tri_unpack
    return tri_unpack(p)


def _rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


class Guarded:
    """A poisoned output of ``shape`` between two guard zones of GUARD elements holding -7."""

    def __init__(self, shape, dtype=torch.float32, fill=float("nan")):
        n = int(np.prod(shape))
        self.whole = torch.full((n + 2 * GUARD,), -7.0, dtype=dtype, device=DEV)
        self.t = self.whole[GUARD:GUARD + n].view(shape)
        self.t.fill_(fill)

    def intact(self):
        return bool((self.whole[:GUARD] == -7).all() and (self.whole[-GUARD:] == -7).all())

    def numpy(self):
        return self.t.cpu().numpy()


# ================================================================================================ class statistics
@pytest.mark.parametrize("Rk", R.STATS_RANKS)
def test_class_stats(Rk):
    X, off = R.stats_case(Rk)
    n, S = X.shape[0], len(off) - 1
    X = np.concatenate([X, np.ones((2, Rk), np.float32)])          # two rows no speaker owns
    Xd, means, mu, model = Guarded((n + 2, Rk)), Guarded((S, Rk), torch.float64), Guarded((Rk,), torch.float64), Guarded((S, Rk))
    Xg, offg = _dev(X), _dev(off)
    _call("ssv_plda_class_stats", _p(Xg), _p(offg), off.ctypes.data, _p(Xd.t), _p(means.t), _p(mu.t), _p(model.t), n + 2, S, Rk, 1, _st())
    assert Xd.intact() and means.intact() and mu.intact() and model.intact()
    rXd, rmeans, rmu, counts = R.class_stats(X[:n], off)
    gXd, gmeans, gmu, gmodel = Xd.numpy(), means.numpy(), mu.numpy(), model.numpy()
    empty = int(np.nonzero(counts == 0)[0][0])
    assert np.isnan(gmeans[empty]).all() and np.isnan(gXd[n:]).all() and (gmodel[empty] == 0).all()        # untouched; a zero model row
    live = counts > 0
    big = np.abs(R.normalise(X[:n])).max()
    e_mean, e_mu = np.abs(gmeans[live] - rmeans[live]).max() / np.abs(rmeans).max(), np.abs(gmu - rmu).max() / np.abs(rmeans).max()
    print("class stats R=%d: means %.2e, mu %.2e of the largest entry (bar %.0e)" % (Rk, e_mean, e_mu, R.BAR_MEAN))
    assert e_mean <= R.BAR_MEAN and e_mu <= R.BAR_MEAN
    assert np.isfinite(gXd[:n]).all() and (np.abs(gXd[:n] - rXd) <= R.BAR_ROUND * np.abs(rXd) + R.BAR_MEAN * big).all()
    assert np.array_equal(rXd[off[2] + 1], -rmeans[2])                 # (the case's zero vector stays zero: its residual is -m)
    rmodel = R.model_rows(X[:n], off)
    assert (np.abs(gmodel - rmodel) <= R.BAR_ROUND * np.abs(rmodel) + R.BAR_MEAN * np.sqrt(Rk)).all()
    # the scatter of the device's own residuals, by the existing transposed product
    from spoofsv_amd.ivector import product_tn
    Sigma = torch.zeros((Rk, Rk), dtype=torch.float64, device=DEV)
    product_tn(Xd.t[:n], Xd.t[:n], Sigma)
    d = gXd[:n].astype(np.float64)
    err = float((np.abs(Sigma.cpu().numpy() - d.T @ d) / np.maximum(np.abs(d).T @ np.abs(d), 1e-300)).max())
    print("scatter R=%d: %.3e of sum |d||d|, bar %.3e" % (Rk, err, R.bar(R.MEASURED_SCATTER[Rk])))
    assert err <= R.bar(R.MEASURED_SCATTER[Rk])
    # without length normalisation, means alone
    m2 = Guarded((S, Rk), torch.float64)
    _call("ssv_plda_class_stats", _p(Xg), _p(offg), None, None, _p(m2.t), None, None, n + 2, S, Rk, 0, _st())
    want = R.class_stats(X[:n], off, False)[1]
    assert m2.intact() and np.abs(m2.numpy()[live] - want[live]).max() <= R.BAR_MEAN * np.abs(want).max()


# ================================================================================================ the mixed inverse
@pytest.mark.parametrize("J", (1, 5))
@pytest.mark.parametrize("Rk", R.INVERSE_RANKS)
def test_mixed_inverse(Rk, J):
    _, a, b = R.model_case(Rk, seed=3)
    coef = np.array([0.5, 1.0, 2.0, 3.0, 9.0])[:J]
    P = Rk * (Rk + 1) // 2
    out, ld = Guarded((J, P), torch.float64), Guarded((J,), torch.float64)
    ag, bg, cg = _dev(_pack(a)), _dev(_pack(b)), _dev(coef)                # (held: a tensor dropped before the call gives its memory to the next)
    _call("ssv_plda_mixed_inverse", _p(ag), _p(bg), 0, _p(cg), _p(out.t), _p(ld.t), J, Rk, _st())
    assert out.intact() and ld.intact()
    got, gld = _unpack(out.numpy()), ld.numpy()
    for j in range(J):
        M = a + coef[j] * b
        e, el = _rel(got[j], np.linalg.inv(M)), abs(gld[j] - np.linalg.slogdet(M)[1]) / max(1.0, abs(np.linalg.slogdet(M)[1]))
        assert e <= R.BAR_F64 and el <= R.BAR_F64, (Rk, j, e, el)
    # plain inverses of two matrices side by side, no coefficients, no log-determinant
    plain, both = Guarded((2, P), torch.float64), _dev(np.stack([_pack(b), _pack(a)]))
    _call("ssv_plda_mixed_inverse", None, _p(both), P, None, _p(plain.t), None, 2, Rk, _st())
    assert plain.intact() and _rel(_unpack(plain.numpy())[0], np.linalg.inv(b)) <= R.BAR_F64 and _rel(_unpack(plain.numpy())[1], np.linalg.inv(a)) <= R.BAR_F64


def test_mixed_inverse_nan_poisons_its_own_matrix_only():
    Rk, J = 17, 5
    _, a, b = R.model_case(Rk, seed=3)
    P = Rk * (Rk + 1) // 2
    for coef in (np.array([0.5, 1.0, np.nan, 3.0, 9.0]), np.array([0.5, 1.0, -50.0, 3.0, 9.0])):      # a NaN; a matrix that is not positive definite
        out, ld = Guarded((J, P), torch.float64, fill=5.0), Guarded((J,), torch.float64, fill=5.0)
        ag, bg, cg = _dev(_pack(a)), _dev(_pack(b)), _dev(coef)
        _call("ssv_plda_mixed_inverse", _p(ag), _p(bg), 0, _p(cg), _p(out.t), _p(ld.t), J, Rk, _st())
        got, gld = out.numpy(), ld.numpy()
        assert out.intact() and ld.intact() and np.isnan(got[2]).all() and np.isnan(gld[2])
        for j in (0, 1, 3, 4):
            assert _rel(_unpack(got[j]), np.linalg.inv(a + coef[j] * b)) <= R.BAR_F64 and np.isfinite(gld[j])


# ================================================================================================ EM
def _estimator(Rk, S):
    X, off = R.train_case(Rk, S)
    est = _pl().PldaEstimator(_dev(X), off)
    return est, est.Sigma.cpu().numpy(), est.means.cpu().numpy(), est.mu.cpu().numpy(), np.diff(off)


@pytest.mark.parametrize("shape", R.EM_SHAPES)
def test_one_em_iteration_piece_by_piece(shape):
    Rk, S = shape
    est, Sigma, means, mu, counts = _estimator(Rk, S)
    _, W, B = R.model_case(Rk, seed=1)
    est.W.copy_(_dev(_pack(W)))
    est.B.copy_(_dev(_pack(B)))
    est._estep()
    terms = R.speaker_terms(means, mu, counts, W, B)
    errs = {"Winv": _rel(_unpack(est.Winv.cpu().numpy()), np.linalg.inv(W)), "Binv": _rel(_unpack(est.Binv.cpu().numpy()), np.linalg.inv(B))}
    distinct = np.unique(counts)
    Mx, ldMx = _unpack(est.Mx.cpu().numpy()), est.ldMx.cpu().numpy()
    Winv, Binv = np.linalg.inv(W), np.linalg.inv(B)
    errs["Mx"] = max(_rel(Mx[j], np.linalg.inv(Binv + n * Winv)) for j, n in enumerate(distinct))
    errs["ldMx"] = max(abs(ldMx[j] - np.linalg.slogdet(Binv + n * Winv)[1]) / max(1.0, abs(ldMx[j])) for j, n in enumerate(distinct))
    w, r, quad = est.w.cpu().numpy(), est.r.cpu().numpy(), est.quad.cpu().numpy()
    rw, rr, rq = (np.array([t[i] for t in terms]) for i in (3, 4, 6))
    errs["w"], errs["r"], errs["quad"] = _rel(w, rw), _rel(r, rr), _rel(quad, rq)
    # log|B + W/n| as the objective kernel assembles it
    ldW, ldB = float(est.ldW[0]), float(est.ldB[0])
    errs["logdet"] = max(abs(ldW - Rk * np.log(n) + ldB + ldMx[np.searchsorted(distinct, n)] - ld) / max(1.0, abs(ld)) for _, n, _, _, _, ld, _ in terms)
    obj = float(est.em_step())
    robj, rW, rB = R.em_step(Sigma, means, mu, counts, W, B)
    errs["WW"] = _rel(est.WW.cpu().numpy(), sum(np.outer(t[3], t[3]) for t in terms))
    errs["RR"] = _rel(est.RR.cpu().numpy(), sum(t[1] * np.outer(t[4], t[4]) for t in terms))
    errs["W"], errs["B"] = _rel(_unpack(est.W.cpu().numpy()), rW), _rel(_unpack(est.B.cpu().numpy()), rB)
    errs["obj"] = abs(obj - robj) / max(1.0, abs(robj))
    print("EM pieces at %s: %s (bar %.0e)" % (shape, ", ".join("%s %.2e" % kv for kv in errs.items()), R.BAR_F64))
    assert all(e <= R.BAR_F64 for e in errs.values()), errs
    assert abs(float(est.objective()) - R.objective(Sigma, means, mu, counts, rW, rB)) <= R.BAR_F64 * max(1.0, abs(robj))


def test_wsyrk_adds_to_what_is_there():
    rng = np.random.default_rng(4)
    for S, Rk in ((1, 1), (65, 17), (130, 33)):
        V, c = rng.standard_normal((S, Rk)), rng.uniform(0, 9, S)
        acc = Guarded((Rk, Rk), torch.float64, fill=3.0)
        Vg, cg = _dev(V), _dev(c)
        _call("ssv_plda_wsyrk_f64", _p(Vg), _p(cg), _p(acc.t), S, Rk, _st())
        assert acc.intact() and _rel(acc.numpy() - 3.0, (V.T * c) @ V) <= R.BAR_F64


def test_ten_em_iterations():
    Rk, S = R.EM_SHAPES[0]
    X, off = R.train_case(Rk, S)
    logged = []
    model, hist = _pl().train_plda(_dev(X), off, iters=10, log=logged.append)
    est, Sigma, means, mu, counts = _estimator(Rk, S)
    assert set(counts) == set(range(1, 10))
    dev_hist = [float(est.em_step()) for _ in range(10)] + [float(est.objective())]
    assert dev_hist == hist and len(logged) == 11
    rhist, rW, rB = R.em_fit(Sigma, means, mu, counts, 10)
    scale = 1.0 + np.abs(rhist).max()
    eW, eB, eh = _rel(_unpack(est.W.cpu().numpy()), rW), _rel(_unpack(est.B.cpu().numpy()), rB), float(np.abs(np.array(hist) - rhist).max() / scale)
    print("10 EM iterations at %s: W %.2e, B %.2e, history %.2e (bar %.0e); history %s" % ((Rk, S), eW, eB, eh, R.BAR_F64, " ".join("%.6f" % h for h in hist)))
    assert eW <= R.BAR_F64 and eB <= R.BAR_F64 and eh <= R.BAR_F64
    assert (np.diff(hist) >= -R.BAR_F64 * scale).all()
    A, psi = R.finalize(_unpack(est.W.cpu().numpy()), _unpack(est.B.cpu().numpy()))
    assert np.array_equal(model.A.cpu().numpy(), A) and np.array_equal(model.psi.cpu().numpy(), psi) and np.array_equal(model.mean.cpu().numpy(), mu)


# ================================================================================================ the transform
@functools.lru_cache(maxsize=None)
def _transform_ref(Rk):
    X, mu, A, psi, nex = R.transform_case(130, Rk)
    X2 = X.copy()
    X2[65] = X[0]
    return X, X2, mu, A, psi, nex, R.transform(X2, mu, A, psi, nex, True), R.transform(X, mu, A, psi, 3, False)


@pytest.mark.parametrize("n", (63, 64, 65, 130))
@pytest.mark.parametrize("Rk", R.TRANSFORM_RANKS)
def test_transform(Rk, n):
    X, X2, mu, A, psi, nex, want_rows, want_all = _transform_ref(Rk)
    model = _pl().Plda(_dev(mu), _dev(A), _dev(psi))
    bars = [R.bar(m) for m in R.MEASURED_TRANSFORM[Rk]]
    # per-row counts, length-normalised, through the entry itself
    U, Xc = Guarded((n, Rk)), Guarded((n, Rk))
    Xg, nexg = _dev(X2[:n]), _dev(nex[:n])
    _call("ssv_plda_transform", _p(Xg), _p(model.mean), _p(model.At), _p(model.psi), _p(nexg), 0, _p(Xc.t), _p(U.t), n, Rk, 1, _st())
    got = U.numpy().astype(np.float64)
    e1 = R.transform_error(got, want_rows[:n])
    assert U.intact() and Xc.intact() and np.isfinite(got).all() and e1 <= bars[0], (e1, bars[0])
    # one count for all rows, not normalised; the row equal to mu comes back zero (its factor is 1)
    got2 = model.transform(_dev(X[:n]), 3, length_norm=False).cpu().numpy().astype(np.float64)
    e2 = R.transform_error(got2, want_all[:n])
    print("transform R=%d n=%d: %.3e (bar %.3e), plain %.3e (bar %.3e)" % (Rk, n, e1, bars[0], e2, bars[1]))
    assert np.isfinite(got2).all() and e2 <= bars[1], (e2, bars[1])
    if n > 65:
        assert (got2[65] == 0).all()
    # a row alone gives the same bits
    alone = model.transform(_dev(X2[n // 2:n // 2 + 1]), int(nex[n // 2]), True)
    assert torch.equal(alone[0], U.t[n // 2])


# ================================================================================================ planes and score
@functools.lru_cache(maxsize=None)
def _score_ref(Rk):
    t, y, n, psi = R.score_case(R.SCORE_SHAPE[0], R.SCORE_SHAPE[1], Rk)
    H, k = R.planes(y, n, psi)
    return t, y, n, psi, R.score_direct(t, y, n, psi), R.term_scale(t, H, k), H, k


@pytest.mark.parametrize("S", (1, 64, 65))
@pytest.mark.parametrize("E", (1, 63, 65, 130))
@pytest.mark.parametrize("Rk", R.SCORE_RANKS)
def test_speaker_planes_and_score(Rk, E, S):
    t, y, n, psi, want, scale, rH, rk = _score_ref(Rk)
    model = _pl().Plda(_dev(np.zeros(Rk)), _dev(np.eye(Rk)), _dev(psi))
    H, k, out = Guarded((S, 2 * Rk)), Guarded((S,), torch.float64), Guarded((E, S))
    tg, yg, ng = _dev(t[:E]), _dev(y[:S]), _dev(n[:S])
    _call("ssv_plda_speaker_planes", _p(yg), _p(ng), _p(model.psi), _p(H.t), _p(k.t), S, Rk, _st())
    gH, gk = H.numpy(), k.numpy()
    assert H.intact() and k.intact()
    assert (np.abs(gH - rH[:S]) <= R.BAR_ROUND * np.abs(rH[:S]) + 1e-12 * np.abs(rH[:S]).max()).all()
    assert (np.abs(gk - rk[:S]) <= R.BAR_F64 * np.maximum(1.0, np.abs(rk[:S]))).all()
    _call("ssv_plda_score", _p(tg), _p(H.t), _p(k.t), _p(out.t), E, S, Rk, _st())
    got = out.numpy()
    err = float((np.abs(got - want[:E, :S]) / np.maximum(scale[:E, :S], 1e-300)).max())
    assert out.intact() and np.isfinite(got).all() and err <= R.bar(R.MEASURED_SCORE[Rk]), (err, R.bar(R.MEASURED_SCORE[Rk]))
    if S > 2:
        assert n[2] == 0 and (gH[2] == 0).all() and gk[2] == 0 and (got[:, 2] == 0).all() and not np.signbit(got[:, 2]).any()
    assert torch.equal(model.score(yg, ng, tg), out.t)
    # each row scored alone is the same bits
    for e in sorted({0, E // 2, E - 1}):
        assert torch.equal(model.score_planes(H.t, k.t, tg[e:e + 1])[0], out.t[e])


@pytest.mark.parametrize("Rk", (17, 129, 192))          # K = 2 R: two past a staged step of 32, two past a run of 256, the largest rank
def test_score_is_the_product_tile(Rk):
    """ssv_plda_score and ssv_ivec_product are ONE tile (csrc/exact_product.h): with k = 0 the score equals the plain product of
    [t^2, t] (t^2 one float32 product, as the score's loader makes it) with H^T bit for bit -- the same values staged at the same LDS
    positions, the same MFMA sequence, the folds into double at the same steps, and (float)(sum + 0.0) is (float)sum."""
    E, S = 65, 63
    t, y, n, psi = R.score_case(E, S, Rk)
    tg, Hg, kg = _dev(t), _dev(R.planes(y, n, psi)[0].astype(np.float32)), torch.zeros(S, dtype=torch.float64, device=DEV)
    score, prod = Guarded((E, S)), Guarded((E, S))
    _call("ssv_plda_score", _p(tg), _p(Hg), _p(kg), _p(score.t), E, S, Rk, _st())
    left, right = torch.cat([tg * tg, tg], 1).contiguous(), Hg.t().contiguous()
    _call("ssv_ivec_product", _p(left), _p(right), _p(prod.t), E, S, 2 * Rk, _st())
    assert score.intact() and prod.intact() and np.isfinite(score.numpy()).all() and np.abs(score.numpy()).max() > 0
    assert np.array_equal(score.numpy().view(np.int32), prod.numpy().view(np.int32))


# ================================================================================================ the model's file and the chain
@functools.lru_cache(maxsize=None)
def _chain():
    Xtr, off, enroll, en_lines, evalv, ev_lines = R.chain_case()
    model, hist = _pl().train_plda(_dev(Xtr), off, iters=R.CHAIN_SHAPE["iters"], log=None)
    return model, hist, enroll, en_lines, evalv, ev_lines


def test_save_load_round_trip(tmp_path):
    model, _, enroll, _, evalv, _ = _chain()
    eoff = np.arange(0, enroll.shape[0] + 1, R.CHAIN_SHAPE["enroll"])
    before = model.trials(_dev(enroll), eoff, _dev(evalv))
    path = str(tmp_path / "plda.npz")
    model.save(path)
    loaded = _pl().Plda.load(path, DEV)
    for a, b in zip(model.state_dict().values(), loaded.state_dict().values()):
        assert torch.equal(a, b)
    assert torch.equal(loaded.trials(_dev(enroll), eoff, _dev(evalv)), before)
    other = _pl().Plda(_dev(np.zeros(model.R)), _dev(np.eye(model.R)), _dev(np.ones(model.R)))
    other.load_state_dict(model.state_dict())
    assert torch.equal(other.trials(_dev(enroll), eoff, _dev(evalv)), before)


def test_chain_to_curve_and_eer(tmp_path):
    from spoofsv_amd import ge2e_harness as H
    from spoofsv_amd import ivector
    s = R.CHAIN_SHAPE
    model, hist, enroll, en_lines, evalv, ev_lines = _chain()
    assert len(hist) == s["iters"] + 1 and (np.diff(hist) >= -R.BAR_F64 * (1.0 + np.abs(hist).max())).all()
    path = str(tmp_path / "plda.score")
    out = H.ivector_trials(_dev(enroll), en_lines, _dev(evalv), ev_lines, path, plda=model)
    # the reference scores under the device's model, in float64 by the direct form
    mu, A, psi = (model.state_dict()[k].cpu().numpy() for k in ("mean", "transform", "psi"))
    eoff = np.arange(0, enroll.shape[0] + 1, s["enroll"])
    want, scale = R.trials(enroll, eoff, evalv, mu, A, psi)
    got = out["scores"].cpu().numpy().astype(np.float64)
    b = R.bar(R.MEASURED_CHAIN) * scale
    print("chain: worst score error %.3e of the term scale, bar %.3e" % (float((np.abs(got - want) / scale).max()), R.bar(R.MEASURED_CHAIN)))
    assert got.shape == (len(ev_lines), s["S_test"]) and (np.abs(got - want) <= b).all()
    # the curve over curve.py's own thresholds: its counts between those of the reference scores moved down and up by the bar
    thr = np.array(H.curve_thresholds("ivector"))
    assert out["thresholds"] == H.curve_thresholds("ivector") and out["counts"].shape == (8000, 2)
    spk = np.repeat(np.arange(s["S_test"]), s["real"] + s["spoof"])
    fake = np.tile(np.arange(s["real"] + s["spoof"]) >= s["real"], s["S_test"])
    own = lambda m: m[np.arange(len(spk)), spk]
    for col, rows in ((0, ~fake), (1, fake)):
        lo = (own(want - b)[rows][None, :] > thr[:, None]).sum(1)
        hi = (own(want + b)[rows][None, :] > thr[:, None]).sum(1)
        assert (lo <= out["counts"][:, col]).all() and (out["counts"][:, col] <= hi).all()
    assert out["counts"][:, 0].max() > 0
    # the equal error rate: compute_eer on the device's own scores, by the trial list's labels
    target = np.array([line.split()[2] == "target" for line in ivector.trial_list(ev_lines)]).reshape(got.shape)
    assert (out["eer"], out["eer_threshold"]) == _pl().compute_eer(got[target], got[~target]) == R.compute_eer(got[target], got[~target])
    assert out["eer"] < 0.5
    e2, t2 = H.ivector_eer(path, ivector.trial_list(ev_lines))           # the same from the file, whose scores carry 9 significant digits
    assert e2 == out["eer"] and abs(t2 - out["eer_threshold"]) <= 1e-8 * max(1.0, abs(t2))
    # without plda= the function is what it was: cosine scores, thresholds required, the same keys
    cos_thr = [-1.0 + 0.01 * i for i in range(200)]
    old = H.ivector_trials(_dev(enroll), en_lines, _dev(evalv), ev_lines, str(tmp_path / "cos.score"), cos_thr)
    assert sorted(old) == ["counts", "gt_frr", "scores", "speakers", "spoof_rate", "thresholds"]
    assert torch.equal(old["scores"], ivector.cosine_trials(_dev(enroll), eoff, _dev(evalv)))
    with pytest.raises(TypeError):
        H.ivector_trials(_dev(enroll), en_lines, _dev(evalv), ev_lines, str(tmp_path / "none.score"))
