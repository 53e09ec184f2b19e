"""The i-vector extractor on the device against the float64 restatement (tests/_ivector_tv_ref.py): the planes, the centring, the product
family, the E-step, the M-step, EM, extraction from frames in passes, cosine scoring and the whole chain to the spoof-rate curve.  Every
bar is recorded or derived in _ivector_tv_ref.py.  Outputs are poisoned (NaN / -7) and sit between guard zones that must come back whole."""
import functools

import numpy as np
import pytest
import torch

import _ivector_tv_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64


def _iv():
    from spoofsv_amd import ivector
    return ivector


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


def _tv(T, var, w=None, mu=None):
    C, D, _ = T.shape
    w = np.full(C, 1.0 / C) if w is None else w
    mu = np.zeros((C, D)) if mu is None else mu
    return _iv().TotalVariability(_dev(T), _dev(w), _dev(mu), _dev(var))


# ================================================================================================ products
@pytest.mark.parametrize("shape", R.PRODUCT_SHAPES)
def test_plain_product(shape):
    m, n, K = shape
    a, b = R.product_case(m, n, K)
    ad, bd = _dev(a), _dev(b)
    out = Guarded((m, n))
    _call("ssv_ivec_product", _p(ad), _p(bd), _p(out.t), m, n, K, _st())
    got = out.numpy()
    err = R.product_error(got, a.astype(np.float64), b.astype(np.float64))
    print("product %s: error %.3e of sum |a||b|, bar %.3e" % (shape, err, R.bar(R.MEASURED_PRODUCT[shape])))
    assert out.intact() and np.isfinite(got).all() and err <= R.bar(R.MEASURED_PRODUCT[shape])
    again = Guarded((m, n))
    _call("ssv_ivec_product", _p(ad), _p(bd), _p(again.t), m, n, K, _st())
    assert torch.equal(again.t, out.t)
    # a row does not depend on the rows that share its launch
    r = m // 2
    alone = _iv().product(ad[r:r + 1].contiguous(), bd)
    assert torch.equal(alone[0], out.t[r])


@pytest.mark.parametrize("shape", R.PRODUCT_TN_SHAPES)
def test_transposed_product_over_two_passes(shape):
    m, n, K = shape
    a, b = R.product_tn_case(m, n, K)                      # a (K, m), b (K, n)
    ad, bd = _dev(a), _dev(b)
    want = a.T.astype(np.float64) @ b.astype(np.float64)
    scale = np.abs(a.T.astype(np.float64)) @ np.abs(b.astype(np.float64))
    cut = K // 2
    runs = []
    for _ in range(2):
        acc = Guarded((m, n), dtype=torch.float64, fill=3.0)              # += : what the accumulator held stays in
        for u0, u1 in ((0, cut), (cut, K)):
            if u1 > u0:
                _call("ssv_ivec_product_tn", _p(ad[u0:u1].contiguous()), _p(bd[u0:u1].contiguous()), _p(acc.t), u1 - u0, m, n, _st())
        assert acc.intact()
        runs.append(acc.numpy())
    err = float((np.abs(runs[0] - 3.0 - want) / scale).max())
    print("product_tn %s in two passes: error %.3e of sum |a||b|, bar %.3e" % (shape, err, R.bar(R.MEASURED_PRODUCT_TN[shape])))
    assert err <= R.bar(R.MEASURED_PRODUCT_TN[shape]) and np.array_equal(runs[0], runs[1])
    one = torch.zeros((m, n), dtype=torch.float64, device=DEV)
    _iv().product_tn(ad, bd, one)
    assert float((np.abs(one.cpu().numpy() - want) / scale).max()) <= R.bar(R.MEASURED_PRODUCT_TN[shape])


# ================================================================================================ planes and centring
@pytest.mark.parametrize("C,D,Rk", [(5, 7, 1), (8, 5, 17), (3, 4, 192)])
def test_planes(C, D, Rk):
    rng = np.random.default_rng(C + D + Rk)
    T, var = rng.normal(0, 1, (C, D, Rk)), rng.uniform(0.5, 2.0, (C, D))
    G, Pk = Guarded((C * D, Rk)), Guarded((C, Rk * (Rk + 1) // 2))
    Td, vd = _dev(T), _dev(var)
    _call("ssv_ivec_tv_planes", _p(Td), _p(vd), _p(G.t), _p(Pk.t), C, D, Rk, _st())
    G64, Pk64 = R.planes(T, var)
    Pabs = R.planes(np.abs(T), var)[1]
    # each is a float64 value rounded once (2^-24 of itself, at most of the sum of its terms' magnitudes); the double sum's order may move
    # the value by D 2^-53 of that sum, which can only flip the rounding: 2^-23
    eg, ep = float((np.abs(G.numpy() - G64) / np.abs(G64)).max()), float((np.abs(Pk.numpy() - Pk64) / Pabs).max())
    print("planes (%d, %d, %d): G %.3e, Pk %.3e, bar %.3e" % (C, D, Rk, eg, ep, 2.0 ** -23))
    assert G.intact() and Pk.intact() and eg <= 2.0 ** -23 and ep <= 2.0 ** -23


def test_centring_is_one_rounding():
    N, F, _, mu, _, _, _ = R.stats_case(5, 7, 3, 9, seed=2, empty=4)
    iv = _iv()
    ubm = iv.DiagUbm(_dev(np.full(5, 0.2)), _dev(mu), _dev(np.ones((5, 7))))
    out = Guarded((9, 5, 7))
    Nd, Fd = _dev(N), _dev(F)
    iv.centre_stats(ubm, Nd, Fd, out=out.t)
    exact = F.astype(np.float64) - N.astype(np.float64)[:, :, None] * mu.astype(np.float32).astype(np.float64)[None]      # exact in double but for the last subtraction
    got = out.numpy()
    assert out.intact() and np.all(np.abs(got - exact) <= 2.0 ** -24 * np.abs(exact) * (1 + 1e-9)) and not got[4].any()
    assert torch.equal(iv.centre_stats(ubm, Nd, Fd), out.t)
    assert torch.equal(iv.centre_stats(ubm, Nd, Fd, out=Fd), out.t)                   # in place


# ================================================================================================ E-step
@functools.lru_cache(maxsize=None)
def _estep_case(Rk):
    N, Ft, T, var = R.estep_case(Rk)
    ref = R.estep(N, Ft, T, var)
    for a in (N, Ft, T, var) + tuple(ref):
        a.setflags(write=False)
    return N, Ft, T, var, ref


@pytest.mark.parametrize("Rk", R.ESTEP_RANKS)
def test_estep(Rk):
    N, Ft, T, var, (w64, obj64, M64, scale, _, _) = _estep_case(Rk)
    iv = _iv()
    tv = _tv(T, var)
    U, P = N.shape[0], Rk * (Rk + 1) // 2
    Nd, Fd = _dev(N), _dev(Ft.reshape(U, -1))
    Lp, b = iv.product(Nd, tv.Pk), iv.product(Fd, tv.G)
    w, M, obj = Guarded((U, Rk)), Guarded((U, P)), Guarded((U,), dtype=torch.float64)
    _call("ssv_ivec_estep", _p(Lp), _p(b), _p(w.t), _p(M.t), _p(obj.t), U, Rk, _st())
    gw, gM, gobj = w.numpy().astype(np.float64), M.numpy().astype(np.float64), obj.numpy()
    assert w.intact() and M.intact() and obj.intact() and np.isfinite(gw).all() and np.isfinite(gM).all() and np.isfinite(gobj).all()
    # the utterance without frames
    assert not gw[0].any() and gobj[0] == 0 and np.array_equal(R.tri_unpack(gM[0]), np.eye(Rk))
    assert N[1].sum() > 4000
    # against float64 from the device's own Lp and b: the factorisation alone
    own = R.estep_from(Lp.cpu().numpy(), b.cpu().numpy())
    ew, eM, eo = R.estep_errors(gw, gobj, gM, own)
    print("estep R=%d from the device's Lp, b: w %.3e M %.3e (bar %.3e) obj %.3e (bar %.1e)" % (Rk, ew, eM, R.BAR_ESTEP_OWN, eo, R.BAR_ESTEP_OWN_OBJ))
    assert ew <= R.BAR_ESTEP_OWN and eM <= R.BAR_ESTEP_OWN and eo <= R.BAR_ESTEP_OWN_OBJ
    # against float64 from T
    ew, eM, eo = R.estep_errors(gw, gobj, gM, (w64, obj64, M64, scale))
    bars = R.bar(R.MEASURED_ESTEP_W[Rk]), R.bar(R.MEASURED_ESTEP_M[Rk]), R.bar(R.MEASURED_ESTEP_OBJ[Rk])
    print("estep R=%d from T: w %.3e (bar %.3e) M %.3e (bar %.3e) obj %.3e (bar %.3e)" % (Rk, ew, bars[0], eM, bars[1], eo, bars[2]))
    assert ew <= bars[0] and eM <= bars[1] and eo <= bars[2]
    # extraction: M's buffer stays untouched, w and obj are the same bits; the module's own call agrees
    w2, M2, obj2 = Guarded((U, Rk)), Guarded((U, P), fill=-7.0), Guarded((U,), dtype=torch.float64)
    _call("ssv_ivec_estep", _p(Lp), _p(b), _p(w2.t), None, _p(obj2.t), U, Rk, _st())
    assert bool((M2.whole == -7).all()) and torch.equal(w2.t, w.t) and torch.equal(obj2.t, obj.t)
    e = tv.estep(Nd, Fd, want_M=True)
    assert torch.equal(e.w, w.t) and torch.equal(e.M, M.t) and torch.equal(e.obj, obj.t) and tv.estep(Nd, Fd).M is None


# ================================================================================================ M-step
@pytest.mark.parametrize("C,D,Rk,U", [(2, 3, 1, 8), (5, 7, 17, 40), (3, 9, 192, 6)])
def test_update_against_a_float64_solve(C, D, Rk, U):
    N, F, _, mu, var, T_true, _ = R.stats_case(C, D, Rk, U, seed=C + Rk, starved=C - 1)
    Ft = R.centre(N, F, mu, np.float32)
    T0 = R.init_T(var, Rk, seed=1)
    w, _, M, _, _, _ = R.estep(N, Ft, T0, var)
    A, Cm, Nc, Msum = R.accumulate(N, Ft, w, M)
    J = R.min_div_factor(Msum, U)
    Ad, Cd, Nd = _dev(A), _dev(Cm), _dev(Nc)
    for Jm in (None, J):
        T = Guarded((C, D, Rk), dtype=torch.float64)
        T.t.copy_(_dev(T0))
        Jd = None if Jm is None else _dev(Jm)
        _call("ssv_ivec_tv_update", _p(Ad), _p(Cd), _p(Nd), _p(Jd), _p(T.t), C, D, Rk, 10.0, _st())
        got, want = T.numpy(), R.mstep(A, Cm, Nc, T0, Jm, 10.0)
        err = float((np.abs(got - want).max(axis=(1, 2)) / np.abs(want).max(axis=(1, 2))).max())
        print("update (%d, %d, %d) J=%s: %.3e of max |T_c|, bar %.1e" % (C, D, Rk, Jm is not None, err, R.BAR_UPDATE))
        assert T.intact() and np.isfinite(got).all() and err <= R.BAR_UPDATE
        assert np.array_equal(got[C - 1], T0[C - 1]) and not np.array_equal(got[0], T0[0])          # the starved Gaussian: bit for bit


# ================================================================================================ EM
@functools.lru_cache(maxsize=None)
def _em_reference(iters):
    s = R.EM_SHAPE
    N, Ft, T0, var = R.em_case()
    h64, T64 = R.em_fit(N, Ft, T0, var, iters, True, s["min_count"])
    return N, Ft, T0, var, h64, T64, R.em_scales(N, Ft, T0, var)


def _check_em(tv, Nd, Fd, iters):
    s = R.EM_SHAPE
    N, Ft, T0, var, h64, T64, scale = _em_reference(iters)
    hist = np.array(tv.fit(Nd, Fd, iters=iters, min_count=s["min_count"], log=None))
    T = tv.T.cpu().numpy()
    eh, eT = float(np.abs(hist - h64).max() / scale), float(np.abs(T - T64).max() / np.abs(T64).max())
    print("EM %d iterations: history %s\n  history error %.3e of the objective's scale (bar %.3e), T error %.3e of max |T| (bar %.3e)"
          % (iters, hist, eh, R.bar(R.MEASURED_EM_HISTORY), eT, R.bar(R.MEASURED_EM_T)))
    assert eh <= R.bar(R.MEASURED_EM_HISTORY) and eT <= R.bar(R.MEASURED_EM_T)
    assert np.all(np.diff(hist) >= -R.bar(R.MEASURED_EM_HISTORY) * scale)
    assert np.array_equal(T[-1], T0[-1])                                                  # the starved Gaussian
    G64, Pk64 = R.planes(T64, var)                                                         # the planes are those of the new T
    assert np.abs(tv.G.cpu().numpy() - G64).max() <= 1e-4 * np.abs(G64).max()


def test_em_follows_the_float64_reference():
    s = R.EM_SHAPE
    N, Ft, T0, var = _em_reference(s["iters"])[:4]
    _check_em(_tv(T0, var), _dev(N), _dev(Ft), s["iters"])


def test_em_in_single_utterance_passes(monkeypatch):
    from spoofsv_amd import ops
    s = R.EM_SHAPE
    N, Ft, T0, var = _em_reference(2)[:4]
    need = _iv().plan_tv_passes(s["U"], s["C"], s["D"], s["R"], 0, True)[1]
    monkeypatch.setattr(ops, "free_bytes", lambda device: need)
    assert len(_iv().plan_tv_passes(s["U"], s["C"], s["D"], s["R"], ops.free_bytes(DEV), True)[0]) == s["U"]
    _check_em(_tv(T0, var), _dev(N), _dev(Ft), 2)


# ================================================================================================ extraction
def test_extraction_from_frames_does_not_depend_on_the_passes(monkeypatch):
    from spoofsv_amd import ops
    iv = _iv()
    C, D, Rk, nsel = 8, 5, 17, 4
    rng = np.random.default_rng(9)
    w, mu, var = R.ubm_case(C, D, rng)
    lens = np.array([129, 130, 128, 0])           # (alike, so that no two share a pass of the least plan; 0: an utterance without frames)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    comp = rng.integers(0, C, off[-1])
    X = (mu[comp] + np.sqrt(var[comp]) * rng.standard_normal((off[-1], D))).astype(np.float32)
    tv = _tv(0.3 * np.sqrt(var)[:, :, None] * rng.standard_normal((C, D, Rk)), var, w, mu)
    Xd = _dev(X)
    N, F = iv.bw_stats(tv.ubm(), Xd, off, nsel=nsel)
    Ft = iv.centre_stats(tv, N, F)
    want = tv.estep(N, Ft).w
    assert bool(torch.isfinite(want).all()) and not bool(want[3].any()) and bool(want[0].any())
    assert torch.equal(iv.extract_ivectors(tv, Xd, off, nsel=nsel), want) and torch.equal(tv.extract(N, Ft), want)
    need = iv.plan_extract_passes(lens, C, D, Rk, nsel, 0)[1]
    monkeypatch.setattr(ops, "free_bytes", lambda device: need)
    assert iv.plan_extract_passes(lens, C, D, Rk, nsel, ops.free_bytes(DEV))[0] == [(u, u + 1) for u in range(4)]
    assert torch.equal(iv.extract_ivectors(tv, Xd, off, nsel=nsel), want)
    need = iv.plan_tv_passes(4, C, D, Rk, 0, False)[1]
    monkeypatch.setattr(ops, "free_bytes", lambda device: need)
    assert torch.equal(tv.extract(N, Ft), want)
    monkeypatch.setattr(ops, "free_bytes", lambda device: need - 1)
    with pytest.raises(RuntimeError, match="bytes of device memory"):
        tv.extract(N, Ft)


# ================================================================================================ scoring
def test_cosine_trials_on_ragged_enrolment():
    enroll, off, evalv = R.cosine_case()
    want = R.cosine_trials(enroll, off, evalv)
    E, S = want.shape
    ed, vd = _dev(enroll), _dev(evalv)
    sc = Guarded((E, S))
    _call("ssv_ivec_cosine_trials", _p(ed), _p(_dev(off)), None, _p(vd), _p(sc.t), enroll.shape[0], S, E, enroll.shape[1], _st())
    got = sc.numpy()
    err = float(np.abs(got - want).max())
    print("cosine trials: error %.3e, bar %.3e" % (err, R.bar(R.MEASURED_COSINE)))
    assert sc.intact() and err <= R.bar(R.MEASURED_COSINE)
    assert not got[5].any() and not got[:, 2].any() and np.abs(np.delete(got[:, [0, 1, 3]], 5, axis=0)).min() > 0          # a zero vector and a speaker without enrolment score 0
    assert torch.equal(_iv().cosine_trials(ed, off, vd), sc.t) and torch.equal(_iv().cosine_trials(ed, _dev(off), vd), sc.t)
    with pytest.raises(ValueError, match="spk_off"):
        _iv().cosine_trials(ed, [0, 5, 3, 9], vd)
    one = _iv().cosine_trials(ed[:1], [0, 1], ed[:1])                                           # a vector against itself
    assert abs(float(one[0, 0]) - 1.0) <= 2.0 ** -22


# ================================================================================================ the whole chain
def test_statistics_to_the_curve(tmp_path):
    from spoofsv_amd import ge2e_harness as H
    iv = _iv()
    s = R.E2E_SHAPE
    N, F, w, mu, var, T0, lines = R.e2e_case()
    tv = _tv(T0, var, w, mu)
    Nd = _dev(N)
    Ft = iv.centre_stats(tv, Nd, _dev(F))
    tv.fit(Nd, Ft, iters=s["iters"], log=None)
    vec = tv.extract(Nd, Ft)
    enroll_lines, eval_lines = iv.split_enroll_eval(lines)
    row = {l.split()[0]: i for i, l in enumerate(lines)}
    pick = lambda ls: vec[torch.tensor([row[l.split()[0]] for l in ls], device=DEV)].contiguous()
    thresholds = [-1.0 + 0.05 * i for i in range(41)]
    path = str(tmp_path / "scores.txt")
    out = H.ivector_trials(pick(enroll_lines), enroll_lines, pick(eval_lines), eval_lines, path, thresholds)
    scores = out["scores"].cpu().numpy()
    want, target = R.e2e_reference()
    assert scores.shape == want.shape == (len(eval_lines), s["S"]) and out["speakers"] == ["S%02d" % (k + 1) for k in range(s["S"])]
    assert [(r.split()[1], r.split()[0]) for r in open(path).read().splitlines()] == [tuple(t.split()[:2]) for t in iv.trial_list(eval_lines)]
    print("whole chain: worst score difference from the float64 chain %.3e; target mean %.3f, non-target mean %.3f"
          % (np.abs(scores - want).max(), scores[target].mean(), scores[~target].mean()))
    assert np.abs(scores - want).max() < 1e-3 and scores[target].mean() > scores[~target].mean() + 0.5
    # the curve's counts are a host count of the same scores: real = own-speaker trials numbered <= 23, spoofing = those above
    num = np.array([int(l.split()[0][-3:]) for l in eval_lines])
    real, fake = H.parse_ivector_scores(path)
    assert np.array_equal(real.astype(np.float32), scores[target][num <= 23]) and np.array_equal(fake.astype(np.float32), scores[target][num > 23])
    thr = np.array(thresholds)
    assert np.array_equal(out["counts"][:, 0], (real[None, :] > thr[:, None]).sum(1)) and np.array_equal(out["counts"][:, 1], (fake[None, :] > thr[:, None]).sum(1))
    assert np.array_equal(out["spoof_rate"], out["counts"][:, 1] / len(fake)) and out["gt_frr"][0] == 0 and out["gt_frr"][-1] == 1
