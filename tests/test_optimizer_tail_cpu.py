"""The references of the optimizer-tail GPU tests (tests/_optimizer_tail_ref.py), checked on their own: the Adam step against torch.optim.Adam in
float64 and the golden file, the plane index map as a bijection, and the reconstruction bounds of the two split formats."""
import numpy as np
import pytest
import torch

import _optimizer_tail_ref as R
from _golden import load

CONFIGS = [(2e-4, 0.5, 0.9, 1e-6), (1e-3, 0.9, 0.999, 1e-8)]


@pytest.mark.parametrize("lr,b1,b2,eps", CONFIGS)
def test_adam_step_ref_is_torch_adam_in_float64(lr, b1, b2, eps):
    f = lambda x: float(np.float32(x))                     # the reference rounds the hyper-parameters to float32: hand torch the same values
    rng = np.random.default_rng(0)
    n = 1000
    p0 = rng.standard_normal(n)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], f(lr), (f(b1), f(b2)), f(eps))
    p, m, v = p0, np.zeros(n), np.zeros(n)
    for t in range(1, 6):
        g = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 3, n)
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        r = R.adam_step_ref(p, g, m, v, lr, b1, b2, eps, t)               # one step from torch's own state: no drift between the two
        st = opt.state[tp]
        # float64 against float64: a few roundings of 2^-53 each.  torch forms m' as m + (g - m)(1 - b1), whose roundings scale with |m| + |g|
        big = np.abs(m) + np.abs(g)
        assert np.all(np.abs(r.m - st["exp_avg"].numpy()) <= 2.0 ** -50 * big), t
        assert np.all(np.abs(r.v - st["exp_avg_sq"].numpy()) <= 2.0 ** -50 * r.v), t
        assert np.all(np.abs(r.p - tp.detach().numpy()) <= 2.0 ** -52 * np.abs(r.p) + 2.0 ** -48 * r.step_size * big / r.denom), t
        p, m, v = tp.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()


def test_adam_step_ref_reproduces_the_golden_steps():
    """adam.npz holds three float32 steps of the reference's optimizer (2e-4, (0.5, 0.9), 1e-6).  Each golden step is one float32 evaluation
    from the previous golden p: one rounding of p, and a relative error of the update of ~8u from its own roundings plus ~4u per earlier step
    from the float32 moments it carries -- 32u covers three steps."""
    g = load("adam.npz")
    p, m, v = g["p0"].astype(np.float64), 0.0 * g["p0"], 0.0 * g["p0"]
    for t in (1, 2, 3):
        r = R.adam_step_ref(p, g["g%d" % t], m, v, 2e-4, 0.5, 0.9, 1e-6, t)
        tol = R.U * np.abs(r.p) + 32 * R.U * r.step_size * r.mag / r.denom
        assert np.all(np.abs(r.p - g["p%d" % t]) <= tol), (t, float((np.abs(r.p - g["p%d" % t]) / tol).max()))
        p, m, v = g["p%d" % t].astype(np.float64), r.m, r.v


def test_adam_bounds_hold_for_a_float32_evaluation():
    """The bounds of the GPU test against a float32 numpy evaluation of the same formula (one rounding per operation, no fused multiply-add):
    it must fit, or the bounds would test the rounding mode of the device and not the formula."""
    rng = np.random.default_rng(1)
    n = 100000
    f32 = np.float32
    for (lr, b1, b2, eps) in CONFIGS:
        for t in (1, 2, 10, 1000, 100000):
            scale = np.array([1e-12, 1e-6, 1.0, 1e4])[rng.integers(0, 4, n)]
            g = (rng.standard_normal(n) * scale).astype(f32)
            p = rng.standard_normal(n).astype(f32)
            m = (0.1 * rng.standard_normal(n) * scale).astype(f32) if t > 1 else np.zeros(n, f32)
            v = ((rng.standard_normal(n) * scale) ** 2).astype(f32) if t > 1 else np.zeros(n, f32)
            keep = (np.abs(g) >= 1e-15) & ((np.abs(m) >= 1e-15) | (t == 1)) & ((v >= 1e-15) | (t == 1))
            p, g, m, v = p[keep], g[keep], m[keep], v[keep]
            r = R.adam_step_ref(p, g, m, v, lr, b1, b2, eps, t)
            lrf, b1f, b2f, epsf = f32(lr), f32(b1), f32(b2), f32(eps)
            m1 = b1f * m + (f32(1) - b1f) * g
            v1 = b2f * v + (f32(1) - b2f) * g * g
            ss = f32(float(lrf) / (1.0 - float(b1f) ** t))
            isb = f32(1.0 / np.sqrt(1.0 - float(b2f) ** t))
            p1 = p - ss * (m1 / (np.sqrt(v1) * isb + epsf))
            assert p1.dtype == m1.dtype == v1.dtype == f32
            (fp, _), (fm, _), (fv, _), (fu, _) = R.adam_fractions(p1, m1, v1, r)
            print("float32 numpy, lr=%g t=%d: fraction of the bound used p %.3f (update part %.3f) m %.3f v %.3f" % (lr, t, fp, fu, fm, fv))
            assert fm <= 1.0 and fv <= 1.0 and fp <= 1.0, (lr, t, fp, fm, fv)


@pytest.mark.parametrize("shape", R.PACK_SHAPES)
def test_plane_index_map_is_a_bijection(shape):
    (jobs, total) = R.plan_jobs_ref(*shape)
    Cout, Cin, k = shape
    rng = np.random.default_rng(2)
    w = rng.uniform(1.0, 2.0, Cout * Cin * k).astype(np.float32)          # no zero: every written slot shows
    for job, off in jobs:
        assert job.Kpad % 32 == 0 and job.Kpad >= job.K and job.Kpad - job.K < 32
        t, m, kk = R._grid(job)
        idx = R.plane_index(t, m, kk, job)
        n = R.plane_elems(job)
        assert idx.min() >= 0 and idx.max() < n
        assert np.unique(idx).size == idx.size == job.KT * job.M * job.K
        # the source map reads every element of the weight exactly once
        src = m * job.sm + kk * job.sk + t
        assert np.array_equal(np.sort(src), np.arange(Cout * Cin * k))
        assert off % 256 == 0 and R.lo_offset(job) == R.split_bytes(job.M, job.K, job.KT) and off + 2 * R.lo_offset(job) <= total - 256
        for mode in ("bf16x3", "f16x2"):
            hi, lo, inv = R.pack_planes_ref(w, job, mode)
            assert hi.size == lo.size == n
            written = np.zeros(n, dtype=bool)
            written[idx] = True
            assert np.all(hi[written] != 0) and not hi[~written].any() and not lo[~written].any()
            # and the entry at the slot is the element the map names
            sc = R.pow2_scale(np.abs(w).max())[0] if mode == "f16x2" else None
            assert np.array_equal(hi[idx], R.split_values(w[src], mode, sc)[0])
    assert total == jobs[1][1] + 2 * R.lo_offset(jobs[1][0]) + 256


def test_pow2_scale_is_the_documented_power_of_two():
    for amax, E in ((0.0, 15), (1e-38, 15), (1.0, 127), (1.5, 127), (2.0, 128), (3e38, 254), (2.0 ** -100, 27)):
        sc, inv = R.pow2_scale(amax)
        assert float(sc) == 2.0 ** (141 - E) and float(inv) == 2.0 ** (E - 141), amax
        assert float(np.float32(amax) * sc) < 2.0 ** 15                   # the scaled maximum stays inside fp16


def test_f16x2_reconstruction_bound():
    """|x sc - (hi + lo)| <= 2^-22 |x sc| + 2^-25 on 2 10^6 log-uniform values under one scale: hi rounds to 11 bits (or to the subnormal grid,
    2^-25 at most), lo rounds the exact remainder the same way."""
    rng = np.random.default_rng(3)
    n = 2_000_000
    x = (2.0 ** rng.uniform(-40, 0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    x[0] = 1.9999                                            # the maximum: scaled to just under 2^15
    sc, inv = R.pow2_scale(np.abs(x).max())
    assert float(sc) * float(inv) == 1.0
    hi, lo = R.split_values(x, "f16x2", sc)
    worst = R.reconstruction_excess(x, hi, lo, "f16x2", sc)
    assert worst <= 1.0, worst
    l = lo.view(np.float16)
    sub = float(np.mean((l != 0) & (np.abs(l.astype(np.float32)) < 2.0 ** -14)))
    assert sub > 0.1, sub                                    # fp16-subnormal lo halves are common in wide-range data, not a corner case


def test_bf16x3_reconstruction_bound():
    rng = np.random.default_rng(4)
    n = 2_000_000
    x = (2.0 ** rng.uniform(-100, 100, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    hi, lo = R.split_values(x, "bf16x3")
    worst = R.reconstruction_excess(x, hi, lo, "bf16x3")
    assert worst <= 1.0, worst
    assert worst <= 0.5 + 1e-3, worst                        # (the format gives 2^-17 |x|; the stated bound is twice that)
