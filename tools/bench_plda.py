#!/usr/bin/env python3
"""The PLDA back end, the project's kernels beside the same mathematics on torch's stock operators, on one device.

  statistics      PldaEstimator's set-up: ssv_plda_class_stats, the scatter   | float64: normalise, per-speaker means by index_add, residuals, Xd^T Xd
                  by ssv_ivec_product_tn                                      |
  10 EM + obj     10 x em_step and the final objective                        | float64, the SAME algebra (one inverse per distinct count, the
                  (n = 35,000 rows, S = 1,000 speakers, R = 192)              |   inversion lemma for the quadratic forms and determinants): batched
                                                                              |   linalg.cholesky / cholesky_inverse, bmm against the gathered Mx
  score           ssv_plda_score on given planes, E = 16,384, S = 1,024       | float32 matmul cat([t^2, t]) H^T + k;  and the direct form broadcast
                  and at the paper's shape E = 800, S = 20                    |   over (chunk, S, R) in float32, 256 eval rows at a time

The stock forms are written here for the comparison alone.  Each of their batched factorisation calls is followed by a device
synchronisation, for the reason DESIGN 4.13 gives (queued back to back they returned garbage here); the waits are inside the stock forms'
time.  The forms alternate block by block in ONE process, each timed with device events around the whole stage after an untimed first call;
the figure is the median over the blocks (at least 7).  The outputs are compared inside the run.  No device: the tool fails.

    python tools/bench_plda.py [--blocks 7] [--out profiles/plda.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spoofsv_amd import plda                                                    # noqa: E402
from spoofsv_amd.ivector import tri_unpack                                      # noqa: E402

DEV = "cuda:0"
R, S_TRAIN, N_TRAIN, ITERS = 192, 1000, 35000, 10
F32, F64 = torch.float32, torch.float64


def train_case(seed=0):
    """Rows drawn from a two-covariance model, mixed counts 5 .. 65 that sum to N_TRAIN (set-up, not timed)."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(5, 66, S_TRAIN)
    while counts.sum() != N_TRAIN:
        k = rng.integers(0, S_TRAIN)
        step = int(np.sign(N_TRAIN - counts.sum()))
        if 5 <= counts[k] + step <= 65:
            counts[k] += step
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV, dtype=F64)
    lam_b = torch.logspace(-0.5, 1.0, R, dtype=F64, device=DEV).sqrt()
    lam_w = torch.logspace(-1.0, 0.3, R, dtype=F64, device=DEV).sqrt()
    q1, q2 = torch.linalg.qr(rn(R, R))[0], torch.linalg.qr(rn(R, R))[0]
    spk = torch.repeat_interleave(torch.arange(S_TRAIN, device=DEV), torch.from_numpy(counts).to(DEV))
    y = (rn(S_TRAIN, R) * lam_b) @ q1.T
    X = 0.5 * rn(1, R) + y[spk] + (rn(N_TRAIN, R) * lam_w) @ q2.T
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return X.float().contiguous(), off, counts, spk


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "plda.txt"))
    a = ap.parse_args()
    if a.blocks < 7:
        ap.error("--blocks must be at least 7")
    if not torch.cuda.is_available():
        sys.exit("bench_plda: no ROCm device; nothing is measured on a CPU")
    X, off, counts, spk = train_case()
    distinct = np.unique(counts)
    cls = torch.from_numpy(np.searchsorted(distinct, counts)).to(DEV)
    nd = torch.from_numpy(distinct.astype(np.float64)).to(DEV)
    nk = torch.from_numpy(counts.astype(np.float64)).to(DEV)
    nspk = torch.from_numpy(np.array([(counts == c).sum() for c in distinct], dtype=np.float64)).to(DEV)
    eye = torch.eye(R, dtype=F64, device=DEV)
    kept = {}

    def chol_inv(M):
        C = torch.linalg.cholesky(M)
        torch.cuda.synchronize()
        inv = torch.cholesky_inverse(C)
        torch.cuda.synchronize()
        return inv, 2.0 * torch.log(torch.diagonal(C, dim1=-2, dim2=-1)).sum(-1)

    def stock_stats():
        x = X.double()
        ss = (x * x).sum(1, keepdim=True)
        xh = x * torch.where(ss > 0, (R / ss.clamp_min(1e-300)).sqrt(), torch.zeros_like(ss))
        means = torch.zeros((S_TRAIN, R), dtype=F64, device=DEV).index_add_(0, spk, xh) / nk[:, None]
        Xd = xh - means[spk]
        kept["ss"] = (Xd.T @ Xd, means, means.mean(0))

    def ours_stats():
        kept["os"] = plda.PldaEstimator(X, off)

    def stock_iter(Sigma, c, W, B, update):
        Winv, ldW = chol_inv(W)
        Binv, ldB = chol_inv(B)
        Mx, ldMx = chol_inv(Binv[None] + nd[:, None, None] * Winv[None])
        t = c @ Winv
        w = nk[:, None] * torch.bmm(Mx[cls], t[:, :, None])[:, :, 0]
        r = c - w
        quad = nk * (t * r).sum(1)
        sk = (ldW - R * torch.log(nk) + ldB + ldMx[cls] + quad).sum()
        obj = (-0.5 * ((N_TRAIN - S_TRAIN) * ldW + (Winv * Sigma).sum()) - 0.5 * sk) / N_TRAIN
        if not update:
            return obj, W, B
        Bn = ((nspk[:, None, None] * Mx).sum(0) + w.T @ w) / S_TRAIN
        Wn = (Sigma + ((nspk * nd)[:, None, None] * Mx).sum(0) + (r * nk[:, None]).T @ r) / N_TRAIN
        return obj, Wn, Bn

    def stock_em():
        Sigma, means, mu = kept["ss"]
        c, W, B, hist = means - mu, eye.clone(), eye.clone(), []
        for _ in range(ITERS):
            obj, W, B = stock_iter(Sigma, c, W, B, True)
            hist.append(obj)
        hist.append(stock_iter(Sigma, c, W, B, False)[0])
        kept["sem"] = (torch.stack(hist), W, B)

    def ours_em():
        est = kept["os"]
        est.WB.copy_(torch.from_numpy(np.stack([plda.tri_pack(np.eye(R))] * 2)))
        hist = [est.em_step() for _ in range(ITERS)] + [est.objective()]
        kept["oem"] = (torch.stack(hist), est.W.clone(), est.B.clone())

    def score_forms(E, S, tag):
        g = torch.Generator(device=DEV).manual_seed(E + S)
        psi = torch.sort(12 * torch.rand(R, generator=g, device=DEV, dtype=F64), descending=True)[0]
        model = plda.Plda(torch.zeros(R, dtype=F64, device=DEV), eye.clone(), psi)
        y = (torch.randn(S, R, generator=g, device=DEV, dtype=F64) * (psi + 0.3).sqrt()).float()
        n = torch.randint(1, 10, (S,), generator=g, device=DEV).to(torch.int32)
        T = (0.7 * y[torch.randint(0, S, (E,), generator=g, device=DEV)] + torch.randn(E, R, generator=g, device=DEV)).contiguous()
        H, k = model.planes(y, n)
        k32 = k.float()
        out = torch.empty((E, S), dtype=F32, device=DEV)
        den = n.double()[:, None] * psi + 1.0
        cc, v = (n.double()[:, None] * psi / den), 1.0 + psi / den
        cy, av, p1 = (cc * y.double()).float(), (1.0 / v).float(), (1.0 / (psi + 1.0)).float()
        const = (-0.5 * torch.log(v).sum(1) + 0.5 * torch.log(psi + 1.0).sum()).float()

        def ours():
            kept[tag + "o"] = model.score_planes(H, k, T, out=out)

        def matmul():
            kept[tag + "m"] = torch.cat([T * T, T], dim=1) @ H.T + k32

        def direct():
            res = torch.empty((E, S), dtype=F32, device=DEV)
            for e0 in range(0, E, 256):
                t = T[e0:e0 + 256]
                d = t[:, None, :] - cy[None]
                res[e0:e0 + 256] = -0.5 * (av[None] * d * d).sum(2) + 0.5 * (t * t * p1).sum(1)[:, None] + const
            kept[tag + "d"] = res

        def check():
            t64 = T.double()
            ref = torch.cat([t64 * t64, t64], dim=1) @ H.double().T + k
            scale = torch.cat([t64 * t64, t64], dim=1).abs() @ H.double().abs().T + k.abs()
            return tuple(float(((kept[tag + f].double() - ref).abs() / scale).max()) for f in "omd")
        return [("score %-10s ours  " % tag, ours), ("score %-10s matmul" % tag, matmul), ("score %-10s direct" % tag, direct)], check

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    big, check_big = score_forms(16384, 1024, "16384x1024")
    small, check_small = score_forms(800, 20, "800x20")
    forms = [("statistics       ours  ", ours_stats), ("statistics       stock ", stock_stats), ("10 EM + obj      ours  ", ours_em),
             ("10 EM + obj      stock ", stock_em)] + big + small
    for _, fn in forms:
        fn()                                                             # untimed: code objects, the allocator, the library's algorithm choice
    torch.cuda.synchronize()
    times = {name: [] for name, _ in forms}
    for _ in range(a.blocks):
        for name, fn in forms:
            times[name].append(timed(fn))
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max())
    oh, oW, oB = kept["oem"]
    sh, sW, sB = kept["sem"]
    unp = lambda p: torch.from_numpy(tri_unpack(p.cpu().numpy(), R)).to(DEV)
    d_hist, d_W, d_B = float((oh - sh).abs().max() / sh.abs().max()), rel(unp(oW), sW), rel(unp(oB), sB)
    d_sigma = rel(kept["os"].Sigma, kept["ss"][0])
    mono = float((oh[1:] - oh[:-1]).min())
    eb, es = check_big(), check_small()
    med = {name: statistics.median(t) for name, t in times.items()}
    lines = ["PLDA back end: milliseconds per stage, median of %d blocks (min .. max), device events, forms alternating in one process" % a.blocks,
             "training: n = %d rows, S = %d speakers of %d distinct counts (%d .. %d), R = %d, %d EM iterations; %s, torch %s"
             % (N_TRAIN, S_TRAIN, distinct.size, counts.min(), counts.max(), R, ITERS, torch.cuda.get_device_name(0), torch.__version__), ""]
    for name, _ in forms:
        t = times[name]
        lines.append("  %-30s %10.3f ms  (%.3f .. %.3f)" % (name, med[name], min(t), max(t)))
    n = [name for name, _ in forms]
    flop = 2.0 * 16384 * 1024 * 2 * R
    lines += ["",
              "stock / ours: statistics x%.3g, 10 EM + obj x%.3g; score 16384x1024: matmul x%.3g, direct x%.3g; score 800x20: matmul x%.3g, direct x%.3g"
              % (med[n[1]] / med[n[0]], med[n[3]] / med[n[2]], med[n[5]] / med[n[4]], med[n[6]] / med[n[4]], med[n[8]] / med[n[7]], med[n[9]] / med[n[7]]),
              "dense arithmetic of the 16384 x 1024 score (%.2f GFLOP) over our time: %.2f TFLOP/s" % (flop / 1e9, flop / med[n[4]] / 1e9),
              "agreement of the training forms (ours against stock, relative to the largest entry): Sigma %.3e, history %.3e, W %.3e, B %.3e; "
              "smallest step of our history %+.3e" % (d_sigma, d_hist, d_W, d_B, mono),
              "score error against the float64 product of the same planes, of the term scale: 16384x1024 ours %.3e, matmul %.3e, direct %.3e; "
              "800x20 ours %.3e, matmul %.3e, direct %.3e" % (eb + es)]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    if not (d_sigma < 1e-4 and d_hist < 1e-5 and d_W < 1e-4 and d_B < 1e-4 and max(eb + es) < 1e-4):
        sys.exit("bench_plda: the forms disagree")


if __name__ == "__main__":
    main()
