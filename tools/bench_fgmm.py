#!/usr/bin/env python3
"""The stages of a full-covariance UBM EM pass and the extractor's planes, the project's kernels beside the same mathematics on torch's
stock operators, on one device: 200,000 synthetic frames (clustered: 128 centres x N(0, 3^2) plus unit noise), D = 60, C = 1024,
nsel = 20, covariances Q diag(lambda) Q^T with lambda in [0.5, 2]; the selection is the diagonal mixture's and is held.

  posteriors   FullUbm.posteriors on the held selection and lists   | gathered pairs: (x - mu_c), a batched matmul with W_c gathered per
               (ssv_fgmm_select_post)                               |   pair (from torch.linalg.cholesky + solve_triangular, once), softmax
  statistics   FullUbm.full_stats (ssv_fgmm_stats + the reduction)  | index_add_ of gamma [1, xc, vech(xc xc^T)] into a float64
                                                                    |   (C, 1 + D + Pd) accumulator, pairs in chunks
  EM step      FullUbm.em_step (the two above + ssv_fgmm_update)    | the two above + the M-step in float64 tensor operations (batched
                                                                    |   cholesky of the new covariances, its inverse, the planes)
  planes       TotalVariability.planes at R = 192, full covariances | einsum in float64: Sigma^-1 T and T^T Sigma^-1 T, rounded
               (ssv_ivec_tv_planes_full) beside the diagonal entry  |
  grouping     FullUbm.group (ssv_fgmm_group_selection), once a fit | a stable torch.sort of the slots by Gaussian + bincount

The stock forms are written here for the comparison alone.  The forms alternate block by block in ONE process, each timed with device
events around the whole stage after an untimed first call; the figure is the median over the blocks (at least 7).  The outputs are
compared inside the run.  No device: the tool fails, it measures nothing on a CPU.

    python tools/bench_fgmm.py [--blocks 7] [--frames 200000] [--out profiles/fgmm.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spoofsv_amd import _lib, ivector                                           # noqa: E402

DEV = "cuda:0"
D, C, NSEL, RANK = 60, 1024, 20, 192
PD = D * (D + 1) // 2
LOG2PI = float(np.log(2 * np.pi))


def make_case(F, seed=0):
    rng = np.random.default_rng(seed)
    cent = rng.normal(0, 3, (128, D))
    X = (cent[rng.integers(0, 128, F)] + rng.normal(0, 1, (F, D))).astype(np.float32)
    mu = X[rng.choice(F, C, replace=False)].astype(np.float64) + rng.normal(0, .3, (C, D))
    Q = np.stack([np.linalg.qr(rng.standard_normal((D, D)))[0] for _ in range(C)])
    S = np.einsum("cij,cj,ckj->cik", Q, rng.uniform(.5, 2, (C, D)), Q)
    w = rng.dirichlet(np.ones(C) * 5)
    return X, w, mu, ivector.tri_pack((S + S.transpose(0, 2, 1)) / 2)


def unpack(cov):
    i, j = torch.tril_indices(D, D, device=cov.device)
    S = torch.zeros((cov.shape[0], D, D), dtype=cov.dtype, device=cov.device)
    S[:, i, j] = cov
    S[:, j, i] = cov
    return S


def stock_planes(w, mu, cov):
    S = unpack(cov)
    Lc = torch.linalg.cholesky(S)
    W = torch.linalg.solve_triangular(Lc, torch.eye(D, dtype=S.dtype, device=S.device).expand_as(S), upper=False)
    g = torch.log(w) - 0.5 * (D * LOG2PI + 2 * torch.log(torch.diagonal(Lc, dim1=1, dim2=2)).sum(1))
    return W.float(), mu.float(), g.float(), torch.cholesky_inverse(Lc)


def stock_posteriors(X, idx, W, muf, g, rows=8192):
    F = X.shape[0]
    post = torch.empty((F, NSEL), dtype=torch.float32, device=X.device)
    ll = torch.empty((F,), dtype=torch.float32, device=X.device)
    for f in range(0, F, rows):
        i = idx[f:f + rows].long()
        xc = X[f:f + rows, None, :] - muf[i]                                     # (rows, nsel, D)
        z = torch.matmul(W[i], xc[..., None])[..., 0]                            # W gathered per pair: what a user of stock operators writes
        L = g[i] - 0.5 * (z * z).sum(-1)
        lse = torch.logsumexp(L, dim=1)
        post[f:f + rows], ll[f:f + rows] = torch.exp(L - lse[:, None]), lse
    return post, ll


def stock_stats(X, idx, post, muf, rows=4096):
    acc = torch.zeros((C, 1 + D + PD), dtype=torch.float64, device=X.device)
    ti, tj = torch.tril_indices(D, D, device=X.device)
    for f in range(0, X.shape[0], rows):
        i = idx[f:f + rows].long()
        xc = (X[f:f + rows, None, :] - muf[i]).double()
        V = torch.cat([torch.ones(xc.shape[:2] + (1,), dtype=torch.float64, device=X.device), xc, xc[..., ti] * xc[..., tj]], dim=-1)
        acc.index_add_(0, i.reshape(-1), (post[f:f + rows].double()[..., None] * V).reshape(-1, 1 + D + PD))
    return acc


def stock_update(acc, mu, cov, var_floor=1e-3, min_count=10.0, min_weight=1e-5):
    N = acc[:, 0]
    dl = acc[:, 1:1 + D] / N[:, None]
    Sn = unpack(acc[:, 1 + D:] / N[:, None]) - dl[:, :, None] * dl[:, None, :]
    Lc, info = torch.linalg.cholesky_ex(Sn)
    kept = (N < min_count) | ~(N > 0) | (info != 0) | (torch.diagonal(Lc, dim1=1, dim2=2).square().min(1)[0] < var_floor)
    w = N / N.sum()
    w = torch.where(kept, w.clamp_min(min_weight), w)
    ti, tj = torch.tril_indices(D, D, device=acc.device)
    m = torch.where(kept[:, None], mu, mu + dl)
    c = torch.where(kept[:, None], cov, Sn[:, ti, tj])
    return (w / w.sum(), m, c, kept) + stock_planes(w / w.sum(), m, c)


def stock_tv_planes(T, icov_full):
    G = torch.einsum("cde,cer->cdr", icov_full, T)
    Pk = torch.einsum("cdi,cdj->cij", T, G)
    i, j = torch.tril_indices(RANK, RANK, device=T.device)
    return G.reshape(C * D, RANK).float(), Pk[:, i, j].float()


def stock_group(idx):
    flat = idx.reshape(-1).long()
    order = torch.sort(flat, stable=True)[1]
    return torch.cumsum(torch.bincount(flat, minlength=C), 0), order


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--frames", type=int, default=200000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fgmm.txt"))
    a = ap.parse_args()
    if a.blocks < 7:
        ap.error("--blocks must be at least 7")
    if not torch.cuda.is_available():
        sys.exit("bench_fgmm: no ROCm device; nothing is measured on a CPU")
    F = a.frames
    Xh, w, mu, cov = make_case(F)
    X = torch.from_numpy(Xh).to(DEV)
    state = [torch.from_numpy(t).to(DEV) for t in (w, mu, cov)]
    ubm = ivector.FullUbm(*state)
    ubm.planes()
    idx = ubm.diag().posteriors(X, NSEL, 0.0)[0]
    groups = ubm.group(idx)
    sW, smuf, sg, sicov = stock_planes(*state)
    tv_full = ivector.TotalVariability.from_ubm(ubm, RANK, seed=0)
    tv_diag = ivector.TotalVariability.from_ubm(ubm.diag(), RANK, seed=0)
    kept = {}

    def ours_post():
        kept["op"] = ubm.posteriors(X, idx=idx, groups=groups)[1:]

    def stock_post():
        kept["sp"] = stock_posteriors(X, idx, sW, smuf, sg)

    def ours_stats():
        kept["os"] = ubm.full_stats(X, idx, kept["op"][0], groups)

    def stock_st():
        kept["ss"] = stock_stats(X, idx, kept["sp"][0], smuf)

    def ours_em():
        fresh = ivector.FullUbm(*state)
        fresh.planes()
        kept["oe"] = (fresh.em_step(X, idx, groups)[0], fresh)

    def stock_em():
        post, ll = stock_posteriors(X, idx, sW, smuf, sg)
        kept["se"] = (ll.double().sum() / F, stock_update(stock_stats(X, idx, post, smuf), state[1], state[2]))

    def ours_planes():
        tv_full._planes = None
        kept["opl"] = tv_full.planes()

    def diag_planes():
        tv_diag._planes = None
        kept["dpl"] = tv_diag.planes()

    def stock_planes_tv():
        kept["spl"] = stock_tv_planes(tv_full.T, sicov)

    def ours_group():
        kept["og"] = ubm.group(idx)

    def stock_gr():
        kept["sg"] = stock_group(idx)

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    groups_of = [[("posteriors  ours ", ours_post), ("posteriors  stock", stock_post)], [("statistics  ours ", ours_stats), ("statistics  stock", stock_st)],
                 [("EM step     ours ", ours_em), ("EM step     stock", stock_em)],
                 [("tv planes   full ", ours_planes), ("tv planes   stock", stock_planes_tv), ("tv planes   diag ", diag_planes)],
                 [("grouping    ours ", ours_group), ("grouping    stock", stock_gr)]]
    forms = [f for grp in groups_of for f in grp]
    for _, fn in forms:
        fn()                                                             # untimed: code objects, the allocator, the library's algorithm choice
    torch.cuda.synchronize()
    times = {name: [] for name, _ in forms}
    for _ in range(a.blocks):
        for name, fn in forms:
            times[name].append(timed(fn))
    # the forms computed the same thing
    d_post = float((kept["op"][0] - kept["sp"][0]).abs().max())
    d_ll = float((kept["op"][1] - kept["sp"][1]).abs().max())
    d_stats = float(((kept["os"] - kept["ss"]).abs() / (kept["ss"].abs() + 1.0)).max())
    d_em = abs(float(kept["oe"][0]) - float(kept["se"][0]))
    d_mu = float((kept["oe"][1].mu - kept["se"][1][1]).abs().max())
    d_cov = float((kept["oe"][1].cov - kept["se"][1][2]).abs().max())
    d_pl = max(float(((a_ - b_).abs().max() / b_.abs().max())) for a_, b_ in zip(kept["opl"], kept["spl"]))
    same_group = bool(torch.equal(kept["og"][0][1:].long(), kept["sg"][0]) and torch.equal(kept["og"][1].long(), kept["sg"][1]))
    med = {name: statistics.median(t) for name, t in times.items()}
    lens = (groups[0][1:] - groups[0][:-1]).double()
    lines = ["Full-covariance UBM EM stages and the extractor's planes: milliseconds per stage, median of %d blocks (min .. max), device events, "
             "forms alternating in one process" % a.blocks,
             "F = %d frames, D = %d, C = %d, nsel = %d, R = %d; pair tile %d, statistics runs %d; list lengths min %d, mean %.0f, max %d; %s, torch %s"
             % (F, D, C, NSEL, RANK, _lib.lib().ssv_fgmm_pair_tile(), _lib.lib().ssv_fgmm_stats_runs(F, NSEL, C), int(lens.min()), float(lens.mean()),
                int(lens.max()), torch.cuda.get_device_name(0), torch.__version__), ""]
    for grp in groups_of:
        for n, _ in grp:
            t = times[n]
            lines.append("  %-20s %10.3f ms  (%.3f .. %.3f)" % (n, med[n], min(t), max(t)))
        lines.append("  %-20s x%.3g" % ("stock / ours", med[grp[1][0]] / med[grp[0][0]]))
        if len(grp) == 3:
            lines.append("  %-20s x%.3g" % ("full / diag", med[grp[0][0]] / med[grp[2][0]]))
    pairs = float(F) * NSEL
    lines += ["",
              "arithmetic of our forms over their stage time (whole stage, not kernel time): posteriors %.2f TFLOP/s of the %.1f GFLOP of the selected "
              "pairs' D x D products, statistics %.2f TFLOP/s of the %.1f GFLOP of their [1, x, vech(x x^T)] sums"
              % (2 * pairs * D * D / med[forms[0][0]] / 1e9, 2 * pairs * D * D / 1e9, 2 * pairs * (1 + D + PD) / med[forms[2][0]] / 1e9, 2 * pairs * (1 + D + PD) / 1e9),
              "agreement: max |post ours - stock| %.3e; max |loglik ours - stock| %.3e; statistics max rel diff %.3e; EM mean log-likelihood diff %.3e; "
              "after the step max |mu ours - stock| %.3e, max |cov ours - stock| %.3e; tv planes max diff %.3e of the largest entry; lists equal: %s"
              % (d_post, d_ll, d_stats, d_em, d_mu, d_cov, d_pl, same_group)]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    if not (d_post < 1e-3 and d_ll < 0.05 and d_stats < 1e-3 and d_em < 1e-4 and d_pl < 1e-5 and same_group):
        sys.exit("bench_fgmm: the forms disagree")


if __name__ == "__main__":
    main()
