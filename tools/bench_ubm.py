#!/usr/bin/env python3
"""The three stages of a diagonal-UBM EM pass, the project's kernels beside the same mathematics on torch's stock operators, on one
device at the shape of a Kaldi diagonal UBM: 200,000 synthetic frames (clustered: 128 centres x N(0, 3^2) plus unit noise), D = 60,
C = 1024, nsel = 20.

  posteriors   DiagUbm.posteriors (ssv_gmm_diag_gselect)            | X @ A.T + (X * X) @ B.T + g, topk, softmax over the selected
  statistics   DiagUbm.stats order 2 + reduce (ssv_gmm_diag_stats,  | index_add_ of gamma [1, x, x^2] into a float64 (C, 1 + 2 D)
               ssv_gmm_stats_reduce)                                |   accumulator, frames in chunks
  EM step      DiagUbm.em_step (the two above + ssv_gmm_diag_update)| the two above + the M-step in float64 tensor operations

The stock forms are written here for the comparison alone; they materialise the dense (F, C) log-likelihoods in chunks.  The forms
alternate block by block in ONE process, each timed with device events around the whole stage after an untimed first call; the figure is
the median over the blocks (at least 7).  The outputs are compared inside the run: the selections must agree except at near ties, the
statistics to float32 accuracy.  No device: the tool fails, it measures nothing on a CPU.

    python tools/bench_ubm.py [--blocks 7] [--frames 200000] [--out profiles/ubm.txt]
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
D, C, NSEL, CHUNK = 60, 1024, 20, 2048


def make_case(F, seed=0):
    rng = np.random.default_rng(seed)
    cent = rng.normal(0, 3, (128, D))
    X = (cent[rng.integers(0, 128, F)] + rng.normal(0, 1, (F, D))).astype(np.float32)
    mu = X[rng.choice(F, C, replace=False)].astype(np.float64) + rng.normal(0, .3, (C, D))
    var = rng.uniform(.5, 2, (C, D))
    w = rng.dirichlet(np.ones(C) * 5)
    return X, w, mu, var


def stock_posteriors(X, A, B, g, rows=16384):
    idx = torch.empty((X.shape[0], NSEL), dtype=torch.int64, device=X.device)
    post = torch.empty((X.shape[0], NSEL), dtype=torch.float32, device=X.device)
    ll = torch.empty((X.shape[0],), dtype=torch.float32, device=X.device)
    for f in range(0, X.shape[0], rows):
        x = X[f:f + rows]
        L = torch.addmm(g, x, A.T) + (x * x) @ B.T
        v, i = torch.topk(L, NSEL, dim=1)
        lse = torch.logsumexp(v, dim=1)
        idx[f:f + rows], post[f:f + rows], ll[f:f + rows] = i, torch.exp(v - lse[:, None]), lse
    return idx, post, ll


def stock_stats(X, idx, post, rows=16384):
    acc = torch.zeros((C, 1 + 2 * D), dtype=torch.float64, device=X.device)
    for f in range(0, X.shape[0], rows):
        x = X[f:f + rows].double()
        V = torch.cat([torch.ones((x.shape[0], 1), dtype=torch.float64, device=X.device), x, x * x], dim=1)
        terms = post[f:f + rows].double()[:, :, None] * V[:, None, :]
        acc.index_add_(0, idx[f:f + rows].reshape(-1), terms.reshape(-1, 1 + 2 * D))
    return acc


def stock_update(acc, mu, var, var_floor=1e-3, min_count=10.0, min_weight=1e-5):
    N = acc[:, 0]
    starved = (N < min_count) | ~(N > 0)
    w = N / N.sum()
    w = torch.where(starved, w.clamp_min(min_weight), w)
    w = w / w.sum()
    Nn = torch.where(starved, torch.ones_like(N), N)[:, None]
    m = torch.where(starved[:, None], mu, acc[:, 1:1 + D] / Nn)
    v = torch.where(starved[:, None], var, (acc[:, 1 + D:] / Nn - m * m).clamp_min(var_floor))
    A, B = (m / v).float(), (-0.5 / v).float()
    g = (torch.log(w) - 0.5 * (torch.log(2 * np.pi * v) + m * m / v).sum(1)).float()
    return w, m, v, A, B, g


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--frames", type=int, default=200000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ubm.txt"))
    a = ap.parse_args()
    if a.blocks < 7:
        ap.error("--blocks must be at least 7")
    if not torch.cuda.is_available():
        sys.exit("bench_ubm: no ROCm device; nothing is measured on a CPU")
    F = a.frames
    Xh, w, mu, var = make_case(F)
    X = torch.from_numpy(Xh).to(DEV)
    state = [torch.from_numpy(t).to(DEV) for t in (w, mu, var)]
    ubm = ivector.DiagUbm(*state)
    A, B, g = (t.clone() for t in ubm.planes())
    seg = np.minimum(np.arange(0, F + CHUNK, CHUNK, dtype=np.int64), F)
    kept = {}

    def ours_post():
        kept["op"] = ubm.posteriors(X, NSEL, 0.0)

    def stock_post():
        kept["sp"] = stock_posteriors(X, A, B, g)

    def ours_stats():
        idx, post, _ = kept["op"]
        kept["os"] = ubm.reduce(ubm.stats(X, seg, 2, idx, post))

    def stock_st():
        idx, post, _ = kept["sp"]
        kept["ss"] = stock_stats(X, idx, post)

    def ours_em():
        fresh = ivector.DiagUbm(*state)
        fresh.planes()
        kept["oe"] = (fresh.em_step(X, NSEL, CHUNK), fresh)

    def stock_em():
        idx, post, ll = stock_posteriors(X, A, B, g)
        kept["se"] = (ll.double().sum() / F, stock_update(stock_stats(X, idx, post), state[1], state[2]))

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    forms = [("posteriors  ours ", ours_post), ("posteriors  stock", stock_post), ("statistics  ours ", ours_stats), ("statistics  stock", stock_st),
             ("EM step     ours ", ours_em), ("EM step     stock", stock_em)]
    for _, fn in forms:
        fn()                                                             # untimed: code objects, the allocator, the library's algorithm choice
    torch.cuda.synchronize()
    times = {name: [] for name, _ in forms}
    for _ in range(a.blocks):
        for name, fn in forms:
            times[name].append(timed(fn))
    # the forms computed the same thing
    (oi, opost, oll), (si, spost, sll) = kept["op"], kept["sp"]
    same_sel = float((torch.sort(oi.long(), dim=1)[0] == torch.sort(si, dim=1)[0]).all(dim=1).double().mean())
    d_ll = float((oll - sll).abs().max())
    d_stats = float(((kept["os"] - kept["ss"]).abs() / (kept["ss"].abs() + 1.0)).max())
    d_em = abs(float(kept["oe"][0]) - float(kept["se"][0]))
    d_mu = float((kept["oe"][1].mu - kept["se"][1][1]).abs().max())
    med = {name: statistics.median(t) for name, t in times.items()}
    flop_post, flop_stats = 2.0 * F * 2 * D * C, 2.0 * F * C * (1 + 2 * D)
    lines = ["Diagonal-UBM EM stages: milliseconds per stage, median of %d blocks (min .. max), device events, forms alternating in one process" % a.blocks,
             "F = %d frames, D = %d, C = %d, nsel = %d, EM chunk %d frames; frame tile of the selection kernel %d; %s, torch %s"
             % (F, D, C, NSEL, CHUNK, _lib.lib().ssv_gmm_frame_tile(D, C), torch.cuda.get_device_name(0), torch.__version__), ""]
    for k in range(0, len(forms), 2):
        (n0, _), (n1, _) = forms[k], forms[k + 1]
        for n in (n0, n1):
            t = times[n]
            lines.append("  %-20s %10.3f ms  (%.3f .. %.3f)" % (n, med[n], min(t), max(t)))
        lines.append("  %-20s x%.3g" % ("stock / ours", med[n1] / med[n0]))
    lines += ["",
              "dense arithmetic of our forms over their stage time (whole stage, not kernel time): posteriors %.1f TFLOP/s of the (F x 2D)(2D x C) product, "
              "statistics %.1f TFLOP/s of the dense Gamma^T [1, X, X^2] product (of which a share nsel / C = %.3f is non-zero)"
              % (flop_post / med[forms[0][0]] / 1e9, flop_stats / med[forms[2][0]] / 1e9, NSEL / C),
              "agreement: frames with the same selected set %.6f; max |loglik ours - stock| %.3e; statistics max rel diff %.3e; "
              "EM mean log-likelihood diff %.3e; max |mu ours - stock| after the step %.3e" % (same_sel, d_ll, d_stats, d_em, d_mu)]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    if not (same_sel > 0.999 and d_ll < 0.05 and d_stats < 1e-3 and d_em < 1e-4):
        sys.exit("bench_ubm: the forms disagree")


if __name__ == "__main__":
    main()
