#!/usr/bin/env python3
"""The counting behind curve.py's GE2E sweep -- 5,000 thresholds over the similarity matrices of a test -- four forms side by side on a
device stack at the configuration's shape (N = 20, V = 80, one matrix per batch of a ten-epoch test: 10 matrices):

  (a) the host form: the stack downloaded, then curve.py's loop on CPU tensors, vectorised per threshold over the whole stack (wall time);
  (b) the only device route there was: ssv_sv_eer_sweep called per matrix with nthr = 5000, one workgroup per threshold re-reading the
      matrix (device events);
  (c) ge2e.sv_score_curve: the thresholds checked and uploaded, then ssv_sv_score_curve -- one launch, every matrix read once per tile of
      thresholds (device events around the whole operator);
  (d) that launch alone, thresholds and table already on the device, as (b) has them (device events).

The four alternate block by block in ONE process; the figure is the median over the blocks (at least 7).  The counts of (b) and (c) are
compared inside the run, (d)'s with (c)'s, and (a)'s own-column counts with them.

    python tools/bench_sv_curve.py [--blocks 7] [--nmat 10] [--out profiles/sv_curve.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spoofsv_amd import _lib, ge2e                                              # noqa: E402
from spoofsv_amd import ge2e_harness as GH                                      # noqa: E402
from spoofsv_amd.ops import _p, _stream                                         # noqa: E402

DEV = "cuda:0"
N, V, ROWS = 20, 80, 40


def make_stack(nmat, seed=0):
    """Scores as a trained embedder spreads them: off-speaker around 0.45, own-speaker genuine rows high, spoofing rows a little lower."""
    g = torch.Generator().manual_seed(seed)
    stack = 0.25 + 0.4 * torch.rand(nmat, N, V, N, generator=g)
    idx = torch.arange(N)
    own = 0.55 + 0.45 * torch.rand(N, nmat, V, generator=g)
    own[:, :, ROWS:] -= 0.08
    stack[:, idx, :, idx] = own
    return stack.to(DEV)


def host_form(stack, thr):
    host = stack.cpu()
    idx = torch.arange(N)
    head, tail = [], []
    for t in thr:
        own = (host > t)[:, idx, :, idx]                                 # (N, nmat, V)
        head.append(own[:, :, :ROWS].float().sum(dim=(0, 2)))
        tail.append(own[:, :, -ROWS:].float().sum(dim=(0, 2)))
    return torch.stack(head, 1), torch.stack(tail, 1)                    # (nmat, K) each


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--nmat", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sv_curve.txt"))
    a = ap.parse_args()
    if a.blocks < 7:
        ap.error("--blocks must be at least 7")
    thr = GH.curve_thresholds("ge2e")
    K = len(thr)
    stack = make_stack(a.nmat)
    thr_dev = torch.tensor(thr, dtype=torch.float32).to(DEV)
    sweep_counts = torch.zeros((a.nmat, K, 4), dtype=torch.int32, device=DEV)
    hist = torch.zeros((a.nmat, 6), dtype=torch.float64, device=DEV)
    step_dev = torch.zeros((1,), dtype=torch.int32, device=DEV)
    kept = {}

    def per_threshold():
        for m in range(a.nmat):
            _lib.call("ssv_sv_eer_sweep", _p(stack[m]), N, V, _p(thr_dev), K, ROWS, ROWS, float(V), float(V), float(ROWS), float(ROWS), _p(sweep_counts[m]),
                      _p(hist), a.nmat, _p(step_dev), _stream())
        kept["b"] = sweep_counts

    def binned():
        kept["c"] = ge2e.sv_score_curve(stack, thr, ROWS, ROWS)

    curve_counts = torch.zeros((a.nmat, K, 4), dtype=torch.int32, device=DEV)

    def launch_alone():
        _lib.call("ssv_sv_score_curve", _p(stack), a.nmat, N, V, ROWS, ROWS, _p(thr_dev), K, _p(curve_counts), _stream())
        kept["d"] = curve_counts

    def host():
        kept["a"] = host_form(stack, thr)

    def timed(fn, events):
        torch.cuda.synchronize()
        if not events:
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    forms = [("(a) download + curve.py's loop on CPU tensors", host, False), ("(b) ssv_sv_eer_sweep per matrix, nthr = 5000", per_threshold, True),
             ("(c) ge2e.sv_score_curve: upload + one launch", binned, True), ("(d) ssv_sv_score_curve alone", launch_alone, True)]
    for _, fn, _ in forms[1:]:
        fn()                                                             # untimed: first-call planning, the allocator
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in forms}
    for _ in range(a.blocks):
        for name, fn, events in forms:
            times[name].append(timed(fn, events))
    b, c = kept["b"].cpu().numpy(), kept["c"].cpu().numpy()
    same = np.array_equal(b, c) and np.array_equal(kept["d"].cpu().numpy(), c)
    head, tail = kept["a"]
    same_host = np.array_equal(head.numpy().astype(np.int64), c[:, :, 2]) and np.array_equal(tail.numpy().astype(np.int64), c[:, :, 3])
    med = {name: statistics.median(t) for name, t in times.items()}
    lines = ["Counts of curve.py's GE2E sweep: milliseconds per whole stack, median of %d blocks (min .. max), forms alternating in one process" % a.blocks,
             "stack: %d matrices (N = %d, V = %d, N) float32 on the device, K = %d thresholds, head = tail = %d rows; tile %d thresholds per workgroup; %s, torch %s"
             % (a.nmat, N, V, K, ROWS, _lib.lib().ssv_sv_curve_tile(), torch.cuda.get_device_name(0), torch.__version__), ""]
    for name, _, events in forms:
        t = times[name]
        lines.append("  %-48s %10.3f ms  (%.3f .. %.3f)  %s  (b) / this = x%.3g" % (name, med[name], min(t), max(t), "device events" if events else "wall time    ",
                                                                              med[forms[1][0]] / med[name]))
    lines += ["", "counts of (b), (c) and (d) equal: %s; own-column head and tail counts of (a) equal (c)'s: %s" % (same, same_host),
              "(a) includes the download of the stack (%.1f MB); (b) includes its one-thread finishing kernel per matrix, which loops over the 5,000 rows."
              % (stack.numel() * 4 / 1e6)]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    if not (same and same_host):
        sys.exit("bench_sv_curve: the forms disagree")


if __name__ == "__main__":
    main()
