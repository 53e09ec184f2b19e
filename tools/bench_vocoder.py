#!/usr/bin/env python3
"""Griffin-Lim vocoder timing at the synthesis size (MAX_FRAME_NUM 325 -> 1300 linear frames, 64 iterations), for the basis-GEMM
transform ("dft", the default) and the LDS FFT back end ("fft").

Usage: python tools/bench_vocoder.py [B ...] [--transform dft|fft|both] [--out FILE] [--errors-from LOG]      (default B: 1 16 20)

Every case -- (B, T) with T = 1300 and its neighbour 1301, eager and replayed from a captured graph -- is warmed up, then timed in
several blocks of whole 64-iteration runs, each block ending in a device synchronise; the figure is the median block, with the spread
(min .. max) beside it.  With ``both`` the two back ends run in the same process on the same inputs, their blocks alternating, and
the results go to profiles/fft_vocoder.txt (``--out``) together with the worst errors of the GPU tests when ``--errors-from`` names a
``pytest -s`` log of tests/test_gpu_fft_vocoder.py."""
import argparse
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                    # noqa: E402
from spoofsv_amd.vocoder import Vocoder         # noqa: E402

N_ITER, BLOCKS = 64, 7


def block(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / reps


def measure(vocs, B, T, replayed):
    """{transform: (median, min, max) ms per 64-iteration call}; the back ends' blocks alternate"""
    S = torch.rand(B, 513, T, device="cuda")
    a = next(iter(vocs.values())).random_angles(B, T)
    fns = {}
    for name, v in vocs.items():
        fns[name] = (lambda v=v: v.griffinlim_graph(S, a, N_ITER)) if replayed else (lambda v=v: v.griffinlim(S, a, N_ITER))
    reps = {}
    for name, fn in fns.items():                # warm-up: code objects, allocator, graph capture; then size a block to ~0.3 s
        fn()
        fn()
        reps[name] = max(2, min(50, int(300.0 / max(block(fn, 2), 1e-3))))
    times = {name: [] for name in fns}
    for _ in range(BLOCKS):
        for name, fn in fns.items():
            times[name].append(block(fn, reps[name]))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def worst_errors(log):
    """worst "<what> (...): <error>, bar <bar>" figure per kind of check in a pytest -s log"""
    worst = {}
    for m in re.finditer(r"^\.*([A-Za-z][\w\-() ]*?) \((\d+), (\d+), T=\d+\)( \d+ iterations)?: ([0-9.e+-]+), bar ([0-9.e+-]+)", open(log).read(), flags=re.M):
        key = m.group(1).strip() + (m.group(4) or "")
        e, b = float(m.group(5)), float(m.group(6))
        if key not in worst or e > worst[key][0]:
            worst[key] = (e, b, "(%s, %s)" % (m.group(2), m.group(3)))
    return worst


def other_figures(log):
    """the figures the tests print in another form (full size, the 64-iteration trace, the harness's wav files), as printed"""
    return [m.group(1) for m in re.finditer(r"^\.*((?:full size|inconsistency first|s\d+_\d+\.wav:) .*)$", open(log).read(), flags=re.M)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("B", nargs="*", type=int, default=[1, 16, 20])
    ap.add_argument("--transform", choices=("dft", "fft", "both"), default="dft")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fft_vocoder.txt"), help="where `--transform both` writes its table")
    ap.add_argument("--errors-from", help="pytest -s log of tests/test_gpu_fft_vocoder.py: its worst errors are added to the table")
    a = ap.parse_args()
    names = ("dft", "fft") if a.transform == "both" else (a.transform,)
    vocs = {n: Vocoder(1024, 256, transform=n) for n in names}
    lines = ["Griffin-Lim vocoder, n_fft 1024, hop 256, %d iterations, ms per call (median of %d blocks, min .. max) and ms per utterance" % (N_ITER, BLOCKS),
             "device: %s" % torch.cuda.get_device_name(0)]
    for B in a.B:
        for T in (1300, 1301):
            for replayed in (False, True):
                res = measure(vocs, B, T, replayed)
                for n in names:
                    med, lo, hi = res[n]
                    extra = ""
                    if n == "dft":
                        extra = "  (DFT GEMMs alone %.0f TFLOP/s-equivalent)" % (N_ITER * 2 * 2.0 * 1026 * 1024 * B * T / med / 1e9)
                    elif "dft" in res:
                        extra = "  (%.2fx the dft time)" % (med / res["dft"][0])
                    lines.append("B=%-3d T=%d %-8s %s: %8.2f ms (%.2f .. %.2f)  %.3f ms/utterance%s"
                                 % (B, T, "replayed" if replayed else "eager", n, med, lo, hi, med / B, extra))
                    print(lines[-1], flush=True)
    if a.errors_from:
        lines.append("")
        lines.append("worst error of transform=\"fft\" against the float64 oracle in tests/test_gpu_fft_vocoder.py, relative to the oracle's peak, with its bar")
        lines.append("(the bar: ten times the error of the float32 scipy.fft emulation of tests/_fft_vocoder_ref.py on the same input)")
        for key, (e, b, where) in sorted(worst_errors(a.errors_from).items()):
            lines.append("%-36s %.2e  (bar %.2e) at %s" % (key, e, b, where))
            print(lines[-1], flush=True)
        lines.append("further figures as those tests print them (full size: B = 4, T = 1300; 64 iterations at (1024, 256, T=25); wav files of "
                     "generate_test_utterances, fft against dft)")
        lines += other_figures(a.errors_from)
    if a.transform == "both":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
