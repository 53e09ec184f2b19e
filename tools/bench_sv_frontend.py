#!/usr/bin/env python
"""Times the speaker-verification front end (spoofsv_amd.sv_frontend) at the evaluation's real size: 20 waveforms of 83,200 samples
at 22,050 Hz per speaker, 16 and 108 speakers per batch -- per stage (resample, trim, frames + DFT + mel / log) and in total, eager and
replayed from a captured graph, device-synchronised, warm-up then enough repetitions for >= 0.5 s per figure.  Beside it the float64
restatement of tests/_sv_frontend_ref.py on the host's cores (--cpu-procs, default 16) for a sample of the same batch, scaled to the
batch: the "what a user would otherwise run" figure.  librosa / resampy themselves are not installed and cannot be timed.

    python tools/bench_sv_frontend.py [--speakers 16 108] [--cpu-sample 32] [--out FILE]
"""
import argparse
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N_SAMPLES, PER_SPEAKER, SR_IN = 83200, 20, 22050


def waveform(seed):
    rng = np.random.default_rng(seed)
    t = np.arange(N_SAMPLES) / float(SR_IN)
    y = sum(rng.uniform(0.3, 1.0) / h ** 1.5 * np.sin(2 * np.pi * 130.0 * h * t + rng.uniform(0, 6.28)) for h in range(1, 20))
    y = 0.2 * y * (0.55 + 0.45 * np.sin(2 * np.pi * 3.0 * t)) + 1e-4 * rng.standard_normal(N_SAMPLES)
    y[:4000] *= 1e-4
    y[-6000:] *= 1e-4
    return y.astype(np.float32)


def _cpu_one(seed):
    import _sv_frontend_ref as R
    return R.features(waveform(seed), SR_IN)[1]


def cpu_seconds(sample, procs):
    with multiprocessing.get_context("spawn").Pool(procs) as pool:
        pool.map(_cpu_one, range(procs))                                        # start the workers, import numpy / scipy
        t0 = time.perf_counter()
        pool.map(_cpu_one, range(sample))
        return time.perf_counter() - t0


def timed(fn, sync, min_s=0.5, warm=3):
    for _ in range(warm):
        fn()
    sync()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        if n % 5 == 0 or n < 5:
            sync()
            dt = time.perf_counter() - t0
            if dt >= min_s:
                return dt / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--speakers", type=int, nargs="+", default=[16, 108])
    ap.add_argument("--cpu-sample", type=int, default=32)
    ap.add_argument("--cpu-procs", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    cpu = cpu_seconds(a.cpu_sample, a.cpu_procs) if a.cpu_sample > 0 else None      # before the GPU is opened: the workers never see it
    import torch
    from spoofsv_amd.sv_frontend import TisvFrontEnd
    fe = TisvFrontEnd(device="cuda:0")
    sync = torch.cuda.synchronize
    for S in a.speakers:
        B = S * PER_SPEAKER
        base = torch.from_numpy(np.stack([waveform(i) for i in range(PER_SPEAKER)])).to("cuda:0")
        y = base.repeat(S, 1).contiguous()
        n = torch.full((B,), N_SAMPLES, dtype=torch.int32, device="cuda:0")
        y16, n16 = fe.resample(y, n, SR_IN)
        bounds = fe.trim_bounds(y16, n16, 30)
        _, valid = fe.slices(y16, bounds)
        assert int(valid.sum()) == B
        t_res = timed(lambda: fe.resample(y, n, SR_IN), sync)
        t_trim = timed(lambda: fe.trim_bounds(y16, n16, 30), sync)
        t_sl = timed(lambda: fe.slices(y16, bounds), sync)
        t_all = timed(lambda: fe(y, n, SR_IN), sync)
        sync()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fe(y, n, SR_IN)
        t_graph = timed(g.replay, sync)
        say("B = %4d utterances (%3d speakers x %d, %d samples at %d Hz): resample %.3f ms, trim %.3f ms, frames + DFT + mel/log %.3f ms, "
            "chain eager %.3f ms, replayed %.3f ms (%.1f us per utterance)" % (B, S, PER_SPEAKER, N_SAMPLES, SR_IN, t_res, t_trim, t_sl, t_all,
                                                                              t_graph, t_graph * 1e3 / B))
        if cpu is not None:
            say("    float64 restatement on %d host processes: %.2f s for %d utterances -> %.1f s for this batch (scaled), %.0fx the replayed chain"
                % (a.cpu_procs, cpu, a.cpu_sample, cpu / a.cpu_sample * B, cpu / a.cpu_sample * B / (t_graph * 1e-3)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
