#!/usr/bin/env python
"""Times whole-utterance d-vector extraction (spoofsv_amd.dvector.DvectorExtractor) on ragged batches of 1-6 s utterances at 16 kHz,
320 and 2,160 per batch, one voiced span per utterance: utterances / s and frames / s of the eager call, the same call restricted to
its front half (frames -> DFT -> log-mel), and the split into frames, DFT, mel, gather, embedder and mean (device-synchronised around
every stage, so the parts add up to more than the unsynchronised call).  Beside the useful bandwidth of ssv_span_frames (unique samples
read + frames written) the same figure for ssv_tisv_frames, the stride-one-hop gather of the first / last 120 frames, on the same batch
in the same process.  Warm-up, then enough repetitions for >= 0.5 s per figure.

    python tools/bench_dvector.py [--utterances 320 2160] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR = 16000


def timed(fn, sync, min_s=0.5, warm=2):
    for _ in range(warm):
        fn()
    sync()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        sync()
        dt = time.perf_counter() - t0
        if dt >= min_s:
            return dt / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, nargs="+", default=[320, 2160])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    import torch
    from spoofsv_amd.dvector import DvectorExtractor
    from spoofsv_amd.ge2e import SpeechEmbedder
    from spoofsv_amd.sv_frontend import TisvFrontEnd
    dev = "cuda:0"
    fe = TisvFrontEnd(device=dev)
    torch.manual_seed(0)
    net = SpeechEmbedder(40, 768, 3, 256).to(dev).eval()
    ex = DvectorExtractor(fe, net)
    sync = torch.cuda.synchronize
    for B in a.utterances:
        rng = np.random.default_rng(B)
        lens = rng.integers(1 * SR, 6 * SR + 1, size=B)
        n_max = int(lens.max())
        y = 0.1 * torch.randn((B, n_max), device=dev)
        n = torch.tensor(lens, dtype=torch.int32, device=dev)
        spans = [[(0, int(v))] for v in lens]
        pl = ex.plan(y, n, spans)
        G, Nw = pl.n_frames, pl.n_windows
        stage = {}
        mark = [0.0]

        def tick(name):
            sync()
            now = time.perf_counter()
            if name is not None:
                stage[name] = stage.get(name, 0.0) + (now - mark[0])
            mark[0] = now
        ex(y, n, spans)                                                        # warm: weight planes split, allocator primed
        reps = 3
        stage.clear()
        for _ in range(reps):
            ex(y, n, spans, timers=tick)
        parts = {k: v / reps * 1e3 for k, v in stage.items()}
        t_all = timed(lambda: ex(y, n, spans), sync)
        t_front = timed(lambda: ex.log_mel(y, pl), sync)
        t_trim = timed(lambda: ex(y, n), sync)
        say("B = %4d utterances of 1-6 s (%d frames, %d windows, %d rows): eager %.2f ms = %.0f utterances/s, %.2f M frames/s; front half "
            "(frames + DFT + mel) %.2f ms = %.2f M frames/s; with spans=None (trim + one host read of the bounds) %.2f ms"
            % (B, G, Nw, int(pl.offs.shape[0]) - 1, t_all, B / t_all * 1e3, G / t_all * 1e-3, t_front, G / t_front * 1e-3, t_trim))
        say("    stages, synchronised: " + ", ".join("%s %.2f ms" % (k, parts.get(k, 0.0)) for k in ("frames", "dft", "mel", "gather", "embedder", "mean")))
        # the framing kernels alone, on whole items so that one launch covers a chunk
        tiles = torch.from_numpy(pl.tiles).to(dev)
        nf = min(G, ex.frames_per_call)
        hi = int(np.searchsorted(pl.tiles[:, 4], nf, side="left"))
        fr = torch.empty((-(-nf // ex.COLS), fe.nfft, ex.COLS), device=dev)
        t_sf = timed(lambda: ex.span_frames(y, tiles[:hi], 0, nf, out=fr), sync)
        useful = nf * (fe.nfft + fe.hop_length) * 4.0                           # every frame written once, every sample read once
        say("    ssv_span_frames: %d frames in %.3f ms: %.2f TB/s useful (%.1f MB written, %.1f MB of samples read once)"
            % (nf, t_sf, useful / t_sf * 1e-9, nf * fe.nfft * 4e-6, nf * fe.hop_length * 4e-6))
        bounds = torch.stack([torch.zeros_like(n), n], 1).contiguous()
        t_old = timed(lambda: fe.frames(y, bounds), sync)
        old_bytes = 2 * B * fe.nfft * fe.tisv_frame * 4.0 + 2 * B * ((fe.tisv_frame - 1) * fe.hop_length + fe.nfft) * 4.0
        say("    ssv_tisv_frames (first / last %d frames of the same %d utterances): %.3f ms: %.2f TB/s useful"
            % (fe.tisv_frame, B, t_old, old_bytes / t_old * 1e-9))
        del y, fr
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
