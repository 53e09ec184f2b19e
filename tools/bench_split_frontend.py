#!/usr/bin/env python
"""Times the synthetic-data TI-SV front end (GE2E/synthetic_data_preprocess.py:34-45) on 20 utterances of 9 s at 22,050 Hz with four
pauses each, waveforms already on the device as the vocoder leaves them:

* device: ``TisvFrontEnd.split_call`` -- resample, ssv_split_intervals, ssv_select_spans, ssv_tisv_frames_table, DFT, mel/log; nothing
  is read on the host;
* host form (what the tree could do before): resample on the device, download the waveforms, ``vocoder.split_silence`` per utterance,
  upload the kept intervals as the bounds of replicated rows, ``TisvFrontEnd.slices``.

One process; both forms warmed up, then timed alternately with device events (the host form's interval includes its host work: the
end event is recorded after it).  Median, minimum and maximum over the repetitions; no ratio is promised in advance.

    python tools/bench_split_frontend.py [--reps 30] [--out profiles/split_frontend.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR_IN, SECONDS, UTTERANCES, PAUSES = 22050, 9, 20, 4


def utterances(seed=0):
    """Noise under a syllable-rate envelope, four pauses of 0.25-0.6 s of near-silence (-80 dB) at random places."""
    rng = np.random.default_rng(seed)
    n = SR_IN * SECONDS
    t = np.arange(n) / float(SR_IN)
    rows = []
    for _ in range(UTTERANCES):
        y = 0.2 * rng.standard_normal(n) * (0.6 + 0.4 * np.sin(2 * np.pi * rng.uniform(2.5, 4.0) * t))
        for c in (np.arange(PAUSES) + 1) * n // (PAUSES + 1) + rng.integers(-SR_IN // 2, SR_IN // 2, PAUSES):
            w = int(rng.uniform(0.25, 0.6) * SR_IN)
            y[c - w // 2:c + w // 2] *= 1e-4
        rows.append(y.astype(np.float32))
    return np.stack(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from spoofsv_amd.sv_frontend import TisvFrontEnd
    from spoofsv_amd.vocoder import split_silence
    if not torch.cuda.is_available():
        raise SystemExit("bench_split_frontend: needs a ROCm device; nothing is measured without one")
    dev = "cuda:0"
    fe = TisvFrontEnd(device=dev)
    y = torch.from_numpy(utterances()).to(dev)
    n = torch.full((UTTERANCES,), y.shape[1], dtype=torch.int32, device=dev)
    capacity = UTTERANCES * (PAUSES + 1)

    def device_form():
        return fe.split_call(y, n, SR_IN, capacity=capacity)

    def host_form():
        y16, n16 = fe.resample(y, n, SR_IN)
        host, lens = y16.cpu().numpy(), n16.cpu().tolist()
        rows, bounds = [], []
        for b in range(UTTERANCES):
            for s, e in split_silence(host[b, :lens[b]], 30):
                if e - s > fe.min_len:
                    rows.append(b)
                    bounds.append((int(s), int(e)))
        rep = y16.index_select(0, torch.tensor(rows, device=dev))
        return fe.slices(rep, torch.tensor(bounds, dtype=torch.int32, device=dev)) + (bounds,)

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    for _ in range(3):                                           # warm-up of both forms: code objects, filter bank, allocator
        once(device_form)
        once(host_form)
    t_dev, t_host = [], []
    for _ in range(a.reps):
        t_dev.append(once(device_form)[0])
        t_host.append(once(host_form)[0])
    (feats, table, valid, total, count), (hf, hv, hb) = device_form(), host_form()
    total = int(total.item())
    same = table[:total, 1:].cpu().tolist() == [list(b) for b in hb]
    dmax = float((feats[:total] - hf).abs().max()) if same else float("nan")
    lines = ["split front end, %d utterances of %d s at %d Hz, %d pauses each: %d intervals kept of %d (device), %d (host form)"
             % (UTTERANCES, SECONDS, SR_IN, PAUSES, total, int(count.sum().item()), len(hb)),
             "device events, %d alternating repetitions after 3 warm-up rounds, one process; ms per batch: median (min .. max)" % a.reps,
             "  device  split_call                                              %8.3f (%.3f .. %.3f)" % (np.median(t_dev), min(t_dev), max(t_dev)),
             "  host    resample, download, split_silence, upload, slices       %8.3f (%.3f .. %.3f)" % (np.median(t_host), min(t_host), max(t_host)),
             "  ratio of the medians, host form / device: %.2f" % (np.median(t_host) / np.median(t_dev)),
             "intervals of the two forms %s; largest |feature difference| on them %.3e (fp32 against float64 frame energies may move an edge: DESIGN.md 9)"
             % ("equal" if same else "DIFFER", dmax)]
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
