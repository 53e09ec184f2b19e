#!/usr/bin/env python
"""Times a training iteration of the spoof countermeasure WITH its data path, at B = 64 on ``lin`` and ``mel`` features, in three forms:

  wav       today's loop: ``CmSource.batches`` decodes the wav files, pads, uploads and extracts features for every batch, then the eager
            iteration (zero_grad, forward, loss, backward, ``FusedAdamEx``);
  resident  ``CmResidentCorpus``: features extracted once (untimed), every batch gathered on the device, the same eager iteration;
  replayed  the resident corpus with ``CmBucketedStep``: full batches gathered into a width bucket's static buffer and the iteration
            replayed from its hipGraph (captures untimed: every bucket is reached in the warm-up epoch).

Corpus: ``--items`` synthetic utterances of 1 - 4 s at 16 kHz (tests' toy sinusoids, two classes) written as 16-bit wav files into a
temporary directory.  The three forms run in ONE process and alternate block by block over the same shuffled batches; a block is
``--iters`` iterations, timed twice: device events around it, and the host's wall clock around it with a synchronisation at its end (the
data path of the wav form is host time, which device events between launches also see, as idle time).  No loss is read back inside a
block.  Reported per form: the median over ``--blocks`` blocks [fastest .. slowest] of both clocks, per iteration, after one untimed
block; then the ratios of the wall-clock medians.  Partial batches are left out of all three forms (the replayed form runs them eagerly).

    python tools/bench_cm_resident.py [--items 320] [--blocks 7] [--iters 20] [--out profiles/cm_resident.txt]
"""
import argparse
import json
import os
import sys
import tempfile
import time
import wave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BUCKETS = {"lin": [96, 128, 160, 192, 224, 256], "mel": [24, 32, 40, 48, 56, 64]}


def toy_wave(np, i, cls, seconds, rate=16000):
    """Three sinusoids in 200..1400 Hz (class 1) or 4000..6400 Hz (class 0) under a raised-cosine envelope, noise 50 dB down."""
    rng = np.random.default_rng(1000 * cls + i)
    t = np.arange(int(rate * seconds)) / rate
    lo, hi = (200.0, 1400.0) if cls == 1 else (4000.0, 6400.0)
    y = sum(np.sin(2 * np.pi * f * t + ph) for f, ph in zip(rng.uniform(lo, hi, 3), rng.uniform(0, 2 * np.pi, 3)))
    y = y / np.abs(y).max() * 0.5 * (0.6 + 0.4 * np.sin(np.pi * t / t[-1]) ** 2)
    return (y + 1.5e-3 * rng.standard_normal(len(t))).astype(np.float32)


def write_corpus(np, root, items):
    out = {1: [], 0: []}
    rng = np.random.default_rng(7)
    for i in range(items):
        cls = i % 2
        y = toy_wave(np, i, cls, float(rng.uniform(1.0, 4.0)))
        path = os.path.join(root, "%s_%04d.wav" % ("bona" if cls else "spoof", i))
        with wave.open(path, "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes(np.clip(np.round(y.astype(np.float64) * 32768.0), -32768, 32767).astype("<i2").tobytes())
        out[cls].append(path)
    return out[1], out[0]


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=320)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cm_resident.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from spoofsv_amd import countermeasure as C
    from spoofsv_amd.train import FusedAdamEx
    if not torch.cuda.is_available():
        raise SystemExit("bench_cm_resident: needs a ROCm device; a CPU run measures nothing")
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = json.load(open(os.path.join(ROOT, "config.json")))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("countermeasure training iteration with its data path, B = %d, DISC_DIM = %d, %s; %d synthetic utterances of 1 - 4 s at 16 kHz; %d blocks "
        "of %d iterations per form after one untimed block, forms alternating; ms per iteration, median [fastest .. slowest]"
        % (a.batch, cfg["DISC_DIM"], torch.cuda.get_device_name(dev), a.items, a.blocks, a.iters))
    with tempfile.TemporaryDirectory() as root:
        bona, spoof = write_corpus(np, root, a.items)
        source = C.CmSource(cfg, bona, spoof, batch_size=a.batch, seed=0, device=dev)
        for feat in ("lin", "mel"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            corpus = C.CmResidentCorpus(source, feat)
            say("%s: resident corpus of %d items, %.1f MB held (%.1f MB used), built in %.2f s; widths %d .. %d frames, buckets %s"
                % (feat, len(corpus), corpus.bytes / 1e6, 4 * corpus.used / 1e6, time.perf_counter() - t0, int(corpus.lens.min()),
                   int(corpus.lens.max()), BUCKETS[feat]))
            full = len(corpus) // a.batch                     # full batches per epoch

            def make(capturable):
                torch.manual_seed(0)
                m = C.build_model(cfg, feat).to(dev).train()
                o = FusedAdamEx([p for p in m.parameters() if p.requires_grad], capturable=capturable, **C.ADAM)
                o.refresh_resident_weights()
                return m, o

            def eager(m, o, sp):
                o.zero_grad()
                loss, _ = m.loss(sp[corpus.key], sp["data_2"])
                loss.backward()
                o.step()

            m_w, o_w = make(False)
            m_r, o_r = make(False)
            m_g, o_g = make(True)
            stepper = C.CmBucketedStep(m_g, o_g, corpus, BUCKETS[feat])
            spans = lambda ep: [(ep, k) for k in range(full)]
            work = [s for ep in range(1 + (a.blocks + 1) * a.iters // full + 1) for s in spans(ep)]

            def run_wav(ep, k):
                order = source.order(True, ep)
                eager(m_w, o_w, source.batch(order[k * a.batch:(k + 1) * a.batch]))

            def run_resident(ep, k):
                order, rows = corpus.epoch(True, ep)
                eager(m_r, o_r, corpus.gather(rows, k * a.batch, order[k * a.batch:(k + 1) * a.batch]))

            def run_replayed(ep, k):
                order, rows = corpus.epoch(True, ep)
                stepper.step(rows, k * a.batch, order[k * a.batch:(k + 1) * a.batch])
            # every batch the timed blocks will see goes through the replayed form once, so that no capture falls into a timed block
            for ep, k in sorted(set(work)):
                run_replayed(ep, k)
            torch.cuda.synchronize()
            say("%s: %d captures in %.2f s (untimed), %d of %d warm-up batches replayed"
                % (feat, stepper.captures, stepper.capture_seconds, stepper.replays, stepper.replays + stepper.eager))
            stepper.replays = stepper.eager = 0
            forms = {"wav": run_wav, "resident": run_resident, "replayed": run_replayed}
            dev_ms, wall_ms = {k: [] for k in forms}, {k: [] for k in forms}
            for blk in range(a.blocks + 1):
                chunk = work[blk * a.iters:(blk + 1) * a.iters]
                for name, fn in forms.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record()
                    for ep, k in chunk:
                        fn(ep, k)
                    e1.record()
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    if blk:
                        dev_ms[name].append(e0.elapsed_time(e1) / len(chunk))
                        wall_ms[name].append(1e3 * (t1 - t0) / len(chunk))
            md, mw = {k: med(v) for k, v in dev_ms.items()}, {k: med(v) for k, v in wall_ms.items()}
            for name in forms:
                say("%s, %-8s: device events %.3f ms [%.3f .. %.3f]; wall %.3f ms [%.3f .. %.3f]"
                    % ((feat, name) + md[name] + mw[name]))
            say("%s: timed replayed form: %d replays, %d eager (batches wider than every bucket)" % (feat, stepper.replays, stepper.eager))
            say("%s: wall, wav / resident = %.2f, wav / replayed = %.2f, resident / replayed = %.2f"
                % (feat, mw["wav"][0] / mw["resident"][0], mw["wav"][0] / mw["replayed"][0], mw["resident"][0] / mw["replayed"][0]))
            stepper.close()
            del corpus, stepper, m_w, m_r, m_g, o_w, o_r, o_g
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
