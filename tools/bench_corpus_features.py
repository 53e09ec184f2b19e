#!/usr/bin/env python
"""Times corpus feature extraction on a fixed synthetic corpus: ``--files`` gated-tone utterances of 2-8 s (the generator style of
tests/test_gpu_sv_frontend.py), written once at 48 kHz and once at 22.05 kHz as int16 wavs in the reference's layout.

(a) utterances / s of ``harness.extract_features`` (one utterance at a time, the yardstick) against ``harness.extract_features_batched``
    at B = 8, 32, 64 on the 22.05 kHz files, files written, and the batched device work alone (waveforms resident, no copy back, no files);
    the 48 kHz files through the batched path (``extract_features`` does not resample);
(b) the stages of one B = 32 batch, device-synchronised after each (so the parts add up to more than the unsynchronised call);
(c) ms per SSRN training batch (B = 32) read from the spectrogram cache and uploaded, against CORPUS_FEATURES = "device".
Every figure: one warm-up pass, then ``--repeats`` passes; median [min .. max] is printed.

    python tools/bench_corpus_features.py [--files 256] [--repeats 3] [--out profiles/corpus_features.txt]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def gated_tone(rng, n, sr):
    f0 = rng.uniform(90, 220)
    t = np.arange(n) / float(sr)
    y = np.zeros(n)
    for h in range(1, 13):
        y += rng.uniform(0.3, 1.0) / h ** 1.5 * np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 6.28))
    y = 0.25 * y * (0.55 + 0.45 * np.sin(2 * np.pi * rng.uniform(2.5, 4.0) * t)) + 1e-4 * rng.standard_normal(n)
    gate = np.zeros(n)
    gate[int(0.1 * sr):n - int(0.1 * sr)] = 1.0
    return y * gate


def write_corpus(root, files, cfg):
    """-> {rate: [wav paths]}; the 22.05 kHz copy also gets path lists, transcripts and speaker codes (what CorpusSource reads)."""
    from scipy.io import wavfile
    rng = np.random.default_rng(2024)
    out = {48000: [], 22050: []}
    txts = []
    for i in range(files):
        dur = rng.uniform(2.0, 8.0)
        spk = "p%d" % (225 + i % 8)
        for sr in out:
            d = os.path.join(root, "wav%d" % sr, spk)
            os.makedirs(d, exist_ok=True)
            path = os.path.join(d, "%s_%03d.wav" % (spk, i + 1))
            y = gated_tone(np.random.default_rng(i), int(dur * sr), sr)
            wavfile.write(path, sr, (y * 32767).astype(np.int16))
            out[sr].append(path)
        tdir = os.path.join(root, "txt", spk)
        os.makedirs(tdir, exist_ok=True)
        txts.append(os.path.join(tdir, "%s_%03d.txt" % (spk, i + 1)))
        open(txts[-1], "w").write("Please call Stella.\n")
        os.makedirs(cfg["SPK_EMB_DIR"], exist_ok=True)
        np.save(os.path.join(cfg["SPK_EMB_DIR"], spk + ".npy"), np.zeros(cfg["SPK_EMB_DIM"], np.float32))
    lists = os.path.join(cfg["DATA_ROOT_DIR"], "data_path", "ordinary")
    os.makedirs(lists, exist_ok=True)
    for mode in ("train", "validate"):
        open(os.path.join(lists, "wav.path." + mode), "w").write("\n".join(out[22050]) + "\n")
        open(os.path.join(lists, "txt.path." + mode), "w").write("\n".join(txts) + "\n")
    return out


def spread(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corpus_features.txt"))
    a = ap.parse_args()
    import torch
    from spoofsv_amd import harness
    from spoofsv_amd.corpus_features import CorpusFeatureExtractor, corpus_feature_bytes
    if not torch.cuda.is_available():
        raise SystemExit("bench_corpus_features: needs a ROCm device; a CPU run measures nothing")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    cfg = json.load(open(os.path.join(ROOT, "config.json")))
    tmp = tempfile.mkdtemp(prefix="corpus_features_")
    try:
        cfg.update(DATA_ROOT_DIR=os.path.join(tmp, "corpus") + os.sep, SPK_EMB_DIR=os.path.join(tmp, "spk") + os.sep,
                   SRC_ROOT_DIR=os.path.join(tmp, "runs") + os.sep)
        wavs = write_corpus(tmp, a.files, cfg)
        n = a.files
        sync = torch.cuda.synchronize
        ex = CorpusFeatureExtractor(cfg, "cuda")
        fmt = lambda t: "%.1f [%.1f .. %.1f] utterances/s" % (n / t[0], n / t[2], n / t[1])
        say("corpus: %d files of 2-8 s, int16, at 22,050 and 48,000 Hz; %d repeats after one warm-up, median [slowest .. fastest]" % (n, a.repeats))

        # (a) the yardstick and the batched path, files written
        spec = lambda tag: os.path.join(tmp, "spec_" + tag) + os.sep
        t = spread(lambda: harness.extract_features(wavs[22050], cfg, spec("old")), a.repeats)
        say("(a) extract_features, one utterance at a time, 22.05 kHz files, files written: " + fmt(t))
        loaded = [harness._read_wav(p)[1] for p in wavs[22050]]
        for B in (8, 32, 64):
            t = spread(lambda: harness.extract_features_batched(wavs[22050], cfg, spec("new%d" % B), B, extractor=ex), a.repeats)
            say("(a) extract_features_batched B = %2d, 22.05 kHz files, files written: " % B + fmt(t))
            batches = []
            for i in range(0, n, B):
                grp = loaded[i:i + B]
                y = torch.zeros((len(grp), max(len(w) for w in grp)))
                for b, w in enumerate(grp):
                    y[b, :len(w)] = torch.from_numpy(w)
                batches.append((y.cuda(), torch.tensor([len(w) for w in grp], dtype=torch.int32).cuda()))

            def device_only():
                for y, k in batches:
                    ex(y, k, 22050)
                sync()
            t = spread(device_only, a.repeats)
            say("(a) the same batches, device work alone (waveforms resident, nothing copied back): " + fmt(t)
                + "; %.0f MB of buffers for the largest batch" % (corpus_feature_bytes(B, max(b[0].shape[1] for b in batches), cfg) / 1e6))
            del batches
        t = spread(lambda: harness.extract_features_batched(wavs[48000], cfg, spec("new48"), 32, extractor=ex), a.repeats)
        say("(a) extract_features_batched B = 32, 48 kHz files (resampled 147/320 on the device), files written: " + fmt(t))

        # (b) the stages of one B = 32 batch
        for sr in (22050, 48000):
            grp = [harness._read_wav(p)[1] for p in wavs[sr][:32]]
            y = torch.zeros((len(grp), max(len(w) for w in grp)))
            for b, w in enumerate(grp):
                y[b, :len(w)] = torch.from_numpy(w)
            y, k = y.cuda(), torch.tensor([len(w) for w in grp], dtype=torch.int32).cuda()
            ex(y, k, sr)
            stage, mark = {}, [0.0]

            def tick(name):
                sync()
                now = time.perf_counter()
                stage.setdefault(name, []).append(now - mark[0])
                mark[0] = now
            for _ in range(max(3, a.repeats)):
                sync()
                mark[0] = time.perf_counter()
                ex(y, k, sr, tick)
            whole = spread(lambda: (ex(y, k, sr), sync()), max(3, a.repeats))
            say("(b) one batch of %d x %.1f s at %d Hz: %.2f ms unsynchronised [%.2f .. %.2f]; stages, synchronised after each (median ms): "
                % (len(grp), y.shape[1] / sr, sr, whole[0] * 1e3, whole[1] * 1e3, whole[2] * 1e3)
                + ", ".join("%s %.3f" % (name, sorted(v)[len(v) // 2] * 1e3) for name, v in stage.items()))

        # (c) an SSRN training batch: cache read + upload against "device" mode
        c = dict(cfg, BATCH_SIZE=32)
        cache = harness.CorpusSource(c, "train_ssrn", "conditional", "train", 32, spec("old"))
        device = harness.CorpusSource(dict(c, CORPUS_FEATURES="device"), "train_ssrn", "conditional", "train", 32, spec("none"))

        def run(src):
            def go():
                for sp in src:
                    for v in sp.values():
                        v.to("cuda")
                sync()
            return go
        nb = len(cache)
        for name, src in (("spectrogram cache (np.load, pad, upload)", cache), ('CORPUS_FEATURES = "device" (wav read, pad, upload, extract)', device)):
            t = spread(run(src), a.repeats)
            say("(c) SSRN training batch, B = 32, %s: %.1f ms per batch [%.1f .. %.1f]" % (name, t[0] / nb * 1e3, t[1] / nb * 1e3, t[2] / nb * 1e3))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
