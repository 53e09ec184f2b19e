#!/usr/bin/env python
"""Times training from the spectrogram cache (np.load per item, pad, pin, upload: ``harness.Prefetcher`` over the cache mode) against the
resident corpus (config key CORPUS_RESIDENT: arenas on the device, gather kernels) on ONE synthetic cache: ``--items`` utterances in the
reference's layout, random float32 spectrograms of the config's sizes (80 x T, 513 x 4T), lengths spread over the corpus range as
tools/bench_ragged.py spreads them (text 20..130 ids, frames 40..248), eight speakers.

(a) load time and resident bytes per step kind;
(b) the data path alone: batches / s of one epoch at B = 32 through ``Prefetcher``, every batch on the device at the end;
(c) whole training iterations (batch, forward, backward, Adam, the loss read back as ``ordinary_train`` reads it) at B = 32, eager and with
    LENGTH_BUCKETS, full-size models.
Method: the page cache is warmed first (every cache file read once), so the cache mode is timed against memory, not the disk -- its best
case.  Both modes alternate in one process, epoch by epoch; every figure is the median of ``--blocks`` epochs after one untimed epoch of
each mode (which also captures the buckets), with [fastest .. slowest].  The ratio is cache time / resident time.

    python tools/bench_resident_corpus.py [--items 256] [--blocks 3] [--out profiles/resident_corpus.txt]
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

T2M_BUCKETS = [[64, 128], [96, 192], [128, 256], [186, 325]]
SSRN_BUCKETS = [128, 192, 256, 325]


def write_cache(root, items, cfg):
    """-> the spectrogram cache's directory; path lists, transcripts and speaker codes beside it (what CorpusSource reads)."""
    rng = np.random.RandomState(2024)
    vocab = [c for c in cfg["VOCABULARY"][2:] if c.isalpha() or c == " "]
    spec = os.path.join(root, "spec") + os.sep
    wavs, txts = [], []
    os.makedirs(cfg["SPK_EMB_DIR"], exist_ok=True)
    for i in range(items):
        spk = "p%d" % (225 + i % 8)
        name = "%s_%03d" % (spk, i // 8 + 1)
        nl = int(rng.randint(20, 131))
        T = int(np.clip(int(nl * 1.6) + rng.randint(0, 40), 40, cfg["MAX_FRAME_NUM"]))
        os.makedirs(os.path.join(spec, spk), exist_ok=True)
        os.makedirs(os.path.join(root, "txt", spk), exist_ok=True)
        wavs.append(os.path.join(root, "wav22", spk, name + ".wav"))              # (never opened: every item is cached)
        txts.append(os.path.join(root, "txt", spk, name + ".txt"))
        open(txts[-1], "w").write("".join(vocab[k] for k in rng.randint(0, len(vocab), nl - 1)) + "\n")     # + 'E' = nl ids
        np.save(spec + wavs[-1][-17:-4] + "_mel.npy", rng.rand(80, T).astype(np.float32))
        np.save(spec + wavs[-1][-17:-4] + "_lin.npy", rng.rand(1 + cfg["STFT"]["FFT_LENGTH"] // 2, 4 * T).astype(np.float32))
        np.save(os.path.join(cfg["SPK_EMB_DIR"], spk + ".npy"), rng.rand(cfg["SPK_EMB_DIM"]).astype(np.float32))
    lists = os.path.join(cfg["DATA_ROOT_DIR"], "data_path", "ordinary")
    os.makedirs(lists, exist_ok=True)
    for mode in ("train", "validate"):
        open(os.path.join(lists, "wav.path." + mode), "w").write("\n".join(wavs) + "\n")
        open(os.path.join(lists, "txt.path." + mode), "w").write("\n".join(txts) + "\n")
    return spec


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident_corpus.txt"))
    a = ap.parse_args()
    import torch
    from spoofsv_amd import harness, train
    if not torch.cuda.is_available():
        raise SystemExit("bench_resident_corpus: needs a ROCm device; a CPU run measures nothing")
    dev = torch.device("cuda", torch.cuda.current_device())
    sync = torch.cuda.synchronize
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    cfg = json.load(open(os.path.join(ROOT, "config.json")))
    tmp = tempfile.mkdtemp(prefix="resident_corpus_")
    try:
        cfg.update(DATA_ROOT_DIR=os.path.join(tmp, "corpus") + os.sep, SPK_EMB_DIR=os.path.join(tmp, "spk") + os.sep,
                   SRC_ROOT_DIR=os.path.join(tmp, "runs") + os.sep, BATCH_SIZE=a.batch)
        spec = write_cache(tmp, a.items, cfg)
        nbytes = 0
        for d, _, fs in os.walk(spec):                                             # warm the page cache
            for f in fs:
                nbytes += np.load(os.path.join(d, f)).nbytes
        say("corpus: %d cached utterances, %.0f MB of float32 spectrograms, B = %d; page cache warm; %d timed epochs per mode after one untimed, "
            "modes alternating; median [fastest .. slowest]" % (a.items, nbytes / 1e6, a.batch, a.blocks))
        gaw = train.guided_attention_mat(cfg["MAX_TEXT_LEN"], cfg["MAX_FRAME_NUM"], device=dev)
        for step in ("train_ssrn", "train_text2mel"):
            kind = train.step_kind(step)
            srcs = {"cache": harness.Prefetcher(harness.BatchSource(cfg, step, a.batch, spec, pattern="conditional"), dev)}
            res = harness.BatchSource(dict(cfg, CORPUS_RESIDENT=True), step, a.batch, spec, pattern="conditional")
            srcs["resident"] = harness.Prefetcher(res, dev)
            rc = res.corpus.resident
            nb = len(res)
            say("(a) %s: resident corpus of %.1f MB (%s) loaded in %.2f s" % (step, rc.nbytes / 1e6, ", ".join(rc.plan.parts), rc.load_seconds))

            def data_epoch(src):
                sync()
                t0 = time.perf_counter()
                for sp in src:
                    pass
                sync()
                return time.perf_counter() - t0
            times = {k: [] for k in srcs}
            for blk in range(a.blocks + 1):
                for k, src in srcs.items():
                    t = data_epoch(src)
                    if blk:
                        times[k].append(t)
            m = {k: med(v) for k, v in times.items()}
            for k in srcs:
                say("(b) %s, data path alone, %s: %.1f batches/s [%.1f .. %.1f] (%.2f ms per batch)"
                    % (step, k, nb / m[k][0], nb / m[k][1], nb / m[k][2], m[k][0] / nb * 1e3))
            say("(b) %s, data path alone: resident is %.2fx the cache mode" % (step, m["cache"][0] / m["resident"][0]))

            for tag, buckets in (("eager", None), ("LENGTH_BUCKETS", T2M_BUCKETS if kind == "text2mel" else SSRN_BUCKETS)):
                torch.manual_seed(0)
                model, _ = harness._build(step, "conditional", cfg, False)
                model.apply(train.init_weights)
                model.to(dev).train()
                opt = harness._adam(model.parameters(), cfg)
                bucketed = None
                if buckets is not None:
                    opt.capturable = True
                    bucketed = train.BucketedTrainStep(kind, model, opt, buckets, gaw=gaw, ddp=None, batch_size=a.batch)

                def train_epoch(src):
                    sync()
                    t0 = time.perf_counter()
                    for sp in src:
                        batch = [sp[k].to(dev) for k in train.KINDS[kind].keys]
                        terms = bucketed(*batch) if bucketed is not None else train.TrainStep(kind, model, opt, batch, gaw, None, graph=False)()
                        sum(float(t.detach()) for t in tuple(terms))
                    sync()
                    return time.perf_counter() - t0
                try:
                    times = {k: [] for k in srcs}
                    for blk in range(a.blocks + 1):
                        for k, src in srcs.items():
                            t = train_epoch(src)
                            if blk:
                                times[k].append(t)
                    m = {k: med(v) for k, v in times.items()}
                    extra = "" if bucketed is None else " (replays %d, eager %d, captures %d)" % (bucketed.replays, bucketed.eager, bucketed.captures)
                    for k in srcs:
                        say("(c) %s, %s, training iteration from the %s: %.2f ms [%.2f .. %.2f]"
                            % (step, tag, k if k == "resident" else "cache", m[k][0] / nb * 1e3, m[k][1] / nb * 1e3, m[k][2] / nb * 1e3))
                    say("(c) %s, %s: resident is %.2fx the cache mode%s" % (step, tag, m["cache"][0] / m["resident"][0], extra))
                finally:
                    if bucketed is not None:
                        bucketed.close()
                del model, opt
            del srcs, res, rc
            torch.cuda.empty_cache()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
