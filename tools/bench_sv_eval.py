#!/usr/bin/env python3
"""The speaker-verification test INCLUDING its data path, three forms side by side on a synthetic on-disk test corpus this tool writes:

  (a) today's sequence: ge2e_harness.test + test_nospoof + spoof_rate_at (DataLoader over the speakers' .npy files, stock-op scoring, the
      host sweep, the similarity matrices through the disk);
  (b) ge2e_harness.evaluate on a corpus held on the device, the batch eager (cfg["test"]["graph"] = False);
  (c) the same, the batch replayed from one hipGraph.

At the shipped configuration: N = 20, M = 86, enroll 3, eval 20, 10 epochs, 20 speaker files of 86 x (40, 120), the shipped embedder
(768 x 3 -> 256).  All three forms run in ONE process and alternate block by block; a block is one whole evaluation (model load, corpus
load and, for (c), warm-up and capture included -- what a user waits for), timed wall-clock; the figure is the median over the blocks
(at least 7 per form).  Form (a) is code this project has had all along: the baseline measured on the same machine in the same minutes.
(b) and (c) draw each epoch's batches once for both sweeps, (a) twice: they do half of (a)'s embedder forwards by construction.

    python tools/bench_sv_eval.py [--blocks 7] [--epochs 10] [--out profiles/sv_eval.txt]
"""
import argparse
import contextlib
import io
import os
import random
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spoofsv_amd import ge2e_harness as GH                                      # noqa: E402

DEV = "cuda:0"
N, M, ENROLL, EVAL, NMELS, FRAMES = 20, 86, 3, 20, 40, 120


def write_corpus(path, speakers, seed=0):
    rng = np.random.RandomState(seed)
    os.makedirs(path, exist_ok=True)
    for s in range(speakers):
        np.save(os.path.join(path, "speaker%02d.npy" % s), (rng.standard_normal((1, NMELS, 1)) + 0.5 * rng.standard_normal((M, NMELS, FRAMES))).astype(np.float32))


def seed_all(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def quiet(fn, *args):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--speakers", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sv_eval.txt"))
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it (the file may hold the score bar already)")
    a = ap.parse_args()
    if a.blocks < 7:
        ap.error("--blocks must be at least 7")
    lines = ["Speaker-verification test with its data path: seconds per whole evaluation (%d epochs), median of %d blocks (min .. max), forms alternating in one process"
             % (a.epochs, a.blocks),
             "test corpus: %d speakers x %d utterances of (%d, %d) float32 in .npy files; N = %d, M = %d, enroll %d, eval %d; embedder 768 x 3 -> 256; %s, torch %s"
             % (a.speakers, M, NMELS, FRAMES, N, M, ENROLL, EVAL, torch.cuda.get_device_name(0), torch.__version__), ""]
    with tempfile.TemporaryDirectory() as tmp:
        write_corpus(os.path.join(tmp, "test"), a.speakers)
        cfg = GH.default_config()
        cfg["data"]["test_path"] = os.path.join(tmp, "test")
        cfg["test"].update(N=N, M=M, epochs=a.epochs)
        cfg["save_simmat_dir"] = os.path.join(tmp, "simmat")
        model_path = os.path.join(tmp, "net.model")
        torch.manual_seed(0)
        torch.save({k: v.cpu() for k, v in GH._embedder(cfg, "cpu").state_dict().items()}, model_path)

        def host():
            for f in os.listdir(cfg["save_simmat_dir"]) if os.path.isdir(cfg["save_simmat_dir"]) else []:
                os.remove(os.path.join(cfg["save_simmat_dir"], f))
            eer, spoof = GH.test(cfg, model_path, ENROLL)
            thres = GH.test_nospoof(cfg, model_path, ENROLL, EVAL)
            return dict(EER=eer, spoof_rate=spoof, threshold=thres, spoof_rate_at_eer=GH.spoof_rate_at(cfg, thres, EVAL))

        def resident(graph):
            c = {k: (dict(v) if isinstance(v, dict) else v) for k, v in cfg.items()}
            c["test"]["graph"] = graph
            return lambda: GH.evaluate(c, model_path, ENROLL, EVAL)
        forms = [("(a) test + test_nospoof + spoof_rate_at (host)", host), ("(b) evaluate, resident corpus, eager", resident(False)),
                 ("(c) evaluate, resident corpus, replayed", resident(True))]
        times, last = {name: [] for name, _ in forms}, {}
        for name, fn in forms:                                               # one untimed evaluation each: allocator, first-call planning
            seed_all(1)
            quiet(fn)
        torch.cuda.synchronize()
        for b in range(a.blocks):
            for name, fn in forms:
                seed_all(100 + b)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[name] = quiet(fn)
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
        base = statistics.median(times[forms[0][0]])
        for name, _ in forms:
            t, r = times[name], last[name]
            lines.append("  %-48s %8.3f s  (%.3f .. %.3f)  x%.2f   EER %.4f  spoof rate %.4f  threshold %.4f  spoof rate at it %.4f"
                         % (name, statistics.median(t), min(t), max(t), base / statistics.median(t), r["EER"], r["spoof_rate"], r["threshold"], r["spoof_rate_at_eer"]))
        lines += ["", "(a) embeds every epoch's batches twice (test and test_nospoof draw their own), (b) and (c) once; the untrained embedder's figures are",
                  "not meaningful as verification results, they show that the three forms ran the same experiment."]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
