#!/usr/bin/env python3
"""GE2E training iteration INCLUDING its data path, three forms side by side on a synthetic on-disk corpus this tool writes itself:

  (a) today's loop: DataLoader over the speakers' .npy files + ge2e.train_iteration + float(loss), as ge2e_harness.train runs it;
  (b) the corpus resident on the device, the iteration eager (ResidentSpeakerCorpus + GE2ETrainStep(graph=False));
  (c) the same, replayed from one hipGraph (GE2ETrainStep(graph=True)).

At (N, M) = (6, 50) -- the shipped config -- and (88, 10), 120 frames of 40 mel bins, the shipped embedder (768 x 3 -> 256).  All three
forms run in ONE process and alternate block by block; a block is 20 iterations timed wall-clock with one torch.cuda.synchronize() at
its end; the figure is the median over the blocks (at least 7 per form).  Form (a) is code this project has had all along, so it is
the baseline measured on the same machine in the same minutes.

    python tools/bench_ge2e_train.py [--blocks 7] [--iters 20] [--out profiles/ge2e_resident_train.txt]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spoofsv_amd import ge2e_harness as GH                                      # noqa: E402
from spoofsv_amd.ge2e import GE2ELoss, GE2ETrainStep, SpeechEmbedder, train_iteration   # noqa: E402

DEV = "cuda:0"
NMELS, FRAMES, LR = 40, 120, 0.01


def write_corpus(path, speakers, utterances, seed=0):
    rng = np.random.RandomState(seed)
    os.makedirs(path, exist_ok=True)
    for s in range(speakers):
        np.save(os.path.join(path, "speaker%d.npy" % s), rng.standard_normal((utterances, NMELS, FRAMES)).astype(np.float32))


def forever(iterable):
    while True:
        for item in iterable:
            yield item


def host_form(path, N, M):
    net, loss = SpeechEmbedder().to(DEV).train(), GE2ELoss(torch.device(DEV))
    opt = torch.optim.SGD([{"params": net.parameters()}, {"params": loss.parameters()}], lr=LR)
    batches = forever(DataLoader(GH.SpeakerDatasetPreprocessed(path, M, shuffle=True), batch_size=N, shuffle=True, num_workers=0, drop_last=True))
    history = []

    def block(iters):
        for _ in range(iters):
            history.append(float(train_iteration(net, loss, opt, next(batches).to(DEV).float(), N, M)))
    return block, history


def resident_form(corpus, N, M, graph, iters):
    net, loss = SpeechEmbedder().to(DEV).train(), GE2ELoss(torch.device(DEV))
    step = GE2ETrainStep(net, loss, N, M, FRAMES, LR, graph=graph, corpus=corpus, hist_len=iters).prepare()
    batches = forever(corpus.batches(N, M))
    history = []

    def block(n):
        for _ in range(n):
            step.run(next(batches))
        history.extend(step.losses(n))                  # one read-back per block; it is also the block's synchronisation point
    return block, history


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--speakers", type=int, default=176)
    ap.add_argument("--utterances", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ge2e_resident_train.txt"))
    a = ap.parse_args()
    if a.blocks < 7:
        ap.error("--blocks must be at least 7")
    lines = ["GE2E training iteration with its data path: ms per iteration, median of %d blocks of %d iterations (min .. max), forms alternating in one process"
             % (a.blocks, a.iters),
             "corpus: %d speakers x %d utterances of (%d, %d) float32 in .npy files; embedder 768 x 3 -> 256; %s, torch %s"
             % (a.speakers, a.utterances, NMELS, FRAMES, torch.cuda.get_device_name(0), torch.__version__), ""]
    with tempfile.TemporaryDirectory() as tmp:
        write_corpus(tmp, a.speakers, a.utterances)
        corpus = GH.ResidentSpeakerCorpus(tmp, DEV)
        lines.append("resident corpus: %.1f MB on the device" % (corpus.bytes / 1e6))
        for N, M in ((6, 50), (88, 10)):
            torch.manual_seed(0)
            np.random.seed(0)
            forms = [("(a) DataLoader over .npy + train_iteration", host_form(tmp, N, M)),
                     ("(b) resident corpus, eager", resident_form(corpus, N, M, False, a.iters)),
                     ("(c) resident corpus, replayed", resident_form(corpus, N, M, True, a.iters))]
            times = {name: [] for name, _ in forms}
            for name, (block, _) in forms:                                   # one untimed block each: allocator, first-call planning
                block(a.iters)
            torch.cuda.synchronize()
            for _ in range(a.blocks):
                for name, (block, _) in forms:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    block(a.iters)
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) / a.iters * 1e3)
            lines.append("")
            lines.append("N = %d, M = %d (%d utterances per iteration)" % (N, M, N * M))
            base = statistics.median(times[forms[0][0]])
            for name, (_, history) in forms:
                t = times[name]
                lines.append("  %-46s %8.3f ms  (%.3f .. %.3f)  x%.2f   last loss %.4f" % (name, statistics.median(t), min(t), max(t), base / statistics.median(t), history[-1]))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
