#!/usr/bin/env python3
"""Profiling target: column-incremental free run at full size (326 frames).  python tools/prof_synth.py [batch]
python tools/prof_synth.py --wide S: the wide step instead, S speakers x 20 shared sentences of 43 characters (two runs of 326 frames)."""
import sys, time
sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import torch
from spoofsv_amd import harness, train
from spoofsv_amd.tts import melSyn
dev = "cuda:0"
B = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1] != "--wide" else 20
torch.manual_seed(1234)
m = melSyn(34, True, 200, 128, 80, 256); m.apply(train.init_weights); m = m.to(dev).eval()
if len(sys.argv) > 2 and sys.argv[1] == "--wide":
    S, U, N, frames = int(sys.argv[2]), 20, 43, 326
    text = torch.randint(2, 33, (U, 1, N), device=dev); text[:, :, -1] = 1
    spk = (0.04 + 0.05 * torch.rand(S, 200, 1, device=dev)).repeat_interleave(U, dim=0).contiguous()
    with torch.no_grad():
        harness._free_run(m, text, spk, frames, 80, wide=True, shared_texts=U)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        harness._free_run(m, text, spk, frames, 80, wide=True, shared_texts=U)
        torch.cuda.synchronize(); print("S=%d (%d items) wide free run: %.3f ms/frame" % (S, S * U, (time.perf_counter() - t0) / frames * 1e3), flush=True)
    sys.exit(0)
N, frames = 80, 326
text = torch.randint(2, 33, (B, 1, N), device=dev); text[:, :, -1] = 1
spk = 0.04 + 0.05 * torch.rand(B, 200, 1, device=dev)
with torch.no_grad():
    harness._free_run(m, text, spk, frames, 80, incremental=True)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    harness._free_run(m, text, spk, frames, 80, incremental=True)
    torch.cuda.synchronize(); print("B=%d incremental free run: %.3f ms/frame" % (B, (time.perf_counter() - t0) / frames * 1e3), flush=True)
