#!/usr/bin/env python
"""Dump the names of the library calls of ONE eager training iteration (after one warm-up iteration) as JSON: ``train.TrainStep`` over a
``DataParallelRanks(model=...)`` gradient arena with batched weight gradients (``defer_wgrad=True``), Text2Mel at B=4, N=40, T=64 and
SSRN at B=4, T=40, 65 linear bins.  Needs a GPU.  ``_lib.call`` is wrapped by a recorder that appends the entry-point name and calls
through; names only -- no pointers, no sizes.  Which entries run says which path every operator took: a weight gradient that is not
deferred, or joins another batched launch, shows as another sequence.

tests/golden/train_step_calls.json is the output of this tool on the commit BEFORE gradient slots and deferral marks were found by
parameter instead of by address (tests/test_gpu_ddp.py records the working tree and compares); it changes by editing that fixture,
not by accident."""
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


@contextlib.contextmanager
def recording():
    """``_lib.call`` appends the entry-point name to the list this yields, then calls through."""
    from spoofsv_amd import _lib
    names, real = [], _lib.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    _lib.call = call
    try:
        yield names
    finally:
        _lib.call = real


def record_step(kind):
    import torch
    from spoofsv_amd import train
    from spoofsv_amd.tts import SSRN, melSyn
    if kind == "text2mel":
        torch.manual_seed(100)
        m = melSyn(34, True, 200, textemb_dim=16, freq_bins=80, hidden_dim=32)
        batch = list(train.synthetic_text2mel_batch(4, N=40, T=64, seed=3, device=DEV))
        gaw = train.guided_attention_mat(40, 64, device=DEV)
    else:
        torch.manual_seed(101)
        m = SSRN(80, 65, 32)
        batch = list(train.synthetic_ssrn_batch(4, T=40, out_bins=65, seed=3, device=DEV))
        gaw = None
    m.apply(train.init_weights)
    m.to(DEV).train()
    opt = train.FusedAdam(m.parameters(), 2e-4, (0.5, 0.9), 1e-6)
    opt.refresh_resident_weights()
    ddp = train.DataParallelRanks(model=m)
    step = train.TrainStep(kind, m, opt, batch, gaw, ddp, graph=False, defer_wgrad=True)
    step()                                   # warm-up: pinned job tables, seed vectors, the optimizer's state
    with recording() as names:
        step()
    torch.cuda.synchronize()
    ddp.close()
    return names


def collect():
    return {kind: record_step(kind) for kind in ("text2mel", "ssrn")}


def render(d):
    """One line per call: a diff names the launch that moved."""
    return "{\n%s\n}\n" % ",\n".join(" %s: [\n%s\n ]" % (json.dumps(k), ",\n".join("  " + json.dumps(n) for n in d[k])) for k in sorted(d))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.stdout.write(render(collect()))
