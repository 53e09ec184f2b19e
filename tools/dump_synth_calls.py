#!/usr/bin/env python
"""Dump the library calls of ONE replayed step of the column synthesizers (spoofsv_amd/synth.py) as JSON, without a device and without
libssv_hip.so: ``_lib.call`` is replaced by a recorder, the model and the synthesizer's buffers are CPU tensors, and every pointer
argument is printed as the name of what it points to --

    param:<qualified parameter name>    a parameter of the melSyn, read in place
    <buffer attribute> | hist<i>        a buffer of the synthesizer (kv, mel_cur, a, b, rq, ..., the i-th highway input history)
    tap_major:<module name>             the IncrementalSynthesizer's (M, k, C) copy of that k = 3 conv's weight
    planes:<parameter name>             the resident split planes of that weight (wide step, split modes)
    null | stream                       a null pointer | the current stream

A pointer that resolves to none of these is an error.  Two versions of synth.py launch the same step exactly when their dumps are
equal.  tests/golden/synth_step_calls.json is the output of this tool on the commit BEFORE the synthesizers were given one column
schedule and one lifecycle (tests/test_wide_synth_cpu.py records the working tree and compares): the step is what takes the time of a
free run, and it changes by editing that fixture, not by accident."""
import contextlib
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, TEXT_LEN, FRAMES = 6, 5, 4
# name -> (class name, conditioned, shared_texts, stubbed arithmetic mode)
CONFIGS = {
    "incremental/conditioned": ("IncrementalSynthesizer", True, None, 0),
    "incremental/unconditioned": ("IncrementalSynthesizer", False, None, 0),
    "wide/conditioned/fp32": ("WideSynthesizer", True, None, 0),
    "wide/unconditioned/fp32": ("WideSynthesizer", False, None, 0),
    "wide/conditioned/shared_texts=3/f16x2": ("WideSynthesizer", True, 3, 2),
}
BUFFERS = ("kv", "mel_cur", "Y", "Yw", "A", "pma", "t", "s1", "s2", "a", "b", "pre", "pre1", "rq", "y_cur")


class _Planes:
    """What the stubbed ``resident.lookup`` returns: the planes OF a weight, so the record shows whose planes a launch was given."""

    def __init__(self, addr):
        self.value = addr


@contextlib.contextmanager
def stubbed(precision):
    """No library, no device: ``_lib.call`` appends (entry, raw arguments) to the list this yields."""
    from spoofsv_amd import _lib, ops, resident, synth
    calls = []
    saved = (_lib.call, _lib.precision, ops._stream, synth._wide_tile, resident.lookup)
    _lib.call = lambda name, *args: calls.append((name, args))
    _lib.precision = lambda: precision
    ops._stream = lambda: "stream"
    synth._wide_tile = lambda: 32
    resident.lookup = lambda w: _Planes(w.data_ptr())
    try:
        yield calls
    finally:
        _lib.call, _lib.precision, ops._stream, synth._wide_tile, resident.lookup = saved


def tap_major_copies(g):
    """{address: module name} of the tap-major weight copies an IncrementalSynthesizer holds (``_wt``: id(conv) -> (copy, conv))."""
    names = {id(mod): name for name, mod in g.model.named_modules()}
    return {buf.data_ptr(): "tap_major:" + names[id(conv)] for buf, conv in getattr(g, "_wt", {}).values()}


def record_step(cls_name, conditioned, shared_texts=None, precision=0):
    """The calls of one ``_step()`` of a fresh synthesizer, as lists ``[entry, arg, ...]`` with the pointers named."""
    import torch
    from spoofsv_amd import synth
    from spoofsv_amd.tts import melSyn
    model = melSyn(34, conditioned, 200 if conditioned else None, textemb_dim=16, freq_bins=80, hidden_dim=32).eval()
    with stubbed(precision) as calls:
        kw = {} if shared_texts is None else {"shared_texts": shared_texts}
        g = getattr(synth, cls_name)(model, BATCH, TEXT_LEN, FRAMES, "cpu", **kw)
        with torch.no_grad():
            g._step()
    where = {p.data_ptr(): "param:" + n for n, p in model.named_parameters()}
    planes = {a: "planes:" + n[len("param:"):] for a, n in where.items()}
    where.update(tap_major_copies(g))
    where.update({getattr(g, n).data_ptr(): n for n in BUFFERS if hasattr(g, n)})
    where.update({h.data_ptr(): "hist%d" % i for i, h in enumerate(g.hist)})

    def name(entry, a):
        if a is None:
            return None
        if isinstance(a, _Planes):
            return planes[a.value]
        if isinstance(a, ctypes.c_void_p):
            if a.value not in where:
                raise RuntimeError("%s: a pointer argument of %s is no parameter, buffer or weight copy" % (cls_name, entry))
            return where[a.value]
        if isinstance(a, (int, str)) and not isinstance(a, bool):
            return a
        raise RuntimeError("%s: argument %r of %s" % (cls_name, a, entry))

    return [[entry] + [name(entry, a) for a in args] for entry, args in calls]


def collect():
    return {cfg: record_step(*args) for cfg, args in CONFIGS.items()}


def render(d):
    """One line per call: a diff names the launch that moved."""
    parts = []
    for cfg in sorted(d):
        lines = ",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in d[cfg])
        parts.append(" %s: [\n%s\n ]" % (json.dumps(cfg), lines))
    return "{\n%s\n}\n" % ",\n".join(parts)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.stdout.write(render(collect()))
