"""Host-side checks of the wide column-incremental synthesis step: ABI, argument checks before the device, the planning of the
speaker groups of generate_test_utterances, and the device-byte count of a WideSynthesizer.  No GPU needed."""
import ctypes

import pytest

WIDE_ENTRIES = ("ssv_column_wide_tile", "ssv_column_highway_wide", "ssv_column_pwln_wide", "ssv_attention_column_wide",
                "ssv_synth_column_advance_wide")
BAD_SHAPE, UNSUPPORTED = -1, -2
X = ctypes.c_void_p(4096)            # a non-null pointer that is never dereferenced: every call below fails its host-side checks


def test_header_declares_and_library_exports_the_wide_entries():
    from spoofsv_amd import _lib
    protos = _lib.parse_header()
    L = _lib.lib()
    for name in WIDE_ENTRIES:
        assert name in protos, name
        assert hasattr(L, name), name
    assert L.ssv_version() == 7
    assert L.ssv_column_wide_tile() == 32
    ret, argtypes, names = protos["ssv_column_highway_wide"]
    assert names[-1] == "stream" and "w_packed" in names and "t_dev" in names and "hist" in names
    assert "s" in protos["ssv_column_pwln_wide"][2] and "U" in protos["ssv_attention_column_wide"][2]


def _highway(**over):
    a = dict(w=X, w_packed=X, bias=X, g1=X, b1=X, g2=X, b2=X, cur=X, hist=X, Tmax=70, t_dev=X, dilation=3, out=ctypes.c_void_p(8192),
             B=37, Bw=64, C=256, k=3, stream=None)
    a.update(over)
    return list(a.values())


def _pwln(**over):
    a = dict(x=X, w=X, w_packed=X, bias=X, s=None, gamma=X, beta=X, y=ctypes.c_void_p(8192), B=37, Bw=64, Cin=80, Cout=256, act=1, stream=None)
    a.update(over)
    return list(a.values())


def _attn(**over):
    a = dict(kv=X, kv_bs=2 * 256 * 43, U=20, q=X, pma=X, a=X, a_T=326, t_dev=X, rq=X, B=40, Bw=64, d=256, N=43, stream=None)
    a.update(over)
    return list(a.values())


def _advance(**over):
    a = dict(y_cur=X, Y=X, mel_cur=X, t_dev=X, Bw=64, F=80, T=326, stream=None)
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize("entry,args,code,word", [
    ("ssv_column_highway_wide", _highway(w=None), BAD_SHAPE, "null"),
    ("ssv_column_highway_wide", _highway(hist=None), BAD_SHAPE, "null"),
    ("ssv_column_highway_wide", _highway(t_dev=None), BAD_SHAPE, "null"),
    ("ssv_column_highway_wide", _highway(B=0), BAD_SHAPE, "bad shape"),
    ("ssv_column_highway_wide", _highway(B=65), BAD_SHAPE, "bad shape"),
    ("ssv_column_highway_wide", _highway(k=1), UNSUPPORTED, "kernel size"),
    ("ssv_column_highway_wide", _highway(k=5), UNSUPPORTED, "kernel size"),
    ("ssv_column_highway_wide", _highway(C=20), UNSUPPORTED, "multiple of 8"),
    ("ssv_column_highway_wide", _highway(C=288), UNSUPPORTED, "multiple of 8"),
    ("ssv_column_highway_wide", _highway(Bw=40), UNSUPPORTED, "column tile"),
    ("ssv_column_highway_wide", _highway(out=X), BAD_SHAPE, "input column"),
    ("ssv_column_pwln_wide", _pwln(x=None), BAD_SHAPE, "null"),
    ("ssv_column_pwln_wide", _pwln(gamma=None), BAD_SHAPE, "null"),
    ("ssv_column_pwln_wide", _pwln(act=3), BAD_SHAPE, "bad shape"),
    ("ssv_column_pwln_wide", _pwln(Cout=513), UNSUPPORTED, "channels"),
    ("ssv_column_pwln_wide", _pwln(Bw=48), UNSUPPORTED, "column tile"),
    ("ssv_attention_column_wide", _attn(kv=None), BAD_SHAPE, "null"),
    ("ssv_attention_column_wide", _attn(U=0), BAD_SHAPE, "shared texts"),
    ("ssv_attention_column_wide", _attn(U=7), BAD_SHAPE, "shared texts"),
    ("ssv_attention_column_wide", _attn(N=2000, kv_bs=2 * 256 * 2000), UNSUPPORTED, "at most"),
    ("ssv_synth_column_advance_wide", _advance(Y=None), BAD_SHAPE, "bad argument"),
    ("ssv_synth_column_advance_wide", _advance(T=0), BAD_SHAPE, "bad argument"),
])
def test_bad_arguments_fail_before_the_device(entry, args, code, word):
    from spoofsv_amd import _lib
    L = _lib.lib()
    assert getattr(L, entry)(*args) == code
    assert word in L.ssv_last_error().decode()


def test_split_modes_need_the_resident_planes():
    from spoofsv_amd import _lib
    L = _lib.lib()
    prev = L.ssv_set_precision(2)
    try:
        assert L.ssv_column_highway_wide(*_highway(w_packed=None)) == BAD_SHAPE
        assert "resident planes" in L.ssv_last_error().decode()
        assert L.ssv_column_pwln_wide(*_pwln(w_packed=None)) == BAD_SHAPE
    finally:
        L.ssv_set_precision(prev)


@pytest.mark.parametrize("n_speakers", [1, 5, 108])
@pytest.mark.parametrize("per_batch", [1, 4, 108, 200])
def test_speaker_groups_cover_every_pair_once_in_file_order(n_speakers, per_batch):
    from spoofsv_amd.harness import plan_utterance_groups
    U = 20
    groups = plan_utterance_groups(n_speakers, U, per_batch)
    flat = [pair for g in groups for pair in g]
    assert flat == [(s, u) for s in range(n_speakers) for u in range(U)]          # today's loop: speaker by speaker, sentence by sentence
    assert len(groups) == -(-n_speakers // per_batch)
    for g in groups:
        assert 0 < len(g) <= per_batch * U and len(g) % U == 0
        assert all(u == b % U for b, (s, u) in enumerate(g))                        # item b speaks text b % U
        assert all(s == g[0][0] + b // U for b, (s, u) in enumerate(g))
    assert all(len(g) == per_batch * U for g in groups[:-1])
    with pytest.raises(ValueError):
        plan_utterance_groups(n_speakers, U, 0)


def test_byte_helper_equals_a_hand_count():
    from spoofsv_amd import synth
    # 40 items -> Bw = 64 columns; hidden 32, 80 mel bins, 17 characters, 33 frames, a text per item, 16 highway layers
    B, Bw, N, T, d, F = 40, 64, 17, 33, 32, 80
    want = (B * 2 * d * N * 4            # K | V
            + F * Bw * 4                 # input column
            + T * F * Bw * 4             # Y, frame-major
            + B * N * T * 4              # A
            + B * 8 + 4                  # pma, frame counter
            + 2 * d * Bw * 4             # speaker terms of conv1 / conv3
            + 2 * d * Bw * 4             # two ping-pong columns
            + 2 * d * Bw * 4             # [r ; q]
            + F * Bw * 4                 # output column
            + 16 * T * d * Bw * 4)       # input histories
    assert synth.wide_synth_bytes(B, N, T, hidden=d, freq_bins=F) == want
    # shared texts: K | V of the U texts only
    assert synth.wide_synth_bytes(B, N, T, hidden=d, freq_bins=F, shared_texts=8) == want - (B - 8) * 2 * d * N * 4
    # what __init__ allocates is this list
    total = 0
    for name, shape, size in synth._wide_buffers(B, N, T, d, F):
        n = size
        for s in shape:
            n *= s
        total += n
    assert total == want
    # the full-size run of 108 speakers x 20 sentences: 5.4 MB of history per item dominate
    assert 11e9 < synth.wide_synth_bytes(2160, 43, 326) < 13e9


def _dump_synth_calls():
    """tools/dump_synth_calls.py: the recorder of one synthesis step's library calls, shared with the tool that wrote the fixture."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("dump_synth_calls", os.path.join(root, "tools", "dump_synth_calls.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool, os.path.join(root, "tests", "golden", "synth_step_calls.json")


def test_one_step_launches_what_the_committed_record_says():
    """One step of IncrementalSynthesizer (50 calls) and of WideSynthesizer (26), conditioned and not, and the wide step with shared
    texts in a split mode, recorded without a device: the same library entries in the same order with the same scalars, buffers,
    parameters, weight copies and planes as tests/golden/synth_step_calls.json, which was recorded BEFORE the synthesizers shared a
    column schedule.  The replayed step is what a free run's time goes to; the fixture is never regenerated from a later synth.py."""
    import json
    tool, path = _dump_synth_calls()
    want = json.load(open(path))
    got = json.loads(json.dumps(tool.collect()))
    assert sorted(got) == sorted(want) == sorted(tool.CONFIGS) and len(want) == 5
    for cfg in sorted(want):
        assert len(want[cfg]) == (50 if cfg.startswith("incremental") else 26), cfg
        for i, (g, w) in enumerate(zip(got[cfg], want[cfg])):
            assert g == w, (cfg, i)
        assert len(got[cfg]) == len(want[cfg]), cfg
    split = want["wide/conditioned/shared_texts=3/f16x2"]                  # every launch is given the planes of its own weight
    w_at = {"ssv_column_pwln_wide": 2, "ssv_column_highway_wide": 1}      # (w, w_packed) follow each other in both prototypes
    pairs = [(c[w_at[c[0]]], c[w_at[c[0]] + 1]) for c in split if c[0] in w_at]
    assert len(pairs) == 24 and all(w.endswith(".weight") and pl == "planes:" + w[len("param:"):] for w, pl in pairs)
    assert tool.render(got) == open(path).read()


def _small_melsyn(condition):
    from spoofsv_amd.tts import melSyn
    return melSyn(34, condition, 200 if condition else None, textemb_dim=16, freq_bins=80, hidden_dim=32).eval()


@pytest.mark.parametrize("condition", [True, False])
def test_column_schedule_is_the_models_forward_order(condition):
    """column_schedule(model): 26 operations in the order of audioEncoder.forward / audioDecoder.forward (the modules' registration
    order, read from named_modules()), each reading what the one before wrote, highway histories 0..15, speaker terms exactly when
    the model is conditioned."""
    from spoofsv_amd import synth
    from spoofsv_amd.tts import highwayConv
    m = _small_melsyn(condition)
    sched = synth.column_schedule(m)
    assert len(sched) == 26
    names = {id(mod): name for name, mod in m.named_modules()}

    def layers(part):                       # the convs (with the LayerNorm registered right after) and highway layers of a part, in order
        mods = list(getattr(m, part).named_modules())
        out = []
        for (name, mod), nxt in zip(mods, mods[1:] + [(None, None)]):
            if isinstance(mod, highwayConv):
                out.append(("highway", (name,)))
            elif type(mod).__name__ == "Conv1d" and not name.endswith(".conv") and name != "conv":
                out.append(("link", (name, nxt[0])))
        return [(kind, tuple(part + "." + n for n in ns)) for kind, ns in out]

    want = layers("audio_encoder") + [("attention", ())] + layers("audio_decoder") + [("advance", ())]
    assert [(op.kind, tuple(names[id(x)] for x in op.mods)) for op in sched] == want
    assert [k for k, _ in want].count("link") == 8 and [k for k, _ in want].count("highway") == 16
    # the buffers: a chain from mel_cur back to mel_cur, ping-pong between a and b except where the step leaves it
    assert sched[0].src == "mel_cur" and sched[-1].dst == "mel_cur"
    for prev, op in zip(sched, sched[1:]):
        assert op.src == prev.dst
    last_link = [op for op in sched if op.kind == "link"][-1]
    for op in sched[:-1]:
        if op.kind == "attention":
            assert op.dst == "rq"
        elif op is last_link:
            assert op.dst == "y_cur" and op.act == 2
        else:
            assert op.dst in ("a", "b") and op.dst != op.src
    assert sched[-2] is last_link
    assert [op.hist for op in sched if op.kind == "highway"] == list(range(16))
    assert all(op.hist is None for op in sched if op.kind != "highway")
    assert [op.spk for op in sched if op.kind == "link"] == ([("s1" if condition else None), None, ("s2" if condition else None)] + [None] * 5)
    assert [op.act for op in sched if op.kind == "link"] == [1, 1, 0, 0, 1, 1, 1, 2]
    assert all(op.spk is None for op in sched if op.kind != "link")


@pytest.mark.parametrize("attr,value", [("causal", False), ("dilation", 0), ("kernel_size", 1), ("dimension", 64)])
@pytest.mark.parametrize("layer", ["audio_encoder.hci2.hc3", "audio_decoder.hc2"])
def test_column_schedule_refuses_a_layer_the_step_cannot_run(layer, attr, value):
    """One highway layer that is not causal, has no kernel of 3, another width or no positive dilation: refused, by the schedule and so
    by both column synthesizers under their own names, before anything is allocated."""
    from spoofsv_amd import synth
    m = _small_melsyn(True)
    setattr(m.get_submodule(layer), attr, value)
    with pytest.raises(RuntimeError, match="unexpected highwayConv configuration"):
        synth.column_schedule(m)
    for cls in (synth.IncrementalSynthesizer, synth.WideSynthesizer):
        with pytest.raises(RuntimeError, match=cls.__name__ + ": unexpected highwayConv configuration"):
            cls(m, 6, 5, 4, "cpu")


def test_synthesizers_share_one_lifecycle_and_one_fifo_cache_per_kind(monkeypatch):
    """One ``run`` and one ``_capture`` for the three synthesizers; ``run`` resets the state BEFORE a capture as well as after it, on
    every path (the warm-up step of a capture runs at the current frame index); the cache holds four synthesizers per kind, first in
    first out, and rebuilds for another model object or moved parameters."""
    import torch
    from spoofsv_amd import synth
    kinds = (synth.GraphSynthesizer, synth.IncrementalSynthesizer, synth.WideSynthesizer)
    for cls in kinds:
        assert cls.run is synth._Replayed.run and cls._capture is synth._Replayed._capture
        assert "run" not in vars(cls) and "_capture" not in vars(cls)
    m = _small_melsyn(False)
    tool, _ = _dump_synth_calls()
    with tool.stubbed(0):
        g = synth.IncrementalSynthesizer(m, 6, 5, 4, "cpu")
        log = []
        monkeypatch.setattr(g, "_refresh", lambda: log.append("refresh"))
        monkeypatch.setattr(g, "_load", lambda text, spk: log.append("load"))
        monkeypatch.setattr(g, "_reset", lambda: log.append("reset"))
        monkeypatch.setattr(g, "_result", lambda: log.append("result"))

        class Graph:
            def replay(self):
                log.append("replay")

        def capture():
            assert log[-1] == "reset"
            log.append("capture")
            g.graph = Graph()
        monkeypatch.setattr(g, "_capture", capture)
        text = torch.zeros((6, 1, 5), dtype=torch.long)
        g.run(text, None)
        assert log == ["refresh", "load", "reset", "capture", "reset"] + ["replay"] * 4 + ["result"]
        del log[:]
        g.run(text, None)
        assert log == ["refresh", "load", "reset"] + ["replay"] * 4 + ["result"]
        g.graph = None                                   # an invalidation after a completed run: reset comes before the capture
        del log[:]
        g.run(text, None)
        assert log[:5] == ["refresh", "load", "reset", "capture", "reset"]
        with pytest.raises(RuntimeError, match=r"IncrementalSynthesizer was built for text ids of shape \(6, 1, 5\), got \(5, 1, 5\)"):
            g.run(text[:5], None)
    # the cache
    built = []
    monkeypatch.setattr(synth.IncrementalSynthesizer, "__init__", lambda self, model, *shape: built.append(shape) or
                        self.__dict__.update(model=model, addresses=synth._addresses(model)))
    monkeypatch.setitem(synth._CACHES, synth.IncrementalSynthesizer, {})
    first = synth._cached(synth.IncrementalSynthesizer, m, 6, 5, 4, "cpu")
    assert synth._cached(synth.IncrementalSynthesizer, m, 6, 5, 4, "cpu") is first and len(built) == 1
    for frames in (5, 6, 7):
        synth._cached(synth.IncrementalSynthesizer, m, 6, 5, frames, "cpu")
    assert synth._cached(synth.IncrementalSynthesizer, m, 6, 5, 4, "cpu") is first and len(built) == 4
    synth._cached(synth.IncrementalSynthesizer, m, 6, 5, 8, "cpu")              # a fifth: the oldest leaves
    assert len(synth._CACHES[synth.IncrementalSynthesizer]) == 4
    assert synth._cached(synth.IncrementalSynthesizer, m, 6, 5, 4, "cpu") is not first and len(built) == 6
    again = synth._cached(synth.IncrementalSynthesizer, m, 6, 5, 8, "cpu")
    m.audio_decoder.conv5.bias.data = m.audio_decoder.conv5.bias.data.clone()    # a parameter moved: a new synthesizer
    assert synth._cached(synth.IncrementalSynthesizer, m, 6, 5, 8, "cpu") is not again
    assert len(synth._CACHES[synth.IncrementalSynthesizer]) == 4 and synth._CACHE_MAX == 4
