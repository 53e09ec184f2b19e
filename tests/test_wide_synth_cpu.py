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
