"""CPU checks of the vocoder's FFT back end: the C ABI of its six entries, their host-side argument checks and tables, the bar rule of
tests/_fft_vocoder_ref.py, and the index arithmetic of spoofsv_amd/csrc/fft_core.h run on the host under the address sanitizer
(tests/fft_core_check.cpp: a stand-alone program, run as a child process)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import _fft_vocoder_ref as R
from oracle import vocoder_oracle as vo
from spoofsv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ssv_fft_tables_floats", "ssv_fft_tables_host", "ssv_fft_frame_tile", "ssv_stft_fft", "ssv_istft_frames_fft", "ssv_ola_signal_fm",
           "ssv_gl_step_fft")
SIZES = (64, 128, 256, 512, 1024, 2048)


def _table(n_fft):
    L = _lib.lib()
    tab = np.empty(L.ssv_fft_tables_floats(n_fft), dtype=np.float32)
    assert L.ssv_fft_tables_host(tab.ctypes.data, n_fft) == 0
    return tab


def test_header_declares_and_library_exports_the_entries():
    protos = _lib.parse_header()
    L = _lib.lib()
    raw = ctypes.CDLL(_lib.LIBPATH)
    for name in ENTRIES:
        assert name in protos and hasattr(raw, name), name
    assert protos["ssv_fft_tables_floats"][0] is ctypes.c_size_t
    assert protos["ssv_gl_step_fft"][2] == ["fr", "inv_env", "tab", "mag", "tprev", "alpha", "reb", "proj", "B", "n_fft", "T", "hop", "stream"]
    assert L.ssv_version() == 7


def test_bad_arguments_fail_before_the_device():
    L = _lib.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)          # `one`: never dereferenced, the checks come first
    n = 256 * 24
    calls = {
        "stft": lambda y=one, tab=one, spec=one, B=1, n=n, N=1024, hop=256, T=None: L.ssv_stft_fft(y, tab, spec, B, n, N, hop, 1 + n // hop if T is None else T, null),
        "inv": lambda spec=one, tab=one, fr=one, B=1, N=1024, T=25: L.ssv_istft_frames_fft(spec, tab, fr, B, N, T, null),
        "ola": lambda fr=one, env=one, y=one, B=1, N=1024, T=25, hop=256: L.ssv_ola_signal_fm(fr, env, y, B, N, T, hop, null),
        "gl": lambda fr=one, env=one, tab=one, mag=one, tprev=null, reb=one, proj=one, B=1, N=1024, T=25, hop=256:
            L.ssv_gl_step_fft(fr, env, tab, mag, tprev, 0.5, reb, proj, B, N, T, hop, null),
    }
    # NULL pointers
    assert calls["stft"](y=null) == -1 and b"stft_fft" in L.ssv_last_error()
    assert calls["stft"](tab=null) == -1 and calls["stft"](spec=null) == -1
    assert calls["inv"](spec=null) == -1 and calls["inv"](tab=null) == -1 and calls["inv"](fr=null) == -1
    assert calls["ola"](fr=null) == -1 and calls["ola"](env=null) == -1 and calls["ola"](y=null) == -1
    for k in ("fr", "env", "tab", "mag", "reb", "proj"):
        assert calls["gl"](**{k: null}) == -1, k
    assert calls["gl"](tprev=one, reb=one) == -1 and b"alias" in L.ssv_last_error()
    assert L.ssv_fft_tables_host(null, 1024) == -1
    assert calls["inv"](fr=ctypes.c_void_p(20)) == -1 and b"8-byte" in L.ssv_last_error()        # frames are stored two floats at a time
    # sizes no transform exists for
    for bad in (1000, 4096, 32):
        for name in ("stft", "inv", "gl"):
            assert calls[name](N=bad, **({"n": 8192} if name == "stft" else {})) == -2, (name, bad)
            assert b"n_fft" in L.ssv_last_error(), name
        assert L.ssv_fft_tables_host(one, bad) == -2 and b"n_fft" in L.ssv_last_error()
        assert L.ssv_fft_tables_floats(bad) == 0
    # shapes
    assert calls["stft"](hop=2048, n=8192) == -1                     # hop > n_fft
    assert calls["gl"](hop=2048) == -1 and calls["ola"](hop=2048) == -1
    assert calls["gl"](T=3) == -1 and calls["ola"](T=3) == -1        # hop * (T - 1) = 512 <= n_fft / 2
    assert calls["stft"](n=512) == -1                                # n <= n_fft / 2
    assert calls["stft"](T=7) == -1                                  # T != 1 + n / hop
    for name in calls:
        assert calls[name](B=0) == -1, name
    assert calls["inv"](T=0) == -1 and calls["stft"](hop=0, T=25) == -1


def test_frame_tile_is_positive_for_every_supported_size_only():
    L = _lib.lib()
    for n_fft in SIZES:
        t = L.ssv_fft_frame_tile(n_fft)
        assert t > 0 and t & (t - 1) == 0 and L.ssv_fft_tables_floats(n_fft) == 2 * n_fft, n_fft
    assert L.ssv_fft_frame_tile(1024) >= 16                          # runs of 64 bytes in the T-fastest arrays at the synthesis size
    for bad in (0, -1024, 32, 96, 1000, 4096):
        assert L.ssv_fft_frame_tile(bad) < 0, bad


@pytest.mark.parametrize("n_fft", SIZES)
def test_tables_window_bitwise_twiddles_within_half_an_ulp(n_fft):
    tab = _table(n_fft)
    assert np.array_equal(tab[:n_fft].view(np.uint32), vo.hann_periodic(n_fft).astype(np.float32).view(np.uint32))
    ang = 2.0 * np.pi * np.arange(n_fft // 2) / n_fft
    for got, ref in ((tab[n_fft:n_fft + n_fft // 2], np.cos(ang)), (tab[n_fft + n_fft // 2:], np.sin(ang))):
        # a float64 value rounded once lies within half a float32 ulp of it (the ulp of the neighbour below at a power of two is
        # smaller: take the ulp of the smaller magnitude); the two libms' float64 results may differ in their last bit, 2^-52
        ulp = np.minimum(np.spacing(got.astype(np.float32)), np.spacing(np.abs(ref).astype(np.float32))).astype(np.float64)
        assert np.all(np.abs(got.astype(np.float64) - ref) <= 0.5 * np.abs(ulp) + 2.0 ** -52 * np.abs(ref) + 1e-300)


def test_unknown_transform_is_a_value_error_and_cpu_devices_still_fail_loudly():
    from spoofsv_amd.vocoder import Vocoder
    with pytest.raises(ValueError, match="transform"):
        Vocoder(transform="dct")
    with pytest.raises(ValueError, match="transform"):
        Vocoder(1024, 256, device="cpu", transform="dct")            # before anything else
    with pytest.raises(ValueError, match="64 to 2048"):
        Vocoder(1000, 250, device="cpu", transform="fft")
    with pytest.raises(ValueError, match="64 to 2048"):
        Vocoder(4096, 1024, device="cpu", transform="fft")
    for tr in ("dft", "fft"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            Vocoder(128, 32, device="cpu", transform=tr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):       # any integer type is a size: the range check passes
        Vocoder(np.int64(1024), np.int32(256), device="cpu", transform="fft")
    with pytest.raises(TypeError):
        Vocoder(1024.0, 256, device="cpu", transform="fft")


def test_the_emulation_stays_below_2e_7_for_one_transform():
    """Guards the helper the GPU bars are computed with: a float32 chain that lost precision would widen every bar."""
    for n_fft, hop, T in R.SHAPES:
        rng = np.random.RandomState(n_fft + T)
        y = R.wave(rng, hop * (T - 1))
        ref = vo.stft(y, n_fft, hop)
        e = R.rel_err(R.stft32(y, n_fft, hop), ref)
        spec = rng.randn(n_fft // 2 + 1, T) + 1j * rng.randn(n_fft // 2 + 1, T)
        ei = R.rel_err(R.istft32(spec, hop), vo.istft(spec.astype(np.complex64).astype(np.complex128), hop))
        print("(%d, %d, %d): emulation stft %.2e, istft with its overlap-add %.2e" % (n_fft, hop, T, e, ei))
        assert e < 2e-7, (n_fft, hop, T, e)
        # the inverse chain rounds three more times per sample than one transform (the window product, the overlap-add of up to
        # n_fft / hop = 4 frames, the envelope division), each within 2^-24 = 6e-8 of the peak: 2e-7 + 3 * 6e-8 < 4e-7.
        # Measured here: 1.3e-7 .. 2.6e-7.
        assert ei < 4e-7, (n_fft, hop, T, ei)


# ---- the index arithmetic of fft_core.h on the host ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/fft_core_check.cpp compiled with the address and undefined-behaviour sanitizers, their runtimes linked statically; run as a
    child process of its own in this process's environment."""
    d = tmp_path_factory.mktemp("fft_core_check")
    exe = str(d / "fft_core_check")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-Wall", "-Werror",
                        os.path.join(ROOT, "tests", "fft_core_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ)                       # as it is: the sanitizer runtimes are inside the executable, no library order matters
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=0"

    def run(mode, n_fft, hop, count, *arrays):
        paths = []
        for i, a in enumerate(arrays):
            p = str(d / ("in%d.f32" % i))
            np.ascontiguousarray(a, dtype=np.float32).tofile(p)
            paths.append(p)
        out = str(d / "out.f32")
        r = subprocess.run([exe, mode, str(n_fft), str(hop), str(count)] + paths + [out], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (mode, n_fft, hop, count, r.returncode, r.stderr[-3000:])
        return np.fromfile(out, dtype=np.float32)
    return run


def _cases():
    L = _lib.lib()
    for n_fft in SIZES:
        tile = L.ssv_fft_frame_tile(n_fft)
        yield n_fft, n_fft // 4, tile + 3                            # two tiles, the last one short
    yield 512, 160, 30                                               # hop does not divide n_fft; first tile = last tile
    yield 1024, 256, 5                                               # a short signal inside one tile: every frame reflects
    yield 64, 64, 66                                                 # hop = n_fft


def test_staged_transforms_of_a_frame_tile_match_numpy_fft_in_float64(checker):
    for n_fft, hop, T in _cases():
        rng = np.random.RandomState(n_fft + hop + T)
        F, tab = n_fft // 2 + 1, _table(n_fft)
        y = R.wave(rng, hop * (T - 1) + hop // 3)                    # a length that is no multiple of hop
        ref = vo.stft(y, n_fft, hop)
        assert ref.shape[1] == T
        got = checker("stft", n_fft, hop, len(y), y, tab).reshape(2 * F, T)
        e, b = R.rel_err(got, R.packed(ref)), R.bar(R.stft32(y, n_fft, hop), ref)
        print("stft (%d, %d, %d): %.2e, bar %.2e" % (n_fft, hop, T, e, b))
        assert e <= b, ("stft", n_fft, hop, T, e, b)
        spec = (rng.randn(F, T) + 1j * rng.randn(F, T)).astype(np.complex64)        # DC and Nyquist carry imaginary parts: ignored
        w = vo.hann_periodic(n_fft)
        ref = np.stack([w * np.fft.irfft(spec[:, t].astype(np.complex128), n_fft) for t in range(T)])
        got = checker("istft", n_fft, hop, T, R.packed(spec), tab).reshape(T, n_fft)
        e, b = R.rel_err(got, ref), R.bar(R.inverse_frames32(spec, n_fft), ref)
        print("inverse frames (%d, %d, %d): %.2e, bar %.2e" % (n_fft, hop, T, e, b))
        assert e <= b, ("istft", n_fft, hop, T, e, b)


def test_span_and_reflect_arithmetic_of_the_griffin_lim_step(checker):
    """Overlap-add, envelope, trim, reflect padding, re-framing and the forward transform from frame-major frames, every tile of a short
    signal -- the first and the last, which reflect, among them -- against stft(istft(.)) of the oracle's pieces in float64."""
    from spoofsv_amd.vocoder import _inv_envelope
    for n_fft, hop, T in _cases():
        rng = np.random.RandomState(7 * n_fft + hop + T)
        F, tab = n_fft // 2 + 1, _table(n_fft)
        fr = (rng.randn(T, n_fft) * vo.hann_periodic(n_fft)[None]).astype(np.float32)
        env = vo.window_sumsquare(T, n_fft, hop)
        y64 = np.zeros(n_fft + hop * (T - 1))
        for t in range(T):
            y64[t * hop:t * hop + n_fft] += fr[t].astype(np.float64)
        nz = env > np.finfo(np.float32).tiny
        y64[nz] /= env[nz]
        y64 = y64[n_fft // 2:-(n_fft // 2)]
        ref = vo.stft(y64, n_fft, hop)
        emu = R.stft32(R.overlap_add32(fr, hop), n_fft, hop)
        got = checker("gl", n_fft, hop, T, fr, _inv_envelope(n_fft, hop, T), tab).reshape(2 * F, T)
        e, b = R.rel_err(got, R.packed(ref)), R.bar(emu, ref)
        print("griffin-lim span (%d, %d, %d): %.2e, bar %.2e" % (n_fft, hop, T, e, b))
        assert e <= b, (n_fft, hop, T, e, b)
