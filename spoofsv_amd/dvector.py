"""Whole-utterance d-vector extraction on one ROCm device: ``GE2E/dvector_create.py`` of the reference for ragged batches.

For every utterance the reference computes the log-mel frames of every (concatenated) voiced segment, cuts them into 24-frame windows
every 12 frames, embeds every window and averages the window embeddings in partitions of about 0.4 s -- the ``*_sequence.npy`` rows
uis-rnn reads.  Here the voiced intervals are an INPUT (webrtcvad stays on the host, out of scope); everything after them runs on the
device: ``ssv_span_frames`` (all centred frames of all spans, staged through LDS) -> the DFT as the library's 1x1 convolution in exact
fp32 -> ``ssv_power_mel_log`` -> ``ssv_gather_windows`` -> ``SpeechEmbedder`` (``ssv_lstm_fwd_cached``) -> ``ssv_segment_mean``.

The first half of this file is host logic in plain integers and float64, importable without a device; every function names the
reference lines it restates.  ``DvectorExtractor`` is the device pipeline.  There is no CPU fallback: a non-ROCm tensor raises.
"""
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, ops
from .ops import _p
from .wave import check_wave

TILE = 64          # frames of one ssv_span_frames tile (DV_TILE in csrc/dvector.hip: the kernel skips a longer one)


# ------------------------------------------------------------------------------------------------------------ host logic
def spans_from_vad(times, sr, n):
    """``concat_segs`` (dvector_create.py:24-36) on what ``VAD_chunk`` returns (VAD_segments.py:130-150): ``times`` are (start, end)
    seconds of chunks of at most 0.4 s, whose samples are ``audio[int(start * sr):int(end * sr)]`` (:145, :149).  Chunks with
    ``times[i][1] == times[i + 1][0]`` -- exact float equality, as :29 compares -- are concatenated, so a joined run is the sample span
    [int(first start * sr), int(last end * sr)) of an ``n``-sample waveform, clipped to it as Python's slices clip.  Returns a list of
    (start, end) ints, one per entry of ``concat_segs``' result (a span may be empty, as a segment there may be)."""
    times = list(times)
    if not times:
        return []

    def clip(t0, t1):
        a, b = min(max(int(t0 * sr), 0), n), min(max(int(t1 * sr), 0), n)
        return a, max(a, b)
    spans = []
    first = times[0][0]
    for i in range(len(times) - 1):
        if times[i][1] == times[i + 1][0]:
            continue
        spans.append(clip(first, times[i][1]))
        first = times[i + 1][0]
    spans.append(clip(first, times[-1][1]))                      # the for ... else of :34-35
    return spans


def frames_of(length, hop):
    """Frames of ``librosa.core.stft(y, hop_length=hop)`` with its default ``center=True`` (dvector_create.py:43) for ``length`` samples."""
    return 1 + int(length) // int(hop)


def windows_of(F, window=24, shift=12):
    """Windows ``get_STFTs`` keeps of F frames (dvector_create.py:48-52): j = 0, shift, ... while ``j + window < F`` -- strictly, so a
    segment of exactly ``window`` frames gives none."""
    return max(0, (int(F) - window + shift - 1) // shift)


def align_partitions(n):
    """The partition list of ``align_embeddings`` (dvector_create.py:55-69) for ``n`` window embeddings, with the reference's own
    float expressions; the ``for ... else`` always appends the last partition (for n = 0 that is the empty (0, 0))."""
    partitions = []
    start = end = 0
    j = 1
    for i in range(int(n)):
        if (i * .12) + .24 < j * .401:
            end = end + 1
        else:
            partitions.append((start, end))
            start = end
            end = end + 1
            j += 1
    partitions.append((start, end))
    return partitions


def plan(spans_per_utterance, hop, window=24, shift=12, lengths=None, tile=TILE):
    """The compact tables of one batch.  ``spans_per_utterance``: per utterance (= row of the waveform batch) a list of (start, end)
    sample spans, clipped here to [0, lengths[row]) when ``lengths`` is given.  A span with no window (``frames_of(len) <= window``,
    the strict compare of dvector_create.py:49) is not framed at all; the frames of the others are numbered consecutively in (row, span)
    order -- the compact frame index g -- and so are their windows.  An utterance with no window contributes no row and is listed in
    ``empty`` (the reference would crash there, in ``np.stack([])``, :98).  Returns a namespace of

    * ``tiles`` (n_tiles, 6) int32: (row, span start, span end, first frame of the tile in its span, its g, frame count <= tile),
    * ``g0`` (n_windows,) int32: the first compact frame of every window (windows never straddle spans),
    * ``offs`` (rows + 1,) int32: window offsets of ``align_partitions`` of every utterance's windows, all utterances in order,
    * ``utt_offs`` (B + 1,) int32: window offsets per utterance, ``rows_per_utterance``, ``windows_per_utterance``, ``empty``,
    * ``n_frames``, ``n_windows``."""
    hop, window, shift, tile = int(hop), int(window), int(shift), int(tile)
    if hop <= 0 or window <= 0 or shift <= 0 or tile <= 0:
        raise ValueError("plan: hop, window, shift and tile must be positive")
    tiles, g0, offs, utt_offs, rows, wins, empty = [], [], [0], [0], [], [], []
    g = 0
    for row, spans in enumerate(spans_per_utterance):
        nw_row = 0
        for (s, e) in spans:
            s, e = int(s), int(e)
            if lengths is not None:
                n = int(lengths[row])
                s, e = min(max(s, 0), n), min(max(e, 0), n)
            F = frames_of(e - s, hop) if e > s else 0
            nw = windows_of(F, window, shift)
            if nw == 0:
                continue
            for f in range(0, F, tile):
                tiles.append((row, s, e, f, g + f, min(tile, F - f)))
            g0.extend(g + shift * k for k in range(nw))
            g += F
            nw_row += nw
        base = utt_offs[-1]
        utt_offs.append(base + nw_row)
        wins.append(nw_row)
        if nw_row == 0:
            empty.append(row)
            rows.append(0)
            continue
        parts = align_partitions(nw_row)
        rows.append(len(parts))
        offs.extend(base + b for (_, b) in parts)
    return SimpleNamespace(tiles=np.asarray(tiles, dtype=np.int32).reshape(-1, 6), g0=np.asarray(g0, dtype=np.int32),
                           offs=np.asarray(offs, dtype=np.int32), utt_offs=np.asarray(utt_offs, dtype=np.int32),
                           rows_per_utterance=rows, windows_per_utterance=wins, empty=empty, n_frames=g, n_windows=len(g0))


# ------------------------------------------------------------------------------------------------------------ device pipeline
class DvectorExtractor:
    """dvector_create.py:92-101 for a ragged batch on one device.  ``front_end``: a ``TisvFrontEnd`` (its rate, n_fft, hop, mel basis and
    Fourier basis are used; its ``tisv_frame`` is not), ``embedder``: a ``SpeechEmbedder`` on the same device.  ``window`` / ``shift``:
    frames per window and between windows (24 / 12: 240 ms windows with 50 % overlap at a 10 ms hop, :39, :48).

    The plan is COMPACT: only frames of spans that give a window are computed and only their windows embedded, nothing is padded to the
    longest utterance.  Frames go through the frame / spectrum buffers in chunks of at most ``frames_per_call`` (rounded down to whole
    items of ``COLS`` columns); the embedder always sees exactly ``windows_per_call`` rows, the last chunk zero-padded, so that its
    cached workspace -- the split weight planes -- serves every chunk of every call (``ge2e._FWD_CACHE``'s key holds the batch size)."""

    COLS = 256         # columns per item of the frame buffer (R, n_fft, COLS): the convolution's L

    def __init__(self, front_end, embedder, window=24, shift=12, windows_per_call=2048, frames_per_call=65536):
        self.fe, self.net, self.window, self.shift = front_end, embedder, int(window), int(shift)
        if self.window <= 0 or self.shift <= 0 or int(windows_per_call) <= 0 or int(frames_per_call) <= 0:
            raise ValueError("DvectorExtractor: window, shift, windows_per_call and frames_per_call must be positive")
        if self.window * front_end.hop_length <= front_end.nfft // 2:
            raise ValueError("DvectorExtractor: window * hop = %d samples must exceed n_fft / 2 = %d (one reflection per span end)"
                             % (self.window * front_end.hop_length, front_end.nfft // 2))
        if embedder.dims[0] != front_end.nmels:
            raise ValueError("DvectorExtractor: the embedder expects %d mel bins, the front end makes %d" % (embedder.dims[0], front_end.nmels))
        self.windows_per_call = int(windows_per_call)
        self.frames_per_call = max(self.COLS, int(frames_per_call) // self.COLS * self.COLS)

    # ------------------------------------------------------------------ planning
    def plan(self, y16, lengths, spans=None):
        """``spans=None``: one span per utterance, its ``trim_bounds(..., 30)``.  That default reads the (B, 2) bounds to the host ONCE
        (and the lengths, to clip explicit spans) -- the plan's tables are built there."""
        check_wave(y16, lengths, device=self.fe.device)
        if spans is None:
            b = self.fe.trim_bounds(y16, lengths, 30).cpu().tolist()
            spans = [[(s, e)] for s, e in b]
        elif len(spans) != y16.shape[0]:
            raise ValueError("DvectorExtractor: %d span lists for %d utterances" % (len(spans), y16.shape[0]))
        n = [min(max(int(v), 0), y16.shape[1]) for v in lengths.cpu().tolist()]
        return plan(spans, self.fe.hop_length, self.window, self.shift, lengths=n)

    # ------------------------------------------------------------------ stages
    def span_frames(self, y16, tiles, g_base, n_frames, out=None):
        """Compact frames [g_base, g_base + n_frames) of the device tile table ``tiles`` -> (R, nfft, COLS), R = ceil(n_frames / COLS)."""
        fe, Tc = self.fe, self.COLS
        R = -(-n_frames // Tc)
        fr = out if out is not None else torch.empty((R, fe.nfft, Tc), dtype=torch.float32, device=y16.device)
        _lib.call("ssv_span_frames", _p(y16), _p(tiles), _p(fr), y16.shape[0], y16.shape[1], tiles.shape[0], fe.nfft, fe.hop_length, self.window, Tc,
                  R, int(g_base), int(n_frames), ops._stream())
        return fr

    def log_mel(self, y16, pl, timers=None):
        """All frames of the plan -> the compact frames-major log-mel array (ceil(n_frames / COLS) * COLS, nmels); rows past n_frames
        belong to zero frames."""
        fe, Tc, G = self.fe, self.COLS, pl.n_frames
        dev = y16.device
        mel = torch.empty((-(-G // Tc) * Tc, fe.nmels), dtype=torch.float32, device=dev)
        tiles_h = pl.tiles
        tiles = torch.from_numpy(tiles_h).to(dev)
        tick = timers or (lambda name: None)
        for g_base in range(0, G, self.frames_per_call):
            nf = min(self.frames_per_call, G - g_base)
            # tiles are in ascending g: those that overlap [g_base, g_base + nf)
            lo = int(np.searchsorted(tiles_h[:, 4] + tiles_h[:, 5], g_base, side="right"))
            hi = int(np.searchsorted(tiles_h[:, 4], g_base + nf, side="left"))
            tick(None)
            fr = self.span_frames(y16, tiles[lo:hi], g_base, nf)
            tick("frames")
            S = fe.dft(fr)
            tick("dft")
            fe.mel_log(S, out=mel[g_base:g_base + fr.shape[0] * Tc])
            tick("mel")
        return mel

    def gather(self, mel, g0, lo, n, out):
        """Windows [lo, lo + n) of the device table ``g0`` into the first n rows of ``out`` (rows, window, nmels)."""
        _lib.call("ssv_gather_windows", _p(mel), _p(g0[lo:]), _p(out), mel.shape[0], n, self.window, self.fe.nmels,
                  ops._stream())

    def window_features(self, y16, lengths, spans=None, pl=None):
        """The (n_windows, window, nmels) windows themselves -- what the reference stacks at dvector_create.py:98-99 -- and the plan."""
        pl = pl or self.plan(y16, lengths, spans)
        out = torch.empty((pl.n_windows, self.window, self.fe.nmels), dtype=torch.float32, device=y16.device)
        if pl.n_windows:
            self.gather(self.log_mel(y16, pl), torch.from_numpy(pl.g0).to(y16.device), 0, pl.n_windows, out)
        return out, pl

    def window_embeddings(self, y16, lengths, spans=None, pl=None, timers=None):
        """(n_windows, proj) embeddings of every window (eval mode, no_grad), and the plan."""
        pl = pl or self.plan(y16, lengths, spans)
        dev, W = y16.device, self.windows_per_call
        P = self.net.dims[3]
        E = torch.empty((pl.n_windows, P), dtype=torch.float32, device=dev)
        if not pl.n_windows:
            return E, pl
        tick = timers or (lambda name: None)
        mel = self.log_mel(y16, pl, timers)
        g0 = torch.from_numpy(pl.g0).to(dev)
        was_training = self.net.training
        self.net.eval()
        try:
            with torch.no_grad():
                x = torch.zeros((W, self.window, self.fe.nmels), dtype=torch.float32, device=dev)
                for lo in range(0, pl.n_windows, W):
                    n = min(W, pl.n_windows - lo)
                    tick(None)
                    if n < W:
                        x[n:].zero_()                            # the padded last chunk
                    self.gather(mel, g0, lo, n, x)
                    tick("gather")
                    E[lo:lo + n] = self.net(x)[:n]
                    tick("embedder")
        finally:
            self.net.train(was_training)
        return E, pl

    def _means(self, E, offs, normalize):
        P = offs.shape[0] - 1
        out = torch.empty((P, E.shape[1]), dtype=torch.float32, device=E.device)
        if P > 0 and E.shape[0] > 0:
            _lib.call("ssv_segment_mean", _p(E), _p(torch.from_numpy(offs).to(E.device)), _p(out), E.shape[0], P, E.shape[1], int(normalize), ops._stream())
        else:
            out.zero_()
        return out

    # ------------------------------------------------------------------ entry points
    def __call__(self, y16, lengths, spans=None, timers=None):
        """``y16`` (B, n_max) float32 at the front end's rate with int32 device ``lengths``; ``spans``: per utterance a list of (start,
        end) sample spans (``spans_from_vad``), or None for one span per utterance equal to its ``trim_bounds(..., 30)`` -- which reads
        the (B, 2) bounds back to the host once, to build the plan.  Returns (sequence (rows, proj) float32 on the device: the rows of
        ``align_embeddings`` of every utterance in order, rows_per_utterance); an utterance with no window has 0 rows."""
        E, pl = self.window_embeddings(y16, lengths, spans, timers=timers)
        if timers:
            timers(None)
        seq = self._means(E, pl.offs, 0)
        if timers:
            timers("mean")
        return seq, list(pl.rows_per_utterance)

    def utterance_dvectors(self, y16, lengths, spans=None):
        """One unit-norm d-vector per utterance: the mean over ALL its window embeddings, L2-normalised (the utterance-level d-vector
        of the GE2E paper).  (B, proj); the row of an utterance with no window is zeros.  Also returns windows_per_utterance."""
        E, pl = self.window_embeddings(y16, lengths, spans)
        return self._means(E, pl.utt_offs, 1), list(pl.windows_per_utterance)
