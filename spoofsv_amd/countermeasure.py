"""The spoof countermeasure of the reference (``anti_spoofing/``): a conv1d classifier trained with binary cross-entropy to tell bona fide
from spoofed speech, on the HIP path from the waveform to the score.

What each piece replaces in the reference:
  CmLinDisc / CmMelDisc  anti_spoofing/discriminator.py:96-132 / :56-94 (the critics' stack with a sigmoid on top)
  CmSource               ASVspoofDataset.__getitem__ + collate_pad_3 + DataLoader, anti_spoofing/spoof_conv1d.py:43-91, main_spoof_conv1d.py:64
  protocol_items         ASVspoofDataset.__init__, anti_spoofing/spoof_conv1d.py:16-38
  train / score          anti_spoofing/main_spoof_conv1d.py:68-106 / :108-132
  CmResidentCorpus       the same dataset and collate, run once instead of once per epoch (spoof_conv1d.py:43-91 for up to 20,000 epochs)
  CmBucketedStep         the iteration of main_spoof_conv1d.py:84-90, captured per batch width
  cm_eer                 (the ASVspoof tools the reference leaves its score file to)

The classifier's trunk is ``critic._Disc`` -- convolutions, LayerNorms, highway gate, pools and dropout on the HIP kernels -- and its head
(leaky-ReLU, conv5, global average pool, sigmoid, and in training the loss) is ONE fused operator, ``ops.cm_head``.  The optimizer is
``train.FusedAdamEx`` (Adam with weight decay and AMSGrad, one launch).  Features come from ``CorpusFeatureExtractor`` at 16 kHz with
the 22 dB trim of the reference; synthesized speech enters as device waveforms at the synthesizer's rate and is resampled on the device,
so nothing leaves the GPU between synthesis and score.  Training is eager by default (batch widths vary from batch to batch); with
``resident=True`` the features are extracted once into a ``CmResidentCorpus`` and every batch is gathered on the device, and with
``width_buckets`` full batches are replayed from one hipGraph per width bucket (``CmBucketedStep``).

Deviations from the reference, all forced:
  * ``melDisc`` declares ``ln4 = LayerNorm(4)`` behind an 8-channel ``conv4`` (discriminator.py:71-72): its first forward raises, so the
    reference's hard-wired ``feat_type = 'mel'`` never trained and no reference mel checkpoint exists.  ``CmMelDisc`` sizes ln4 to 8.
  * ``melDisc_v1/_v2`` and ``linDisc_v1/_v2`` call ``super(melDisc, self)`` / ``super(linDisc, self)`` from other classes and cannot be
    constructed; they are not built here.
  * flac files are not decoded (no decoder is a dependency of this project): ``protocol_items(ext=...)`` lets a converted corpus in.
  * 1 - pred is evaluated as sigmoid(-z) (see ``ssv_cm_head_fwd``): the reference's float32 subtraction loses q beyond z of about 17.
There is no CPU fallback: a non-ROCm tensor raises.
"""
import argparse
import json
import os
import time as _time

import numpy as np
import torch

from . import _lib, gradarena, ops
from .critic import _Disc
from .ops import _p, _stream
from .train import BucketedReplay, FusedAdamEx, PhasedStep, StagedUpload

CM_RATE = 16000                 # spoof_conv1d.py:45,48
POOLS = {"lin": (8, 4), "mel": (2, 2)}          # discriminator.py:104,108 / :64,68: the two AvgPool1d of CmLinDisc / CmMelDisc
# main_spoof_conv1d.py:52 (lr is torch's default)
ADAM = dict(lr=1e-3, betas=(0.9, 0.98), eps=1e-9, weight_decay=1e-4, amsgrad=True)
_SLOPE = 0.05


class _CmDisc(_Disc):
    def forward(self, x):
        """The reference's output: sigmoid scores (B, 1, 1)."""
        return ops.cm_head(self.trunk(x), self.conv5.weight, self.conv5.bias, None, _SLOPE).view(-1, 1, 1)

    def loss(self, x, labels, live=None):
        """(mean binary cross-entropy of main_spoof_conv1d.py:87, pred (B,)); differentiable once through the loss.  ``live``: two int32 on
        the device, (L, head width), for an ``x`` padded to a wider buffer: its first L columns are the batch, and of what reaches the head
        the first ``head_width(L)`` columns are; loss, scores and gradients are then those of the unpadded batch."""
        if live is None:
            return ops.cm_head(self.trunk(x), self.conv5.weight, self.conv5.bias, labels, _SLOPE)
        return ops.cm_head(self.trunk(x, ops.Live(live, 0)), self.conv5.weight, self.conv5.bias, labels, _SLOPE, ops.Live(live, 1))


class CmLinDisc(_CmDisc):
    """anti_spoofing/discriminator.py:96-132: pools 8 and 4, conv4 16 -> 8 -- the stack of ``critic.linDisc``.  Same sub-module names as the
    reference, so state dicts interchange.  Dropout follows ``self.training`` (the reference calls ``model.eval()`` for scoring)."""

    def __init__(self, freq_bins, disc_dim):
        super().__init__(freq_bins, disc_dim, pool1=8, pool2=4, last=8)


class CmMelDisc(_CmDisc):
    """anti_spoofing/discriminator.py:56-94: pools 2 and 2, conv4 16 -> 8.  DEVIATION: the reference's ``ln4 = LayerNorm(4)`` cannot
    normalise conv4's 8 channels (its forward raises), so ln4 has 8 channels here; no reference mel checkpoint can exist."""

    def __init__(self, freq_bins, disc_dim):
        super().__init__(freq_bins, disc_dim, pool1=2, pool2=2, last=8)


def build_model(cfg, feat_type):
    """main_spoof_conv1d.py:34."""
    if feat_type == "mel":
        return CmMelDisc(int(cfg["COARSE_MELSPEC"]["FREQ_BINS"]), int(cfg["DISC_DIM"]))
    if feat_type == "lin":
        return CmLinDisc(1 + int(cfg["STFT"]["FFT_LENGTH"]) // 2, int(cfg["DISC_DIM"]))
    raise ValueError("feat_type must be 'mel' or 'lin', got %r" % (feat_type,))


# ------------------------------------------------------------------------------------------------------ data
def protocol_items(cfg, step, time, ext=".flac"):
    """The reference's two lists (spoof_conv1d.py:16-38), host logic only: (bona fide paths, spoof paths).  Bona fide: the first 20000
    lines of ``DATA_ROOT_DIR + 'data_path/ordinary/wav.path.train'`` for ``step == 'train'``, the rest otherwise.  Spoof: the lines of the
    protocol (the ASVspoof 2019 LA train protocol, or ``customized_data_<time>.txt``) whose last field is ``spoof``, as
    ``ANTISPOOF_DIR + <ASVspoof2019_LA_train | time> + '/flac/' + <second field> + ext``."""
    train = step == "train"
    with open(cfg["DATA_ROOT_DIR"] + "data_path/ordinary/wav.path.train") as f:
        audio = [ln.strip() for ln in f.readlines()]
    bona = audio[:20000] if train else audio[20000:]
    suffix = ("ASVspoof2019_LA_cm_protocols/ASVspoof2019.LA.cm.train.trn.txt" if train
              else "ASVspoof2019_LA_cm_protocols/customized_data_{}.txt".format(time))
    mid = "ASVspoof2019_LA_train" if train else time
    spoof = []
    with open(cfg["ANTISPOOF_DIR"] + suffix) as f:
        for proto in f.readlines():
            fields = proto.strip().split()
            if fields and fields[-1] == "spoof":
                spoof.append(cfg["ANTISPOOF_DIR"] + mid + "/flac/" + fields[1] + ext)
    return bona, spoof


def epoch_order(n, seed, epoch, shuffle=True):
    """The item order of one epoch: a permutation seeded by (seed, epoch), or 0 .. n - 1."""
    return np.random.default_rng([int(seed), int(epoch)]).permutation(n) if shuffle else np.arange(n)


class CmSource:
    """Bona fide (label 1) and spoof (label 0) items, each side either a list of wav paths (``ge2e_harness.read_wav``) or a device tuple
    ``(waveforms (U, n) float32, lengths (U,) int32, rate)`` -- what ``harness.generate_test_utterances(return_waveforms=True)`` leaves
    on the device per speaker, with the synthesizer's rate added -- or a list of such tuples.  Items are numbered bona fide first, as the
    reference concatenates its labels.  ``batches`` yields the reference's collated dict: ``data_0`` (B, n_mels, w) reduced mel,
    ``data_1`` (B, F, r * w) linear, ``data_2`` (B,) labels, zero-padded to the batch's longest item (collate_pad_3), all on the device,
    from ``CorpusFeatureExtractor(dict(cfg, SAMPLING_RATE=16000))``; items at another rate go through its resampler (22.05 kHz ->
    16 kHz is the ratio 320 / 441, within ``wave.polyphase_bank``'s limits).  The last batch is partial, as ``DataLoader`` gives it."""

    def __init__(self, cfg, bonafide, spoof, batch_size=64, seed=0, device="cuda"):
        from .corpus_features import CorpusFeatureExtractor
        self.cfg = dict(cfg, SAMPLING_RATE=CM_RATE)
        self.fx = CorpusFeatureExtractor(self.cfg, device)
        self.device = self.fx.device
        self.batch_size, self.seed = int(batch_size), int(seed)
        if self.batch_size <= 0:
            raise ValueError("batch_size must be positive")
        self.items, labels = [], []                              # ("path", path) or ("dev", block index, row)
        self.blocks = []
        for side, label in ((bonafide, 1.0), (spoof, 0.0)):
            for it in self._side(side):
                self.items.append(it)
                labels.append(label)
        if not self.items:
            raise ValueError("CmSource: no items")
        self.labels = np.asarray(labels, dtype=np.float32)

    def _side(self, side):
        if isinstance(side, tuple) and len(side) == 3 and torch.is_tensor(side[0]):
            side = [side]
        for it in side:
            if isinstance(it, (str, os.PathLike)):
                yield ("path", os.fspath(it))
                continue
            y, n, rate = it
            ops._dev(y, "waveforms")
            if y.dim() != 2 or n.shape != (y.shape[0],):
                raise ValueError("CmSource: a device block is (waveforms (U, n), lengths (U,), rate)")
            lens = [int(v) for v in n.cpu().tolist()]            # read once, here: batches are then assembled without a readback
            if any(v < 0 or v > y.shape[1] for v in lens):
                raise ValueError("CmSource: a length outside its row")
            self.blocks.append((y.to(self.device, torch.float32).contiguous(), lens, int(rate)))
            for r in range(y.shape[0]):
                yield ("dev", len(self.blocks) - 1, r)

    def __len__(self):
        return len(self.items)

    def n_batches(self):
        return -(-len(self.items) // self.batch_size)

    def order(self, shuffle, epoch=0):
        return epoch_order(len(self.items), self.seed, epoch, shuffle)

    def _waves(self, idx):
        """The items ``idx`` grouped by sample rate: [(rate, positions in the batch, y (b, n_max), lengths (b,))], zero-padded rows."""
        from .ge2e_harness import read_wav
        groups = {}
        for pos, i in enumerate(idx):
            it = self.items[int(i)]
            if it[0] == "path":
                rate, y = read_wav(it[1])
                groups.setdefault(rate, []).append((pos, torch.from_numpy(y), len(y)))
            else:
                y, lens, rate = self.blocks[it[1]]
                groups.setdefault(rate, []).append((pos, y[it[2], :max(lens[it[2]], 1)], lens[it[2]]))
        out = []
        for rate, rows in groups.items():
            n_max = max(int(r[1].shape[0]) for r in rows)
            y = torch.zeros((len(rows), n_max), dtype=torch.float32, device=self.device)
            for k, r in enumerate(rows):
                y[k, :r[1].shape[0]].copy_(r[1], non_blocking=True)
            lens = torch.tensor([r[2] for r in rows], dtype=torch.int32).to(self.device)
            out.append((rate, [r[0] for r in rows], y, lens))
        return out

    def batch(self, idx):
        """The collated batch of the items ``idx`` (in that order)."""
        parts = [(pos,) + tuple(self.fx.collated(y, lens, rate)) for rate, pos, y, lens in self._waves(idx)]
        labels = torch.from_numpy(self.labels[np.asarray(idx, dtype=np.int64)]).to(self.device)
        self.last_rt = [0] * len(idx)                            # the extractor's reduced frame counts of this batch, by position
        for pos, _, _, rt in parts:
            for at, v in zip(pos, rt):
                self.last_rt[at] = int(v)
        if len(parts) == 1 and parts[0][0] == list(range(len(idx))):
            _, mel, lin, _ = parts[0]
            return {"data_0": mel, "data_1": lin, "data_2": labels}
        r = self.fx.r
        w = max(p[1].shape[2] for p in parts)
        mel = torch.zeros((len(idx), self.fx.M, w), dtype=torch.float32, device=self.device)
        lin = torch.zeros((len(idx), self.fx.F, r * w), dtype=torch.float32, device=self.device)
        for pos, m, l, _ in parts:
            at = torch.tensor(pos, dtype=torch.int64, device=self.device)
            mel[at, :, :m.shape[2]] = m
            lin[at, :, :l.shape[2]] = l
        return {"data_0": mel, "data_1": lin, "data_2": labels}

    def batches(self, shuffle=False, epoch=0):
        order = self.order(shuffle, epoch)
        for at in range(0, len(order), self.batch_size):
            yield self.batch(order[at:at + self.batch_size])


# ------------------------------------------------------------------------------------------------------ resident corpus
def head_width(feat_type, L):
    """Columns that reach the classifier head from a batch ``L`` feature frames wide: ``(L // k1) // k2`` for the two pools."""
    k1, k2 = POOLS[feat_type]
    return (int(L) // k1) // k2


def check_width_buckets(buckets):
    """The bucket widths as a list of ints; ``ValueError`` unless they are positive integers in strictly ascending order."""
    if isinstance(buckets, (str, bytes)) or not hasattr(buckets, "__iter__"):
        raise ValueError("width_buckets: a list of widths in feature frames, got %r" % (buckets,))
    out = list(buckets)
    if not out or not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and v > 0 for v in out):
        raise ValueError("width_buckets: widths must be positive integers, got %r" % (buckets,))
    if any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError("width_buckets: widths must be strictly ascending, got %r" % (buckets,))
    return [int(v) for v in out]


def pick_width_bucket(buckets, width):
    """The smallest bucket that holds a batch ``width`` frames wide, or None."""
    for b in buckets:
        if width <= b:
            return b
    return None


def frames_bound(cfg, samples, feat_type):
    """Upper bounds of the items' widths in the feature's own frames, before one waveform is decoded: ``samples`` = [(n, rate)] from the
    wav headers / the device blocks' lengths; an item resampled to 16 kHz is at most ``resampled_width`` samples long, and the 22 dB trim
    only shortens it, so its frame count is at most ``feature_lengths`` of the untrimmed length."""
    from .corpus_features import feature_lengths
    from .wave import resampled_width
    n_fft, hop, r = int(cfg["STFT"]["FFT_LENGTH"]), int(cfg["STFT"]["HOP_LENGTH"]), int(cfg["COARSE_MELSPEC"]["REDUCTION"])
    out = np.zeros((len(samples),), dtype=np.int64)
    for i, (n, rate) in enumerate(samples):
        m = int(n) if int(rate) == CM_RATE else resampled_width(int(n), int(rate), CM_RATE)
        _, rt, lin = feature_lengths(m, n_fft, hop, r)
        out[i] = lin if feat_type == "lin" else rt
    return out


def cm_resident_bytes(n_items, frames, rows, free=None):
    """Device bytes of a resident corpus of ``n_items`` items, ``frames`` feature frames in all, ``rows`` bins per frame: the arena, its
    two tables, the labels and theirs.  With ``free`` (bytes of free device memory): a ``RuntimeError`` naming both figures when the
    corpus does not fit."""
    need = 4 * int(rows) * max(1, int(frames)) + 12 * int(n_items) + 16 * int(n_items)
    if free is not None:
        ops.require_free_bytes(need, None, "CmResidentCorpus: %d items (%d frames of %d bins) need" % (n_items, frames, rows),
                               "train from the wav files instead (resident=False)", free=free)
    return need


class CmResidentCorpus:
    """The countermeasure's features held on the device: a ``CmSource`` is extracted ONCE, in item order, in passes of its batch size
    (``source.batch`` as today, then one ``ssv_corpus_scatter`` of the collated ``data_1`` (``feat_type`` "lin") or ``data_0`` ("mel") into a
    ragged arena), and every later batch is an ``ssv_corpus_gather`` of that arena: no wav file is opened, nothing is padded, uploaded or
    extracted again.  Only the requested feature is held.  An unshuffled batch has the bits of the source's batch; a shuffled epoch uses
    the source's ``epoch_order`` (uploaded once per epoch).  Offers what ``train`` and ``score`` use of a source: ``device``, ``len``,
    ``n_batches()``, ``batch(idx)``, ``batches(shuffle, epoch)`` -- a batch is {"data_1" | "data_0": (B, F, w), "data_2": (B,)}, w the
    batch's longest item -- plus ``gather_into`` for a caller's wider static buffer.  The arena is sized by ``frames_bound`` before anything
    is allocated and refused (``RuntimeError``) when it exceeds the free device memory; ``bytes`` is what it holds.  ROCm only."""

    def __init__(self, source, feat_type):
        self._start(feat_type, source.device, source.batch_size, source.seed)
        cfg = source.cfg
        r = int(cfg["COARSE_MELSPEC"]["REDUCTION"])
        rows = 1 + int(cfg["STFT"]["FFT_LENGTH"]) // 2 if feat_type == "lin" else int(cfg["COARSE_MELSPEC"]["FREQ_BINS"])
        bound = frames_bound(cfg, self._samples(source), feat_type)
        self._allocate(len(source), rows, int(bound.sum()), r if feat_type == "lin" else 1)
        key, mult = self.key, (r if feat_type == "lin" else 1)
        at, used, B = 0, 0, source.batch_size
        while at < self.n:
            b = min(B, self.n - at)
            feat = source.batch(np.arange(at, at + b))[key]
            lens = np.asarray(source.last_rt, dtype=np.int64) * mult          # the extractor's lengths, read once per pass
            if np.any(lens > bound[at:at + b]):
                raise RuntimeError("CmResidentCorpus: an item came out longer than the bound taken from its header")
            self.lens[at:at + b] = lens
            self.offs[at:at + b] = used + np.concatenate([[0], np.cumsum(lens * rows)[:-1]])
            used += int(lens.sum()) * rows
            self.len_d[at:at + b].copy_(torch.from_numpy(self.lens[at:at + b]))
            self.off_d[at:at + b].copy_(torch.from_numpy(self.offs[at:at + b]))
            if feat.stride(2) != 1 or feat.stride(1) != feat.shape[2]:
                feat = feat.contiguous()
            _lib.call("ssv_corpus_scatter", _p(feat), feat.stride(0) if b > 1 else rows * feat.shape[2], b, rows, feat.shape[2], _p(self.arena),
                      self.arena.numel(), _p(self.off_d), _p(self.len_d), self.n, at, _stream())
            at += b
        self.used = used
        self._labels(torch.from_numpy(np.asarray(source.labels, dtype=np.float32)))
        torch.cuda.synchronize(self.device)

    @classmethod
    def from_features(cls, blocks, labels, feat_type, batch_size=64, seed=0, device="cuda"):
        """The corpus of ready features: ``blocks`` a list of (F, len_i) float tensors (cached features; the tests), ``labels`` their
        classes (1 bona fide, 0 spoof)."""
        self = cls.__new__(cls)
        self._start(feat_type, device, batch_size, seed)
        if not blocks or any(b.dim() != 2 or b.shape[0] != blocks[0].shape[0] for b in blocks) or len(labels) != len(blocks):
            raise ValueError("CmResidentCorpus.from_features: blocks are (F, len_i) tensors of one F, with one label each")
        rows = int(blocks[0].shape[0])
        lens = np.asarray([int(b.shape[1]) for b in blocks], dtype=np.int64)
        self._allocate(len(blocks), rows, int(lens.sum()), 1)
        self.lens[:] = lens
        self.offs[:] = np.concatenate([[0], np.cumsum(lens * rows)[:-1]])
        self.used = int(lens.sum()) * rows
        if self.used:
            self.arena[:self.used].copy_(torch.cat([b.to(self.device, torch.float32).reshape(-1) for b in blocks]))
        self.len_d.copy_(torch.from_numpy(self.lens))
        self.off_d.copy_(torch.from_numpy(self.offs))
        self._labels(torch.as_tensor(labels, dtype=torch.float32).reshape(-1))
        torch.cuda.synchronize(self.device)
        return self

    # ---- construction
    def _start(self, feat_type, device, batch_size, seed):
        if feat_type not in POOLS:
            raise ValueError("feat_type must be 'mel' or 'lin', got %r" % (feat_type,))
        self.device = torch.device(device)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("CmResidentCorpus needs a ROCm device: the corpus is filed and gathered by HIP kernels, there is no host fallback")
        self.feat_type, self.key = feat_type, "data_1" if feat_type == "lin" else "data_0"
        self.batch_size, self.seed = int(batch_size), int(seed)
        if self.batch_size <= 0:
            raise ValueError("batch_size must be positive")
        self._epoch = None

    @staticmethod
    def _samples(source):
        """[(samples, rate)] of a ``CmSource``'s items from the wav headers and the device blocks' lengths; nothing is decoded."""
        from scipy.io import wavfile
        out = []
        for it in source.items:
            if it[0] == "path":
                rate, y = wavfile.read(it[1], mmap=True)             # the header, and a map of the samples that is never touched
                out.append((int(y.shape[0]), int(rate)))
            else:
                _, lens, rate = source.blocks[it[1]]
                out.append((lens[it[2]], rate))
        return out

    def _allocate(self, n, rows, frames, min_width):
        self.n, self.rows, self.min_width = int(n), int(rows), int(min_width)
        self.bytes = cm_resident_bytes(self.n, frames, rows, ops.free_bytes(self.device))
        dev = self.device
        self.arena = torch.zeros((max(1, frames * rows),), dtype=torch.float32, device=dev)
        self.lens, self.offs = np.zeros((self.n,), dtype=np.int32), np.zeros((self.n,), dtype=np.int64)
        self.len_d = torch.zeros((self.n,), dtype=torch.int32, device=dev)
        self.off_d = torch.zeros((self.n,), dtype=torch.int64, device=dev)

    def _labels(self, labels):
        self.labels = labels.to(self.device).contiguous()
        self.lab_off = torch.arange(self.n, dtype=torch.int64, device=self.device)          # the labels as an F = 1, len = 1 table
        self.lab_len = torch.ones((self.n,), dtype=torch.int32, device=self.device)

    # ---- what train / score use of a source
    def __len__(self):
        return self.n

    def n_batches(self):
        return -(-self.n // self.batch_size)

    def order(self, shuffle, epoch=0):
        return epoch_order(self.n, self.seed, epoch, shuffle)

    def rows_of(self, order):
        """An item order as the int32 device table the gathers read (one upload)."""
        order = np.ascontiguousarray(order, dtype=np.int32)
        if order.size == 0 or order.min() < 0 or order.max() >= self.n:
            raise ValueError("CmResidentCorpus: the order names an item outside [0, %d)" % self.n)
        return torch.from_numpy(order).to(self.device)

    def width(self, idx):
        """Width of the collated batch of the items ``idx``: the longest of them, as the source pads (host arithmetic)."""
        return max(int(self.lens[np.asarray(idx, dtype=np.int64)].max()), self.min_width)

    def gather_into(self, out, rows, row0, labels=None):
        """``out`` (B, F, W) <- the items ``rows[row0 : row0 + B]`` (``rows``: ``rows_of`` an order), zero-padded to W (an item longer
        than W is clipped); ``labels`` (B,) <- their labels.  ``out`` may be a caller's static buffer wider than the batch."""
        B, F, W = out.shape
        if F != self.rows or out.dtype != torch.float32 or out.stride(2) != 1 or out.stride(1) != W or out.device != self.arena.device:
            raise ValueError("CmResidentCorpus.gather_into: out must be a float32 (B, %d, W) device tensor with dense rows" % self.rows)
        _lib.call("ssv_corpus_gather", _p(self.arena), self.arena.numel(), _p(self.off_d), _p(self.len_d), self.n, _p(rows), rows.numel(), row0,
                  _p(out), B, F, W, out.stride(0) if B > 1 else F * W, _stream())
        if labels is not None:
            _lib.call("ssv_corpus_gather", _p(self.labels), self.n, _p(self.lab_off), _p(self.lab_len), self.n, _p(rows), rows.numel(), row0,
                      _p(labels), B, 1, 1, 1, _stream())

    def gather(self, rows, row0, idx):
        """The collated batch of the items ``idx`` = the host copy of ``rows[row0 : row0 + len(idx)]``."""
        B = len(idx)
        feat = torch.empty((B, self.rows, self.width(idx)), dtype=torch.float32, device=self.device)
        labels = torch.empty((B,), dtype=torch.float32, device=self.device)
        self.gather_into(feat, rows, row0, labels)
        return {self.key: feat, "data_2": labels}

    def batch(self, idx):
        """The collated batch of the items ``idx`` (in that order)."""
        return self.gather(self.rows_of(idx), 0, idx)

    def epoch(self, shuffle=False, epoch=0):
        """(order on the host, its device table) of one epoch; the table is uploaded once and kept until another epoch is asked for."""
        key = (bool(shuffle), int(epoch) if shuffle else 0)
        if self._epoch is None or self._epoch[0] != key:
            order = self.order(shuffle, epoch)
            self._epoch = (key, order, self.rows_of(order))
        return self._epoch[1], self._epoch[2]

    def batches(self, shuffle=False, epoch=0):
        order, rows = self.epoch(shuffle, epoch)
        for at in range(0, self.n, self.batch_size):
            yield self.gather(rows, at, order[at:at + self.batch_size])


# ------------------------------------------------------------------------------------------------------ scores
def cm_eer(scores, labels):
    """Equal error rate of countermeasure scores (higher = more bona fide; labels 1 bona fide, 0 spoof).  Thresholds are the distinct
    scores, the midpoints between neighbours and one beyond each end; at a threshold t a spoof trial scoring >= t is a false acceptance
    and a bona fide trial scoring <= t is a false rejection, so a trial that ties with the threshold counts as an error on BOTH sides
    (a score shared by the two classes cannot separate them).  Returns (FAR + FRR) / 2 at the threshold where |FAR - FRR| is smallest
    (the smaller maximum breaks ties).  A single class raises."""
    s = np.asarray(scores, dtype=np.float64).ravel()
    y = np.asarray(labels).ravel()
    if s.shape != y.shape or not np.all(np.isfinite(s)):
        raise ValueError("cm_eer: scores and labels must be finite and of one length")
    bona, spoof = np.sort(s[y == 1]), np.sort(s[y != 1])
    if bona.size == 0 or spoof.size == 0:
        raise ValueError("cm_eer: needs both bona fide and spoof trials")
    u = np.unique(s)
    t = np.concatenate([[u[0] - 1.0], u, (u[:-1] + u[1:]) / 2.0, [u[-1] + 1.0]])
    far = (spoof.size - np.searchsorted(spoof, t, side="left")) / spoof.size          # spoof >= t
    frr = np.searchsorted(bona, t, side="right") / bona.size                          # bona <= t
    key = np.lexsort((np.maximum(far, frr), np.abs(far - frr)))[0]
    return float((far[key] + frr[key]) / 2.0)


def score_line(idx, label, value):
    """main_spoof_conv1d.py:129."""
    return "LA_D_{} - {} {}\n".format(str(idx).zfill(7), "bonafide" if label == 1 else "spoof", str(value))


# ------------------------------------------------------------------------------------------------------ train / score
def _feat(batch, feat_type):
    return batch["data_0"] if feat_type == "mel" else batch["data_1"]


class _Bucket:
    """One width bucket's static buffers, its captured iteration and the device scalars it leaves."""

    def __init__(self, B, rows, width, device):
        self.x = torch.zeros((B, rows, width), dtype=torch.float32, device=device)
        self.y = torch.zeros((B,), dtype=torch.float32, device=device)
        self.live = torch.tensor([width, 1], dtype=torch.int32, device=device)
        self.live_upload = StagedUpload(self.live)
        self.loss = torch.zeros((1,), dtype=torch.float32, device=device)
        self.stepper = None

    def release(self):
        self.stepper.release()


class CmBucketedStep(BucketedReplay):
    """Training iterations (main_spoof_conv1d.py:84-90) on batches of a ``CmResidentCorpus``, replayed from one hipGraph per width bucket.
    A full batch whose width fits a bucket is gathered into the bucket's static buffer (zero-padded there by the gather), its width L and
    ``head_width(L)`` are written to two device ints, and the captured iteration -- zero_grad, ``model.loss(x, y, live)``, backward, Adam
    -- is replayed: ``_Disc.trunk(live=)`` and the ``_len`` head make it compute what the unpadded batch would.  One ``train.PhasedStep``
    per bucket, captured on the first batch that reaches it; its warm-up iterations are undone (``train.BucketedReplay``).  A batch wider
    than every bucket, a batch of another size than ``corpus.batch_size`` (the partial last one) and a batch whose head width would be 0
    run eagerly, as ``train`` runs them without buckets.  Gradients live in a ``gradarena.GradArena``: every bucket's graph and every
    eager step hand the optimizer the same addresses.  ``opt``: ``FusedAdamEx(capturable=True)``.  Dropout draws from the device
    Philox counter (``ops.act_dropout``), so every replay gets fresh masks.  Counters: ``replays``, ``eager``, ``captures``,
    ``capture_seconds``.  ``step`` returns the iteration's loss as a 1-element device tensor (valid until the bucket's next step)."""

    def __init__(self, model, opt, corpus, width_buckets):
        super().__init__(opt, "FusedAdamEx")
        self.model, self.opt, self.corpus = model, opt, corpus
        self.buckets = check_width_buckets(width_buckets)
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.arena = gradarena.GradArena([("all", [[p] for p in self.params])])

    def _release_arena(self):
        self.arena.release()

    def bucket_of(self, idx):
        """The bucket the batch of items ``idx`` replays in, or None when it runs eagerly."""
        L = self.corpus.width(idx)
        if len(idx) != self.corpus.batch_size or head_width(self.corpus.feat_type, L) < 1:
            return None
        return pick_width_bucket(self.buckets, L)

    def _iteration(self, x, y, live, loss_out=None):
        self.opt.zero_grad(set_to_none=True)
        loss, _ = self.model.loss(x, y, live)
        loss.backward()
        self.arena.adopt()
        self.opt.step()
        if loss_out is None:
            return loss.detach().reshape(1)
        loss_out.copy_(loss.detach().reshape(1))
        return loss_out

    def _set_live(self, st, L):
        host = st.live_upload.host()
        host[0], host[1] = int(L), head_width(self.corpus.feat_type, L)
        st.live_upload.send()

    def step(self, rows, row0, idx):
        """One iteration on the items ``idx`` = the host copy of ``rows[row0 : row0 + len(idx)]`` (``corpus.rows_of`` an order)."""
        bucket = self.last_bucket = self.bucket_of(idx)
        if bucket is None:
            self.eager += 1
            sp = self.corpus.gather(rows, row0, idx)
            return self._iteration(sp[self.corpus.key], sp["data_2"], None)
        st = self.steps.get(bucket) or _Bucket(self.corpus.batch_size, self.corpus.rows, bucket, self.corpus.device)
        self.corpus.gather_into(st.x, rows, row0, st.y)
        self._set_live(st, self.corpus.width(idx))
        if st.stepper is None:          # captured on this batch, in the static buffers just filled; registered once the capture has succeeded
            st.stepper = self._captured([self.model], [self.opt], lambda: PhasedStep(
                [("graph", lambda: self._iteration(st.x, st.y, st.live, st.loss))], graph=True).prepare())
            self.steps[bucket] = st
        st.stepper.run()
        self.replays += 1
        return st.loss


def train(cfg, source, feat_type="lin", save_dir="./checkpoints/cm", resume=None, save_interval=1000, max_epochs=20000, max_iterations=None,
          log=print, resident=False, width_buckets=None, log_interval=1):
    """main_spoof_conv1d.py:47-106 on the HIP path.  Checkpoints hold ``epoch``, ``global_iteration``, ``model_state_dict`` and
    ``optimizer_state_dict`` and are written to ``save_dir/<global_iteration + 1>_iteration.tar.pth`` when ``global_iteration %
    save_interval == 0`` and ``global_iteration > 0``; ``resume`` (a path) continues from the stored ``global_iteration`` and ``epoch``
    as the reference's ``-R`` does.  ``max_iterations`` (not in the reference) ends the run after that many iterations of THIS call.
    ``resident``: the source's features are extracted once into a ``CmResidentCorpus`` and every batch is gathered there (a
    ``CmResidentCorpus`` given as ``source`` is used as it is).  ``width_buckets`` (resident only): ascending widths in the feature's own
    frames; full batches that fit one are replayed from its hipGraph (``CmBucketedStep``), the others run eagerly.  Losses are kept on
    the device and read back every ``log_interval`` iterations; the log lines and the returned ``losses`` are the same.
    Returns dict(model, optimizer, epoch, global_iteration, losses, checkpoints, replays, eager, captures, capture_seconds)."""
    if resident and not isinstance(source, CmResidentCorpus):
        source = CmResidentCorpus(source, feat_type)
    is_resident = isinstance(source, CmResidentCorpus)
    if width_buckets is not None:
        if not is_resident:
            raise ValueError("width_buckets needs the resident corpus (resident=True or a CmResidentCorpus)")
        width_buckets = check_width_buckets(width_buckets)
    if is_resident and source.feat_type != feat_type:
        raise ValueError("the resident corpus holds %r features, feat_type is %r" % (source.feat_type, feat_type))
    log_interval = max(1, int(log_interval))
    model = build_model(cfg, feat_type)
    epoch = global_iteration = 0
    ckpt = None
    if resume is not None:
        ckpt = torch.load(resume, map_location="cpu")
        model.load_state_dict(ckpt["model_state_dict"])
    model.to(source.device)
    opt = FusedAdamEx([p for p in model.parameters() if p.requires_grad], capturable=width_buckets is not None, **ADAM)
    if ckpt is not None:
        opt.load_state_dict(ckpt["optimizer_state_dict"])
        epoch, global_iteration = int(ckpt["epoch"]), int(ckpt["global_iteration"])
    os.makedirs(save_dir, exist_ok=True)
    opt.refresh_resident_weights()
    model.train()
    stepper = CmBucketedStep(model, opt, source, width_buckets) if width_buckets is not None else None
    losses, saved, done = [], [], 0
    n_batches = source.n_batches()
    history = torch.zeros((log_interval,), dtype=torch.float32, device=source.device)
    pending = []                                   # per iteration not yet logged: (epoch, i, global_iteration, seconds)

    def flush():
        if pending:
            values = history[:len(pending)].cpu().tolist()              # one readback for the whole interval
            for value, (ep, i, gi, seconds) in zip(values, pending):
                losses.append(value)
                log("Epoch {}: Iteration{}/{}".format(str(ep + 1), str(i + 1), str(n_batches)))
                log("Loss: ", value)
                log("Global iteration: ", gi + 1)
                log("Time elapsed: {}\n".format(str(seconds)))
            del pending[:]

    def iterations(ep):
        """One closure per batch of the epoch, each running the iteration and returning its loss on the device."""
        if stepper is not None:
            order, rows = source.epoch(True, ep)
            for at in range(0, len(order), source.batch_size):
                yield lambda at=at: stepper.step(rows, at, order[at:at + source.batch_size])
            return
        for sp in source.batches(shuffle=True, epoch=ep):
            def run(sp=sp):
                opt.zero_grad()
                loss, _ = model.loss(_feat(sp, feat_type), sp["data_2"])
                loss.backward()
                opt.step()
                return loss.detach()
            yield run

    try:
        while epoch < max_epochs:
            log("Epoch ", epoch + 1)
            log("*******************")
            for i, run in enumerate(iterations(epoch)):
                if max_iterations is not None and done >= max_iterations:
                    break
                start_iter = _time.time()
                history[len(pending)].copy_(run().reshape(()))
                pending.append((epoch, i, global_iteration, None))
                if len(pending) == log_interval:
                    torch.cuda.synchronize(source.device)
                pending[-1] = pending[-1][:3] + (_time.time() - start_iter,)
                if len(pending) == log_interval:
                    flush()
                if global_iteration % save_interval == 0 and global_iteration > 0:
                    path = os.path.join(save_dir, "{}_iteration.tar.pth".format(str(global_iteration + 1)))
                    torch.save({"epoch": epoch + 1, "global_iteration": global_iteration, "model_state_dict": model.state_dict(),
                                "optimizer_state_dict": opt.state_dict()}, path)
                    saved.append(path)
                global_iteration += 1
                done += 1
            if max_iterations is not None and done >= max_iterations:
                break
            epoch += 1
        flush()
    finally:
        counters = dict(replays=0, eager=done, captures=0, capture_seconds=0.0)
        if stepper is not None:
            counters = stepper.stats()
            stepper.close()
    return dict(model=model, optimizer=opt, epoch=epoch, global_iteration=global_iteration, losses=losses, checkpoints=saved, **counters)


def load_model(cfg, checkpoint, feat_type, device):
    """The classifier of a checkpoint (a path, or the dict ``train`` saves) in eval mode on ``device``."""
    ckpt = torch.load(checkpoint, map_location="cpu") if isinstance(checkpoint, (str, os.PathLike)) else checkpoint
    model = build_model(cfg, feat_type)
    model.load_state_dict(ckpt["model_state_dict"])
    return model.to(device).eval()


def score(cfg, source, checkpoint, out_path, feat_type="lin", log=lambda *a: None):
    """main_spoof_conv1d.py:108-132: the checkpoint's model in eval mode over the source's batches in order; one line
    ``LA_D_%07d - bonafide|spoof <score>`` per item into ``out_path``.  Returns ``cm_eer`` of the written scores."""
    model = load_model(cfg, checkpoint, feat_type, source.device)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    scores, labels, idx = [], [], 0
    n_batches = source.n_batches()
    with open(out_path, "w") as f, torch.no_grad():
        for i, sp in enumerate(source.batches(shuffle=False)):
            log("Utterance: {}/{}".format(str(i + 1), n_batches))
            pred = model(_feat(sp, feat_type)).view(-1).cpu().numpy()
            label = sp["data_2"].cpu().numpy()
            for k in range(pred.shape[0]):
                value = float(pred[k])                                   # what .item() gives: the float32 score as a Python float
                f.write(score_line(idx, label[k], value))
                scores.append(value)
                labels.append(int(label[k] == 1))
                idx += 1
    return cm_eer(scores, labels)


def main(argv=None):
    """``python -m spoofsv_amd.countermeasure train|dev -T <time> -C <config> [-R <checkpoint>] [--feat lin|mel] [--ext .wav]``: the
    reference's front (main_spoof_conv1d.py:14-21) plus the feature kind, which the reference hard-wires."""
    ps = argparse.ArgumentParser(prog="python -m spoofsv_amd.countermeasure")
    ps.add_argument("step", choices=["train", "dev"], metavar="s")
    ps.add_argument("-T", "--time", type=str, required=True)
    ps.add_argument("-R", "--resume", type=str, default=None)
    ps.add_argument("-C", "--configuration", type=str, required=True)
    ps.add_argument("--feat", choices=["lin", "mel"], default="lin")
    ps.add_argument("--ext", type=str, default=".flac", help="extension of the spoof files (flac is not decoded: convert, then pass .wav)")
    ps.add_argument("--resident", action="store_true", help="extract the features once into a device-resident corpus and gather every batch there")
    ps.add_argument("--width-buckets", type=str, default=None, metavar="64,96,...",
                    help="with --resident: ascending widths (feature frames) whose full batches are replayed from captured graphs")
    args = ps.parse_args(argv)
    with open(args.configuration) as f:
        cfg = json.load(f)
    bona, spoof = protocol_items(cfg, args.step, args.time, args.ext)
    source = CmSource(cfg, bona, spoof)
    buckets = [int(v) for v in args.width_buckets.split(",")] if args.width_buckets else None
    if buckets is not None and not args.resident:
        ps.error("--width-buckets needs --resident")
    if args.step == "train":
        train(cfg, source, args.feat, save_dir="./checkpoints/" + args.time, resume=args.resume, resident=args.resident, width_buckets=buckets)
        return 0
    if args.resume is None:
        ps.error("dev needs -R <checkpoint>")
    if args.resident:
        source = CmResidentCorpus(source, args.feat)
    eer = score(cfg, source, args.resume, "./cm_scores/scores_{}.txt".format(args.time), args.feat, log=print)
    print("EER: {}".format(eer))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
