"""The Text2Mel / SSRN spectrogram corpus held on the device (config key CORPUS_RESIDENT): the ``.npy`` cache of data/dataset.py:85-91 is
read ONCE into ragged device arenas, and every batch is gathered there by ``ssv_corpus_gather`` / ``ssv_corpus_gather_ids`` in the layout
and zero padding of the collated batch (data/dataset.py:187-258).  Per batch the host does integer bookkeeping only: no file is opened,
nothing is padded, pinned or uploaded, nothing is read back.

  plan(...)                    what the corpus holds and how large it is, from the files' headers alone
  resident_corpus_bytes(...)   its device bytes; with a device: refuses a corpus that does not fit, before anything is allocated
  ResidentTtsCorpus            the arenas; ``rows(order)`` uploads an epoch's item order once, ``batch(row0, B)`` gathers a batch of it
  epoch_rows(batches)          an epoch's index batches -> one int32 table and the (row0, B) of every batch

``harness.CorpusSource`` owns the epoch order (the permutation, the per-rank slices, the wrap-around) and drives this module.
"""
import os

import numpy as np
import torch

from . import _lib, ops
from .ops import _p, _stream

_STAGE_BYTES = 64 << 20          # one pinned staging buffer (there are two): the files of a chunk cross in one copy


def _npy_header(path):
    """(shape, dtype) of the array in a ``.npy`` file, from its header alone."""
    fmt = np.lib.format
    try:
        with open(path, "rb") as f:
            major = fmt.read_magic(f)[0]
            shape, _, dtype = (fmt.read_array_header_1_0 if major == 1 else fmt.read_array_header_2_0)(f)
    except (OSError, ValueError) as e:
        raise ValueError("resident corpus: %s is not a readable .npy file (%s)" % (path, e))
    return tuple(int(s) for s in shape), dtype


def _offsets(sizes):
    sizes = np.asarray(sizes, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64) if len(sizes) else np.zeros((0,), np.int64)


class CorpusPlan:
    """What ``plan`` returns.  ``parts``: the arenas this step needs, of "mel", "lin", "text", "spk".  Per spectrogram arena ``rows[name]`` (F),
    ``len[name]`` (n int32: the items' widths), ``off[name]`` (n int64: the items' first elements, cumulative), ``elems[name]``.  Text:
    ``text_ids`` (the packed int32 ids of all items), ``len["text"]`` / ``off["text"]``.  Speakers: ``spk_files`` (the distinct code files, in order
    of first use), ``spk_index`` (n int32: item -> row of the table), ``spk_dim``.  ``bytes``: device bytes per arena, its two tables included."""

    def __init__(self):
        self.n, self.parts, self.files, self.rows, self.len, self.off, self.elems, self.bytes = 0, (), {}, {}, {}, {}, {}, {}
        self.text_ids, self.spk_files, self.spk_index, self.spk_dim = None, [], None, 0

    @property
    def total_bytes(self):
        return int(sum(self.bytes.values()))


def parts_of(step, mode):
    """The arenas a step reads: what ``CorpusSource._item`` loads for it (data/dataset.py:121-132)."""
    if step == "train_ssrn":
        return ("mel", "lin")
    if step == "synthesize" and mode != "validate":
        return ("mel", "text", "spk", "lin")
    return ("mel", "text", "spk")


def plan(cfg, wavlist, txtlist, cache, step, mode):
    """Lengths, offsets and bytes of the resident corpus of ``wavlist`` / ``txtlist`` for ``step``, without reading one spectrogram: the ``.npy``
    headers give the shapes (the transcripts, a line each, are read: their ids ARE the text arena).  Raises ``ValueError`` naming the file for a
    cache entry that is not a (FREQ_BINS, T) / (1 + FFT_LENGTH / 2, REDUCTION * T) floating-point array, or a speaker code of another size
    than the first.  An item of width 0 is legal (it is all padding in its batch)."""
    from .harness import text2id
    p = CorpusPlan()
    p.n, p.parts = len(wavlist), parts_of(step, mode)
    red = int(cfg["COARSE_MELSPEC"]["REDUCTION"])
    want = {"mel": int(cfg["COARSE_MELSPEC"]["FREQ_BINS"]), "lin": 1 + int(cfg["STFT"]["FFT_LENGTH"]) // 2}
    table_bytes = 12 * p.n                                           # per arena: int64 offsets and int32 lengths
    widths = {}
    for name in ("mel", "lin"):
        if name not in p.parts:
            continue
        p.files[name] = [cache + w[-17:-4] + "_%s.npy" % name for w in wavlist]
        w = np.zeros((p.n,), dtype=np.int64)
        for i, path in enumerate(p.files[name]):
            shape, dtype = _npy_header(path)
            if len(shape) != 2 or shape[0] != want[name] or dtype.kind != "f":
                raise ValueError("resident corpus: %s holds %s of shape %s; the %s cache entry must be a floating-point (%d, T) array"
                                 % (path, dtype, shape, name, want[name]))
            if name == "lin" and shape[1] != red * widths["mel"][i]:
                raise ValueError("resident corpus: %s is %d frames wide, %d x the %d of %s are %d (COARSE_MELSPEC.REDUCTION)"
                                 % (path, shape[1], red, widths["mel"][i], p.files["mel"][i], red * widths["mel"][i]))
            if shape[1] > 0x7fffffff // want[name]:
                raise ValueError("resident corpus: %s is %d frames wide: an item must stay below 2^31 elements" % (path, shape[1]))
            w[i] = shape[1]
        widths[name] = w
        p.rows[name], p.len[name], p.off[name] = want[name], w.astype(np.int32), _offsets(w * want[name])
        p.elems[name] = int(w.sum()) * want[name]
        p.bytes[name] = 4 * p.elems[name] + table_bytes
    if "text" in p.parts:
        ids = []
        for path in txtlist:
            with open(path) as f:
                ids.append(np.asarray(text2id(f.readline().strip(), cfg["VOCABULARY"]), dtype=np.int32))
        p.len["text"] = np.asarray([len(v) for v in ids], dtype=np.int32)
        p.off["text"] = _offsets(p.len["text"])
        p.text_ids = np.concatenate(ids).astype(np.int32) if ids else np.zeros((0,), np.int32)
        p.elems["text"] = int(p.text_ids.size)
        p.bytes["text"] = 4 * p.elems["text"] + table_bytes
    if "spk" in p.parts:
        seen = {}
        p.spk_index = np.zeros((p.n,), dtype=np.int32)
        for i, w in enumerate(wavlist):
            path = os.path.join(cfg["SPK_EMB_DIR"], w[-12:-8] + ".npy")
            if path not in seen:
                shape, dtype = _npy_header(path)
                size = int(np.prod(shape, dtype=np.int64))
                if dtype.kind not in "fiu" or size < 1 or (seen and size != p.spk_dim):
                    raise ValueError("resident corpus: %s holds %s of shape %s; every speaker code must be numeric with the %s elements of the first"
                                     % (path, dtype, shape, p.spk_dim or ">= 1"))
                p.spk_dim = size
                seen[path] = len(seen)
                p.spk_files.append(path)
            p.spk_index[i] = seen[path]
        p.elems["spk"] = len(p.spk_files) * p.spk_dim
        p.bytes["spk"] = 4 * p.elems["spk"] + table_bytes
    return p


def resident_corpus_bytes(p, device=None):
    """Device bytes of the corpus ``p`` (a ``CorpusPlan``) describes.  With ``device``: a ``RuntimeError`` naming this figure and the free
    device memory when the first exceeds the second -- before anything is allocated."""
    need = p.total_bytes
    if device is not None:
        ops.require_free_bytes(need, device, "CORPUS_RESIDENT: %d items (%s) need" % (p.n, ", ".join(p.parts)),
                               "train from the spectrogram cache instead (remove the key)")
    return need


def epoch_rows(batches):
    """An epoch's index batches (what ``CorpusSource`` slices from its permutation, wrap-around included) -> (table, spans): the batches
    back to back as ONE int32 array, and (row0, B) of each."""
    batches = [np.asarray(b, dtype=np.int64).reshape(-1) for b in batches]
    spans, at = [], 0
    for b in batches:
        spans.append((at, len(b)))
        at += len(b)
    return (np.concatenate(batches).astype(np.int32) if batches else np.zeros((0,), np.int32)), spans


class EpochRows:
    """One epoch's item order: ``host`` (int32 array) and, from its first batch on, ``dev`` -- uploaded once, by the thread that gathers."""

    def __init__(self, host):
        self.host, self.dev = np.ascontiguousarray(host, dtype=np.int32), None


class _Arena:
    def __init__(self, data, off, length, rows):
        self.data, self.off, self.len, self.rows = data, off, length, rows


class ResidentTtsCorpus:
    """The arenas of a ``CorpusPlan`` on ``device``.  Spectrograms are converted as the cache mode converts them (``torch.from_numpy(np.load(p))
    .float()``) into one of two pinned staging buffers and cross in chunks of ``stage_bytes``, not file by file; ids and speaker codes are
    one copy each.  ``nbytes`` = the plan's figure; ``load_seconds`` the time the load took."""

    def __init__(self, p, device, stage_bytes=_STAGE_BYTES):
        import time
        self.plan, self.device = p, torch.device(device)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("CORPUS_RESIDENT needs a ROCm device: the corpus is gathered by HIP kernels, there is no host fallback")
        self.nbytes = resident_corpus_bytes(p, self.device)
        t0 = time.time()
        self.arenas = {}
        dev = self.device
        tab = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        for name in ("mel", "lin"):
            if name in p.parts:
                data = torch.empty((max(1, p.elems[name]),), dtype=torch.float32, device=dev)
                self._load(data, p.files[name], p.off[name], p.len[name].astype(np.int64) * p.rows[name], stage_bytes)
                self.arenas[name] = _Arena(data, tab(p.off[name]), tab(p.len[name]), p.rows[name])
        if "text" in p.parts:
            ids = p.text_ids if p.text_ids.size else np.zeros((1,), np.int32)
            self.arenas["text"] = _Arena(tab(ids), tab(p.off["text"]), tab(p.len["text"]), 1)
        if "spk" in p.parts:
            codes = [torch.from_numpy(np.asarray(np.load(f), dtype=np.float32)).reshape(-1) for f in p.spk_files]       # as CorpusSource._item reads them
            table = torch.stack(codes, 0).to(dev) if codes else torch.zeros((1,), dtype=torch.float32, device=dev)
            self.arenas["spk"] = _Arena(table.reshape(-1), tab(p.spk_index.astype(np.int64) * p.spk_dim), tab(np.full((p.n,), p.spk_dim, np.int32)), 1)
        torch.cuda.synchronize(dev)
        self.load_seconds = time.time() - t0
        self._rows = None

    @staticmethod
    def _load(data, files, off, sizes, stage_bytes):
        """files[i] -> data[off[i] : off[i] + sizes[i]].  Consecutive items are consecutive in the arena, so a staging buffer holds a run of them
        and leaves in one copy; while it is in flight the other buffer fills."""
        cap = max(int(stage_bytes) // 4, int(sizes.max()) if len(sizes) else 1, 1)
        stages = [torch.empty((cap,), dtype=torch.float32).pin_memory() for _ in range(2)]
        done = [None, None]
        which, fill, start = 0, 0, 0

        def flush():
            nonlocal which, fill, start
            if fill:
                data[start:start + fill].copy_(stages[which][:fill], non_blocking=True)
                done[which] = torch.cuda.Event()
                done[which].record()
                which ^= 1
                if done[which] is not None:
                    done[which].synchronize()                    # the buffer about to be filled has left
            start, fill = start + fill, 0
        for path, o, n in zip(files, off, sizes):
            o, n = int(o), int(n)
            if fill + n > cap:
                flush()
            assert o == start + fill, "resident corpus: offsets are not cumulative"
            if n:
                stages[which][fill:fill + n].view(-1).copy_(torch.from_numpy(np.load(path)).float().reshape(-1))
            fill += n
        flush()
        torch.cuda.synchronize(data.device)

    def rows(self, order):
        """Upload nothing yet: wrap an epoch's order (``epoch_rows``) for ``batch``; the table goes to the device with its first batch."""
        self._rows = order if isinstance(order, EpochRows) else EpochRows(order)
        return self._rows

    def _gather(self, name, rows, row0, B, width, F=None, ids=False):
        a = self.arenas[name]
        F = a.rows if F is None else F
        out = torch.empty((B, F, width), dtype=torch.int64 if ids else torch.float32, device=self.device)
        if width == 0:
            return out
        if ids:
            _lib.call("ssv_corpus_gather_ids", _p(a.data), a.data.numel(), _p(a.off), _p(a.len), a.off.numel(), _p(rows.dev), rows.dev.numel(), row0,
                      _p(out), B, width, _stream())
        else:
            _lib.call("ssv_corpus_gather", _p(a.data), a.data.numel(), _p(a.off), _p(a.len), a.off.numel(), _p(rows.dev), rows.dev.numel(), row0,
                      _p(out), B, F, width, F * width, _stream())
        return out

    def batch(self, row0, B, rows=None):
        """The collated batch of items ``rows.host[row0 : row0 + B]`` (``rows``: an ``EpochRows``; default: the last one ``rows()`` made), on the
        device: the dict ``CorpusSource._collate`` builds, bit for bit.  Widths come from the host's length tables: no device read, no sync."""
        rows = self._rows if rows is None else rows
        if rows is None or row0 < 0 or B < 1 or row0 + B > len(rows.host):
            raise ValueError("ResidentTtsCorpus.batch: rows [%d, %d) are not in the epoch's table" % (row0, row0 + B))
        idx = rows.host[row0:row0 + B]
        if idx.min() < 0 or idx.max() >= self.plan.n:
            raise ValueError("ResidentTtsCorpus.batch: the epoch's table names an item outside [0, %d)" % self.plan.n)
        if rows.dev is None:
            rows.dev = torch.from_numpy(rows.host).to(self.device)
        p = self.plan
        width = lambda name: int(p.len[name][idx].max())
        out = {"data_0": self._gather("mel", rows, row0, B, width("mel"))}
        if p.parts == ("mel", "lin"):
            out["data_1"] = self._gather("lin", rows, row0, B, width("lin"))
            return out
        out["data_1"] = self._gather("text", rows, row0, B, width("text"), ids=True)
        out["data_2"] = self._gather("spk", rows, row0, B, p.spk_dim).view(B, p.spk_dim, 1)
        if "lin" in p.parts:
            out["data_3"] = self._gather("lin", rows, row0, B, width("lin"))
        return out
