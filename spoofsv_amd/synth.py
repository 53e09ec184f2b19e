"""Free-running Text2Mel synthesis as a hipGraph replay (reference loop: synthesize.py:103-109, ordinary.py:59-65).

The reference calls ``melSyn`` once per frame with the growing prefix; every call costs ~60 small kernel launches and the
loop is launch-bound (~1 ms per frame for any batch).  The audio encoder and decoder are strictly causal and LayerNorm is
per column, so running them on a FIXED (B, F, frames) buffer whose future columns are still zero gives exactly the same
values in the columns already synthesised.  One fixed-shape step

    Q = audio_encoder(mel_in)  ->  attention column `col` (mask, softmax, arg-max; frame index on the device)
      ->  R = V A, decoder  ->  mel_in[:, :, col + 1] = Y[:, :, col];  col += 1

is captured once per (batch, text length, frames) and replayed ``frames`` times; K, V come from one eager text-encoder
call.  Same kernels per column as ``melSyn.forward`` in eval mode; the only difference from the step-by-step loop is
that very short prefixes (B*T < 128) run on the exact-fp32 GEMM kernels there and on the split-bf16 ones here (1e-5).
Measured (tools/bench_synth.py): 0.92 -> 0.57 ms per frame at batch 1, 0.90 -> 0.65 at batch 8, no gain at batch 32 --
each step still computes all ``frames`` columns.  ``IncrementalSynthesizer`` below computes one column per step instead
(0.19 / 0.25 / 0.30 ms per frame at batch 1 / 8 / 32).

Three synthesizers, one lifecycle (``_Replayed``: what a ``run`` does and in which order, the one ``_capture``), and for the two
column-incremental ones one statement of what a step is (``column_schedule``), which each executes with its own launchers.
"""
import collections

import torch

from . import _lib, ops, resident

_p = ops._p


def _addresses(model):
    """Where the model's parameters live.  A captured step holds these addresses: a model that was moved (``.cpu()`` and back,
    ``load_state_dict(assign=True)``) needs a new capture, its old one would read freed memory."""
    return tuple(p.data_ptr() for p in model.parameters())


class _Replayed:
    """The lifecycle of a synthesizer whose step is captured once and replayed ``frames`` times.  A subclass allocates its buffers, lists
    in ``self._state`` those a reset zeroes, and supplies ``_step`` (one frame, on fixed buffers), ``_load`` (K | V and the speaker terms
    into them), ``_result`` and, where it keeps copies of the weights, ``_refresh``."""

    def __init__(self, model, batch, text_len, frames, device, n_texts=None):
        if model.training:
            raise RuntimeError("%s needs the model in eval mode" % type(self).__name__)
        self.model, self.B, self.N, self.T, self.dev = model, batch, text_len, frames, device
        self.n_texts = batch if n_texts is None else n_texts
        self.addresses = _addresses(model)
        self.graph = None

    def _refresh(self):
        """Bring the synthesizer's copies of the weights up to date; drop ``self.graph`` if the captured step no longer holds."""

    def _reset(self):
        for t in self._state:
            t.zero_()

    def _capture(self):
        """Warm step on a side stream (the allocator settles outside the capture), then the capture.  The warm step RUNS, at the
        frame index the state holds, and writes that frame of the output and the histories: ``run`` resets the state before every
        capture, or a capture after a completed run (frame index == frames) would write one frame past those buffers."""
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            self._step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph), torch.no_grad():
            self._step()

    @torch.no_grad()
    def run(self, text_id, spk_emb):
        want = (self.n_texts, 1, self.N)
        if tuple(text_id.shape) != want:
            raise RuntimeError("%s was built for text ids of shape %s, got %s" % (type(self).__name__, want, tuple(text_id.shape)))
        self._refresh()
        self._load(text_id, spk_emb)
        self._reset()
        if self.graph is None:
            self._capture()                      # (its warm step ran on frame 0 and advanced the state: start again)
            self._reset()
        for _ in range(self.T):
            self.graph.replay()
        return self._result()


class GraphSynthesizer(_Replayed):
    """``run(text_id, spk_emb) -> (Y, A)`` with Y (B, F, frames), A (B, N, frames) as the reference loop returns them."""

    def __init__(self, model, batch, text_len, frames, device):
        super().__init__(model, batch, text_len, frames, device)
        d, F = model.hidden_dim, model.audio_decoder.conv5.out_channels
        self.kv = torch.zeros((batch, 2 * d, text_len), device=device)
        self.spk = None
        self.mel_in = torch.zeros((batch, F, frames), device=device)
        self.A = torch.zeros((batch, text_len, frames), device=device)
        self.pma = torch.zeros((batch,), dtype=torch.int64, device=device)
        self.col = torch.zeros((1,), dtype=torch.int32, device=device)
        self.Y = None
        self._state = [self.mel_in, self.A, self.pma, self.col]

    def _step(self):
        m = self.model
        Q = m.audio_encoder(self.mel_in, self.spk)
        ops.attention_step_dev(self.kv, Q, self.pma, self.A, self.col)
        self.Y = m.audio_decoder(ops.attention_apply(self.kv, self.A, Q, self.T))
        ops.synth_advance(self.Y, self.mel_in, self.col)

    def _load(self, text_id, spk_emb):
        self.kv.copy_(self.model.text_encoder.encode(text_id))            # (B, 2d, N): K | V
        spk = spk_emb.to(self.dev).float()
        if self.spk is None:
            self.spk = spk.clone()
        else:
            self.spk.copy_(spk)

    def _result(self):
        return self.Y.clone(), self.A.clone()


# ------------------------------------------------------------------------------------------------ the column step, as data
Op = collections.namedtuple("Op", "kind mods src dst act spk hist", defaults=(0, None, None))


def column_schedule(model, who="column_schedule"):
    """One column-incremental step of ``melSyn`` as an ordered list of ``Op``: what ``audioEncoder.forward``, the attention and
    ``audioDecoder.forward`` (spoofsv_amd/tts.py) do to ONE new column, and which buffer every operation reads and writes.

    ``kind``  ``"link"`` (``mods`` = (conv, ln): act(LN(1x1 conv [+ speaker term ``spk`` = ``"s1"`` | ``"s2"``])), act 0 none, 1 relu,
              2 sigmoid), ``"highway"`` (``mods`` = (highwayConv,), ``hist`` = index of its input history), ``"attention"``, ``"advance"``.
    ``src``, ``dst``  buffer names.  The column starts in ``mel_cur`` and ping-pongs between ``a`` and ``b`` (an operation writes ``a``
              unless it reads ``a``); the attention writes [R ; Q] to ``rq``, the last link the new frame to ``y_cur``, and the advance
              feeds it back to ``mel_cur``.
    Needs no device and no library.  Every highway layer must be causal with kernel 3 on ``hidden_dim`` channels: the step reads
    frames t - dilation, t - 2 dilation from the layer's input history."""
    enc, dec, d = model.audio_encoder, model.audio_decoder, model.hidden_dim
    sched, src = [], "mel_cur"

    def then(kind, mods=(), dst=None, **kw):
        nonlocal src
        dst = dst or ("b" if src == "a" else "a")
        sched.append(Op(kind, mods, src, dst, **kw))
        src = dst

    def highways(*layers):
        for hc in layers:
            if not (hc.causal and hc.kernel_size == 3 and hc.dimension == d and hc.dilation >= 1):
                raise RuntimeError("%s: unexpected highwayConv configuration" % who)
            then("highway", (hc,), hist=sum(op.kind == "highway" for op in sched))

    then("link", (enc.conv1, enc.ln1), act=1, spk="s1" if enc.condition else None)       # fc1(spk), fc2(spk): models/TTSModel.py:174,179
    then("link", (enc.conv2, enc.ln2), act=1)
    then("link", (enc.conv3, enc.ln3), spk="s2" if enc.condition else None)
    highways(*enc.hci1.children(), *enc.hci2.children(), enc.hc1, enc.hc2)
    then("attention", dst="rq")
    then("link", (dec.conv1, dec.ln1))
    highways(*dec.hci.children(), dec.hc1, dec.hc2)
    then("link", (dec.conv2, dec.ln2), act=1)
    then("link", (dec.conv3, dec.ln3), act=1)
    then("link", (dec.conv4, dec.ln4), act=1)
    then("link", (dec.conv5, dec.ln5), dst="y_cur", act=2)
    then("advance", dst="mel_cur")
    return sched


class _ColumnSynthesizer(_Replayed):
    """A synthesizer that computes one NEW column per step: walks ``column_schedule`` with the launchers of its subclass
    (``_link``, ``_highway``, ``_attention``, ``_advance``) on the buffers the schedule names."""

    def __init__(self, model, batch, text_len, frames, device, n_texts=None):
        super().__init__(model, batch, text_len, frames, device, n_texts)
        self.d, self.F = model.hidden_dim, model.audio_decoder.conv5.out_channels
        self.schedule = column_schedule(model, type(self).__name__)

    def _step(self):
        buf = lambda name: getattr(self, name)
        for op in self.schedule:
            if op.kind == "link":
                self._link(*op.mods, buf(op.src), buf(op.dst), op.act, None if op.spk is None else buf(op.spk))
            elif op.kind == "highway":
                self._highway(*op.mods, self.hist[op.hist], buf(op.src), buf(op.dst))
            elif op.kind == "attention":
                self._attention(buf(op.src), buf(op.dst))
            else:
                self._advance(buf(op.src), buf(op.dst))

    def _load(self, text_id, spk_emb):
        enc = self.model.audio_encoder
        self.kv.copy_(self.model.text_encoder.encode(text_id))
        if enc.condition:
            spk = spk_emb.to(self.dev).float()
            if spk.shape[0] != self.B:
                raise RuntimeError("%s was built for %d items, got %d speaker codes" % (type(self).__name__, self.B, spk.shape[0]))
            for fc, s in ((enc.fc1, self.s1), (enc.fc2, self.s2)):
                self._items(s).copy_(ops.conv1d(spk, fc.weight.unsqueeze(-1), fc.bias).reshape(self.B, self.d))


class IncrementalSynthesizer(_ColumnSynthesizer):
    """The same loop with one NEW column per step instead of the whole prefix (include/ssv_hip.h, "Column-incremental
    synthesis").  The audio encoder and decoder are causal and LayerNorm acts per column, so the values of every layer at
    frames < t are final; step t computes column t only: 1x1 convs and causal k=3 convs as ``ssv_column_matvec`` (the k=3
    ones read frames t-d, t-2d from their (B, Tmax, C) input history), LayerNorm / highway gate on a length-1 sequence with
    the fused kernels of the full path, ``ssv_attention_column`` for the new attention frame.  ~55 launches per step, each a
    few microseconds, captured once per (batch, text length, frames) and replayed; work per step no longer grows with t.

    Values differ from the prefix loop only by fp32 summation order (plain fp32 dot products here, split-bf16 GEMMs there).
    """

    def __init__(self, model, batch, text_len, frames, device):
        super().__init__(model, batch, text_len, frames, device)
        B, d, F = batch, self.d, self.F
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)
        self.kv = z(B, 2 * d, text_len)
        self.mel_cur = z(B, F)
        self.Y = z(B, F, frames)
        self.A = z(B, text_len, frames)
        self.pma = torch.zeros((B,), dtype=torch.int64, device=device)
        self.t = torch.zeros((1,), dtype=torch.int32, device=device)
        self.s1, self.s2 = z(B, d), z(B, d)
        self.hist = [z(B, frames, d) for op in self.schedule if op.kind == "highway"]
        self.pre, self.a, self.b = z(B, 2 * d), z(B, d), z(B, d)              # gate pre-activations / two ping-pong columns
        self.pre1 = z(B, max(d, F))                                            # 1x1 conv outputs before their LayerNorm
        self.rq = z(B, 2 * d)
        self.y_cur = z(B, F)
        self._state = [self.mel_cur, self.pma, self.t, self.A, self.Y] + self.hist
        self._wt = {}

    def _items(self, s):
        return s                                     # a speaker term is (B, d), as computed

    def _result(self):
        return self.Y.clone(), self.A.clone()

    # ---- one-column operators on fixed buffers -------------------------------------------------------------------
    def _tap_major(self, conv):
        """(M, k, C) copy of a k = 3 conv weight in a buffer that lives as long as the synthesizer (the captured step holds its
        address); k = 1 weights are read in place.  ``_refresh`` rewrites the copies at the start of every ``run``."""
        w = conv.weight
        if w.shape[2] == 1:
            return w
        ent = self._wt.get(id(conv))
        if ent is None:
            ent = self._wt[id(conv)] = (torch.empty((w.shape[0], w.shape[2], w.shape[1]), dtype=torch.float32, device=w.device), conv)
            ent[0].copy_(w.detach().permute(0, 2, 1))
        return ent[0]

    def _refresh(self):
        """Bring the tap-major copies up to date with the live weights (one strided copy per k = 3 layer, 16 per run against
        ~50 launches per frame).  The synthesizer is cached per model and the validation pass of the trainers calls it on the
        model that is being trained; FusedAdam updates weights through raw pointers, so no version counter would tell."""
        for buf, conv in self._wt.values():
            buf.copy_(conv.weight.detach().permute(0, 2, 1))

    def _mv(self, conv, cur, out, hist=None, dilation=1, bias_b=None):
        M, C, k = conv.weight.shape
        _lib.call("ssv_column_matvec", _p(self._tap_major(conv)), _p(conv.bias), _p(bias_b), M, _p(cur), cur.stride(0),
                  _p(hist), 0 if hist is None else hist.stride(0), self.T, _p(self.t), dilation, _p(out), out.stride(0),
                  self.B, C, M, k, ops._stream())

    def _link(self, conv, ln, x, y, act, s):
        pre = self.pre1
        self._mv(conv, x, pre, bias_b=s)
        _lib.call("ssv_column_ln_act", _p(pre), pre.stride(0), _p(ln.weight), _p(ln.bias), _p(y), y.stride(0),
                  self.B, ln.weight.shape[0], act, ops._stream())

    def _highway(self, hc, hist, cur, out):
        self._mv(hc.conv, cur, self.pre, hist=hist, dilation=hc.dilation)
        _lib.call("ssv_column_gate", _p(self.pre), _p(cur), cur.stride(0), _p(hc.ln1.weight), _p(hc.ln1.bias),
                  _p(hc.ln2.weight), _p(hc.ln2.bias), _p(out), out.stride(0), self.B, self.d, ops._stream())

    def _attention(self, q, rq):
        _lib.call("ssv_attention_column", _p(self.kv), self.kv.stride(0), _p(q), _p(self.pma), _p(self.A), self.T,
                  _p(self.t), _p(rq), self.B, self.d, self.N, ops._stream())

    def _advance(self, y_cur, mel_cur):
        _lib.call("ssv_synth_column_advance", _p(y_cur), _p(self.Y), _p(mel_cur), _p(self.t), self.B, self.F, self.T, ops._stream())


# ------------------------------------------------------------------------------------------------ wide column-incremental synthesis
def _wide_tile():
    return int(_lib.lib().ssv_column_wide_tile())


def _wide_buffers(batch, text_len, frames, hidden, freq_bins, shared_texts=None, n_highway=16, tile=32):
    """(name, shape, bytes per element) of every device buffer a ``WideSynthesizer`` of this shape allocates."""
    B, N, T, d, F = batch, text_len, frames, hidden, freq_bins
    Bw = -(-B // tile) * tile
    U = B if shared_texts is None else shared_texts
    bufs = [("kv", (U, 2 * d, N), 4), ("mel_cur", (F, Bw), 4), ("Yw", (T, F, Bw), 4), ("A", (B, N, T), 4), ("pma", (B,), 8), ("t", (1,), 4),
            ("s1", (d, Bw), 4), ("s2", (d, Bw), 4), ("a", (d, Bw), 4), ("b", (d, Bw), 4), ("rq", (2 * d, Bw), 4), ("y_cur", (F, Bw), 4)]
    bufs += [("hist%d" % i, (T, d, Bw), 4) for i in range(n_highway)]
    return bufs


def wide_synth_bytes(batch, text_len, frames, hidden=256, freq_bins=80, shared_texts=None, n_highway=16, tile=32):
    """Device bytes a ``WideSynthesizer(model, batch, text_len, frames, ...)`` holds (its own buffers; the model and its resident weight
    planes are not counted).  Nearly all of it is the input history of the ``n_highway`` causal kernel-3 layers, kept whole:
    ``frames * hidden * Bw`` floats each with ``Bw`` = ``batch`` rounded up to the column tile (32)."""
    total = 0
    for _, shape, size in _wide_buffers(batch, text_len, frames, hidden, freq_bins, shared_texts, n_highway, tile):
        n = size
        for s in shape:
            n *= s
        total += n
    return total


class WideSynthesizer(_ColumnSynthesizer):
    """``IncrementalSynthesizer`` for LARGE batches: the same column-incremental step with every layer as ONE matrix product over the
    batch on the MFMA units (include/ssv_hip.h, "Wide column-incremental synthesis"; csrc/synth_wide.hip), 27 launches per frame.
    Step activations are (C, Bw) with the items contiguous.  The weights are read from the model's resident pre-split planes
    (``resident.ensure``), re-split at the start of every ``run``: no second copy, no tap-major repack.

    ``shared_texts=U``: ``text_id`` is (U, 1, N), ``spk_emb`` (B, spkemb_dim, 1) with ``B % U == 0`` and item ``b`` speaks text ``b % U`` --
    S speakers x U sentences need one text-encoder call and one K | V.  Same contract as ``IncrementalSynthesizer`` otherwise (eval mode,
    ``run(text_id, spk_emb) -> (Y (B, F, frames), A (B, N, frames))``).  In the split-fp16 mode an item's operand scale is that of its
    32-column tile, so its values depend on its neighbours to rounding (not at all in the fp32 mode)."""

    def __init__(self, model, batch, text_len, frames, device, shared_texts=None):
        super().__init__(model, batch, text_len, frames, device, shared_texts)
        self.U = U = shared_texts
        if U is not None and (U <= 0 or batch % U != 0):
            raise RuntimeError("WideSynthesizer: %d items do not divide into %r shared texts" % (batch, U))
        self.tile = _wide_tile()
        self.Bw = -(-batch // self.tile) * self.tile
        dims = (batch, text_len, frames, self.d, self.F, U, sum(op.kind == "highway" for op in self.schedule), self.tile)
        need = wide_synth_bytes(*dims)
        if torch.device(device).type == "cuda":
            ops.require_free_bytes(need, device, "WideSynthesizer(batch=%d, text_len=%d, frames=%d) needs" % (batch, text_len, frames),
                                   "run fewer items per batch")
        self.nbytes = need
        self.hist = []
        for name, shape, size in _wide_buffers(*dims):
            t = torch.zeros(shape, dtype=torch.int64 if size == 8 else (torch.int32 if name == "t" else torch.float32), device=device)
            if name.startswith("hist"):
                self.hist.append(t)
            else:
                setattr(self, name, t)
        self._state = [self.mel_cur, self.pma, self.t, self.A, self.Yw]
        self._key = None

    def _items(self, s):
        return s[:, :self.B].t()                     # a speaker term is (d, Bw): the items' columns, item-major

    def _result(self):
        return self.Yw[:, :, :self.B].permute(2, 1, 0).contiguous(), self.A.clone()

    def _weights(self):
        return [op.mods[0].weight if op.kind == "link" else op.mods[0].conv.weight for op in self.schedule if op.mods]

    def _refresh(self):
        # FusedAdam writes weights through raw pointers, so no version counter tells whether the planes are current: re-split them
        # (one launch per plane set and run, against 27 launches per frame)
        resident.invalidate(list(self.model.parameters()))
        resident.ensure(self.model, ops._stream())
        mode = _lib.precision()
        key = (mode,) + tuple(None if mode == 0 else resident.lookup(w).value for w in self._weights())
        if key != self._key:                     # the captured step holds the plane addresses and the arithmetic mode's kernels
            self.graph, self._key = None, key

    def _planes(self, w):
        if _lib.precision() == 0:
            return None
        pl = resident.lookup(w)
        if pl is None:
            raise RuntimeError("WideSynthesizer: a weight has no resident planes (resident.ensure did not cover it)")
        return pl

    def _link(self, conv, ln, x, y, act, s):
        Cout, Cin, _ = conv.weight.shape
        _lib.call("ssv_column_pwln_wide", _p(x), _p(conv.weight), self._planes(conv.weight), _p(conv.bias), _p(s),
                  _p(ln.weight), _p(ln.bias), _p(y), self.B, self.Bw, Cin, Cout, act, ops._stream())

    def _highway(self, hc, hist, cur, out):
        w = hc.conv.weight
        _lib.call("ssv_column_highway_wide", _p(w), self._planes(w), _p(hc.conv.bias), _p(hc.ln1.weight), _p(hc.ln1.bias),
                  _p(hc.ln2.weight), _p(hc.ln2.bias), _p(cur), _p(hist), self.T, _p(self.t), hc.dilation,
                  _p(out), self.B, self.Bw, self.d, 3, ops._stream())

    def _attention(self, q, rq):
        _lib.call("ssv_attention_column_wide", _p(self.kv), self.kv.stride(0), self.kv.shape[0], _p(q), _p(self.pma),
                  _p(self.A), self.T, _p(self.t), _p(rq), self.B, self.Bw, self.d, self.N, ops._stream())

    def _advance(self, y_cur, mel_cur):
        _lib.call("ssv_synth_column_advance_wide", _p(y_cur), _p(self.Yw), _p(mel_cur), _p(self.t), self.Bw, self.F, self.T, ops._stream())


# ------------------------------------------------------------------------------------------------ cached synthesizers
_CACHES = {GraphSynthesizer: {}, IncrementalSynthesizer: {}, WideSynthesizer: {}}      # small FIFO caches, one per kind: a synthesizer
_CACHE_MAX = 4                                                                         # owns frame-sized buffers and a captured graph


def _cached(cls, model, *shape):
    """The ``cls(model, *shape)`` built for this model object at these parameter addresses; at most ``_CACHE_MAX`` per kind, first in
    first out."""
    cache, key = _CACHES[cls], (id(model),) + shape
    g = cache.get(key)
    if g is None or g.model is not model or g.addresses != _addresses(model):      # an id() can be reused after the first model is gone
        cache.pop(key, None)
        while len(cache) >= _CACHE_MAX:
            cache.pop(next(iter(cache)))
        g = cache[key] = cls(model, *shape)
    return g


def free_run(model, text_id, spk_emb, frames):
    """Drop-in for the step-by-step loop: cached GraphSynthesizer per (model, batch, text length, frames)."""
    return _cached(GraphSynthesizer, model, text_id.shape[0], text_id.shape[2], frames, text_id.device).run(text_id, spk_emb)


def free_run_incremental(model, text_id, spk_emb, frames):
    """Drop-in for the step-by-step loop on the column-incremental path (cached per model / batch / text length / frames)."""
    return _cached(IncrementalSynthesizer, model, text_id.shape[0], text_id.shape[2], frames, text_id.device).run(text_id, spk_emb)


def free_run_wide(model, text_id, spk_emb, frames, shared_texts=None):
    """Drop-in for ``free_run_incremental`` on the wide step (cached per model / batch / text length / frames / shared texts).  With
    ``shared_texts=U``: ``text_id`` (U, 1, N), ``spk_emb`` (B, spkemb_dim, 1), item ``b`` speaks text ``b % U``."""
    B = text_id.shape[0] if shared_texts is None else spk_emb.shape[0]
    return _cached(WideSynthesizer, model, B, text_id.shape[2], frames, text_id.device, shared_texts).run(text_id, spk_emb)
