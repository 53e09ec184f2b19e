"""The spoof countermeasure of the reference (``anti_spoofing/``): a conv1d classifier trained with binary cross-entropy to tell bona fide
from spoofed speech, on the HIP path from the waveform to the score.

What each piece replaces in the reference:
  CmLinDisc / CmMelDisc  anti_spoofing/discriminator.py:96-132 / :56-94 (the critics' stack with a sigmoid on top)
  CmSource               ASVspoofDataset.__getitem__ + collate_pad_3 + DataLoader, anti_spoofing/spoof_conv1d.py:43-91, main_spoof_conv1d.py:64
  protocol_items         ASVspoofDataset.__init__, anti_spoofing/spoof_conv1d.py:16-38
  train / score          anti_spoofing/main_spoof_conv1d.py:68-106 / :108-132
  cm_eer                 (the ASVspoof tools the reference leaves its score file to)

The classifier's trunk is ``critic._Disc`` -- convolutions, LayerNorms, highway gate, pools and dropout on the HIP kernels -- and its head
(leaky-ReLU, conv5, global average pool, sigmoid, and in training the loss) is ONE fused operator, ``ops.cm_head``.  The optimizer is
``train.FusedAdamEx`` (Adam with weight decay and AMSGrad, one launch).  Features come from ``CorpusFeatureExtractor`` at 16 kHz with
the 22 dB trim of the reference; synthesized speech enters as device waveforms at the synthesizer's rate and is resampled on the device,
so nothing leaves the GPU between synthesis and score.  Training is eager: batch widths vary from batch to batch.

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

from . import ops
from .critic import _Disc
from .train import FusedAdamEx

CM_RATE = 16000                 # spoof_conv1d.py:45,48
# main_spoof_conv1d.py:52 (lr is torch's default)
ADAM = dict(lr=1e-3, betas=(0.9, 0.98), eps=1e-9, weight_decay=1e-4, amsgrad=True)
_SLOPE = 0.05


class _CmDisc(_Disc):
    def forward(self, x):
        """The reference's output: sigmoid scores (B, 1, 1)."""
        return ops.cm_head(self.trunk(x), self.conv5.weight, self.conv5.bias, None, _SLOPE).view(-1, 1, 1)

    def loss(self, x, labels):
        """(mean binary cross-entropy of main_spoof_conv1d.py:87, pred (B,)); differentiable once through the loss."""
        return ops.cm_head(self.trunk(x), self.conv5.weight, self.conv5.bias, labels, _SLOPE)


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


def train(cfg, source, feat_type="lin", save_dir="./checkpoints/cm", resume=None, save_interval=1000, max_epochs=20000, max_iterations=None,
          log=print):
    """main_spoof_conv1d.py:47-106 on the HIP path.  Checkpoints hold ``epoch``, ``global_iteration``, ``model_state_dict`` and
    ``optimizer_state_dict`` and are written to ``save_dir/<global_iteration + 1>_iteration.tar.pth`` when ``global_iteration %
    save_interval == 0`` and ``global_iteration > 0``; ``resume`` (a path) continues from the stored ``global_iteration`` and ``epoch``
    as the reference's ``-R`` does.  ``max_iterations`` (not in the reference) ends the run after that many iterations of THIS call.
    Returns dict(model, optimizer, epoch, global_iteration, losses, checkpoints)."""
    model = build_model(cfg, feat_type)
    epoch = global_iteration = 0
    ckpt = None
    if resume is not None:
        ckpt = torch.load(resume, map_location="cpu")
        model.load_state_dict(ckpt["model_state_dict"])
    model.to(source.device)
    opt = FusedAdamEx([p for p in model.parameters() if p.requires_grad], **ADAM)
    if ckpt is not None:
        opt.load_state_dict(ckpt["optimizer_state_dict"])
        epoch, global_iteration = int(ckpt["epoch"]), int(ckpt["global_iteration"])
    os.makedirs(save_dir, exist_ok=True)
    opt.refresh_resident_weights()
    model.train()
    losses, saved, done = [], [], 0
    n_batches = source.n_batches()
    while epoch < max_epochs:
        log("Epoch ", epoch + 1)
        log("*******************")
        for i, sp in enumerate(source.batches(shuffle=True, epoch=epoch)):
            if max_iterations is not None and done >= max_iterations:
                break
            start_iter = _time.time()
            opt.zero_grad()
            loss, _ = model.loss(_feat(sp, feat_type), sp["data_2"])
            loss.backward()
            opt.step()
            value = loss.item()
            losses.append(value)
            log("Epoch {}: Iteration{}/{}".format(str(epoch + 1), str(i + 1), str(n_batches)))
            log("Loss: ", value)
            log("Global iteration: ", global_iteration + 1)
            log("Time elapsed: {}\n".format(str(_time.time() - start_iter)))
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
    return dict(model=model, optimizer=opt, epoch=epoch, global_iteration=global_iteration, losses=losses, checkpoints=saved)


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
    args = ps.parse_args(argv)
    with open(args.configuration) as f:
        cfg = json.load(f)
    bona, spoof = protocol_items(cfg, args.step, args.time, args.ext)
    source = CmSource(cfg, bona, spoof)
    if args.step == "train":
        train(cfg, source, args.feat, save_dir="./checkpoints/" + args.time, resume=args.resume)
        return 0
    if args.resume is None:
        ps.error("dev needs -R <checkpoint>")
    eer = score(cfg, source, args.resume, "./cm_scores/scores_{}.txt".format(args.time), args.feat, log=print)
    print("EER: {}".format(eer))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
