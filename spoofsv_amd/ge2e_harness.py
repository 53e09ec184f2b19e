"""Host-side mirror of the reference's GE2E speaker-verification scripts around the HIP embedder:
``GE2E/data_load.py`` (preprocessed TI-SV data), ``GE2E/train_speech_embedder.py`` (``train``, ``test``,
``test_nospoof``: EER and spoof rate).  The embedder and the loss run in libssv_hip.so (``spoofsv_amd.ge2e``); data
loading, the enrollment/verification bookkeeping and the threshold sweep are host logic, kept as the reference has them.
``preprocess_tisv`` is ``GE2E/data_preprocess.py`` with its librosa pass on the device (``spoofsv_amd.sv_frontend``),
``preprocess_tisv_synthetic`` the same for ``GE2E/synthetic_data_preprocess.py`` (voiced intervals instead of one trimmed span), and
``spoof_evaluation`` the in-memory form of ``test`` for features that never touched a disk.  ``ResidentSpeakerCorpus`` holds the
training corpus on the device and draws the loader's batches as row tables (``train`` with ``cfg["train"]["resident"]``); with
``cfg["test"]["resident"]`` the tests run on a resident test corpus too, scores and sweep in libssv_hip.so (``ge2e.SvEvalStep``), and ``evaluate``
is the three of them -- ``test``, ``test_nospoof``, ``spoof_rate_at`` -- in one pass.  ``spoof_curve``, ``ivector_curve``, ``ivector_spoofrate`` and
``curve`` are the arithmetic of ``curve.py`` and ``kaldi_ivectors/ivector_spoofrate.py`` (spoof rate against the FRR of real speech), counted on the device.

Configuration is a plain dict with the fields of ``GE2E/config/config.yaml`` (``default_config()``), instead of the
reference's module-global ``hparam`` object.
"""
import os
import random
import time

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from .ge2e import (GE2ELoss, GE2ETrainStep, SpeechEmbedder, SvEvalStep, score_list_curve, sv_accept_rate, sv_eer_sweep, sv_eval_shapes, sv_score_curve,
                   sv_trial_scores, tisv_batch_gather, train_iteration)
from .ops import require_free_bytes


def default_config():
    """GE2E/config/config.yaml as shipped."""
    return {
        "training": False, "device": "cuda", "save_simmat_dir": "./simmat",
        "data": {"train_path": "./train_tisv", "test_path": "./test_tisv", "sr": 16000, "nfft": 512, "window": 0.025,
                 "hop": 0.01, "nmels": 40, "tisv_frame": 120},
        "model": {"hidden": 768, "num_layer": 3, "proj": 256, "model_path": None},
        "train": {"N": 6, "M": 50, "num_workers": 0, "lr": 0.01, "epochs": 950, "log_interval": 5, "log_file": None,
                  "checkpoint_interval": 120, "checkpoint_dir": "./speech_id_checkpoint", "restore": False},
        "test": {"N": 20, "M": 86, "num_workers": 0, "epochs": 10},
    }


class SpeakerDatasetPreprocessed(Dataset):
    """SpeakerDatasetTIMITPreprocessed, GE2E/data_load.py:48-86: one ``.npy`` per speaker holding
    (utterances, n_mels, frames); an item is M utterances of one speaker as (M, frames, n_mels)."""

    def __init__(self, path, utter_num, shuffle=False, utter_start=0):
        self.path, self.utter_num, self.shuffle, self.utter_start = path, utter_num, shuffle, utter_start
        self.file_list = sorted(os.listdir(path))

    def __len__(self):
        return len(self.file_list)

    def __getitem__(self, idx):
        files = self.file_list
        selected = files[idx] if self.shuffle else random.sample(files, 1)[0]          # data_load.py:70-73
        utters = np.load(os.path.join(self.path, selected))
        if self.shuffle:
            utterance = utters[np.random.randint(0, utters.shape[0], self.utter_num)]
        else:
            utterance = utters[self.utter_start:self.utter_start + self.utter_num]
        return torch.tensor(np.transpose(utterance, axes=(0, 2, 1)))


def _npy_shape(path):
    """Shape of the array in a ``.npy`` file, from its header alone."""
    fmt = np.lib.format
    with open(path, "rb") as f:
        major = fmt.read_magic(f)[0]
        return tuple((fmt.read_array_header_1_0 if major == 1 else fmt.read_array_header_2_0)(f)[0])


class _SpeakerRows(Dataset):
    """The index-only twin of ``SpeakerDatasetPreprocessed(path, M, shuffle=True)``: item ``idx`` makes the ONE random call the host dataset
    makes (data_load.py:77) and returns the speaker's M global utterance rows.  No file is opened."""

    def __init__(self, offsets, counts, utter_num):
        self.offsets, self.counts, self.utter_num = offsets, counts, utter_num

    def __len__(self):
        return len(self.counts)

    def __getitem__(self, idx):
        return torch.from_numpy(self.offsets[idx] + np.random.randint(0, self.counts[idx], self.utter_num))


class _SpeakerTestRows(Dataset):
    """The index-only twin of ``SpeakerDatasetPreprocessed(path, M)`` (shuffle=False, the test loader): whatever ``idx`` is, the item makes
    the ONE random call the host dataset makes -- ``random.sample`` of one out of the speaker list (data_load.py:73) -- and returns that
    speaker's first M global utterance rows.  No file is opened."""

    def __init__(self, offsets, utter_num):
        self.offsets, self.utter_num = offsets, utter_num
        self.speakers = list(range(len(offsets)))

    def __len__(self):
        return len(self.speakers)

    def __getitem__(self, idx):
        return torch.from_numpy(self.offsets[random.sample(self.speakers, 1)[0]] + np.arange(self.utter_num, dtype=np.int64))


class _RowBatches:
    """One ``DataLoader`` over ``_SpeakerRows``; every ``iter()`` is an epoch of (N*M,) int32 row tables."""

    def __init__(self, loader):
        self.loader = loader

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for rows in self.loader:
            yield rows.reshape(-1).to(torch.int32)


class ResidentSpeakerCorpus:
    """The preprocessed TI-SV corpus of ``SpeakerDatasetPreprocessed`` (one ``.npy`` (utterances, nmels, frames) per speaker, read in
    ``sorted(os.listdir(path))`` order, the list the host dataset indexes) as ONE float32 tensor ``data`` (U_total, nmels, frames) on
    ``device``, every speaker's utterances contiguous from ``offsets[s]``, ``counts[s]`` of them.  Read once; the training loop then
    needs neither the disk nor the host's copies (data_load.py:75-85 per item of every batch).

    ``bytes`` (4 * U_total * nmels * frames) is known from the files' headers before anything is allocated; a corpus that does not fit
    the device's free memory raises a ``RuntimeError`` naming the figure.  A speaker file without utterances (the host loader crashes
    there, in ``randint(0, 0)``) or with another (nmels, frames) than the first raises a ``ValueError`` naming the file.
    ``device`` may be the CPU: the index logic (``batches``) needs no device; ``gather`` does."""

    def __init__(self, path, device):
        self.path, self.device = path, torch.device(device)
        self.file_list = sorted(os.listdir(path))
        if not self.file_list:
            raise ValueError("ResidentSpeakerCorpus: no speaker files under %s" % path)
        shapes = []
        for name in self.file_list:
            shape = _npy_shape(os.path.join(path, name))
            if len(shape) != 3 or shape[0] < 1:
                raise ValueError("ResidentSpeakerCorpus: %s holds no utterances (shape %s); every speaker file must be (utterances >= 1, nmels, frames)"
                                 % (os.path.join(path, name), tuple(shape)))
            if shapes and tuple(shape[1:]) != tuple(shapes[0][1:]):
                raise ValueError("ResidentSpeakerCorpus: %s holds (nmels, frames) = %s, the corpus %s" % (os.path.join(path, name), tuple(shape[1:]), tuple(shapes[0][1:])))
            shapes.append(shape)
        self.counts = np.array([s[0] for s in shapes], dtype=np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.counts)[:-1]]).astype(np.int64)
        self.nmels, self.frames = int(shapes[0][1]), int(shapes[0][2])
        self.total = int(self.counts.sum())
        self.bytes = 4 * self.total * self.nmels * self.frames
        if self.device.type == "cuda":
            require_free_bytes(self.bytes, self.device, "ResidentSpeakerCorpus(%s): %d utterances of (%d, %d) need" % (path, self.total, self.nmels, self.frames),
                               "train from the host loader instead")
        self.data = torch.empty((self.total, self.nmels, self.frames), dtype=torch.float32, device=self.device)
        for name, off, cnt in zip(self.file_list, self.offsets, self.counts):            # one speaker at a time: no second host copy of the corpus
            utters = np.ascontiguousarray(np.load(os.path.join(path, name)), dtype=np.float32)
            self.data[off:off + cnt].copy_(torch.from_numpy(utters))

    def __len__(self):
        return len(self.file_list)

    def batches(self, N, M):
        """The row tables of ``DataLoader(SpeakerDatasetPreprocessed(path, M, shuffle=True), batch_size=N, shuffle=True, drop_last=True)``,
        with exactly its random stream: a real ``DataLoader`` with the same arguments (``num_workers=0``) over ``_SpeakerRows``, so the same
        ``torch`` / ``numpy`` seeds select the same speakers and utterances.  Every ``iter()`` of the result is one epoch; an item is the
        batch's (N*M,) int32 table of global utterance rows, speaker after speaker."""
        return _RowBatches(DataLoader(_SpeakerRows(self.offsets, self.counts, M), batch_size=N, shuffle=True, num_workers=0, drop_last=True))

    def test_batches(self, N, M):
        """The row tables of ``DataLoader(SpeakerDatasetPreprocessed(path, M), batch_size=N, shuffle=True, drop_last=True)``, the loader of
        ``test`` / ``test_nospoof``, with exactly its random stream: a real ``DataLoader`` with the same arguments (``num_workers=0``) over
        ``_SpeakerTestRows``, so the same ``random`` / ``torch`` seeds select the same speakers.  The host dataset ignores the index it is given
        and draws the speaker itself, so a speaker may repeat within a batch; an item is the speaker's FIRST M utterances.  A speaker file
        with fewer than M utterances raises a ``ValueError`` naming it here (the host loader fails there, inside ``torch.stack``)."""
        short = [(n, c) for n, c in zip(self.file_list, self.counts) if c < M]
        if short:
            raise ValueError("ResidentSpeakerCorpus.test_batches: %s holds %d utterances, the test takes the first M = %d of every speaker"
                             % (os.path.join(self.path, short[0][0]), short[0][1], M))
        return _RowBatches(DataLoader(_SpeakerTestRows(self.offsets, M), batch_size=N, shuffle=True, num_workers=0, drop_last=True))

    def gather(self, rows_dev, out):
        """``out[b, t, f] = data[rows_dev[b], f, t]`` on the device (``ssv_tisv_batch_gather``)."""
        return tisv_batch_gather(self.data, rows_dev, out)


def _embedder(cfg, device):
    m = cfg["model"]
    return SpeechEmbedder(cfg["data"]["nmels"], m["hidden"], m["num_layer"], m["proj"]).to(device)


def _train_resident(cfg, model_path=None):
    """``train`` on a corpus held on the device: ``ResidentSpeakerCorpus`` draws the loader's batches as row tables, ``GE2ETrainStep`` runs
    the iteration (replayed unless cfg["train"]["graph"] is False).  The loss is not read back per iteration: the step keeps a history on
    the device, read at every ``log_interval`` and at the end of an epoch.  Same log lines, checkpoints and returned history as ``train``."""
    device = torch.device(cfg["device"])
    tr = cfg["train"]
    corpus = ResidentSpeakerCorpus(cfg["data"]["train_path"], device)
    batches = corpus.batches(tr["N"], tr["M"])
    net = _embedder(cfg, device)
    if tr["restore"]:
        net.load_state_dict(torch.load(model_path, map_location="cpu"))
    ge2e_loss = GE2ELoss(device)
    if tr["checkpoint_dir"]:
        os.makedirs(tr["checkpoint_dir"], exist_ok=True)
    net.train()
    step = GE2ETrainStep(net, ge2e_loss, tr["N"], tr["M"], corpus.frames, tr["lr"], graph=tr.get("graph", True), corpus=corpus,
                         hist_len=max(1, tr["log_interval"]))
    step.prepare()
    iteration, history = 0, []
    e = batch_id = 0
    for e in range(tr["epochs"]):
        total, pending = 0.0, 0

        def drain():
            nonlocal total, pending
            for v in step.losses(pending):
                history.append(v)
                total += v
            pending = 0
        for batch_id, rows in enumerate(batches):
            step.run(rows)
            pending += 1
            iteration += 1
            if (batch_id + 1) % tr["log_interval"] == 0:
                drain()
                mesg = "{0}\tEpoch:{1}[{2}/{3}],Iteration:{4}\tLoss:{5:.4f}\tTLoss:{6:.4f}\t\n".format(
                    time.ctime(), e + 1, batch_id + 1, len(corpus) // tr["N"], iteration, history[-1], total / (batch_id + 1))
                print(mesg)
                if tr["log_file"]:
                    with open(tr["log_file"], "a") as f:
                        f.write(mesg)
        drain()
        if tr["checkpoint_dir"] and (e + 1) % tr["checkpoint_interval"] == 0:
            torch.save({k: v.cpu() for k, v in net.state_dict().items()},
                       os.path.join(tr["checkpoint_dir"], "ckpt_epoch_%d_batch_id_%d.pth" % (e + 1, batch_id + 1)))
    if tr["checkpoint_dir"]:
        torch.save({k: v.cpu() for k, v in net.state_dict().items()},
                   os.path.join(tr["checkpoint_dir"], "final_epoch_%d_batch_id_%d.model" % (e + 1, batch_id + 1)))
    return net, history


def train(cfg, model_path=None):
    """train_speech_embedder.py:40-108.  Returns (embedder, list of per-iteration losses).  cfg["train"]["resident"] = True (absent by
    default) trains from a corpus held on the device instead of the host loader (``_train_resident``; cfg["train"]["graph"], default True
    there, selects replay)."""
    if cfg["train"].get("resident", False):
        return _train_resident(cfg, model_path)
    device = torch.device(cfg["device"])
    tr = cfg["train"]
    loader = DataLoader(SpeakerDatasetPreprocessed(cfg["data"]["train_path"], tr["M"], shuffle=True), batch_size=tr["N"], shuffle=True,
                        num_workers=tr["num_workers"], drop_last=True)
    net = _embedder(cfg, device)
    if tr["restore"]:
        net.load_state_dict(torch.load(model_path, map_location="cpu"))
    ge2e_loss = GE2ELoss(device)
    optimizer = torch.optim.SGD([{"params": net.parameters()}, {"params": ge2e_loss.parameters()}], lr=tr["lr"])
    if tr["checkpoint_dir"]:
        os.makedirs(tr["checkpoint_dir"], exist_ok=True)
    net.train()
    iteration, history = 0, []
    e = batch_id = 0
    for e in range(tr["epochs"]):
        total = 0.0
        for batch_id, mel_db_batch in enumerate(loader):
            loss = train_iteration(net, ge2e_loss, optimizer, mel_db_batch.to(device).float(), tr["N"], tr["M"])
            history.append(float(loss))
            total += history[-1]
            iteration += 1
            if (batch_id + 1) % tr["log_interval"] == 0:
                mesg = "{0}\tEpoch:{1}[{2}/{3}],Iteration:{4}\tLoss:{5:.4f}\tTLoss:{6:.4f}\t\n".format(
                    time.ctime(), e + 1, batch_id + 1, len(loader.dataset) // tr["N"], iteration, history[-1], total / (batch_id + 1))
                print(mesg)
                if tr["log_file"]:
                    with open(tr["log_file"], "a") as f:
                        f.write(mesg)
        if tr["checkpoint_dir"] and (e + 1) % tr["checkpoint_interval"] == 0:
            torch.save({k: v.cpu() for k, v in net.state_dict().items()},
                       os.path.join(tr["checkpoint_dir"], "ckpt_epoch_%d_batch_id_%d.pth" % (e + 1, batch_id + 1)))
    if tr["checkpoint_dir"]:
        torch.save({k: v.cpu() for k, v in net.state_dict().items()},
                   os.path.join(tr["checkpoint_dir"], "final_epoch_%d_batch_id_%d.model" % (e + 1, batch_id + 1)))
    return net, history


def cossim_eval(verification_embeddings, enrollment_centroids):
    """utils.get_cossim as the tests call it (train_speech_embedder.py:156-159): cosine of every verification embedding
    with every enrollment centroid, + 1e-6; the own-speaker column uses the mean of that speaker's OTHER verification
    embeddings (utils.py:42-43).  (N, V, D), (N, D) -> (N, V, N).  Vectorised; pinned against the reference by
    tests/golden/ge2e_train.npz through the oracle."""
    ver, cent = verification_embeddings, enrollment_centroids
    N, V, _ = ver.shape
    cos = torch.nn.functional.cosine_similarity(ver.unsqueeze(2), cent.view(1, 1, cent.shape[0], -1), dim=3)
    loo = (ver.sum(dim=1, keepdim=True) - ver) / (V - 1)
    own = torch.nn.functional.cosine_similarity(ver, loo, dim=2)
    idx = torch.arange(N, device=ver.device)
    cos = cos.clone()
    cos[idx, :, idx] = own
    return cos + 1e-6


def eer_sweep(sim_matrix, size_1, es1, spoof=True):
    """The threshold sweep of train_speech_embedder.py:168-191 (``test``) / :262-282 (``test_nospoof``): thresholds
    0.50 ... 0.99, first minimum of |FAR - FRR|.  Same counts as the reference's Python loops, computed in one shot."""
    N = sim_matrix.shape[0]
    thr = torch.tensor([0.01 * i + 0.5 for i in range(50)], device=sim_matrix.device, dtype=sim_matrix.dtype)
    th = (sim_matrix.unsqueeze(0) > thr.view(-1, 1, 1, 1)).double()                  # (50, N, V, N)
    idx = torch.arange(N, device=sim_matrix.device)
    own = th[:, idx, :, idx].permute(1, 0, 2)                                        # (50, N, V): own-speaker column
    tot, own_s = th.sum(dim=(1, 2, 3)), own.sum(dim=(1, 2))
    den = float(size_1 - es1) if spoof else float(size_1 / 2 - es1 / 2)
    pos = (size_1 - es1) if spoof else (size_1 // 2 - es1 // 2)
    FAR = (tot - own_s) / (N - 1.0) / den / N
    FRR = (N * pos - own_s) / den / N
    d = (FAR - FRR).abs()
    best, cur = 0, 1.0
    for i in range(50):                                                              # strict "<", as `if diff > abs(FAR-FRR)`
        if cur > float(d[i]):
            cur, best = float(d[i]), i
    out = dict(EER=float((FAR[best] + FRR[best]) / 2), thres=0.01 * best + 0.5, FAR=float(FAR[best]), FRR=float(FRR[best]))
    if spoof:
        half = (size_1 - es1) // 2
        hden = float(size_1 / 2 - es1 / 2)
        out["gt_FRR"] = float((N * (size_1 // 2 - es1 // 2) - own[best, :, :half].sum()) / hden / N)
        out["spoof_rate"] = float(own[best, :, -half:].sum() / hden / N)
    return out


def _verification_batches(cfg, net, enroll_num, device):
    te = cfg["test"]
    loader = DataLoader(SpeakerDatasetPreprocessed(cfg["data"]["test_path"], te["M"]), batch_size=te["N"], shuffle=True,
                        num_workers=te["num_workers"], drop_last=True)
    for e in range(te["epochs"]):
        for batch_id, mel_db_batch in enumerate(loader):
            assert te["M"] % 2 == 0
            size_1, es1 = mel_db_batch.shape[1], 2 * enroll_num
            enr = mel_db_batch[:, :es1].reshape(te["N"] * es1, mel_db_batch.size(2), mel_db_batch.size(3))
            ver = mel_db_batch[:, es1:].reshape(te["N"] * (size_1 - es1), mel_db_batch.size(2), mel_db_batch.size(3))
            e_enr = net(enr.to(device).float()).reshape(te["N"], es1, -1)
            e_ver = net(ver.to(device).float()).reshape(te["N"], size_1 - es1, -1)
            yield e, batch_id, size_1, es1, e_ver, e_enr.mean(dim=1)                  # get_centroids = speaker means


def _load(cfg, model_path, device):
    net = _embedder(cfg, device)
    net.load_state_dict(torch.load(model_path, map_location="cpu"))
    return net.eval()


def _resident_epochs(cfg, net, enroll_num, eval_num, device, per_epoch=None):
    """The batches of ``_verification_batches`` on a corpus held on the device: ``ResidentSpeakerCorpus.test_batches`` draws the loader's
    row tables, one ``SvEvalStep`` (replayed unless cfg["test"]["graph"] is False) embeds, scores and sweeps.  Nothing is read back per
    batch: with ``per_epoch(e, results, sims)`` the epoch's sweeps are read once at its end, without it nothing is read here at all.
    Returns (step, batches per epoch)."""
    te = cfg["test"]
    sv_eval_shapes(te["N"], te["M"], enroll_num, eval_num)
    corpus = ResidentSpeakerCorpus(cfg["data"]["test_path"], device)
    batches = corpus.test_batches(te["N"], te["M"])
    total = max(1, te["epochs"] * len(batches))
    step = SvEvalStep(net, corpus, te["N"], te["M"], enroll_num, eval_num, graph=te.get("graph", True), hist_len=total, stack_len=total).prepare()
    for e in range(te["epochs"]):
        nb = 0
        for rows in batches:
            step.run(rows)
            nb += 1
        if per_epoch is not None and nb:
            per_epoch(e, step.results(nb), step.sims(nb))
    return step, len(batches)


def _epoch_average(per_epoch, n):
    return sum(sum(v) / len(v) for v in per_epoch.values()) / n


@torch.no_grad()
def _test_resident(cfg, model_path, enroll_num):
    device = torch.device(cfg["device"])
    net = _load(cfg, model_path, device)
    save = cfg["test"].get("save_simmat", True)
    if save:
        os.makedirs(cfg["save_simmat_dir"], exist_ok=True)
    per_epoch_eer, per_epoch_spoof = {}, {}

    def per_epoch(e, results, sims):
        if save:
            host = sims.cpu()
        for b, r in enumerate(results):
            if save:
                torch.save(host[b].clone(), os.path.join(cfg["save_simmat_dir"], "simmat_e{}_b{}".format(e + 1, b + 1)))
            print("\nEER : %0.4f (thres:%0.4f)" % (r["EER"], r["thres"]))
            per_epoch_eer.setdefault(e, []).append(r["EER"])
            per_epoch_spoof.setdefault(e, []).append(r["spoof_rate"])
    step, _ = _resident_epochs(cfg, net, enroll_num, None, device, per_epoch)
    test.last_step = step
    n = cfg["test"]["epochs"]
    avg_eer, avg_spoof = _epoch_average(per_epoch_eer, n), _epoch_average(per_epoch_spoof, n)
    print("\n EER across {0} epochs: {1:.4f}".format(n, avg_eer))
    print("\n Spoof rate across {0} epochs: {1:.4f}".format(n, avg_spoof))
    return avg_eer, avg_spoof


@torch.no_grad()
def _test_nospoof_resident(cfg, model_path, enroll_num, eval_num):
    device = torch.device(cfg["device"])
    net = _load(cfg, model_path, device)
    per_epoch_thres = {}

    def per_epoch(e, results, sims):
        for r in results:
            r = r["nospoof"]
            print("\nEER : %0.4f (thres:%0.4f, FAR:%0.4f, FRR:%0.4f)" % (r["EER"], r["thres"], r["FAR"], r["FRR"]))
            per_epoch_thres.setdefault(e, []).append(r["thres"])
    _resident_epochs(cfg, net, enroll_num, eval_num, device, per_epoch)
    avg = _epoch_average(per_epoch_thres, cfg["test"]["epochs"])
    print("\n Average threshold: ", avg)
    return avg


@torch.no_grad()
def evaluate(cfg, model_path, enroll_num, eval_num, curve=False):
    """The whole ``__main__`` of train_speech_embedder.py:309-322 -- ``test``, ``test_nospoof``, then the spoof rate at the averaged
    no-spoof threshold -- in ONE pass over a corpus held on the device: every epoch's batches are drawn once, the mixture sweep and the
    no-spoof sweep run on the same embeddings (``SvEvalStep`` with ``eval_num``), and the spoof rate at the threshold comes from the
    mixture matrices the step holds (``sv_accept_rate``).  Two read-backs in all (the sweeps' history, the accept rates), no disk.
    Returns dict(EER, spoof_rate_at_eer, threshold, spoof_rate), each averaged as the three functions average.  ``curve=True`` adds
    ``"curve"``: the ``spoof_curve`` of the matrices the step holds (one more read-back: the curve's counts).

    NOT draw for draw the reference's two-pass sequence: there ``test_nospoof`` draws batches of its own after ``test`` has drawn its, so
    its threshold is measured on other speakers' draws than the matrices it is applied to.  Here both sweeps see the same batches; the
    figures are those of the same experiment, not the same random numbers."""
    device = torch.device(cfg["device"])
    net = _load(cfg, model_path, device)
    step, nb = _resident_epochs(cfg, net, enroll_num, eval_num, device)
    n = cfg["test"]["epochs"]
    results = step.results(step.batches)
    by_epoch = [results[e * nb:(e + 1) * nb] for e in range(n)] if nb else []

    def avg(get):
        return sum(sum(get(r) for r in ep) / len(ep) for ep in by_epoch) / n
    threshold = avg(lambda r: r["nospoof"]["thres"])
    evaluate.last_step = step
    out = dict(EER=avg(lambda r: r["EER"]), spoof_rate_at_eer=spoof_rate_at(cfg, threshold, eval_num, sims=step.sims()), threshold=threshold,
               spoof_rate=avg(lambda r: r["spoof_rate"]))
    if curve:
        out["curve"] = spoof_curve(cfg, eval_num, sims=step.sims())
    return out


@torch.no_grad()
def test(cfg, model_path, enroll_num):
    """train_speech_embedder.py:112-203: EER and spoof rate of the mixture test; the similarity matrices are saved for
    the later spoof-rate pass exactly as the reference saves them.  Returns (avg_EER, avg_spoof_rate).
    cfg["test"]["resident"] = True (absent by default) runs the test from a corpus held on the device (``SvEvalStep``; cfg["test"]["graph"],
    default True there, selects replay): same lines, printed at the end of each epoch, same return values; the matrices are written only
    when cfg["test"].get("save_simmat", True), and the step that holds them on the device (``sims()``) is left in ``test.last_step``."""
    if cfg["test"].get("resident", False):
        return _test_resident(cfg, model_path, enroll_num)
    device = torch.device(cfg["device"])
    net = _load(cfg, model_path, device)
    os.makedirs(cfg["save_simmat_dir"], exist_ok=True)
    per_epoch_eer, per_epoch_spoof = {}, {}
    for e, batch_id, size_1, es1, e_ver, cent in _verification_batches(cfg, net, enroll_num, device):
        sim = cossim_eval(e_ver, cent)
        torch.save(sim.cpu(), os.path.join(cfg["save_simmat_dir"], "simmat_e{}_b{}".format(e + 1, batch_id + 1)))
        r = eer_sweep(sim, size_1, es1, spoof=True)
        print("\nEER : %0.4f (thres:%0.4f)" % (r["EER"], r["thres"]))
        per_epoch_eer.setdefault(e, []).append(r["EER"])
        per_epoch_spoof.setdefault(e, []).append(r["spoof_rate"])
    n = cfg["test"]["epochs"]
    avg_eer = sum(sum(v) / len(v) for v in per_epoch_eer.values()) / n
    avg_spoof = sum(sum(v) / len(v) for v in per_epoch_spoof.values()) / n
    print("\n EER across {0} epochs: {1:.4f}".format(n, avg_eer))
    print("\n Spoof rate across {0} epochs: {1:.4f}".format(n, avg_spoof))
    return avg_eer, avg_spoof


@torch.no_grad()
def test_nospoof(cfg, model_path, enroll_num, eval_num):
    """train_speech_embedder.py:205-297: threshold at the EER of the genuine-only test.  Returns the average threshold.
    cfg["test"]["resident"] = True: from a corpus held on the device, as ``test``."""
    if cfg["test"].get("resident", False):
        return _test_nospoof_resident(cfg, model_path, enroll_num, eval_num)
    device = torch.device(cfg["device"])
    net = _load(cfg, model_path, device)
    per_epoch = {}
    for e, batch_id, size_1, es1, e_ver, cent in _verification_batches(cfg, net, enroll_num, device):
        sim = cossim_eval(e_ver[:, :2 * eval_num], cent)
        r = eer_sweep(sim, size_1, es1, spoof=False)
        print("\nEER : %0.4f (thres:%0.4f, FAR:%0.4f, FRR:%0.4f)" % (r["EER"], r["thres"], r["FAR"], r["FRR"]))
        per_epoch.setdefault(e, []).append(r["thres"])
    avg = sum(sum(v) / len(v) for v in per_epoch.values()) / cfg["test"]["epochs"]
    print("\n Average threshold: ", avg)
    return avg


def spoof_rate_at(cfg, thres, eval_num, sims=None):
    """train_speech_embedder.py:311-321: fraction of the last 2*eval_num verification trials of each speaker accepted at
    the no-spoof EER threshold, over the saved similarity matrices -- or, with ``sims``, over that device stack (nmat, N, V, N) of
    matrices (``SvEvalStep.sims()``; ``sv_accept_rate``), without the disk."""
    if sims is not None:
        rates = sv_accept_rate(sims, thres, eval_num)
        return sum(rates) / len(rates)
    N, rates = cfg["test"]["N"], []
    for k in sorted(os.listdir(cfg["save_simmat_dir"])):
        mat = torch.load(os.path.join(cfg["save_simmat_dir"], k)) > thres
        idx = torch.arange(N)
        rates.append(float(mat[idx, -2 * eval_num:, idx].float().sum() / float(2 * eval_num) / N))
    return sum(rates) / len(rates)


# --------------------------------------------------------------------------------------------- curve.py: spoof rate against real-speech FRR
def curve_thresholds(kind):
    """The two threshold lists of curve.py as Python floats: "ge2e" (:15, 5,000 over a similarity matrix), "ivector" (:31, 8,000 over a
    Kaldi score file)."""
    if kind == "ge2e":
        return [0.0001 * i + 0.5 for i in range(5000)]
    if kind == "ivector":
        return [-50 + 0.01 * i for i in range(8000)]
    raise ValueError("curve_thresholds: kind is 'ge2e' or 'ivector', got %r" % (kind,))


def ge2e_curve_rates(head_count, tail_count, N, rows):
    """curve.py:21-22 from the counts of accepted own-speaker trials in the first / last ``rows`` verification rows: the script sums float32
    tensors that hold integers (exact), divides twice in float32 and ``.item()`` widens the result --
    spoof_rate = float32(tail) / float32(rows) / float32(N), gt_frr = (float32(N * rows) - float32(head)) / float32(rows) / float32(N).
    Returns (spoof_rate, gt_frr) as float64 arrays of the counts' shape."""
    f = np.float32
    head, tail = np.asarray(head_count).astype(f), np.asarray(tail_count).astype(f)
    spoof = tail / f(rows) / f(N)
    frr = (f(N * rows) - head) / f(rows) / f(N)
    return spoof.astype(np.float64), frr.astype(np.float64)


def _load_simmat(simmat):
    if isinstance(simmat, (str, os.PathLike)):
        path = os.fspath(simmat)
        simmat = np.load(path) if path.endswith(".npy") else torch.load(path, map_location="cpu")
    return torch.as_tensor(simmat)


def spoof_curve(cfg, eval_num=20, sims=None, simmat=None, thresholds=None):
    """The GE2E half of curve.py (:15-25) -- per threshold the spoof rate (accepted own-speaker trials of the last 2*eval_num verification
    rows) and the FRR of real speech (rejected ones of the first 2*eval_num) -- over a device stack ``sims`` (nmat, N, V, N)
    (``SvEvalStep.sims()``) or over one saved matrix ``simmat`` as the script reads it (a ``torch.save``d tensor; also a .npy file or a
    tensor), of cfg["test"]["N"] speakers.  ``thresholds``: default ``curve_thresholds("ge2e")``.  The counting is one launch
    (``ge2e.sv_score_curve``) and one read-back, the counts.  Returns dict(thresholds, spoof_rate, gt_frr, counts, pooled): the two rates
    per matrix, (nmat, K) float64, bit for bit the script's logs (its float32 rounding sequence, ``ge2e_curve_rates``); counts (nmat, K, 4)
    int32 on the host; and ``pooled`` = dict(spoof_rate, gt_frr), (K,) float64: the same two rates from the counts SUMMED over the stack and
    divided in float64.  ``pooled`` is this project's, not the reference's, which draws one matrix."""
    if (sims is None) == (simmat is None):
        raise ValueError("spoof_curve: give either sims (a device stack) or simmat (one saved matrix)")
    thresholds = curve_thresholds("ge2e") if thresholds is None else [float(t) for t in thresholds]
    if sims is None:
        m = _load_simmat(simmat)
        if m.dim() != 3 or m.shape[0] != m.shape[2] or m.shape[0] != int(cfg["test"]["N"]):
            raise ValueError("spoof_curve: the matrix is %s, expected (N, V, N) with N = cfg['test']['N'] = %d" % (tuple(m.shape), int(cfg["test"]["N"])))
        sims = m.float().unsqueeze(0).to(torch.device(cfg["device"]))
    if sims.dim() != 4:
        raise ValueError("spoof_curve: sims is %s, expected a stack (nmat, N, V, N)" % (tuple(sims.shape),))
    nmat, N, V, rows = sims.shape[0], sims.shape[1], sims.shape[2], 2 * int(eval_num)
    if not 1 <= rows <= V:
        raise ValueError("spoof_curve: 2 * eval_num = %d must lie in [1, V = %d]" % (rows, V))
    counts = sv_score_curve(sims, thresholds, rows, rows).cpu().numpy()
    spoof, frr = ge2e_curve_rates(counts[:, :, 2], counts[:, :, 3], N, rows)
    total = float(nmat * N * rows)
    head, tail = counts[:, :, 2].astype(np.int64).sum(axis=0), counts[:, :, 3].astype(np.int64).sum(axis=0)
    pooled = dict(spoof_rate=tail.astype(np.float64) / total, gt_frr=(total - head.astype(np.float64)) / total)
    return dict(thresholds=thresholds, spoof_rate=spoof, gt_frr=frr, counts=counts, pooled=pooled)


def parse_ivector_scores(score_file, enroll_utt_num=3, eval_utt_num=20):
    """curve.py:32-41's reading of a Kaldi trial-score file (`<model speaker> <utterance> <score>` per line): a trial counts only when
    the utterance is the model speaker's own (info[0] == info[1][:3]); its utterance number (the name's last three characters) above
    enroll + eval makes it a spoofing trial, otherwise a real one.  Returns (real, fake) float64 arrays, in file order."""
    real, fake = [], []
    with open(score_file, "r") as f:
        for content in f.readlines():
            info = content.strip().split()
            if not info or info[0] != info[1][:3]:
                continue
            (fake if int(info[1][-3:]) > enroll_utt_num + eval_utt_num else real).append(float(info[-1]))
    return np.array(real, dtype=np.float64), np.array(fake, dtype=np.float64)


def _list_counts(device, groups, thresholds):
    """counts (K, len(groups)) on the host: per threshold the scores of each group above it, in float64 on the device."""
    scores = np.concatenate(groups)
    cls = np.concatenate([np.full(len(g), c, dtype=np.uint8) for c, g in enumerate(groups)])
    dev = torch.device(device)
    return score_list_curve(torch.from_numpy(scores).to(dev), torch.from_numpy(cls).to(dev), thresholds, len(groups)).cpu().numpy()


def ivector_curve(score_file, enroll_utt_num=3, eval_utt_num=20, thresholds=None, device="cuda"):
    """The i-vector half of curve.py (:27-49): the file parsed on the host (``parse_ivector_scores``), the 8,000 thresholds
    (``curve_thresholds("ivector")`` unless given) counted on the device in float64 (``ge2e.score_list_curve``), then
    spoof_rate = fake_count / L and gt_frr = 1 - real_count / L in float64, as the script computes them.  Unequal numbers of real and
    spoofing trials are a ``ValueError`` (the script asserts).  Returns dict(thresholds, spoof_rate, gt_frr, counts (K, 2): real, fake)."""
    real, fake = parse_ivector_scores(score_file, enroll_utt_num, eval_utt_num)
    if len(real) != len(fake) or len(real) == 0:
        raise ValueError("ivector_curve: %s holds %d real and %d spoofing own-speaker trials; curve.py:42 needs as many of one as of the other (and some)"
                         % (score_file, len(real), len(fake)))
    thresholds = curve_thresholds("ivector") if thresholds is None else [float(t) for t in thresholds]
    counts = _list_counts(device, [real, fake], thresholds)
    L = len(real)
    return dict(thresholds=thresholds, spoof_rate=counts[:, 1].astype(np.int64) / L, gt_frr=1 - counts[:, 0].astype(np.int64) / L, counts=counts)


def ivector_trials(enroll, enroll_utt2spk, evalv, eval_utt2spk, score_file, thresholds=None, enroll_utt_num=3, eval_utt_num=20, plda=None):
    """The trials of the i-vector system without Kaldi: ``enroll`` (n, R) and ``evalv`` (E, R) float32 device i-vectors with their
    '<utterance> <speaker>' lines (``ivector.split_enroll_eval`` order: a speaker's enrolment rows are consecutive), scored by cosine on the
    device (``ivector.cosine_trials``), written to ``score_file`` in ``trial_list`` order as '<speaker> <utterance> <score>', and swept by
    ``ivector_curve(score_file, thresholds=thresholds)``, whose dict is returned with ``scores`` (E, S) and ``speakers`` added.
    Without ``plda`` the ``thresholds`` are required: ``curve_thresholds("ivector")`` spans PLDA's range, cosine scores lie in [-1, 1].
    ``plda``: a ``plda.Plda`` model; the scores are then its log-likelihood ratios (``Plda.trials``), ``thresholds=None`` means
    ``curve_thresholds("ivector")``, and the dict gains ``eer`` and ``eer_threshold``: ``plda.compute_eer`` over the target / nontarget
    trials of ``ivector.trial_list``."""
    from . import ivector
    en, ev = ivector._utt2spk(enroll_utt2spk, "ivector_trials"), ivector._utt2spk(eval_utt2spk, "ivector_trials")
    if len(en) != enroll.shape[0] or len(ev) != evalv.shape[0]:
        raise ValueError("ivector_trials: %d enrolment lines for %d vectors, %d eval lines for %d vectors" % (len(en), enroll.shape[0], len(ev), evalv.shape[0]))
    speakers, off = [], [0]
    for i, (_, spk) in enumerate(en):
        if not speakers or spk != speakers[-1]:
            if spk in speakers:
                raise ValueError("ivector_trials: the enrolment rows of speaker %s are not consecutive" % spk)
            if speakers:
                off.append(i)
            speakers.append(spk)
    off.append(len(en))
    if plda is None and thresholds is None:
        raise TypeError("ivector_trials: thresholds are required for cosine scores (curve_thresholds('ivector') spans PLDA's range)")
    scores = ivector.cosine_trials(enroll, off, evalv) if plda is None else plda.trials(enroll, off, evalv)
    ivector.write_trial_scores(score_file, speakers, [utt for utt, _ in ev], scores)
    out = ivector_curve(score_file, enroll_utt_num, eval_utt_num, thresholds, device=enroll.device)
    out.update(scores=scores, speakers=speakers)
    if plda is not None:
        from .plda import compute_eer
        target = np.array([[spk == model for model in speakers] for _, spk in ev], dtype=bool)         # trial_list's labels, as a mask
        host = scores.cpu().numpy()
        out["eer"], out["eer_threshold"] = compute_eer(host[target], host[~target])
    return out


def ivector_eer(score_file, trial_lines):
    """The last line of kaldi_ivectors/ivector_eer.sh -- awk '{print $3}' scores | paste - trials | awk '{print $1, $4}' | compute-eer -- the
    third column of line i of the score file paired with the target / nontarget label of line i of ``trial_lines`` ('<utterance> <speaker>
    target|nontarget', ``ivector.trial_list``), then ``plda.compute_eer``.  Returns (eer, threshold)."""
    from .plda import compute_eer
    with open(score_file, "r") as f:
        scores = [line.split() for line in f if line.strip()]
    trials = [line.split() for line in trial_lines if line.strip()]
    if len(scores) != len(trials):
        raise ValueError("ivector_eer: %d score lines for %d trials" % (len(scores), len(trials)))
    groups = {"target": [], "nontarget": []}
    for sc, tr in zip(scores, trials):
        if len(sc) != 3 or len(tr) != 3 or tr[2] not in groups:
            raise ValueError("ivector_eer: %r / %r are not '<speaker> <utterance> <score>' and '<utterance> <speaker> target|nontarget'" % (" ".join(sc), " ".join(tr)))
        groups[tr[2]].append(float(sc[2]))
    return compute_eer(groups["target"], groups["nontarget"])


def ivector_spoofrate(score_file, thres, train_spk_num=88, enroll_utt_num=3, eval_utt_num=20, device="cuda"):
    """kaldi_ivectors/ivector_spoofrate.py whole: the spoofing own-speaker trials of a score file accepted at ``thres`` (score > thres in
    float64; counted by the list entry with one threshold), over total_num = (lines / 2) // (108 - train_spk_num), which must equal
    (108 - train_spk_num) * eval_utt_num (the script asserts; a ``ValueError`` here)."""
    with open(score_file, "r") as f:
        lines = f.readlines()
    total_num = (len(lines) / 2) // (108 - train_spk_num)
    if total_num != (108 - train_spk_num) * eval_utt_num:
        raise ValueError("ivector_spoofrate: %d lines give total_num = %s, expected (108 - %d) * %d = %d (ivector_spoofrate.py:16)"
                         % (len(lines), total_num, train_spk_num, eval_utt_num, (108 - train_spk_num) * eval_utt_num))
    spoof = []
    for line in lines:
        score = line.strip().split()
        if score[0] == score[1][:3] and int(score[1][-3:]) > enroll_utt_num + eval_utt_num:
            spoof.append(float(score[2]))
    if not spoof:
        return 0 / total_num
    counts = _list_counts(device, [np.array(spoof, dtype=np.float64)], [float(thres)])
    return int(counts[0, 0]) / total_num


def curve(cfg, simmat, ivector_score=None, out_dir=".", eval_num=20, plot=None):
    """curve.py: both sweeps, written to ``out_dir``/curve.npz under the script's four names (spoof_rate_log, gt_frr_log for the GE2E matrix;
    spoof_rate_log_2, gt_frr_log_2 for the i-vector score file, empty without one) with the two threshold lists (thresholds, thresholds_2).
    The figure ``out_dir``/curve.png is drawn only when matplotlib imports and ``plot`` is not False; nothing else needs matplotlib.
    Returns the dict that was saved."""
    ge = spoof_curve(cfg, eval_num, simmat=simmat)
    out = dict(spoof_rate_log=ge["spoof_rate"][0], gt_frr_log=ge["gt_frr"][0], thresholds=np.array(ge["thresholds"]),
               spoof_rate_log_2=np.zeros(0), gt_frr_log_2=np.zeros(0), thresholds_2=np.array(curve_thresholds("ivector")))
    if ivector_score is not None:
        iv = ivector_curve(ivector_score, device=cfg["device"])
        out.update(spoof_rate_log_2=iv["spoof_rate"], gt_frr_log_2=iv["gt_frr"])
    os.makedirs(out_dir, exist_ok=True)
    np.savez(os.path.join(out_dir, "curve.npz"), **out)
    if plot is not False:
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
        except ImportError:
            plt = None
        if plt is not None:
            fig = plt.figure()
            ax = fig.add_subplot(111)
            for tag, style, label in (("", "r--", "GE2E"), ("_2", "b", "i-vectors")):
                ax.plot(out["spoof_rate_log" + tag], out["gt_frr_log" + tag], style, linewidth=1, label=label)
            ax.set(xlabel="Spoof Rate", ylabel="FRR in real speech")
            ax.legend()
            fig.savefig(os.path.join(out_dir, "curve.png"))
            plt.close(fig)
    return out


def read_wav(path):
    """(rate, mono float32 waveform) of a PCM or float wav file, as ``harness.extract_features`` decodes them."""
    from scipy.io import wavfile
    sr, y = wavfile.read(path)
    if y.ndim > 1:
        y = y.mean(axis=1)                                       # librosa.load(mono=True)
    if y.dtype.kind in "iu":
        y = y.astype(np.float32) / float(1 << (8 * y.dtype.itemsize - 1))
    return int(sr), np.ascontiguousarray(y, dtype=np.float32)


def pad_batch(wavs, device):
    """List of 1-D float waveforms -> ((B, n_max) float32, (B,) int32 lengths) on ``device``."""
    n_max = max(1, max(len(w) for w in wavs))
    y = np.zeros((len(wavs), n_max), dtype=np.float32)
    for i, w in enumerate(wavs):
        y[i, :len(w)] = w
    return torch.from_numpy(y).to(device), torch.tensor([len(w) for w in wavs], dtype=torch.int32, device=device)


def _fill_slices(specs, want):
    """data_preprocess.py:69-74 / :76-81: a test speaker short of ``want`` utterances is filled with two random earlier slices per
    missing one (``np.random.randint`` below HALF the number of slices, in the reference's call order)."""
    have = len(specs)
    if 2 * want - have > 0:
        for _ in range(want - have // 2):
            loc1 = np.random.randint(0, have // 2)
            loc2 = np.random.randint(0, have // 2)
            specs.extend([specs[loc1], specs[loc2]])


def preprocess_tisv(cfg, speakers, train_spk_num, enroll_num, eval_num, front_end=None):
    """data_preprocess.save_spectrogram_tisv (:15-93) with the librosa pass on the device.  ``speakers``: ordered {name: [wav paths]}
    (the reference walks ``os.listdir`` order, which is not reproducible; the caller gives the order).  One device batch per speaker
    and sample rate.  Training speakers (the first ``train_spk_num``) keep their first 100 files in the caller's order; a test speaker's
    files are SORTED by base name without the extension, as :40 sorts them, and position k in that order decides the split: the first
    ``enroll_num`` files are enrolment, the rest evaluation, each side filled up by random duplication (``np.random``); "Too short!!" utterances are
    dropped.  Writes ``speaker<N>.npy`` as (slices, nmels, frames) under cfg["data"]["train_path"] / ["test_path"] and returns the
    list of written paths.  As at the reference's ``__main__`` (:102), pass ``enroll_num`` = enrolment + evaluation utterances there
    if the genuine evaluation utterances are to sit in the first block.
    ``front_end(wavs, orig_sr) -> ((B, 2, tisv_frame, nmels) array, (B,) bool)`` replaces the device pass (tests inject a CPU restatement)."""
    d = cfg["data"]
    os.makedirs(d["train_path"], exist_ok=True)
    os.makedirs(d["test_path"], exist_ok=True)
    if front_end is None:
        from .sv_frontend import TisvFrontEnd
        fe = TisvFrontEnd.from_config(cfg)

        def front_end(wavs, orig_sr):
            f, v = fe(*pad_batch(wavs, fe.device), orig_sr)
            return f.cpu().numpy(), v.cpu().numpy().astype(bool)
    written = []
    for i, (_, files) in enumerate(speakers.items()):
        test_spk = i >= train_spk_num
        # :37-40: a training speaker's first 100 files as listed; a test speaker's files sorted by name without the extension
        files = sorted(files, key=lambda f: os.path.basename(f)[:-4]) if test_spk else list(files)[:100]
        loaded = [(k, read_wav(f)) for k, f in enumerate(files) if f[-4:] == ".wav"]
        feats = {}
        for rate in sorted({sr for _, (sr, _) in loaded}):
            ks = [k for k, (sr, _) in loaded if sr == rate]
            f, v = front_end([w for _, (sr, w) in loaded if sr == rate], rate)
            for j, k in enumerate(ks):
                if v[j]:
                    feats[k] = f[j]
        utterances_spec, eval_spec = [], []
        for k in sorted(feats):
            dst = eval_spec if (test_spk and k >= enroll_num) else utterances_spec
            dst.extend([np.ascontiguousarray(feats[k][0].T), np.ascontiguousarray(feats[k][1].T)])      # (nmels, frames), first then last
        if test_spk:
            _fill_slices(utterances_spec, enroll_num)
            _fill_slices(eval_spec, eval_num)
            utterances_spec.extend(eval_spec)
        arr = np.array(utterances_spec)
        if test_spk and arr.shape[0] != 2 * (enroll_num + eval_num):
            raise RuntimeError("preprocess_tisv: speaker %d has %d slices, expected %d (data_preprocess.py:88)"
                               % (i, arr.shape[0], 2 * (enroll_num + eval_num)))
        path = os.path.join(d["test_path"], "speaker%d.npy" % (i - train_spk_num)) if test_spk else os.path.join(d["train_path"], "speaker%d.npy" % i)
        np.save(path, arr)
        written.append(path)
    return written


def _device_interval_slices(fe, max_intervals):
    """The device pass of ``preprocess_tisv_synthetic``: (y, lengths, rate, names) -> per utterance a (k, 2, tisv_frame, nmels) array.
    One ``split_call`` per ``capacity`` selected spans; what is read on the host per pass is ``total`` (one integer), then the pass's
    table and features, and the per-row interval counts once."""
    def run(y, n, rate, names):
        B = y.shape[0]
        capacity = 2 * B
        per_row = [[] for _ in range(B)]
        first = 0
        while True:
            feats, table, valid, total, count = fe.split_call(y, n, rate, max_intervals=max_intervals, capacity=capacity, first=first)
            total = int(total.item())
            if first == 0:
                for b, c in enumerate(count.cpu().tolist()):
                    if c > max_intervals:
                        raise RuntimeError("preprocess_tisv_synthetic: %s has %d voiced intervals, more than max_intervals=%d" % (names[b], c, max_intervals))
            here = min(capacity, total - first)
            if here > 0:
                f, t, v = feats[:here].cpu().numpy(), table[:here].cpu().numpy(), valid[:here].cpu().numpy()
                for r in range(here):
                    if v[r]:
                        per_row[int(t[r, 0])].append(f[r])
            first += capacity
            if first >= total:
                break
        T, nm = fe.tisv_frame, fe.nmels
        return [np.stack(p) if p else np.zeros((0, 2, T, nm), dtype=np.float32) for p in per_row]
    return run


def preprocess_tisv_synthetic(cfg, speakers, front_end=None, max_intervals=16):
    """synthetic_data_preprocess.save_spectrogram_tisv (:13-52) with its librosa pass on the device: no trim, but
    ``librosa.effects.split(utter, top_db=30)`` (:35), and of every voiced interval longer than ``utter_min_len`` (strict, :37) the first
    and last ``tisv_frame`` log-mel frames (:44-45).  ``speakers``: ordered {name: value}, a value being

    * a list of wav paths in the caller's order (the reference walks ``os.listdir``, which is not reproducible): every ``.wav`` is
      taken, there is no 100-file limit and no enrolment fill in this script; or
    * a device tuple ``(waveforms (U, n) float32, lengths (U,) int32, rate)`` as ``harness.generate_test_utterances(return_waveforms=
      True)`` returns per speaker (with the TTS sampling rate added), so that synthesized speech never touches the disk.

    One device pass per speaker and sample rate (more when a speaker has more than 2 x utterances selected intervals).  Slices are
    ordered by file, then interval, then first before last, each stored as (nmels, tisv_frame).  The first ``(len(speakers) // 10) * 8``
    speakers (:25) are written to ``train_path/speaker<i>.npy``, the others to ``test_path/speaker<i - train>.npy``.  A speaker without
    any slice is written as an empty ``(0, nmels, tisv_frame)`` float32 array; the reference writes ``np.array([])``, of shape (0,), there
    -- the one difference, so that the loader's ``utters.shape[0]`` and a later concatenation keep working.  A file with more than
    ``max_intervals`` voiced intervals raises a ``RuntimeError`` that names it and the count (raise ``max_intervals``); nothing is
    dropped silently.  Returns the list of written paths.
    ``front_end(wavs, orig_sr) -> list, per utterance, of (k, 2, tisv_frame, nmels) arrays`` replaces the device pass (tests inject a
    CPU restatement); an utterance for which it returns more than ``max_intervals`` intervals raises the same error."""
    d = cfg["data"]
    os.makedirs(d["train_path"], exist_ok=True)
    os.makedirs(d["test_path"], exist_ok=True)
    device_pass = None
    if front_end is None:
        from .sv_frontend import TisvFrontEnd
        fe = TisvFrontEnd.from_config(cfg)
        device_pass = _device_interval_slices(fe, int(max_intervals))
    train_spk_num = (len(speakers) // 10) * 8                                  # :25
    written = []
    for i, (name, value) in enumerate(speakers.items()):
        per_utt = {}                                                           # utterance index -> (k, 2, tisv_frame, nmels)
        if isinstance(value, tuple):
            if device_pass is None:
                raise ValueError("preprocess_tisv_synthetic: speaker %r is a device tuple; an injected front_end takes wav paths" % (name,))
            y, n, rate = value
            names = ["utterance %d of speaker %r" % (k, name) for k in range(y.shape[0])]
            per_utt = dict(enumerate(device_pass(y.contiguous(), n.contiguous(), int(rate), names)))
        else:
            loaded = [(k, f, read_wav(f)) for k, f in enumerate(value) if f[-4:] == ".wav"]      # :32
            for rate in sorted({sr for _, _, (sr, _) in loaded}):
                same = [(k, f, w) for k, f, (sr, w) in loaded if sr == rate]
                wavs, names = [w for _, _, w in same], [f for _, f, _ in same]
                if device_pass is not None:
                    out = device_pass(*pad_batch(wavs, fe.device), rate, names)
                else:
                    out = front_end(wavs, rate)
                    for f, a in zip(names, out):
                        if len(a) > max_intervals:
                            raise RuntimeError("preprocess_tisv_synthetic: %s has %d voiced intervals, more than max_intervals=%d" % (f, len(a), max_intervals))
                for (k, _, _), a in zip(same, out):
                    per_utt[k] = a
        utterances_spec = []
        for k in sorted(per_utt):
            for a in per_utt[k]:
                utterances_spec.extend([np.ascontiguousarray(a[0].T), np.ascontiguousarray(a[1].T)])        # :44-45, (nmels, frames)
        arr = np.array(utterances_spec, dtype=np.float32) if utterances_spec else np.zeros((0, d["nmels"], d["tisv_frame"]), dtype=np.float32)
        path = os.path.join(d["train_path"], "speaker%d.npy" % i) if i < train_spk_num else os.path.join(d["test_path"], "speaker%d.npy" % (i - train_spk_num))
        np.save(path, arr)
        written.append(path)
    return written


@torch.no_grad()
def spoof_evaluation(cfg, net, enrol, genuine, spoof, device_scoring=False):
    """The mixture test of ``test`` (train_speech_embedder.py:112-203) on features held in memory: ``enrol`` (N, ke, 2, frames, nmels),
    ``genuine`` (N, kg, ...) and ``spoof`` (N, ks, ...) straight from ``TisvFrontEnd`` (kg == ks, as the sweep's halves assume), the
    spoofing utterances never written to disk.  Per speaker the slices are laid out as ``speaker<N>.npy`` has them (enrolment, then
    genuine, then spoof), embedded, compared (``cossim_eval``) and swept (``eer_sweep(spoof=True)``).  Returns the sweep's dict plus
    the similarity matrix under "sim".  ``device_scoring=True`` compares and sweeps in libssv_hip.so instead (``sv_trial_scores``,
    ``sv_eer_sweep``): the same dict, one read-back."""
    N = enrol.shape[0]
    if not (genuine.shape[0] == N and spoof.shape[0] == N and genuine.shape[1] == spoof.shape[1]):
        raise ValueError("spoof_evaluation: need the same speakers on all three sides and as many genuine as spoofing utterances")
    fr, nm = enrol.shape[-2], enrol.shape[-1]
    es1 = 2 * enrol.shape[1]
    ver = torch.cat([genuine.reshape(N, -1, fr, nm), spoof.reshape(N, -1, fr, nm)], dim=1)
    size_1 = es1 + ver.shape[1]
    e_enr = net(enrol.reshape(N * es1, fr, nm).float().contiguous()).reshape(N, es1, -1)
    e_ver = net(ver.reshape(N * (size_1 - es1), fr, nm).float().contiguous()).reshape(N, size_1 - es1, -1)
    if device_scoring:
        sim = sv_trial_scores(e_enr, e_ver)
        out = sv_eer_sweep(sim, size_1, es1, spoof=True)
    else:
        sim = cossim_eval(e_ver, e_enr.mean(dim=1))
        out = eer_sweep(sim, size_1, es1, spoof=True)
    out["sim"] = sim
    return out


@torch.no_grad()
def dvector_create(cfg, speaker_folders, vad=None, out_dir=".", utterances_per_batch=64, read=read_wav, net=None):
    """GE2E/dvector_create.py:75-122 with everything after the VAD on the device (``spoofsv_amd.dvector``).  ``speaker_folders``: the
    speakers' folders in the order to walk them (the reference globs ``hp.unprocessed_data``); a folder's index is its label, its
    ``.wav`` files are taken in ``os.listdir`` order, sorted here so that a run can be repeated.  ``vad(path) -> times`` returns what
    ``VAD_chunk`` returns first (VAD_segments.py:130-150; webrtcvad itself is not part of this project); an empty list prints the
    reference's "No voice activity detected" and skips the file.  ``vad=None``: one span per file, its ``trim_bounds(..., 30)``.
    ``vad="split"``: a file's spans are its ``split_intervals(..., 30)`` intervals, computed on the device and read back once per batch;
    a file with no interval (an empty one) prints the same message.  That is an ENERGY detector (``librosa.effects.split``: frames
    within 30 dB of the file's loudest), not webrtcvad: it keeps loud noise, drops quiet speech, and its spans are not cut into 0.4 s
    chunks -- a device span source where no webrtcvad output is at hand, not a restatement of ``VAD_chunk``.
    Files are decoded by ``read`` (path -> (rate, waveform)), resampled on the device when their rate is not cfg["data"]["sr"], and
    embedded ``utterances_per_batch`` at a time, across files and speakers, in one device pass each.  The embedder is ``net`` or the
    checkpoint cfg["model"]["model_path"].

    Writes ``train_sequence.npy`` / ``train_cluster_id.npy`` / ``test_sequence.npy`` / ``test_cluster_id.npy`` under ``out_dir`` as the
    reference does: float64 rows (``align_embeddings`` fills an ``np.zeros`` array), string ids, the training files after the FIRST
    folder whose index i satisfies ``i > (total // 10) * 9`` (:78, :110 -- that folder included), the rest as test.  Where nothing is
    left for a file set the reference's ``np.concatenate([])`` raises; here an empty (0, proj) array and an empty id array are written.
    A file none of whose spans gives a window (the reference crashes there, in ``np.stack([])``) contributes no row.  Returns the four paths."""
    from .dvector import DvectorExtractor, spans_from_vad
    from .sv_frontend import TisvFrontEnd, split_intervals
    if isinstance(vad, str) and vad != "split":
        raise ValueError("dvector_create: vad must be None, a callable or 'split', got %r" % (vad,))
    d = cfg["data"]
    fe = TisvFrontEnd.from_config(cfg)
    if net is None:
        net = _load(cfg, cfg["model"]["model_path"], fe.device)
    ex = DvectorExtractor(fe, net)
    proj = net.dims[3]
    folders = list(speaker_folders)
    files = [(i, os.path.join(folder, f)) for i, folder in enumerate(folders) for f in sorted(os.listdir(folder)) if f[-4:] == ".wav"]
    rows_of = {}                                                 # file index -> (rows, proj) float64, absent: no voice activity
    for lo in range(0, len(files), max(1, int(utterances_per_batch))):
        chunk = list(range(lo, min(len(files), lo + max(1, int(utterances_per_batch)))))
        loaded = [read(files[k][1]) for k in chunk]
        waves = [None] * len(chunk)
        for rate in sorted({sr for sr, _ in loaded}):
            js = [j for j, (sr, _) in enumerate(loaded) if sr == rate]
            y, n = pad_batch([loaded[j][1] for j in js], fe.device)
            if rate != d["sr"]:
                y, n = fe.resample(y, n, rate)
            for j, m in zip(js, n.cpu().tolist()):
                waves[j] = (y, js.index(j), m)
        n_max = max(1, max(m for _, _, m in waves))
        y16 = torch.zeros((len(chunk), n_max), dtype=torch.float32, device=fe.device)
        for j, (y, r, m) in enumerate(waves):
            y16[j, :m] = y[r, :m]
        n16 = torch.tensor([m for _, _, m in waves], dtype=torch.int32, device=fe.device)
        spans, voiced = None, [True] * len(chunk)
        if vad == "split":
            K = 16
            while True:                                          # count is not capped: a second pass holds every interval
                iv, cnt = split_intervals(y16, n16, 30, K)
                iv, cnt = iv.cpu().tolist(), cnt.cpu().tolist()
                if max(cnt) <= K:
                    break
                K = max(cnt)
            spans = [[tuple(se) for se in iv[j][:cnt[j]]] for j in range(len(chunk))]
            voiced = [c > 0 for c in cnt]
        elif vad is not None:
            spans = []
            for j, k in enumerate(chunk):
                times = vad(files[k][1])
                voiced[j] = len(times) > 0
                spans.append(spans_from_vad(times, d["sr"], waves[j][2]))
        seq, rows = ex(y16, n16, spans)
        seq = seq.cpu().numpy().astype(np.float64)
        at = 0
        for j, k in enumerate(chunk):
            if voiced[j]:
                rows_of[k] = seq[at:at + rows[j]]
            at += rows[j]
    # the reference's loop (:84-122) over what the device made of every file
    train_speaker_num = (len(folders) // 10) * 9
    sequence, cluster_id, count, train_saved = [], [], 0, False
    paths = [os.path.join(out_dir, n + ".npy") for n in ("train_sequence", "train_cluster_id", "test_sequence", "test_cluster_id")]
    os.makedirs(out_dir, exist_ok=True)

    def save(seq_path, id_path):
        np.save(seq_path, np.concatenate(sequence, axis=0) if sequence else np.zeros((0, proj)))
        np.save(id_path, np.asarray(cluster_id, dtype=str))
    by_folder = {}
    for k, (i, _) in enumerate(files):
        by_folder.setdefault(i, []).append(k)
    for i in range(len(folders)):
        for k in by_folder.get(i, []):
            if k not in rows_of:
                print("No voice activity detected")
                continue
            sequence.append(rows_of[k])
            cluster_id.extend([str(i)] * rows_of[k].shape[0])
            count += 1
            if count % 100 == 0:
                print("Processed {0}/{1} files".format(count, len(folders)))
        if not train_saved and i > train_speaker_num:
            save(paths[0], paths[1])
            train_saved = True
            sequence, cluster_id = [], []
    save(paths[2], paths[3])
    return paths
