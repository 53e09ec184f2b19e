"""Float64 restatement of GE2E/dvector_create.py around tests/_sv_frontend_ref.py, in numpy, for the tests only: windows, partitions,
the file split.  Nothing under ``spoofsv_amd/`` imports it, and it imports nothing from there."""
import numpy as np

import _sv_frontend_ref as R


def windows_of_segment(S, window=24, shift=12):
    """get_STFTs' inner loop (dvector_create.py:48-52) on one segment's log-mel spectrogram S (nmels, T): list of (window, nmels)
    frames-major windows (what :99's transpose hands the embedder)."""
    out = []
    for j in range(0, S.shape[1], shift):
        if j + window < S.shape[1]:
            out.append(S[:, j:j + window].T)
        else:
            break
    return out


def features(y, spans, window=24, shift=12, **kw):
    """All windows of one utterance: ``spans`` are the concatenated voiced segments as (start, end) samples of ``y``.  A segment
    shorter than n_fft / 2 + 1 samples cannot be reflect-padded and has no window either way; it is skipped.
    Returns (n_windows, window, nmels) float64."""
    wins = []
    for s, e in spans:
        seg = np.asarray(y[s:e], dtype=np.float64)
        if len(seg) <= kw.get("nfft", 512) // 2:
            continue
        S, _ = R.log_mel(seg, **kw)
        wins += windows_of_segment(S, window, shift)
    nm = kw.get("nmels", 40)
    return np.stack(wins) if wins else np.zeros((0, window, nm))


def partitions(n):
    """align_embeddings' partition loop (dvector_create.py:55-69), literally."""
    parts = []
    start = 0
    end = 0
    j = 1
    for i in range(n):
        if (i * .12) + .24 < j * .401:
            end = end + 1
        else:
            parts.append((start, end))
            start = end
            end = end + 1
            j += 1
    else:
        parts.append((start, end))
    return parts


def align(emb):
    """align_embeddings (:55-73) on (n, D) window embeddings, float64."""
    emb = np.asarray(emb, dtype=np.float64)
    return np.stack([np.average(emb[a:b], axis=0) for a, b in partitions(len(emb))])


def split(rows_per_file_by_folder):
    """The bookkeeping of dvector_create.py:77-122 on row COUNTS: ``rows_per_file_by_folder[i]`` lists the rows of folder i's files.
    Returns (train ids, test ids) as lists of label strings, one per row."""
    total = len(rows_per_file_by_folder)
    train_speaker_num = (total // 10) * 9
    ids, train, saved = [], None, False
    label = 0
    for i, files in enumerate(rows_per_file_by_folder):
        for rows in files:
            ids += [str(label)] * rows
        label += 1
        if not saved and i > train_speaker_num:
            train, ids, saved = ids, [], True
    return train, ids


def concat_segs(times, segs):
    """concat_segs (dvector_create.py:24-36): runs of chunks whose times touch (exact float equality) are joined."""
    out = []
    cur = segs[0]
    for i in range(len(times) - 1):
        if times[i][1] == times[i + 1][0]:
            cur = np.concatenate((cur, segs[i + 1]))
        else:
            out.append(cur)
            cur = segs[i + 1]
    out.append(cur)
    return out


def rows_of_file(times, n, sr=16000, hop=160, window=24, shift=12):
    """Rows dvector_create.py:92-101 makes of a file of ``n`` samples whose VAD chunks are ``times``: only counts are followed."""
    tags = np.arange(n)
    segs = concat_segs(times, [tags[int(a * sr):int(b * sr)] for a, b in times])
    nw = 0
    for seg in segs:
        F = 1 + len(seg) // hop
        for j in range(0, F, shift):
            if j + window < F:
                nw += 1
            else:
                break
    return len(partitions(nw)) if nw else 0
