"""The host collate of the reference (data/dataset.py:187-258: zero padding to a common width, then ``torch.stack``) and the loader's
epoch order, restated in numpy for the tests of the resident spectrogram corpus.  Nothing here is shared with the code under test."""
import numpy as np


def gather_ref(arena, off, length, rows, row0, B, F, width):
    """out (B, F, width) float32: item r = rows[row0 + b] is the row-major (F, length[r]) block at arena[off[r]:], clipped to ``width`` and
    zero-padded up to it."""
    out = np.zeros((B, F, width), dtype=np.float32)
    for b in range(B):
        r = int(rows[row0 + b])
        n = int(length[r])
        item = np.asarray(arena[int(off[r]):int(off[r]) + F * n]).reshape(F, n)
        m = min(n, width)
        out[b, :, :m] = item[:, :m]
    return out


def ids_ref(arena, off, length, rows, row0, B, width):
    """out (B, 1, width) int64, 0 ('P') past the item's length."""
    out = np.zeros((B, 1, width), dtype=np.int64)
    for b in range(B):
        r = int(rows[row0 + b])
        m = min(int(length[r]), width)
        out[b, 0, :m] = arena[int(off[r]):int(off[r]) + m]
    return out


def epoch_indices(n, B, world, rank, seed, epoch, mode="train"):
    """The index batches of one epoch of ``DataLoader(shuffle=True, batch_size=B)`` as the harness shards it: a fresh permutation per epoch
    from RandomState(seed + epoch); one process keeps the partial last batch; with several ranks every rank takes B consecutive entries of each
    global batch of B * world, and the last global batch wraps around to the head of the order."""
    order = np.random.RandomState(seed + epoch).permutation(n) if mode == "train" else np.arange(n)
    per = B * world
    out = []
    for i in range((n + per - 1) // per):
        if world > 1:
            out.append([int(order[(i * per + rank * B + j) % n]) for j in range(B)])
        else:
            out.append([int(v) for v in order[i * per:(i + 1) * per]])
    return out
