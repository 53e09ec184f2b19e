"""What the replayed steps share on the host, without a device: ``train.BucketedReplay`` (a capture is timed, counted and its training
undone bitwise; a failed capture counts nothing; ``stats()``; ``close()``), ``train.TrainingSnapshot`` as a context (restores on a clean
exit, not on an exception) and ``ops.require_free_bytes`` (exactly enough is enough; the refusal names both figures)."""
from types import SimpleNamespace

import pytest
import torch

from spoofsv_amd import ops, train


class _Replay(train.BucketedReplay):
    def __init__(self, log):
        super().__init__(SimpleNamespace(capturable=True), "FusedAdam")
        self.log = log

    def _release_arena(self):
        self.log.append("arena")


def _linear():
    torch.manual_seed(3)
    m = torch.nn.Linear(3, 2)
    return m, [p.detach().clone() for p in m.parameters()]


def _perturb(m):
    with torch.no_grad():
        for p in m.parameters():
            p.add_(1.0)


def _same(m, before):
    return all(torch.equal(p.detach(), w) for p, w in zip(m.parameters(), before))


def test_a_capture_is_counted_timed_and_its_training_undone():
    m, before = _linear()
    ptrs = [p.data_ptr() for p in m.parameters()]
    r = _Replay([])
    made = object()

    def make():
        _perturb(m)
        assert not _same(m, before)
        return made
    assert r._captured([m], [], make) is made
    assert _same(m, before) and [p.data_ptr() for p in m.parameters()] == ptrs          # bitwise, in the same tensors
    assert r.captures == 1 and r.capture_seconds > 0
    assert r.steps == {} and r.replays == 0 and r.eager == 0 and r.last_bucket is None  # registering and counting those is the subclass's


def test_a_capture_that_raises_counts_nothing():
    m, before = _linear()
    r = _Replay([])

    def make():
        _perturb(m)
        raise KeyError("no capture")
    with pytest.raises(KeyError, match="no capture"):
        r._captured([m], [], make)
    assert r.steps == {}
    assert r.stats() == dict(replays=0, eager=0, captures=0, capture_seconds=0.0)
    assert not _same(m, before)                                                          # nothing was restored either


def test_stats_close_and_the_capturable_refusal():
    log = []
    r = _Replay(log)
    assert sorted(r.stats()) == ["capture_seconds", "captures", "eager", "replays"]
    r.replays, r.eager = 5, 2
    assert r.stats() == dict(replays=5, eager=2, captures=0, capture_seconds=0.0)
    for b in (40, 64, 96):
        r.steps[b] = SimpleNamespace(release=lambda b=b: log.append(b))
    r.close()
    assert log == [40, 64, 96, "arena"] and r.steps == {}                                # every step once, then the arena hook
    with pytest.raises(ValueError, match=r"_Sub needs FusedAdamEx\(capturable=True\)"):
        type("_Sub", (train.BucketedReplay,), {})(SimpleNamespace(capturable=False), "FusedAdamEx")


def test_the_snapshot_context_restores_on_a_clean_exit_only():
    m, before = _linear()
    with train.TrainingSnapshot([m], []) as snap:
        _perturb(m)
    assert _same(m, before) and isinstance(snap, train.TrainingSnapshot)
    with pytest.raises(ZeroDivisionError):
        with train.TrainingSnapshot([m], []):
            _perturb(m)
            1 / 0
    assert all(torch.equal(p.detach(), w + 1.0) for p, w in zip(m.parameters(), before))


def test_require_free_bytes_at_the_boundary(monkeypatch):
    free = 5 * 2 ** 30 + 123
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda d=None: (free - 700, 1 << 40))
    monkeypatch.setattr(torch.cuda, "memory_reserved", lambda d=None: 1000)
    monkeypatch.setattr(torch.cuda, "memory_allocated", lambda d=None: 300)
    dev = torch.device("cuda", 0)
    assert ops.free_bytes(dev) == free
    ops.require_free_bytes(free, dev, "Thing(3) needs", "use less")                      # exactly enough is enough
    with pytest.raises(RuntimeError) as e:
        ops.require_free_bytes(free + 1, dev, "Thing(3) needs", "use less")
    assert str(e.value) == "Thing(3) needs %d bytes of device memory (5.0 GB), %d are free: use less" % (free + 1, free)
    with pytest.raises(RuntimeError, match="%d are free" % 7):                           # a figure the caller has already
        ops.require_free_bytes(8, None, "Thing needs", "use less", free=7)
