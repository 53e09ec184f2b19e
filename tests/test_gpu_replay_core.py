"""``train.StagedUpload`` on the device, with one and with two pinned slots: a refill never overtakes a copy in flight, an upload inside
a stream capture neither waits for nor records an event and becomes a node of the graph, and construction during a capture is refused.
Run with `-m gpu` on an MI355X."""
import pytest
import torch

from spoofsv_amd.train import StagedUpload

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _upload(up, value):
    up.host().fill_(value)
    up.send()


@pytest.mark.parametrize("slots", [1, 2])
def test_back_to_back_uploads_each_arrive_whole(slots):
    dst = torch.full((8,), -1, dtype=torch.int32, device=DEV)
    up = StagedUpload(dst, slots=slots)
    assert len(up.events) == slots
    clones = []
    for i in range(5):
        _upload(up, i)
        clones.append(dst.clone())
    torch.cuda.synchronize()
    for i, c in enumerate(clones):
        assert c.cpu().tolist() == [i] * 8, (slots, i)


@pytest.mark.parametrize("slots", [1, 2])
def test_an_upload_under_capture_is_a_graph_node_and_touches_no_event(slots):
    dst = torch.zeros((8,), dtype=torch.int32, device=DEV)
    out = torch.zeros((8,), dtype=torch.int32, device=DEV)
    up = StagedUpload(dst, slots=slots)
    _upload(up, 3)
    torch.cuda.synchronize()
    events = list(up.events)
    assert all(ev.query() for ev in events)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                      # (an event wait or record on this thread would fail the capture)
        _upload(up, 7)
        out.copy_(dst)
    assert len(up.events) == slots and all(a is b for a, b in zip(up.events, events))
    assert all(ev.query() for ev in up.events)     # none was recorded into the capture: all are still complete
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [0] * 8           # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [7] * 8 and dst.cpu().tolist() == [7] * 8


def test_construction_during_a_capture_is_refused():
    dst = torch.zeros((8,), dtype=torch.int32, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                      # (the context ends the capture whatever happens inside; one node, so it is not empty)
        dst.add_(1)
        with pytest.raises(RuntimeError, match="cannot be allocated during a hipGraph capture"):
            StagedUpload(dst)
    torch.cuda.synchronize()
    assert dst.cpu().tolist() == [0] * 8
