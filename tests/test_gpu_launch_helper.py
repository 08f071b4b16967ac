"""ops._launch on the MI355X: one timing event per launch with the kind and variant strings bench.py's tables are keyed
on, and no event objects — and the same bits — when no sink is set. The smallest case there is: a 5-node graph at d = 4
through ops.spmm_raw."""
import pytest
import torch

from rgb_experiment_amd import ops
from rgb_experiment_amd.graph import LOOPS_KEEP, get_graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def test_one_event_per_launch_and_none_without_a_sink(dev, monkeypatch):
    ei = torch.tensor([[0, 1, 2, 3, 4, 0, 2], [1, 2, 3, 4, 0, 2, 2]], dtype=torch.int64, device=dev)
    g = get_graph(ei, 5, LOOPS_KEEP)
    x = torch.arange(20, dtype=torch.float32, device=dev).reshape(5, 4) / 7
    saved = ops._EVENT_SINK
    try:
        sink = []
        ops.set_event_sink(sink)
        with_sink = ops.spmm_raw(g.fwd, None, None, x)
        assert len(sink) == 1
        kind, start, end = sink[0]
        assert kind == "spmm" and isinstance(kind, ops.Kind) and kind.variant == "rows+d4"
        ops.spmm_raw(g.fwd, None, None, x, kind="sum_fwd")
        assert [(k, k.variant) for k, _, _ in sink] == [("spmm", "rows+d4"), ("sum_fwd", "rows+d4")]
        torch.cuda.synchronize()
        assert start.elapsed_time(end) >= 0.0

        ops.set_event_sink(None)
        made = []
        real_event = torch.cuda.Event
        monkeypatch.setattr(torch.cuda, "Event", lambda *a, **k: made.append(1) or real_event(*a, **k))
        without = ops.spmm_raw(g.fwd, None, None, x)
        assert made == [] and len(sink) == 2
        assert torch.equal(with_sink, without)
        ref = torch.zeros(5, 4, dtype=torch.float64)
        ref.index_add_(0, ei[1].cpu(), x.double().cpu()[ei[0].cpu()])
        assert torch.allclose(without.double().cpu(), ref, rtol=1e-6, atol=1e-6)
    finally:
        ops.set_event_sink(saved)
