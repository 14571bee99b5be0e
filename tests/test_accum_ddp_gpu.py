"""optim.GradAccumulator under DDP + SyncBN + bf16 AMP, two processes sharing the GPU over the
xGMI engine: the ranks stay bitwise equal, the graph-replayed run whose optimizer owns the
deferred average equals the eager run whose reducer runs it (``DPA_FUSED_GRAD=0``), and a
window issues one gradient all-reduce per bucket, not one per micro-step."""
import pytest

from ._dist import launch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("opt_name", ["SGD", "AdamW"])
def test_accum_ddp_one_average_per_window(C, opt_name):
    from ._accum_ddp_worker import worker

    runs = {}
    for fused_grad, use_graph in ((True, True), (False, False)):
        outs = launch(worker, 2, (fused_grad, use_graph, opt_name), timeout=240)
        assert outs[0]["params"] == outs[1]["params"], (fused_grad, use_graph)
        assert outs[0]["calls"] == outs[1]["calls"] and outs[0]["issued"] == outs[1]["issued"]
        runs[fused_grad] = outs[0]
    assert runs[True]["params"] == runs[False]["params"]
    # DPA_FUSED_GRAD=0, eager, two windows of two micro-steps: nobody owns the deferral, so the
    # accumulator drops the first micro-step's pending average and runs the second's -- and the
    # engine's host side issued exactly one all-reduce per bucket and window
    r = runs[False]
    assert not r["owned"] and r["buckets"] >= 1
    assert r["calls"] == {"drop": 2, "run": 2}
    assert r["issued"] == 2 * r["buckets"], r
    # the optimizer owns the deferral: its step averages (SGD: inside the fused launch)
    assert runs[True]["owned"] and runs[True]["calls"]["run"] == 0
