"""optim.AdamW under DDP + SyncBN + bf16 AMP, two processes sharing the GPU over the xGMI
engine: the reducer defers the gradient average to any optimizer with ``fused_amp_step``, and
AdamW's ``_flush_deferred`` (the first thing its step does) runs it."""
import pytest

from ._dist import launch

pytestmark = pytest.mark.gpu


def test_adamw_ddp_ranks_bitwise_equal_and_equal_to_the_reducer_average(C):
    from ._adamw_ddp_worker import worker

    runs = {}
    for fused_grad in (True, False):
        outs = launch(worker, 2, (fused_grad,), timeout=240)
        assert outs[0]["deferred"] == fused_grad
        assert outs[0]["step"] == outs[1]["step"] == 4.0
        assert outs[0]["params"] == outs[1]["params"] and outs[0]["state"] == outs[1]["state"], fused_grad
        runs[fused_grad] = outs[0]
    # deferred to the optimizer (flushed by its step) == averaged by the reducer in backward
    assert runs[True]["params"] == runs[False]["params"] and runs[True]["state"] == runs[False]["state"]
