"""optim.AdamW with a gradient clip under DDP + SyncBN + bf16 AMP, two processes sharing the GPU
over the xGMI engine: every rank clips by the same global norm of the averaged gradients, whether
the reducer averaged them in backward or left that to the optimizer's step (which flushes before
its norm launch reads them)."""
import pytest

from ._dist import launch

pytestmark = pytest.mark.gpu

CLIP = 0.05  # far below the ConvNet's first gradient norms (about 1): every step clips


def test_clipped_adamw_ddp_ranks_bitwise_equal_and_equal_to_the_reducer_average(C):
    from ._clip_ddp_worker import worker

    runs = {}
    for fused_grad in (True, False):
        outs = launch(worker, 2, (fused_grad, CLIP), timeout=240)
        assert outs[0]["deferred"] == fused_grad
        assert outs[0]["step"] == outs[1]["step"] == 4.0
        assert outs[0]["params"] == outs[1]["params"] and outs[0]["state"] == outs[1]["state"], fused_grad
        assert outs[0]["grad_norm"] == outs[1]["grad_norm"] and outs[0]["grad_norm"] > CLIP, outs[0]["grad_norm"]
        runs[fused_grad] = outs[0]
    # deferred to the optimizer (flushed by its step) == averaged by the reducer in backward
    assert runs[True]["params"] == runs[False]["params"] and runs[True]["state"] == runs[False]["state"]
    assert runs[True]["grad_norm"] == runs[False]["grad_norm"]
