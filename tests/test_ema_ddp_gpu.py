"""optim.EMA under DDP + SyncBN + bf16 AMP, two processes sharing the GPU over the xGMI engine:
every rank keeps the same average of the same weights, whether the reducer averaged the
gradients in backward or left that to the optimizer's step."""
import pytest

from ._dist import launch
from .test_cli_cpu import REF_KEYS

pytestmark = pytest.mark.gpu


def test_ema_ddp_ranks_bitwise_equal_and_equal_to_the_reducer_average(C):
    from ._ema_ddp_worker import worker

    runs = {}
    for fused_grad in (True, False):
        outs = launch(worker, 2, (fused_grad, 0.9), timeout=240)
        assert outs[0]["n_averaged"] == outs[1]["n_averaged"] == 4
        assert outs[0]["keys"] == REF_KEYS  # the wrapped module's names, no "module." prefix
        assert outs[0]["params"] == outs[1]["params"] and outs[0]["shadows"] == outs[1]["shadows"], fused_grad
        assert outs[0]["averaged"] and outs[1]["averaged"]
        runs[fused_grad] = outs[0]
    # deferred to the optimizer's fused step == averaged by the reducer in backward
    assert runs[True]["params"] == runs[False]["params"] and runs[True]["shadows"] == runs[False]["shadows"]
