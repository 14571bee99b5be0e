"""Worker bodies for tests/test_accum_ref_cpu.py (run under tests/_dist.run)."""
import torch
import torch.nn as nn

from ._ddp_workers import _batch


def ddp_syncbn_accum(rank, world, per_rank, K, bucket_view):
    """DDP(SyncBN ConvNet) with GradAccumulator(steps=K) on per-rank shards == one process that,
    per micro-step, runs the ranks' micro-batches concatenated and accumulates the same way."""
    from ddp_practice_amd.models import ConvNet
    from ddp_practice_amd.optim import SGD, GradAccumulator
    from ddp_practice_amd.parallel import DistributedDataParallel, convert_sync_batchnorm

    torch.manual_seed(0)
    ref = ConvNet()
    model = ConvNet()
    model.load_state_dict(ref.state_dict())
    model = DistributedDataParallel(convert_sync_batchnorm(model), gradient_as_bucket_view=bucket_view)
    opt = SGD(model.parameters(), lr=0.1)
    ref_opt = SGD(ref.parameters(), lr=0.1)
    acc = GradAccumulator(opt, steps=K, model=model)
    ref_acc = GradAccumulator(ref_opt, steps=K)
    mode = acc._ddp
    assert mode == ("defer" if bucket_view else "no_sync"), mode
    local_differs = False
    for window in range(2):
        for i in range(K):
            x, y = _batch(10 * window + i, per_rank * world)
            xs, ys = x[rank * per_rank:(rank + 1) * per_rank], y[rank * per_rank:(rank + 1) * per_rank]
            opt.zero_grad(set_to_none=True)
            with acc.micro_step():
                nn.functional.cross_entropy(model(xs), ys).backward()
            ref_opt.zero_grad(set_to_none=True)
            nn.functional.cross_entropy(ref(x), y).backward()
            if i == 0:
                # a non-final micro-step's gradients are this rank's own: nothing was averaged
                mine = model.module.fc.weight.grad
                local_differs |= not torch.allclose(mine, ref.fc.weight.grad, rtol=1e-4, atol=1e-5)
            done = acc.accumulate()
            assert ref_acc.accumulate() == done == (i == K - 1)
            if bucket_view:
                assert not model.deferred_grad_sync_pending()
            if not done:
                assert all(p.grad is None for p in model.parameters())
        for (n, p), (_, q) in zip(model.module.named_parameters(), ref.named_parameters()):
            torch.testing.assert_close(p.grad, q.grad, rtol=1e-4, atol=1e-5, msg=f"grad {n} window {window}")
        opt.step()
        ref_opt.step()
    for (n, b), (_, rb) in zip(model.module.named_buffers(), ref.named_buffers()):
        torch.testing.assert_close(b.float(), rb.float(), rtol=1e-4, atol=1e-5, msg=f"buffer {n}")
    assert local_differs
    # plain bytes: a tensor on the queue shares its storage with a process that has left by then
    return [p.detach().numpy().tobytes() for p in model.parameters()]
