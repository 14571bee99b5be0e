"""Worker for tests/test_accum_ddp_gpu.py: DDP + SyncBN ConvNet in bf16 AMP through
TrainLoop(accum_steps=2), two processes on ONE GPU over the xGMI engine, two windows of two
micro-batches of 8.  Reports digests of the parameters, how often the accumulator dropped and
ran the reducer's deferred average, and how many all-reduces the engine's host side issued."""
import hashlib
import os
import re
import traceback

import torch


def _digest(tensors):
    h = hashlib.sha1()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _issued(xc) -> int:
    """One- and two-shot all-reduces this rank's host has issued (the watchdog report's count)."""
    m = re.search(r"host issued: oneshot (\d+) twoshot (\d+)", xc.debug_state(0.0))
    assert m is not None
    return int(m.group(1)) + int(m.group(2))


def worker(rank, world, port, fused_grad, use_graph, opt_name, q):
    try:
        from ._dist import client_env

        os.environ.update(client_env(rank, world, port))
        os.environ["DPA_FUSED_GRAD"] = "1" if fused_grad else "0"
        torch.cuda.set_device(0)
        import ddp_practice_amd.distributed as dist
        from ddp_practice_amd import optim
        from ddp_practice_amd.amp import GradScaler
        from ddp_practice_amd.data import DeviceLoader, DistributedSampler, synthetic
        from ddp_practice_amd.engine import TrainLoop
        from ddp_practice_amd.models import ConvNet
        from ddp_practice_amd.nn import CrossEntropyLoss
        from ddp_practice_amd.parallel import DistributedDataParallel, XgmiCommunicator, convert_sync_batchnorm

        K, windows = 2, 2
        c = dist.init_process_group("xgmi")
        assert isinstance(c, XgmiCommunicator)
        torch.manual_seed(rank)  # different init per rank: DDP broadcasts rank 0's
        ddp = DistributedDataParallel(convert_sync_batchnorm(ConvNet(amp_dtype=torch.bfloat16).cuda()), device_ids=[0],
                                      gradient_as_bucket_view=True)
        ds = synthetic(8 * world * K * windows, seed=11)
        sampler = DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=False)
        loader = DeviceLoader(ds, batch_size=8, shuffle=False, sampler=sampler, device="cuda", dtype=torch.bfloat16)
        kw = dict(lr=1e-3, weight_decay=0.01) if opt_name == "AdamW" else dict(lr=1e-2)
        opt = getattr(optim, opt_name)(ddp.parameters(), **kw)
        loop = TrainLoop(ddp, CrossEntropyLoss(), opt, loader, GradScaler(), use_graph=use_graph, steps_per_graph=4,
                         accum_steps=K)
        assert loop.accum._ddp == "defer"
        calls = {"drop": 0, "run": 0}
        drop, run = ddp.drop_deferred_grad_sync, ddp.run_deferred_grad_sync

        def count_drop():
            calls["drop"] += ddp.deferred_grad_sync_pending()  # (reset() drops with nothing pending)
            drop()

        def count_run():
            calls["run"] += 1
            run()

        ddp.drop_deferred_grad_sync, ddp.run_deferred_grad_sync = count_drop, count_run
        before = _issued(c.xgmi)
        loop.run_epoch()
        torch.cuda.synchronize()
        issued = _issued(c.xgmi) - before
        assert loop.graph_error is None, loop.graph_error
        assert loop.global_step == windows
        assert not ddp.deferred_grad_sync_pending()
        assert c.async_error() == "", c.async_error()
        res = {"params": _digest(list(ddp.module.parameters())), "calls": calls, "issued": issued,
               "buckets": len(ddp.bucket_sizes_bytes()), "owned": ddp.grad_sync_deferred_to(opt)}
        dist.destroy_process_group()
        q.put((rank, "ok", res))
    except Exception:  # pragma: no cover - reported to the parent
        q.put((rank, "err", traceback.format_exc()))
    finally:
        q.close()
        q.join_thread()
        os._exit(0)
