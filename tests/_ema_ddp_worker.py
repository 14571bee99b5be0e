"""Worker for tests/test_ema_ddp_gpu.py: DDP + SyncBN ConvNet in bf16 AMP with optim.AdamW and an
optim.EMA of the wrapped module (TrainLoop(ema=)), two processes on ONE GPU over the xGMI engine,
four graph-replayed steps.  The update launch reads the parameters after the optimizer's step,
whichever launch averaged the gradients."""
import hashlib
import os
import traceback

import torch


def _digest(tensors):
    h = hashlib.sha1()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def worker(rank, world, port, fused_grad, decay, q):
    try:
        from ._dist import client_env

        os.environ.update(client_env(rank, world, port))
        os.environ["DPA_FUSED_GRAD"] = "1" if fused_grad else "0"
        torch.cuda.set_device(0)
        import ddp_practice_amd.distributed as dist
        from ddp_practice_amd.amp import GradScaler
        from ddp_practice_amd.data import DeviceLoader, DistributedSampler, synthetic
        from ddp_practice_amd.engine import TrainLoop
        from ddp_practice_amd.models import ConvNet
        from ddp_practice_amd.nn import CrossEntropyLoss
        from ddp_practice_amd.optim import EMA, AdamW
        from ddp_practice_amd.parallel import DistributedDataParallel, XgmiCommunicator, convert_sync_batchnorm

        c = dist.init_process_group("xgmi")
        assert isinstance(c, XgmiCommunicator)
        torch.manual_seed(rank)  # different init per rank: DDP broadcasts rank 0's
        ddp = DistributedDataParallel(convert_sync_batchnorm(ConvNet(amp_dtype=torch.bfloat16).cuda()), device_ids=[0],
                                      gradient_as_bucket_view=True)
        ds = synthetic(16 * world * 4, seed=11)  # 4 full steps
        sampler = DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=False)
        loader = DeviceLoader(ds, batch_size=16, shuffle=False, sampler=sampler, device="cuda", dtype=torch.bfloat16)
        opt = AdamW(ddp.parameters(), lr=1e-3, weight_decay=0.01)
        ema = EMA(ddp, decay=decay)  # created after the broadcast: every rank starts from rank 0's weights
        assert ema.model is ddp.module
        loop = TrainLoop(ddp, CrossEntropyLoss(), opt, loader, GradScaler(), use_graph=True, steps_per_graph=4,
                         ema=ema)
        loop.run_epoch()
        torch.cuda.synchronize()
        assert loop.graph_error is None, loop.graph_error
        assert loop.global_step == 4
        assert c.async_error() == "", c.async_error()
        live = ddp.module.state_dict()
        res = {"params": _digest(list(ddp.module.parameters())),
               "shadows": _digest(list(ema.shadows.values())), "keys": list(ema.shadows),
               "n_averaged": int(ema.n_averaged),
               "averaged": not torch.equal(ema.shadows["fc.weight"], live["fc.weight"])}
        dist.destroy_process_group()
        q.put((rank, "ok", res))
    except Exception:  # pragma: no cover - reported to the parent
        q.put((rank, "err", traceback.format_exc()))
    finally:
        q.close()
        q.join_thread()
        os._exit(0)
