"""Cost of a per-step device-resident schedule: graph-replayed ConvNet steps (bf16, batch 32,
16 steps per graph) with and without an optim.DeviceLR stepped inside the captured step.

usage: python scripts/exp/lr_sched_cost.py {none|device_lr} [--epochs N]
One variant per process (scripts/exp/lr_sched_cost.sh alternates them); prints one line per
timed epoch and the median, in microseconds per step.  The difference between the variants is
the price of one 64-lane lr_advance launch per step."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from ddp_practice_amd.amp import GradScaler  # noqa: E402
from ddp_practice_amd.data import DeviceLoader, synthetic  # noqa: E402
from ddp_practice_amd.engine import TrainLoop  # noqa: E402
from ddp_practice_amd.models import ConvNet  # noqa: E402
from ddp_practice_amd.nn import CrossEntropyLoss  # noqa: E402
from ddp_practice_amd.optim import SGD, DeviceLR  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("variant", choices=["none", "device_lr"])
    ap.add_argument("--epochs", type=int, default=7)
    ap.add_argument("--steps", type=int, default=2048, help="steps per epoch (a multiple of 16)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = ConvNet(amp_dtype=torch.bfloat16).to(dev)
    opt = SGD(model.parameters(), 1e-4)
    loader = DeviceLoader(synthetic(32 * args.steps, seed=1), batch_size=32, shuffle=False, device=dev,
                          dtype=torch.bfloat16)
    sched = None
    if args.variant == "device_lr":
        total = args.steps * (args.epochs + 1)
        sched = DeviceLR.from_torch(opt, lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=total), total)
    loop = TrainLoop(model, CrossEntropyLoss(), opt, loader, GradScaler(), steps_per_graph=16, scheduler=sched)
    loop.run_epoch()  # capture + first replays
    torch.cuda.synchronize()
    assert loop.graph_error is None, loop.graph_error
    us = []
    for e in range(args.epochs):
        t0 = time.perf_counter()
        loop.run_epoch()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) / args.steps * 1e6)
        print(f"{args.variant} epoch {e}: {us[-1]:.3f} us/step", flush=True)
    pos = sched.state_dict()["pos"] if sched is not None else None
    print(f"{args.variant} median {statistics.median(us):.3f} us/step  min {min(us):.3f}  max {max(us):.3f}"
          f"  (schedule position {pos})", flush=True)


if __name__ == "__main__":
    main()
