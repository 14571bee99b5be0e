"""Same-box measurement of what optim.EMA costs (csrc/kernels/ema.hip), on the tensor set of
ResNet-50 (161 parameters + 159 buffers) or the ConvNet (10 + 6):

  * ``EMA.update()`` alone, graph-replayed: the kernel's variants (1 / 2 / 4 granules per lane;
    ``ema.set_variant``), with the buffers copied and averaged;
  * ``torch.optim.swa_utils.AveragedModel.update_parameters`` (EMA configuration) on the same
    set, eager -- its host branch cannot be captured -- timed by a host clock around a window
    that ends in a device synchronise;
  * ``--set convnet``: the whole graph-replayed training step (``TrainLoop``, bf16 AMP, SGD, 16
    steps per graph) with and without ``ema=``, as epochs of 1875 steps timed the same way.

    python scripts/exp/ema_update_ab.py --set resnet50 [--rounds 5] [--steps 20] [--out FILE]

Every captured variant is one graph of --steps updates; a round replays each variant's graph
once after the others (alternating), timed by events around the replay; the table gives the
median, minimum and maximum of the rounds in microseconds per update.  The traffic floor counts
12 bytes per averaged element (shadow read and written, source read) and 8 per copied one.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

import torch  # noqa: E402
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn  # noqa: E402

from adamw_step_ab import capture  # noqa: E402


def model_of(which):
    if which == "resnet50":
        from ddp_practice_amd.models import resnet50

        return resnet50(fused=False)
    from ddp_practice_amd.models import ConvNet

    return ConvNet(fused=False)


def convnet_step(rounds, lines):
    from ddp_practice_amd.amp import GradScaler
    from ddp_practice_amd.data import DeviceLoader, synthetic
    from ddp_practice_amd.engine import TrainLoop
    from ddp_practice_amd.models import ConvNet
    from ddp_practice_amd.nn import CrossEntropyLoss
    from ddp_practice_amd.optim import EMA, SGD

    dev = torch.device("cuda")
    ds = synthetic(60000, seed=1, device=dev)
    loops = {}
    for name in ("step without ema", "step with ema=EMA(decay 0.999)"):
        torch.manual_seed(0)
        model = ConvNet(amp_dtype=torch.bfloat16).to(dev)
        loader = DeviceLoader(ds, batch_size=32, shuffle=False, device=dev, dtype=torch.bfloat16)
        ema = EMA(model, decay=0.999) if "with ema" in name else None
        loops[name] = TrainLoop(model, CrossEntropyLoss().to(dev), SGD(model.parameters(), lr=1e-4), loader,
                                GradScaler(), use_graph=True, steps_per_graph=16, ema=ema)
    steps = 60000 // 32
    times = {k: [] for k in loops}
    for r in range(1 + rounds):  # the first epoch captures
        for k, loop in loops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop.run_epoch()
            torch.cuda.synchronize()
            if r >= 1:
                times[k].append((time.perf_counter() - t0) * 1e6 / steps)
            assert loop.graph_error is None, loop.graph_error
    lines.append(f"# ConvNet training step, bf16 AMP + SGD, graph-replayed (16 steps per graph), epochs of {steps} "
                 f"steps, {rounds} alternating rounds; us per step: median (min-max)")
    for k, ts in times.items():
        lines.append(f"{k:62s} {statistics.median(ts):9.2f}  ({min(ts):.2f}-{max(ts):.2f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="resnet50", choices=["resnet50", "convnet"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ddp_practice_amd import _ext
    from ddp_practice_amd.optim import EMA

    C = _ext.load()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    graphs, keep = {}, []
    counts = None
    for u, buffers in [(0, False), (1, False), (2, False), (4, False), (0, True)]:
        model = model_of(a.set).to(dev)
        ema = EMA(model, decay=0.999, use_buffers=buffers)
        ema.update()  # n_averaged = 1: the replays average
        C.ema.set_variant(u)
        name = (f"EMA.update(), {'granules/lane by size' if u == 0 else str(u) + ' granules/lane'}"
                f"{', use_buffers' if buffers else ''}")
        graphs[name] = capture(ema.update, a.steps)
        keep.append((model, ema))
        if counts is None:
            avg = sum(s.numel() for k, s in ema.shadows.items() if not ema._copy[k])
            cp = sum(s.numel() * s.element_size() // 4 for k, s in ema.shadows.items() if ema._copy[k])
            counts = (len(ema.shadows), avg, cp)
    C.ema.set_variant(0)

    times = {k: [] for k in graphs}
    for r in range(a.warmup + a.rounds):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.steps)
    # torch's AveragedModel, eager
    for buffers in (False, True):
        model = model_of(a.set).to(dev)
        avg = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(0.999), use_buffers=buffers)
        k = f"torch AveragedModel.update_parameters, eager{', use_buffers' if buffers else ''}"
        times[k] = []
        for r in range(a.warmup + a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                avg.update_parameters(model)
            torch.cuda.synchronize()
            if r >= a.warmup:
                times[k].append((time.perf_counter() - t0) * 1e6 / a.steps)
    rows, n_avg, n_copy = counts
    lines = [f"# {a.set}: {rows} rows, {n_avg:,} averaged floats, {n_copy:,} copied words (use_buffers off); graphs of "
             f"{a.steps} updates, {a.rounds} alternating rounds after {a.warmup} warm-up rounds; us per update: "
             "median (min-max)"]
    for k, ts in times.items():
        lines.append(f"{k:62s} {statistics.median(ts):9.2f}  ({min(ts):.2f}-{max(ts):.2f})")
    nbytes = 12 * n_avg + 8 * n_copy
    for bw in (5.5e12, 6.0e12):
        lines.append(f"{f'traffic floor, {nbytes:,} B at {bw / 1e12:.1f} TB/s':62s} {nbytes / bw * 1e6:9.2f}")
    if a.set == "convnet":
        convnet_step(a.rounds, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
