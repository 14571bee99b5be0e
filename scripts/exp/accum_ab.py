"""Same-box measurement of what gradient accumulation costs (csrc/kernels/accum.hip,
optim/accum.py), on the gradient set of ResNet-50 (161 tensors) or the ConvNet (10):

  * the accumulate launch alone, graph-replayed, per mode (first / add / last): the kernel's
    variants (1 / 2 / 4 granules per lane, plain and non-temporal loads of the accumulator;
    ``accum.set_variant``) against ``torch._foreach_copy_`` / ``_foreach_add_`` /
    ``_foreach_add`` + ``_foreach_mul_`` on the same tensors and the traffic floor (8 B per
    element for first, 12 B for add and last);
  * ``--set convnet``: the graph-replayed training loop (``TrainLoop``, bf16 AMP, SGD, batch 32)
    per micro-step: the plain step, ``accum_steps=4``, and the route this replaces -- ``.grad``
    kept between the backwards of a window (``accum_impl="torch"`` on the native model), which
    makes the fused producers step aside and autograd add per parameter.

    python scripts/exp/accum_ab.py --set resnet50 [--rounds 5] [--steps 20] [--out FILE]

Every captured variant is one graph of --steps launches; a round replays each variant's graph
once after the others (alternating), timed by events around the replay; the table gives the
median, minimum and maximum of the rounds in microseconds per launch.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

import torch  # noqa: E402

from adamw_step_ab import capture  # noqa: E402
from ema_update_ab import model_of  # noqa: E402


def convnet_windows(rounds, lines, K=4):
    from ddp_practice_amd.amp import GradScaler
    from ddp_practice_amd.data import DeviceLoader, synthetic
    from ddp_practice_amd.engine import TrainLoop
    from ddp_practice_amd.models import ConvNet
    from ddp_practice_amd.nn import CrossEntropyLoss
    from ddp_practice_amd.optim import SGD

    dev = torch.device("cuda")
    micro = 1872  # a multiple of 16 and of K: whole graphs, whole windows, no eager tail
    ds = synthetic(32 * micro, seed=1, device=dev)
    loops = {}
    for name, kw in (("plain step (accum_steps=1)", {}),
                     (f"accum_steps={K} (one accumulate launch per micro-step)", dict(accum_steps=K)),
                     (f"accum_steps={K}, .grad kept between backwards (autograd adds)",
                      dict(accum_steps=K, accum_impl="torch"))):
        torch.manual_seed(0)
        model = ConvNet(amp_dtype=torch.bfloat16).to(dev)
        loader = DeviceLoader(ds, batch_size=32, shuffle=False, device=dev, dtype=torch.bfloat16)
        loops[name] = TrainLoop(model, CrossEntropyLoss().to(dev), SGD(model.parameters(), lr=1e-4), loader,
                                GradScaler(), use_graph=True, steps_per_graph=16, **kw)
    times = {k: [] for k in loops}
    for r in range(1 + rounds):  # the first epoch captures
        for k, loop in loops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop.run_epoch()
            torch.cuda.synchronize()
            if r >= 1:
                times[k].append((time.perf_counter() - t0) * 1e6 / micro)
            assert loop.graph_error is None, loop.graph_error
    lines.append(f"# ConvNet training loop, bf16 AMP + SGD, batch 32, graph-replayed (16 micro-steps per graph), epochs "
                 f"of {micro} micro-steps, {rounds} alternating rounds; us per micro-step: median (min-max)")
    for k, ts in times.items():
        lines.append(f"{k:66s} {statistics.median(ts):9.2f}  ({min(ts):.2f}-{max(ts):.2f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="resnet50", choices=["resnet50", "convnet"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ddp_practice_amd import _ext

    C = _ext.load()
    A = C.accum
    dev = torch.device("cuda")
    torch.manual_seed(0)
    params = [p.detach() for p in model_of(a.set).to(dev).parameters()]
    grads = [torch.randn_like(p) for p in params]
    n = sum(g.numel() for g in grads)
    flat = torch.zeros(sum((g.numel() + 3) // 4 * 4 for g in grads), dtype=torch.float32, device=dev)
    accs, o = [], 0
    for g in grads:
        accs.append(flat[o:o + g.numel()].view(g.shape))
        o += (g.numel() + 3) // 4 * 4
    kw, lists = {}, (accs, grads)
    if len(grads) > A.MAXT:
        kw = {"table": A.accum_table(accs, grads), "total_granules": sum((g.numel() + 3) // 4 for g in grads)}
        lists = ([], [])
    c = 1.0  # with the accumulators zeroed before every replay, last leaves g as it is: nothing drifts
    graphs = {}
    modes = (("first", A.FIRST), ("add", A.ADD), ("last", A.LAST))
    for mname, mode in modes:
        for u, nt in [(0, False), (1, False), (2, False), (4, False), (0, True), (2, True)]:
            if nt and mode == A.FIRST:
                continue  # first does not load the accumulator
            A.set_variant(u, nt)
            name = (f"accumulate {mname:5s} {'granules/lane by size' if u == 0 else str(u) + ' granules/lane'}"
                    f"{', non-temporal acc loads' if nt else ''}")
            graphs[name] = capture(lambda mode=mode: A.accumulate(*lists, mode, c, **kw), a.steps)
    A.set_variant(0, False)
    graphs["torch._foreach_copy_(accs, grads)              [first]"] = capture(
        lambda: torch._foreach_copy_(accs, grads), a.steps)
    graphs["torch._foreach_add_(accs, grads)               [add]"] = capture(
        lambda: torch._foreach_add_(accs, grads), a.steps)

    def torch_last():
        t = torch._foreach_add(accs, grads)
        torch._foreach_mul_(t, c)

    graphs["torch._foreach_add(accs, grads) + _foreach_mul_ [last, into new tensors]"] = capture(torch_last, a.steps)

    times = {k: [] for k in graphs}
    for r in range(a.warmup + a.rounds):
        for k, g in graphs.items():
            flat.zero_()  # the sums stay finite however often a graph has run
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.steps)
    lines = [f"# {a.set}: {len(grads)} gradients, {n:,} floats; graphs of {a.steps} launches, {a.rounds} alternating "
             f"rounds after {a.warmup} warm-up rounds; us per launch: median (min-max)"]
    for k, ts in times.items():
        lines.append(f"{k:78s} {statistics.median(ts):9.2f}  ({min(ts):.2f}-{max(ts):.2f})")
    for what, per in (("first", 8), ("add / last", 12)):
        for bw in (5.5e12, 6.0e12):
            lines.append(f"{f'traffic floor {what}, {per * n:,} B at {bw / 1e12:.1f} TB/s':78s} "
                         f"{per * n / bw * 1e6:9.2f}")
    if a.set == "convnet":
        convnet_windows(a.rounds, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
