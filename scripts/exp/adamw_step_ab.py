"""Same-box A/B of the Adam update launch (csrc/kernels/adam.hip), graph-replayed:
the kernel's variants (non-temporal exp_avg / exp_avg_sq loads x granules per lane), the launch
without its step-count advance, and torch.optim.AdamW(fused=True, capturable=True), on the
parameter set of ResNet-50 (161 tensors, 25.6 M floats) or the ConvNet (10 tensors, 29,034).

    python scripts/exp/adamw_step_ab.py --set resnet50 [--rounds 5] [--steps 20] [--out FILE]

Every variant is one captured graph of --steps update launches; a round replays each variant's
graph once after the others (alternating), timed by events around the replay; the table gives
the median, minimum and maximum of the rounds in microseconds per step, and the traffic floor:
28 bytes per parameter (p, g, m, v read; p, m, v written) at 5.5 and 6.0 TB/s, the rates the
BatchNorm passes reach (README "Performance engineering log").
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

import torch  # noqa: E402


def shapes(which):
    if which == "resnet50":
        from ddp_practice_amd.models import resnet50

        return [tuple(p.shape) for p in resnet50(fused=False).parameters()]
    from ddp_practice_amd.models import ConvNet

    return [tuple(p.shape) for p in ConvNet(fused=False).parameters()]


def capture(fn, steps):
    fn()  # state, tables: before capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(steps):
            fn()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="resnet50", choices=["resnet50", "convnet"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ddp_practice_amd import _ext
    from ddp_practice_amd.optim import AdamW

    C = _ext.load()
    dev = torch.device("cuda")
    shp = shapes(a.set)
    numel = sum(torch.Size(s).numel() for s in shp)
    gen = torch.Generator(device="cpu").manual_seed(0)
    hyper = dict(lr=1e-3, weight_decay=0.01)

    def params():
        ps = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev)) for s in shp]
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen).to(dev)
        return ps

    graphs, keep = {}, []
    for nt in (False, True):
        for u in (1, 2, 4):
            C.adam.set_variant(nt, u)  # read at launch, i.e. at capture
            ps = params()
            opt = AdamW(ps, **hyper)
            graphs[f"native nt={int(nt)} u={u}"] = capture(opt.step, a.steps)
            keep.append((ps, opt))
    C.adam.set_variant(True, 2)
    # the same launch without the ticket (the count is not advanced): what the advance costs
    ps = params()
    opt = AdamW(ps, **hyper)
    opt.step()
    groups = opt._collect()
    (group, pp, gg, ms, vs, word), = groups
    lists, kw = opt._launch_args(0, pp, gg, ms, vs)

    def no_advance():
        C.adam.adam_step(*lists, word, 1e-3, 0.9, 0.999, 1e-8, 0.01, True, False, ticket=None, **kw)

    graphs["native nt=1 u=2, no step-count advance"] = capture(no_advance, a.steps)
    keep.append((ps, opt))
    C.adam.set_variant(True, 0)  # the default: granules per lane by size
    ps = params()
    opt = AdamW(ps, **hyper)
    graphs["native default (nt=1, u by size)"] = capture(opt.step, a.steps)
    keep.append((ps, opt))
    ps = params()
    topt = torch.optim.AdamW(ps, fused=True, capturable=True, **hyper)
    graphs["torch fused capturable"] = capture(topt.step, a.steps)
    keep.append((ps, topt))
    ps = params()
    fopt = torch.optim.AdamW(ps, foreach=True, capturable=True, **hyper)
    graphs["torch foreach capturable"] = capture(fopt.step, a.steps)
    keep.append((ps, fopt))

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
    lines = [f"# {a.set}: {len(shp)} tensors, {numel:,} floats; graphs of {a.steps} steps, {a.rounds} alternating "
             f"rounds after {a.warmup} warm-up rounds; us per step: median (min-max)"]
    for k, ts in times.items():
        lines.append(f"{k:45s} {statistics.median(ts):9.2f}  ({min(ts):.2f}-{max(ts):.2f})")
    for rate in (5.5, 6.0):
        lines.append(f"{'traffic floor, 28 B/parameter at %.1f TB/s' % rate:45s} {numel * 28 / (rate * 1e12) * 1e6:9.2f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
