"""Same-box A/B of what global-norm gradient clipping costs (csrc/kernels/clip.hip), graph-replayed,
on the gradient set of ResNet-50 (161 tensors, 25.6 M floats) or the ConvNet (10 tensors, 29,034):

  * the AMP AdamW step (``fused_amp_step``: check, update, scale update) without a clip and with
    one (``set_grad_clip``: the norm launch in place of the non-finite check, the coefficient
    read by the update);
  * ``optim.clip_grad_norm_`` alone, on steps that clip and on steps that do not (the scale
    launch then returns after one load per workgroup);
  * ``torch.nn.utils.clip_grad_norm_(foreach=True)`` alone, on the same two kinds of step.

    python scripts/exp/clip_step_ab.py --set resnet50 [--rounds 5] [--steps 20] [--out FILE]

Every variant is one captured graph of --steps steps; a round replays each variant's graph once
after the others (alternating), timed by events around the replay; the table gives the median,
minimum and maximum of the rounds in microseconds per step.  "clips" uses max_norm = 1e-30: the
gradients shrink from replay to replay but the coefficient stays below 1, so every step reads
and writes every gradient (a max_norm near the norm would stop clipping after the first step).
For orientation: the norm pass reads 4 bytes per parameter, the scale pass moves 8.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

import torch  # noqa: E402

from adamw_step_ab import capture, shapes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="resnet50", choices=["resnet50", "convnet"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ddp_practice_amd import _ext
    from ddp_practice_amd.optim import AdamW, clip_grad_norm_

    _ext.load()
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
    for clip in (None, 1e-30, 1e30):
        ps = params()
        opt = AdamW(ps, **hyper)
        opt.set_grad_clip(clip)
        scale = torch.full((1,), 1.0, device=dev)
        tracker = torch.zeros(1, dtype=torch.int32, device=dev)
        found_inf = torch.zeros(1, device=dev)
        opt.step()  # state, tables, clip words: before capture

        def amp_step(opt=opt, scale=scale, tracker=tracker, found_inf=found_inf):
            opt.fused_amp_step(scale, tracker, found_inf, 2.0, 0.5, 1 << 30)

        name = "no clip" if clip is None else ("clip, clips" if clip < 1 else "clip, does not clip")
        graphs[f"AMP AdamW step, {name}"] = capture(amp_step, a.steps)
        keep.append((ps, opt, scale, tracker, found_inf))
    for clip in (1e-30, 1e30):
        kind = "clips" if clip < 1 else "does not clip"
        ps = params()
        graphs[f"optim.clip_grad_norm_ alone, {kind}"] = capture(lambda ps=ps, clip=clip: clip_grad_norm_(ps, clip),
                                                                 a.steps)
        keep.append(ps)
        ps = params()
        graphs[f"torch clip_grad_norm_(foreach=True) alone, {kind}"] = capture(
            lambda ps=ps, clip=clip: torch.nn.utils.clip_grad_norm_(ps, clip, foreach=True), a.steps)
        keep.append(ps)

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
        lines.append(f"{k:55s} {statistics.median(ts):9.2f}  ({min(ts):.2f}-{max(ts):.2f})")
    lines.append(f"{'one read of the gradients, 4 B/parameter at 5.5 TB/s':55s} {numel * 4 / 5.5e12 * 1e6:9.2f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
