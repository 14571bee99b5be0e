"""Narrow pointwise convs of MobileNetV1 (widths 0.25, 0.5, 0.75, 1.0; 224 x 224) at batch 128: the
pointwise kernels (ops/conv_pw.py) against what ops/conv1x1.py ran for them before (the ``else``
branch of Conv1x1Fn: the weight cast, ``torch.mm`` forward and data gradient, split-K ``torch.bmm``
+ ``sum`` weight gradient), per operation.  Narrow: C or K no multiple of 64, the shapes the
implicit-GEMM kernel refuses.

  python scripts/pwconv_bench.py [--batch 128] [--dtype bf16] [--repeats 5] > profiles/pwconv_bench.txt

Each figure is the median of ``repeats`` windows of ``iters`` back-to-back calls timed with
device events after a warm-up; min..max of the windows is the spread.  GB/s: the bytes the
operation has to move (activations in and out once, the fp32 weights once) over the native time.
A row marked LOSES belongs in ops/conv_pw._LIBRARY_SHAPES.
"""
import argparse
import statistics

import torch

from ddp_practice_amd._ext import load
from ddp_practice_amd.models.mobilenet import _BLOCKS, _width
from ddp_practice_amd.ops.conv1x1 import _wgrad

CL = torch.channels_last
# one shape of the chunked regime (C and K above 256, weights restaged per tile), which no narrow
# MobileNetV1 conv reaches, and one with two channel blocks in the single-stage regime
PROBES = [(520, 264, 14), (256, 120, 28)]


def shapes():
    """{width: [(C, K, side), ...]} of the pointwise convs the implicit-GEMM kernel refuses."""
    out = {}
    for mult in (0.25, 0.5, 0.75, 1.0):
        c, side, rows = _width(32, mult), 112, []
        for cout, stride in _BLOCKS:
            side, k = side // stride, _width(cout, mult)
            if c % 64 or k % 64:
                rows.append((c, k, side))
            c = k
        out[mult] = rows
    return out


def windows(fn, iters, repeats):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / iters)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}[a.dtype]
    K_ = load().conv_pw
    N = a.batch
    by_width = shapes()
    print(f"# pointwise 1x1, batch {N}, {a.dtype}; us per call: median (min..max) of {a.repeats} windows of "
          f"{a.iters} calls; fallback = weight cast + torch.mm (fwd, dgrad), torch.bmm + sum (wgrad)")
    for mult, rows in by_width.items():
        print(f"# width {mult}: " + ", ".join(f"{c}->{k}@{s}" for c, k, s in rows))
    print(f"{'C':>4} {'K':>4} {'HxW':>7} {'op':>5} | {'native us':>24} {'GB/s':>6} | {'fallback us':>24} | fb/native")
    tot = {"native": 0.0, "fallback": 0.0}
    todo = sorted({r for rows in by_width.values() for r in rows}, key=lambda r: (-r[2], r[0], r[1])) + PROBES
    print("# probes (no MobileNetV1 conv): " + ", ".join(f"{c}->{k}@{s}" for c, k, s in PROBES))
    for C, K, H in todo:
        x = torch.randn(N, C, H, H, device="cuda").to(dt).contiguous(memory_format=CL)
        w = torch.randn(K, C, 1, 1, device="cuda")
        y = torch.empty(N, K, H, H, device="cuda", dtype=dt).contiguous(memory_format=CL)
        dy = torch.randn_like(y)
        dx, dw = torch.empty_like(x), torch.empty_like(w)
        P = N * H * H
        slab = torch.empty(int(K_.wgrad_splits(P, K, C)) * w.numel(), device="cuda")
        rows, dyr = x.permute(0, 2, 3, 1).reshape(P, C), dy.permute(0, 2, 3, 1).reshape(P, K)  # views: NHWC in memory
        bx, by, bw = x.numel() * 2, y.numel() * 2, w.numel() * 4
        ops = [("fwd", lambda: K_.fwd(x, w, y), lambda: torch.mm(rows, w.view(K, C).to(dt).t())),
               ("dgrad", lambda: K_.dgrad(dy, w, dx), lambda: torch.mm(dyr, w.view(K, C).to(dt))),
               ("wgrad", lambda: K_.wgrad(dy, x, dw, slab), lambda: _wgrad(dyr, rows).view(K, C, 1, 1))]
        for name, nat, lib in ops:
            n, l = windows(nat, a.iters, a.repeats), windows(lib, a.iters, a.repeats)
            if (C, K, H) not in PROBES:
                tot["native"] += n[0]
                tot["fallback"] += l[0]
            print(f"{C:>4} {K:>4} {H:>3}x{H:<3} {name:>5} | {n[0]:8.1f} ({n[1]:6.1f}..{n[2]:6.1f}) "
                  f"{(bx + by + bw) / n[0] / 1e3:6.0f} | {l[0]:8.1f} ({l[1]:6.1f}..{l[2]:6.1f}) | {l[0] / n[0]:5.2f}"
                  + ("   LOSES by more than the fallback's spread" if n[0] - l[0] > l[2] - l[1] else ""), flush=True)
    print(f"# sum of medians over the {len(todo) - len(PROBES)} distinct MobileNetV1 shapes x 3 ops: native {tot['native']:.0f} us, "
          f"fallback {tot['fallback']:.0f} us")


if __name__ == "__main__":
    main()
