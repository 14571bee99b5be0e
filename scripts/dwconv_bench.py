"""Depthwise 3x3 convs of MobileNetV1 (or, with --ksize 5, the 5x5 convs of MnasNet-B1) at batch
128: the depthwise kernels (ops/conv_dw.py) against the library branch of
models/resnet.py::_conv (weight cast, aten.convolution with groups == C, convolution_backward,
the weight gradient cast back to fp32), per operation.

  python scripts/dwconv_bench.py [--batch 128] [--dtype bf16] [--repeats 5] > profiles/dwconv_bench.txt
  python scripts/dwconv_bench.py --ksize 5 > profiles/dwconv5_bench.txt

Each figure is the median of ``repeats`` windows of ``iters`` back-to-back calls timed with
device events after a warm-up; min..max of the windows is the spread.  GB/s: the bytes the
operation has to move (activations in and out once, the fp32 weights once) over the native time;
GFMA/s: k * k multiply-adds per element of y (at stride 2 the data gradient's count per element
of dy: the same number) over the native time.
"""
import argparse
import statistics

import torch

from ddp_practice_amd._ext import load

# (C, input side, stride) of the 13 depthwise convs at 224 x 224
SHAPES = [(32, 112, 1), (64, 112, 2), (128, 56, 1), (128, 56, 2), (256, 28, 1), (256, 28, 2)] \
    + [(512, 14, 1)] * 5 + [(512, 14, 2), (1024, 7, 1)]
# (C, input side, stride) of MnasNet-B1's ten 5x5 depthwise convs at 224 x 224
SHAPES5 = [(72, 56, 2), (120, 28, 1), (120, 28, 1), (240, 28, 2), (480, 14, 1), (480, 14, 1), (576, 14, 2)] \
    + [(1152, 7, 1)] * 3
CL = torch.channels_last


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
    ap.add_argument("--ksize", type=int, default=3, choices=[3, 5])
    a = ap.parse_args()
    k, pad = a.ksize, a.ksize // 2
    shapes = SHAPES if k == 3 else SHAPES5
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}[a.dtype]
    K = load().conv_dw if k == 3 else load().conv_dw5
    N = a.batch
    print(f"# depthwise {k}x{k}, batch {N}, {a.dtype}; us per call: median (min..max) of {a.repeats} windows "
          f"of {a.iters} calls; library = weight cast + aten.convolution / convolution_backward (+ cast back)")
    print(f"{'C':>5} {'HxW':>7} {'s':>1} {'x':>2} {'op':>5} | {'native us':>24} {'GB/s':>6} {'GFMA/s':>7} | {'library us':>24} | lib/native")
    tot = {"native": 0.0, "library": 0.0}
    for C, H, s in sorted(set(shapes), key=shapes.index):
        mult, OH = shapes.count((C, H, s)), (H - 1) // s + 1
        x = torch.randn(N, C, H, H, device="cuda").to(dt).contiguous(memory_format=CL)
        w = torch.randn(C, 1, k, k, device="cuda")
        y = torch.empty(N, C, OH, OH, device="cuda", dtype=dt).contiguous(memory_format=CL)
        dy = torch.randn_like(y)
        dx, dw = torch.empty_like(x), torch.empty_like(w)
        slab = torch.empty(int(K.wgrad_splits(N, OH, OH, C, s)) * w.numel(), device="cuda")
        wl = w.to(dt)
        bx, by, bw = x.numel() * 2, y.numel() * 2, w.numel() * 4
        fmas = y.numel() * k * k

        def lib_fwd():
            o = torch.ops.aten.convolution(x, w.to(dt), None, [s, s], [pad, pad], [1, 1], False, [0, 0], C)
            return o if o.is_contiguous(memory_format=CL) else o.contiguous(memory_format=CL)

        def lib_bwd(mask):
            r = torch.ops.aten.convolution_backward(dy, x, wl, None, [s, s], [pad, pad], [1, 1], False, [0, 0], C, mask)
            return r[1].float() if mask[1] else r[0]

        ops = [("fwd", lambda: K.fwd(x, w, y, s), lib_fwd, bx + by + bw),
               ("dgrad", lambda: K.dgrad(dy, w, dx, s), lambda: lib_bwd([True, False, False]), bx + by + bw),
               ("wgrad", lambda: K.wgrad(dy, x, dw, s, slab), lambda: lib_bwd([False, True, False]), bx + by + bw)]
        for name, nat, lib, nbytes in ops:
            n, l = windows(nat, a.iters, a.repeats), windows(lib, a.iters, a.repeats)
            tot["native"] += mult * n[0]
            tot["library"] += mult * l[0]
            print(f"{C:>5} {H:>3}x{H:<3} {s} {mult:>2} {name:>5} | {n[0]:8.1f} ({n[1]:6.1f}..{n[2]:6.1f}) "
                  f"{nbytes / n[0] / 1e3:6.0f} {fmas / n[0] / 1e3:7.0f} | {l[0]:8.1f} ({l[1]:6.1f}..{l[2]:6.1f}) | {l[0] / n[0]:5.2f}"
                  + ("   LOSES by more than the library's spread" if n[0] - l[0] > l[2] - l[1] else ""), flush=True)
    print(f"# sum of medians over the {len(shapes)} convs x 3 ops: native {tot['native']:.0f} us, library {tot['library']:.0f} us")


if __name__ == "__main__":
    main()
