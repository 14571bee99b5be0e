"""Which products ATen's lerp contracts on this GPU, and the EMA kernel against it
(csrc/common.h lerp_rule): for weights in both of ATen's branches, the number of elements of
``torch._foreach_lerp_(a, b, w)`` that differ from (1) the EMA kernel, (2) the formula with every
operation rounded on its own (torch ops, one rounding each), (3) the formula with the product and
the sum as one fma (emulated in float64: the product of two float32 values is exact there, and
the one rounding to float32 follows).

    python scripts/exp/ema_vs_torch.py [--out FILE]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ddp_practice_amd import _ext

    C = _ext.load()
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    n = 1 << 20
    x = (torch.randn(n, generator=gen) * torch.logspace(-3, 3, n)).to(dev)
    y = (torch.randn(n, generator=gen) * torch.logspace(-3, 3, n).flip(0)).to(dev)
    lines = [f"optim.EMA's kernel vs torch._foreach_lerp_ on this GPU, torch {torch.__version__}: elements of {n:,} "
             "that differ from _foreach_lerp_(a, b, w)",
             f"{'w (Python double)':>20s} {'branch':>8s} {'EMA kernel':>11s} {'every op rounded':>17s} {'one fma':>8s}"]
    for w in (1.0 - 0.999, 1.0 - 0.9999, 0.1, 0.3, 0.49, 0.5, 1.0 - 0.3, 0.9, 0.999, 1.0):
        want = x.clone()
        torch._foreach_lerp_([want], [y], w)
        s = x.clone()
        cnt = torch.ones((), dtype=torch.int64, device=dev)
        ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        C.ema.ema_update([s], [y], [False], cnt, ticket, w, 1.0 - w, False)
        wf = torch.tensor(w, dtype=torch.float32, device=dev)
        d = y - x
        if abs(w) < 0.5:
            plain = x + wf * d
            fma = (x.double() + wf.double() * d.double()).float()
        else:
            plain = y - d * (1.0 - wf)
            fma = (y.double() - d.double() * (1.0 - wf).double()).float()
        torch.cuda.synchronize()
        diff = lambda t: int((t.view(torch.int32) != want.view(torch.int32)).sum())  # noqa: E731
        lines.append(f"{w!r:>20s} {'< 0.5' if abs(w) < 0.5 else '>= 0.5':>8s} {diff(s):11d} {diff(plain):17d} "
                     f"{diff(fma):8d}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
