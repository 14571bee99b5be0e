"""The SE blocks of SE-ResNet-50 / SE-ResNeXt-50 at batch 128: the kernels of csrc/kernels/se.hip
(ops/se.squeeze_excite) against the torch composition of the same math (ops/se.squeeze_excite_torch),
forward and forward + backward, each captured once in a hipGraph and replayed.

  python scripts/se_bench.py [--batch 128] [--dtype bf16] [--repeats 5] > profiles/se_bench.txt

Every figure is one window of ``iters`` replays timed with device events after a warm-up; the four
graphs of a shape are timed in turn, ``repeats`` times over, and every window is printed (no best-of).
backward = (forward + backward) - forward of the same round.  GB/s: the activation bytes the native
kernels have to move (forward: u twice, identity, y; backward: g, y twice, u, du, d_identity; the fp32
vectors and parameters are below 1 %) over the native time -- a rate of the launches together, so a
lower bound on the rate of each activation kernel.  A shape where the native op loses by more than
the spread belongs in ops/se._LIBRARY_SHAPES.
"""
import argparse
import sys

import torch

sys.path.insert(0, __file__.rsplit("/scripts", 1)[0])
from ddp_practice_amd.ops import se as S  # noqa: E402

SHAPES = [(256, 56), (512, 28), (1024, 14), (2048, 7)]
CL = torch.channels_last


def graph_of(fn, leaves, g, backward):
    def step():
        if not backward:
            with torch.no_grad():
                return fn(*leaves)
        return torch.autograd.grad(fn(*leaves), leaves, g)

    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for _ in range(3):
            step()
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            keep = step()
    return graph, keep


def window(graph, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        graph.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}[a.dtype]
    N = a.batch
    print(f"# SE block (reduction 16), batch {N}, {a.dtype}, {torch.cuda.get_device_name(0)}; us per hipGraph "
          f"replay, one window of {a.iters} replays per figure, {a.repeats} rounds in turn")
    for C, H in SHAPES:
        Cr = C // 16
        act = lambda: torch.randn(N, C, H, H, device="cuda").to(dt).contiguous(memory_format=CL).requires_grad_()
        par = lambda *s: (torch.randn(*s, device="cuda") / s[-1] ** 0.5).requires_grad_()
        leaves = [act(), act(), par(Cr, C), par(Cr), par(C, Cr), par(C)]
        g = act().detach()
        graphs = {(name, bwd): graph_of(fn, leaves, g, bwd)
                  for name, fn in (("native", S.squeeze_excite), ("torch", S.squeeze_excite_torch))
                  for bwd in (False, True)}
        for gr, _ in graphs.values():
            window(gr, a.iters)
        nbytes = N * C * H * H * 2
        rows = []
        for r in range(a.repeats):
            t = {k: window(gr, a.iters) for k, (gr, _) in graphs.items()}
            nf, tf = t["native", False], t["torch", False]
            nb, tb = t["native", True] - nf, t["torch", True] - tf
            rows.append((nf, tf, nb, tb))
            print(f"C {C:>4} Cr {Cr:>3} {H:>2}x{H:<2} round {r}: forward native {nf:7.1f} torch {tf:7.1f} | backward "
                  f"native {nb:7.1f} torch {tb:7.1f} | native GB/s forward {4 * nbytes / nf / 1e3:5.0f} backward "
                  f"{6 * nbytes / nb / 1e3:5.0f}", flush=True)
        lose = [min(x[0] for x in rows) > max(x[1] for x in rows), min(x[2] for x in rows) > max(x[3] for x in rows)]
        print(f"C {C:>4}: native loses in every round: forward {lose[0]}, backward {lose[1]}")


if __name__ == "__main__":
    main()
