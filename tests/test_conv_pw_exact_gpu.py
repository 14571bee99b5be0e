"""csrc/kernels/conv_pw.hip through ops/conv_pw.py against a float64 CPU reference.

Exact tests: x, w, dy are uniform in {-1, +1} (tests/_conv_ref.py), so every fp32 partial sum
is an exact integer whatever the tile, the order or the pixel split, and every expected |y| and
|dx| is at most INT_EXACT[dtype] (asserted on the CPU; C, K <= 256 in bf16): torch.equal.

(C, K): (8, 8) one granule, three of four K-blocks zero, half a channel tile masked; (24, 40)
Kc % 32 = 24 and Nc % 16 = 8 forward, Kc % 32 = 8 and Nc % 16 = 8 in the data gradient; (32, 64)
MobileNetV1's; (72, 136) a full 64-block plus a one-granule remainder on both sides; (200, 96)
several K-steps with a tail (one channel block of pw_kernel both ways, two 64-blocks only in the
weight gradient); (256, 120) more than one channel block in the single-stage regime both ways with
a ragged last block (forward 112 + 8, data gradient 224 + 32: asserted from channel_block());
fp16 only (2 * chunk + 8, chunk + 8) = (520, 264): both cross the 256-deep weight-staging chunk
(the chunked regime, last chunk of one granule, five and nine 64-channel blocks).
(N, H, W): one pixel; (2, 7, 7) under one tile; (1, 2 * T + 3, 1) two full tiles and a ragged one;
BIG at (72, 136) in fp16: 2047 * T + 1 pixels, the smallest P with 2048 tiles, which is where one
channel block's workgroups walk two tiles (2048 * 1 / 1024); the weight gradient is split there too.

Rounding test: standard normal x, w, dy already rounded to the compute dtype; per element against
float64: one storage rounding (u = 2^-8 bf16, 2^-11 fp16) plus fp32 accumulation of the T terms
(C, K, P for y, dx, dw), T * 2^-23 * sum |a||b|; the fp32 weight gradient has no storage term.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from . import _conv_ref as R

pytestmark = pytest.mark.gpu
CL = torch.channels_last
T, NB = 128, 64  # asserted against conv_pw.tile()
KCH = 256  # asserted against conv_pw.chunk()
BIG = (1, 2047 * T + 1, 1)
SHAPES = [(1, 1, 1), (2, 7, 7), (1, 2 * T + 3, 1)]
PAIRS = ((8, 8), (24, 40), (32, 64), (72, 136), (200, 96), (256, 120))
CASES = [(dt, ck, nhw) for dt in ("bf16", "f16") for ck in PAIRS for nhw in SHAPES]
CASES += [("f16", (2 * KCH + 8, KCH + 8), nhw) for nhw in SHAPES] + [("f16", (72, 136), BIG)]
U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}


@functools.lru_cache(maxsize=None)
def _case(dt, ck, nhw, normal=False):
    """float64 inputs and expected y, dx, dw of a case (shared by the tests; not modified)."""
    (C, K), (N, H, W) = ck, nhw
    g = R.gen("conv_pw", dt, ck, nhw, normal)
    if normal:
        draw = lambda *shape: torch.randn(*shape, generator=g).to(R.DT[dt]).double()  # noqa: E731
    else:
        draw = lambda *shape: R.ints(shape, (-1, 1), g)  # noqa: E731
    x, w = draw(N, C, H, W).requires_grad_(), draw(K, C, 1, 1).requires_grad_()
    y = F.conv2d(x, w)
    dy = draw(*y.shape)
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    if not normal:
        for t in (y.detach(), dx):
            assert float(t.abs().max()) <= R.INT_EXACT[dt], (float(t.abs().max()), R.INT_EXACT[dt])
        assert float(dw.abs().max()) < R.F32_EXACT
    return x.detach(), w.detach(), dy, y.detach(), dx, dw


def _run(case, normal=False):
    from ddp_practice_amd.ops import conv_pw as G

    dt, (C, K), nhw = case
    x64, w64, dy64, y64, dx64, dw64 = _case(*case, normal)
    assert G.tile() == (T, NB) and G.chunk() == KCH
    if (C, K) == (256, 120):  # two channel blocks both ways, the last one ragged
        assert (G.channel_block(C, K), G.channel_block(K, C)) == (112, 224)
    x = x64.to(R.DT[dt]).cuda().contiguous(memory_format=CL).requires_grad_()
    w = w64.float().cuda().requires_grad_()
    G.clear_launches()
    y = G.conv_pw(x, w, R.DT[dt])
    dy = dy64.to(R.DT[dt]).cuda().contiguous(memory_format=CL)
    dx, dw = torch.autograd.grad(y, (x, w), dy, retain_graph=True)
    dw2 = torch.autograd.grad(y, w, dy)[0]  # (the node's x needs a gradient: both gradients run again)
    want = {"fwd": ([C, K], dt, 1), "dgrad": ([C, K], dt, 2), "wgrad": ([C, K], dt, 2)}
    assert G.last_launch() == want, (G.last_launch(), want)
    P = nhw[0] * nhw[1] * nhw[2]
    if nhw == BIG:
        assert G.tiles_per_workgroup(P, C, K) == 2 and G.tiles_per_workgroup(P, K, C) == 2
        assert G.tiles_per_workgroup(P - 1, C, K) == 1 and G.wgrad_splits(P, K, C) > 1
    return (y, dx, dw, dw2), (y64, dx64, dw64)


def _ids(c):
    return f"{c[0]}-{c[1][0]}to{c[1][1]}-{'x'.join(map(str, c[2]))}"


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_forward(case):
    (y, _, _, _), (y64, _, _) = _run(case)
    assert y.dtype == R.DT[case[0]] and y.is_contiguous(memory_format=CL)
    assert torch.equal(y.detach().double().cpu(), y64)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_data_gradient(case):
    (_, dx, _, _), (_, dx64, _) = _run(case)
    assert dx.dtype == R.DT[case[0]] and dx.is_contiguous(memory_format=CL)
    assert torch.equal(dx.double().cpu(), dx64)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_weight_gradient(case):
    (_, _, dw, dw2), (_, _, dw64) = _run(case)
    assert dw.dtype == torch.float32 and dw.is_contiguous() and dw.shape == dw64.shape  # fp32 OIHW
    assert torch.equal(dw.double().cpu(), dw64)
    assert torch.equal(dw, dw2)  # the fixed-order reduction: the same bits on the same inputs


@pytest.mark.parametrize("case", [(dt, (72, 136), (2, 13, 9)) for dt in ("bf16", "f16")], ids=_ids)
def test_rounding(case):
    dt, (C, K), (N, H, W) = case
    (y, dx, dw, _), (y64, dx64, dw64) = _run(case, True)
    x64, w64, dy64 = _case(*case, True)[:3]
    xa, wa = x64.abs().requires_grad_(), w64.abs().requires_grad_()
    absy = F.conv2d(xa, wa)  # sum |x||w| per output
    absdx, absdw = torch.autograd.grad(absy, (xa, wa), dy64.abs())
    e = 2.0 ** -23
    for name, got, ref, bound in (("y", y.detach(), y64, U[dt] * y64.abs() + C * e * absy.detach()),
                                  ("dx", dx, dx64, U[dt] * dx64.abs() + K * e * absdx),
                                  ("dw", dw, dw64, N * H * W * e * absdw)):
        err = (got.double().cpu() - ref).abs()
        print(f"{name}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), name
