"""csrc/kernels/conv_dw5.hip through ops/conv_dw.py against a float64 CPU reference; the method
of tests/test_conv_dw_exact_gpu.py.

Exact tests: x, w, dy are uniform in {-1, +1} (tests/_conv_ref.py), so |y| <= 25, |dx| <= 25 and
|dw| <= N * OH * OW < 2^24 (asserted on the CPU): every fp32 partial sum is an exact integer
whatever the tile, the order or the pixel split, and the comparison is torch.equal.

Shapes: the channel block is 64, so C = 8 (one granule = two half-granule threads), 72 (a full
block plus a one-granule remainder), 128 (two blocks); (1, 1, 1) and (1, 3, 2) smaller than the
filter (nearly every tap is padding), (2, 7, 7) below one tile with two images, (2, 13, 9) odd and
non-square, 2 * tile + 3 per side.  (1024, 7, 7) at C = 72 in fp16: one tile per image and two
channel blocks, so 2048 tile-blocks, the fewest at which tile_grid gives a workgroup two tiles; the
weight gradient then takes 512 splits of two tiles.

Rounding test: standard normal x, w, dy already rounded to the compute dtype; per element against
float64, one storage rounding (u = 2^-8 bf16, 2^-11 fp16) plus fp32 accumulation of the T terms,
T * 2^-23 * sum |a||b|; the fp32 weight gradient has no storage term.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from . import _conv_ref as R

pytestmark = pytest.mark.gpu
CL = torch.channels_last
TILES = {1: (8, 16), 2: (8, 8)}  # asserted against conv_dw.tile(stride, 5)
BIG = (1024, 7, 7)


def _shapes(s):
    return [(1, 1, 1), (1, 3, 2), (2, 7, 7), (2, 13, 9), (1,) + tuple(2 * t + 3 for t in TILES[s])]


CASES = [(dt, C, nhw, s) for dt in ("bf16", "f16") for C in (8, 72, 128) for s in (1, 2) for nhw in _shapes(s)]
CASES += [("f16", 72, BIG, s) for s in (1, 2)]
U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}


@functools.lru_cache(maxsize=None)
def _case(dt, C, nhw, stride, normal=False):
    """float64 inputs and expected y, dx, dw of a case (shared by the tests; not modified)."""
    N, H, W = nhw
    g = R.gen("conv_dw5", dt, C, nhw, stride, normal)
    if normal:
        draw = lambda *shape: torch.randn(*shape, generator=g).to(R.DT[dt]).double()  # noqa: E731
    else:
        draw = lambda *shape: R.ints(shape, (-1, 1), g)  # noqa: E731
    x, w = draw(N, C, H, W).requires_grad_(), draw(C, 1, 5, 5).requires_grad_()
    y = F.conv2d(x, w, None, stride, 2, 1, C)
    dy = draw(*y.shape)
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    if not normal:
        assert float(y.detach().abs().max()) <= 25 <= R.INT_EXACT[dt] and float(dx.abs().max()) <= 25
        assert float(dw.abs().max()) <= N * y.shape[2] * y.shape[3] < R.F32_EXACT
    return x.detach(), w.detach(), dy, y.detach(), dx, dw


def _run(case, normal=False):
    from ddp_practice_amd.ops import conv_dw as G

    dt, C, nhw, stride = case
    x64, w64, dy64, y64, dx64, dw64 = _case(*case, normal)
    assert G.tile(stride, 5) == TILES[stride]
    x = x64.to(R.DT[dt]).cuda().contiguous(memory_format=CL).requires_grad_()
    w = w64.float().cuda().requires_grad_()
    G.clear_launches()
    y = G.conv_dw(x, w, stride, R.DT[dt])
    dy = dy64.to(R.DT[dt]).cuda().contiguous(memory_format=CL)
    dx, dw = torch.autograd.grad(y, (x, w), dy, retain_graph=True)
    dw2 = torch.autograd.grad(y, w, dy)[0]  # (the node's x needs a gradient: both gradients run again)
    want = {"fwd5": ([stride, C], dt, 1), "dgrad5": ([stride, C], dt, 2), "wgrad5": ([stride, C], dt, 2)}
    assert G.last_launch() == want, (G.last_launch(), want)  # (and no 3x3 family)
    if nhw == BIG:
        assert G.wgrad_splits(nhw[0], y.shape[2], y.shape[3], C, stride, 5) == 512
    return (y, dx, dw, dw2), (y64, dx64, dw64)


def _ids(c):
    return f"{c[0]}-C{c[1]}-{'x'.join(map(str, c[2]))}-s{c[3]}"


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


@pytest.mark.parametrize("case", [(dt, 72, (2, 13, 9), s) for dt in ("bf16", "f16") for s in (1, 2)], ids=_ids)
def test_rounding(case):
    dt, C, _, stride = case
    (y, dx, dw, _), (y64, dx64, dw64) = _run(case, True)
    x64, w64, dy64 = _case(*case, True)[:3]
    absy = F.conv2d(x64.abs(), w64.abs(), None, stride, 2, 1, C)  # sum |x||w| per output
    xa = x64.abs().requires_grad_()
    wa = w64.abs().requires_grad_()
    absdx, absdw = torch.autograd.grad(F.conv2d(xa, wa, None, stride, 2, 1, C), (xa, wa), dy64.abs())
    terms = dy64.shape[0] * dy64.shape[2] * dy64.shape[3]
    for name, got, ref, bound in (("y", y.detach(), y64, U[dt] * y64.abs() + 25 * 2.0 ** -23 * absy),
                                  ("dx", dx, dx64, U[dt] * dx64.abs() + 25 * 2.0 ** -23 * absdx),
                                  ("dw", dw, dw64, terms * 2.0 ** -23 * absdw)):
        err = (got.double().cpu() - ref).abs()
        print(f"{name}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), name
