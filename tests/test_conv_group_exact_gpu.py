"""csrc/kernels/conv_group.hip through ops/conv_group.py against a float64 CPU reference, EXACTLY.

x, w, dy are uniform in {-1, +1} (tests/_conv_ref.py): every fp32 partial sum is an exact
integer whatever the tile, the order, the pixel split or the zero padding of the
block-diagonal weight, and every expected value is at most INT_EXACT[dtype] (asserted on
the CPU), so the storage is exact too and the comparison is torch.equal.  One missing,
duplicated or misplaced term moves an output by at least 1.

Shapes: C = 64 (two channel blocks; at Cg = 32 two groups) for every Cg, C = 128 / Cg = 4
(the model's first stage); (2, 7, 7) an image below one tile and two images, (2, 13, 9) odd
and non-square, (1, 19, 35) past the 8 x 16 tile both ways by a non-multiple (and 9 / 4 / 2
pixel splits of the weight gradient at Cg = 4 / 8 / 16).  (1024, 7, 7) in fp16 is the smallest batch at
which a workgroup walks more than one tile (2048 tile-blocks; fp16 because its weight-gradient
sums of 50,176 terms pass 256).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from . import _conv_ref as R

pytestmark = pytest.mark.gpu
CL = torch.channels_last
SHAPES = [(2, 7, 7), (2, 13, 9), (1, 19, 35)]
ROWS = ([("bf16", 64, cg) for cg in (4, 8, 16, 32)] + [("bf16", 128, 4), ("f16", 64, 4), ("f16", 64, 32)])
CASES = [(dt, C, cg, nhw, s) for dt, C, cg in ROWS for nhw in SHAPES for s in (1, 2)]
CASES += [("f16", 64, 16, (1024, 7, 7), s) for s in (1, 2)]


@functools.lru_cache(maxsize=None)
def _case(dt, C, cg, nhw, stride):
    """float64 inputs and expected y, dx, dw of a case (shared by the three tests; not modified)."""
    N, H, W = nhw
    g = R.gen("conv_group", dt, C, cg, nhw, stride)
    x = R.ints((N, C, H, W), (-1, 1), g).requires_grad_()
    w = R.ints((C, cg, 3, 3), (-1, 1), g).requires_grad_()
    y = F.conv2d(x, w, None, stride, 1, 1, C // cg)
    dy = R.ints(tuple(y.shape), (-1, 1), g)
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    for t in (y.detach(), dx, dw):
        assert float(t.abs().max()) <= R.INT_EXACT[dt], (float(t.abs().max()), R.INT_EXACT[dt])
    return x.detach(), w.detach(), dy, y.detach(), dx, dw


def _run(case):
    from ddp_practice_amd.ops import conv_group as G

    dt, C, cg, nhw, stride = case
    x64, w64, dy64, y64, dx64, dw64 = _case(*case)
    assert SHAPES[2][1:] == tuple(2 * t + 3 for t in G.tile())  # past the tile both ways by a non-multiple
    x = x64.to(R.DT[dt]).cuda().contiguous(memory_format=CL).requires_grad_()
    w = w64.float().cuda().requires_grad_()
    G.clear_launches()
    y = G.conv_group(x, w, stride, C // cg, R.DT[dt])
    dy = dy64.to(R.DT[dt]).cuda().contiguous(memory_format=CL)
    dx, dw = torch.autograd.grad(y, (x, w), dy, retain_graph=True)
    dw2 = torch.autograd.grad(y, w, dy)[0]  # (the node's x needs a gradient: both gradients run again)
    want = {"fwd": ([stride, cg], dt, 1), "dgrad": ([stride, cg], dt, 2), "wgrad": ([stride, cg], dt, 2)}
    assert G.last_launch() == want, (G.last_launch(), want)
    return (y, dx, dw, dw2), (y64, dx64, dw64)


def _ids(c):
    return f"{c[0]}-C{c[1]}-cg{c[2]}-{'x'.join(map(str, c[3]))}-s{c[4]}"


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
