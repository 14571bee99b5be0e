"""tests/_conv_ref.py (the float64 reference of the exact implicit-GEMM tests) against
independent formulations, and the exactness conditions of EVERY case of
tests/_conv_cases.py -- all on the CPU."""
import itertools

import pytest
import torch

from . import _conv_cases as T
from . import _conv_ref as R

D = torch.float64


def _taps(x, w, stride, pad):
    """y = sum over (r, s) of einsum(x shifted by the tap, w[:, :, r, s]): explicit tap loop."""
    N, C, H, W = x.shape
    K, _, Rr, S = w.shape
    OH, OW = (H + 2 * pad - Rr) // stride + 1, (W + 2 * pad - S) // stride + 1
    xp = torch.zeros(N, C, H + 2 * pad, W + 2 * pad, dtype=D)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    y = torch.zeros(N, K, OH, OW, dtype=D)
    for r, s in itertools.product(range(Rr), range(S)):
        win = xp[:, :, r:r + (OH - 1) * stride + 1:stride, s:s + (OW - 1) * stride + 1:stride]
        y += torch.einsum("nchw,kc->nkhw", win, w[:, :, r, s])
    return y


def _taps_dgrad(dy, w, x_shape, stride, pad):
    N, C, H, W = x_shape
    K, _, Rr, S = w.shape
    OH, OW = dy.shape[2:]
    dxp = torch.zeros(N, C, H + 2 * pad, W + 2 * pad, dtype=D)
    for r, s in itertools.product(range(Rr), range(S)):
        dxp[:, :, r:r + (OH - 1) * stride + 1:stride, s:s + (OW - 1) * stride + 1:stride] += torch.einsum(
            "nkhw,kc->nchw", dy, w[:, :, r, s])
    return dxp[:, :, pad:pad + H, pad:pad + W]


def _taps_wgrad(dy, x, wshape, stride, pad):
    N, C, H, W = x.shape
    K, _, Rr, S = wshape
    OH, OW = dy.shape[2:]
    xp = torch.zeros(N, C, H + 2 * pad, W + 2 * pad, dtype=D)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    dw = torch.zeros(wshape, dtype=D)
    for r, s in itertools.product(range(Rr), range(S)):
        win = xp[:, :, r:r + (OH - 1) * stride + 1:stride, s:s + (OW - 1) * stride + 1:stride]
        dw[:, :, r, s] = torch.einsum("nkhw,nchw->kc", dy, win)
    return dw


@pytest.mark.parametrize("Rr,stride,pad", [(1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1), (3, 1, 0), (5, 1, 2), (5, 2, 3),
                                           (7, 2, 3), (3, 2, 2)])
def test_reference_matches_tap_loops(Rr, stride, pad):
    g = R.gen("taps", Rr, stride, pad)
    N, C, H, W, K = 2, 3, 9, 12, 4
    x, w = R.ints((N, C, H, W), (-3, -2, -1, 1, 2, 3), g), R.ints((K, C, Rr, Rr), (-2, -1, 1, 2), g)
    y = R.conv(x, w, stride, pad)
    assert y.shape[2:] == R.out_hw(H, W, Rr, stride, pad) and y.shape[2] != y.shape[3]
    assert torch.equal(y, _taps(x, w, stride, pad))
    dy = R.ints(y.shape, (-1, 1), g)
    assert torch.equal(R.dgrad(dy, w, x.shape, stride, pad), _taps_dgrad(dy, w, x.shape, stride, pad))
    assert torch.equal(R.wgrad(dy, x, w.shape, stride, pad), _taps_wgrad(dy, x, w.shape, stride, pad))
    if stride == 1 and Rr - 1 - pad >= 0:
        assert torch.equal(R.dgrad_s1(dy, w, pad), _taps_dgrad(dy, w, x.shape, 1, pad))


def test_s2t_reference_matches_parity_decomposition():
    """conv_igemm.h MODE_S2T: dx of a 3x3 / stride-2 / pad-1 conv split by output parity
    (py, px) into four stride-1 sub-convolutions of dy with 1, 2, 2 and 4 of the taps."""
    g = R.gen("s2t")
    N, Cin, OH, OW, K = 2, 3, 4, 6, 5
    dy, w = R.ints((N, K, OH, OW), (-2, -1, 1, 2), g), R.ints((K, Cin, 3, 3), (-3, -1, 1, 2), g)
    dyp = torch.zeros(N, K, OH + 1, OW + 1, dtype=D)  # dy rows / columns past the end read zero
    dyp[:, :, :OH, :OW] = dy
    dx = torch.zeros(N, Cin, 2 * OH, 2 * OW, dtype=D)
    ntaps = []
    for py, px in itertools.product((0, 1), (0, 1)):
        rows = [(1, 0)] if py == 0 else [(0, 1), (2, 0)]  # (forward-filter tap r, dy row offset)
        cols = [(1, 0)] if px == 0 else [(0, 1), (2, 0)]
        ntaps.append(len(rows) * len(cols))
        for (r, dh), (s, dw) in itertools.product(rows, cols):
            dx[:, :, py::2, px::2] += torch.einsum("nkhw,kc->nchw", dyp[:, :, dh:dh + OH, dw:dw + OW], w[:, :, r, s])
    assert ntaps == [1, 2, 2, 4]
    assert torch.equal(R.dgrad(dy, w, (N, Cin, 2 * OH, 2 * OW), 2, 1), dx)


def test_accumulate_rounds_twice_on_a_tie():
    """bf16: the tile value 257 is stored as 256 (tie to even); + old = 1 gives 257 -> 256
    again, where one rounding of 257 + 1 would give 258.  fp16: the same at 2049."""
    for dtype, base in (("bf16", 257.0), ("f16", 2049.0)):
        y64 = torch.full((1, 1, 2, 2), base, dtype=D)
        old = torch.ones(1, 1, 2, 2, dtype=D)
        assert R.store(y64, dtype).double().unique().tolist() == [base - 1]
        assert R.store_acc(y64, dtype, old).double().unique().tolist() == [base - 1]
        assert R.store(y64 + old, dtype).double().unique().tolist() == [base + 1]
        aux = torch.ones(1, 1, 1, 1, dtype=D)
        got = R.store_acc(y64, dtype, None, aux).double()
        assert got[0, 0, 0, 0] == base - 1 and got[0, 0, 1, 1] == base - 1  # (257 -> 256, + 1 -> 256)
        # 259 -> 260 (tie to even); + old = 261 -> 260 (tie) at the other pixels, + old + aux = 262 at
        # the even pixel, where one rounding of 259 + 2 = 261 would give 260
        got = R.store_acc(y64 + 2, dtype, old, aux).double()
        assert got[0, 0, 0, 1] == base + 3 and got[0, 0, 0, 0] == base + 5
        assert R.store(y64 + 2 + 2, dtype).double()[0, 0, 0, 0] == base + 3


def test_statistics_reference_matches_batchnorm():
    g = R.gen("stats")
    y = R.ints((3, 5, 4, 7), (-9, -4, -1, 2, 3, 8), g)
    shift = R.ints((5,), (-2, -1, 1, 2), g)
    st = R.stats(y, shift)
    M = 3 * 4 * 7
    assert st[10] == M
    bn = torch.nn.BatchNorm2d(5, momentum=1.0).double().train()
    bn(y)
    mean = shift + st[:5] / M
    var = st[5:10] / M - (st[:5] / M) ** 2
    torch.testing.assert_close(mean, bn.running_mean, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(var * M / (M - 1), bn.running_var, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("act", [1, 2])
def test_bn_sum_reference_matches_batchnorm_autograd(act):
    g = R.gen("bnsums", act)
    N, Cc, H, W = 3, 4, 5, 6
    x = R.ints((N, Cc, H, W), (-3, -2, -1, 1, 2, 3), g)
    dx = R.ints((N, Cc, H, W), (-5, -2, 1, 3), g)
    res = R.ints((N, Cc, H, W), (-1, 1), g) * 0.5
    bn = torch.nn.BatchNorm2d(Cc).double().train()
    with torch.no_grad():
        bn.weight.copy_(R.ints((Cc,), (-2, -1, 1, 2), g))
        bn.bias.copy_(R.ints((Cc,), (-3, -1, 1, 3), g) * 0.25)
    out = torch.relu(bn(x) + res) if act == 1 else torch.relu(bn(x))
    out.backward(dx)
    mean = x.mean((0, 2, 3))
    invstd = (x.var((0, 2, 3), unbiased=False) + bn.eps).rsqrt()
    mask = R.bn_mask(act, x, out.detach(), mean, invstd, bn.weight.detach(), bn.bias.detach())
    assert torch.equal(mask, out.detach() > 0)
    s1, s2, s2abs = R.bn_sums(dx, mask, x, mean, invstd)
    torch.testing.assert_close(s1, bn.bias.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(s2, bn.weight.grad, rtol=1e-12, atol=1e-12)
    assert (s2abs >= s2.abs() - 1e-9).all()


def test_case_table_is_well_formed():
    names = [c.name for c in T.CASES]
    assert len(set(names)) == len(names)
    ops = {c.op for c in T.CASES}
    assert ops == {"fwd", "fwd+stats", "acc", "aux", "s2t", "stem", "dgrad_bn", "wgrad", "wgrad_batch"}
    for c in T.CASES:
        assert c.dtype in R.DT and c.regime in ("small", "small2", "large")
        if c.op in ("fwd", "fwd+stats", "acc", "aux", "wgrad"):  # non-square input and output
            N, C, H, W, K, Rr, stride, pad = c.shape
            assert H != W and len(set(R.out_hw(H, W, Rr, stride, pad))) == 2 or H == W == 56, c.name
        if c.op == "wgrad":
            assert c.splits is not None
    # fp16 at least once per kernel template and loader mode; the large regime per op
    f16 = {(f, v) for c in T.CASES if c.dtype == "f16" for f, v in c.expect}
    assert {m for f, v in f16 if f == "fwd" for m in v[1:]} == {T.GEN, T.STEM, T.S2T}
    assert {(v[2], v[3]) for f, v in f16 if f == "glds"} >= {(0, 0), (0, 1), (T.BS_Y, 0), (T.BS_REC, 0), (T.BS_REC, 1)}
    assert {v[4] for f, v in f16 if f == "wgrad_glds"} == {0, 1}
    f16w = {c.extra["wgrad"][1][2] for c in T.CASES if c.dtype == "f16" and "wgrad" in c.extra}
    assert f16w == {T.STEM} and any(f == "wgrad" and v[2] == T.GEN for f, v in f16)
    large = {(c.op, c.shape[5] if c.op == "fwd" else 0, c.dtype) for c in T.CASES if c.regime == "large"}
    for dt in R.DT:
        assert large >= {("fwd", 3, dt), ("fwd", 1, dt), ("acc", 0, dt), ("aux", 0, dt), ("s2t", 0, dt)}


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_case_is_exact(name):
    """The conditions under which the case's expected output is known bit for bit."""
    case = T.BY_NAME[name]
    inp, exp, pre = R.build(case)
    R.check_preconditions(case, pre)
    if "single_rounding_differs" in (exp if isinstance(exp, dict) else {}):
        print(f"{name}: one rounding instead of two would change {100 * exp['single_rounding_differs']:.3f} % of "
              f"the outputs")
