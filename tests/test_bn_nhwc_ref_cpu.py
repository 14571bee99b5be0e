"""tests/_bn_ref.py is itself right: it equals nn.BatchNorm2d in float64 (forward, running
statistics, autograd gradients), its integer generators give exactly representable sums, and
the float cases of tests/test_bn_nhwc_exact_gpu.py stay inside the skip allowance."""
import copy
import itertools

import pytest
import torch

from . import _bn_ref as R

N, C, H, W = 3, 5, 7, 9
M = N * H * W


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _nchw(rows):
    return rows.reshape(N, H, W, -1).permute(0, 3, 1, 2)


def _bn(momentum, seed):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm2d(C, momentum=momentum).double()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=g, dtype=torch.float64))
        bn.bias.copy_(torch.randn(C, generator=g, dtype=torch.float64))
        bn.running_mean.copy_(torch.randn(C, generator=g, dtype=torch.float64))
        bn.running_var.copy_(torch.rand(C, generator=g, dtype=torch.float64) + 0.5)
    return bn


def _close(a, b):
    assert torch.allclose(a, b, rtol=1e-11, atol=1e-11), (a - b).abs().max().item()


@pytest.mark.parametrize("momentum", [0.1, None])
@pytest.mark.parametrize("res,relu", list(itertools.product([False, True], [False, True])))
def test_train_matches_batchnorm2d(res, relu, momentum):
    g = torch.Generator().manual_seed(3)
    bn = _bn(momentum, 4)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    gamma, beta = bn.weight.detach().clone(), bn.bias.detach().clone()
    for it in range(2):
        x = (torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 1.5 + 0.7).requires_grad_()
        r = torch.randn(N, C, H, W, generator=g, dtype=torch.float64).requires_grad_() if res else None
        dy = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
        y = bn(x) + (r if res else 0)
        y = y.relu() if relu else y
        bn.zero_grad()
        y.backward(dy)

        xr, rr, dyr = _rows(x.detach()), (_rows(r.detach()) if res else None), _rows(dy)
        s1, s2, n = R.fwd_sums(xr, rm)  # the kernels sum around the running mean
        mean, var, invstd = R.moments_from_sums(s1, s2, n, rm, bn.eps)
        mean2, var2, invstd2 = R.batch_moments(xr, bn.eps)
        _close(mean, mean2), _close(var, var2), _close(invstd, invstd2)
        rm, rv = R.running_update(rm, rv, mean, var, n, momentum, it + 1)
        _close(rm, bn.running_mean), _close(rv, bn.running_var)
        assert int(bn.num_batches_tracked) == it + 1
        yr, pre, A = R.bn_y(xr, mean, invstd, gamma, beta, rr, relu)
        _close(_nchw(yr), y.detach())
        assert (A >= pre.abs() - 1e-12).all()
        # act 1: mask from the stored y (a residual was added); act 2: from the pre-activation
        act = (1 if res else 2) if relu else 0
        b = R.bn_bwd(dyr, xr, mean, invstd, gamma, R.relu_mask(act, y=yr, pre=pre))
        _close(_nchw(b["dx"]), x.grad)
        _close(b["dgamma"], bn.weight.grad), _close(b["dbeta"], bn.bias.grad)
        if res:
            _close(_nchw(b["dres"]), r.grad)
        dx2, A2 = R.bn_dx(b["dz"], xr, mean, invstd, gamma, b["S1"], b["S2"], n)
        assert torch.equal(dx2, b["dx"]) and (A2 >= dx2.abs() - 1e-12).all()


def test_eval_matches_batchnorm2d():
    g = torch.Generator().manual_seed(5)
    bn = _bn(0.1, 6).eval()
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    r = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    invstd = (bn.running_var + bn.eps).rsqrt()
    for res, relu in itertools.product([False, True], [False, True]):
        y = bn(x) + (r if res else 0)
        y = y.relu() if relu else y
        yr, _, _ = R.bn_y(_rows(x), bn.running_mean, invstd, bn.weight.detach(), bn.bias.detach(),
                          _rows(r) if res else None, relu)
        _close(_nchw(yr), y.detach())


@pytest.mark.parametrize("train", [True, False])
def test_tail_matches_two_batchnorms(train):
    g = torch.Generator().manual_seed(7)
    bn, rbn = _bn(0.1, 8), _bn(None, 9)
    ref, rref = copy.deepcopy(bn), copy.deepcopy(rbn)
    if not train:
        bn.eval(), rbn.eval()
    x = (torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 2 - 0.4).requires_grad_()
    r = (torch.randn(N, C, H, W, generator=g, dtype=torch.float64) + 0.3).requires_grad_()
    dy = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    y = (bn(x) + rbn(r)).relu()
    xr, rr = _rows(x.detach()), _rows(r.detach())
    if train:
        mean, var, invstd = R.batch_moments(xr, bn.eps)
        rmean, rvar, rinvstd = R.batch_moments(rr, rbn.eps)
        a, b = R.running_update(ref.running_mean, ref.running_var, mean, var, M, 0.1, 1)
        _close(a, bn.running_mean), _close(b, bn.running_var)
        a, b = R.running_update(rref.running_mean, rref.running_var, rmean, rvar, M, None, 1)
        _close(a, rbn.running_mean), _close(b, rbn.running_var)
    else:
        mean, invstd = bn.running_mean, (bn.running_var + bn.eps).rsqrt()
        rmean, rinvstd = rbn.running_mean, (rbn.running_var + rbn.eps).rsqrt()
    ga, be, rga, rbe = (t.detach() for t in (bn.weight, bn.bias, rbn.weight, rbn.bias))
    yr, pre, A = R.tail_fwd(xr, rr, mean, invstd, ga, be, rmean, rinvstd, rga, rbe)
    _close(_nchw(yr), y.detach())
    assert (A >= pre.abs() - 1e-12).all()
    if train:
        y.backward(dy)
        main, side = R.tail_bwd(_rows(dy), yr, xr, rr, mean, invstd, ga, rmean, rinvstd, rga)
        _close(_nchw(main["dx"]), x.grad), _close(_nchw(side["dx"]), r.grad)
        _close(main["dgamma"], bn.weight.grad), _close(main["dbeta"], bn.bias.grad)
        _close(side["dgamma"], rbn.weight.grad), _close(side["dbeta"], rbn.bias.grad)


LARGEST_M = 38400  # the 300-row-block bf16 case of the GPU module


@pytest.mark.parametrize("Mi,Ci", [(2, 8), (189, 24), (1025, 72), (LARGEST_M, 64)])
def test_integer_generators_are_exact(Mi, Ci):
    x, dy = R.int_rows(Mi, Ci, 1), R.int_rows(Mi, Ci, 2)
    y = R.int_rows(Mi, Ci, 3).clamp(min=0)
    shift, save = R.int_shift(Ci, 4), R.int_save(Ci, 5)
    gamma, beta = R.int_affine(Ci, 6)
    assert x.abs().max() <= 3 and shift.abs().max() <= 2 and save[:Ci].abs().max() <= 2
    assert set(save[Ci:].tolist()) <= {0.25, 0.5} and gamma.abs().max() <= 2 and (beta * 2 == (beta * 2).round()).all()
    for dt in R.Q:  # every value survives the storage types
        for t in (x, dy, y):
            assert torch.equal(R.rounded(t, dt), t)
    assert 30 * LARGEST_M < 2 ** 24  # 25 M (forward) and 4 * 7.5 M (backward) stay fp32 integers
    s1, s2, n = R.fwd_sums(x, shift)
    i1, i2 = R.int_fwd_sums(x, shift)
    assert n == Mi and torch.equal(s1, i1.double()) and torch.equal(s2, i2.double())
    assert torch.equal(s2.float().double(), s2) and torch.equal(s1.float().double(), s1)
    mean, invstd = save[:Ci], save[Ci:]
    _, pre, _ = R.bn_y(x, mean, invstd, gamma, beta)
    assert torch.equal(pre * 8, (pre * 8).round())  # the recomputed mask's argument is exact
    if Mi > 100:
        assert (pre == 0).any()  # ... and hits the threshold: y > 0 is false there
    for act in (0, 1, 2):
        mask = R.relu_mask(act, y=y, pre=pre)
        b = R.bn_bwd(dy, x, mean, invstd, gamma, mask)
        S1, S2x4 = R.int_bwd_sums(dy, x, save, mask)
        assert torch.equal(b["S1"], S1.double()) and torch.equal(b["S2"] * 4, S2x4.double())
        assert torch.equal(b["S2"].float().double(), b["S2"])
        if act == 2:
            assert (b["dz"][pre == 0] == 0).all()


def test_distinct_rows_leave_no_constant_channel():
    for seed in range(20):
        x = R.int_rows(2, 64, seed, distinct=True)
        assert (x[0] != x[1]).all() and x.abs().max() <= 3


def test_float_rows_have_the_requested_moments():
    delta, sigma = torch.tensor([0.0, 4.0, -32.0]), torch.tensor([1.0, 0.5, 2.0])
    for Mi in (2, 189):
        x = R.float_rows(Mi, 3, 11, delta.double(), sigma.double())
        mean, var, _ = R.batch_moments(x)
        _close(mean, delta.double()), _close(var.sqrt(), sigma.double())


def test_one_row_block_cases_walk_a_pass_and_a_tail():
    """The one-row-block cases of the GPU module: one row block per chunk at M = 189 under
    targets (1, 1, 1); every active lane makes at least one pass of U rows and some lane then
    walks a tail row -- except the listed tail-only case, whose dtype another case covers."""
    Mi = R.ELEM_ROWS[0]
    full = [c for c in R.ONE_BLOCK_CASES + R.ONE_BLOCK_EXTRA if c not in R.ONE_BLOCK_TAIL_ONLY]
    assert set(R.ONE_BLOCK_TAIL_ONLY) <= set(R.ONE_BLOCK_CASES)
    assert {dt for dt, _ in full} == set(R.Q)  # every dtype has a pass + tail case
    for dt, Ci in R.ONE_BLOCK_CASES + R.ONE_BLOCK_EXTRA:
        assert (dt, Ci) in R.elem_cases()
        gr, gc, rp, rows, active = R.geom(Mi, Ci, 1, dt, cc=256)
        assert gr == 1 and rows == Mi and active <= R.THR
        walk = R.lane_walk(rows, rp, R.U)
        if (dt, Ci) in R.ONE_BLOCK_TAIL_ONLY:
            assert all(p == 0 and t >= 1 for p, t in walk), (dt, Ci, walk)
        else:
            assert all(p >= 1 for p, _ in walk) and any(t >= 1 for _, t in walk), (dt, Ci, walk)
        # under the default targets no lane does both (the gap these cases close)
        gr, _, rp, rows, _ = R.geom(Mi, Ci, 1024, dt, cc=256)
        assert not any(p >= 1 and t >= 1 for p, t in R.lane_walk(rows, rp, R.U))
    # hand counts: bf16 C = 72 is 9 lanes per row, RP = 28, 4 idle lanes; C = 320 five chunks of 64
    assert R.geom(Mi, 72, 1, torch.bfloat16, cc=256)[1:] == (1, 28, Mi, 252)
    assert R.geom(Mi, 320, 1, torch.bfloat16, cc=256)[1:] == (5, 32, Mi, 256)


def test_statistics_cases_walk_a_pass_and_a_tail():
    """Section a of the GPU module already holds a one-row-block case in which a lane makes a pass
    (UF = 8 rows forward, U = 4 backward) and then walks a tail row: fp32, C = 64, M = 189 at
    target 1 (RP = 16)."""
    dt, Ci, Mi = R.STATS_ONE_BLOCK
    gr, gc, rp, rows, _ = R.geom(Mi, Ci, 1, dt)
    assert (gr, gc, rp, rows) == (1, 1, 16, Mi)
    for u in (R.UF, R.U):
        assert any(p >= 1 and t >= 1 for p, t in R.lane_walk(rows, rp, u)), u


@pytest.mark.parametrize("dtype,Ci", R.elem_cases(), ids=lambda v: str(v).replace("torch.", ""))
def test_float_cases_stay_inside_the_skip_allowance(dtype, Ci):
    """The GPU module may skip, per case, at most skip_allowance(numel) elements whose float64
    pre-activation lies within 16 u A of 0: 1 in 1000 (none at all in the 2-row cases).  The
    reference inputs alone must stay far inside it (here: at most a tenth of it, and 0 below
    10,000 elements), and the integer inputs have nothing to skip."""
    for Mi in R.ELEM_ROWS:
        t = R.elem_inputs("float", Mi, Ci, dtype, R.elem_seed(dtype, Ci, Mi))
        _, pre, A = R.bn_y(t["x"], t["save"][:Ci], t["save"][Ci:], t["gamma"], t["beta"])
        near = int(R.near_zero(pre, A).sum())
        allowed = R.skip_allowance(pre.numel())
        assert allowed == pre.numel() // 1000
        assert near <= allowed // 10, (Mi, near, allowed)
        # the generator's promises behind the y bound (see _bn_ref's docstring)
        mean, var, _ = R.batch_moments(t["x"])
        assert (mean.abs() <= 0.26 * var.sqrt()).all()
        assert (t["beta"].abs() >= 0.25 - 1e-6).all() and (t["gamma"].abs() <= 1.5 + 1e-6).all()
        assert (t["gamma"] == 0).any() and (t["gamma"] < 0).any()
