"""tests/_head_ref.py is itself right: in float64 it equals F.linear, F.cross_entropy
(ignore_index, label_smoothing) and the module chain BatchNorm2d(train) -> ReLU ->
MaxPool2d(2) -> flatten -> Linear -> cross_entropy with their autograd gradients; its
generators meet the conditions the exact checks of tests/test_head_exact_gpu.py rest on; and
torch has the edge semantics those tests expect of the kernels."""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from . import _head_ref as R

F64 = torch.float64
DTYPES = list(R.Q)
INF = float("inf")


def _close(a, b, what=""):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs().max().item() if a.numel() else 0.0
    assert err <= 1e-12 * max(1.0, b.abs().max().item() if b.numel() else 0.0), (what, err)


def _exact_in(t, dtype):
    return torch.equal(t.to(dtype).double(), t)


# ------------------------------------------------------------------------------ linear
@pytest.mark.parametrize("bias", [True, False])
def test_linear_matches_torch(bias):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(7, 13, generator=g, dtype=F64).requires_grad_()
    w = torch.randn(5, 13, generator=g, dtype=F64).requires_grad_()
    b = torch.randn(5, generator=g, dtype=F64).requires_grad_() if bias else None
    dout = torch.randn(7, 5, generator=g, dtype=F64)
    out = F.linear(x, w, b)
    out.backward(dout)
    ref, A = R.linear(x.detach(), w.detach(), b.detach() if bias else None)
    _close(ref, out.detach(), "out")
    assert bool((A >= ref.abs() - 1e-12).all())
    dx, dw, db = R.linear_bwd(dout, x.detach(), w.detach())
    _close(dx, x.grad, "dx")
    _close(dw, w.grad, "dw")
    if bias:
        _close(db, b.grad, "db")


@pytest.mark.parametrize("M,N,K", R.LIN_SHAPES)
def test_linear_generator_is_exact(M, N, K):
    t = R.lin_inputs(M, N, K, 7 * M + N)
    for v in t.values():
        assert float(v.abs().max()) <= 3 and torch.equal(v, v.round())
        assert all(_exact_in(v, dt) for dt in DTYPES)
    # every partial sum of every result is an integer bounded by the sum of magnitudes
    worst = max(float(R.linear(t["x"], t["w"], t["b"])[1].max()),
                float((t["dout"].abs() @ t["w"].abs()).max()),
                float((t["dout"].abs().t() @ t["x"].abs()).max()), float(t["dout"].abs().sum(0).max()))
    assert worst < 2 ** 24 and K <= 1056


# ----------------------------------------------------------------------- cross entropy
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("ignored", [0, 3, "all"])
@pytest.mark.parametrize("Bn,N", [(1, 1), (3, 2), (37, 10), (5, 1000)])
def test_cross_entropy_matches_torch(Bn, N, ignored, smoothing):
    lg = R.ce_logits(Bn, N, 11).requires_grad_()
    t = R.ce_targets(Bn, N, 11, ignored)
    seed = 3.0
    loss = F.cross_entropy(lg, t, ignore_index=-100, label_smoothing=smoothing)
    ref, dlog, A_loss, A_dlog = R.cross_entropy(lg.detach(), t, -100, smoothing, scale=seed)
    n_counted = int((t != -100).sum())
    if n_counted == 0:
        assert math.isnan(float(loss.detach())) and math.isnan(float(ref))
        assert not dlog.any()
        return
    (loss * seed).backward()
    _close(ref, loss.detach(), "loss")
    _close(dlog, lg.grad, "dlog * seed")
    assert not dlog[t == -100].any(), "an ignored row's gradient is exactly 0"
    assert A_loss == 1 + float(lg.detach().abs().max())
    assert bool(((A_dlog[0] + A_dlog[1]) >= dlog.abs() - 1e-15).all())


def test_cross_entropy_bad_target_and_inf_column():
    lg = R.ce_logits(6, 5, 3)
    t = R.ce_targets(6, 5, 3)
    good = R.cross_entropy(lg, t, -100, 0.1)
    for bad in (5, -1):
        tb = t.clone()
        tb[2] = bad
        loss, dlog, _, _ = R.cross_entropy(lg, tb, -100, 0.1)
        assert math.isnan(float(loss))
        sm = lg.softmax(1)
        _close(dlog[2], (sm[2] - 0.1 / 5) / 6, "bad row")
        keep = torch.arange(6) != 2
        _close(dlog[keep], good[1][keep], "other rows")
    # a masked class: -inf off the targets.  torch: finite at smoothing 0, inf at smoothing > 0
    t = torch.tensor([0, 1, 3, 0, 1, 3])
    lg[:, 2] = -INF
    for s, want_inf in ((0.0, False), (0.1, True)):
        tl = F.cross_entropy(lg, t, label_smoothing=s)
        loss, dlog, A_loss, _ = R.cross_entropy(lg, t, -100, s)
        assert bool(tl.isinf()) == want_inf and bool(loss.isinf()) == want_inf
        if not want_inf:
            _close(loss, tl, "loss with a -inf column")
        assert bool(tl.isfinite()) != want_inf and math.isfinite(A_loss)
        if s == 0:
            assert not dlog[:, 2].any()


def test_torch_edge_semantics():
    lg = R.ce_logits(4, 3, 5)
    assert math.isnan(float(F.cross_entropy(lg, torch.full((4,), -100))))
    a = torch.tensor([[1.0, 2.0, 2.0, 0.0], [-INF, -INF, -INF, -INF], [0.0, 0.0, 0.0, 0.0]], dtype=F64)
    assert a.argmax(1).tolist() == [1, 0, 0] == R.argmax_first(a).tolist()
    assert R.accuracy(a, torch.tensor([2, 0, 1])) == (3, 1)


@pytest.mark.parametrize("Bn,N", [(1, 1), (64, 17), (5, 1000), (65, 1025), (4099, 3)])
def test_ce_generator(Bn, N):
    lg = R.ce_logits(Bn, N, 100 * Bn + N)
    assert torch.equal(lg * 8, (lg * 8).round()) and float(lg.abs().max()) <= 8
    assert all(_exact_in(lg, dt) for dt in DTYPES)
    assert float((lg.max(1).values - lg.min(1).values).max()) <= R.SPREAD
    t = R.ce_targets(Bn, N, 100 * Bn + N, 3 if Bn > 1 else 0)
    assert bool(((t >= 0) & (t < N) | (t == -100)).all())


@pytest.mark.parametrize("Bn,N", R.ACC_SHAPES)
def test_accuracy_generator(Bn, N):
    lg, t = R.acc_inputs(Bn, N, 10 * Bn + N)
    assert all(_exact_in(lg, dt) for dt in DTYPES)
    first = R.argmax_first(lg)
    assert torch.equal(first, lg.argmax(1))
    rows, hit = R.accuracy(lg, t)
    assert rows == Bn and hit == int((lg.argmax(1) == t).sum())
    if Bn >= 5 and N > 1:
        tied = (lg == lg.max(1, keepdim=True).values).sum(1) > 1
        assert int(tied.sum()) * 2 >= Bn - 1, "most rows tie on the maximum"
        later = (t != first) & (lg.gather(1, t.view(-1, 1)).squeeze(1) == lg.max(1).values)
        assert bool(later.any()), "a target on a later tied maximum"
        assert 0 < hit < Bn
    if Bn > 2:
        assert bool(lg[Bn // 2].isinf().all()) and int(first[Bn // 2]) == 0


# ------------------------------------------------------------------------- ConvNet head
@pytest.mark.parametrize("momentum", [0.1, None])
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_head_chain_matches_modules(momentum, smoothing):
    Bn, N, seed = 3, 10, 3.0
    t = R.head_inputs(Bn, N, R.head_seed(Bn, N), 5)
    bn = torch.nn.BatchNorm2d(R.HC, eps=t["eps"], momentum=momentum).double()
    lin = torch.nn.Linear(R.HK, N).double()
    pool = torch.nn.MaxPool2d(2, return_indices=True)
    with torch.no_grad():
        bn.weight.copy_(t["gamma"]); bn.bias.copy_(t["beta"])
        bn.running_mean.copy_(t["rm0"]); bn.running_var.copy_(t["rv0"])
        lin.weight.copy_(t["wfc"]); lin.bias.copy_(t["bfc"])
    target = R.ce_targets(Bn, N, 5)
    target[1] = -100
    y2 = t["y2"].clone()
    p4, ind = pool(F.relu(bn(y2)))
    p4.retain_grad()
    logits = lin(p4.flatten(1))
    logits.retain_grad()
    loss = F.cross_entropy(logits, target, label_smoothing=smoothing)
    (loss * seed).backward()

    st = R.bn_from_rows(t["rows"], t["shift"], t["gamma"], t["beta"], t["eps"], t["rm0"], t["rv0"], momentum, 1)
    _close(st["mean"], y2.mean((0, 2, 3)), "mean")
    _close(st["var"], y2.var((0, 2, 3), unbiased=False), "var")
    _close(st["rm"], bn.running_mean, "running_mean")
    _close(st["rv"], bn.running_var, "running_var")
    p, idx, xhat, A_p, _ = R.bn_relu_pool(y2, st["mean"], st["invstd"], t["gamma"], t["beta"], F64)
    _close(p, p4.detach().flatten(1), "p")
    assert bool((A_p >= p - 1e-12).all())
    ho = torch.arange(7).view(1, 1, 7, 1)
    wo = torch.arange(7).view(1, 1, 1, 7)
    arg = ((ind // 14 - 2 * ho) * 2 + (ind % 14 - 2 * wo)).flatten(1)
    assert torch.equal((idx & 3).long(), arg), "argmax (first maximum)"
    assert torch.equal((idx & 4) != 0, p > 0)
    lg, _ = R.fc(p, t["wfc"], t["bfc"])
    _close(lg, logits.detach(), "logits")
    ref_loss, dlog, _, _ = R.cross_entropy(lg, target, -100, smoothing, scale=seed)
    _close(ref_loss, loss.detach(), "loss")
    _close(dlog, logits.grad, "dlog * seed")
    hb = R.head_bwd(dlog, t["wfc"], p, idx, xhat, F64)
    _close(hb["dp2"], p4.grad.flatten(1), "dp2")
    _close(hb["dW"], lin.weight.grad, "dW")
    _close(hb["db"], lin.bias.grad, "db")
    _close(hb["S1"], bn.bias.grad, "S1 = dbeta")
    _close(hb["S2"], bn.weight.grad, "S2 = dgamma")
    _close(hb["S1_rows"].sum(0), hb["S1"])
    # a second batch under momentum None: the cumulative average weighs it 1/2
    st2 = R.bn_from_rows(t["rows"], t["shift"], t["gamma"], t["beta"], t["eps"], st["rm"], st["rv"], momentum, 2)
    bn(y2)
    _close(st2["rm"], bn.running_mean, "running_mean, second batch")
    _close(st2["rv"], bn.running_var, "running_var, second batch")


HEAD_CASES = list(itertools.product(R.HEAD_B, R.HEAD_N + R.HEAD_N_FWD))


@pytest.mark.parametrize("Bn,N", HEAD_CASES)
def test_head_generator(Bn, N):
    t = R.head_inputs(Bn, N, R.head_seed(Bn, N), 131 if Bn == 3 else 4 * Bn)
    n, d = t["n"], t["d"]
    y2 = t["y2"]
    assert torch.equal(y2, y2.round()) and all(_exact_in(y2, dt) for dt in DTYPES)
    assert int(d.abs().max()) <= 8 and not d.sum(1).any()
    _close(y2.mean((0, 2, 3)), t["m"], "integer mean")
    # the slab: integer rows, integer partial sums below 2^24, the totals of y2 around the shift
    rows = t["rows"]
    assert torch.equal(rows, rows.round()) and float(rows.abs().sum(0).max()) < 2 ** 24
    dd = y2 - t["shift"].view(1, -1, 1, 1)
    tot = rows.sum(0)
    assert torch.equal(tot[:R.HC], dd.sum((0, 2, 3))) and torch.equal(tot[R.HC:2 * R.HC], (dd * dd).sum((0, 2, 3)))
    assert float(tot[-1]) == n
    st = R.bn_from_rows(rows, t["shift"], t["gamma"], t["beta"], t["eps"])
    assert torch.equal(st["mean"], t["m"])
    sc = t["gamma"] * st["invstd"]
    assert float((sc.abs() - 1).abs().max()) <= R.U32 and int((t["gamma"] < 0).sum()) >= 3
    for v in (t["gamma"], t["beta"], t["rm0"], t["rv0"], t["wfc"], t["bfc"], t["shift"]):
        assert _exact_in(v, torch.float32)
    assert torch.equal((2 * t["beta"]) % 2, torch.ones(R.HC, dtype=F64))
    # distance from the ReLU threshold; ties on the maximum; wholly negative windows
    z = (y2 - st["mean"].view(1, -1, 1, 1)) * sc.view(1, -1, 1, 1) + t["beta"].view(1, -1, 1, 1)
    assert float(z.abs().min()) >= 0.25 and float(z.abs().max()) <= 10.5 + 1e-5
    zw = R._windows(z.round_(decimals=1))
    top = zw.max(-1, keepdim=True).values
    assert bool(((zw == top).sum(-1) > 1)[top.squeeze(-1) > 0].any()), "a tie on a positive maximum"
    assert bool((top < 0).any()), "a wholly negative window"
    srt = zw.sort(-1).values
    gap = srt[..., 1:] - srt[..., :-1]
    assert bool(((gap == 0) | (gap >= 1 - 1e-5)).all())
    w64 = t["wfc"] * 64
    assert torch.equal(w64, w64.round()) and float(w64.abs().max()) <= 4
    assert all(_exact_in(t["wfc"], dt) for dt in DTYPES)
    for dt in DTYPES[1:]:  # bf16 / fp16: p is the exact half-integer, the logits exact in fp32
        p, idx, xhat, _, _ = R.bn_relu_pool(y2, st["mean"], st["invstd"], t["gamma"], t["beta"], dt)
        assert torch.equal(2 * p, (2 * p).round()) and float(p.max()) <= 10.5
        lg, A = R.fc(p, t["wfc"], t["bfc"])
        assert torch.equal(lg * 128, (lg * 128).round()) and float(A.max()) < 2 ** 11
        lr = R.rounded(lg.float(), dt)
        assert float((lr.max(1).values - lr.min(1).values).max()) <= R.SPREAD


@pytest.mark.parametrize("Bn,N", [(1, 1), (33, 10), (64, 16)])
def test_head_bwd_generator(Bn, N):
    t = R.head_bwd_inputs(Bn, N, R.head_seed(Bn, N))
    for dt in DTYPES:
        assert all(_exact_in(t[k], dt) for k in ("dl", "p2", "xh2", "wfc"))
        hb = R.head_bwd(t["dl"], t["wfc"], t["p2"], t["idx2"], t["xh2"], dt)
        assert _exact_in(hb["dp2"], dt), "dp2: multiples of 1/64 below 4"
        for k in ("dp2", "S1", "S2", "S1_rows", "S2_rows"):
            assert torch.equal(hb[k] * 64, (hb[k] * 64).round())
        assert float(hb["A2_rows"].sum(0).max()) * 64 < 2 ** 24
        assert torch.equal(hb["dW"], hb["dW"].round()) and float((t["dl"].abs().t() @ t["p2"]).max()) < 2 ** 24
    assert bool((t["idx2"] & 4).any()) and not bool((t["idx2"] & 4).all())
