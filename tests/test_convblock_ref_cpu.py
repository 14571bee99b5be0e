"""tests/_convblock_ref.py against torch autograd through conv2d -> batch_norm(training) -> relu
-> max_pool2d in float64, and the conditions its generators promise (no GPU)."""
import pytest
import torch
import torch.nn.functional as F

from . import _bn_ref as B
from . import _convblock_ref as R
from . import _head_ref as HR

TOL = dict(rtol=1e-9, atol=1e-9)


def _autograd(layer, Bn=2, seed=0):
    ci, co, H, W = R.LAYERS[layer]
    g = torch.Generator().manual_seed(100 * layer + seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, w, b = rn(Bn, ci, H, W).requires_grad_(), (0.2 * rn(co, ci, 5, 5)).requires_grad_(), rn(co).requires_grad_()
    gamma, beta = (0.5 + torch.rand(co, generator=g, dtype=torch.float64)).requires_grad_(), (0.3 * rn(co)).requires_grad_()
    rm0, rv0 = rn(co), 0.5 + torch.rand(co, generator=g, dtype=torch.float64)
    dp = rn(Bn, co, H // 2, W // 2)
    return dict(x=x, w=w, b=b, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, dp=dp)


@pytest.mark.parametrize("momentum", [0.1, None])
@pytest.mark.parametrize("layer", [1, 2])
def test_reference_matches_autograd(layer, momentum):
    c = _autograd(layer)
    x, w, b, gamma, beta, dp = (c[k] for k in ("x", "w", "b", "gamma", "beta", "dp"))
    co, Bn = w.shape[0], x.shape[0]
    nbt = 5  # batches tracked after this one
    rm, rv = c["rm0"].clone(), c["rv0"].clone()
    y = F.conv2d(x, w, b, padding=2)
    y.retain_grad()
    z = F.batch_norm(y, rm, rv, gamma, beta, training=True, momentum=momentum if momentum is not None else 1.0 / nbt,
                     eps=R.EPS32)
    p, ind = F.max_pool2d(F.relu(z), 2, 2, return_indices=True)
    p.backward(dp)
    xd, wd, bd, gd, bed = (t.detach() for t in (x, w, b, gamma, beta))
    # forward: conv, statistics from per-image rows around a shift, BN -> ReLU -> pool
    yr, _ = R.conv_fwd(xd, wd, bd)
    assert torch.allclose(yr, y.detach(), **TOL)
    shift = c["rm0"]
    st = HR.bn_from_rows(R.fwd_stat_rows(yr, shift), shift, gd, bed, R.EPS32, c["rm0"], c["rv0"], momentum, nbt)
    assert torch.allclose(st["rm"], rm, **TOL) and torch.allclose(st["rv"], rv, **TOL)
    f = R.bn_relu_pool(yr, st["mean"], st["invstd"], gd, bed, torch.float64)
    assert torch.allclose(f["p"], p.detach(), **TOL)
    H, W = yr.shape[2:]
    pos = ((ind // W) % 2) * 2 + (ind % W) % 2
    assert torch.equal(f["idx"].long(), pos)
    und = ~R.pool_decided(f["z"], f["A"], yr, f["idx"], torch.float32)
    assert int(und.sum()) <= 2  # random doubles: a window within 32 u A of a tie is a 1e-5 event
    # backward: routing, BN sums and input gradient, conv gradients
    dz = R.route(dp, f["p"], f["idx"])
    bw = R.bn_bwd(dz, yr, st["mean"], st["invstd"], gd)
    assert torch.allclose(bw["S1"], beta.grad, **TOL) and torch.allclose(bw["S2"], gamma.grad, **TOL)
    assert torch.allclose(bw["S1_rows"].sum(0), bw["S1"], **TOL) and torch.allclose(bw["S2_rows"].sum(0), bw["S2"], **TOL)
    assert torch.allclose(bw["dx"], y.grad, **TOL)
    dx2, _ = R.bn_dx(dz, yr, st["mean"], st["invstd"], gd, bw["S1"], bw["S2"], st["n"])
    assert torch.allclose(dx2, bw["dx"], **TOL)
    dy = y.grad
    rows, _ = R.conv_wgrad_rows(xd, dy)
    nw = wd.numel()
    for i in range(Bn):  # per image
        wi = torch.nn.grad.conv2d_weight(xd[i:i + 1], wd.shape, dy[i:i + 1], padding=2)
        assert torch.allclose(rows[i, :nw], wi.reshape(-1), **TOL)
        assert torch.allclose(rows[i, nw:], dy[i].sum((1, 2)), **TOL)
    assert torch.allclose(rows.sum(0)[:nw], w.grad.reshape(-1), **TOL)
    assert torch.allclose(rows.sum(0)[nw:], b.grad, **TOL)
    # row chunks add up to the image (the conv1 chunks of 4 rows)
    parts = sum(R.conv_wgrad_rows(xd, dy, lo, lo + H // 7)[0] for lo in range(0, H, H // 7))
    assert torch.allclose(parts, rows, **TOL)
    dxr, _ = R.conv_dgrad(dy, wd)
    assert torch.allclose(dxr, x.grad, **TOL)


def test_head_ref_pool_agrees():
    """On the 14x14 map the pooling of this module is _head_ref.bn_relu_pool (its idx byte
    is the position | 4 where p > 0)."""
    c = _autograd(2, seed=1)
    y = R.conv_fwd(c["x"].detach(), c["w"].detach(), c["b"].detach())[0]
    mean, _, invstd = B.batch_moments(R.rows_of(y), R.EPS32)
    gamma, beta = c["gamma"].detach(), c["beta"].detach()
    for dt in R.DTYPES:
        f = R.bn_relu_pool(y, mean, invstd, gamma, beta, dt)
        p, idx, _, _, _ = HR.bn_relu_pool(y, mean, invstd, gamma, beta, dt)
        assert torch.equal(f["p"].reshape(p.shape), p)
        assert torch.equal((f["idx"] | torch.where(f["p"] > 0, 4, 0).to(torch.uint8)).reshape(idx.shape), idx)


@pytest.mark.parametrize("Bn", [1, 3])
@pytest.mark.parametrize("layer", [1, 2])
def test_integer_conv_cases_are_exact(layer, Bn):
    """Every integer conv case: |value| exact in bf16 (<= 256) and the sum of |terms| per
    output (and of the statistics, over a whole image) below 2^24."""
    c = R.int_conv(layer, Bn, 10 * layer + Bn)
    y, A = R.conv_fwd(c["x"], c["w"], c["bias"])
    assert float(y.abs().max()) <= R.INT_MAX[torch.bfloat16] and float(A.max()) < R.EXACT
    assert torch.equal(y, y.round())
    d = (y - c["shift"].view(1, -1, 1, 1)).abs()
    assert float(d.sum((2, 3)).max()) < R.EXACT and float((d * d).sum((2, 3)).max()) < R.EXACT
    w = R.int_wgrad(layer, Bn, 30 * layer + Bn)
    rows, Aw = R.conv_wgrad_rows(w["x"], w["dy"])
    assert float(Aw.max()) < R.EXACT and torch.equal(rows, rows.round())
    if layer == 2:
        dg = R.int_dgrad(Bn, 20 + Bn)
        dx, Ad = R.conv_dgrad(dg["dy"], dg["w"])
        assert float(dx.abs().max()) <= R.INT_MAX[torch.bfloat16] and float(Ad.max()) < R.EXACT


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("layer", [1, 2])
def test_impulse_cases_hit_every_tap_and_border(layer, variant):
    _, _, H, W = R.LAYERS[layer]
    x, dy, where = R.impulse_wgrad(layer, variant, 5 * layer + variant)
    rows, _ = R.conv_wgrad_rows(x, dy)
    nw = rows.shape[1] - dy.shape[1]
    assert sorted((kh, kw) for _, _, kh, kw, _, _ in where) == [(a, b) for a in range(5) for b in range(5)]
    border = set()
    for t, (co, ci, kh, kw, v, dv) in enumerate(where):
        nz = rows[t, :nw].nonzero().flatten().tolist()
        assert nz == [(co * x.shape[1] + ci) * 25 + kh * 5 + kw] and rows[t, nz[0]] == v
        assert rows[t, nw:].nonzero().flatten().tolist() == [co] and rows[t, nw + co] == dv
        for img in (dy[t], x[t]):
            h, w = (int(v) for v in img.abs().sum(0).nonzero()[0])
            border |= {("top", h == 0), ("bottom", h == H - 1), ("left", w == 0), ("right", w == W - 1)}
    assert {(k, True) for k in ("top", "bottom", "left", "right")} <= border


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("layer", [1, 2])
def test_pool_cases_stay_within_the_skip_allowance(layer, dtype):
    """The reference alone: no window of a generated case is left undecided beyond the skip
    allowance, the cases hold ties and all-negative windows, and the slab rows sum exactly."""
    C = R.LAYERS[layer][1]
    G = 256 // (2 * C + 1)
    for nrows in (1, G, 4 * G - 1, 4 * G, 4 * G + 1):
        c = R.pool_case(layer, 3, nrows, dtype, 7 * layer + nrows)
        assert c["rows"].shape == (nrows, 2 * C + 1) and float(c["rows"].abs().sum(0).max()) < R.EXACT
        st = HR.bn_from_rows(c["rows"].double(), c["shift"], c["gamma"], c["beta"], R.EPS32)
        assert st["n"] == c["n"] and bool((st["var"] > 0.2).all())
        assert torch.equal(R.rounded(c["y"], dtype), c["y"])
        f = R.bn_relu_pool(c["y"], st["mean"], st["invstd"], c["gamma"], c["beta"], dtype)
        und = ~R.pool_decided(f["z"], f["A"], c["y"], f["idx"], dtype)
        assert int(und.sum()) <= B.skip_allowance(und.numel())
        aw = R.windows(f["act"])
        top2 = aw.sort(-1, descending=True).values
        assert int(((top2[..., 0] == top2[..., 1]) & (top2[..., 0] > 0)).sum()) > 50  # positive ties
        assert int((aw.max(-1).values == 0).sum()) > 50  # all-negative windows: index 0
        assert bool((f["idx"][aw.max(-1).values == 0] == 0).all())
        # ATen's max_pool2d on the reference's own rounded activations gives the same index
        _, ind = F.max_pool2d(f["act"], 2, 2, return_indices=True)
        W = c["y"].shape[3]
        assert torch.equal(((ind // W) % 2) * 2 + (ind % W) % 2, f["idx"].long())


@pytest.mark.parametrize("Bn", [1, 3, 8, 9, 11])
@pytest.mark.parametrize("layer", [1, 2])
def test_bwd_reduce_cases_are_exact(layer, Bn):
    c = R.bwd_case(layer, Bn, 50 * layer + Bn, "int")
    C = R.LAYERS[layer][1]
    assert torch.equal(c["mean"], c["fstats"][2 * C + 1:]) and torch.equal(c["mean"], c["mean"].round())
    dz = R.route(c["dp"], c["p"], c["idx"])
    bw = R.bn_bwd(dz, c["y"], c["mean"], c["invstd"], c["gamma"])
    assert torch.equal(bw["S1"], bw["S1"].round()) and float(bw["A1_rows"].sum(0).max()) < R.EXACT
    prod = dz * (c["y"] - c["mean"].view(1, -1, 1, 1))
    assert torch.equal(prod, prod.round()) and float(prod.abs().max()) < R.EXACT
    assert int((c["p"] <= 0).sum()) > 0 and int((c["p"] > 0).sum()) > 0


@pytest.mark.parametrize("Bn", [1, 3, 5])
def test_conv1_wgrad_integer_case(Bn):
    """dy = gamma * g is a multiple of 1/2 (|dy| <= 6, exact in bf16 / fp16), the per-image
    sums of |terms| are far below 2^24 / 2, and invstd is 1 to a few fp32 ulp."""
    c = R.conv1_wgrad_int(Bn, Bn)
    assert torch.equal(2 * c["dy"], (2 * c["dy"]).round()) and float(c["dy"].abs().max()) <= 6
    for dt in R.DTYPES:
        assert torch.equal(R.rounded(c["dy"], dt), c["dy"]) and torch.equal(R.rounded(c["x"], dt), c["x"])
    rows, A = R.conv_wgrad_rows(c["x"], c["dy"])
    assert float(A.max()) < R.EXACT / 2 and torch.equal(2 * rows, (2 * rows).round())
    n, f = c["n"], c["fstats"]
    invstd = (f[16:32] / n + R.EPS32).rsqrt()
    assert float((invstd - 1).abs().max()) < 4 * R.U32
    assert {int(v) for v in c["idx"].unique()} == set(range(8))
    assert {float(v) for v in c["gamma"].abs().unique()} <= {0.5, 1.0, 2.0}
