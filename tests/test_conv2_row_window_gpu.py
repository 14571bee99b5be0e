"""Row-window staging of the fused conv2 kernels (csrc/kernels/conv5x5.h conv5x5_body WR):
a workgroup stages only the input rows its own output pixels read, and the pooled outputs are
shared out by output pixel range.

convnet.conv2_fwd and convnet.conv2_bwd are called directly at the layer's own shapes
(16 -> 32 channels, 14 x 14), batch 1 and 3, against float64 torch references on the CPU:

  forward   BN1 from the GIVEN statistics -> ReLU -> max_pool2d -> conv2d (+ bias):
            y2, the summed BN2 partial rows, p1 / idx1 / xh1;
  backward  BN2 / ReLU / pool backward (autograd) -> conv_transpose2d: dp1 and the summed
            BN1 partial rows [S1 | S2].

Every input value is random per element, so rows differ: a window off by one row, a row left
unstaged (stale LDS: garbage, or the previous launch's data) or a halo row not zeroed changes
y2 / dp1 far beyond the bounds.  The kernels run at the split counts they were compiled with
(no runtime knob); the checks do not depend on them.

Bounds.  GEMM outputs and the sums over them follow tests/test_convnet_fused_gpu.py
::test_convnet_fused_fwd_bwd: relative error (norm) against float64 at most FAC x the error
of torch's own computation of the same quantity in the same dtype, FAC = 2 (bf16 / fp16) or
4 (fp32), floors 2e-3 / 1e-5.  The pooled outputs are one fp32 expression of the inputs
rounded once to the storage dtype, so they are bounded per element from the formats: half
an ulp of the dtype at the value plus SLACK = 16 * 2^-24 of the expression's operand
magnitudes for its fp32 operations (subtract, multiply, add, and the rsqrt / divide in the
coefficients).  The argmax is compared exactly wherever the float64 window maximum leads the
runner-up by more than that rounding; elsewhere the kernel's choice must be within the
rounding of the maximum.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-5
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
IDS = ["bf16", "fp16", "fp32"]
HALF_ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}  # relative
SLACK = 16 * 2.0 ** -24


def _fac_floor(dtype):
    return (4.0, 1e-5) if dtype == torch.float32 else (2.0, 2e-3)


def _rel(a, r):
    return ((a.double() - r.double()).norm() / (r.double().norm() + 1e-12)).item()


def _bound(what, a, r, t, dtype):
    fac, floor = _fac_floor(dtype)
    e, lim = _rel(a.cpu(), r), max(fac * _rel(t.cpu(), r), floor)
    print(f"{what}: err {e:.3e} limit {lim:.3e}")
    assert e < lim, (what, e, lim)


def _pack_fwd(w2, dtype):
    """[32][16][5][5] -> the forward LDS tile [32][424], k = tap * 16 + ci, K padding zero."""
    t = torch.zeros(32, 424)
    t[:, :400] = w2.reshape(32, 16, 25).permute(0, 2, 1).reshape(32, 400)
    return t.reshape(-1).to(dtype)


def _pack_dgrad(w2, dtype):
    """-> the data-gradient tile [16][808], k = (24 - tap) * 32 + co (the flipped transpose)."""
    t = torch.zeros(16, 808)
    t[:, :800] = w2.reshape(32, 16, 25).flip(2).permute(1, 2, 0).reshape(16, 800)
    return t.reshape(-1).to(dtype)


# ---------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fwd_case(B, dtype, seed=0, scale=1.0):
    """Seeded inputs (CPU) and the float64 / torch-in-dtype references; never modified."""
    g = torch.Generator().manual_seed(100 * B + 10 * DTYPES.index(dtype) + seed)
    y1 = (torch.randn(B, 16, 28, 28, generator=g) * scale).to(dtype)
    gamma = torch.rand(16, generator=g) + 0.5
    beta = torch.rand(16, generator=g) * 0.4 - 0.2
    w2 = (torch.randn(32, 16, 5, 5, generator=g) * 0.05).to(dtype).float()  # exact in the dtype
    bias2 = torch.randn(32, generator=g) * 0.1
    rm2 = torch.rand(32, generator=g) * 0.2 - 0.1  # BN2's shift (its running mean)
    # the GIVEN statistics: one slab row [sum(y - shift) | sum((y - shift)^2) | n] in fp32
    yd = y1.double()
    shift = (yd.mean((0, 2, 3)) + 0.01).float()
    d = yd - shift.double().view(1, -1, 1, 1)
    n = float(B * 784)
    fslab1 = torch.cat([d.sum((0, 2, 3)), (d * d).sum((0, 2, 3)), torch.tensor([n], dtype=torch.float64)]).float()
    fstats1 = torch.cat([torch.zeros(33), shift])
    # float64 reference FROM the fp32 statistics
    m1 = fslab1[:16].double() / n
    mean = shift.double() + m1
    var = (fslab1[16:32].double() / n - m1 * m1).clamp_(min=0)
    istd = torch.rsqrt(var + EPS)
    V = lambda v: v.view(1, -1, 1, 1)  # noqa: E731
    z = (yd - V(mean)) * V(gamma.double() * istd) + V(beta.double())
    win = z.reshape(B, 16, 14, 2, 14, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, 16, 14, 14, 4)  # k = dy * 2 + dx
    zmax, kref = win.max(-1)
    p1 = zmax.clamp(min=0)
    y2 = F.conv2d(p1, w2.double(), bias2.double(), padding=2)
    # operand magnitudes of the two fp32 expressions, per window element (y - mean cancels: its
    # error is relative to |y| + |mean|, the fp32 mean's own rounding included)
    W4 = lambda v: v.reshape(B, 16, 14, 2, 14, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, 16, 14, 14, 4)  # noqa: E731
    ymag = yd.abs() + V(mean.abs())
    zmag = W4(ymag * V((gamma.double() * istd).abs()) + V(beta.double().abs()))
    xmag = W4(ymag * V(istd))
    xwin = W4((yd - V(mean)) * V(istd))
    sh2 = V(rm2.double())
    stats2 = torch.cat([(y2 - sh2).sum((0, 2, 3)), ((y2 - sh2) ** 2).sum((0, 2, 3))])
    # torch in `dtype` (GPU): the same chain with every intermediate in the dtype
    zt = F.batch_norm(y1.to(DEV), mean.float().to(DEV), var.float().to(DEV), gamma.to(DEV), beta.to(DEV), False, 0.0,
                      EPS)
    y2t = F.conv2d(F.max_pool2d(F.relu(zt), 2, 2), w2.to(DEV, dtype), bias2.to(DEV, dtype), padding=2).double().cpu()
    stats2t = torch.cat([(y2t - sh2).sum((0, 2, 3)), ((y2t - sh2) ** 2).sum((0, 2, 3))])
    return dict(B=B, dtype=dtype, y1=y1, gamma=gamma, beta=beta, w2=w2, bias2=bias2, rm2=rm2, fslab1=fslab1,
                fstats1=fstats1, win=win, kref=kref, p1=p1, y2=y2, zmag=zmag, xmag=xmag, xwin=xwin, stats2=stats2, y2t=y2t,
                stats2t=stats2t, wpk=_pack_fwd(w2, dtype))


def _run_fwd(C, c, sentinel=True):
    cn = C.convnet
    B, dt = c["B"], c["dtype"]
    dev = lambda k: c[k].to(DEV)  # noqa: E731
    ns = cn.fwd2_split(dt == torch.float32)
    y2 = torch.full((B, 32, 14, 14), float("nan"), device=DEV, dtype=dt)
    fslab2 = torch.full((B * ns * 65,), float("nan"), device=DEV)
    fstats2 = torch.zeros(97, device=DEV)
    p1 = torch.full((B, 16, 14, 14), float("nan") if sentinel else 0.0, device=DEV, dtype=dt)
    xh1 = torch.full((B, 16, 14, 14), float("nan") if sentinel else 0.0, device=DEV, dtype=dt)
    idx1 = torch.full((B, 16, 14, 14), 0xFF if sentinel else 0, device=DEV, dtype=torch.uint8)
    rm1, rv1 = torch.zeros(16, device=DEV), torch.ones(16, device=DEV)
    nbt1 = torch.zeros(1, dtype=torch.int64, device=DEV)
    cn.conv2_fwd(dev("y1"), dev("fslab1"), dev("fstats1"), dev("gamma"), dev("beta"), rm1, rv1, nbt1, 0.1, EPS, True,
                 dev("w2"), dev("bias2"), y2, fslab2, fstats2, dev("rm2"), p1, idx1, xh1, dev("wpk"), None)
    torch.cuda.synchronize()
    return dict(y2=y2.cpu(), rows2=fslab2.view(B * ns, 65).cpu(), p1=p1.cpu(), idx1=idx1.cpu(), xh1=xh1.cpu())


def _check_fwd(c, o, tag):
    B, dt = c["B"], c["dtype"]
    hu = HALF_ULP[dt]
    # write-once outputs: no sentinel left
    assert not bool(torch.isnan(o["p1"].float()).any()), "p1: element not written"
    assert not bool(torch.isnan(o["xh1"].float()).any()), "xh1: element not written"
    assert not bool((o["idx1"] == 0xFF).any()), "idx1: element not written"
    assert not bool(torch.isnan(o["y2"].float()).any()), "y2: element not written"
    # conv output and BN2 partial sums
    _bound(f"{tag} y2", o["y2"], c["y2"], c["y2t"], dt)
    rows = o["rows2"].double()
    assert not bool(torch.isnan(rows).any())
    assert rows[:, 64].sum().item() == B * 196, "BN2 partial rows: pixel counts"
    _bound(f"{tag} BN2 sums", rows[:, :32].sum(0), c["stats2"][:32], c["stats2t"][:32], dt)
    _bound(f"{tag} BN2 sums of squares", rows[:, 32:64].sum(0), c["stats2"][32:], c["stats2t"][32:], dt)
    # pooled map: per element from the formats
    p1, ref = o["p1"].double(), c["p1"]
    k = (o["idx1"] & 3).long()
    zsel = c["win"].gather(-1, k.unsqueeze(-1)).squeeze(-1)       # float64 z at the kernel's argmax
    slack = SLACK * c["zmag"].amax(-1)
    lim = hu * (ref.abs() + slack) + slack
    err = (p1 - ref).abs()
    print(f"{tag} p1: max err/limit {(err / lim.clamp_min(1e-30)).max().item():.3f}")
    assert bool((err <= lim).all()), ("p1", (err / lim.clamp_min(1e-30)).max().item())
    # argmax (first maximum of the ReLU outputs: a window with nothing positive keeps position
    # 0): exact where float64 decides by more than the rounding, a maximum wherever one is positive
    top2 = c["win"].topk(2, -1).values
    tol = 2 * (hu * (top2[..., 0].abs() + slack) + slack)
    positive = top2[..., 0] > tol
    decided = positive & ((top2[..., 0] - top2[..., 1]) > tol)
    print(f"{tag} idx1: {decided.float().mean().item():.3f} of the windows decided beyond rounding")
    # (1/16 of the windows have no positive value; a few percent are within the rounding)
    assert decided.float().mean().item() > 0.8
    assert bool((k == c["kref"])[decided].all()), "idx1: argmax differs from the reference"
    assert bool((top2[..., 0] - zsel <= tol)[positive].all()), "idx1: argmax is not a maximum of its window"
    assert bool((k == 0)[top2[..., 0] < -tol].all()), "idx1: a window with nothing positive keeps position 0"
    relu = (o["idx1"] & 4) != 0
    assert bool((o["idx1"] < 8).all()) and bool((relu == (o["p1"].float() > 0)).all()), "idx1: ReLU bit"
    # xhat at the kernel's argmax
    xref = c["xwin"].gather(-1, k.unsqueeze(-1)).squeeze(-1)
    xs = SLACK * c["xmag"].gather(-1, k.unsqueeze(-1)).squeeze(-1)
    xlim = hu * (xref.abs() + xs) + xs
    xerr = (o["xh1"].double() - xref).abs()
    print(f"{tag} xh1: max err/limit {(xerr / xlim.clamp_min(1e-30)).max().item():.3f}")
    assert bool((xerr <= xlim).all()), ("xh1", (xerr / xlim.clamp_min(1e-30)).max().item())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B", [1, 3])
def test_forward_matches_float64(C, B, dtype):
    """y2, the summed BN2 partial rows and the sentinel-prefilled p1 / idx1 / xh1 (every element
    written, none differing from the reference: a hole or an overlap of the ownership shows)."""
    c = _fwd_case(B, dtype)
    _check_fwd(c, _run_fwd(C, c), f"B={B} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_forward_no_stale_lds_and_deterministic(C, dtype):
    """Image set A (large values), then a different set B in the same process: B is checked, so
    a row left unstaged -- which would still hold A's data or garbage -- shows.  Reruns of B
    are bitwise equal whatever the outputs held before."""
    a, b = _fwd_case(3, dtype, seed=1, scale=8.0), _fwd_case(3, dtype, seed=2)
    _run_fwd(C, a)
    ob = _run_fwd(C, b)
    _check_fwd(b, ob, f"after A, {dtype}")
    _run_fwd(C, a)
    ob2 = _run_fwd(C, b, sentinel=False)
    for k in ob:
        assert torch.equal(ob[k], ob2[k]), k


# ---------------------------------------------------------------------------------------
# data gradient
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bwd_case(B, dtype, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(5000 + 100 * B + 10 * DTYPES.index(dtype) + seed)
    y2 = (torch.randn(B, 32, 14, 14, generator=g) * scale).to(dtype)
    dp2 = (torch.randn(B, 32, 7, 7, generator=g) * scale).to(dtype)
    gamma = torch.rand(32, generator=g) + 0.5
    beta = torch.rand(32, generator=g) * 0.4 - 0.2
    w2 = (torch.randn(32, 16, 5, 5, generator=g) * 0.05).to(dtype).float()
    idx1 = torch.randint(0, 8, (B, 16, 14, 14), generator=g, dtype=torch.uint8)
    xh1 = torch.randn(B, 16, 14, 14, generator=g).to(dtype)
    p1 = torch.randn(B, 16, 14, 14, generator=g).clamp_(min=0).to(dtype)  # the weight-gradient role's operand
    # float64: BN2 (batch statistics) -> ReLU -> MaxPool and its backward
    y = y2.double().requires_grad_()
    z = F.batch_norm(y, None, None, gamma.double(), beta.double(), training=True, eps=EPS)
    z.retain_grad()
    pool, ind = F.max_pool2d(F.relu(z), 2, 2, return_indices=True)
    pool.backward(dp2.double())
    dy64, gz = y.grad, z.grad
    pos = ((ind // 14) % 2) * 2 + (ind % 14) % 2
    idx2 = (pos + 4 * (pool > 0)).to(torch.uint8)
    yd = y2.double()
    mean, var = yd.mean((0, 2, 3)), yd.var((0, 2, 3), unbiased=False)
    shift = mean.float()
    d = yd - shift.double().view(1, -1, 1, 1)
    fstats2 = torch.cat([d.sum((0, 2, 3)), (d * d).sum((0, 2, 3)), torch.tensor([float(B * 196)], dtype=torch.float64),
                         shift.double()]).float()
    xhat = (yd - mean.view(1, -1, 1, 1)) * torch.rsqrt(var + EPS).view(1, -1, 1, 1)
    gsum2 = torch.cat([gz.sum((2, 3)), (gz * xhat).sum((2, 3))], 1).float().contiguous()  # [B][64]
    # data gradient and the BN1 sums of the block below, from the given idx1 / xh1
    dp1 = F.conv_transpose2d(dy64, w2.double(), padding=2)
    open1 = ((idx1 & 4) != 0).double()
    sums = lambda v: torch.cat([(v * open1).sum((0, 2, 3)), (v * open1 * xh1.double()).sum((0, 2, 3))])  # noqa: E731
    dp1t = F.conv_transpose2d(dy64.to(dtype).to(DEV), w2.to(DEV, dtype), padding=2).double().cpu()
    return dict(B=B, dtype=dtype, y2=y2, dp2=dp2, gamma=gamma, idx1=idx1, xh1=xh1, p1=p1, idx2=idx2, fstats2=fstats2,
                gsum2=gsum2, dp1=dp1, bsum=sums(dp1), dp1t=dp1t, bsumt=sums(dp1t), wpk_d=_pack_dgrad(w2, dtype))


def _run_bwd(C, c, fill=float("nan")):
    cn = C.convnet
    B, dt = c["B"], c["dtype"]
    dev = lambda k: c[k].to(DEV)  # noqa: E731
    rows = cn.dgrad2_rows(B, dt == torch.float32)
    dp1 = torch.full((B, 16, 14, 14), fill, device=DEV, dtype=dt)
    bslab1 = torch.full((rows * 32,), fill, device=DEV)
    wslab2 = torch.empty(cn.wgrad_bn_rows(2, B) * (32 * 400 + 32), device=DEV)
    cn.conv2_bwd(dev("wpk_d"), dev("y2"), dev("dp2"), dev("idx2"), dev("fstats2"), dev("gsum2"), dev("gamma"), EPS, dp1,
                 dev("idx1"), dev("xh1"), bslab1, dev("p1"), wslab2, None, None, None, None, None, None, None, None, None)
    torch.cuda.synchronize()
    return dict(dp1=dp1.cpu(), rows=bslab1.view(rows, 32).cpu())


def _check_bwd(c, o, tag):
    dt = c["dtype"]
    assert not bool(torch.isnan(o["dp1"].float()).any()), "dp1: element not written"
    assert not bool(torch.isnan(o["rows"]).any()), "BN1 partial rows: element not written"
    _bound(f"{tag} dp1", o["dp1"], c["dp1"], c["dp1t"], dt)
    s = o["rows"].double().sum(0)
    _bound(f"{tag} BN1 S1", s[:16], c["bsum"][:16], c["bsumt"][:16], dt)
    _bound(f"{tag} BN1 S2", s[16:], c["bsum"][16:], c["bsumt"][16:], dt)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B", [1, 3])
def test_dgrad_matches_float64(C, B, dtype):
    """dp1 (prefilled with NaN: every element written) and the summed BN1 partial rows."""
    c = _bwd_case(B, dtype)
    _check_bwd(c, _run_bwd(C, c), f"B={B} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dgrad_no_stale_lds_and_deterministic(C, dtype):
    """As the forward's: set A (large values), then set B, which is checked; reruns bitwise equal."""
    a, b = _bwd_case(3, dtype, seed=1, scale=8.0), _bwd_case(3, dtype, seed=2)
    _run_bwd(C, a)
    ob = _run_bwd(C, b)
    _check_bwd(b, ob, f"after A, {dtype}")
    _run_bwd(C, a)
    ob2 = _run_bwd(C, b, fill=0.0)
    for k in ob:
        assert torch.equal(ob[k], ob2[k]), k
