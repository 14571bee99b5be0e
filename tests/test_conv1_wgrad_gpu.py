"""The conv1 weight gradient of the fused ConvNet step: conv5x5_wgrad_body<T, 1, 16, 28, 28, 4, PRO 2>
(csrc/kernels/conv5x5_wgrad.h), 7 chunks of 4 rows per image with BN1's backward applied on the
fly, as launched by C.convnet.conv_wgrad_bn (layer-1 branch) and by C.convnet.conv1_wgrad_slab2,
which also sums the columns of the conv2 slab in extra workgroups (slab_reduce_chunks_body<4>)
and writes BN1's dgamma / dbeta.

  a  exact on integers (bf16 / fp16; fp32 within a derived bound), NaN-prefilled slab, the two
     launches and two runs bitwise equal
  b  float64 per slab row on random floats with the full BN backward: the rule of
     tests/test_conv2_wgrad_slices_gpu.py::test_rows_match_float64 (error at most 2x torch's
     in the same dtype, floors 1e-5 / 2e-3; bias columns absolute), applied to every chunk
     on its own, so the chunks with a halo row above row 0 or below row 27 cannot hide
  c  dgamma / dbeta from gsum, or from a distinct lsum
  d  out2 = exact column sums of an integer conv2 slab at the row counts where
     slab_colsum_chunks changes path (B = 1, 17, 32 | 33, 257), into a view with guards
  e  the producer-side check word

Reference: tests/_convblock_ref.py (CPU, float64).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from . import _convblock_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
EPS = 1e-5
N1, N2 = 16 * 25 + 16, 32 * 400 + 32
CH = 7  # chunks (slab rows) per image
FLT_MAX = 3.402823466e38
IDS = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
DT = pytest.mark.parametrize("dtype", R.DTYPES, ids=[IDS[d] for d in R.DTYPES])
LAUNCH = pytest.mark.parametrize("which", ["conv_wgrad_bn", "conv1_wgrad_slab2"])
RATIOS = {}


def _act(t, dtype):
    return t.to(dtype).to(DEV).contiguous()


def _f(t):
    return t.float().to(DEV).contiguous()


def _grows(C, Bn, dtype):
    return C.convnet.dgrad2_rows(Bn, dtype == torch.float32)


def _run(C, which, dtype, c, gsum, lsum=None, wslab2=None, out2=None, chk=None):
    """One launch on the inputs of case c (CPU tensors); returns (slab rows [7B][416], dg1, dbe1)."""
    cn = C.convnet
    Bn = c["x"].shape[0]
    nwg1 = cn.wgrad_bn_rows(1, Bn)
    assert nwg1 == CH * Bn
    wslab1 = torch.full((nwg1 * N1,), NAN, device=DEV)
    dg, dbe = torch.full((16,), NAN, device=DEV), torch.full((16,), NAN, device=DEV)
    args = (_act(c["x"], dtype), _act(c["y"], dtype), _act(c["dp"], dtype), c["idx"].to(DEV), _f(c["fstats"]),
            _f(gsum.reshape(-1)), None if lsum is None else _f(lsum.reshape(-1)), _f(c["gamma"]), EPS, dg, dbe, wslab1)
    if which == "conv_wgrad_bn":
        cn.conv_wgrad_bn(*args, None)
    else:
        if wslab2 is None:
            wslab2 = torch.zeros(cn.wgrad_bn_rows(2, Bn) * N2, device=DEV)
            out2 = torch.empty(N2, device=DEV)
        cn.conv1_wgrad_slab2(*args, wslab2, out2, None, chk)
    torch.cuda.synchronize()
    return wslab1.view(nwg1, N1), dg, dbe


def _chk():
    return torch.zeros(2, dtype=torch.int32, device=DEV)


# =============================================================================== a
@DT
@pytest.mark.parametrize("Bn", [1, 3, 5])
def test_integer_rows_exact(C, Bn, dtype):
    """dy = gamma * g is an exact multiple of 1/2 in bf16 / fp16: the seven rows of an image sum
    exactly to its [dW1 | db1].  fp32 keeps gamma * invstd * g unrounded (invstd = 1 to a few
    ulp): per element within (K + 8) 2^-24 sum|terms|, K = 784 terms per image."""
    c = R.conv1_wgrad_int(Bn, Bn)
    gsum = torch.zeros(_grows(C, Bn, dtype), 32)
    chk = _chk()
    a, dg, dbe = _run(C, "conv_wgrad_bn", dtype, c, gsum)
    b, dg2, dbe2 = _run(C, "conv1_wgrad_slab2", dtype, c, gsum, chk=chk)
    for rows in (a, b):
        assert not bool(torch.isnan(rows).any()), torch.isnan(rows).nonzero()[:8].tolist()
    assert torch.equal(a, b), (a != b).nonzero()[:8].tolist()
    assert torch.equal(a, _run(C, "conv_wgrad_bn", dtype, c, gsum)[0])
    assert torch.equal(b, _run(C, "conv1_wgrad_slab2", dtype, c, gsum)[0])
    assert int(chk[0]) == 0
    for t in (dg, dbe, dg2, dbe2):
        assert bool((t == 0).all())
    want, A = R.conv_wgrad_rows(c["x"], c["dy"])
    got = a.double().cpu().view(Bn, CH, N1).sum(1)
    err = (got - want).abs()
    bnd = torch.zeros_like(A) if dtype != torch.float32 else (784 + 8) * R.U32 * A
    bad = ~(err <= bnd)
    assert not bool(bad.any()), (f"{int(bad.sum())} of {bad.numel()} differ, first at (image, column) "
                                 f"{bad.nonzero()[0].tolist()}: got {got[bad][0].item()} want {want[bad][0].item()}")


# =============================================================================== b
@functools.lru_cache(maxsize=None)
def _fcase(Bn, dtype, grows):
    """Random float inputs, the float64 rows per chunk and torch's own rows in `dtype` (dy rounded
    to the dtype, the same products and sums in that dtype).  Computed once, never modified."""
    g = torch.Generator().manual_seed(2000 * Bn + R.DTYPES.index(dtype))
    y1 = torch.randn(Bn, 16, 28, 28, generator=g).to(dtype)
    x = torch.rand(Bn, 1, 28, 28, generator=g).to(dtype)
    dp1 = torch.randn(Bn, 16, 14, 14, generator=g).to(dtype)
    gamma = torch.rand(16, generator=g) + 0.5
    beta = torch.rand(16, generator=g) * 0.4 - 0.2
    y = y1.double().requires_grad_()
    z = F.batch_norm(y, None, None, gamma.double(), beta.double(), training=True, eps=R.EPS32)
    z.retain_grad()
    pool, ind = F.max_pool2d(F.relu(z), 2, 2, return_indices=True)
    pool.backward(dp1.double())
    dy64, gz = y.grad, z.grad
    idx = (((ind // 28) % 2) * 2 + (ind % 28) % 2 + 4 * (pool > 0)).to(torch.uint8)
    yd = y1.double()
    mean, var = yd.mean((0, 2, 3)), yd.var((0, 2, 3), unbiased=False)
    shift = mean.float().double()
    d = yd - shift.view(1, -1, 1, 1)
    n = Bn * 784
    fstats = R.fstats_of(d.sum((0, 2, 3)), (d * d).sum((0, 2, 3)), n, shift)
    xhat = (yd - mean.view(1, -1, 1, 1)) * torch.rsqrt(var + R.EPS32).view(1, -1, 1, 1)
    per = torch.cat([gz.sum((2, 3)), (gz * xhat).sum((2, 3))], 1)  # [B][32]: [S1 | S2] per image
    split = grows // Bn
    gsum = (per / split).repeat_interleave(split, 0)  # grows rows with the batch's column sums
    rows64 = torch.stack([R.conv_wgrad_rows(x.double(), dy64, 4 * r, 4 * r + 4)[0] for r in range(CH)], 1)
    assert torch.allclose(rows64.sum((0, 1))[:400],
                          torch.nn.grad.conv2d_weight(x.double(), (16, 1, 5, 5), dy64, padding=2).reshape(-1))
    dyt = dy64.to(dtype).to(DEV).reshape(Bn, 16, CH, 112).permute(0, 2, 1, 3).reshape(Bn * CH, 16, 112)
    colt = F.unfold(x.to(DEV), 5, padding=2).reshape(Bn, 25, CH, 112).permute(0, 2, 1, 3).reshape(Bn * CH, 25, 112)
    rows_t = torch.cat([torch.bmm(dyt, colt.transpose(1, 2)).reshape(Bn * CH, 400), dyt.sum(2)], 1)
    return dict(x=x, y=y1, dp=dp1, idx=idx, fstats=fstats, gamma=gamma, gsum=gsum, S=per.sum(0),
                rows64=rows64.reshape(Bn * CH, N1), rows_t=rows_t.double().cpu())


@LAUNCH
@DT
@pytest.mark.parametrize("Bn", [1, 3, 5])
def test_rows_match_float64(C, Bn, dtype, which):
    c = _fcase(Bn, dtype, _grows(C, Bn, dtype))
    rows, dg, dbe = _run(C, which, dtype, c, c["gsum"])
    rows = rows.double().cpu()
    r64, rt = c["rows64"], c["rows_t"]
    lp = dtype != torch.float32
    rel = lambda a, r: (a - r).norm(dim=-1) / (r.norm(dim=-1) + 1e-12)
    e = rel(rows[:, :400], r64[:, :400])
    lim = (2.0 * rel(rt[:, :400], r64[:, :400])).clamp_(min=2e-3 if lp else 1e-5)
    k = int((e / lim).argmax())
    print(f"B={Bn} {IDS[dtype]} {which} dW rows: worst row {k} (image {k // CH} chunk {k % CH}): "
          f"err {e[k].item():.3e} limit {lim[k].item():.3e}")
    RATIOS["b dW"] = max(RATIOS.get("b dW", 0.0), (e / lim).max().item())
    assert bool((e < lim).all()), ("dW", k, e[k].item(), lim[k].item())
    # bias columns: absolute, per row
    e = (rows[:, 400:] - r64[:, 400:]).abs().amax(1)
    lim = (4.0 if lp else 2.0) * (rt[:, 400:] - r64[:, 400:]).abs().amax(1) + (1e-2 if lp else 1e-4)
    k = int((e / lim).argmax())
    print(f"B={Bn} {IDS[dtype]} {which} db rows: worst row {k}: abs err {e[k].item():.3e} limit {lim[k].item():.3e}")
    RATIOS["b db"] = max(RATIOS.get("b db", 0.0), (e / lim).max().item())
    assert bool((e < lim).all()), ("db", k, e[k].item(), lim[k].item())
    # dgamma / dbeta: the column sums of gsum
    S = c["S"]
    assert torch.allclose(dbe.double().cpu(), S[:16], rtol=1e-5, atol=1e-5)
    assert torch.allclose(dg.double().cpu(), S[16:], rtol=1e-5, atol=1e-5)


# =============================================================================== c
@LAUNCH
@pytest.mark.parametrize("lrows", [None, 1, 3])
def test_dgamma_dbeta_sources(C, which, lrows):
    """Integer-valued sum rows: dg1 / dbe1 are the exact column sums of gsum, or of lsum when one is
    given -- and the slab rows follow gsum either way (bitwise the rows of the run without lsum)."""
    dtype, Bn = torch.bfloat16, 3
    c = R.conv1_wgrad_int(Bn, 40)
    g = torch.Generator().manual_seed(41)
    gsum = torch.randint(-20, 21, (_grows(C, Bn, dtype), 32), generator=g).double()
    base, dg0, dbe0 = _run(C, which, dtype, c, gsum)
    assert not bool(torch.isnan(base).any())
    src = gsum
    if lrows is not None:
        src = torch.randint(-20, 21, (lrows, 32), generator=g).double() + 100
        rows, dg0, dbe0 = _run(C, which, dtype, c, gsum, lsum=src)
        assert torch.equal(rows, base)
    assert torch.equal(dbe0.double().cpu(), src.sum(0)[:16]) and torch.equal(dg0.double().cpu(), src.sum(0)[16:])


# =============================================================================== d
def _plain(Bn, dtype):
    """A finite all-zero case of B images, built on the device."""
    n = float(Bn * 784)
    z = lambda *s: torch.zeros(*s, dtype=dtype, device=DEV)
    fstats = torch.zeros(49, device=DEV)
    fstats[16:33] = n
    return (z(Bn, 1, 28, 28), z(Bn, 16, 28, 28), z(Bn, 16, 14, 14),
            torch.zeros(Bn, 16, 14, 14, dtype=torch.uint8, device=DEV), fstats)


@pytest.mark.parametrize("Bn,dtype", [(b, d) for b in (1, 17, 32, 33) for d in R.DTYPES] + [(257, torch.bfloat16)],
                         ids=lambda v: IDS.get(v, str(v)))
def test_out2_column_sums(C, Bn, dtype):
    """out2 = int64 column sums of the conv2 slab (one row per image): B = 1 and 17 (the two-row
    path and its row clamp), 32 | 33 (the switch to the 16-row batch), 257 (its tail loop).
    N2 = 12832 is no multiple of 64: the last workgroup's column clamp runs in every case."""
    cn = C.convnet
    assert cn.wgrad_bn_rows(2, Bn) == Bn
    g = torch.Generator().manual_seed(Bn)
    slab = torch.randint(-8, 9, (Bn, N2), generator=g)
    assert int(slab.abs().sum(0).max()) < R.EXACT
    x, y, dp, idx, fstats = _plain(Bn, dtype)
    wslab1 = torch.empty(cn.wgrad_bn_rows(1, Bn) * N1, device=DEV)
    dg, dbe = torch.empty(16, device=DEV), torch.empty(16, device=DEV)
    gsum = torch.zeros(_grows(C, Bn, dtype) * 32, device=DEV)
    buf = torch.full((N2 + 16,), NAN, device=DEV)
    chk = _chk()
    cn.conv1_wgrad_slab2(x, y, dp, idx, fstats, gsum, None, torch.ones(16, device=DEV), EPS, dg, dbe, wslab1,
                         slab.float().to(DEV).reshape(-1), buf.narrow(0, 8, N2), None, chk)
    torch.cuda.synchronize()
    out = buf.cpu()
    assert bool(torch.isnan(out[:8]).all()) and bool(torch.isnan(out[-8:]).all())
    got, want = out[8:-8].double(), slab.sum(0).double()
    bad = got != want
    assert not bool(bad.any()), (int(bad.sum()), bad.nonzero()[:8].flatten().tolist(), got[bad][:4], want[bad][:4])
    assert int(chk[0]) == 0


# =============================================================================== e
def _chk_run(C, Bn, x=None, dp=None, wslab2=None, lsum=None, dtype=torch.bfloat16):
    cn = C.convnet
    x0, y, dp0, idx, fstats = _plain(Bn, dtype)
    idx.fill_(4)  # window position 0, ReLU open
    nwg1 = cn.wgrad_bn_rows(1, Bn)
    wslab1 = torch.full((nwg1 * N1,), NAN, device=DEV)
    dg, dbe = torch.empty(16, device=DEV), torch.empty(16, device=DEV)
    gsum = torch.zeros(_grows(C, Bn, dtype) * 32, device=DEV)
    if wslab2 is None:
        wslab2 = torch.zeros(Bn * N2, device=DEV)
    chk = _chk()
    cn.conv1_wgrad_slab2(x0 if x is None else x, y, dp0 if dp is None else dp, idx, fstats, gsum, lsum,
                         torch.ones(16, device=DEV), EPS, dg, dbe, wslab1, wslab2, torch.empty(N2, device=DEV), None, chk)
    torch.cuda.synchronize()
    return int(chk[0]), wslab1.view(nwg1, N1), dg


@pytest.mark.parametrize("col", [5, N2 - 1])
def test_check_word_conv2_column_overflow(C, col):
    """Finite rows whose column sums beyond FLT_MAX (the first workgroup, and the last real
    column of the clamped last one)."""
    slab = torch.zeros(2, N2, device=DEV)
    slab[:, col] = 3.0e38
    assert _chk_run(C, 2, wslab2=slab.reshape(-1))[0] != 0
    slab[1, col] = -3.0e38
    assert _chk_run(C, 2, wslab2=slab.reshape(-1))[0] == 0


@pytest.mark.parametrize("xval,flagged", [(1e8, True), (1e6, False)])
def test_check_word_conv1_weight_partial(C, xval, flagged):
    """One open window with dp = 1e30 and a constant image: the weight partials of the chunk
    holding the pixel are 1e30 * xval, finite, against the row bound FLT_MAX / 7 at B = 1;
    the bias partial (1e30) stays far inside it."""
    dt = torch.bfloat16
    dp = torch.zeros(1, 16, 14, 14, dtype=dt, device=DEV)
    dp[0, 3, 2, 2] = 1e30
    word, rows, _ = _chk_run(C, 1, x=torch.full((1, 1, 28, 28), xval, dtype=dt, device=DEV), dp=dp)
    assert bool(torch.isfinite(rows).all())
    assert rows[:, 400:].abs().max().item() < FLT_MAX / CH
    assert (rows[:, :400].abs().max().item() > FLT_MAX / CH) == flagged
    assert (word != 0) == flagged


def test_check_word_nonfinite_dgamma(C):
    """dg1 (the column sums of lsum) non-finite while every slab row is finite."""
    lsum = torch.zeros(3, 32, device=DEV)
    lsum[1, 16 + 2] = float("inf")
    word, rows, dg = _chk_run(C, 2, lsum=lsum.reshape(-1))
    assert bool(torch.isfinite(rows).all()) and bool(torch.isinf(dg[2]))
    assert word != 0
    assert _chk_run(C, 2, lsum=torch.zeros(96, device=DEV))[0] == 0


def test_zz_report_ratios():
    """Largest error / limit of section b (how much room the rule leaves)."""
    for k, v in sorted(RATIOS.items()):
        print(f"\nerror/limit maximum, section {k}: {v:.4f}", end="")
    assert all(v < 1 for v in RATIOS.values())
