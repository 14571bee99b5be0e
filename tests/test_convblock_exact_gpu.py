"""The per-layer conv-block kernels (csrc/kernels/convblock.hip, C.convblock), kernel by kernel:
exact on integer inputs, float64 per element on floats (reference: tests/_convblock_ref.py,
pure torch on the CPU; its generators' conditions are asserted in test_convblock_ref_cpu.py).

  a  conv_fwd      integers, with the BN partial sums (MODE 0) and without (MODE 1)
  b  conv_dgrad    integers (MODE 2, 16 <- 32 at 14x14)
  c  conv_wgrad    integers and one-pixel impulses on every tap (PRO 0)
  d  bn_relu_pool  float64 per element, ATen's argmax, the finalize from 1 .. 4G+1 slab rows
  e  bwd_reduce    exact S1, float64 S2, uneven batch splits
  f  bwd_elemt     float64 per element, every pixel written

The plain-input modes of conv5x5_body / conv5x5_wgrad_body run here are the same tile loops
as the fused step's: an element that differs is named by its index.  The largest error /
bound ratio of the float sections is printed by the last test.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from . import _bn_ref as B
from . import _convblock_ref as R
from . import _head_ref as HR

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
SENTINEL = 1000.0  # exact in the three types, outside every integer case's range
IDS = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
DT = pytest.mark.parametrize("dtype", R.DTYPES, ids=[IDS[d] for d in R.DTYPES])
RATIOS = {}


def _act(t, dtype):
    return t.to(dtype).to(DEV).contiguous()


def _f(t):
    return t.float().to(DEV).contiguous()


def _cpu(t):
    return t.detach().double().cpu()


def _same(got, want, name):
    got = _cpu(got).reshape(want.shape)
    bad = got != want  # NaN != anything: an unwritten element counts
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} of {want.numel()} differ, first at "
                                 f"{bad.nonzero()[0].tolist()}: got {got[bad][0].item()} want {want[bad][0].item()}")


def _within(got, ref, bnd, name, section, keep=None):
    """|got - ref| <= bnd on every (kept) element; NaN fails."""
    err = (_cpu(got).reshape(ref.shape) - ref).abs()
    bnd = bnd.expand_as(err)
    bad = ~(err <= bnd)
    if keep is not None:
        bad = bad & keep
        err, bnd = err[keep], bnd[keep]
    if err.numel() == 0:
        return
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd.clamp(min=1e-300))
    worst = float(ratio.max()) if not ratio.isnan().any() else float("inf")
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} outside the bound, first at {bad.nonzero()[0].tolist()}, "
                                 f"error / bound <= {worst:.3g}")
    if worst >= RATIOS.get(section, (0.0, ""))[0]:
        RATIOS[section] = (worst, name)


# =============================================================================== a
@pytest.mark.parametrize("stats", [True, False], ids=["stats", "eval"])
@DT
@pytest.mark.parametrize("Bn", [1, 3])
@pytest.mark.parametrize("layer", [1, 2])
def test_conv_fwd_integers(C, layer, Bn, dtype, stats):
    cb = C.convblock
    ci, co, H, W = R.LAYERS[layer]
    c = R.int_conv(layer, Bn, 10 * layer + Bn)
    yr, _ = R.conv_fwd(c["x"], c["w"], c["bias"])
    assert float(yr.abs().max()) <= R.INT_MAX[dtype]
    y = torch.full((Bn, co, H, W), SENTINEL, dtype=dtype, device=DEV)
    x, w, bias, shift = _act(c["x"], dtype), _f(c["w"]), _f(c["bias"]), _f(c["shift"])
    if not stats:
        cb.conv_fwd(x, w, bias, y)
        torch.cuda.synchronize()
        _same(y, yr, "y")
        return
    RL = cb.fslab_row(co)
    nrows = cb.fwd_rows(ci, co, H, W, Bn)
    assert nrows % Bn == 0 and RL == 2 * co + 1
    fslab = torch.full((nrows * RL,), NAN, device=DEV)
    fstats = torch.full((cb.stats_len(co),), NAN, device=DEV)
    cb.conv_fwd(x, w, bias, y, fslab, fstats, shift)
    torch.cuda.synchronize()
    _same(y, yr, "y")
    _same(fstats[2 * co + 1:], c["shift"], "fstats shift")
    rows = _cpu(fslab).view(Bn, nrows // Bn, RL)
    # the rows of an image (whichever pixels each owns) add up to the image's sums and count
    _same(rows.sum(1), R.fwd_stat_rows(yr, c["shift"]), "[sum | sumsq | count] per image")
    assert bool((rows[:, :, 2 * co] > 0).all())


# =============================================================================== b
@DT
@pytest.mark.parametrize("Bn", [1, 3])
def test_conv_dgrad_integers(C, Bn, dtype):
    c = R.int_dgrad(Bn, 20 + Bn)
    dxr, _ = R.conv_dgrad(c["dy"], c["w"])
    assert float(dxr.abs().max()) <= R.INT_MAX[dtype]
    dx = torch.full((Bn, 16, 14, 14), NAN, dtype=dtype, device=DEV)
    C.convblock.conv_dgrad(_act(c["dy"], dtype), _f(c["w"]), dx)
    torch.cuda.synchronize()
    _same(dx, dxr, "dx")


# =============================================================================== c
def _wgrad(C, layer, x, dy, dtype):
    cb = C.convblock
    ci, co, H, W = R.LAYERS[layer]
    Bn, row = x.shape[0], co * ci * 25 + co
    nrows = cb.wgrad_rows(ci, co, H, W, Bn)
    assert nrows % Bn == 0
    wslab = torch.full((nrows * row,), NAN, device=DEV)
    cb.conv_wgrad(_act(x, dtype), _act(dy, dtype), wslab)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(wslab).any()), torch.isnan(wslab).nonzero()[:8].flatten().tolist()
    return _cpu(wslab).view(Bn, nrows // Bn, row)


@DT
@pytest.mark.parametrize("Bn", [1, 3])
@pytest.mark.parametrize("layer", [1, 2])
def test_conv_wgrad_integers(C, layer, Bn, dtype):
    c = R.int_wgrad(layer, Bn, 30 * layer + Bn)
    want, _ = R.conv_wgrad_rows(c["x"], c["dy"])
    _same(_wgrad(C, layer, c["x"], c["dy"], dtype).sum(1), want, "[dW | db] per image")


@DT
@pytest.mark.parametrize("variant", [0, 1], ids=["dy-on-border", "x-on-border"])
@pytest.mark.parametrize("layer", [1, 2])
def test_conv_wgrad_impulses(C, layer, variant, dtype):
    """One non-zero dy pixel and one non-zero x pixel per image, image t on tap t: the slab holds
    exactly one non-zero weight partial per image, at that tap (and the one bias partial)."""
    ci = R.LAYERS[layer][0]
    x, dy, where = R.impulse_wgrad(layer, variant, 5 * layer + variant)
    rows = _wgrad(C, layer, x, dy, dtype)
    nw = rows.shape[2] - dy.shape[1]
    for t, (co, c_in, kh, kw, v, dv) in enumerate(where):
        nz = rows[t].abs().sum(0).nonzero().flatten().tolist()
        at = (co * ci + c_in) * 25 + kh * 5 + kw
        assert nz == [at, nw + co], (t, (kh, kw), nz, at)
        assert rows[t, :, at].sum().item() == v and rows[t, :, nw + co].sum().item() == dv, (t, kh, kw)


# =============================================================================== d
@functools.lru_cache(maxsize=None)
def _pool_case(layer, nrows, dtype):
    return R.pool_case(layer, 3, nrows, dtype, 7 * layer + nrows)


def _pool_run(C, c, dtype, fslab, momentum, train, nbt0=4):
    Bn, co, H, W = c["y"].shape
    y = _act(c["y"], dtype)
    fstats = torch.cat([torch.full((2 * co + 1,), NAN), c["shift"].float()]).to(DEV)
    rm, rv = _f(c["rm0"]), _f(c["rv0"])
    nbt = torch.tensor([nbt0], dtype=torch.long, device=DEV)
    p = torch.full((Bn, co, H // 2, W // 2), NAN, dtype=dtype, device=DEV)
    idx = torch.full((Bn, co, H // 2, W // 2), 255, dtype=torch.uint8, device=DEV)
    C.convblock.bn_relu_pool(y, fslab, fstats, _f(c["gamma"]), _f(c["beta"]), rm, rv, nbt, momentum, 1e-5, train, p, idx)
    torch.cuda.synchronize()
    return p, idx.cpu(), fstats, rm, rv, int(nbt)


def _pool_check(c, dtype, mean, invstd, p, idx, name):
    f = R.bn_relu_pool(c["y"], mean, invstd, c["gamma"], c["beta"], dtype)
    _, ind = F.max_pool2d(f["act"], 2, 2, return_indices=True)  # ATen on the reference's rounded activations
    W = c["y"].shape[3]
    aten = (((ind // W) % 2) * 2 + (ind % W) % 2).to(torch.uint8)
    assert torch.equal(aten, f["idx"])
    dec = R.pool_decided(f["z"], f["A"], c["y"], f["idx"], dtype)
    assert int((~dec).sum()) <= B.skip_allowance(dec.numel())
    bad = (idx != aten) & dec
    assert not bool(bad.any()), (f"{name} idx: {int(bad.sum())} windows differ from ATen's argmax, first at "
                                 f"{bad.nonzero()[0].tolist()}: got {idx[bad][0].item()} want {aten[bad][0].item()}")
    assert bool((idx <= 3).all())
    bw = R.windows(B.bound(f["A"], f["z"], dtype))
    bnd = torch.where(dec, bw.gather(-1, f["idx"].long().unsqueeze(-1)).squeeze(-1), bw.max(-1).values)
    _within(p, f["pz"], bnd, f"{name} p", "d")


@DT
@pytest.mark.parametrize("k", range(5), ids=["1", "G", "4G-1", "4G", "4G+1"])
@pytest.mark.parametrize("layer", [1, 2])
def test_bn_relu_pool_train(C, layer, k, dtype):
    """Training: the finalize from k slab rows (the 4-way unrolled loop and its remainder), the
    running statistics (momentum 0.1, or < 0: the cumulative average), then the pooling."""
    co = R.LAYERS[layer][1]
    G = 256 // (2 * co + 1)
    nrows = (1, G, 4 * G - 1, 4 * G, 4 * G + 1)[k]
    momentum = 0.1 if k % 2 == 0 else -1.0
    c = _pool_case(layer, nrows, dtype)
    nbt0 = 4
    p, idx, fstats, rm, rv, nbt = _pool_run(C, c, dtype, _f(c["rows"].reshape(-1)), momentum, True, nbt0)
    st = HR.bn_from_rows(c["rows"].double(), c["shift"], c["gamma"], c["beta"], R.EPS32, c["rm0"], c["rv0"],
                         R.MOM32 if momentum >= 0 else None, nbt0 + 1)
    name = f"layer {layer} {IDS[dtype]} rows {nrows}"
    _same(fstats[:2 * co + 1], st["sums"], f"{name} fstats sums")
    _same(fstats[2 * co + 1:], c["shift"], f"{name} fstats shift")
    assert nbt == nbt0 + 1
    _within(rm, st["rm"], B.bound(st["A_rm"], st["rm"], torch.float32), f"{name} running_mean", "d")
    _within(rv, st["rv"], B.bound(st["A_rv"], st["rv"], torch.float32), f"{name} running_var", "d")
    _pool_check(c, dtype, st["mean"], st["invstd"], p, idx, name)


@DT
@pytest.mark.parametrize("layer", [1, 2])
def test_bn_relu_pool_eval(C, layer, dtype):
    """Eval: the running statistics are used and nothing but p / idx is written."""
    co = R.LAYERS[layer][1]
    c = _pool_case(layer, 1, dtype)
    p, idx, fstats, rm, rv, nbt = _pool_run(C, c, dtype, None, 0.1, False)
    assert bool(torch.isnan(fstats[:2 * co + 1]).all()) and nbt == 4
    _same(rm, c["rm0"], "running_mean")
    _same(rv, c["rv0"], "running_var")
    _pool_check(c, dtype, c["rm0"], (c["rv0"] + R.EPS32).rsqrt(), p, idx, f"eval layer {layer} {IDS[dtype]}")


# =============================================================================== e
@DT
@pytest.mark.parametrize("Bn", [1, 3, 8, 9, 11])
@pytest.mark.parametrize("layer", [1, 2])
def test_bwd_reduce(C, layer, Bn, dtype):
    """bslab row s = the sums over the images [B s / ns, B (s + 1) / ns): S1 exact, S2 within
    16 u of its sum of magnitudes (at most two images, 392 windows, per row: two terms per
    lane, a 6-level wave tree, 3 adds across the waves, the product with invstd and rsqrtf).
    The image in the middle of the batch has p <= 0 everywhere and must contribute exactly 0."""
    cb = C.convblock
    co = R.LAYERS[layer][1]
    c = R.bwd_case(layer, Bn, 50 * layer + Bn, "int")
    p = c["p"].clone()
    if Bn >= 3:
        p[Bn // 2] = 0
    ns = cb.bwd_split(Bn)
    assert ns == min(Bn, 8)
    bslab = torch.full((ns * 2 * co,), NAN, device=DEV)
    cb.bwd_reduce(_act(c["dp"], dtype), _act(p, dtype), c["idx"].to(DEV), _act(c["y"], dtype), _f(c["fstats"]), 1e-5,
                  bslab)
    torch.cuda.synchronize()
    bw = R.bn_bwd(R.route(c["dp"], p, c["idx"]), c["y"], c["mean"], c["invstd"], c["gamma"])
    rng = [slice(Bn * s // ns, Bn * (s + 1) // ns) for s in range(ns)]
    per = lambda k: torch.stack([bw[k][r].sum(0) for r in rng])
    got = _cpu(bslab).view(ns, 2 * co)
    _same(got[:, :co], per("S1_rows"), "S1 rows")
    _within(got[:, co:], per("S2_rows"), B.bound(per("A2_rows"), per("S2_rows"), torch.float32),
            f"layer {layer} {IDS[dtype]} B {Bn} S2 rows", "e")
    if Bn >= 3:
        s = [i for i, r in enumerate(rng) if r == slice(Bn // 2, Bn // 2 + 1)]
        assert s and bool((got[s[0]] == 0).all())


# =============================================================================== f
@DT
@pytest.mark.parametrize("grows", [1, 3, 8])
@pytest.mark.parametrize("layer", [1, 2])
def test_bwd_elemt(C, layer, grows, dtype):
    co = R.LAYERS[layer][1]
    Bn = 3
    c = R.bwd_case(layer, Bn, 70 * layer + grows, "float")
    dp, p, y = (R.rounded(c[k], dtype) for k in ("dp", "p", "y"))
    g = torch.Generator().manual_seed(grows)
    gslab = torch.randint(-40, 41, (grows, 2 * co), generator=g).double() / 8  # exact column sums
    dx = torch.full(tuple(y.shape), NAN, dtype=dtype, device=DEV)
    C.convblock.bwd_elemt(_act(dp, dtype), _act(p, dtype), c["idx"].to(DEV), _act(y, dtype), _f(c["fstats"]),
                          _f(gslab.reshape(-1)), _f(c["gamma"]), 1e-5, dx)
    torch.cuda.synchronize()
    S = gslab.sum(0)
    ref, A = R.bn_dx(R.route(dp, p, c["idx"]), y, c["mean"], c["invstd"], c["gamma"], S[:co], S[co:], float(c["n"]))
    _within(dx, ref, B.bound(A, ref, dtype), f"layer {layer} {IDS[dtype]} gslab rows {grows} dx", "f")


def test_zz_report_ratios():
    """Largest observed error / bound per float section (how much room the bounds leave)."""
    for k, (v, name) in sorted(RATIOS.items()):
        print(f"\nerror/bound maximum, section {k}: {v:.4f} ({name})", end="")
    assert all(v <= 1 for v, _ in RATIOS.values())
