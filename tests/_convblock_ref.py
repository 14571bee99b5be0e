"""Float64 / integer reference of the 5x5 conv-block kernels and the input generators of
tests/test_convblock_exact_gpu.py, test_conv1_wgrad_gpu.py and test_slab_sums_gpu.py.  Pure
torch on the CPU, written out from the formulas (the convolution as an im2col product, not
through conv2d; tests/test_convblock_ref_cpu.py checks it against autograd through
conv2d -> batch_norm(training) -> relu -> max_pool2d).

  csrc/kernels/convblock.hip      conv_fwd, conv_dgrad, conv_wgrad, bn_relu_pool, bwd_reduce,
                                  bwd_elemt, slab_reduce (the per-layer op, C.convblock)
  csrc/kernels/conv5x5_wgrad.h    conv5x5_wgrad_body with BN1 backward applied on the fly
                                  (C.convnet.conv_wgrad_bn layer 1, conv1_wgrad_slab2)

Integer cases hold integers (or multiples of 1/2) in float64, far below 2^53: float64
arithmetic on them is integer arithmetic, and the int64 sums below are taken on .long().
A case is exact in fp32 for ANY summation order when the sum of the magnitudes of the terms
of every output is below 2^24 (every partial sum is then an integer below 2^24); the
generators return that sum next to the value and tests/test_convblock_ref_cpu.py asserts it.

Tolerance model of the float checks: tests/_bn_ref.py (bound, storage, near_zero,
skip_allowance) and tests/_head_ref.py (bn_from_rows: the BN finalize from slab rows).

The pooling index of C.convblock.bn_relu_pool is the position 0..3 in the 2x2 window
((dy, dx) scan order, first maximum wins, as ATen's max_pool2d); the fused path's byte adds
4 where the pooled value is > 0 (_head_ref.bn_relu_pool).
"""
import torch
import torch.nn.functional as F

from . import _bn_ref as B
from . import _head_ref as HR

U32 = B.U32
EPS32 = HR.EPS32
MOM32 = HR.MOM32
LAYERS = {1: (1, 16, 28, 28), 2: (16, 32, 14, 14)}  # (CIN, COUT, H, W) of the two instantiations
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
EXACT = 2 ** 24
# integers every storage type holds exactly: bf16 has 8 significand bits
INT_MAX = {torch.float32: 2 ** 24, torch.bfloat16: 2 ** 8, torch.float16: 2 ** 11}


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def rounded(t, dtype):
    return t.to(dtype).double()


# ------------------------------------------------------------------------- convolution
def unfold5(x):
    """[B][CIN][H][W] -> [B][CIN * 25][H * W], rows in (ci, kh, kw) order, zero padding 2."""
    return F.unfold(x, 5, padding=2)


def conv_fwd(x, w, bias):
    """(y, A): y[b][co] = w[co] . unfold(x[b]) + bias[co]; A the sum of |terms|."""
    Bn, _, H, W = x.shape
    co = w.shape[0]
    wm = w.reshape(co, -1)
    y = wm @ unfold5(x) + bias.view(1, -1, 1)
    A = wm.abs() @ unfold5(x.abs()) + bias.abs().view(1, -1, 1)
    return y.reshape(Bn, co, H, W), A.reshape(Bn, co, H, W)


def conv_dgrad(dy, w):
    """(dx, A): the transposed convolution, dx = fold(w^T . dy)."""
    Bn, co, H, W = dy.shape
    wm = w.reshape(co, -1)
    fold = lambda a, b: F.fold(a.t() @ b.reshape(Bn, co, H * W), (H, W), 5, padding=2)
    return fold(wm, dy), fold(wm.abs(), dy.abs())


def conv_wgrad_rows(x, dy, lo=0, hi=None):
    """Per image [dW (co, ci, kh, kw) | db] from the output rows [lo, hi) alone, and the sums
    of |terms|: ([B][COUT * CIN * 25 + COUT], same)."""
    Bn, co, H, W = dy.shape
    hi = H if hi is None else hi
    sl = slice(lo * W, hi * W)
    d = dy.reshape(Bn, co, H * W)[:, :, sl]
    rows = lambda dd, cols: torch.cat([torch.bmm(dd, cols[:, :, sl].transpose(1, 2)).reshape(Bn, -1), dd.sum(2)], 1)
    return rows(d, unfold5(x)), rows(d.abs(), unfold5(x.abs()))


def fwd_stat_rows(y, shift):
    """Per image [sum(y - shift) | sum((y - shift)^2) | count]: [B][2C + 1]."""
    d = y - shift.view(1, -1, 1, 1)
    cnt = torch.full((y.shape[0], 1), float(y.shape[2] * y.shape[3]), dtype=y.dtype)
    return torch.cat([d.sum((2, 3)), (d * d).sum((2, 3)), cnt], 1)


# --------------------------------------------------------------- BN -> ReLU -> MaxPool
def windows(t):
    """[B][C][H][W] -> [B][C][H/2][W/2][4], window order (0,0), (0,1), (1,0), (1,1)."""
    Bn, C, H, W = t.shape
    return t.reshape(Bn, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(Bn, C, H // 2, W // 2, 4)


def unwindows(t):
    """Inverse of windows."""
    Bn, C, HO, WO, _ = t.shape
    return t.reshape(Bn, C, HO, WO, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(Bn, C, 2 * HO, 2 * WO)


def first_max(zw):
    """Position of the first maximum of the last dimension."""
    four = torch.arange(zw.shape[-1]).expand_as(zw)
    return torch.where(zw == zw.max(-1, keepdim=True).values, four, torch.full_like(four, zw.shape[-1])).min(-1).values


def bn_relu_pool(y, mean, invstd, gamma, beta, dtype):
    """The kernel's form z = (y - mean) * (gamma * invstd) + beta.  Returns a dict:
    z (unrounded float64, full resolution), A (|t| + |beta|, full resolution), act (z rounded to
    the storage type, then ReLU), p / idx (2x2 max of act, first maximum wins), pz (the max of
    the UNROUNDED relu(z): what the per-element bound is taken against)."""
    v = lambda t: t.view(1, -1, 1, 1)
    t = (y - v(mean)) * v(gamma * invstd)
    z = t + v(beta)
    A = t.abs() + v(beta).abs().expand_as(t)
    act = rounded(z, dtype).clamp(min=0)
    aw = windows(act)
    idx = first_max(aw)
    return dict(z=z, A=A, act=act, p=aw.max(-1).values, idx=idx.to(torch.uint8),
                pz=windows(z.clamp(min=0)).max(-1).values)


def pool_decided(z, A, y, idx, dtype):
    """Windows whose argmax no kernel within _bn_ref.bound of z can decide otherwise: with
    [lo_k, hi_k] = relu(z_k -+ bound_k), every earlier candidate lies strictly below the
    winner's interval and every later one not above it (or is the same input value, which
    any kernel maps to the same activation).  The others are the near ties, exempt from the
    index check as the near-zero pre-activations of the bn_nhwc tests (_bn_ref.near_zero)."""
    bnd = B.bound(A, z, dtype)
    lo, hi, yw = windows((z - bnd).clamp(min=0)), windows((z + bnd).clamp(min=0)), windows(y)
    k = idx.long().unsqueeze(-1)
    lo_w, y_w = lo.gather(-1, k), yw.gather(-1, k)
    pos = torch.arange(4).expand_as(lo)
    ok = torch.where(pos < k, hi < lo_w, (hi <= lo_w) | (yw == y_w) | (pos == k))
    return ok.all(-1)


def route(dp, p, idx):
    """Pooled gradient through max-pool and ReLU: full-resolution dz (dp at the argmax of the
    windows whose pooled output is > 0, else 0)."""
    g = torch.where(p > 0, dp, torch.zeros_like(dp))
    one = F.one_hot(idx.long(), 4).to(dp.dtype)
    return unwindows(one * g.unsqueeze(-1))


def rows_of(t):
    """[B][C][H][W] -> [B*H*W][C] (the layout of _bn_ref)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def like_of(r, t):
    Bn, C, H, W = t.shape
    return r.reshape(Bn, H, W, C).permute(0, 3, 1, 2)


def bn_bwd(dz, y, mean, invstd, gamma):
    """_bn_ref.bn_bwd on [B][C][H][W]: S1, S2 (= dbeta, dgamma), dx and its A; plus the
    per-image sums S1_rows / S2_rows [B][C] and their sums of magnitudes."""
    r = B.bn_bwd(rows_of(dz), rows_of(y), mean, invstd, gamma)
    xh = (y - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)
    return dict(S1=r["S1"], S2=r["S2"], dx=like_of(r["dx"], y), A=like_of(r["A"], y),
                S1_rows=dz.sum((2, 3)), S2_rows=(dz * xh).sum((2, 3)),
                A1_rows=dz.abs().sum((2, 3)), A2_rows=(dz * xh).abs().sum((2, 3)))


def bn_dx(dz, y, mean, invstd, gamma, S1, S2, n):
    """(dx, A) of dx = gamma * invstd * (dz - S1 / n - xhat * S2 / n) on [B][C][H][W]."""
    dx, A = B.bn_dx(rows_of(dz), rows_of(y), mean, invstd, gamma, S1, S2, n)
    return like_of(dx, y), like_of(A, y)


def fstats_of(s1, s2, n, shift):
    """The final statistics buffer [s1 | s2 | n | shift] (stats_len(C) = 3C + 1 floats)."""
    return torch.cat([s1, s2, torch.tensor([float(n)], dtype=s1.dtype), shift])


# ---------------------------------------------------------------- integer generators
def int_conv(layer, Bn, seed):
    """x, w, bias, shift of conv_fwd.  Layer 1 (25 terms): x, w, bias in [-2, 2], |y| <= 102.
    Layer 2 (400 terms): weights in {-1, 0, 1}, x in [-2, 2] on a quarter of the pixels."""
    ci, co, H, W = LAYERS[layer]
    g = _gen(seed)
    if layer == 1:
        x = torch.randint(-2, 3, (Bn, ci, H, W), generator=g)
        w = torch.randint(-2, 3, (co, ci, 5, 5), generator=g)
    else:
        x = torch.randint(-2, 3, (Bn, ci, H, W), generator=g) * (torch.randint(0, 4, (Bn, ci, H, W), generator=g) == 0)
        w = torch.randint(-1, 2, (co, ci, 5, 5), generator=g)
    bias = torch.randint(-2, 3, (co,), generator=g)
    shift = torch.randint(-2, 3, (co,), generator=g)
    return dict(x=x.double(), w=w.double(), bias=bias.double(), shift=shift.double())


def int_dgrad(Bn, seed):
    """dy in [-2, 2] on a quarter of the pixels, w in {-1, 0, 1} ([32][16][5][5])."""
    g = _gen(seed)
    dy = torch.randint(-2, 3, (Bn, 32, 14, 14), generator=g) * (torch.randint(0, 4, (Bn, 32, 14, 14), generator=g) == 0)
    return dict(dy=dy.double(), w=torch.randint(-1, 2, (32, 16, 5, 5), generator=g).double())


def int_wgrad(layer, Bn, seed):
    """x and dy in [-3, 3]."""
    ci, co, H, W = LAYERS[layer]
    g = _gen(seed)
    return dict(x=torch.randint(-3, 4, (Bn, ci, H, W), generator=g).double(),
                dy=torch.randint(-3, 4, (Bn, co, H, W), generator=g).double())


def impulse_wgrad(layer, variant, seed):
    """25 images, image t for tap t = (kh, kw): ONE non-zero dy pixel (channel co, at (h, w))
    and ONE non-zero x pixel (channel ci, at (h + kh - 2, w + kw - 2)), so the image's weight
    gradient is the single value dy * x at [co][ci][kh][kw] (and db[co] = dy).  Variant 0
    puts the dy pixel on the image border (last row / column for kh, kw <= 2, else the
    first), variant 1 the x pixel (first row / column for kh, kw <= 2, else the last).
    Returns x, dy and per image (co, ci, kh, kw, value, dy value)."""
    ci_n, co_n, H, W = LAYERS[layer]
    g = _gen(seed)
    x, dy, where = torch.zeros(25, ci_n, H, W), torch.zeros(25, co_n, H, W), []
    for t in range(25):
        kh, kw = t // 5, t % 5
        if variant == 0:
            h, w = (H - 1 if kh <= 2 else 0), (W - 1 if kw <= 2 else 0)
        else:
            h, w = (2 - kh if kh <= 2 else H - 1 - (kh - 2)), (2 - kw if kw <= 2 else W - 1 - (kw - 2))
        co, ci = int(torch.randint(0, co_n, (1,), generator=g)), int(torch.randint(0, ci_n, (1,), generator=g))
        dv, xv = (float(torch.randint(1, 4, (1,), generator=g)) * (-1) ** t), float(torch.randint(1, 4, (1,), generator=g))
        dy[t, co, h, w] = dv
        x[t, ci, h + kh - 2, w + kw - 2] = xv
        where.append((co, ci, kh, kw, dv * xv, dv))
    return x.double(), dy.double(), where


def int_slab_rows(total, nrows, seed, lo=-50, hi=50):
    """nrows integer rows whose column sums are ``total`` (int64 [n]): random integers in
    [lo, hi], the last row takes the remainder."""
    rows = torch.zeros(nrows, total.numel(), dtype=torch.long)
    if nrows > 1:
        rows[:-1] = torch.randint(lo, hi + 1, (nrows - 1, total.numel()), generator=_gen(seed))
    rows[-1] = total - rows[:-1].sum(0)
    return rows


def pool_case(layer, Bn, nrows, dtype, seed):
    """Inputs of bn_relu_pool.  The statistics are GIVEN as integer slab rows (exact column
    sums s1, s2, n for any order) and are independent of y: per channel sigma in [0.5, 2],
    |s1 / n| <= 1/16 and a shift in {-1/16, 0, 1/16}, so |mean| <= sigma / 4 and the rounding
    of the fp32 mean = shift + s1 / n stays below the |beta| term of A (_bn_ref docstring).
    y = mean + sigma * normal, rounded to the
    storage type; in an eighth of the windows one pixel repeats another (exact ties) and a
    window whose argmax is not decided (pool_decided) is overwritten with copies of its first
    pixel, so the reference alone stays within the skip allowance (asserted on the CPU)."""
    _, C, H, W = LAYERS[layer]
    g = _gen(seed)
    n = Bn * H * W
    sigma = 0.5 + 1.5 * torch.rand(C, generator=g, dtype=torch.float64)
    s1 = torch.randint(-(n // 16), n // 16 + 1, (C,), generator=g)
    s2 = (n * (sigma ** 2 + (s1.double() / n) ** 2)).round().long()
    shift = torch.randint(-1, 2, (C,), generator=g).double() / 16
    total = torch.cat([s1, s2, torch.tensor([n])])
    rows = int_slab_rows(total, nrows, seed + 1)
    st = HR.bn_from_rows(rows.double(), shift, None, None, EPS32)
    gamma, beta = B.float_affine(C, seed + 2)
    gamma, beta = rounded(gamma, torch.float32), rounded(beta, torch.float32)
    y = st["mean"].view(1, -1, 1, 1) + sigma.view(1, -1, 1, 1) * torch.randn(Bn, C, H, W, generator=g, dtype=torch.float64)
    yw = windows(rounded(y, dtype)).clone()
    dup = torch.randint(0, 8, yw.shape[:-1], generator=g) == 0
    src, dst = torch.randint(0, 4, yw.shape[:-1], generator=g), torch.randint(0, 4, yw.shape[:-1], generator=g)
    yw.scatter_(-1, dst.unsqueeze(-1), torch.where(dup, yw.gather(-1, src.unsqueeze(-1)).squeeze(-1),
                                                   yw.gather(-1, dst.unsqueeze(-1)).squeeze(-1)).unsqueeze(-1))
    y = unwindows(yw)
    r = bn_relu_pool(y, st["mean"], st["invstd"], gamma, beta, dtype)
    und = ~pool_decided(r["z"], r["A"], y, r["idx"], dtype)
    yw = torch.where(und.unsqueeze(-1), yw[..., :1].expand_as(yw), yw)
    rm0 = rounded(st["mean"] + 0.1 * sigma * torch.randn(C, generator=g, dtype=torch.float64), torch.float32)
    rv0 = rounded(sigma ** 2 * (0.8 + 0.4 * torch.rand(C, generator=g, dtype=torch.float64)), torch.float32)
    return dict(y=unwindows(yw).contiguous(), rows=rows, shift=shift, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0,
                n=n, ties=int(dup.sum()) + int(und.sum()))


def bwd_case(layer, Bn, seed, kind):
    """Inputs of bwd_reduce (kind 'int') and bwd_elemt (kind 'float').
    int: dp in [-3, 3], y in [-4, 4], integer mean (s1 = 0: mean = shift in [-2, 2]), so
    S1 = sum g is an integer sum and g * (y - mean) an exact integer before the one product
    with invstd; p in {0, 1, 2} (a third of the windows closed).
    float: normal dp / y rounded to the storage type by the caller; s1 = 0 again, so the
    fp32 mean is the shift itself (no cancellation error outside A, _bn_ref docstring)."""
    _, C, H, W = LAYERS[layer]
    g = _gen(seed)
    n = Bn * H * W
    shift = torch.randint(-2, 3, (C,), generator=g).double()
    sigma = 0.5 + 1.5 * torch.rand(C, generator=g, dtype=torch.float64)
    s2 = rounded(n * sigma ** 2, torch.float32)
    fstats = fstats_of(torch.zeros(C, dtype=torch.float64), s2, n, shift)
    idx = torch.randint(0, 4, (Bn, C, H // 2, W // 2), generator=g).to(torch.uint8)
    if kind == "int":
        dp = torch.randint(-3, 4, idx.shape, generator=g).double()
        p = torch.randint(0, 3, idx.shape, generator=g).double()
        y = torch.randint(-4, 5, (Bn, C, H, W), generator=g).double()
    else:
        dp = torch.randn(idx.shape, generator=g, dtype=torch.float64)
        p = torch.randn(idx.shape, generator=g, dtype=torch.float64).clamp(min=0)
        y = shift.view(1, -1, 1, 1) + sigma.view(1, -1, 1, 1) * torch.randn(Bn, C, H, W, generator=g, dtype=torch.float64)
    gamma = rounded(B.float_affine(C, seed + 1)[0], torch.float32)
    mean, var, invstd = B.moments_from_sums(fstats[:C], s2, float(n), shift, EPS32)
    return dict(dp=dp, p=p, idx=idx, y=y, fstats=fstats, gamma=gamma, mean=mean, invstd=invstd, n=n)


def conv1_wgrad_int(Bn, seed):
    """Integer case of the conv1 weight gradient with BN1 backward on the fly: all-zero BN sums
    (k1 = k2 = 0), fstats1 = [0 | n (1 - eps) | n | 0] (invstd = 1 to a few fp32 ulp), gamma in
    {+-1, +-2, +-1/2}, dp1 in [-3, 3], random idx bytes 0..7, x in [-3, 3], finite random y1.
    dy = gamma * g is a multiple of 1/2 of magnitude <= 6 (exact in the three types)."""
    g = _gen(seed)
    n = Bn * 784
    x = torch.randint(-3, 4, (Bn, 1, 28, 28), generator=g).double()
    dp = torch.randint(-3, 4, (Bn, 16, 14, 14), generator=g).double()
    idx = torch.randint(0, 8, (Bn, 16, 14, 14), generator=g).to(torch.uint8)
    y = torch.randn(Bn, 16, 28, 28, generator=g, dtype=torch.float64)
    gamma = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5, -0.5], dtype=torch.float64)[torch.randint(0, 6, (16,), generator=g)]
    z = torch.zeros(16, dtype=torch.float64)
    fstats = fstats_of(z, rounded(torch.full((16,), n * (1.0 - EPS32), dtype=torch.float64), torch.float32), n, z)
    dy = route(dp, ((idx & 4) != 0).double(), idx & 3) * gamma.view(1, -1, 1, 1)
    return dict(x=x, dp=dp, idx=idx, y=y, gamma=gamma, fstats=fstats, dy=dy, n=n)
