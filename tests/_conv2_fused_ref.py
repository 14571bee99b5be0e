"""Integer cases and float64 references of the fused conv2 launches (csrc/kernels/convnet_fused.hip):

  conv2_fwd        BN1 from the slab -> ReLU -> pool1 in the prologue of conv5x5_body (PRO 1), conv2,
                   the BN2 partial rows, one per (image, split)
  conv_wgrad_bn /  BN2 / ReLU / pool2 backward on the fly, then conv5x5_wgrad_body NSL: one slab row
  conv2_bwd        per image, written by 2 * WG2_NSL workgroups
  conv2_bwd /      the data-gradient role (PRO 2, EPI 1) in fp32
  conv2_dgrad

for tests/test_conv2_fused_ref_cpu.py (every condition the generators rely on) and
tests/test_conv2_fused_exact_gpu.py.  Pure torch on the CPU, on the helpers of _convblock_ref.py.

The integer prologue.  The BN statistics are GIVEN: all-zero first-moment sums (mean = shift, an
integer, exactly) and a second moment of n (forward: integer slab rows whose columns sum to
[0 | n | n]) or n (1 - eps) (backward: one fstats buffer), so var + eps = 1 + eps or 1 and
invstd = 1 - 5e-6 or 1 to a few fp32 ulp.  With gamma a power of two, integer y1 and beta = +-1/2
the forward's z = gamma (y1 - shift) invstd + beta lies within |t| 6e-6 of a half-integer that is
never 0 (|gamma| >= 1), far inside the rounding interval of bf16 / fp16 at that value: the stored
activations are half-integers, exactly, and every later sum is exact in fp32 in any order while the
sums of magnitudes stay below 2^24 in units of the grid (1/2; 1/4 for the squares).

fp32 stores nothing rounded, so the operands reach the 16x16x4 MFMA with the coefficient's error
intact; there the float64 reference uses the true invstd and the comparison is within

    K u A,   u = 2^-24,  A the sum of the magnitudes of the terms,

K counted from the fp32 operations, first order in u, one line per constant:

  invstd   rsqrtf(fl(var + eps)): the addition's 1/2 u (the root halves its u) + rsqrtf's 1 ulp = 2 u
           -> 2.5 u; forward var = n / n - 0 is exact; backward var = fl(n (1 - eps)) / n carries 2 u
           more, halved -> 3.5 u
  K_PRO 8  forward z = fl(fl(t sc) + beta), sc = gamma invstd exact (gamma a power of two):
           2.5 + 1 + 1 = 4.5 u of A_z = |t sc| + |beta| (3.5 u if the compiler contracts the two
           operations into one FMA); xhat = fl(t invstd): 3.5 u of |t|.  8 covers both with slack
  K_Y2     y2 = 400 products + bias.  A is built from A_z, not from |p1|, so it already carries the
           operand's magnitude: K_PRO u A for the operands, and 400 additions, each rounding a
           partial sum of magnitude <= A (products with w in {-1, 0, 1} are exact): 400 + K_PRO
  K_S1     slab row sum over <= 64 pixels of d = fl(v - shift): K_Y2 for v, 1 for the subtraction,
           64 additions, all of sum(A + |shift|): K_Y2 + 1 + 64
  K_S2     sum of d^2: d^2 has twice d's relative error (2 (K_Y2 + 1)) plus the product's 1, then 64
           additions, all of sum((A + |shift|)^2): 2 (K_Y2 + 1) + 1 + 64
  K_WG     backward dy = fl(gi g), gi = gamma invstd (k1 = k2 = 0 exactly): 3.5 + 1, taken as 8 (as
           tests/test_conv1_wgrad_gpu.py section a); 196 pixels per image row: 196 + 8
  K_DG     data gradient, 800 terms of dy: 800 + 8
  K_Q1/2   quarter rows of the data gradient over <= 64 pixels: K_DG + 64 additions; S2 has the
           product with xhat, 1 more
"""
import torch

from . import _convblock_ref as R
from . import _dgrad_rows as Q
from . import _head_ref as HR

U32 = R.U32
EPS32 = R.EPS32
MT, HW2 = 13, 196
N2 = 32 * 400 + 32
GAMMAS_FWD = (1.0, -1.0, 2.0, -2.0)
GAMMAS_BWD = (1.0, -1.0, 2.0, -2.0, 0.5, -0.5)
TMAX = 6  # |y1 - shift| of the forward cases
LP = (torch.bfloat16, torch.float16)

K_PRO = 8
K_Y2 = 400 + K_PRO
K_S1 = K_Y2 + 1 + 64
K_S2 = 2 * (K_Y2 + 1) + 1 + 64
K_WG = 196 + 8
K_DG = 800 + 8
K_Q1 = K_DG + 64
K_Q2 = K_DG + 1 + 64


# ------------------------------------------------------------------------ the split map
def win_rows(H, W, nsplit, even):
    """conv5x5_win_rows of csrc/kernels/conv5x5.h, transcribed line by line."""
    hw, mt = H * W, (H * W + 15) // 16
    mx = 0
    for sp in range(nsplit):
        p0, p1e = 16 * (mt * sp // nsplit), 16 * (mt * (sp + 1) // nsplit)
        p1 = min(p1e, hw)
        if p1 <= p0:
            return 0
        lo, hi = max(p0 // W - 2, 0), min((p1 - 1) // W + 2, H - 1)
        if even:
            lo, hi = lo & ~1, hi | 1
        mx = max(mx, hi - lo + 1)
    return mx


def split_pixels(sp, ns):
    """Output pixels [p0, p1) of workgroup sp of ns: m-tiles [13 sp / ns, 13 (sp + 1) / ns) of 16,
    clipped at 196.  Its slab row is b * ns + sp."""
    lo, hi = Q.split_range(sp, ns)
    return 16 * lo, min(16 * hi, HW2)


def split_window(sp, ns):
    """Input (pooled) rows [lo, hi] workgroup sp stages: its output rows and two halo rows each side."""
    p0, p1 = split_pixels(sp, ns)
    return max(p0 // 14 - 2, 0), min((p1 - 1) // 14 + 2, 13)


# ------------------------------------------------------------------------ forward
def fwd_int(Bn, seed, nrows=None):
    """Inputs of conv2_fwd.  u = sign(gamma) (y1 - shift) is in [-6, -1] except on 7 % of the pixels,
    where it is 0, 1 or 2: z = |gamma| u + beta > 0 on about a quarter of the windows, p1 <= 4.5.  In an
    eighth of the windows one pixel repeats another (ties between positive candidates; the windows with
    nothing positive tie at 0 in all four)."""
    g = R._gen(seed)
    n = Bn * 784
    pick = lambda vals, k: torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), (k,), generator=g)]
    gamma, beta = pick(GAMMAS_FWD, 16), pick((0.5, -0.5), 16)
    shift = torch.randint(-2, 3, (16,), generator=g).double()
    shp = (Bn, 16, 28, 28)
    u = torch.randint(-TMAX, 0, shp, generator=g)
    u = torch.where(torch.rand(shp, generator=g) < 0.07, torch.randint(0, 3, shp, generator=g), u).double()
    uw = R.windows(u).clone()
    sel = uw.shape[:-1]
    dup = torch.randint(0, 8, sel, generator=g) == 0
    src, dst = torch.randint(0, 4, sel, generator=g).unsqueeze(-1), torch.randint(0, 4, sel, generator=g).unsqueeze(-1)
    uw.scatter_(-1, dst, torch.where(dup.unsqueeze(-1), uw.gather(-1, src), uw.gather(-1, dst)))
    v = lambda t: t.view(1, -1, 1, 1)
    y1 = v(shift) + R.unwindows(uw) * v(gamma.sign())
    nrows = 4 * Bn if nrows is None else nrows
    total = torch.cat([torch.zeros(16, dtype=torch.long), torch.full((17,), n, dtype=torch.long)])
    rows1 = R.int_slab_rows(total, nrows, seed + 1)
    w2 = torch.randint(-1, 2, (32, 16, 5, 5), generator=g).double()
    bias2 = torch.randint(-2, 3, (32,), generator=g).double()
    rm2 = torch.randint(-2, 3, (32,), generator=g).double()
    # running statistics of BN1 before the launch: far from (shift, n / (n - 1)), so an update that is
    # skipped or applied twice moves them by 0.1 |rm0 - shift| >= 0.3 or 0.09 of it
    rm0 = shift + pick((3.0, -3.0, 4.5, -5.25), 16)
    rv0 = pick((2.5, 3.0, 0.25, 4.75), 16)
    return dict(B=Bn, n=n, y1=y1.contiguous(), rows1=rows1, shift1=shift, gamma=gamma, beta=beta, w2=w2, bias2=bias2,
                rm2=rm2, rm0=rm0, rv0=rv0, ties=int(dup.sum()))


def fwd_impulse(variant, ns):
    """25 images, image t for tap t = (kh, kw): ONE positive window, so one non-zero pooled pixel
    (channel t % 16, value v - 1/2), and sparse weights -- w2[co_t][t % 16] is non-zero at tap t alone --
    so the image's output is the single weight times the pixel at (co_t, h - kh + 2, w - kw + 2), plus,
    for the images t and t + 16 that share an input channel, the other one's weight at its own pixel.
    variant 0: the OUTPUT pixel is the first or the last pixel of a workgroup's range.  A workgroup's
    row window is its output rows plus two halo rows each side, so only the taps kh = 0 (from the range's
    first row) and kh = 4 (from its last row) can read the window's border row at all: for kh = 0 the
    output pixel is a range's first pixel and the input lies ON the window's first row, for kh = 4 a
    range's last pixel and the input ON the window's last row; the taps kh = 1..3 take either edge, their
    input one or two rows inside the border (the window spans the image's width: its border columns are
    the image's, variant 1).  variant 1: the INPUT pixel is on the
    image border (row / column 0 for kh, kw <= 2, else 13).  gamma = 1, beta = -1/2, shift = 0, bias = 0.
    Returns the case and per image (co, oh, ow, value)."""
    g = R._gen(77 + variant)
    firsts = [split_pixels(sp, ns)[0] for sp in range(ns)]
    lasts = [split_pixels(sp, ns)[1] - 1 for sp in range(ns)]
    y1, w2, where = torch.zeros(25, 16, 28, 28), torch.zeros(32, 16, 5, 5), []
    cos = torch.randperm(32, generator=g)[:25].tolist()
    for t in range(25):
        kh, kw = t // 5, t % 5
        if variant == 0:
            edges = firsts if kh == 0 else (lasts if kh == 4 else [p for pair in zip(firsts, lasts) for p in pair])
            for k in range(len(edges)):
                oh, ow = divmod(edges[(t + k) % len(edges)], 14)
                h, w = oh + kh - 2, ow + kw - 2
                if 0 <= h < 14 and 0 <= w < 14:
                    break
            else:
                raise AssertionError(t)
        else:
            h, w = (0 if kh <= 2 else 13), (0 if kw <= 2 else 13)
        ci, co = t % 16, cos[t]
        v, wv = float(torch.randint(1, 4, (1,), generator=g)), float(torch.randint(1, 4, (1,), generator=g)) * (-1) ** t
        y1[t, ci, 2 * h + (t % 4) // 2, 2 * w + t % 2] = v
        w2[co, ci, kh, kw] = wv
        where.append((co, h - kh + 2, w - kw + 2, wv * (v - 0.5)))
    n = 25 * 784
    total = torch.cat([torch.zeros(16, dtype=torch.long), torch.full((17,), n, dtype=torch.long)])
    one, z16 = torch.ones(16, dtype=torch.float64), torch.zeros(16, dtype=torch.float64)
    c = dict(B=25, n=n, y1=y1.double(), rows1=R.int_slab_rows(total, 5, 78), shift1=z16, gamma=one, beta=-0.5 * one,
             w2=w2.double(), bias2=torch.zeros(32, dtype=torch.float64), rm2=torch.zeros(32, dtype=torch.float64),
             rm0=z16 + 3.0, rv0=one * 2.5, ties=0)
    return c, where


def invstd_of(dtype, var=1.0):
    """The invstd of the reference: 1 where the storage type rounds the difference away (the CPU tests
    assert that it does), the true float64 value of rsqrt(var + eps) for fp32."""
    return 1.0 if dtype in LP else float((torch.tensor(var, dtype=torch.float64) + EPS32).rsqrt())


def fwd_ref(c, dtype, ns, coef=None):
    """What conv2_fwd writes: y2 (rounded once), p1 / idx1 byte / xh1, the B * ns slab rows
    [sum | sum of squares | count] of y2 - rm2 over each workgroup's pixels, and the sums of magnitudes
    the fp32 bounds are taken against (A_*).  coef: invstd (default invstd_of(dtype))."""
    Bn = c["B"]
    istd = invstd_of(dtype) if coef is None else coef
    lp = dtype in LP
    rnd = (lambda t: R.rounded(t, dtype)) if lp else (lambda t: t)
    v = lambda t: t.view(1, -1, 1, 1)
    t = c["y1"] - v(c["shift1"])
    ts = t * v(c["gamma"] * istd)
    z = ts + v(c["beta"])
    Az = ts.abs() + v(c["beta"]).abs().expand_as(ts)
    aw = R.windows(rnd(z).clamp(min=0))
    k = R.first_max(aw).unsqueeze(-1)
    p = aw.gather(-1, k).squeeze(-1)
    xh = rnd(R.windows(t * istd).gather(-1, k).squeeze(-1))
    Ap = torch.where(p > 0, R.windows(Az).gather(-1, k).squeeze(-1), torch.zeros_like(p))
    idx = (k.squeeze(-1) | torch.where(p > 0, 4, 0)).to(torch.uint8)
    y2, _ = R.conv_fwd(p, c["w2"], c["bias2"])
    _, A = R.conv_fwd(Ap, c["w2"], c["bias2"])  # |w| . A_z + |bias| >= the sum of |terms|
    y2r = rnd(y2)
    d = (y2r - v(c["rm2"])).reshape(Bn, 32, HW2)
    Ad = (A + v(c["rm2"]).abs()).reshape(Bn, 32, HW2)
    rows, Ar = torch.zeros(Bn, ns, 65, dtype=torch.float64), torch.zeros(Bn, ns, 65, dtype=torch.float64)
    for sp in range(ns):
        p0, p1 = split_pixels(sp, ns)
        rows[:, sp, :32], rows[:, sp, 32:64], rows[:, sp, 64] = d[:, :, p0:p1].sum(-1), (d[:, :, p0:p1] ** 2).sum(-1), p1 - p0
        Ar[:, sp, :32], Ar[:, sp, 32:64] = Ad[:, :, p0:p1].sum(-1), (Ad[:, :, p0:p1] ** 2).sum(-1)
    # A_rows: [sum(A + |shift|) | sum((A + |shift|)^2) | 0] (K_S1, K_S2; the count is exact)
    return dict(y2=y2r, A_y2=A, p1=p, A_p1=Ap, xh1=xh, A_xh1=xh.abs(), idx1=idx, z=z, A_z=Az,
                rows=rows.reshape(Bn * ns, 65), A_rows=Ar.reshape(Bn * ns, 65), d=d)


def fwd_running(c):
    """BN1's running statistics after ONE update (momentum 0.1, unbiased variance) and their A terms."""
    return HR.bn_from_rows(c["rows1"].double(), c["shift1"], None, None, EPS32, c["rm0"], c["rv0"], HR.MOM32)


# ------------------------------------------------------------------------ weight gradient
def pick_gamma(k, g):
    return torch.tensor(GAMMAS_BWD, dtype=torch.float64)[torch.randint(0, 6, (k,), generator=g)]


def bwd_fstats(n):
    """[0 | n (1 - eps) | n | 0] of BN2: invstd = 1 to a few fp32 ulp."""
    z = torch.zeros(32, dtype=torch.float64)
    return R.fstats_of(z, R.rounded(torch.full((32,), n * (1.0 - EPS32), dtype=torch.float64), torch.float32), n, z)


def wgrad_int(Bn, seed):
    """The layer-2 analogue of _convblock_ref.conv1_wgrad_int: all-zero backward sums, dp2 in [-3, 3],
    idx2 bytes 0..7, p1 in {0, 1, 2}, finite random y2.  dy = gamma g is a multiple of 1/2, |dy| <= 6.
    lsum: integer rows the launch's dgamma / dbeta are the column sums of."""
    g = R._gen(seed)
    p1 = torch.randint(0, 3, (Bn, 16, 14, 14), generator=g).double()
    dp = torch.randint(-3, 4, (Bn, 32, 7, 7), generator=g).double()
    idx = torch.randint(0, 8, (Bn, 32, 7, 7), generator=g).to(torch.uint8)
    y = torch.randn(Bn, 32, 14, 14, generator=g, dtype=torch.float64)
    gamma = pick_gamma(32, g)
    lsum = torch.randint(-20, 21, (3, 64), generator=g).double() + 100
    dy = R.route(dp, ((idx & 4) != 0).double(), idx & 3) * gamma.view(1, -1, 1, 1)
    return dict(B=Bn, p1=p1, dp2=dp, idx2=idx, y2=y, gamma=gamma, fstats2=bwd_fstats(Bn * 196), dy=dy, lsum=lsum)


def wgrad_impulse(variant, co, ci, seed):
    """_convblock_ref.impulse_wgrad's placement for layer 2 with dy produced by the prologue: image t
    has ONE open pooling window of channel co (dp2 = dv, the argmax at the dy pixel, gamma = 1) and ONE
    p1 pixel of channel ci, so its slab row is dv * xv at [co][ci][kh][kw] and dv at db[co], 0 elsewhere.
    Returns the case and per image (column of dW, value, db value)."""
    g = R._gen(seed)
    p1, dp = torch.zeros(25, 16, 14, 14), torch.zeros(25, 32, 7, 7)
    idx = torch.randint(0, 4, (25, 32, 7, 7), generator=g).to(torch.uint8)  # every other window closed
    where = []
    for t in range(25):
        kh, kw = t // 5, t % 5
        if variant == 0:
            h, w = (13 if kh <= 2 else 0), (13 if kw <= 2 else 0)
        else:
            h, w = (2 - kh if kh <= 2 else 13 - (kh - 2)), (2 - kw if kw <= 2 else 13 - (kw - 2))
        dv = float(torch.randint(1, 4, (1,), generator=g)) * (-1) ** t
        xv = float(torch.randint(1, 3, (1,), generator=g))
        dp[t, co, h // 2, w // 2] = dv
        idx[t, co, h // 2, w // 2] = 4 | ((h % 2) * 2 + w % 2)
        p1[t, ci, h + kh - 2, w + kw - 2] = xv
        where.append(((co * 16 + ci) * 25 + t, dv * xv, dv))
    y = torch.randn(25, 32, 14, 14, generator=g, dtype=torch.float64)
    gamma = torch.ones(32, dtype=torch.float64)
    dy = R.route(dp.double(), ((idx & 4) != 0).double(), idx & 3)
    c = dict(B=25, p1=p1.double(), dp2=dp.double(), idx2=idx, y2=y, gamma=gamma, fstats2=bwd_fstats(25 * 196), dy=dy,
             lsum=torch.zeros(1, 64, dtype=torch.float64))
    return c, where


def wgrad_ref(c):
    """(rows [B][12832], A) = [dW | db] per image and the sums of |terms|."""
    return R.conv_wgrad_rows(c["p1"], c["dy"])


# ------------------------------------------------------------------------ data gradient (fp32)
def dgrad_int(Bn, seed):
    """The integer case of tests/test_dgrad_rows_gpu.py::_int_case (any dtype): dy = gamma g through
    the BN2 backward prologue, w2 in {-1, 0, 1}; idx1 / xh1 of the block below random (xh1 integer)."""
    bc = R.bwd_case(2, Bn, seed, "int")
    w2 = R.int_dgrad(Bn, seed + 1)["w"]
    g = R._gen(seed + 2)
    gamma = pick_gamma(32, g)
    idx2 = (bc["idx"] | (4 * (bc["p"] > 0)).to(torch.uint8)).contiguous()
    dy = R.route(bc["dp"], bc["p"], bc["idx"]) * gamma.view(1, -1, 1, 1)
    idx1 = torch.randint(0, 8, (Bn, 16, 14, 14), generator=g).to(torch.uint8)
    xh1 = torch.randint(-2, 3, (Bn, 16, 14, 14), generator=g).double()
    p1 = torch.randint(0, 3, (Bn, 16, 14, 14), generator=g).double()
    return dict(B=Bn, y2=bc["y"], dp2=bc["dp"], idx2=idx2, fstats2=bwd_fstats(Bn * 196), gamma=gamma, w2=w2, dy=dy,
                idx1=idx1, xh1=xh1, p1=p1)


def dgrad_ref(c):
    """dp1 and the 4 B quarter rows [S1 | S2] (fp32: nothing is rounded), with their A terms."""
    dp1, A = R.conv_dgrad(c["dy"], c["w2"])
    opened = ((c["idx1"] & 4) != 0).double()
    return dict(dp1=dp1, A=A, rows=Q.quarter_rows(dp1 * opened, c["xh1"]),
                A_rows=Q.quarter_rows(A * opened, c["xh1"].abs()))
