"""Float64 reference of the channels-last BatchNorm kernels (csrc/kernels/bn_nhwc.hip) and the
input generators of tests/test_bn_nhwc_exact_gpu.py.  Pure torch on the CPU, no GPU, and
written out from the formulas (not through nn.BatchNorm2d; tests/test_bn_nhwc_ref_cpu.py
checks it against that module).  Activations are rows [M][C] (M = N*H*W), float64.

Tolerance model of the per-element checks: with the fp32 unit roundoff u = 2^-24,

    |got - ref| <= 16 u A + q |ref|

A: sum of the magnitudes of the terms of the formula (returned next to every value below);
16 u: a short fp32 chain plus the 1-2 ulp of rsqrtf; q: storage rounding (Q: 0 for fp32;
2^-8 for bf16, which is its unit roundoff (8 significand bits), so a value on a rounding tie
uses the whole term; 2^-10 for fp16, twice its unit roundoff; below fp16's smallest normal the
format rounds absolutely and the term is 2^-24, see storage()).  The recomputed ReLU mask
may differ from the float64 one only where the float64 pre-activation lies within 16 u A of
0 (near_zero); at most SKIP_CAP of a case may be skipped.

The y bound leaves out the terms in |mean| of the kernels' fma form y = fma(x, s, b),
b = beta - mean*s: b is rounded once (u |mean * s|) and the fp32 mean = shift + s1/n carries
u (|shift| + |s1/n|) |s|.  The generators keep them below the |beta| term of A: the float
ones have |mean| / std <= 1/4, a shift within 0.35 std of it, |beta| >= 1/4 and |gamma| <=
3/2; the integer ones |beta| >= 1/2, |shift| <= 2 and no constant channel (|mean| / std <= 5
at two rows).  A constant channel (var = 0, invstd = eps^-1/2) carries u |mean| eps^-1/2 in
fp32 and is outside what A describes; the conditioning of the statistics themselves is the
subject of section (c) of the GPU module.
"""
import torch

U32 = 2.0 ** -24
Q = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}
VEC = {torch.float32: 4, torch.bfloat16: 8, torch.float16: 8}
EPS = 1e-5
SKIP_CAP = 1e-3  # share of a case's elements the masked checks may skip

# section (b) of the GPU module: rows of (N, H, W) = (3, 7, 9) and (1, 1, 2), these channels
ELEM_ROWS = (189, 2)
ELEM_C = (8, 24, 72, 320)
ELEM_C_BIG = 2048  # one bf16 case


# "one row block" cases of section (b): ELEM_ROWS[0] rows under set_grid_targets(1, 1, 1), where
# every active lane walks at least one full pass of U rows and some lane a tail row as well
# (tests/test_bn_nhwc_ref_cpu.py checks that from geom; one exception, below)
ONE_BLOCK_CASES = ((torch.float32, 72), (torch.bfloat16, 72), (torch.float16, 24), (torch.bfloat16, 320))
# (fp16, 24) is one chunk of 3 lanes per row, RP = 85: 189 rows are 2-3 rows per lane, tail rows
# only.  It runs (a row block of tails alone), and fp16 gets its pass + tail from C = 72.
ONE_BLOCK_TAIL_ONLY = ((torch.float16, 24),)
ONE_BLOCK_EXTRA = ((torch.float16, 72),)
STATS_ONE_BLOCK = (torch.float32, 64, 189)  # (dtype, C, M) with a pass and a tail row in the statistics kernels
THR, U, UF, MAXGR = 256, 4, 8, 1024  # csrc/kernels/bn_nhwc.hip


def geom(M, ch, target, dtype, cc=64):
    """(row blocks, channel chunks, rows per pass RP, rows per row block, active lanes) of
    chunk_grid / Chunk / row_range (cc 64: the statistics kernels; 256: the elementwise ones)."""
    vec = VEC[dtype]
    while cc > vec and not (ch <= cc or ch % cc == 0):
        cc //= 2
    ccw = ch if ch <= cc else cc
    lr = ccw // vec
    rp, gc = THR // lr, ch // ccw
    gr = min(max(1, -(-M // (rp * U))), max(1, -(-target // gc)), MAXGR)
    return gr, gc, rp, -(-M // gr), rp * lr


def lane_walk(rows, rp, u):
    """Per row offset ro < RP of a row block of ``rows`` rows: (passes of u rows, tail rows)."""
    out = []
    for ro in range(rp):
        n = len(range(ro, rows, rp))
        out.append((n // u, n % u))
    return out


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def rounded(t, dtype):
    """t as the storage type holds it, back in float64."""
    return t.to(dtype).double()


# ---------------------------------------------------------------------------- reference
def fwd_sums(x, shift):
    """(s1, s2, n): per-channel sum(x - shift), sum((x - shift)^2), row count."""
    d = x - shift
    return d.sum(0), (d * d).sum(0), x.shape[0]


def moments_from_sums(s1, s2, n, shift, eps=EPS):
    """mean, biased variance, invstd from sums around a shift (the apply kernels' formula)."""
    m1 = s1 / n
    var = (s2 / n - m1 * m1).clamp(min=0)
    return shift + m1, var, (var + eps).rsqrt()


def batch_moments(x, eps=EPS):
    """mean, biased variance, invstd, two-pass."""
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return mean, var, (var + eps).rsqrt()


def running_update(rm, rv, mean, var, n, momentum, nbt):
    """torch semantics: unbiased variance into running_var; momentum None = cumulative
    average with nbt = num_batches_tracked after this batch."""
    mom = float(momentum) if momentum is not None else 1.0 / float(nbt)
    unb = var * (n / max(n - 1.0, 1.0))
    return (1 - mom) * rm + mom * mean, (1 - mom) * rv + mom * unb


def bn_y(x, mean, invstd, gamma, beta, res=None, relu=False):
    """(y, pre-activation, A)."""
    t = (x - mean) * invstd * gamma
    pre = t + beta
    A = t.abs() + beta.abs()
    if res is not None:
        pre = pre + res
        A = A + res.abs()
    return (pre.clamp(min=0) if relu else pre), pre, A


def relu_mask(act, y=None, pre=None):
    """1/0 ReLU derivative: act 0 none, 1 from the stored y, 2 from the pre-activation."""
    if act == 0:
        return None
    return ((y if act == 1 else pre) > 0).double()


def bn_dx(dz, x, mean, invstd, gamma, S1, S2, n):
    """(dx, A) of dx = gamma*invstd * (dz - S1/n - xhat * S2/n)."""
    xh = (x - mean) * invstd
    gi, k1, k2 = gamma * invstd, S1 / n, S2 / n
    dx = gi * (dz - k1 - xh * k2)
    A = gi.abs() * (dz.abs() + k1.abs() + (xh * k2).abs())
    return dx, A


def bn_bwd(dy, x, mean, invstd, gamma, mask=None):
    """dz, S1 = sum dz, S2 = sum dz*xhat, dgamma, dbeta, dx, dres (= dz), A (of dx)."""
    dz = dy if mask is None else dy * mask
    xh = (x - mean) * invstd
    S1, S2 = dz.sum(0), (dz * xh).sum(0)
    dx, A = bn_dx(dz, x, mean, invstd, gamma, S1, S2, x.shape[0])
    return dict(dz=dz, S1=S1, S2=S2, dgamma=S2, dbeta=S1, dx=dx, dres=dz, A=A)


def tail_fwd(x, r, mean, invstd, gamma, beta, rmean, rinvstd, rgamma, rbeta):
    """relu(bn(x) + bn_r(r)): (y, pre-activation, A)."""
    _, p, A = bn_y(x, mean, invstd, gamma, beta)
    _, rp, rA = bn_y(r, rmean, rinvstd, rgamma, rbeta)
    pre = p + rp
    return pre.clamp(min=0), pre, A + rA


def tail_bwd(dy, y, x, r, mean, invstd, gamma, rmean, rinvstd, rgamma):
    """Backward of tail_fwd: (bn_bwd of the main BN, bn_bwd of the residual BN), both on
    dz = dy * (y > 0)."""
    m = relu_mask(1, y=y)
    main = bn_bwd(dy, x, mean, invstd, gamma, m)
    return main, bn_bwd(main["dz"], r, rmean, rinvstd, rgamma)


def near_zero(pre, A):
    """Elements whose mask the fp32 kernels may decide either way."""
    return pre.abs() <= 16 * U32 * A


def skip_allowance(numel):
    """How many elements of a case the masked checks may skip (0 below 1000 elements)."""
    return int(SKIP_CAP * numel)


def storage(ref, dtype):
    """Storage rounding of ``ref`` with the factor 2 margin: relative Q, except that fp16
    rounds absolutely below its smallest normal 2^-14 (half a subnormal spacing, 2^-25)."""
    s = Q[dtype] * ref.abs()
    return torch.where(ref != 0, s.clamp(min=2.0 ** -24), s) if dtype == torch.float16 else s


def bound(A, ref, dtype):
    return 16 * U32 * A + storage(ref, dtype)


# ------------------------------------------------------------------- integer generators
# x in {-3..3}, shift in {-2..2}: exact in bf16 / fp16 / fp32, (x - shift)^2 <= 25, so s1 and
# s2 are exact fp32 integers while 25 M < 2^24.  Backward: integer dy and y, integer means,
# invstd in {1/4, 1/2}, gamma in {-2..2}, beta on the half-integers: dz * xhat is a multiple
# of 1/4 of magnitude <= 7.5 (exact sums while 30 M < 2^24) and fma(x, gamma*invstd, b) is
# exact, 0 included.
def int_rows(M, C, seed, lo=-3, hi=3, distinct=False):
    x = torch.randint(lo, hi + 1, (M, C), generator=_gen(seed)).double()
    if distinct and M >= 2:  # no constant channel: row 1 differs from row 0
        x[1] = torch.where(x[1] == x[0], torch.where(x[0] >= hi, x[0] - 1, x[0] + 1), x[1])
    return x


def int_shift(C, seed):
    return torch.randint(-2, 3, (C,), generator=_gen(seed)).double()


def int_save(C, seed):
    """[mean | invstd]: integer means, invstd in {1/4, 1/2}."""
    g = _gen(seed)
    mu = torch.randint(-2, 3, (C,), generator=g).double()
    inv = torch.randint(1, 3, (C,), generator=g).double() / 4
    return torch.cat([mu, inv])


def int_affine(C, seed):
    """gamma in {-2..2} (zero and negative included), beta on the half-integers
    {-1.5, -0.5, 0.5, 1.5} (never 0: A >= 1/2 in the y bound)."""
    g = _gen(seed)
    return (torch.randint(-2, 3, (C,), generator=g).double(),
            (2 * torch.randint(-2, 2, (C,), generator=g).double() + 1) / 2)


def int_fwd_sums(x, shift):
    """int64 (s1, s2)."""
    d = x.long() - shift.long()
    return d.sum(0), (d * d).sum(0)


def int_bwd_sums(dy, x, save, mask=None):
    """(S1 int64, 4*S2 int64) for int_save-style statistics."""
    C = x.shape[1]
    dz = dy.long() if mask is None else dy.long() * mask.long()
    mu, is4 = save[:C].long(), (save[C:] * 4).long()
    return dz.sum(0), (dz * (x.long() - mu) * is4).sum(0)


# --------------------------------------------------------------------- float generators
def float_rows(M, C, seed, delta, sigma):
    """Normal rows standardised per channel in float64, then x = delta + sigma * z: the
    batch mean is delta and the biased batch std sigma (up to the storage rounding)."""
    z = torch.randn(M, C, generator=_gen(seed), dtype=torch.float64)
    z = z - z.mean(0)
    z = z / (z * z).mean(0).sqrt()
    return delta + sigma * z


def float_affine(C, seed):
    """|gamma| in [0.5, 1.5] of either sign, every 8th channel 0; |beta| in [0.25, 0.75]."""
    g = _gen(seed)
    sg = torch.randint(0, 2, (C,), generator=g).double() * 2 - 1
    sb = torch.randint(0, 2, (C,), generator=g).double() * 2 - 1
    gamma = sg * (0.5 + torch.rand(C, generator=g, dtype=torch.float64))
    beta = sb * (0.25 + 0.5 * torch.rand(C, generator=g, dtype=torch.float64))
    gamma[1::8] = 0
    return gamma, beta


def elem_inputs(kind, M, C, dtype, seed):
    """Inputs of one elementwise case, float64, activations already rounded to ``dtype`` and
    per-channel tensors to fp32: x, res, dy, y (a stored ReLU output for act 1), gamma, beta,
    rm0 / rv0 (running statistics; rm0 is also the statistics shift), save ([mean | invstd]
    handed to the backward kernels)."""
    f32 = torch.float32
    if kind == "int":
        x = int_rows(M, C, seed, distinct=True)
        res = int_rows(M, C, seed + 1)
        dy = int_rows(M, C, seed + 2)
        y = int_rows(M, C, seed + 3).clamp(min=0)
        gamma, beta = int_affine(C, seed + 4)
        rm0 = int_shift(C, seed + 5)
        rv0 = 2.0 + 4 * torch.rand(C, generator=_gen(seed + 6), dtype=torch.float64)
        save = int_save(C, seed + 7)
    else:
        g = _gen(seed + 8)
        sigma = 0.5 + 1.5 * torch.rand(C, generator=g, dtype=torch.float64)
        delta = sigma * (torch.rand(C, generator=g, dtype=torch.float64) - 0.5) * 0.5  # |delta| <= sigma / 4
        x = rounded(float_rows(M, C, seed, delta, sigma), dtype)
        res = rounded(torch.randn(M, C, generator=g, dtype=torch.float64), dtype)
        dy = rounded(torch.randn(M, C, generator=g, dtype=torch.float64), dtype)
        gamma, beta = float_affine(C, seed + 4)
        mean, _, invstd = batch_moments(x)
        rm0 = mean + 0.1 * sigma * torch.randn(C, generator=g, dtype=torch.float64)
        rv0 = sigma * sigma * (0.8 + 0.4 * torch.rand(C, generator=g, dtype=torch.float64))
        save = torch.cat([mean, invstd])
        y = None
    gamma, beta, rm0, rv0, save = (rounded(t, f32) for t in (gamma, beta, rm0, rv0, save))
    if y is None:  # the ReLU output a forward with this residual would have stored
        y = rounded(bn_y(x, save[:C], save[C:], gamma, beta, res, True)[0], dtype)
    return dict(x=x, res=res, dy=dy, y=y, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, save=save)


def elem_seed(dtype, C, M):
    return 1000 * list(Q).index(dtype) + 7 * C + M


def elem_cases():
    """(dtype, C) of section (b)."""
    return [(dt, C) for dt in Q for C in ELEM_C] + [(torch.bfloat16, ELEM_C_BIG)]
