"""Float64 reference of the classifier head kernels and the input generators of
tests/test_head_exact_gpu.py.  Pure torch on the CPU, written out from the formulas (not
through the nn modules; tests/test_head_ref_cpu.py checks it against them).

  csrc/kernels/head.hip           linear_fwd / linear_bwd, ce_fwd (three kernels), ce_bwd, accuracy
  csrc/kernels/convnet_fused.hip  head_fwd_kernel, head_bwd_kernel, fc_wgrad_body
  csrc/kernels/convnet_head.hip   head_row_kernel (forward + loss + backward in one launch)

Tolerance model, as tests/_bn_ref.py (u = 2^-24, the fp32 unit roundoff; Q the storage term):

    |got - ref| <= c u A + q |ref|

A is the sum of the magnitudes of the terms of the formula and is returned next to every
value; every c is counted from the fp32 roundings of the kernel's chain, here:

  dot products and sums (fc, dp2, the BN2 backward sums, the slab column sums)
      c = n + 2 for n terms (DOT): any summation order of n terms stays within (n - 1) u A,
      one more rounding for the products' own and one for a bias / final add.
  softmax gradient, valid while every |x_i - x_j| <= SPREAD = 16 (asserted by the generators)
      __expf(d) is v_exp_f32(d * log2e): the fp32 product d * log2e is off by u |d log2e|,
      which moves the exponential by ln2 * u * 16 * log2e = 16 u relative; the instruction adds
      about 2 u: 18 u.  The row sum of N <= 1024 such terms is at most 16 per-lane adds and a
      6-level shuffle tree: 22 adds, 24 u with the terms' own.  1 / se, sm = e * rs, (sm - oh),
      * inv and inv = 1 / count: 4 u.  Sum 18 + 18 + 24 + 4 = 64 on the softmax term.  The one-hot
      term oh = (1 - s) [n == t] + s / N is rounded in its operations ((1 - s) and the sum on
      the target, s / N elsewhere): 2 u.  The subtraction sm - oh, inv = 1 / count and the
      product by inv are roundings of the DIFFERENCE, so they act on oh as much as on sm: 3 u
      more on oh (the softmax term's 64 holds its share).  A first count gave oh 2 u only and
      was exceeded (by 10%) exactly where sm << oh: the wrong classes of a confident row under
      smoothing, and a target of softmax ~ 0.
          |dlog - ref| <= (64 u softmax_n + 5 u oh_n) / count                  (CE_SM, CE_OH)
  loss
      lse = mx + __logf(se): se within 42 u relative (above), the logarithm adds that
      absolutely plus 2 u |log se| <= 14 u; the additions lse, lse - x_t and the mean over the
      rows are each relative to values below 2 (max |logit|) + 7.  All of it stays below
          |loss - ref| <= 64 u (1 + max |logit|)                                (CE_LOSS)
      head_row_kernel adds every row as a multiple of 2^-24 (round to nearest: half a
      quantum each, and the mean of the halves is half a quantum) and rounds the mean once
      more to fp32: FIX_Q = 2^-25 on top.
  BN2 finalize of the head (cb::bn_finalize) on exact integer sums
      mean = shift + s1 / n (2 roundings), var = s2 / n - m1^2 (4), running statistics
      (1 - mom) r + mom v with the unbiased factor (6 more): at most 12 of the terms of A,
      bounded with _bn_ref.bound's 16 u A.
  BN -> ReLU -> pool (cb::bn_relu_max4x), z = (y - mean) * (gamma * invstd) + beta
      invstd = rsqrtf(var + eps): var 4 u relative, the add u, the instruction 1 ulp = 2 u,
      halved by the root except the instruction's: <= 5 u; gamma * invstd one more, the product
      with (y - mean) and the sum with beta one each: c = 8 <= 16 u A with A = |t| + |beta|
      (_bn_ref.bound).  xhat = (y - mean) * invstd: c = 6 <= 16.

Generators (seeded CPU generators; tests/test_head_ref_cpu.py asserts their conditions):

  linear     integers in [-3, 3] for x, w, b, dout: with K <= 1056 every partial sum is an
             integer below 9 * 1056 + 3 < 2^24, so out, dx, dw, db are exact in fp32 whatever
             the wave split or tile order, and the integers themselves are exact in bf16 / fp16.
  cross entropy  logits are multiples of 1/8 in [-8, 8] (exact in the three dtypes; spread 16).
  accuracy   logits in {-2..2}: most rows tie on the maximum.
  ConvNet head  (head_inputs) y2 = m_c + d, integers, |d| <= 8 with sum d = 0 per channel (d is
             a shuffled [r, -r]), so the batch mean is the integer m_c; the statistics shift is
             m_c + delta_c, delta in {-1, 0, 1}, so s1 = -n delta and s2 = sum d^2 + n delta^2 are
             integers, split over the slab rows as random integers (the last row takes the
             remainder): exact column sums.  gamma = +-sqrt(var + eps) rounded to fp32, so
             gamma * invstd is within u of +-1 in float64 (negative on every fifth channel).
             beta is an odd multiple of 1/2: z = +-d + beta is a half-integer, never within 1/4
             of the ReLU threshold, exact in bf16 / fp16 (|z| <= 10.5), and in those types
             the fp32 z, within 16 u A of it, rounds to exactly it.  Window values are equal or
             at least 1 apart.  fc weights are multiples of 1/64 in [-1/16, 1/16] (15 of 16 are
             zero, which keeps the logit spread below 16), biases small integers: every logit
             partial sum is a multiple of 2^-7 below 2^11, exact in fp32.
"""
import torch

from . import _bn_ref as B

U32 = B.U32
Q = B.Q
EPS32 = float(torch.tensor(1e-5, dtype=torch.float32))  # the eps the kernels see ((float)1e-5)
MOM32 = float(torch.tensor(0.1, dtype=torch.float32))
SPREAD = 16.0
CE_SM, CE_OH, CE_LOSS = 64.0, 5.0, 64.0
FIX_Q = 2.0 ** -25
HC, HH, HW, HP = 32, 14, 14, 49  # the ConvNet head's channels, map and pooled positions
HK = HC * HP


def DOT(n):
    return n + 2.0


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def rounded(t, dtype):
    return t.to(dtype).double()


def dot_bound(n, A, ref, dtype):
    """(n + 2) u A + q |ref|."""
    return DOT(n) * U32 * A + B.storage(ref, dtype)


# ------------------------------------------------------------------------------ linear
def linear(x, w, b=None):
    """(out, A): out[M][N] = x[M][K] . w[N][K]^T + b."""
    out, A = x @ w.t(), x.abs() @ w.abs().t()
    if b is not None:
        out, A = out + b, A + b.abs()
    return out, A


def linear_bwd(dout, x, w):
    """dx[M][K] = dout . w, dw[N][K] = dout^T . x, db[N] = sum_m dout."""
    return dout @ w, dout.t() @ x, dout.sum(0)


# ----------------------------------------------------------------------- cross entropy
def cross_entropy(logits, target, ignore_index=-100, smoothing=0.0, scale=None):
    """Mean cross entropy over the rows whose target is not ignore_index, with label smoothing.
    Returns (loss, dlog[B][N], A_loss, A_dlog):
      loss   NaN when no row counts, or when a counted row's target is outside [0, N);
             at smoothing 0 the smoothing term is absent (a -inf logit off the target leaves
             the loss finite, as torch), at smoothing > 0 such a logit gives +inf;
      dlog   d(scale * loss)/dlogits = scale * (softmax - oh) / count on a counted row, oh =
             (1 - s) [n == t] + s / N (an out-of-range target has no n == t); exactly 0 on an
             ignored row;
      A_loss 1 + max |finite logit|;
      A_dlog (softmax / count, oh / count) * scale, the two terms of dlog_bound."""
    Bn, N = logits.shape
    s = float(smoothing)
    sc = 1.0 if scale is None else float(scale)
    counted = target != ignore_index
    count = int(counted.sum())
    mx = logits.max(1, keepdim=True).values
    e = (logits - mx).exp()
    se = e.sum(1, keepdim=True)
    lse = (mx + se.log()).squeeze(1)
    sm = e / se
    valid = counted & (target >= 0) & (target < N)
    tt = torch.where(valid, target, torch.zeros_like(target))
    onehot = torch.zeros_like(logits)
    onehot[valid, tt[valid]] = 1.0
    xt = torch.where(valid, logits.gather(1, tt.view(-1, 1)).squeeze(1), torch.full_like(lse, float("nan")))
    row = (1.0 - s) * (lse - xt)
    if s > 0:
        row = row + s * (lse - logits.sum(1) / N)
    loss = row[counted].sum() / count if count > 0 else torch.tensor(float("nan"), dtype=logits.dtype)
    oh = (1.0 - s) * onehot + s / N
    inv = 1.0 / count if count > 0 else 0.0
    keep = counted.view(-1, 1).to(logits.dtype)
    dlog = (sm - oh) * inv * keep * sc
    fin = logits[logits.isfinite()]
    A_loss = 1.0 + (float(fin.abs().max()) if fin.numel() else 0.0)
    return loss, dlog, A_loss, (sm * inv * keep * abs(sc), oh * inv * keep * abs(sc))


def dlog_bound(A_dlog):
    return U32 * (CE_SM * A_dlog[0] + CE_OH * A_dlog[1])


def loss_bound(A_loss, fixed_point=False):
    return CE_LOSS * U32 * A_loss + (FIX_Q if fixed_point else 0.0)


def argmax_first(logits):
    """Index of the first maximal element of each row (0 for a row of -inf, as torch)."""
    N = logits.shape[1]
    ismax = logits == logits.max(1, keepdim=True).values
    return torch.where(ismax, torch.arange(N).expand_as(logits), torch.full_like(logits, N, dtype=torch.long)).min(1).values


def accuracy(logits, target):
    """(rows, rows whose first maximum is the target)."""
    return logits.shape[0], int((argmax_first(logits) == target).sum())


# ------------------------------------------------------------------------- ConvNet head
def bn_from_rows(rows, shift, gamma, beta, eps, rm=None, rv=None, momentum=None, nbt=1):
    """BN2 finalize from the slab rows [nrows][2C + 1] = [sum(y - shift) | sum((y - shift)^2) |
    count]: the column sums, mean / biased var / invstd, and (rm given) the running-statistics
    update with its A terms (momentum None: cumulative, nbt = batches tracked after this one)."""
    C = shift.numel()
    sums = rows.sum(0)
    s1, s2, n = sums[:C], sums[C:2 * C], float(sums[2 * C])
    mean, var, invstd = B.moments_from_sums(s1, s2, n, shift, eps)
    out = dict(sums=sums, n=n, mean=mean, var=var, invstd=invstd, gamma=gamma, beta=beta)
    if rm is not None:
        out["rm"], out["rv"] = B.running_update(rm, rv, mean, var, n, momentum, nbt)
        mom = float(momentum) if momentum is not None else 1.0 / float(nbt)
        m1 = s1 / n
        out["A_rm"] = abs(1 - mom) * rm.abs() + mom * (shift.abs() + m1.abs())
        out["A_rv"] = abs(1 - mom) * rv.abs() + mom * (s2 / n + m1 * m1) * (n / max(n - 1.0, 1.0))
    return out


def _windows(t):
    """[B][C][14][14] -> [B][C][7][7][4], window order (0,0), (0,1), (1,0), (1,1)."""
    Bn, C = t.shape[:2]
    return t.reshape(Bn, C, HH // 2, 2, HW // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(Bn, C, HH // 2, HW // 2, 4)


def bn_relu_pool(y2, mean, invstd, gamma, beta, dtype):
    """BN -> ReLU -> 2x2 max-pool in the kernel's form z = (y - mean) * (gamma * invstd) + beta,
    z rounded to the storage dtype, then ReLU; the first maximum wins.  Returns p [B][K], the
    idx byte (argmax | 4 where p > 0), xhat at the argmax, A_p = |t| + |beta| and A_xh = |xhat|
    (all [B][K], K = C * 49)."""
    v = lambda t: t.view(1, -1, 1, 1)
    t = (y2 - v(mean)) * v(gamma * invstd)
    z = rounded(t + v(beta), dtype).clamp(min=0)
    zw = _windows(z)
    best = zw.max(-1, keepdim=True).values
    four = torch.arange(4).expand_as(zw)
    arg = torch.where(zw == best, four, torch.full_like(four, 4)).min(-1, keepdim=True).values
    Bn = y2.shape[0]
    take = lambda w: w.gather(-1, arg).reshape(Bn, -1)
    p = best.reshape(Bn, -1)
    xhat = take(_windows((y2 - v(mean)) * v(invstd)))
    A_p = take(_windows(t.abs() + v(beta).abs().expand_as(t)))
    idx = (arg.reshape(Bn, -1) | torch.where(p > 0, 4, 0)).to(torch.uint8)
    return p, idx, xhat, A_p, xhat.abs()


def fc(p, w, b):
    """(logits, A): w already rounded to the compute dtype."""
    return linear(p, w, b)


def bn_bwd_rows(g, xhat):
    """Per-image BN2 backward sums of g [B][K]: S1 = sum g, S2 = sum g * xhat over the 49 pooled
    positions of each channel ([B][C]), and the sums of magnitudes A1, A2."""
    per = lambda t: t.reshape(t.shape[0], HC, HP).sum(-1)
    return per(g), per(g * xhat), per(g.abs()), per((g * xhat).abs())


def head_bwd(dlogits, w, p, idx, xhat, dtype):
    """fc backward and the BN2 backward sums: dp2 = dlogits . w (and its A), dW = dlogits^T . p,
    db, and with g = dp2 rounded to the storage dtype where the ReLU bit of idx is set:
    S1 = sum g, S2 = sum g * xhat per image ([B][C]) and over the batch ([C]), with A1 / A2 the
    sums of magnitudes per image.  (On the integer inputs of head_bwd_inputs every value is a
    multiple of 1/64 far below 2^53 / 64: float64 is exact, as integer arithmetic on 64 w.)"""
    dp2, A_dp2 = dlogits @ w, dlogits.abs() @ w.abs()
    g = rounded(dp2, dtype) * ((idx & 4) != 0).double()
    S1, S2, A1, A2 = bn_bwd_rows(g, xhat)
    return dict(dp2=dp2, A_dp2=A_dp2, dW=dlogits.t() @ p, db=dlogits.sum(0), S1_rows=S1, S2_rows=S2,
                A1_rows=A1, A2_rows=A2, S1=S1.sum(0), S2=S2.sum(0))


# --------------------------------------------------------------------------- generators
def lin_inputs(M, N, K, seed):
    g = _gen(seed)
    r = lambda *s: torch.randint(-3, 4, s, generator=g).double()
    return dict(x=r(M, K), w=r(N, K), b=r(N), dout=r(M, N))


LIN_SHAPES = ((1, 1, 8), (16, 16, 32), (17, 15, 36), (5, 3, 40), (33, 10, 1056), (7, 33, 100), (40, 65, 70))


def ce_logits(Bn, N, seed):
    """Multiples of 1/8 in [-8, 8]."""
    return torch.randint(-64, 65, (Bn, N), generator=_gen(seed)).double() / 8


def ce_targets(Bn, N, seed, ignored=0, ignore_index=-100):
    """Uniform targets; ignored: 0 none, an int k every k-th row (from row 1), 'all'."""
    t = torch.randint(0, N, (Bn,), generator=_gen(seed + 1))
    if ignored == "all":
        t[:] = ignore_index
    elif ignored:
        t[1::ignored] = ignore_index
    return t


def acc_inputs(Bn, N, seed):
    """Logits in {-2..2} (row B // 2 all -inf when B > 2); targets: the first maximum on about
    half the rows, a LATER tied maximum where there is one on about a quarter (must not
    count), uniform elsewhere."""
    g = _gen(seed)
    lg = torch.randint(-2, 3, (Bn, N), generator=g).double()
    if Bn > 2:
        lg[Bn // 2] = float("-inf")
    first = argmax_first(lg)
    ismax = lg == lg.max(1, keepdim=True).values
    last = torch.where(ismax, torch.arange(N).expand_as(lg), torch.full_like(lg, -1, dtype=torch.long)).max(1).values
    pick = torch.randint(0, 4, (Bn,), generator=g)
    t = torch.randint(0, N, (Bn,), generator=g)
    t = torch.where(pick < 2, first, t)
    t = torch.where(pick == 2, last, t)
    return lg, t


ACC_SHAPES = ((1, 1), (37, 10), (5, 65), (9, 1000), (259, 7))


def head_inputs(Bn, N, seed, nrows):
    """Inputs of the ConvNet head (see the module docstring), float64; per-channel tensors are
    fp32-representable."""
    g = _gen(seed)
    n = Bn * HH * HW
    r = torch.randint(-8, 9, (HC, n // 2), generator=g)
    d = torch.cat([r, -r], 1)
    d = d.gather(1, torch.rand(HC, n, generator=g).argsort(1))
    m = torch.randint(-3, 4, (HC,), generator=g)
    delta = torch.randint(-1, 2, (HC,), generator=g)
    y2 = (d + m.view(-1, 1)).reshape(HC, Bn, HH, HW).permute(1, 0, 2, 3).contiguous().double()
    shift = (m + delta).double()
    s1 = -n * delta
    s2 = (d * d).sum(1) + n * delta * delta
    tot = torch.cat([s1, s2, torch.tensor([n])])
    rows = torch.zeros(nrows, 2 * HC + 1, dtype=torch.long)
    if nrows > 1:
        rows[:-1, :HC] = torch.randint(-50, 51, (nrows - 1, HC), generator=g)
        rows[:-1, HC:2 * HC] = torch.randint(0, 101, (nrows - 1, HC), generator=g)
        rows[:-1, 2 * HC] = torch.randint(0, 2 * HH * HW, (nrows - 1,), generator=g)
    rows[-1] = tot - rows[:-1].sum(0)
    var = (d * d).sum(1).double() / n
    sign = torch.where(torch.arange(HC) % 5 == 3, -1.0, 1.0).double()
    gamma = (sign * (var + EPS32).sqrt()).float().double()
    beta = (2 * torch.randint(-3, 3, (HC,), generator=g).double() + 1) / 2
    rm0 = torch.randint(-4, 5, (HC,), generator=g).double() / 4
    rv0 = (1.0 + 3 * torch.rand(HC, generator=g, dtype=torch.float64)).float().double()
    nz = torch.randint(0, 16, (N, HK), generator=g) == 0
    wfc = torch.randint(-4, 5, (N, HK), generator=g).double() / 64 * nz
    bfc = torch.randint(-2, 3, (N,), generator=g).double()
    return dict(y2=y2, d=d, m=m.double(), shift=shift, rows=rows.double(), gamma=gamma, beta=beta, eps=EPS32,
                rm0=rm0, rv0=rv0, wfc=wfc, bfc=bfc, n=n)


def head_bwd_inputs(Bn, N, seed):
    """Integer inputs of head_bwd / fc_wgrad: dlogits in [-3, 3], p2 in [0, 10], xh2 in [-4, 4],
    random idx bytes (argmax 0..3 | ReLU bit), the fc weights of head_inputs."""
    g = _gen(seed)
    nz = torch.randint(0, 16, (N, HK), generator=g) == 0
    return dict(dl=torch.randint(-3, 4, (Bn, N), generator=g).double(),
                p2=torch.randint(0, 11, (Bn, HK), generator=g).double(),
                xh2=torch.randint(-4, 5, (Bn, HK), generator=g).double(),
                idx2=torch.randint(0, 8, (Bn, HK), generator=g).to(torch.uint8),
                wfc=torch.randint(-4, 5, (N, HK), generator=g).double() / 64 * nz)


HEAD_B = (1, 3, 33, 64)
HEAD_N = (1, 10, 11, 16)
HEAD_N_FWD = (17, 64)  # head_fwd only (its NMAX = 64 instance)


def head_seed(Bn, N):
    return 100 * Bn + N
