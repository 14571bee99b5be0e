"""Integer inputs and float64 CPU references for the implicit-GEMM convolution kernels
(csrc/kernels/conv_igemm.hip, conv_wgrad.hip).  No extension import: the CPU tier uses it.

The kernels multiply bf16 / fp16 operands and accumulate in fp32.  With small non-zero
integer operands every partial sum is an integer below 2^24 in magnitude, hence exact in
fp32 whatever the order, the tile shape, the pixel split or the MFMA adder's rounding; the
stored value is one round-to-nearest-even of a known integer and the fused sums are exact
too.  The expected outputs below are therefore expected BIT FOR BIT, and one missing,
duplicated or misplaced term moves an output by at least 1.

Regimes (``values``):
  small   x, w, dy in {-1, +1}: every output is an integer the storage type holds exactly;
  small2  as small with x in {+-1, +-2};
  large   bf16: x, w in {+-1, +-2, +-3}; fp16: {+-1 .. +-15} (the same recipe scaled so that
          the outputs pass 2048, where fp16 starts to round integers): the storage rounding,
          ties included, is exercised and the expected value is still y64.float().to(dtype).

``build(case)`` returns the inputs (float64 CPU tensors holding integers, NCHW shapes), the
expected outputs and ``pre``: the quantities that make the case exact, which
``check_preconditions`` compares with their limits.  These are conditions on the inputs,
not tolerances: a case that misses one gets other inputs, never another limit.
"""
import functools
import zlib

import torch
import torch.nn.functional as F

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
INT_EXACT = {"bf16": 256, "f16": 2048}  # every integer of at most this magnitude is representable
F32_EXACT = float(1 << 24)
F16_MAX = 65504.0
D = torch.float64


def values(regime, dtype):
    """(x values, w values) of a regime."""
    pm = lambda n: tuple(v for i in range(1, n + 1) for v in (-i, i))  # noqa: E731
    if regime == "small":
        return pm(1), pm(1)
    if regime == "small2":
        return pm(2), pm(1)
    assert regime == "large", regime
    return (pm(3), pm(3)) if dtype == "bf16" else (pm(15), pm(15))


def ints(shape, vals, g):
    """Uniform draws from a list of NON-ZERO integers (every term then matters), float64."""
    assert len(vals) > 0 and all(float(v) != 0.0 for v in vals), vals
    v = torch.tensor([float(a) for a in vals], dtype=D)
    return v[torch.randint(0, len(vals), tuple(shape), generator=g)]


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def out_hw(H, W, R, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1


# ---- the operations, float64 -----------------------------------------------------------
def conv(x, w, stride, pad):
    return F.conv2d(x.to(D), w.to(D), None, stride, pad)


def store(y64, dtype):
    """Cvt<T>::from_f of an exact fp32 value: one round-to-nearest-even."""
    y32 = y64.float()
    assert torch.equal(y32.double(), y64), "not an fp32 value"
    return y32.to(DT[dtype])


def store_acc(y64, dtype, old=None, aux=None):
    """store_tile: the tile is rounded to T (stage_tile), then old + aux + tile is summed in
    fp32 and rounded again; aux [N, K, OH/2, OW/2] lands on the even output pixels."""
    t = store(y64, dtype).float()
    if old is not None:
        t = t + store(old, dtype).float()
    if aux is not None:
        full = torch.zeros_like(t)
        full[:, :, ::2, ::2] = store(aux, dtype).float()
        t = t + full
    return t.to(DT[dtype])


def dgrad_s1(dy, w, pad):
    """Stride-1 data gradient: conv of dy with the flipped, transposed filter, pad R-1-pad."""
    R = w.shape[2]
    return conv(dy, w.flip(2, 3).transpose(0, 1), 1, R - 1 - pad)


def dgrad(dy, w, x_shape, stride, pad):
    x = torch.zeros(x_shape, dtype=D, requires_grad=True)
    conv(x, w, stride, pad).backward(dy.to(D))
    return x.grad


def wgrad(dy, x, wshape, stride, pad):
    w = torch.zeros(wshape, dtype=D, requires_grad=True)
    conv(x, w, stride, pad).backward(dy.to(D))
    return w.grad


def stats(y_stored, shift):
    """[sum(y - shift) | sum((y - shift)^2) | rows] of the STORED output, float64."""
    K = y_stored.shape[1]
    d = y_stored.double().permute(0, 2, 3, 1).reshape(-1, K) - shift.to(D)
    return torch.cat([d.sum(0), (d * d).sum(0), torch.tensor([float(d.shape[0])], dtype=D)])


def bn_mask(act, x, y, mean, invstd, gamma, beta):
    """ReLU mask of the BN whose output gradient the conv produces: from the BN's output y
    (act 1) or recomputed as the kernel does (act 2):
    fma(x, gamma*invstd, fma(-mean, gamma*invstd, beta)) > 0."""
    if act == 1:
        return y.to(D) > 0
    v = lambda t: t.to(D).view(1, -1, 1, 1)  # noqa: E731
    sc = v(gamma) * v(invstd)
    return x.to(D) * sc + (v(beta) - v(mean) * sc) > 0


def bn_sums(dx_stored, mask, x, mean, invstd):
    """(S1 = sum dz, S2 = sum dz * xhat), dz = stored dx under the mask; also sum |dz| |xhat|."""
    dz = torch.where(mask, dx_stored.double(), torch.zeros((), dtype=D))
    xhat = (x.to(D) - mean.to(D).view(1, -1, 1, 1)) * invstd.to(D).view(1, -1, 1, 1)
    return dz.sum((0, 2, 3)), (dz * xhat).sum((0, 2, 3)), (dz.abs() * xhat.abs()).sum((0, 2, 3))


# ---- one case --------------------------------------------------------------------------
def _pre_gemm(pre, terms, *operands):
    """sum |a| |b| <= terms * max|a| * max|b| (+ what is added in the epilogue)."""
    b = float(terms)
    for t in operands:
        b *= float(t.abs().max())
    pre["partial_sum_bound"] = pre.get("partial_sum_bound", 0.0) + b


@functools.lru_cache(maxsize=None)
def _build(op, shape, regime, dtype, extra):
    extra = dict(extra)
    xv, wv = values(regime, dtype)
    g = gen(op, shape, regime, xv, extra.get("seed", 1))
    pre, inp, exp = {}, {}, {}
    if op in ("fwd", "fwd+stats", "acc", "aux"):
        N, C, H, W, K, R, stride, pad = shape
        OH, OW = out_hw(H, W, R, stride, pad)
        x, w = ints((N, C, H, W), xv, g), ints((K, C, R, R), wv, g)
        y64 = conv(x, w, stride, pad)
        _pre_gemm(pre, R * R * C, x, w)
        old = aux = None
        if op == "acc":
            old = ints((N, K, OH, OW), xv, g)
        if op == "aux":
            assert OH % 2 == 0 and OW % 2 == 0
            aux = ints((N, K, OH // 2, OW // 2), xv, g)
        inp = dict(x=x, w=w, old=old, aux=aux)
        y = store_acc(y64, dtype, old, aux) if op in ("acc", "aux") else store(y64, dtype)
        exp["y"] = y
        pre["max_abs_y"] = float(y64.abs().max()) + sum(float(t.abs().max()) for t in (old, aux) if t is not None)
        if op in ("acc", "aux"):  # what one rounding of the fp32 sum would have stored
            full = torch.zeros_like(y64)
            if aux is not None:
                full[:, :, ::2, ::2] = aux
            one = store(y64 + (old if old is not None else 0) + full, dtype)
            exp["single_rounding_differs"] = float((one != y).double().mean())
        if op == "fwd+stats":
            shift = ints((K,), (-2, -1, 1, 2), g)
            inp["shift"] = shift
            exp["stats"] = stats(y, shift)
            pre["stat_sumsq"] = float(exp["stats"][K:2 * K].max())
    elif op == "s2t":
        N, Cin, OH, OW, K = shape
        dy, w = ints((N, K, OH, OW), xv, g), ints((K, Cin, 3, 3), wv, g)
        inp = dict(dy=dy, w=w)
        d64 = dgrad(dy, w, (N, Cin, 2 * OH, 2 * OW), 2, 1)
        _pre_gemm(pre, 4 * K, dy, w)
        exp["y"] = store(d64, dtype)
        pre["max_abs_y"] = float(d64.abs().max())
    elif op == "stem":
        N, H, W, K = shape
        OH, OW = out_hw(H, W, 7, 2, 3)
        x, w = ints((N, 3, H, W), xv, g), ints((K, 3, 7, 7), wv, g)
        dy, shift = ints((N, K, OH, OW), (-1, 1), g), ints((K,), (-2, -1, 1, 2), g)
        inp = dict(x=x, w=w, dy=dy, shift=shift)
        y64 = conv(x, w, 2, 3)
        _pre_gemm(pre, 147, x, w)
        exp["y"] = store(y64, dtype)
        exp["stats"] = stats(exp["y"], shift)
        exp["dw"] = wgrad(dy, x, (K, 3, 7, 7), 2, 3).float()
        pre["max_abs_y"] = float(y64.abs().max())
        pre["stat_sumsq"] = float(exp["stats"][K:2 * K].max())
        pre["wgrad_bound"] = N * OH * OW * float(dy.abs().max()) * float(x.abs().max())
    elif op == "dgrad_bn":
        N, K, H, W, Cc = shape
        act, R = extra["act"], extra["R"]
        dy, wt = ints((N, K, H, W), (-1, 1), g), ints((Cc, K, R, R), (-1, 1), g)
        x = ints((N, Cc, H, W), (-3, -2, -1, 1, 2, 3), g)
        mean, invstd = ints((Cc,), (-1, 1, 2), g) - 1.0, ints((Cc,), (0.5, 1, 2), g)  # mean in {-2, 0, 1}
        gamma, beta = ints((Cc,), (-2, -1, 1, 2), g), ints((Cc,), (-5, -3, -1, 1, 3, 5), g) * 0.25
        y = acc = None
        if act == 1:
            y, acc = ints((N, Cc, H, W), (-1, 1), g), ints((N, Cc, H, W), (-2, -1, 1, 2), g)
        inp = dict(dy=dy, wt=wt, x=x, y=y, acc=acc, mean=mean, invstd=invstd, gamma=gamma, beta=beta)
        d64 = conv(dy, wt, 1, R // 2)
        _pre_gemm(pre, R * R * K, dy, wt)
        dx = store_acc(d64, dtype, acc)
        mask = bn_mask(act, x, y, mean, invstd, gamma, beta)
        if act == 2:  # the recomputed pre-activation is exact and never zero
            sc = (gamma * invstd).view(1, -1, 1, 1)
            assert float((x * sc + (beta - mean * gamma * invstd).view(1, -1, 1, 1)).abs().min()) >= 0.25
        s1, s2, s2abs = bn_sums(dx, mask, x, mean, invstd)
        exp.update(y=dx, s1=s1, s2=s2)
        pre["max_abs_y"] = float(d64.abs().max()) + (float(acc.abs().max()) if acc is not None else 0.0)
        # dz * xhat is a multiple of min(invstd) = 1/2: exact while the sums stay below 2^24 halves
        pre["bn_sum_bound"] = float(s2abs.max()) / float(invstd.min())
    elif op == "wgrad":
        N, C, H, W, K, R, stride, pad = shape
        OH, OW = out_hw(H, W, R, stride, pad)
        x, dy = ints((N, C, H, W), xv, g), ints((N, K, OH, OW), wv, g)
        inp = dict(x=x, dy=dy)
        exp["dw"] = wgrad(dy, x, (K, C, R, R), stride, pad).float()
        pre["wgrad_bound"] = N * OH * OW * float(dy.abs().max()) * float(x.abs().max())
    else:
        raise ValueError(op)
    return inp, exp, pre


def build(case):
    """(inputs, expected, preconditions) of a case (tests/_conv_cases.py); cached: the
    tensors are shared between tests and must not be modified."""
    if case.op == "wgrad_batch":
        parts = [_build("wgrad", s, case.regime, case.dtype, ()) for s in case.shape]
        pre = {"wgrad_bound": max(p[2]["wgrad_bound"] for p in parts)}
        return [p[0] for p in parts], [p[1] for p in parts], pre
    return _build(case.op, tuple(case.shape), case.regime, case.dtype, tuple(sorted(case.extra.items())))


def preconditions(case):
    """The quantities that make a case exact (see check_preconditions)."""
    return build(case)[2]


def check_preconditions(case, pre):
    """Assert the exactness conditions of a case."""
    name = case.name
    if "partial_sum_bound" in pre:
        assert pre["partial_sum_bound"] < F32_EXACT, (name, pre)
    if "max_abs_y" in pre:
        if case.regime == "large":
            # the storage rounding is really exercised, and fp16 does not overflow
            assert pre["max_abs_y"] > INT_EXACT[case.dtype], (name, pre)
            assert pre["max_abs_y"] < (F16_MAX if case.dtype == "f16" else F32_EXACT), (name, pre)
        else:
            assert pre["max_abs_y"] <= INT_EXACT[case.dtype], (name, pre)
    for k in ("stat_sumsq", "bn_sum_bound", "wgrad_bound"):
        if k in pre:
            assert pre[k] < F32_EXACT, (name, k, pre)
