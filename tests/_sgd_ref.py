"""Float64 reference of the SGD / AMP step (csrc/kernels/optim.hip with csrc/kernels/amp_step.h:
unscale + non-finite check, SGD, scale update, their fused forms) and of the batch gather
(csrc/kernels/data.hip), with the per-element error bounds of one float32 step.  Pure torch /
numpy on the CPU, written out from torch/optim/sgd.py (_single_tensor_sgd) and
torch/amp/grad_scaler.py (_unscale_grads_, _maybe_opt_step, update); tests/test_sgd_ref_cpu.py
checks it against ``torch.optim.SGD`` in float64 and against torch's own
``_amp_foreach_non_finite_check_and_unscale_`` / ``_amp_update_scale_`` on the CPU.

``amp_step`` takes float32 inputs, computes in float64 with the hyper-parameters as the Python
doubles they are given as, and returns the new params, grads and buffers next to a bound for each.

Tolerance model, as tests/_adam_ref.py (u = 2^-24, the fp32 unit roundoff): every fp32 rounding
of a value x errs by at most u |x|, every hyper-parameter the kernel holds in fp32 (lr, momentum,
dampening, weight_decay) and 1/scale is off by at most u of itself, and a rounding that lands in
the subnormal range errs by at most ETA = 2^-149 instead.  Counting the roundings of common.h
sgd_rule line by line (G the scaled gradient as stored, primes the new values):

  g'   G * (1/scale): the reciprocal's rounding and the product's:    dg  = 2 u |g'|
       (a power-of-two scale: both exact, dg = 0 above the subnormal range)
  d    +-g', then the decay's one fma, wd in fp32:                    dd  = dg + u (wd |p| + |d|)
  mb   momentum * buf, rounded on its own, momentum in fp32:          dmb = 2 u |mb|
  b'   first: b' = d, db = dd.  Else one fma of w = 1.f - dampening (dampening in fp32 and the
       subtraction's rounding: w off by u (dampening + w); exact when dampening == 0):
                                        db  = dmb + u (dampening + w) |d| + w dd + u |b'|
  d2   nesterov: one fma, momentum in fp32:  dd2 = dd + u momentum |b'| + momentum db + u |d2|
       else d2 = b' (momentum) or d (none)
  p'   one fma, lr in fp32:                                           dp  = u lr |d2| + lr dd2 + u |p'|

plus ETA for each rounding.  No constant is fitted: every term is a rounding named above times
the magnitude it acts on (second-order terms, u^2, are left out as in _adam_ref.py).

The exact leg (``dyadic``): every value is k/8 with |k| <= 16, lr = 0.25, momentum = 0.5,
dampening = 0.25, weight_decay = 0.125 and the scale a power of two, so every intermediate of
two consecutive steps is a float32 (with dampening step 1 ends on multiples of 2^-10 and step 2
on 2^-17, below 8: 20 bits); ``exact=True`` asserts x == float32(x) at every rounding point.  A
third step with dampening needs multiples of 2^-24, so the exact leg is two steps.
"""
import numpy as np
import torch

U32 = 2.0 ** -24
ETA = 2.0 ** -149

DYADIC = dict(lr=0.25, momentum=0.5, dampening=0.25, weight_decay=0.125)
FLOAT = dict(lr=0.1, momentum=0.9, dampening=0.1, weight_decay=1e-4)

# (momentum on, dampening on, nesterov): the combinations torch.optim.SGD accepts
_MDN = [(False, False, False), (True, False, False), (True, False, True), (True, True, False)]
# every option combination the GPU tests run: (momentum, dampening, nesterov, maximize, decay) on/off
OPTION_GRID = [(m, d, n, mx, wd) for (m, d, n) in _MDN for mx in (False, True) for wd in (False, True)]


def options(base, m, d, n, mx, wd):
    """The hyper-parameters of one OPTION_GRID entry, values from ``base`` (DYADIC or FLOAT)."""
    return dict(lr=base["lr"], momentum=base["momentum"] if m else 0.0, dampening=base["dampening"] if d else 0.0,
                weight_decay=base["weight_decay"] if wd else 0.0, nesterov=n, maximize=mx)


def option_id(o):
    return "-".join(k for k, on in zip(("mom", "damp", "nest", "max", "wd"), o) if on) or "plain"


def f32(x: float) -> float:
    """The float32 a kernel receives for a by-value double."""
    return float(np.float32(x))


def _d(x):
    return x.detach().to("cpu", torch.float64)


def _rt(x, exact, what):
    """A rounding point: on the exact leg the value must already be a float32."""
    if exact:
        bad = ~((x.float().double() == x) | x.isnan())
        assert not bool(bad.any()), f"{what}: not a float32 at {bad.nonzero()[0].tolist()}: {x[bad][0].item()!r}"
    return x


def sgd_rule(p, g, buf, first, dg, *, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False,
             maximize=False, exact=False):
    """torch/optim/sgd.py _single_tensor_sgd for one tensor, float64.  ``g`` is the unscaled
    gradient and ``dg`` its bound.  Returns p', b' (None without momentum), dp, db."""
    u = U32
    d = -g if maximize else g
    dd = dg
    if weight_decay != 0:
        d = _rt(d + weight_decay * p, exact, "g + wd p")
        dd = dd + u * (weight_decay * p.abs() + d.abs()) + ETA
    b1 = db = None
    if momentum != 0:
        if first:
            b1, db = d.clone(), dd
        else:
            mb = _rt(momentum * buf, exact, "momentum buf")
            dmb = 2 * u * mb.abs() + ETA
            w = 1.0 - dampening
            b1 = _rt(mb + w * d, exact, "buf")
            db = dmb + (u * (dampening + w) * d.abs() if dampening != 0 else 0.0) + w * dd + u * b1.abs() + ETA
        if nesterov:
            d2 = _rt(d + momentum * b1, exact, "g + momentum buf")
            dd2 = dd + u * momentum * b1.abs() + momentum * db + u * d2.abs() + ETA
        else:
            d2, dd2 = b1, db
    else:
        d2, dd2 = d, dd
    p1 = _rt(p - lr * d2, exact, "p")
    dp = u * lr * d2.abs() + lr * dd2 + u * p1.abs() + ETA
    return p1, b1, dp, db


def _pow2(x: float) -> bool:
    m, _ = np.frexp(x)
    return m == 0.5


def unscale_check(grads, scale, found_inf=0.0):
    """torch._amp_foreach_non_finite_check_and_unscale_: the check on the scaled gradients as
    given, every gradient multiplied by 1/scale (also when one is non-finite); a product beyond
    float32's range is the infinity float32 makes of it.  Returns grads, bounds, found."""
    inv = 1.0 / scale
    found = bool(found_inf)
    out, bnd = [], []
    for g in grads:
        g = _d(g)
        found = found or not bool(torch.isfinite(g).all())
        g1 = g * inv
        over = g1.float().double()
        g1 = torch.where(over.isinf(), over, g1)
        out.append(g1)
        bnd.append((0.0 if _pow2(scale) else 2 * U32) * g1.abs() + ETA)
    return out, bnd, found


def update_scale(scale, tracker, found, growth=2.0, backoff=0.5, interval=2000):
    """torch._amp_update_scale_ (float32 scale, int32 tracker): returns (scale, tracker)."""
    s = np.float32(scale)
    if found:
        return float(np.float32(np.float64(s) * backoff)), 0
    succ = tracker + 1
    if succ == interval:
        with np.errstate(over="ignore"):
            ns = np.float32(np.float64(s) * growth)
        return float(ns if np.isfinite(ns) else s), 0
    return float(s), succ


def amp_step(params, grads, bufs, first=(), *, scale=None, tracker=0, found_inf=0.0, growth=2.0, backoff=0.5,
             interval=2000, unscale_by=None, grad_scale=None, exact=False, **hyper):
    """One step over a list of tensors.

    AMP mode (``scale``): GradScaler.unscale_ + step + update -- the grads are unscaled in place
    (by ``unscale_by`` when given, else by ``scale``), any non-finite scaled gradient (or a set
    ``found_inf``) skips every parameter and buffer, then the scale / growth tracker move.
    Plain mode (no scale): the gradients stay as given and non-finite values are applied, as
    torch.optim.SGD does; ``grad_scale`` divides them inside the rule only (the optimizer's own
    grad_scale argument), unchecked.  ``first[i]``: tensor i's momentum buffer is new (b = d).

    Returns {"p", "g", "b"} (float64 lists; "b" empty without momentum), their bounds
    {"bp", "bg", "bb"}, and "scale", "tracker", "found"."""
    ps = [_d(p) for p in params]
    bs = [_d(b) for b in bufs] if hyper.get("momentum", 0.0) != 0 else []
    n = len(ps)
    first = list(first) if len(first) else [0] * n
    assert len(grads) == n and len(first) == n and (not bs or len(bs) == n)
    zero = [torch.zeros_like(p) for p in ps]
    if scale is not None:
        g_out, bg, found = unscale_check(grads, scale if unscale_by is None else unscale_by, found_inf)
        g_use, dg = g_out, bg
        new_scale, new_tracker = update_scale(scale, tracker, found, growth, backoff, interval)
    else:
        g_out, bg, found = [_d(g) for g in grads], zero, bool(found_inf)  # a set word skips (_maybe_opt_step)
        g_use, dg = g_out, bg
        if grad_scale is not None:
            g_use, dg, _ = unscale_check(grads, grad_scale)
        new_scale, new_tracker = None, tracker
    out = {"g": g_out, "bg": bg, "scale": new_scale, "tracker": new_tracker, "found": found}
    if found:
        out.update(p=ps, b=bs, bp=zero, bb=zero if bs else [])
        return out
    p1, b1, bp, bb = [], [], [], []
    for i in range(n):
        p, b, dp, db = sgd_rule(ps[i], g_use[i], bs[i] if bs else None, bool(first[i]), dg[i], exact=exact, **hyper)
        p1.append(p)
        bp.append(dp)
        if bs:
            b1.append(b)
            bb.append(db)
    out.update(p=p1, b=b1, bp=bp, bb=bb)
    return out


# ------------------------------------------------------------------------------ generators
def _k8(n, gen):
    return torch.randint(-16, 17, (n,), generator=gen).float() / 8


def dyadic(sizes, seed, scale=1024.0):
    """params, scaled grads, buffers for the exact leg: k/8 with |k| <= 16 (grads times the
    power-of-two scale)."""
    assert _pow2(scale)
    gen = torch.Generator().manual_seed(seed)
    return [_k8(n, gen) for n in sizes], [_k8(n, gen) * scale for n in sizes], [_k8(n, gen) for n in sizes]


def dyadic_grads(sizes, seed, scale=1024.0):
    gen = torch.Generator().manual_seed(seed)
    return [_k8(n, gen) * scale for n in sizes]


def normal(sizes, seed, scale=1024.0):
    """params, scaled grads, buffers for the float leg: standard normals (buffers 0.1 of that)."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda n: torch.randn(n, generator=gen)
    return [r(n) for n in sizes], [r(n) * scale for n in sizes], [r(n) * 0.1 for n in sizes]


def slab_rows(col_sums, rows, seed, scale=1024.0):
    """A [rows][n] slab (the fused step's slab source) of dyadic values, multiples of scale / 8,
    whose column sums are ``col_sums`` (dyadic too) exactly in whatever order they are added."""
    gen = torch.Generator().manual_seed(seed)
    slab = torch.stack([_k8(col_sums.numel(), gen) * scale for _ in range(rows)])
    slab[rows - 1] = col_sums - slab[:rows - 1].sum(0)
    assert torch.equal(slab.double().sum(0), col_sums.double())
    return slab.contiguous()


# ------------------------------------------------------------------------------ scale table
# (scale, tracker, found, growth, backoff, interval): torch._amp_update_scale_'s branches
SCALE_TABLE = [
    (1024.0, 0, False, 2.0, 0.5, 3),            # tracker counts
    (1024.0, 2, False, 2.0, 0.5, 3),            # growth at the interval
    (1024.0, 0, False, 2.0, 0.5, 1),            # interval == 1: grows every step
    (2.0 ** 127, 0, False, 2.0, 0.5, 1),        # growth would overflow: scale kept, tracker reset
    (1024.0, 2, True, 2.0, 0.5, 3),             # backoff, tracker reset
    (2.0 ** -126, 1, True, 2.0, 0.5, 3),        # backoff into the subnormal range
    (3.0, 1, False, 1.5, 0.25, 2),              # other factors
    (3.0, 5, False, 1.5, 0.25, 2),              # tracker past the interval: no growth
]


# ------------------------------------------------------------------------------ gather
def gather(imgs, labels, order, step, B, scale, shift, dtype):
    """data.hip gather: out[i] = Cvt<T>(float32(u8) * scale + shift) for the images at positions
    step * B + i of ``order`` (a position past the end repeats the last index, the kernel's
    clamp), with scale / shift the float32 the kernel receives.  Returns (candidates, labels):
    one candidate when shift == 0 (one correctly rounded product), else two -- the fma and the
    rounded product plus shift -- since the contraction is the compiler's choice."""
    n = order.numel()
    pos = (step * B + torch.arange(B)).clamp(max=n - 1)
    src = order.cpu()[pos]
    x = imgs.cpu().reshape(imgs.shape[0], -1)[src].double()
    s, sh = float(np.float32(scale)), float(np.float32(shift))
    prod = x * s  # exact: 8 bits times 24
    fma = (prod + sh).float()  # exact sum in float64 (within 2^-30 .. 2^2 here), rounded once
    cands = [fma.to(dtype)]
    if sh != 0:
        cands.append((prod.float().double() + sh).float().to(dtype))
    return cands, labels.cpu()[src]
