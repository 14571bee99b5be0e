"""Float64 reference of the Adam / AdamW update (csrc/common.h adam_bias + adam_rule, the
kernels of csrc/kernels/adam.hip) and the per-element error bounds of one float32 step.
Pure torch on the CPU, written out from the formulas of torch/optim/adam.py;
tests/test_adam_ref_cpu.py checks it against ``torch.optim.AdamW`` / ``Adam`` in float64.

``step`` takes float32 (or float64) inputs, computes in float64 with the hyper-parameters as
the Python doubles they are given as, and returns the new p, m, v next to a bound for each.

Tolerance model, as tests/_head_ref.py (u = 2^-24, the fp32 unit roundoff): every fp32
rounding of a value x errs by at most u |x|, every hyper-parameter the kernel holds in fp32
(lr, beta1, beta2, eps, weight_decay) is off by at most u of itself, and a rounding that
lands in the subnormal range errs by at most ETA = 2^-149 instead.  Counting the roundings of
adam_rule line by line (t is the step count the update uses, G' the gradient after
maximize / coupled decay, d = G' - m, primes are the new values):

  g'   coupled decay only, one fma, wd in fp32:            dg  = u (|g'| + wd |p|)
  m'   d rounded, w1 = (float)(1 - beta1) off by u of itself (rounded from the host's double),
       the fma's rounding:                                 dm  = u (2 w1 |d| + |m'|) + w1 dg
  v'   v * beta2 rounded with beta2 off by u of itself, g'^2 rounded, w2 = (float)(1 - beta2)
       off by u of itself, the fma's rounding:             dv  = u (2 beta2 v + 2 w2 g'^2 + v') + 2 w2 |g'| dg
  bias beta^t by powf, 1 ulp = 2 u (the HIP math library's documented bound), of a base off by
       u, so beta^t is off by (2 + t) u beta^t; the subtraction from 1 rounds once more and
       keeps the absolute error:  e(b) = (2 + t) beta^t / (1 - beta^t) + 1   (relative, in u)
       step_size = 1 / (b1 * (float)(1 / lr)): the reciprocal's rounding and two more:  e_ss = e(b1) + 3
       bc2_sqrt = sqrt(b2): halves it, rounds once:        e_c2 = e(b2) / 2 + 1
  den  s = sqrt(v'): |sqrt(a) - sqrt(b)| <= |a - b| / sqrt(b) (and <= sqrt|a - b|), one rounding;
       q = s / bc2_sqrt: one rounding; r = q + eps: one rounding and eps's; den = r / step_size:
       one rounding.  In absolute terms  ds = min(dv / sqrt(v'), sqrt(dv)) + u s,
       dq = ds / c2 + u q (e_c2 + 1),  dr = dq + u (r + eps),  dden = (dr + u r (e_ss + 1)) / |ss|
  p'   decoupled decay: (float)(1 - lr wd) and the product, 2 u |p|; m' / den rounded; the sum
       rounded:  dp = 2 u |p| [decay] + dm / |den| + |upd| dden / |den| + u |upd| + u |p'|

plus 4 ETA on each for the subnormal roundings (the 1e-20 gradient: its square is 1e-40).  No
constant is fitted: every term is a rounding named above times the magnitude it acts on.
"""
import torch

U32 = 2.0 ** -24
ETA = 2.0 ** -149


def step(p, g, m, v, t, *, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=True, maximize=False):
    """One update with step count ``t`` (the count AFTER the increment, >= 1).
    Returns {"p", "m", "v"} and their bounds {"bp", "bm", "bv"}, all float64."""
    p, g, m, v = (x.detach().to("cpu", torch.float64) for x in (p, g, m, v))
    b1, b2 = float(betas[0]), float(betas[1])
    u = U32
    gg = -g if maximize else g
    dg = torch.zeros_like(gg)
    p0 = p
    decay = False
    if weight_decay != 0:
        if decoupled:
            p0 = p * (1.0 - lr * weight_decay)
            decay = True
        else:
            gg = gg + weight_decay * p
            dg = u * (gg.abs() + weight_decay * p.abs())
    w1, w2 = 1.0 - b1, 1.0 - b2
    d = gg - m
    m1 = m + w1 * d
    dm = u * (2 * w1 * d.abs() + m1.abs()) + w1 * dg + 4 * ETA
    v1 = b2 * v + w2 * gg * gg
    dv = u * (2 * b2 * v + 2 * w2 * gg * gg + v1) + 2 * w2 * gg.abs() * dg + 4 * ETA
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    e_b1 = (2 + t) * b1 ** t / bc1 + 1
    e_b2 = (2 + t) * b2 ** t / bc2 + 1
    ss = -lr / bc1
    e_ss = e_b1 + 3
    c2 = bc2 ** 0.5
    e_c2 = e_b2 / 2 + 1
    s = v1.sqrt()
    ds = torch.minimum(dv / s.clamp_min(1e-300), dv.sqrt()) + u * s
    q = s / c2
    dq = ds / c2 + u * q * (e_c2 + 1)
    r = q + eps
    dr = dq + u * (r + eps)
    den = r / ss
    dden = (dr + u * r * (e_ss + 1)) / abs(ss)
    upd = m1 / den
    p1 = p0 + upd
    dp = ((2 * u * p.abs() if decay else 0.0) + dm / den.abs() + upd.abs() * dden / den.abs() + u * upd.abs()
          + u * p1.abs() + 4 * ETA)
    return {"p": p1, "m": m1, "v": v1, "bp": dp, "bm": dm, "bv": dv}


def trajectory(p, grads, *, m=None, v=None, t0=0, lrs=None, **hyper):
    """``len(grads)`` steps in float64 from float32 inputs; ``lrs``: one rate per step (else
    ``hyper["lr"]``).  Returns the final {"p", "m", "v"}."""
    p = p.detach().to("cpu", torch.float64)
    m = torch.zeros_like(p) if m is None else m.detach().to("cpu", torch.float64)
    v = torch.zeros_like(p) if v is None else v.detach().to("cpu", torch.float64)
    for k, g in enumerate(grads):
        h = dict(hyper)
        if lrs is not None:
            h["lr"] = float(lrs[k])
        o = step(p, g, m, v, t0 + k + 1, **h)
        p, m, v = o["p"], o["m"], o["v"]
    return {"p": p, "m": m, "v": v}


def ulp_distance(a: torch.Tensor, b: torch.Tensor) -> int:
    """Largest distance between two float32 tensors in units in the last place (bit patterns
    mapped to a monotone integer line, so it counts representable values between them)."""
    def key(x):
        i = x.detach().to("cpu", torch.float32).contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    if a.numel() == 0:
        return 0
    return int((key(a) - key(b)).abs().max())
