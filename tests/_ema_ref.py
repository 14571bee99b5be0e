"""Float64 reference of the EMA update (csrc/common.h lerp_rule + ema_warmup_weight, the kernel
of csrc/kernels/ema.hip; optim/ema.py) and the per-element bound of one float32 update with
warm-up.  Pure torch on the CPU; tests/test_ema_ref_cpu.py checks it against torch's
``AveragedModel`` in float64.

``decay_of(n, decay, warmup)`` is the decay update ``n`` uses (``n`` = ``n_averaged`` before
the update, >= 1): ``decay``, or with warm-up ``min(decay, (1 + n) / (10 + n))``.
``update`` computes ``shadow + (1 - decay_n) (source - shadow)`` in float64 with ``decay`` as
the Python double it is given as; ``n == 0`` copies.

Tolerance model, as tests/_adam_ref.py (u = 2^-24, the fp32 unit roundoff; every fp32 rounding
of a value x errs by at most u |x|).  Counting the roundings of ema_warmup_weight and lerp_rule
line by line (D = source - shadow, w the exact weight, r the exact result):

  nf, a = 1 + nf, b = 10 + nf   exact for n < 2^24 - 10 (integers below 2^24)
  q = a / b                     one rounding:                              u q
  min(decay, q)                 decay is held in fp32, off by u of itself; when the two lie within
                                that of each other the kernel may pick the other one:  u decay
  w = 1 - q (or the host's      one rounding:                              u w
      float32 of 1 - decay)
                                dw = u (q + decay + w) <= 2 u   (q <= decay, decay + w <= 1 + q u)
  d = source - shadow           one rounding:                              u |D|
  |w| <  0.5: fma(w, d, shadow) the fma's rounding u |r|, w's error dw |D|, d's error w u |D|
  |w| >= 0.5: fma(-d, 1 - w, source), 1 - w exact (Sterbenz): u |r| + dw |D| + (1 - w) u |D|

  bound = u (|r| + 3 |D|) + 2 ETA

(max(w, 1 - w) <= 1; ETA = 2^-149 for a rounding that lands in the subnormal range.)  No
constant is fitted: every term is a rounding named above times the magnitude it acts on.
"""
import torch

U32 = 2.0 ** -24
ETA = 2.0 ** -149


def decay_of(n: int, decay: float, warmup: bool = False) -> float:
    """The decay of update ``n`` >= 1, in float64."""
    return min(float(decay), (1.0 + n) / (10.0 + n)) if warmup else float(decay)


def update(shadow, source, n: int, decay: float, warmup: bool = False):
    """One update from ``n_averaged == n``.  Returns (new shadow, bound), both float64."""
    a = shadow.detach().to("cpu", torch.float64)
    b = source.detach().to("cpu", torch.float64)
    if n == 0:
        return b.clone(), torch.zeros_like(b)
    w = 1.0 - decay_of(n, decay, warmup)
    D = b - a
    r = a + w * D
    return r, U32 * (r.abs() + 3.0 * D.abs()) + 2 * ETA


def trajectory(sources, decay: float, warmup: bool = False, n0: int = 0, shadow=None):
    """``len(sources)`` updates in float64; returns the final shadow."""
    s = None if shadow is None else shadow.detach().to("cpu", torch.float64)
    for k, x in enumerate(sources):
        n = n0 + k
        s = x.detach().to("cpu", torch.float64).clone() if n == 0 else update(s, x, n, decay, warmup)[0]
    return s
