"""Float64 reference of a gradient-accumulation window (csrc/kernels/accum.hip, optim/accum.py)
and the per-element bound of the float32 kernel.  Pure torch on the CPU;
tests/test_accum_ref_cpu.py checks it against the torch idiom in float64.

``window(grads, K)`` is the exact mean ``(g_0 + ... + g_{n-1}) / K`` of a window of ``n <= K``
micro-steps (a short window keeps the factor ``1 / K``), in float64.

Tolerance model, as tests/_adam_ref.py (u = 2^-24, the fp32 unit roundoff; every fp32 rounding
of a value x errs by at most u |x|).  The kernel's roundings of a window of n micro-steps:

  acc = g_0                 exact (a copy)
  acc = acc + g_i           one rounding per sum, n - 1 of them (the last inside the LAST
                            launch); each partial sum is at most S = sum_i |g_i| in magnitude
  c = float32(1 / K)        one rounding of the factor:  u / K
  (acc + g) * c             one rounding of the product

n + 1 roundings in all, each relative to a value bounded by S (for the sums) or S / K (for the
product), so by the usual (1 + u)^m - 1 <= m u / (1 - m u):

  bound = gamma(n + 1) * S / K + ETA,   gamma(m) = m u / (1 - m u)

(ETA = 2^-149 for a product that lands in the subnormal range; sums of floats are exact
there.)  No constant is fitted.
"""
import torch

U32 = 2.0 ** -24
ETA = 2.0 ** -149


def gamma(m: int) -> float:
    return m * U32 / (1.0 - m * U32)


def window(grads, K: int):
    """The mean of a window in float64 and its bound: (mean, bound, S / K)."""
    gs = [g.detach().to("cpu", torch.float64) for g in grads]
    n = len(gs)
    assert 1 <= n <= K
    total = gs[0].clone()
    mag = gs[0].abs()
    for g in gs[1:]:
        total += g
        mag += g.abs()
    return total / K, gamma(n + 1) * mag / K + ETA, mag / K


def kernel_loop(grads, K: int):
    """The kernel's arithmetic with torch ops in the gradients' own dtype: ``acc = g_0``,
    ``acc = acc + g_i``, ``(acc + g_last) * c`` with ``c = float32(1 / K)`` (one micro-step:
    ``g_0 * c``)."""
    c = torch.tensor(1.0 / K, dtype=torch.float32).item()
    if len(grads) == 1:
        return grads[0] * c
    acc = grads[0].clone()
    for g in grads[1:-1]:
        acc = acc + g
    return (acc + grads[-1]) * c
