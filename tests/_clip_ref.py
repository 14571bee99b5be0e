"""Float64 reference of global-norm gradient clipping (csrc/kernels/clip.hip grad_norm / scale_,
optim/clip.py) and the error bounds of the float32 kernels, counted from their roundings as
tests/_adam_ref.py counts adam_rule's.  Pure torch on the CPU; tests/test_clip_ref_cpu.py checks
it against ``torch.nn.utils.clip_grad_norm_`` in float64.

Tolerance model (u = 2^-24, the fp32 unit roundoff; every rounding of a value x errs by at
most u |x|).  Every term of the sum of squares is non-negative, so relative errors do not
amplify: the sum is off by at most the number of roundings on the longest path from an element
to the result, times u.  With U granules per lane and chunk and W waves per workgroup that
path is, in the kernel's order:

  unscale   x = g * (1 / scale), rounded on its own; 1 / scale is rounded too, so x^2 carries
            4 u (AMP route only; with a power-of-two scale both are exact)
  square    x * x                                                       1
  lane      the lane's 4 U squares added in index order                 4 U - 1
  wave      group_sum<64>: six levels                                   6
  waves     the W wave sums added in wave order through LDS             W - 1
  final     the partials are added in float64 (its 2^-53 roundings are not counted: a few
            thousand of them are below 1e-12 of the sum) and rounded to fp32 once   1

  norm      sqrt halves a relative error; sqrtf rounds once:  R u / 2 + u
  coef      fl(norm + 1e-6f), the reciprocal, the product with (float)max_norm and that cast:
            the norm's error + 4 u; the clamp to 1 only shrinks an error
  clipped   g * coef rounds once more:  |g coef| (norm's + 5 u)

No constant is fitted.  The values the GPU tests draw have |g| in [1e-6, 1e3], so every square
is a normal fp32 and no subnormal term is needed.
"""
import torch

U32 = 2.0 ** -24
WAVES = 4  # ADAM_THR / 64


def sumsq_roundings(U: int, unscale: bool = False) -> int:
    return (4 if unscale else 0) + 1 + (4 * U - 1) + 6 + (WAVES - 1) + 1


def sumsq_rel_bound(U: int, unscale: bool = False) -> float:
    return sumsq_roundings(U, unscale) * U32


def norm_rel_bound(U: int, unscale: bool = False) -> float:
    return sumsq_rel_bound(U, unscale) / 2 + U32


def clipped_rel_bound(U: int, unscale: bool = False) -> float:
    return norm_rel_bound(U, unscale) + 5 * U32


def reference(grads, max_norm: float, scale: float | None = None):
    """{"norm", "coef"} as Python floats and "clipped", the float64 gradients times the
    coefficient, of float32 (or float64) ``grads`` (divided by ``scale`` first when given)."""
    xs = [g.detach().to("cpu", torch.float64).reshape(-1) for g in grads]
    if scale is not None:
        xs = [x / float(scale) for x in xs]
    total = sum(float((x * x).sum()) for x in xs) if xs else 0.0
    norm = total ** 0.5
    coef = min(1.0, float(max_norm) / (norm + 1e-6))
    return {"norm": norm, "coef": coef, "clipped": [x * coef for x in xs]}
