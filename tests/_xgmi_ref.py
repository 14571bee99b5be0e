"""Bit-exact CPU reference of what the xGMI engine computes (csrc/comm/xgmi_allreduce.hip one-shot
and two-shot all-reduce, csrc/comm/xsite.h site / wide-site exchange, the XG gradient average of
csrc/kernels/amp_step.h), written from the protocol those files document:

  every rank's value is widened to fp32 (exact), the W values are combined in RANK ORDER with
  every step rounded to fp32 (acc = x[0]; acc = acc op x[p], p = 1 .. W-1), ``avg`` is ONE fp32
  multiply by the fp32 number 1/W (not a division), and the result is rounded ONCE, to nearest
  even, to the storage type -- the same bits on every rank.

numpy float32 arithmetic is IEEE round-to-nearest-even with subnormals, so every step below is
the operation itself, not an approximation of it: the comparison needs no tolerance.

Comparison (``mismatch`` / ``assert_bits`` / ``Guarded``): bitwise on the storage type's bits, so
signed zeros count for sum and avg; where the reference is NaN the result must be a NaN (payloads
are not compared: the hardware's default NaN and a propagated one differ).  For max and min the
kernels use fmaxf / fminf, which DROP a NaN operand and do not order +0 against -0; that is left
unspecified here: keep NaN and +-0 ties out of max / min inputs (``SPECIALS`` go to sum / avg only).
"""
import numpy as np
import torch

OPS = ("sum", "avg", "max", "min")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
# quiet NaNs no kernel produces (a propagated or default NaN has none of these payloads)
SENTINEL = {torch.float32: 0x7FC0BEEF, torch.bfloat16: 0x7FEB, torch.float16: 0x7EEB}
GUARD = 16  # guard elements on each side of a Guarded view (a multiple of 16 bytes for every type)

_F = np.float32
_MAXF = float(np.finfo(np.float32).max)

# Values placed on one rank at a time (the other ranks keep their randn data).  An entry is a
# tuple: (v,) goes to rank r, (a, b) puts a on rank r and b on rank (r + 1) % W.
SPECIALS = [
    (0.0,), (-0.0,),
    (2.0 ** -149,), (-(2.0 ** -149),),            # smallest fp32 subnormal
    (2.0 ** -126 - 2.0 ** -149,),                 # largest subnormal
    (2.0 ** -126,), (-(2.0 ** -126),),            # smallest normal
    (_MAXF,), (-_MAXF,),                          # largest normal
    (float("inf"),), (float("-inf"),), (float("nan"),),
    (float("inf"), float("-inf")),                # inf - inf: NaN
    (60000.0, 60000.0),                           # finite fp32 sum, inf once rounded to fp16
    (3e38, 3e38), (-3e38, -3e38),                 # finite fp32 values whose sum overflows
]


def _np32(t):
    return t.detach().cpu().to(torch.float32).numpy()


def _acc(xs, op):
    """Rank-ordered fp32 accumulation of float32 numpy arrays."""
    acc = xs[0].astype(_F, copy=True)
    with np.errstate(over="ignore", invalid="ignore"):
        for x in xs[1:]:
            x = x.astype(_F, copy=False)
            acc = np.maximum(acc, x) if op == "max" else np.minimum(acc, x) if op == "min" else acc + x
    assert acc.dtype == _F
    return acc


def inv_world(world):
    """The fp32 number the kernels multiply an average by."""
    return _F(1) / _F(world)


def reduce(xs, op, dtype):
    """The all-reduce of ``xs[r]`` (rank r's tensor of ``dtype``): the one-shot result, as a CPU
    tensor of ``dtype``.  The two-shot result is the same value (``reduce_twoshot``)."""
    assert op in OPS and all(x.dtype == dtype for x in xs)
    acc = _acc([_np32(x) for x in xs], op)
    if op == "avg":
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            acc = acc * inv_world(len(xs))
    return torch.from_numpy(acc).to(dtype)


def reduce_twoshot(xs, op, dtype):
    """The two-shot engine rounds the owner's reduced shard to ``dtype`` before it pushes it as
    fp32 granules, and every rank rounds what it receives to ``dtype`` again."""
    return reduce(xs, op, dtype).to(torch.float32).to(dtype)


def site_sum(rows):
    """Rank-ordered fp32 sum of the ranks' float32 rows (site_probe, wide_probe)."""
    return torch.from_numpy(_acc([_np32(r) for r in rows], "sum"))


def xg_average(grads_per_rank):
    """``grads_per_rank[r][t]``: rank r's (scaled) float32 gradient of tensor t.  Per element the
    rank-ordered fp32 sum times fp32 1/W: the value the fused step unscales and checks."""
    world = len(grads_per_rank)
    out = []
    for t in range(len(grads_per_rank[0])):
        acc = _acc([_np32(grads_per_rank[r][t]) for r in range(world)], "sum")
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            acc = acc * inv_world(world)
        out.append(torch.from_numpy(acc))
    return out


# ------------------------------------------------------------------------------ comparison
def bits(t):
    """The storage bits of a float tensor as a CPU integer tensor."""
    return t.detach().cpu().contiguous().view(_INT[t.dtype])


def mismatch(got, want):
    """Boolean mask of the elements that are not the reference's: other bits, except that any NaN
    meets a NaN reference."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    return (bits(got) != bits(want)) & ~(got.isnan() & want.isnan())


def assert_bits(got, want, what):
    bad = mismatch(got, want)
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {want.numel()} elements differ, first at {i}: got "
                             f"{got.detach().cpu()[i].item()!r} ({int(bits(got)[i]) & 0xFFFFFFFF:#x}) want "
                             f"{want[i].item()!r} ({int(bits(want)[i]) & 0xFFFFFFFF:#x})")
    return want.numel()


def sentinel(n, dtype, device="cpu"):
    s = SENTINEL[dtype]
    if dtype == torch.float32:
        return torch.full((n,), s, dtype=torch.int32, device=device).view(dtype)
    return torch.full((n,), s, dtype=torch.int16, device=device).view(dtype)


class Guarded:
    """``n`` elements as a 16-byte aligned view into a sentinel-filled buffer with ``GUARD``
    sentinel elements (and the rest of the last 16 bytes) on both sides."""

    def __init__(self, n, dtype, device="cpu"):
        self.n, self.dtype = n, dtype
        per16 = 16 // torch.empty(0, dtype=dtype).element_size()
        self.total = GUARD + (n + per16 - 1) // per16 * per16 + GUARD
        self.buf = sentinel(self.total, dtype, device)
        self.view = self.buf[GUARD:GUARD + n]

    def load(self, x):
        host = sentinel(self.total, self.dtype)
        host[GUARD:GUARD + self.n] = x
        self.buf.copy_(host)
        return self.view

    def check(self, want, what):
        """Guards bitwise the sentinel, the view bitwise ``want``; a NaN that is the sentinel's
        own pattern is an element never written, also where the reference is NaN."""
        raw = bits(self.buf)
        s = bits(sentinel(1, self.dtype))[0]
        pad = torch.ones(self.total, dtype=torch.bool)
        pad[GUARD:GUARD + self.n] = False
        bad = (raw != s) & pad
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            where = f"{GUARD - i} before the start" if i < GUARD else f"{i - GUARD - self.n} past the end"
            raise AssertionError(f"{what}: {int(bad.sum())} guard elements overwritten, first {where} (n = {self.n})")
        got = self.buf.detach().cpu()[GUARD:GUARD + self.n]
        left = raw[GUARD:GUARD + self.n] == s
        if bool(left.any()):
            raise AssertionError(f"{what}: element {int(left.nonzero()[0])} of {self.n} still holds the sentinel")
        return assert_bits(got, want, what)
