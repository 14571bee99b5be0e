"""numpy float32 emulation of the slab column sums in the BatchNorm coefficient prologues
(csrc/kernels/convblock_bn.h bn_finalize / bn_bwd_coef), and the order-sensitive slabs the
tests feed them.

The documented order, for a slab of `rows` rows of RL floats reduced by a 256-thread workgroup:
G = 256 // RL lane groups; group g adds rows g, g + G, g + 2G, ... in ascending order into an
accumulator that starts at +0; the G group sums are then added in the order 0 .. G-1, again
from +0.  Every add is one fp32 add, so the bits follow from the order alone.

  RL 65 (BN2 forward rows [sum(32) | sumsq(32) | n])  G = 3
  RL 33 (BN1 forward rows)                            G = 7
  RL 64 (BN2 backward rows [S1(32) | S2(32)])         G = 4
  RL 32 (BN1 backward rows)                           G = 8
"""
import numpy as np

NTHR = 256
F32 = np.float32


def groups(RL):
    return NTHR // RL


def slab(rows, RL, seed, positive_cols=()):
    """rows x RL float32 of mixed magnitudes: +-2^24, +-1 and +-2^-10 times 1, 1.25, 1.5 or 1.75
    (fixed seed).  Next to a 2^24 term a 1 is at the last bit and a 2^-10 is lost, so another
    grouping of the same values rounds differently.  positive_cols: columns kept positive (the
    pixel-count column, which the kernels divide by)."""
    rng = np.random.default_rng(seed)
    mag = rng.choice(np.array([2.0 ** 24, 1.0, 2.0 ** -10]), size=(rows, RL), p=[0.25, 0.5, 0.25])
    man = rng.choice(np.array([1.0, 1.25, 1.5, 1.75]), size=(rows, RL))
    sgn = rng.choice(np.array([-1.0, 1.0]), size=(rows, RL))
    for c in positive_cols:
        sgn[:, c] = 1.0
    return (sgn * mag * man).astype(F32)


def _seq(terms, RL):
    acc = np.zeros(RL, dtype=F32)
    for t in terms:
        acc = (acc + t).astype(F32)
    return acc


def colsum(s, G=None):
    """The documented order (module docstring)."""
    s = np.asarray(s, dtype=F32)
    rows, RL = s.shape
    G = groups(RL) if G is None else G
    return _seq([_seq([s[r] for r in range(g, rows, G)], RL) for g in range(G)], RL)


def colsum_reversed(s):
    """Same grouping, every sequence walked backwards (rows descending, groups G-1 .. 0)."""
    s = np.asarray(s, dtype=F32)
    rows, RL = s.shape
    G = groups(RL)
    return _seq([_seq([s[r] for r in reversed(range(g, rows, G))], RL) for g in reversed(range(G))], RL)


def colsum_tree(s):
    """A pairwise tree over the rows in row order."""
    v = [r for r in np.asarray(s, dtype=F32)]
    while len(v) > 1:
        v = [(v[i] + v[i + 1]).astype(F32) if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return (np.zeros_like(v[0]) + v[0]).astype(F32)


def colsum64(s):
    return np.asarray(s, dtype=np.float64).sum(0)


def fp32_bound(s):
    """|fp32 sequential sum - exact| <= (adds) * 2^-24 * sum|v| / (1 - adds * 2^-24); a column's
    longest chain is its group's rows plus the G group adds (the adds of +0 are exact)."""
    s = np.asarray(s, dtype=np.float64)
    rows, RL = s.shape
    G = groups(RL)
    adds = -(-rows // G) + G
    u = 2.0 ** -24
    return adds * u / (1 - adds * u) * np.abs(s).sum(0)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.uint32)


# Slab shapes (rows, RL) the GPU test reaches, per batch: what the ops allocate.
BATCHES = (1, 2, 8, 32, 33, 64)
FWD2_SPLIT = 4          # conv2 forward workgroups per image (BN2 forward rows per image)
DGRAD_QUARTERS = 4      # BN1 backward rows per image


def shapes(B, fwd1_rows):
    """{name: (rows, RL)} at batch B; fwd1_rows: the conv1 forward's slab rows at B."""
    return {"bn1_fwd": (fwd1_rows, 33), "bn2_fwd": (FWD2_SPLIT * B, 65), "bn2_bwd": (B, 64),
            "bn1_bwd": (DGRAD_QUARTERS * B, 32)}


_NAMES = ("bn1_bwd", "bn1_fwd", "bn2_bwd", "bn2_fwd")


def case(name, rows, RL):
    """The slab of a shape (seeded by it); a forward slab's count column is kept positive."""
    return slab(rows, RL, 1000 * _NAMES.index(name) + rows, positive_cols=(RL - 1,) if RL % 2 else ())
