"""tests/_bn_coef_ref.py on the CPU: the slabs that tests/test_bn_coef_order_gpu.py feeds the
BatchNorm coefficient prologues really do pin the add order, and the emulated order is a
correct sum.

  order-sensitive  for every slab shape the GPU test uses, a pairwise tree over the rows and the
                   documented grouping walked backwards each give other bits than the documented
                   order in at least one column.  A slab of one or two rows has no order to pin
                   (one term, or one commutative add): those shapes are checked to be exactly
                   that, not skipped.
  float64          the emulation agrees with the float64 column sums within the fp32 bound of
                   its longest add chain (tests/_bn_coef_ref.py fp32_bound).
"""
import numpy as np
import pytest

from . import _bn_coef_ref as R

SHAPES = sorted({(name, rows, RL) for B in R.BATCHES for name, (rows, RL) in R.shapes(B, 4 * B).items()})


@pytest.mark.parametrize("name,rows,RL", SHAPES)
def test_values_pin_the_order(name, rows, RL):
    s = R.case(name, rows, RL)
    want = R.bits(R.colsum(s))
    tree, rev = R.bits(R.colsum_tree(s)), R.bits(R.colsum_reversed(s))
    if rows <= 2:
        assert (tree == want).all() and (rev == want).all()
        return
    assert (tree != want).any(), "a tree over the rows gives the same bits: the values pin nothing"
    assert (rev != want).any(), "the reversed walk gives the same bits: the values pin nothing"
    # and so does another group count, once some group holds two rows (with at most one row per
    # group either count is the rows in order)
    G = R.groups(RL)
    if rows > G + 1:
        assert (R.bits(R.colsum(s, G=G + 1)) != want).any()


@pytest.mark.parametrize("name,rows,RL", SHAPES)
def test_emulation_is_a_sum(name, rows, RL):
    s = R.case(name, rows, RL)
    err = np.abs(R.colsum(s).astype(np.float64) - R.colsum64(s))
    assert (err <= R.fp32_bound(s)).all(), (err / np.maximum(R.fp32_bound(s), 1e-300)).max()


def test_group_counts():
    assert [R.groups(rl) for rl in (65, 33, 64, 32)] == [3, 7, 4, 8]


def test_empty_groups_add_nothing():
    """Fewer rows than groups: the empty groups contribute +0 and the sum is the rows in order."""
    s = R.slab(2, 32, 7)
    assert (R.bits(R.colsum(s)) == R.bits((s[0] + s[1]).astype(np.float32))).all()
