"""The (quarter, slot) rule of the conv2 data gradient's BN1 partial rows (tests/_dgrad_rows.py,
csrc/kernels/conv5x5.h BwdEpi) for the 14 x 14 layer: MT = 13 m-tiles, splits 2 and 4."""
import pytest

from . import _dgrad_rows as Q

SPLITS = [2, 4]


def test_quarters_partition_the_m_tiles():
    tiles = [t for k in range(Q.QUARTERS) for t in range(*Q.quarter_range(k))]
    assert tiles == list(range(Q.MT))
    assert [Q.quarter_range(k) for k in range(4)] == [(0, 3), (3, 6), (6, 9), (9, 13)]
    assert [Q.quarter_pixels(k) for k in range(4)] == [(0, 48), (48, 96), (96, 144), (144, 196)]


def test_every_m_tile_has_one_quarter_and_a_slot_below_4():
    seen = {}
    for t in range(Q.MT):
        k, s = Q.place(t)
        assert 0 <= s < Q.NW, (t, k, s)
        assert (k, s) not in seen, (t, seen[(k, s)])
        seen[(k, s)] = t
    assert len(seen) == Q.MT


@pytest.mark.parametrize("nsplit", SPLITS)
def test_workgroups_cover_whole_quarters(nsplit):
    """A workgroup's m-tiles are exactly those of its quarters -- at 2, the two quarters the
    4-way split gives -- and every m-tile is computed by exactly one wave of one workgroup."""
    owner = {}
    for sp in range(nsplit):
        lo, hi = Q.split_range(sp, nsplit)
        qs = Q.quarters_of(sp, nsplit)
        assert len(qs) == Q.QUARTERS // nsplit
        assert [t for k in qs for t in range(*Q.quarter_range(k))] == list(range(lo, hi))
        assert [Q.split_range(k, 4) for k in qs] == [Q.quarter_range(k) for k in qs]
        for wv in range(Q.NW):
            for t in Q.wave_tiles(sp, nsplit, wv):
                assert lo <= t < hi and t not in owner
                owner[t] = (sp, wv)
                assert Q.place(t)[0] in qs
    assert sorted(owner) == list(range(Q.MT))
    assert sorted(k for sp in range(nsplit) for k in Q.quarters_of(sp, nsplit)) == list(range(Q.QUARTERS))


@pytest.mark.parametrize("nsplit", SPLITS)
def test_no_wave_holds_two_m_tiles_of_one_quarter(nsplit):
    for sp in range(nsplit):
        for wv in range(Q.NW):
            ks = [Q.place(t)[0] for t in Q.wave_tiles(sp, nsplit, wv)]
            assert len(ks) == len(set(ks)) <= Q.QUARTERS // nsplit, (sp, wv, ks)


def test_the_2_way_waves_meet_the_m_tiles_the_kernel_comment_names():
    assert [Q.wave_tiles(0, 2, wv) for wv in range(4)] == [[0, 4], [1, 5], [2], [3]]
    assert [Q.wave_tiles(1, 2, wv) for wv in range(4)] == [[6, 10], [7, 11], [8, 12], [9]]
    # slot == wave index at 4-way (today's per-wave partials)
    for sp in range(4):
        for wv in range(4):
            for t in Q.wave_tiles(sp, 4, wv):
                assert Q.place(t) == (sp, wv)
