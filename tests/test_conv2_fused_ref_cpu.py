"""Every condition the generators of tests/_conv2_fused_ref.py rely on (no GPU): the exactness limits of
the integer cases, the rounding of the prologue's near-integers to the grid in bf16 / fp16 for any
coefficient the fp32 operations can produce, the decidedness of the pooling index in fp32, the split
map against conv5x5_win_rows, the impulse sets, and the references against torch's own operators."""
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from . import _conv2_fused_ref as X
from . import _convblock_ref as R
from . import _dgrad_rows as Q

U = X.U32
# the cases tests/test_conv2_fused_exact_gpu.py runs (its FWD_CASES and the stale-LDS pair)
FWD = [(1, 11), (3, 13), (3, 17), (2, 19)]
NS = (1, 2, 4)


def _is_multiple(t, step):
    return bool(((t / step).round() * step == t).all())


# ------------------------------------------------------------------------ split map
@pytest.mark.parametrize("ns", NS)
def test_split_map_matches_win_rows(ns):
    """The ranges partition the 196 pixels in order, every one non-empty and whole m-tiles; the widest
    window is conv5x5_win_rows' bound (the header's own figures: 14 rows at 1, 10 at 2, 9 at 4)."""
    # X.win_rows is a transcription: the statements it mirrors must still stand in the header (a change
    # there fails here and asks for the transcription to follow).  On the GPU the partition itself is held
    # by the per-row counts and sums, the windows by the exact y2 of tests/test_conv2_fused_exact_gpu.py.
    hdr = " ".join((Path(__file__).resolve().parent.parent / "ddp_practice_amd/csrc/kernels/conv5x5.h").read_text().split())
    for stmt in ("const int HW = H * W, MT = (HW + 15) / 16;",
                 "const int p0 = 16 * (MT * sp / nsplit), p1e = 16 * (MT * (sp + 1) / nsplit), p1 = p1e < HW ? p1e : HW;",
                 "if (p1 <= p0) return 0;", "int lo = p0 / W - 2, hi = (p1 - 1) / W + 2;", "lo = lo < 0 ? 0 : lo;",
                 "hi = hi > H - 1 ? H - 1 : hi;", "lo &= ~1;", "hi |= 1;", "mx = hi - lo + 1 > mx ? hi - lo + 1 : mx;"):
        assert stmt in hdr, stmt
    ranges = [X.split_pixels(sp, ns) for sp in range(ns)]
    assert ranges[0][0] == 0 and ranges[-1][1] == 196
    for (a0, a1), (b0, b1) in zip(ranges, ranges[1:]):
        assert a1 == b0
    assert all(p1 > p0 and p0 % 16 == 0 for p0, p1 in ranges)
    wins = [X.split_window(sp, ns) for sp in range(ns)]
    assert max(hi - lo + 1 for lo, hi in wins) == X.win_rows(14, 14, ns, False) == {1: 14, 2: 10, 4: 9}[ns]
    assert X.win_rows(14, 14, ns, True) == max((hi | 1) - (lo & ~1) + 1 for lo, hi in wins)
    assert X.win_rows(14, 14, 14, False) == 0  # more workgroups than m-tiles: refused
    for sp in range(ns):  # the quarters of the data gradient are the 4-way ranges
        assert [Q.quarter_pixels(k) for k in Q.quarters_of(sp, ns)][0][0] == ranges[sp][0]


# ------------------------------------------------------------------------ the grid and its rounding
def test_prologue_values_round_to_the_grid():
    """For every t = y1 - shift of the generators (and beyond: |t| <= 8), every gamma and beta, and the
    extreme coefficients gamma * invstd (1 +- K_PRO u) with the two roundings of t * sc + beta on top,
    rounding to bf16 and to fp16 returns the half-integer gamma t + beta; xhat returns t; the
    backward's gi * g returns gamma g.  |z|, |xhat| <= 2^7: half steps are exact in bf16."""
    t = torch.arange(-8, 9, dtype=torch.float64).view(-1, 1, 1, 1)
    gam = torch.tensor(X.GAMMAS_FWD, dtype=torch.float64).view(1, -1, 1, 1)
    beta = torch.tensor([0.5, -0.5], dtype=torch.float64).view(1, 1, -1, 1)
    e = torch.tensor([-1.0, 1.0], dtype=torch.float64).view(1, 1, 1, -1)
    grid = (gam * t + beta).expand(17, 4, 2, 2)
    assert bool((grid != 0).all()) and float(grid.abs().max()) <= 2 ** 7 and _is_multiple(grid * 2, 1.0)
    istd = X.invstd_of(torch.float32)
    assert abs(istd - 1) < 6e-6
    for dtype in X.LP:
        for sgn in (-1.0, 1.0):
            sc = gam * istd * (1 + sgn * X.K_PRO * U)
            z = t * sc + beta + e * 2 * U * ((t * sc).abs() + 0.5)
            assert torch.equal(R.rounded(z, dtype), grid), dtype
            xh = t * istd * (1 + sgn * X.K_PRO * U) + e * U * t.abs()
            assert torch.equal(R.rounded(xh, dtype), t.expand_as(xh)), dtype
    # backward: var + eps = fl(n (1 - eps)) / n + eps = 1 to 2 u
    g = torch.arange(-3, 4, dtype=torch.float64).view(-1, 1, 1)
    gb = torch.tensor(X.GAMMAS_BWD, dtype=torch.float64).view(1, -1, 1)
    for n in (196, 588, 25 * 196):
        f = X.bwd_fstats(n)
        assert abs(float(f[32]) / n + X.EPS32 - 1) < 2 * U and bool((f[:32] == 0).all()) and bool((f[65:] == 0).all())
    for dtype in X.LP:
        dy = gb * (1 + e.view(1, 1, -1) * X.K_PRO * U) * g
        assert torch.equal(R.rounded(dy, dtype), (gb * g).expand_as(dy)), dtype


@pytest.mark.parametrize("Bn,seed", FWD)
def test_forward_case_limits(Bn, seed):
    c = X.fwd_int(Bn, seed)
    t = c["y1"] - c["shift1"].view(1, -1, 1, 1)
    assert _is_multiple(c["y1"], 1.0) and float(t.abs().max()) <= X.TMAX and float(c["y1"].abs().max()) <= 2 ** 7
    assert bool((c["gamma"].abs() >= 1).all()) and bool((c["beta"].abs() == 0.5).all())
    # the given statistics: integer rows, exact column sums [0 | n | n] in any order
    rows1 = c["rows1"]
    assert rows1.shape == (4 * Bn, 33) and int(rows1.abs().sum(0).max()) < R.EXACT
    assert torch.equal(rows1.sum(0), torch.cat([torch.zeros(16), torch.full((17,), c["n"])]).long())
    for dtype in R.DTYPES:
        for ns in NS:
            r = X.fwd_ref(c, dtype, ns)
            if dtype in X.LP:
                assert _is_multiple(r["z"], 0.5) and bool((r["z"] != 0).all()) and float(r["z"].abs().max()) <= 2 ** 7
                assert torch.equal(R.rounded(r["z"], dtype), r["z"]) and torch.equal(R.rounded(r["p1"], dtype), r["p1"])
                assert _is_multiple(r["xh1"], 1.0) and float(r["xh1"].abs().max()) <= X.TMAX
                # 400-term sums in units of 1/2; the rows' sums in units of 1/2 and 1/4
                assert 2 * float(r["A_y2"].max()) < R.EXACT
                d = r["d"]
                for sp in range(ns):
                    p0, p1 = X.split_pixels(sp, ns)
                    assert 2 * float(d[:, :, p0:p1].abs().sum(-1).max()) < R.EXACT
                    assert 4 * float((d[:, :, p0:p1] ** 2).sum(-1).max()) < R.EXACT
            frac = float((r["p1"] > 0).double().mean())
            assert 0.15 < frac < 0.35, frac  # about a quarter of the pooled pixels
            assert float(r["p1"].max()) <= 4.5
            assert bool((r["rows"][:, 64] == torch.tensor([X.split_pixels(sp, ns)[1] - X.split_pixels(sp, ns)[0]
                                                           for sp in range(ns)] * Bn)).all())
    # ties: windows whose maximum is positive and attained twice, and windows with nothing positive
    r = X.fwd_ref(c, torch.bfloat16, 4)
    aw = R.windows(r["z"].clamp(min=0))
    twice = (aw == aw.max(-1, keepdim=True).values).sum(-1) >= 2
    assert int((twice & (r["p1"] > 0)).sum()) >= 8 and int((r["p1"] == 0).sum()) > 0
    # a tie later in the window than its first maximum exists: "last maximum wins" would differ
    last = 3 - R.first_max(aw.flip(-1))
    assert int((last != (r["idx1"] & 3)).sum()) > 100


@pytest.mark.parametrize("Bn,seed", FWD)
def test_forward_index_is_decided_in_fp32(Bn, seed):
    """fp32: |z| and the gap between two candidates of different inputs exceed twice the bound
    K_PRO u A_z by orders of magnitude, so idx1 (argmax and ReLU bit) is the integer case's."""
    c = X.fwd_int(Bn, seed)
    r, ri = X.fwd_ref(c, torch.float32, 4), X.fwd_ref(c, torch.bfloat16, 4)
    bnd = X.K_PRO * U * r["A_z"]
    assert float(bnd.max()) < 1e-5 and float(r["z"].abs().min()) > 0.49
    zw = R.windows(r["z"])
    gap = (zw.unsqueeze(-1) - zw.unsqueeze(-2)).abs()
    assert float(gap[gap > 0].min()) > 0.49  # equal inputs give equal values; others are >= invstd / 2 apart
    assert torch.equal(r["idx1"], ri["idx1"])
    # and the fp32 reference is the integer one to 6e-6 relative
    assert float((r["y2"] - ri["y2"]).abs().max()) <= 6e-6 * float(r["A_y2"].max()) + 0.5  # (bf16 rounds y2 > 128)
    assert float((r["p1"] - ri["p1"]).abs().max()) < 1e-4


@pytest.mark.parametrize("Bn,seed", FWD[:2])
def test_forward_reference_against_torch(Bn, seed):
    c = X.fwd_int(Bn, seed)
    r = X.fwd_ref(c, torch.float32, 4)
    var = torch.ones(16, dtype=torch.float64)
    z = F.batch_norm(c["y1"], c["shift1"].clone(), var, c["gamma"], c["beta"], False, 0.0, X.EPS32)
    p, ind = F.max_pool2d(F.relu(z), 2, 2, return_indices=True)
    y2 = F.conv2d(p, c["w2"], c["bias2"], padding=2)
    assert torch.allclose(r["p1"], p, rtol=1e-12, atol=1e-12) and torch.allclose(r["y2"], y2, rtol=1e-12, atol=1e-12)
    pos = ((ind // 28) % 2) * 2 + (ind % 28) % 2
    one = (R.windows(F.relu(z)) == p.unsqueeze(-1)).sum(-1) == 1  # torch's index where the maximum is unique
    assert torch.equal((r["idx1"] & 3).long()[one], pos[one])
    assert torch.equal((r["idx1"] & 4) != 0, p > 0)
    d = y2 - c["rm2"].view(1, -1, 1, 1)
    tot = r["rows"].view(Bn, 4, 65).sum(1)
    assert torch.allclose(tot[:, :32], d.sum((2, 3))) and torch.allclose(tot[:, 32:64], (d * d).sum((2, 3)))
    assert bool((r["A_y2"] >= r["y2"].abs() - 1e-9).all())


def test_running_statistics_move():
    """One update differs from none and from two by far more than the bound of the check."""
    for Bn, seed in FWD:
        c = X.fwd_int(Bn, seed)
        st = X.fwd_running(c)
        assert torch.equal(st["mean"], c["shift1"]) and bool((st["var"] == 1).all())
        bnd_m, bnd_v = R.B.bound(st["A_rm"], st["rm"], torch.float32), R.B.bound(st["A_rv"], st["rv"], torch.float32)
        twice_m = 0.9 * st["rm"] + 0.1 * st["mean"]
        twice_v = 0.9 * st["rv"] + 0.1 * c["n"] / (c["n"] - 1.0)
        far = lambda a, b, bnd: bool(((a - b).abs() > 1000 * bnd).all())  # noqa: E731
        assert far(st["rm"], c["rm0"], bnd_m) and far(st["rm"], twice_m, bnd_m)
        assert far(st["rv"], c["rv0"], bnd_v) and far(st["rv"], twice_v, bnd_v)


# ------------------------------------------------------------------------ impulse sets
@pytest.mark.parametrize("variant", [0, 1])
def test_forward_impulse_set(variant):
    c, where = X.fwd_impulse(variant, 4)
    r = X.fwd_ref(c, torch.bfloat16, 4)
    assert torch.equal((r["p1"] != 0).sum((1, 2, 3)), torch.ones(25, dtype=torch.long))
    y2 = r["y2"]
    for t, (co, oh, ow, val) in enumerate(where):
        assert y2[t, co, oh, ow] == val and val != 0
        # t and t + 16 share an input channel: the other one's weight too, where its pixel is inside the image
        assert int((y2[t] != 0).sum()) in ((1, 2) if t < 9 or t >= 16 else (1,))
        ph, pw = (r["p1"][t] != 0).nonzero()[0, 1:].tolist()
        kh, kw = t // 5, t % 5
        assert (ph - kh + 2, pw - kw + 2) == (oh, ow)
        if variant == 0:  # the output pixel is the first or the last of a workgroup's range
            assert oh * 14 + ow in [p for sp in range(4) for p in (X.split_pixels(sp, 4)[0], X.split_pixels(sp, 4)[1] - 1)]
        else:
            assert ph in (0, 13) and pw in (0, 13)
    if variant == 0:  # every kh = 0 / kh = 4 tap reads the first / last row of its workgroup's row window
        for t, (co, oh, ow, val) in enumerate(where):
            kh, ph = t // 5, oh + t // 5 - 2
            sp = [s for s in range(4) if X.split_pixels(s, 4)[0] <= oh * 14 + ow < X.split_pixels(s, 4)[1]][0]
            lo, hi = X.split_window(sp, 4)
            assert lo <= ph <= hi
            if kh == 0:
                assert ph == lo and oh * 14 + ow == X.split_pixels(sp, 4)[0], (t, ph, lo)
            if kh == 4:
                assert ph == hi and oh * 14 + ow == X.split_pixels(sp, 4)[1] - 1, (t, ph, hi)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("co,ci", [(3, 2), (20, 13)])
def test_wgrad_impulse_set(variant, co, ci):
    c, where = X.wgrad_impulse(variant, co, ci, 5)
    rows, A = X.wgrad_ref(c)
    for t, (col, val, dbv) in enumerate(where):
        want = torch.zeros(X.N2, dtype=torch.float64)
        want[col], want[12800 + co] = val, dbv
        assert torch.equal(rows[t], want) and val != 0
        assert col // (25 * 16) // 16 == co // 16 and (col // 25) % 16 // 8 == ci // 8  # (output tile, slice of 2)


# ------------------------------------------------------------------------ backward cases
@pytest.mark.parametrize("Bn", [1, 2, 3])
def test_wgrad_case_limits(Bn):
    c = X.wgrad_int(Bn, 30 + Bn)
    assert _is_multiple(c["dy"], 0.5) and float(c["dy"].abs().max()) <= 6
    rows, A = X.wgrad_ref(c)
    assert rows.shape == (Bn, X.N2) and 2 * float(A.max()) < R.EXACT
    w = torch.nn.grad.conv2d_weight(c["p1"], (32, 16, 5, 5), c["dy"], padding=2)
    assert torch.equal(rows[:, :12800].sum(0), w.reshape(-1)) and torch.equal(rows[:, 12800:].sum(0), c["dy"].sum((0, 2, 3)))
    assert int(c["lsum"].abs().sum(0).max()) < R.EXACT
    # both bits of the index byte and both output tiles / slices carry weight
    assert int(((c["idx2"] & 4) != 0).sum()) > 0 and int(((c["idx2"] & 4) == 0).sum()) > 0


@pytest.mark.parametrize("Bn", [1, 3])
def test_dgrad_case_limits(Bn):
    c = X.dgrad_int(Bn, 50 + Bn)
    r = X.dgrad_ref(c)
    assert 2 * float(r["A"].max()) < R.EXACT and 2 * float(r["A_rows"].max()) < R.EXACT
    assert torch.equal(r["dp1"], F.conv_transpose2d(c["dy"], c["w2"], padding=2))
    assert r["rows"].shape == (4 * Bn, 32) and bool((r["A_rows"] >= r["rows"].abs()).all())
