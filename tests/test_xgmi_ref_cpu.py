"""tests/_xgmi_ref.py checked on the CPU: against a float64 sum within the W - 1 roundings it
makes, exact on integers in any rank order, the two-shot round trip idempotent, and its comparison
helpers against seeded mistakes -- each must be rejected on this file's own randn inputs, or the
inputs of tests/test_xgmi_exact_gpu.py (the same generator) would be too tame to see it."""
import numpy as np
import pytest
import torch

from . import _xgmi_ref as X

U32 = 2.0 ** -24
HALF_ULP = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
N = 4099


def _randn(world, n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g).to(dtype) for _ in range(world)]


@pytest.mark.parametrize("world", [2, 3, 4, 8])
@pytest.mark.parametrize("dn", list(X.DTYPES))
@pytest.mark.parametrize("op", ["sum", "avg"])
def test_reduce_within_its_roundings_of_float64(world, dn, op):
    """W - 1 additions, for avg the rounding of 1/W and of the product, then one rounding to the
    storage type (half an ulp of it; 2^-25 absolute below fp16's normal range)."""
    dt = X.DTYPES[dn]
    xs = _randn(world, N, dt, 3)
    got = X.reduce(xs, op, dt).double()
    d = [x.double() for x in xs]
    ref = sum(d[1:], d[0])
    mag = sum(x.abs() for x in d)
    bound = (world - 1) * U32 * mag * (1 + 1e-6)
    if op == "avg":
        ref, bound = ref / world, bound / world + 2 * U32 * mag / world
    bound = bound + HALF_ULP[dt] * (ref.abs() + bound) + (2.0 ** -25 if dt == torch.float16 else 0.0)
    err = (got - ref).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    if dt == torch.float32 and op == "sum":
        assert float(err.max()) > 0  # and it does round: not a float64 sum in disguise


@pytest.mark.parametrize("dn", list(X.DTYPES))
def test_reduce_exact_on_integers_in_any_order(dn):
    dt = X.DTYPES[dn]
    g = torch.Generator().manual_seed(5)
    xs = [torch.randint(-16, 17, (N,), generator=g).to(dt) for _ in range(8)]
    exact = sum(x.double() for x in xs)
    for perm in ([0, 1, 2, 3, 4, 5, 6, 7], [7, 6, 5, 4, 3, 2, 1, 0], [3, 0, 7, 1, 6, 2, 5, 4]):
        ys = [xs[i] for i in perm]
        assert not bool(X.mismatch(X.reduce(ys, "sum", dt), exact.to(dt)).any())
        assert not bool(X.mismatch(X.reduce(ys, "avg", dt), (exact / 8).to(dt)).any())  # 1/8 is exact
        assert torch.equal(X.reduce(ys, "max", dt).double(), torch.stack([x.double() for x in xs]).max(0).values)
        assert torch.equal(X.reduce(ys, "min", dt).double(), torch.stack([x.double() for x in xs]).min(0).values)


def _with_specials(xs, dt):
    """Every SPECIALS entry on rank 1 (pairs: ranks 1 and 2), one element each."""
    xs = [x.clone() for x in xs]
    for i, sp in enumerate(X.SPECIALS):
        for k, v in enumerate(sp):
            xs[(1 + k) % len(xs)][i] = v
    return xs


@pytest.mark.parametrize("world", [2, 3, 4])
@pytest.mark.parametrize("dn", list(X.DTYPES))
@pytest.mark.parametrize("op", X.OPS)
def test_twoshot_round_trip_is_idempotent(world, dn, op):
    dt = X.DTYPES[dn]
    xs = _randn(world, N, dt, 7)
    if op in ("sum", "avg"):
        xs = _with_specials(xs, dt)
    one, two = X.reduce(xs, op, dt), X.reduce_twoshot(xs, op, dt)
    assert not bool(X.mismatch(two, one).any()) and not bool(X.mismatch(one, two).any())
    assert torch.equal(X.bits(one)[~one.isnan()], X.bits(two)[~two.isnan()])


@pytest.mark.parametrize("dn", list(X.DTYPES))
def test_specials_behave_as_ieee_says(dn):
    dt = X.DTYPES[dn]
    world = 3
    xs = _with_specials(_randn(world, 64, dt, 9), dt)
    nonfinite = ~torch.stack([x.float().isfinite() for x in xs]).all(0)
    assert int(nonfinite.sum()) >= 4
    for op in ("sum", "avg"):
        out = X.reduce(xs, op, dt)
        assert not bool(out[nonfinite].isfinite().any())  # a rank's non-finite value reaches every rank
    names = {sp: i for i, sp in enumerate(X.SPECIALS)}
    s = X.reduce(xs, "sum", dt)
    assert bool(s[names[(float("inf"), float("-inf"))]].isnan())
    assert bool(s[names[(3e38, 3e38)]].isinf())  # fp32 overflow (fp16: both inputs already inf)
    if dt == torch.float16:
        i = names[(60000.0, 60000.0)]
        assert all(bool(x[i].isfinite()) for x in xs) and bool(s[i].isinf())
        assert bool(X.reduce(xs, "avg", dt)[i].isfinite()) == (world > 2)  # 120000 / 3 fits, the sum does not
    # signed zero: -0 from every rank stays -0, and the comparison tells it from +0
    z = [torch.full((4,), -0.0).to(dt) for _ in range(world)]
    out = X.reduce(z, "sum", dt)
    assert bool((X.bits(out) != 0).all()) and bool(X.mismatch(out, torch.zeros(4).to(dt)).all())
    assert not bool(X.mismatch(torch.tensor([float("nan")]).to(dt), -torch.tensor([float("nan")]).to(dt)).any())
    assert bool(X.mismatch(torch.tensor([1.0]).to(dt), torch.tensor([float("nan")]).to(dt)).all())


def test_site_sum_and_xg_average_are_the_f32_reduce():
    xs = _randn(3, N, torch.float32, 11)
    assert torch.equal(X.site_sum(xs), X.reduce(xs, "sum", torch.float32))
    grads = [[x[:7], x[7:]] for x in xs]
    avg = torch.cat(X.xg_average(grads))
    assert torch.equal(avg, X.reduce(xs, "avg", torch.float32))
    assert float(X.inv_world(3)) == float(np.float32(1.0 / 3.0)) != 1.0 / 3.0


# ------------------------------------------------------------------------------ seeded mistakes
def _f(xs):
    return [x.float().numpy() for x in xs]


def _reversed(xs, dt):
    return X.reduce(xs[::-1], "sum", dt)


def _divided(xs, dt):
    a = _f(xs)
    return torch.from_numpy((a[0] + a[1] + a[2]) / np.float32(3)).to(dt)


def _storage_accumulation(xs, dt):
    acc = xs[0].clone()
    for x in xs[1:]:
        acc = (acc.float() + x.float()).to(dt)
    return acc


def _rounded_before_average(xs, dt):
    a = _f(xs)
    s = torch.from_numpy(a[0] + a[1] + a[2]).to(dt).float().numpy()
    return torch.from_numpy(s * X.inv_world(3)).to(dt)


# (a reversed order under a 16-bit result is hidden by the last rounding: fp32 shows it)
MISTAKES = [("reversed rank order", _reversed, "sum", "f32"),
            ("division, not the multiply", _divided, "avg", "f32"),
            ("accumulation in the storage type", _storage_accumulation, "sum", "bf16"),
            ("accumulation in the storage type", _storage_accumulation, "sum", "f16"),
            ("rounded to the storage type before the average", _rounded_before_average, "avg", "bf16"),
            ("rounded to the storage type before the average", _rounded_before_average, "avg", "f16")]


@pytest.mark.parametrize("name,fn,op,dn", MISTAKES, ids=[f"{m[0]}-{m[3]}" for m in MISTAKES])
def test_arithmetic_mistakes_are_rejected(name, fn, op, dn):
    dt = X.DTYPES[dn]
    xs = _randn(3, N, dt, 13)
    want = X.reduce(xs, op, dt)
    wrong = fn(xs, dt)
    share = float(X.mismatch(wrong, want).float().mean())
    assert share > 0.01, (name, share)
    with pytest.raises(AssertionError, match="elements differ"):
        X.assert_bits(wrong, want, name)


@pytest.mark.parametrize("dn", list(X.DTYPES))
@pytest.mark.parametrize("n", [1, 7, 2049])
def test_placement_mistakes_are_rejected(dn, n):
    dt = X.DTYPES[dn]
    xs, prev = _randn(3, n, dt, 17), _randn(3, n, dt, 18)
    want = X.reduce(xs, "sum", dt)
    g = X.Guarded(n, dt)
    g.load(want)
    assert g.check(want, "clean") == n
    # one tail element left at its sentinel -- also where the reference is NaN
    g.load(want)
    g.buf[X.GUARD + n - 1:X.GUARD + n] = X.sentinel(1, dt)
    with pytest.raises(AssertionError, match="still holds the sentinel"):
        g.check(want, "tail")
    nan_want = want.clone()
    nan_want[n - 1] = float("nan")
    with pytest.raises(AssertionError, match="still holds the sentinel"):
        g.check(nan_want, "tail, NaN reference")
    # one element taken from the previous call's data
    stale = want.clone()
    stale[n // 2] = X.reduce(prev, "sum", dt)[n // 2]
    g.load(stale)
    with pytest.raises(AssertionError, match="elements differ"):
        g.check(want, "stale")
    # a write one element past n, and one before the start
    for at, msg in ((X.GUARD + n, "0 past the end"), (X.GUARD - 1, "1 before the start")):
        g.load(want)
        g.buf[at] = 1.0
        with pytest.raises(AssertionError, match=msg):
            g.check(want, "overrun")
