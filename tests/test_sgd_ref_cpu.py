"""tests/_sgd_ref.py against torch's own SGD in float64 and torch's own AMP functions on the CPU,
the dyadic generator's exactness, and the sensitivity of the GPU file's comparison helpers: a
correct float32 result with one seeded error must be rejected."""
import numpy as np
import pytest
import torch

from . import _sgd_ref as R
from . import test_sgd_amp_exact_gpu as G

SIZES = [5, 12, 1, 17, 7, 3]
GRID = pytest.mark.parametrize("opt", R.OPTION_GRID, ids=R.option_id)


# ------------------------------------------------------------------------------ torch.optim.SGD
@GRID
def test_reference_matches_torch_sgd_float64(opt):
    """Five steps of the reference == torch.optim.SGD on float64 tensors, for every option
    combination of the GPU file (the first step creates the buffers: first on every tensor)."""
    h = R.options(R.FLOAT, *opt)
    gen = torch.Generator().manual_seed(0)
    init = [torch.randn(n, generator=gen) for n in SIZES]
    grads = [[torch.randn(n, generator=gen) for n in SIZES] for _ in range(5)]
    ps = [torch.nn.Parameter(p.double()) for p in init]
    sgd = torch.optim.SGD(ps, foreach=False, **h)
    p, b = init, [torch.zeros_like(x) for x in init]
    for k, gs in enumerate(grads):
        for q, g in zip(ps, gs):
            q.grad = g.double()
        sgd.step()
        o = R.amp_step(p, gs, b, [int(k == 0)] * len(SIZES), **h)
        p, b = o["p"], o["b"] or b
    for i, q in enumerate(ps):
        torch.testing.assert_close(p[i], q.detach(), rtol=1e-13, atol=1e-15)
        if h["momentum"]:
            torch.testing.assert_close(b[i], sgd.state[q]["momentum_buffer"], rtol=1e-13, atol=1e-15)


@GRID
def test_reference_bounds_hold_for_torch_float32(opt):
    """The counted bounds are bounds -- torch's float32 CPU step stays inside them -- and tight
    enough to be a test (p within 1e-6 of |p| + lr (|g| + |buf|))."""
    h = R.options(R.FLOAT, *opt)
    p, g, b = R.normal(SIZES, 1, scale=1.0)
    ps = [torch.nn.Parameter(x.clone()) for x in p]
    sgd = torch.optim.SGD(ps, foreach=False, **h)
    for q, x, y in zip(ps, g, b):
        q.grad = x.clone()
        if h["momentum"]:
            sgd.state[q]["momentum_buffer"] = y.clone()
    sgd.step()
    o = R.amp_step(p, g, b, **h)
    for i, q in enumerate(ps):
        assert bool(((q.detach().double() - o["p"][i]).abs() <= o["bp"][i]).all())
        assert bool((o["bp"][i] <= 1e-6 * (p[i].abs() + h["lr"] * (g[i].abs() + b[i].abs() + 1e-3)).double()).all())
        if h["momentum"]:
            assert bool(((sgd.state[q]["momentum_buffer"].double() - o["b"][i]).abs() <= o["bb"][i]).all())


# ------------------------------------------------------------------------------ torch's AMP functions
def _torch_unscale(grads, scale, found0=0.0):
    gs = [g.clone() for g in grads]
    found = torch.tensor([found0])
    inv = torch.tensor([scale]).double().reciprocal().float()  # grad_scaler.py unscale_
    torch._amp_foreach_non_finite_check_and_unscale_(gs, found, inv)
    return gs, float(found)


@pytest.mark.parametrize("scale", [1024.0, 0.5, 1000.0, 3.0])
@pytest.mark.parametrize("place", [None, (0, 0), (2, 0), (3, 16), (5, 2)])
@pytest.mark.parametrize("val", [float("nan"), float("inf"), -float("inf")])
def test_unscale_check_matches_torch(scale, place, val):
    gen = torch.Generator().manual_seed(2)
    grads = [torch.randn(n, generator=gen) * scale for n in SIZES]
    if place is not None:
        grads[place[0]][place[1]] = val
    want, found = _torch_unscale(grads, scale)
    got, bnd, f = R.unscale_check(grads, scale)
    assert f == bool(found) == (place is not None)
    for x, w, b in zip(got, want, bnd):
        fin = x.isfinite()
        assert bool(((x - w.double()).abs()[fin] <= b[fin]).all())
        assert bool(((x == w.double()) | (x.isnan() & w.isnan()))[~fin].all())
        if R._pow2(scale):
            assert bool(((x.float() == w) | w.isnan()).all())


def test_unscale_check_edges_match_torch():
    # found_inf pre-set stays set
    g = [torch.ones(3)]
    assert _torch_unscale(g, 2.0, 1.0)[1] == 1.0 and R.unscale_check(g, 2.0, 1.0)[2]
    # a finite gradient that overflows only after the unscale: not flagged, becomes inf
    g = [torch.tensor([3e38, -3e38, 1.0])]
    want, found = _torch_unscale(g, 0.5)
    got, _, f = R.unscale_check(g, 0.5)
    assert found == 0.0 and not f and want[0].tolist() == [float("inf"), -float("inf"), 2.0]
    assert torch.equal(got[0].float(), want[0])
    # subnormal results of a power-of-two scale: one correct rounding of the reference
    g = [torch.tensor([2.0 ** -140, 2.0 ** -130, 2.0 ** -120, 3 * 2.0 ** -141, -(2.0 ** -128 + 2.0 ** -149)])]
    want, _ = _torch_unscale(g, 1024.0)
    got, bnd, _ = R.unscale_check(g, 1024.0)
    assert torch.equal(got[0].float(), want[0]) and bool(((got[0] - want[0].double()).abs() <= bnd[0]).all())


@pytest.mark.parametrize("row", R.SCALE_TABLE, ids=lambda r: f"s{r[0]:g}-t{r[1]}-{'inf' if r[2] else 'ok'}-i{r[5]}")
def test_update_scale_matches_torch(row):
    scale, tracker, found, growth, backoff, interval = row
    s, t = torch.tensor([scale]), torch.tensor([tracker], dtype=torch.int32)
    torch._amp_update_scale_(s, t, torch.tensor([float(found)]), growth, backoff, interval)
    assert R.update_scale(*row) == (float(s), int(t))


def test_scale_table_covers_the_branches():
    out = {r: R.update_scale(*r) for r in R.SCALE_TABLE}
    assert out[(1024.0, 2, False, 2.0, 0.5, 3)] == (2048.0, 0)        # growth at the interval
    assert out[(1024.0, 0, False, 2.0, 0.5, 1)] == (2048.0, 0)        # interval == 1
    assert out[(2.0 ** 127, 0, False, 2.0, 0.5, 1)] == (2.0 ** 127, 0)  # would overflow: kept, tracker reset
    assert out[(1024.0, 2, True, 2.0, 0.5, 3)] == (512.0, 0)          # backoff


def test_amp_step_follows_grad_scaler():
    """unscale_ + step + update of torch.amp.GradScaler's code path, float64 SGD: a finite step
    and a skipped one."""
    h = R.options(R.FLOAT, True, False, False, False, True)
    p, g, b = R.normal(SIZES, 3, scale=1024.0)
    for bad in (False, True):
        gs = G._inject(g, 3, 16, float("inf")) if bad else g
        o = R.amp_step(p, gs, b, scale=1024.0, tracker=1, interval=2, **h)
        un, found = _torch_unscale(gs, 1024.0)
        assert o["found"] == bool(found) == bad
        assert (o["scale"], o["tracker"]) == ((512.0, 0) if bad else (2048.0, 0))
        plain = R.amp_step(p, un, b, **h)
        for i in range(len(SIZES)):
            assert torch.equal(o["g"][i].float(), un[i]) or bad
            want = p[i].double() if bad else plain["p"][i]
            assert torch.equal(o["p"][i], want)
            assert torch.equal(o["b"][i], b[i].double() if bad else plain["b"][i])


# ------------------------------------------------------------------------------ the exact leg
def _two_exact_steps(sizes, opt, first1, first2, seed):
    h = R.options(R.DYADIC, *opt)
    p, g, b = R.dyadic(sizes, seed)
    o1 = R.amp_step(p, g, b, first1, scale=1024.0, tracker=0, interval=2, exact=True, **h)
    o2 = R.amp_step(o1["p"], R.dyadic_grads(sizes, seed + 1), o1["b"] or b, first2, scale=o1["scale"],
                    tracker=o1["tracker"], interval=2, exact=True, **h)
    return h, (p, g, b), o1, o2


@GRID
@pytest.mark.parametrize("again", [False, True], ids=["first-once", "first-twice"])
def test_dyadic_two_steps_are_exact(opt, again):
    """The reference's own assertion (x == float32(x) at every rounding point) holds for two
    steps of every option combination, with the first flags the GPU file uses."""
    sizes = [257, 64, 1, 3]
    first = [1, 0, 1, 0] if opt[1] else []
    _, _, o1, o2 = _two_exact_steps(sizes, opt, first, first if again else [], 7)
    for o in (o1, o2):
        for x in o["p"] + o["g"] + o["b"]:
            assert torch.equal(x.float().double(), x)
    assert (o2["scale"], o2["tracker"]) == (2048.0, 0)


def test_dyadic_values():
    p, g, b = R.dyadic([1000], 0, scale=256.0)
    for x, s in ((p[0], 1.0), (g[0], 256.0), (b[0], 1.0)):
        k = x.double() / s * 8
        assert torch.equal(k, k.round()) and float(k.abs().max()) == 16.0
    assert R.DYADIC == dict(lr=0.25, momentum=0.5, dampening=0.25, weight_decay=0.125)


def test_third_step_is_not_exact():
    """Why the exact leg is two steps: with dampening a third step needs multiples of 2^-24."""
    sizes = [4096]
    h, _, _, o2 = _two_exact_steps(sizes, (True, True, False, False, True), [], [], 7)
    with pytest.raises(AssertionError, match="not a float32"):
        R.amp_step(o2["p"], R.dyadic_grads(sizes, 9, 2048.0), o2["b"], scale=o2["scale"], exact=True, **h)


# ------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_gather_reference(dtype):
    imgs = torch.arange(256, dtype=torch.uint8).reshape(8, 32)
    labels, order = torch.arange(8) + 10, torch.tensor([3, 1, 7, 0, 5])
    (one,), lab = R.gather(imgs, labels, order, 1, 2, 1 / 255.0, 0.0, dtype)
    assert lab.tolist() == [17, 10]
    s = torch.tensor(1 / 255.0, dtype=torch.float32)
    assert torch.equal(one, (imgs[[7, 0]].float() * s).to(dtype))  # one rounding, then the type's
    (_,), lab = R.gather(imgs, labels, order, 2, 2, 1 / 255.0, 0.0, dtype)
    assert lab.tolist() == [15, 15]  # position 5 of 5 repeats the last index
    scale, shift = 1 / (255 * 0.3081), -0.1307 / 0.3081
    (fma, two), _ = R.gather(imgs, labels, order, 0, 5, scale, shift, dtype)
    s, sh = torch.tensor(scale, dtype=torch.float32), torch.tensor(shift, dtype=torch.float32)
    assert torch.equal(two, (imgs[order].float() * s + sh).to(dtype))
    if dtype == torch.float32:
        assert not torch.equal(fma, two)  # the contraction is visible
        assert float((fma.double() - two.double()).abs().max()) <= 2.0 ** -23 * 4


# ------------------------------------------------------------------------------ sensitivity
SENS = [5, 12, 1, 17, 7, 3]
SFIRST = [0, 1, 0, 0, 1, 0]


def _f32s(o):
    """The reference rounded to float32: a correct kernel result."""
    return {k: [x.float() for x in o[k]] for k in ("p", "g", "b")}


def _before(p, g, b):
    return {"p": p, "g": g, "b": b}


def _float_case(bad=False, **kw):
    h = R.options(R.FLOAT, True, True, False, False, True)
    p, g, b = R.normal(SENS, 5, scale=1000.0)
    if bad:
        g = G._inject(g, 3, 16, float("nan"))
    kw = dict(dict(scale=1000.0, tracker=1, interval=2), **kw)
    return h, (p, g, b), R.amp_step(p, g, b, SFIRST, **kw, **h)


def test_helpers_accept_the_correct_result():
    for bad in (False, True):
        _, (p, g, b), o = _float_case(bad)
        G.check_step(_f32s(o), o, _before(p, g, b), False, "cpu")
    _, (p, g, b), o1, _ = _two_exact_steps(SENS, (True, True, False, False, True), SFIRST, [], 3)
    G.check_step(_f32s(o1), o1, _before(p, g, b), True, "cpu")


def test_rejects_a_parameter_updated_on_a_skipped_step():
    h, (p, g, b), o = _float_case(bad=True)
    got = _f32s(o)
    assert o["found"] and torch.equal(got["p"][4], p[4])
    got["p"][4][6] -= h["lr"] * got["g"][4][6]
    with pytest.raises(AssertionError, match=r"param\[4\].*index 6"):
        G.check_step(got, o, _before(p, g, b), False, "cpu")


def _wrong_rule(kind, h, p, g, b, first, scale):
    """The float64 step with one mistake a kernel could make."""
    out = {"p": [], "b": []}
    for pi, gi, bi, fi in zip(p, g, b, first):
        pi, gi, bi = pi.double(), gi.double() / scale, bi.double()
        d = gi if kind == "decay-after-momentum" else gi + h["weight_decay"] * pi
        b1 = d.clone() if fi else h["momentum"] * bi + (1 - h["dampening"]) * d
        d2 = b1
        if kind == "nesterov-old-buffer":
            d2 = d + h["momentum"] * bi
        if kind == "decay-after-momentum":
            d2 = d2 + h["weight_decay"] * pi
        out["p"].append((pi - h["lr"] * d2).float())
        out["b"].append(b1.float())
    return out


def test_rejects_nesterov_on_the_old_buffer():
    h = R.options(R.FLOAT, True, False, True, False, True)
    p, g, b = R.normal(SENS, 6, scale=1000.0)
    o = R.amp_step(p, g, b, scale=1000.0, **h)
    got = _f32s(o)
    G.check_step(got, o, _before(p, g, b), False, "cpu")
    got["p"] = _wrong_rule("nesterov-old-buffer", h, p, g, b, [0] * 6, 1000.0)["p"]
    with pytest.raises(AssertionError, match=r"param\[0\]"):
        G.check_step(got, o, _before(p, g, b), False, "cpu")


def test_rejects_weight_decay_added_after_momentum():
    h, (p, g, b), o = _float_case()
    wrong = _wrong_rule("decay-after-momentum", h, p, g, b, SFIRST, 1000.0)
    got = _f32s(o)
    got["p"] = wrong["p"]
    with pytest.raises(AssertionError, match=r"param\[0\]"):
        G.check_step(got, o, _before(p, g, b), False, "cpu")
    got = _f32s(o)
    got["b"] = wrong["b"]
    with pytest.raises(AssertionError, match=r"buf\[0\]"):
        G.check_step(got, o, _before(p, g, b), False, "cpu")


def test_rejects_a_first_flag_shifted_by_one_tensor():
    h, (p, g, b), o = _float_case()
    wrong = R.amp_step(p, g, b, [0] + SFIRST[:-1], scale=1000.0, tracker=1, interval=2, **h)
    with pytest.raises(AssertionError, match=r"param\[1\]"):
        G.check_step(_f32s(wrong), o, _before(p, g, b), False, "cpu")
    got = _f32s(o)
    got["b"] = _f32s(wrong)["b"]
    with pytest.raises(AssertionError, match=r"buf\[1\]"):
        G.check_step(got, o, _before(p, g, b), False, "cpu")


def test_rejects_an_unscale_by_the_post_update_scale():
    h, (p, g, b), o = _float_case()
    assert o["scale"] == 2000.0
    wrong = R.amp_step(p, g, b, SFIRST, scale=1000.0, tracker=1, interval=2, unscale_by=o["scale"], **h)
    with pytest.raises(AssertionError, match=r"param\[0\]"):
        G.check_step(_f32s(wrong), o, _before(p, g, b), False, "cpu")
    got = _f32s(o)
    got["g"] = _f32s(wrong)["g"]
    with pytest.raises(AssertionError, match=r"grad\[0\]"):
        G.check_step(got, o, _before(p, g, b), False, "cpu")


def test_rejects_one_float_written_past_a_tensors_end():
    a = G.Arena(SENS, device="cpu")
    a.load(R.normal(SENS, 8)[0])
    a.check("grad")
    for x, y in zip(a.read(), R.normal(SENS, 8)[0]):
        assert torch.equal(x, y)
    assert all(v.data_ptr() % 16 == 0 for v in a.views)
    a.buf[a.offs[3] + SENS[3]] = 0.25  # numel 17: the second float of its last granule
    with pytest.raises(AssertionError, match=r"0 floats past the end of grad\[3\]"):
        a.check("grad")
    a = G.Arena(SENS, device="cpu")
    a.buf[a.offs[0] - 1] = float("nan")  # another NaN is not the sentinel
    with pytest.raises(AssertionError, match=r"1 floats before grad\[0\]"):
        a.check("grad")


def test_rejects_one_ulp_on_one_parameter_in_the_exact_leg():
    _, (p, g, b), o1, _ = _two_exact_steps(SENS, (True, True, False, False, True), SFIRST, [], 3)
    got = _f32s(o1)
    x = got["p"][3]
    x[9] = torch.nextafter(x[9], torch.tensor(float("inf")))
    with pytest.raises(AssertionError, match=r"param\[3\].*index 9"):
        G.check_step(got, o1, _before(p, g, b), True, "cpu")
    # the float leg's bound is of that order too: four ulps are outside it
    _, (p, g, b), o = _float_case()
    got = _f32s(o)
    x = got["p"][3]
    x[9] += 4 * float(np.spacing(np.float32(abs(float(x[9])))))
    with pytest.raises(AssertionError, match=r"param\[3\].*index 9"):
        G.check_step(got, o, _before(p, g, b), False, "cpu")
