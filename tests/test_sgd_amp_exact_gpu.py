"""The optimizer / AMP kernels every step ends with (csrc/kernels/optim.hip, amp_step.h), kernel by
kernel against the float64 reference of tests/_sgd_ref.py (pure torch on the CPU, checked
against torch's own SGD and AMP functions in test_sgd_ref_cpu.py): bit for bit on the dyadic
inputs, per element within the counted bound on floats.

  a  unscale_check   CHUNK edges, batch splits (37 / 73 tensors), one non-finite at a time
  b  sgd_step        the option grid, first flags across batches, found_inf, grad_scale, lr_dev
  c  update_scale    torch._amp_update_scale_'s table, found_inf re-armed
  d  amp_sgd_fused   36 tensors; a grid of one, U = 1 / 2 / 4; plain mode; pre-checked mode; the
                     slab source (with a peer: tests/test_xgmi_exact_gpu.py)
  e  amp_sgd_large   1 / 37 / 512 tensors, the table reused eager and graph-replayed
  f  flat_copy       both directions, gaps, s = 0.5 and 1/3

Every tensor is a 16-byte aligned view into one buffer pre-filled with a NaN sentinel; the
padding between the views is compared bitwise after every launch, so a store past a tensor's
end is seen.  A failing element is named by tensor and index.  The largest error / bound ratio
of the float sections is printed by the last test; measured on an MI355X against the float64
reference:

  unscale_check   0.896 (grad[17])      sgd_step        0.987 (param[65])
  amp_sgd_fused   0.989 (param[17])     amp_sgd_large   0.983 (param[12])

(half an ulp is u |x| for an x just above a power of two, so the last rounding alone comes close
to its term among a few hundred thousand elements; no element is outside the bound).  The host accepts a
zero-element tensor in unscale_check's list, so that case runs; nothing was left out.
"""
import numpy as np
import pytest
import torch

from . import _sgd_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN, INF = float("nan"), float("inf")
SENT = 0x7FC0BEEF  # a quiet NaN no kernel produces
RATIOS = {}
NAMES = {"p": "param", "g": "grad", "b": "buf"}
CYCLE = [1, 3, 4095, 4096, 4097, 8193, 6]  # CHUNK = 4096 edges, numel % 4 in 1, 2, 3


# ------------------------------------------------------------------------------ helpers
class Arena:
    """Tensors as 16-byte aligned views into one sentinel-filled float32 buffer, ``gap`` floats
    (and the rest of the last granule) of padding around each."""

    def __init__(self, sizes, device=DEV, gap=4):
        self.sizes, self.offs = list(sizes), []
        o = gap
        for n in self.sizes:
            self.offs.append(o)
            o += (n + 3) // 4 * 4 + gap
        self.total = o
        self.pad = torch.ones(o, dtype=torch.bool)
        for a, n in zip(self.offs, self.sizes):
            self.pad[a:a + n] = False
        self.buf = torch.full((o,), SENT, dtype=torch.int32, device=device).view(torch.float32)
        self.views = [self.buf[a:a + n] for a, n in zip(self.offs, self.sizes)]

    def load(self, tensors):
        host = torch.full((self.total,), SENT, dtype=torch.int32).view(torch.float32)
        for a, n, t in zip(self.offs, self.sizes, tensors):
            host[a:a + n] = t.float()
        self.buf.copy_(host)

    def read(self):
        host = self.buf.cpu()
        return [host[a:a + n].clone() for a, n in zip(self.offs, self.sizes)]

    def check(self, name):
        """The padding still holds the sentinel, bit for bit."""
        raw = self.buf.cpu().view(torch.int32)
        bad = (raw != SENT) & self.pad
        if bool(bad.any()):
            at = int(bad.nonzero()[0])
            t = max((i for i, a in enumerate(self.offs) if a <= at), default=-1)
            where = f"{at - self.offs[t] - self.sizes[t]} floats past the end of {name}[{t}]" if t >= 0 \
                else f"{self.offs[0] - at} floats before {name}[0]"
            raise AssertionError(f"{name}: {int(bad.sum())} padding words overwritten, first {where} "
                                 f"(numel {self.sizes[max(t, 0)]}): {raw[at].item():#x}")


def same_bits(got, want, name):
    a, b = got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)
    bad = a != b
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} of {b.numel()} changed, first at index "
                                 f"{int(bad.nonzero()[0])}: got {got[bad][0].item()!r} want {want[bad][0].item()!r}")


def same(got, want, name):
    """Every element equals the float64 reference (NaN where it is NaN)."""
    g = got.double()
    bad = ~((g == want) | (g.isnan() & want.isnan()))
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} of {want.numel()} differ, first at index "
                                 f"{int(bad.nonzero()[0])}: got {g[bad][0].item()!r} want {want[bad][0].item()!r}")


def within(got, ref, bnd, name, section):
    """|got - ref| <= bnd on every element; a non-finite reference value must be met as it is."""
    g = got.double()
    if g.numel() == 0:
        return
    fin = ref.isfinite()
    err = torch.where(fin, (g - ref).abs(), torch.zeros_like(ref))
    ok = torch.where(fin, err <= bnd, (g == ref) | (g.isnan() & ref.isnan()))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd.clamp(min=1e-300))
    worst = float(ratio.max()) if not bool(ratio.isnan().any()) else INF
    assert bool(ok.all()), (f"{name}: {int((~ok).sum())} of {ref.numel()} outside the bound, first at index "
                            f"{int((~ok).nonzero()[0])}: got {g[~ok][0].item()!r} want {ref[~ok][0].item()!r}, "
                            f"error / bound <= {worst:.3g}")
    if worst >= RATIOS.get(section, (0.0, ""))[0]:
        RATIOS[section] = (worst, name)


def check_step(got, ref, before, exact, section):
    """One step's params, grads and buffers (lists of float32 CPU tensors) against
    ``_sgd_ref.amp_step``'s result: a skipped step leaves params and buffers bitwise as before,
    the plain mode the grads, no momentum the buffers."""
    for key in ("p", "g", "b"):
        want, bnd = ref[key], ref["b" + key]
        untouched = (key != "g" and ref["found"]) or (key == "g" and ref["scale"] is None) or \
                    (key == "b" and not want)
        assert untouched or len(got[key]) == len(want)
        for i, x in enumerate(got[key]):
            name = f"{NAMES[key]}[{i}]"
            if untouched:
                same_bits(x, before[key][i], name)
            elif exact:
                same(x, want[i], name)
            else:
                within(x, want[i], bnd[i], name, section)


def check_scalars(st, ref, sync0=None):
    assert float(st.scale) == ref["scale"], (float(st.scale), ref["scale"])
    assert int(st.tracker) == ref["tracker"], (int(st.tracker), ref["tracker"])
    assert float(st.found) == 0.0  # re-armed
    sync = st.sync.tolist()
    if sync0 is not None:
        assert sync[0] == sync0, (sync, sync0)
    assert sync[3] == 0, sync


class State:
    def __init__(self, sizes, device=DEV):
        self.sizes = list(sizes)
        self.P, self.G, self.B = Arena(sizes, device), Arena(sizes, device), Arena(sizes, device)
        self.scale = torch.zeros(1, device=device)
        self.tracker = torch.zeros(1, dtype=torch.int32, device=device)
        self.found = torch.zeros(1, device=device)
        self.sync = torch.zeros(4, dtype=torch.int64, device=device)

    def load(self, p, g, b, scale=1.0, tracker=0, found=0.0):
        self.P.load(p)
        self.G.load(g)
        self.B.load(b)
        self.scale.fill_(scale)
        self.tracker.fill_(tracker)
        self.found.fill_(found)

    def read(self):
        return {"p": self.P.read(), "g": self.G.read(), "b": self.B.read()}

    def check_pads(self):
        self.P.check("param")
        self.G.check("grad")
        self.B.check("buf")


def _run(st, launch, exact, section, *, first=(), amp=True, sync_step=None, tracker=None, found_inf=0.0,
         gbi=(2.0, 0.5, 2), scalars=True, **kw):
    """Read the state, launch, and compare every output with the reference's step from that
    state.  ``sync_step``: by how much sync[0] must advance."""
    before = st.read()
    scale, trk, s0 = float(st.scale), int(st.tracker), int(st.sync[0])
    launch()
    torch.cuda.synchronize()
    got = st.read()
    st.check_pads()
    ref = R.amp_step(before["p"], before["g"], before["b"], first, scale=scale if amp else None, tracker=trk,
                     found_inf=found_inf, growth=gbi[0], backoff=gbi[1], interval=gbi[2], exact=exact, **kw)
    check_step(got, ref, before, exact, section)
    if amp and scalars:
        check_scalars(st, ref, None if sync_step is None else s0 + sync_step)
    elif sync_step is not None:
        assert int(st.sync[0]) == s0 + sync_step and int(st.sync[3]) == 0
    return ref


def _graph(launch):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    return g


def _inject(grads, t, i, val):
    out = [g.clone() for g in grads]
    out[t][i] = val
    return out


# =============================================================================== a
def _list(n, zero_at=None):
    sizes = [CYCLE[i % len(CYCLE)] for i in range(n)]
    if zero_at is not None:
        sizes[zero_at] = 0
    return sizes


def _unscale(C, st, grads, scale, found0=0.0):
    st.G.load(grads)
    st.scale.fill_(scale)
    st.found.fill_(found0)
    C.optim.unscale_check(st.G.views, st.scale, st.found)
    torch.cuda.synchronize()
    st.G.check("grad")
    return st.G.read(), float(st.found)


class _GradsOnly:
    def __init__(self, sizes):
        self.G = Arena(sizes)
        self.scale, self.found = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)


@pytest.mark.parametrize("n", [37, 73])
def test_unscale_check_finite(C, n):
    """Random gradients with subnormal results among them: a power-of-two scale is bit-exact (one
    correct rounding below the normal range), any other within 2u; found_inf stays as it was.
    A zero-element tensor sits in the middle of the list."""
    sizes = _list(n, zero_at=n // 2)
    st = _GradsOnly(sizes)
    _, grads, _ = R.normal(sizes, n, scale=1.0)
    # 2^-140 / 2^10 (a tie below the smallest subnormal), subnormal results from a subnormal and
    # from a normal input, and one that rounds inside the subnormal range
    grads[0][0] = 2.0 ** -140
    grads[1][:3] = torch.tensor([2.0 ** -130, 2.0 ** -120, 3 * 2.0 ** -141])
    grads[4][4096] = -(2.0 ** -128 + 2.0 ** -149)
    for scale in (1024.0, 2.0 ** -3):
        got, found = _unscale(C, st, grads, scale)
        want, _, f = R.unscale_check(grads, scale)
        assert found == 0.0 and not f
        for i, (x, w) in enumerate(zip(got, want)):
            same(x, w.float().double(), f"grad[{i}]")
    for scale in (1000.0, 3.0):
        got, found = _unscale(C, st, grads, scale)
        want, bnd, _ = R.unscale_check(grads, scale)
        assert found == 0.0
        for i, (x, w, b) in enumerate(zip(got, want, bnd)):
            within(x, w, b, f"grad[{i}]", "unscale_check")
    # found_inf pre-set with finite gradients stays set
    _, found = _unscale(C, st, grads, 1024.0, found0=1.0)
    assert found == 1.0


def test_unscale_check_one_nonfinite_at_a_time(C):
    """found_inf is exactly 1 wherever the one non-finite value sits -- the first and the last
    element of the list, the last element of a partial granule, both sides of a CHUNK edge,
    every batch -- and every other element is still unscaled."""
    sizes = _list(73, zero_at=36)
    st = _GradsOnly(sizes)
    _, grads, _ = R.normal(sizes, 5, scale=512.0)
    assert [sizes[i] % 4 for i in (4, 6, 1)] == [1, 2, 3] and sizes[4] == 4097 and sizes[53] == 4097
    places = [(0, 0), (72, sizes[72] - 1), (4, 4096), (6, 5), (1, 2), (4, 4095), (53, 2000), (72, 100), (37, 0)]
    for t, i in places:
        for val in (NAN, INF, -INF):
            gs = _inject(grads, t, i, val)
            got, found = _unscale(C, st, gs, 512.0)
            want, _, f = R.unscale_check(gs, 512.0)
            assert f and found == 1.0, (t, i, val, found)
            for k, (x, w) in enumerate(zip(got, want)):
                same(x, w, f"grad[{k}] (non-finite at grad[{t}][{i}])")


def test_unscale_check_overflow_after_unscale_is_not_flagged(C):
    st = _GradsOnly([3])
    got, found = _unscale(C, st, [torch.tensor([3e38, -3e38, 1.0])], 0.5)
    assert found == 0.0 and got[0].tolist() == [INF, -INF, 2.0]


# =============================================================================== b
FIRST73 = [int(i in (35, 36, 71, 72)) for i in range(73)]


def _sgd(C, st, h, first=(), found=None, grad_scale=None, lr_dev=None, lr=None):
    C.optim.sgd_step(st.P.views, st.G.views, st.B.views, h["lr"] if lr is None else lr, h["momentum"],
                     h["dampening"], h["weight_decay"], h["nesterov"], h["maximize"], list(first), found, grad_scale,
                     lr_dev)


@pytest.mark.parametrize("opt", R.OPTION_GRID, ids=R.option_id)
def test_sgd_step_exact_two_steps(C, opt):
    """73 tensors (three launches), first flags on both sides of each batch split."""
    sizes = _list(73)
    h = R.options(R.DYADIC, *opt)
    st = State(sizes)
    p, g, b = R.dyadic(sizes, 11, scale=1.0)
    st.load(p, g, b)
    first = FIRST73 if opt[1] else ()
    _run(st, lambda: _sgd(C, st, h, first), True, "sgd_step", first=first, amp=False, **h)
    st.G.load(R.dyadic_grads(sizes, 12, scale=1.0))
    _run(st, lambda: _sgd(C, st, h), True, "sgd_step", amp=False, **h)


def test_sgd_step_found_inf_grad_scale_lr_dev(C):
    sizes = _list(73)
    h = R.options(R.DYADIC, True, True, False, False, True)
    st = State(sizes)
    p, g, b = R.dyadic(sizes, 13, scale=1.0)
    # found_inf set: nothing moves
    st.load(p, g, b, found=1.0)
    _run(st, lambda: _sgd(C, st, h, FIRST73, found=st.found), True, "sgd_step", first=FIRST73, amp=False,
         found_inf=1.0, **h)
    assert float(st.found) == 1.0  # only update_scale re-arms it
    # found_inf clear, grad_scale given: the gradients are divided inside the rule, not in memory
    gs = torch.tensor([256.0], device=DEV)
    st.load(p, [x * 256.0 for x in g], b)
    _run(st, lambda: _sgd(C, st, h, FIRST73, found=st.found, grad_scale=gs), True, "sgd_step", first=FIRST73,
         amp=False, grad_scale=256.0, **h)
    # lr_dev: the word wins over the by-value rate
    word = torch.tensor([h["lr"]], device=DEV)
    st.load(p, g, b)
    _run(st, lambda: _sgd(C, st, h, FIRST73, lr_dev=word, lr=0.5), True, "sgd_step", first=FIRST73, amp=False, **h)


@pytest.mark.parametrize("opt", [(True, True, False, False, True), (True, False, True, True, True),
                                 (False, False, False, False, True)], ids=R.option_id)
def test_sgd_step_float(C, opt):
    sizes = _list(73)
    h = R.options(R.FLOAT, *opt)
    st = State(sizes)
    p, g, b = R.normal(sizes, 14, scale=1.0)
    st.load(p, g, b)
    first = FIRST73 if opt[1] else ()
    _run(st, lambda: _sgd(C, st, h, first), False, "sgd_step", first=first, amp=False, **h)
    # the unscale inside the rule, by a scale that is no power of two
    gs = torch.tensor([1000.0], device=DEV)
    st.load(p, [x * 1000.0 for x in g], b)
    _run(st, lambda: _sgd(C, st, h, first, grad_scale=gs), False, "sgd_step", first=first, amp=False,
         grad_scale=1000.0, **h)


# =============================================================================== c
@pytest.mark.parametrize("row", R.SCALE_TABLE, ids=lambda r: f"s{r[0]:g}-t{r[1]}-{'inf' if r[2] else 'ok'}-i{r[5]}")
def test_update_scale_table(C, row):
    scale, tracker, found, growth, backoff, interval = row
    s = torch.tensor([scale], device=DEV)
    t = torch.tensor([tracker], dtype=torch.int32, device=DEV)
    f = torch.tensor([float(found)], device=DEV)
    C.optim.update_scale(s, t, f, growth, backoff, interval)
    want = R.update_scale(scale, tracker, found, growth, backoff, interval)
    assert (float(s), int(t)) == want
    assert float(f) == 0.0  # re-armed for the next step


# =============================================================================== d
def fused_sizes(variant):
    """36 tensors: sizes 1..5 and one large tensor (index 17) that sets the variant; the last
    tensor ends on a partial granule."""
    big = {"solo": 601, "u1": 100_003, "u2": 200_001, "u4": 400_002}[variant]
    small = [1 + i % 5 for i in range(35)]
    sizes = small[:17] + [big] + small[17:]
    sizes[-1] = 7
    return sizes


def fused_shape(sizes):
    """(granules per lane, workgroups) the host picks for these sizes (optim.hip amp_sgd_fused)."""
    gran = sum((n + 3) // 4 for n in sizes)
    U = 1 if gran <= 128 * 256 else 2 if gran <= 128 * 512 else 4
    return U, -(-gran // (256 * U))


def _locate(sizes, gi):
    """(tensor, first element) of granule ``gi`` of the flat granule space."""
    o = 0
    for t, n in enumerate(sizes):
        k = (n + 3) // 4
        if gi < o + k:
            return t, (gi - o) * 4
        o += k
    raise AssertionError("granule past the end")


def fused_places(sizes):
    """Workgroup 0; the last partial granule of the last tensor; granule U - 1 of a lane."""
    U, grid = fused_shape(sizes)
    gi = min(1, grid - 1) * 256 * U + 256 * (U - 1) + 37
    assert gi % (256 * U) >= 256 * (U - 1)
    t, e = _locate(sizes, gi)
    assert t == 17 and sizes[-1] % 4 != 0
    return [(0, 0), (35, sizes[-1] - 1), (t, e + 1)]


def _fused(C, st, h, first=(), amp=True, gbi=(2.0, 0.5, 2), prechk=None, params=None):
    n = len(st.sizes) if params is None else len(params)
    C.optim.amp_sgd_fused(st.P.views if params is None else params, st.G.views if params is None else params,
                          st.B.views if params is None else params, h["lr"], h["momentum"], h["dampening"],
                          h["weight_decay"], h["nesterov"], h["maximize"], list(first) or [0] * n,
                          st.scale if amp else None, st.tracker if amp else None, st.found if amp else None,
                          gbi[0], gbi[1], gbi[2], st.sync, None, prechk=prechk)


VARIANTS = ["solo", "u1", "u2", "u4"]
FIRST36 = [int(i in (0, 17, 35)) for i in range(36)]
FUSED_OPTS = [(True, True, False, False, True), (True, False, True, True, True), (False, False, False, False, False)]


@pytest.mark.parametrize("opt", FUSED_OPTS, ids=R.option_id)
@pytest.mark.parametrize("variant", VARIANTS)
def test_fused_exact_two_steps_second_replayed(C, variant, opt):
    sizes = fused_sizes(variant)
    U, grid = fused_shape(sizes)
    assert (variant == "solo") == (grid == 1) and (sum(sizes) <= 1024 or grid > 1)
    assert U == {"solo": 1, "u1": 1, "u2": 2, "u4": 4}[variant]
    h = R.options(R.DYADIC, *opt)
    st = State(sizes)
    p, g, b = R.dyadic(sizes, 21)
    st.load(p, g, b, scale=1024.0)
    adv = int(grid > 1)
    _run(st, lambda: _fused(C, st, h, FIRST36), True, "amp_sgd_fused", first=FIRST36, sync_step=adv, **h)
    assert float(st.scale) == 1024.0 and int(st.tracker) == 1
    graph = _graph(lambda: _fused(C, st, h))
    st.G.load(R.dyadic_grads(sizes, 22))
    _run(st, graph.replay, True, "amp_sgd_fused", sync_step=adv, **h)
    assert float(st.scale) == 2048.0 and int(st.tracker) == 0  # grown at the interval


@pytest.mark.parametrize("variant", VARIANTS)
def test_fused_float(C, variant):
    sizes = fused_sizes(variant)
    h = R.options(R.FLOAT, True, True, False, False, True)
    st = State(sizes)
    p, g, b = R.normal(sizes, 23, scale=1000.0)
    st.load(p, g, b, scale=1000.0)
    _run(st, lambda: _fused(C, st, h, FIRST36), False, "amp_sgd_fused", first=FIRST36,
         sync_step=int(fused_shape(sizes)[1] > 1), **h)


@pytest.mark.parametrize("variant", VARIANTS)
def test_fused_nonfinite_skips_everything(C, variant):
    """One non-finite gradient, wherever it sits: all 36 params and buffers bitwise unchanged,
    grads unscaled, scale backed off, tracker 0, found_inf 0, one barrier generation."""
    sizes = fused_sizes(variant)
    h = R.options(R.FLOAT, True, True, False, False, True)
    st = State(sizes)
    p, g, b = R.normal(sizes, 24, scale=1000.0)
    adv = int(fused_shape(sizes)[1] > 1)
    for t, i in fused_places(sizes):
        for val in (NAN, INF, -INF):
            st.load(p, _inject(g, t, i, val), b, scale=1000.0, tracker=1)
            ref = _run(st, lambda: _fused(C, st, h, FIRST36), False, "amp_sgd_fused", first=FIRST36, sync_step=adv,
                       **h)
            assert ref["found"] and float(st.scale) == 500.0 and int(st.tracker) == 0


@pytest.mark.parametrize("variant", ["solo", "u2"])
def test_fused_plain_mode(C, variant):
    """No scale: the gradients are untouched, a NaN is applied as torch.optim.SGD applies it,
    and the barrier word does not move."""
    sizes = fused_sizes(variant)
    h = R.options(R.DYADIC, True, True, False, False, True)
    st = State(sizes)
    p, g, b = R.dyadic(sizes, 25, scale=1.0)
    st.load(p, g, b)
    _run(st, lambda: _fused(C, st, h, FIRST36, amp=False), True, "amp_sgd_fused", first=FIRST36, amp=False,
         sync_step=0, **h)
    t, i = fused_places(sizes)[2]
    st.load(p, _inject(g, t, i, NAN), b)
    _run(st, lambda: _fused(C, st, h, FIRST36, amp=False), True, "amp_sgd_fused", first=FIRST36, amp=False,
         sync_step=0, **h)
    assert bool(st.P.read()[t][i].isnan())


def test_fused_rejects_37_tensors(C):
    st = State([4])
    xs = [torch.zeros(4, device=DEV) for _ in range(37)]
    with pytest.raises(RuntimeError, match="<= 36 tensors"):
        _fused(C, st, R.options(R.DYADIC, False, False, False, False, False), params=xs)


def _words(vals, scale):
    w = torch.tensor(list(vals) + [0], dtype=torch.int32)
    w[-1] = int(np.float32(scale).view(np.int32))
    return w.to(DEV)


def test_fused_prechecked_mode(C):
    """prechk = the producers' int32 check words + the bit pattern of the scale they used."""
    sizes = fused_sizes("u1")
    assert fused_shape(sizes)[1] > 1
    h = R.options(R.DYADIC, True, True, False, False, True)
    st = State(sizes)
    p, g, b = R.dyadic(sizes, 26)

    def run(words, exact=True, grads=g, sync_step=0, **kw):
        st.load(p, grads, b, scale=1024.0, tracker=1)
        return _run(st, lambda: _fused(C, st, h, FIRST36, prechk=words), exact, "amp_sgd_fused (pre-checked)",
                    first=FIRST36, sync_step=sync_step, **h, **kw)

    # all words zero: the update is applied without the barrier
    ref = run(_words([0] * 5, 1024.0))
    assert not ref["found"] and float(st.scale) == 2048.0
    # the last word differs from scale[0]: it unscales, the update acts on scale[0]
    ref = run(_words([0] * 5, 256.0), grads=[x / 4 for x in g], unscale_by=256.0)
    assert not ref["found"] and float(st.scale) == 2048.0
    # one word set, finite gradients: skipped, backed off
    for k in (0, 4, 299):
        w = [0] * 300
        w[k] = 1
        ref = run(_words(w, 1024.0), found_inf=1.0)
        assert ref["found"] and float(st.scale) == 512.0 and int(st.tracker) == 0
    # last word < 1: the words are ignored, the kernel's own check decides, the barrier runs
    ref = run(_words([1, 0, 1], 0.5), sync_step=1)
    assert not ref["found"] and float(st.scale) == 2048.0
    t, i = fused_places(sizes)[1]
    ref = run(_words([0, 0, 0], 0.5), grads=_inject(g, t, i, INF), sync_step=1)
    assert ref["found"] and float(st.scale) == 512.0


SLAB_SIZES = [7, 33, 1023, 1025, 36]


@pytest.mark.parametrize("amp", [True, False], ids=["amp", "plain"])
@pytest.mark.parametrize("rows", [5, 37])
def test_fused_slab_source(C, rows, amp):
    """The slab source: the last tensor's gradient is not in memory but the column sums of a
    [rows][36] slab, summed by three extra workgroups (16 columns each, the last with 4; 5 rows
    leave most of the 16 row groups empty, 37 give some three rows).  Dyadic rows whose sums are
    the dyadic gradient, so any association is exact: the step is bitwise the step fed the
    pre-summed gradient, which is bitwise _sgd_ref's.  The region itself is written, never read."""
    sizes = SLAB_SIZES
    h = R.options(R.DYADIC, True, True, False, False, True)
    first = [1, 0, 1, 0, 0]
    sc = 1024.0 if amp else 1.0
    st = State(sizes)
    p, g, b = R.dyadic(sizes, 27 + rows, scale=sc)

    def launch(**kw):
        C.optim.amp_sgd_fused(st.P.views, st.G.views, st.B.views, h["lr"], h["momentum"], h["dampening"],
                              h["weight_decay"], h["nesterov"], h["maximize"], first, st.scale if amp else None,
                              st.tracker if amp else None, st.found if amp else None, 2.0, 0.5, 2, st.sync, None, **kw)

    st.load(p, g, b, scale=sc)
    _run(st, launch, True, "amp_sgd_fused (slab)", first=first, amp=amp, sync_step=int(amp), **h)
    want, want_s = st.read(), (float(st.scale), int(st.tracker))
    slab = R.slab_rows(g[4], rows, 28 + rows, sc).to(DEV)
    st.load(p, g[:4] + [torch.full((36,), 12345.0)], b, scale=sc)
    s0 = int(st.sync[0])
    launch(slab=slab, slab_out=st.G.views[4])
    torch.cuda.synchronize()
    st.check_pads()
    got = st.read()
    for key in ("p", "g", "b"):
        for i, (x, w) in enumerate(zip(got[key], want[key])):
            same_bits(x, w, f"slab rows={rows}: {NAMES[key]}[{i}] vs the pre-summed step")
    assert (float(st.scale), int(st.tracker)) == want_s
    assert int(st.sync[0]) == s0 + int(amp) and int(st.sync[3]) == 0  # 3 + 3 workgroups: one barrier generation


# =============================================================================== e
def large_sizes():
    """512 tensors, about 2.2M floats: sizes 1..7 with four large ones, so tensor boundaries fall
    inside a lane's unrolled stride and every workgroup walks more than one."""
    sizes = [1 + i % 7 for i in range(512)]
    for i, n in ((50, 700_001), (200, 500_002), (350, 600_003), (500, 400_000)):
        sizes[i] = n
    sizes[511] = 6
    return sizes


def _large(C, st, table, h, gbi=(2.0, 0.5, 2)):
    C.optim.amp_sgd_large(table, h["lr"], h["momentum"], h["dampening"], h["weight_decay"], h["nesterov"],
                          h["maximize"], st.scale, st.tracker, st.found, gbi[0], gbi[1], gbi[2], st.sync)


def _large_case(C, sizes, opt, places):
    """Exact for two steps (eager, then graph-replayed, one table), the float leg, and one
    non-finite value at each of ``places`` -- the assertions of the small kernel."""
    n = len(sizes)
    first = [int(i % 3 == 0) for i in range(n)] if opt[1] else []
    h = R.options(R.DYADIC, *opt)
    st = State(sizes)
    table = C.optim.amp_sgd_table(st.P.views, st.G.views, st.B.views, first)
    p, g, b = R.dyadic(sizes, 31)
    st.load(p, g, b, scale=1024.0)
    launch = lambda: _large(C, st, table, h)
    _run(st, launch, True, "amp_sgd_large", first=first, **h)
    s1 = int(st.sync[0])
    graph = _graph(launch)
    st.G.load(R.dyadic_grads(sizes, 32))
    _run(st, graph.replay, True, "amp_sgd_large", first=first, sync_step=1, **h)
    assert float(st.scale) == 2048.0 and int(st.tracker) == 0 and s1 in (0, 1)
    hf = R.options(R.FLOAT, *opt)
    p, g, b = R.normal(sizes, 33, scale=1000.0)
    st.load(p, g, b, scale=1000.0)
    _run(st, lambda: _large(C, st, table, hf), False, "amp_sgd_large", first=first, sync_step=1, **hf)
    for t, i in places:
        for val in (NAN, INF, -INF):
            st.load(p, _inject(g, t, i, val), b, scale=1000.0, tracker=1)
            ref = _run(st, lambda: _large(C, st, table, hf), False, "amp_sgd_large", first=first, sync_step=1, **hf)
            assert ref["found"] and float(st.scale) == 500.0 and int(st.tracker) == 0


def test_large_one_tensor_of_one_element(C):
    _large_case(C, [1], (True, True, False, False, True), [(0, 0)])


def test_large_37_tensors(C):
    """The table is written by two upload launches."""
    sizes = _list(37)
    _large_case(C, sizes, (True, True, False, False, True), [(0, 0), (36, sizes[36] - 1), (35, 0)])


@pytest.mark.parametrize("opt", [(True, True, False, False, True), (True, False, True, True, True)], ids=R.option_id)
def test_large_512_tensors(C, opt):
    sizes = large_sizes()
    assert len(sizes) == C.optim.LARGE_MAXT and sizes[254] == 3 and 2_150_000 < sum(sizes) < 2_250_000
    _large_case(C, sizes, opt, [(0, 0), (511, sizes[511] - 1), (254, 1)])


def test_large_rejects_513_tensors(C):
    xs = [torch.zeros(4, device=DEV) for _ in range(513)]
    with pytest.raises(RuntimeError, match="1..512 tensors"):
        C.optim.amp_sgd_table(xs, xs, xs, [])


# =============================================================================== f
@pytest.mark.parametrize("s", [0.5, 1.0 / 3.0], ids=["half", "third"])
def test_flat_copy_both_directions(C, s):
    """40 tensors (two launches) at offsets with gaps: flat[off + i] = x[i] * s and back, each
    the correctly rounded product with the float32 of s; gaps and padding untouched."""
    sizes = _list(40)
    offs, o = [], 3
    for n in sizes:
        offs.append(o)
        o += n + 1 + n % 3
    src = Arena(sizes)
    xs = R.normal(sizes, 41, scale=1.0)[0]
    src.load(xs)
    flat = torch.full((o + 5,), SENT, dtype=torch.int32, device=DEV).view(torch.float32)
    C.optim.flat_copy(src.views, offs, flat, s, 0)
    torch.cuda.synchronize()
    sf = R.f32(s)
    want = torch.full((o + 5,), SENT, dtype=torch.int32).view(torch.float32)
    for a, x in zip(offs, xs):
        want[a:a + x.numel()] = (x.double() * sf).float()
    same_bits(flat.cpu(), want, "flat")
    src.check("src")
    for x, y in zip(src.read(), xs):
        same_bits(x, y, "src")
    dst = Arena(sizes)
    C.optim.flat_copy(dst.views, offs, flat, s, 1)
    torch.cuda.synchronize()
    dst.check("dst")
    for i, (y, a) in enumerate(zip(dst.read(), offs)):
        same(y, (want[a:a + y.numel()].double() * sf).float().double(), f"dst[{i}]")
    same_bits(flat.cpu(), want, "flat")


# ===============================================================================
def test_print_error_bound_ratios():
    """Not a check of its own: the largest error / bound ratio of each float section above."""
    for section, (worst, name) in sorted(RATIOS.items()):
        print(f"{section}: largest error / bound = {worst:.3g} ({name})")
        assert worst <= 1.0
