"""csrc/kernels/bn_nhwc.hip against tests/_bn_ref.py: exact on integer inputs, per element
against float64 on floats.

  a. statistics geometry: integer inputs, every sum an exact fp32 integer (or multiple of
     1/4) whatever the summation order; one- and two-level ticket trees, both hand-offs;
  b. elementwise kernels per element, |got - ref| <= 16 u A + q |ref| (see _bn_ref);
  c. conditioning of the sums around the shift (fresh and warmed-up running mean);
  d. max-pool 3x3/2 (ties, -inf windows, NaN) and global average pool against ATen on the
     CPU, their grid-stride loops and the channel-multiple checks;
  e. graph capture and replay of one two-level case.

The kernels are called through C.bn_nhwc where that pins the path.  Activations are rows
[M][C].  The largest error / bound ratio of sections b, c, d is kept in RATIOS and printed
by the last test (pytest -s).
"""
import contextlib
import itertools

import pytest
import torch
import torch.nn.functional as F

from . import _bn_ref as R
from .test_igemm_bits_gpu import _bn_row_blocks

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
F32, BF, HF = torch.float32, torch.bfloat16, torch.float16
DTYPES = list(R.Q)
G1, MAXGR, U, THR = 128, 1024, 4, 256  # csrc/kernels/bn_nhwc.hip
NAN = float("nan")
RATIOS = {}


def _id(v):
    return str(v).replace("torch.", "")


def _geom(M, ch, target, dtype, cc=64):
    """(row blocks, channel chunks, rows per pass) of chunk_grid (cc 64: the statistics
    kernels; 256: the elementwise ones)."""
    return R.geom(M, ch, target, dtype, cc)[:3]


_WS = {}


def _ws(B):
    if "w" not in _WS:
        _WS["w"] = (torch.zeros(int(B.MAX_PARTIAL_ROWS) * 2 * 2048, device=DEV),
                    torch.zeros(int(B.MAX_TICKETS), dtype=torch.int32, device=DEV))
    return _WS["w"]


@contextlib.contextmanager
def _targets(B, stats, handoff=1, apply=512, elemt=1024):
    B.set_grid_targets(stats, apply, elemt)
    B.set_handoff(handoff)
    try:
        yield
    finally:
        B.set_grid_targets(0, 512, 1024)
        B.set_handoff(1)


def _act(t, dtype):
    return t.to(dtype).to(DEV)


def _f(t):
    return t.float().to(DEV)


def _cpu(t):
    return t.detach().double().cpu()


def _within(got, ref, bnd, name, section, keep=None):
    """|got - ref| <= bnd on every (kept) element; NaN fails."""
    err = (_cpu(got).reshape(ref.shape) - ref).abs()
    bnd = bnd.expand_as(err)
    if keep is not None:
        err, bnd = err[keep], bnd[keep]
    if err.numel() == 0:
        return
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd.clamp(min=1e-300))
    worst = float(ratio.max()) if not ratio.isnan().any() else float("inf")
    bad = ~(err <= bnd)
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.numel()} outside the bound, error / bound <= {worst:.3g}"
    if worst >= RATIOS.get(section, (0.0, ""))[0]:
        RATIOS[section] = (worst, name)


def _same(got, want, name):
    got = got.detach().cpu()
    want = want.to(got.dtype)
    assert torch.equal(got.reshape(want.shape), want), \
        f"{name}: {int((got.reshape(want.shape) != want).sum())} of {want.numel()} differ"


# =============================================================================== a
STATS_CH = (8, 24, 64, 40, 72, 200, 320, 2048)
_INT = {}
_INT_REF = {}


def _int_base(M, ch):
    """Integer inputs of the statistics kernels (the same integers for every dtype)."""
    k = (M, ch)
    if k not in _INT:
        s = 31 * ch
        t = dict(x=R.int_rows(M, ch, s), dy=R.int_rows(M, ch, s + 1), y=R.int_rows(M, ch, s + 2).clamp(min=0),
                 shift=R.int_shift(ch, s + 3), save=R.int_save(ch, s + 4))
        t["gamma"], t["beta"] = R.int_affine(ch, s + 5)
        t["pre"] = R.bn_y(t["x"], t["save"][:ch], t["save"][ch:], t["gamma"], t["beta"])[1]
        _INT[k] = t
    return _INT[k]


def _int_ref(base, ch, M):
    """fp32 images of the int64 sums over the first M rows of _int_base(base, ch)."""
    k = (base, ch, M)
    if k not in _INT_REF:
        t = _int_base(base, ch)
        s1, s2 = R.int_fwd_sums(t["x"][:M], t["shift"])
        ref = {"fwd": (s1.float(), s2.float())}
        for act in (0, 1, 2):
            S1, S2x4 = R.int_bwd_sums(t["dy"][:M], t["x"][:M], t["save"],
                                      R.relu_mask(act, y=t["y"][:M], pre=t["pre"][:M]))
            ref[f"bwd{act}"] = (S1.float(), (S2x4.double() / 4).float())
        _INT_REF[k] = ref
    return _INT_REF[k]


def _upload(t, dtype):
    return {k: (_act(v, dtype) if k in ("x", "dy", "y") else _f(v)) for k, v in t.items() if k != "pre"}


def _stats_exact(B, which, t, dv, ref, M, ch, tag):
    """Two launches on the same tickets; every output equal to the integer reference."""
    part, tk = _ws(B)
    x = dv["x"][:M]
    e1, e2 = ref[which]
    if which == "fwd":
        st = torch.full((3 * ch + 4,), NAN, device=DEV)
        nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
        for _ in range(2):
            B.fwd_stats(x, ch, dv["shift"], part, tk, st, nbt)
        _same(st[:ch], e1, f"{tag} s1")
        _same(st[ch:2 * ch], e2, f"{tag} s2")
        assert st[2 * ch].item() == M, f"{tag} count"
        _same(st[2 * ch + 4:3 * ch + 4], t["shift"], f"{tag} shift copy")
        assert nbt.item() == 2, f"{tag} num_batches_tracked"
    else:
        act = int(which[-1])
        out, dgamma, dbeta = (torch.full((n,), NAN, device=DEV) for n in (2 * ch, ch, ch))
        for _ in range(2):
            B.bwd_stats(dv["dy"][:M], dv["y"][:M] if act == 1 else None, x, ch, act, dv["save"], dv["gamma"],
                        dv["beta"], part, tk, out, dgamma, dbeta)
        _same(out[:ch], e1, f"{tag} S1")
        _same(out[ch:], e2, f"{tag} S2")
        _same(dbeta, e1, f"{tag} dbeta")
        _same(dgamma, e2, f"{tag} dgamma")
    assert int(tk.abs().sum()) == 0, f"{tag}: tickets not re-armed"


WHICH = ("fwd", "bwd0", "bwd1", "bwd2")


@pytest.mark.parametrize("dtype,ch", [(dt, c) for dt in DTYPES for c in ((4,) if dt == F32 else ()) + STATS_CH],
                         ids=_id)
def test_stats_exact_one_level(C, dtype, ch):
    """Channel geometries (one chunk of width C; 8-channel chunks at C = 72 / 200; 64-channel
    chunks at 320 / 2048; C = 40 is one chunk of 5 vectors in chunk_width) x row counts
    around one pass of the block (RP * U rows) x 1 row block / as many as the rows give."""
    B = C.bn_nhwc
    base = 1025
    assert R.STATS_ONE_BLOCK[1] in STATS_CH and R.STATS_ONE_BLOCK[0] in DTYPES  # M = 189, target 1 below
    _, _, rp = _geom(base, ch, 512, dtype)
    t = _int_base(base, ch)
    dv = _upload(t, dtype)
    for M in (2, rp * U - 1, rp * U, rp * U + 1, 1025, 189):
        ref = _int_ref(base, ch, M)
        for target in (1, 512):
            gr, gc, _ = _geom(M, ch, target, dtype)
            assert gr == _bn_row_blocks(M, ch, target, R.VEC[dtype]) and gr <= G1  # one level
            assert target != 1 or gr == 1
            with _targets(B, target):
                for which in WHICH:
                    _stats_exact(B, which, t, dv, ref, M, ch, f"{which} M={M} blocks={gr}x{gc}")


@pytest.mark.parametrize("handoff", [1, 0])
@pytest.mark.parametrize("blocks,levels", [(G1, 1), (G1 + 1, 2), (147, 2), (300, 2)])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_stats_exact_tree(C, dtype, blocks, levels, handoff):
    """C = 64, M = blocks x RP x U rows: exactly G1 row blocks (one level), G1 + 1 (two levels,
    last group of one), 147 and 300, write-through and fenced hand-off."""
    B = C.bn_nhwc
    ch = 64
    _, _, rp = _geom(1 << 20, ch, 512, dtype)
    base, M = 300 * rp * U, blocks * rp * U
    gr, gc, _ = _geom(M, ch, blocks, dtype)
    assert gr == blocks == _bn_row_blocks(M, ch, blocks, R.VEC[dtype]) and gc == 1
    assert (1 if gr <= G1 else 2) == levels  # 300 blocks: three groups of G1, still two levels
    t = _int_base(base, ch)
    dv = _upload(t, dtype)
    ref = _int_ref(base, ch, M)
    with _targets(B, blocks, handoff):
        for which in WHICH:
            _stats_exact(B, which, t, dv, ref, M, ch, f"{which} blocks={gr}")


# =============================================================================== b
ELEM = pytest.mark.parametrize("dtype,ch", R.elem_cases(), ids=_id)
KIND = pytest.mark.parametrize("kind", ["int", "float"])
u16 = 16 * R.U32


def _elem(kind, M, ch, dtype, extra=0):
    t = R.elem_inputs(kind, M, ch, dtype, R.elem_seed(dtype, ch, M) + extra)
    dv = {k: (_act(v, dtype) if k in ("x", "res", "dy", "y") else _f(v)) for k, v in t.items()}
    return t, dv


def _fwd_stats(B, x, ch, shift):
    part, tk = _ws(B)
    st = torch.zeros(3 * ch + 4, device=DEV)
    B.fwd_stats(x, ch, shift, part, tk, st, None)
    return st


def _train_side(save, rm, rv, st, rm0, rv0, momentum, nbt, ch, tag, sec="b"):
    """Saved mean / invstd and running statistics per channel, from the statistics tensor the
    kernel was given.  Bounds: mean 16 u (|shift| + |s1/n|); variance 16 u (s2/n + (s1/n)^2)
    (its two cancelling terms); invstd relative 16 u plus half the variance bound over
    var + eps; the running statistics 16 u of their two terms plus the above scaled.
    Returns (mean, invstd) in float64."""
    st = _cpu(st)
    s1, s2, n, sh = st[:ch], st[ch:2 * ch], float(st[2 * ch]), st[2 * ch + 4:3 * ch + 4]
    mean, var, invstd = R.moments_from_sums(s1, s2, n, sh)
    m1 = s1 / n
    e_mean, e_var = u16 * (sh.abs() + m1.abs()), u16 * (s2 / n + m1 * m1)
    _within(save[:ch], mean, e_mean, f"{tag} saved mean", sec)
    _within(save[ch:], invstd, invstd * (u16 + 0.5 * e_var / (var + R.EPS)), f"{tag} saved invstd", sec)
    mom = momentum if momentum is not None else 1.0 / nbt
    k = n / max(n - 1.0, 1.0)
    erm, erv = R.running_update(rm0, rv0, mean, var, n, momentum, nbt)
    _within(rm, erm, u16 * (((1 - mom) * rm0).abs() + (mom * mean).abs()) + mom * e_mean, f"{tag} running_mean", sec)
    _within(rv, erv, u16 * (((1 - mom) * rv0).abs() + mom * k * var) + mom * k * e_var, f"{tag} running_var", sec)
    return mean, invstd


MODES = (("train", 0.1), ("train", None), ("eval", 0.1))
NBT = 3  # num_batches_tracked handed to the apply kernels (cumulative average: 1/3)


def _apply_case(B, kind, M, ch, dtype, sec="b"):
    t, dv = _elem(kind, M, ch, dtype)
    st = _fwd_stats(B, dv["x"], ch, dv["rm0"])
    for (mode, momentum), res, relu in itertools.product(MODES, (False, True), (False, True)):
        tag = f"apply M={M} {mode} mom={momentum} res={res} relu={relu}"
        train = mode == "train"
        rm, rv = dv["rm0"].clone(), dv["rv0"].clone()
        nbt = torch.full((1,), NBT, dtype=torch.int64, device=DEV)
        save = torch.full((2 * ch,), NAN, device=DEV)
        y = torch.full_like(dv["x"], NAN)
        B.apply(dv["x"], dv["res"] if res else None, y, ch, st if train else torch.zeros_like(st), dv["gamma"],
                dv["beta"], rm, rv, nbt, -1.0 if momentum is None else momentum, R.EPS, train, relu, save)
        assert nbt.item() == NBT
        if train:
            mean, invstd = _train_side(save, rm, rv, st, t["rm0"], t["rv0"], momentum, NBT, ch, tag, sec)
        else:
            mean, invstd = t["rm0"], (t["rv0"] + R.EPS).rsqrt()
            _same(rm, t["rm0"], f"{tag} running_mean"), _same(rv, t["rv0"], f"{tag} running_var")
            assert save.isnan().all(), f"{tag}: save written in eval"
        ref, _, A = R.bn_y(t["x"], mean, invstd, t["gamma"], t["beta"], t["res"] if res else None, relu)
        _within(y, ref, R.bound(A, ref, dtype), f"{tag} y", sec)


@KIND
@ELEM
def test_apply_per_element(C, dtype, ch, kind):
    for M in R.ELEM_ROWS:
        _apply_case(C.bn_nhwc, kind, M, ch, dtype)


def _apply_resbn_case(B, kind, M, ch, dtype, sec="b"):
    t, dv = _elem(kind, M, ch, dtype)
    s, ds = _elem(kind, M, ch, dtype, extra=500)  # the downsample branch
    st, rst = _fwd_stats(B, dv["x"], ch, dv["rm0"]), _fwd_stats(B, ds["x"], ch, ds["rm0"])
    for train in (True, False):
        tag = f"apply_resbn M={M} train={train}"
        rm, rv, rrm, rrv = dv["rm0"].clone(), dv["rv0"].clone(), ds["rm0"].clone(), ds["rv0"].clone()
        nbt = torch.full((1,), NBT, dtype=torch.int64, device=DEV)
        save, rsave = torch.full((2 * ch,), NAN, device=DEV), torch.full((2 * ch,), NAN, device=DEV)
        y = torch.full_like(dv["x"], NAN)
        B.apply_resbn(dv["x"], ds["x"], y, ch, st, dv["gamma"], dv["beta"], rm, rv, nbt, 0.1, R.EPS, save,
                      rst, ds["gamma"], ds["beta"], rrm, rrv, nbt, -1.0, R.EPS, rsave, train)
        if train:
            mean, invstd = _train_side(save, rm, rv, st, t["rm0"], t["rv0"], 0.1, NBT, ch, tag, sec)
            rmean, rinvstd = _train_side(rsave, rrm, rrv, rst, s["rm0"], s["rv0"], None, NBT, ch, tag + " (r)", sec)
        else:
            mean, invstd = t["rm0"], (t["rv0"] + R.EPS).rsqrt()
            rmean, rinvstd = s["rm0"], (s["rv0"] + R.EPS).rsqrt()
            for got, want in ((rm, t["rm0"]), (rv, t["rv0"]), (rrm, s["rm0"]), (rrv, s["rv0"])):
                _same(got, want, f"{tag} running statistics")
            assert save.isnan().all() and rsave.isnan().all()
        ref, _, A = R.tail_fwd(t["x"], s["x"], mean, invstd, t["gamma"], t["beta"], rmean, rinvstd, s["gamma"],
                               s["beta"])
        _within(y, ref, R.bound(A, ref, dtype), f"{tag} y", sec)


@KIND
@ELEM
def test_apply_resbn_per_element(C, dtype, ch, kind):
    """relu(bn(x) + bn_r(r)) in one pass: y and both BNs' saves / running statistics."""
    for M in R.ELEM_ROWS:
        _apply_resbn_case(C.bn_nhwc, kind, M, ch, dtype)


def _bwd_sums(B, dv, ch, act):
    part, tk = _ws(B)
    out, dgamma, dbeta = (torch.zeros(n, device=DEV) for n in (2 * ch, ch, ch))
    B.bwd_stats(dv["dy"], dv["y"] if act == 1 else None, dv["x"], ch, act, dv["save"], dv["gamma"], dv["beta"], part,
                tk, out, dgamma, dbeta)
    return out


def _fstats(M, ch):
    fs = torch.zeros(3 * ch + 4, device=DEV)
    fs[2 * ch] = M
    return fs


def _bwd_elemt_case(B, kind, M, ch, dtype, sec="b"):
    t, dv = _elem(kind, M, ch, dtype)
    mean, invstd = t["save"][:ch], t["save"][ch:]
    _, pre, Apre = R.bn_y(t["x"], mean, invstd, t["gamma"], t["beta"])
    fs = _fstats(M, ch)
    for act in (0, 1, 2):
        sums = _bwd_sums(B, dv, ch, act)
        s64 = _cpu(sums)
        mask = R.relu_mask(act, y=t["y"], pre=pre)
        dz = t["dy"] if mask is None else t["dy"] * mask
        ref, A = R.bn_dx(dz, t["x"], mean, invstd, t["gamma"], s64[:ch], s64[ch:], float(M))
        keep = None
        if act == 2 and kind == "float":  # the only skip: the recomputed mask next to its threshold
            skip = R.near_zero(pre, Apre)
            assert int(skip.sum()) <= R.skip_allowance(skip.numel())
            keep = ~skip
        for with_dres in (False, True):
            tag = f"bwd_elemt M={M} act={act} dres={with_dres}"
            dx = torch.full_like(dv["x"], NAN)
            dres = torch.full_like(dv["x"], NAN) if with_dres else None
            B.bwd_elemt(dv["dy"], dv["y"] if act == 1 else None, dv["x"], ch, act, dv["save"], sums, fs,
                        dv["gamma"], dv["beta"], dx, dres)
            _within(dx, ref, R.bound(A, ref, dtype), f"{tag} dx", sec, keep)
            if with_dres:
                _within(dres, dz, torch.zeros_like(dz), f"{tag} dres", sec, keep)


@KIND
@ELEM
def test_bwd_elemt_per_element(C, dtype, ch, kind):
    """dx per element and dres = dz exactly, act 0 / 1 / 2, with and without dres.  The
    reference starts from the save / sums tensors the kernel was given."""
    for M in R.ELEM_ROWS:
        _bwd_elemt_case(C.bn_nhwc, kind, M, ch, dtype)


def _rbn_case(B, kind, M, ch, dtype, sec="b"):
    t, dv = _elem(kind, M, ch, dtype)
    s, ds = _elem(kind, M, ch, dtype, extra=500)
    part, tk = _ws(B)
    sums, fs = _bwd_sums(B, dv, ch, 1), _fstats(M, ch)
    dx0, dz0 = torch.full_like(dv["x"], NAN), torch.full_like(dv["x"], NAN)
    B.bwd_elemt(dv["dy"], dv["y"], dv["x"], ch, 1, dv["save"], sums, fs, dv["gamma"], dv["beta"], dx0, dz0)
    dx, dz = torch.full_like(dv["x"], NAN), torch.full_like(dv["x"], NAN)
    rout, rdgamma, rdbeta = (torch.full((n,), NAN, device=DEV) for n in (2 * ch, ch, ch))
    for _ in range(2):
        B.bwd_elemt_rbn(dv["dy"], dv["y"], dv["x"], ch, dv["save"], sums, fs, dv["gamma"], dv["beta"], dx, dz, ds["x"],
                        ds["save"], part, tk, rout, rdgamma, rdbeta)
    tag = f"bwd_elemt_rbn M={M}"
    assert torch.equal(dx, dx0) and torch.equal(dz, dz0), f"{tag}: dx / dres differ from bwd_elemt"
    assert int(tk.abs().sum()) == 0, f"{tag}: tickets not re-armed"
    mask = R.relu_mask(1, y=t["y"])
    if kind == "int":
        S1, S2x4 = R.int_bwd_sums(t["dy"], s["x"], s["save"], mask)
        e1, e2 = S1.float(), (S2x4.double() / 4).float()
        _same(rout[:ch], e1, f"{tag} rout S1"), _same(rout[ch:], e2, f"{tag} rout S2")
        _same(rdbeta, e1, f"{tag} rdbeta"), _same(rdgamma, e2, f"{tag} rdgamma")
    else:  # the sums of M terms: first-order bound M u sum|term| (any order), far below a wrong row
        b = R.bn_bwd(t["dy"], s["x"], s["save"][:ch], s["save"][ch:], s["gamma"], mask)
        xh = (s["x"] - s["save"][:ch]) * s["save"][ch:]
        _within(rout[:ch], b["S1"], M * R.U32 * b["dz"].abs().sum(0), f"{tag} rout S1", sec)
        _within(rout[ch:], b["S2"], (M + 4) * R.U32 * (b["dz"] * xh).abs().sum(0), f"{tag} rout S2", sec)
        assert torch.equal(rdbeta, rout[:ch]) and torch.equal(rdgamma, rout[ch:])


@KIND
@ELEM
def test_bwd_elemt_rbn(C, dtype, ch, kind):
    """The fused form (DPA_FUSE_RBN_SUMS=1 in ops/bn_nhwc.py), called directly: dx / dres bit for
    bit those of bwd_elemt (act 1, with dres), the downsample BN's sums exact on integers."""
    for M in R.ELEM_ROWS:
        _rbn_case(C.bn_nhwc, kind, M, ch, dtype)


def test_bwd_elemt_rbn_two_level(C):
    """300 row blocks: the statistics tree inside the elementwise kernel takes two levels."""
    M, ch = 38400, 64
    gr, gc, _ = _geom(M, ch, 1024, BF, cc=256)
    assert gr == 300 > G1 and gc == 1
    _rbn_case(C.bn_nhwc, "int", M, ch, BF)


# One row block: under set_grid_targets(1, 1, 1) the M = 189 inputs above are one row block per
# channel chunk, so a lane walks whole passes of U rows and then tail rows (under the default
# targets the row blocks are shorter than one pass for every case but C = 2048, which has no
# tail).  tests/test_bn_nhwc_ref_cpu.py derives the pass / tail counts of these cases.
ONE_BLOCK = pytest.mark.parametrize("dtype,ch", R.ONE_BLOCK_CASES + R.ONE_BLOCK_EXTRA, ids=_id)


@KIND
@ONE_BLOCK
@pytest.mark.parametrize("case", [_apply_case, _apply_resbn_case, _bwd_elemt_case, _rbn_case],
                         ids=["apply", "apply_resbn", "bwd_elemt", "bwd_elemt_rbn"])
def test_one_row_block_per_element(C, case, dtype, ch, kind):
    """The four elementwise checks of this section, same inputs, references, bounds and skip cap."""
    M = R.ELEM_ROWS[0]
    assert R.geom(M, ch, 1, dtype, cc=256)[0] == 1
    with _targets(C.bn_nhwc, 1, apply=1, elemt=1):
        case(C.bn_nhwc, kind, M, ch, dtype, sec="b, one row block")


# =============================================================================== c
@pytest.mark.parametrize("warm", [False, True], ids=["fresh", "warm"])
@pytest.mark.parametrize("ratio", [0, 4, 32])
@pytest.mark.parametrize("M", [189, 38400])
@pytest.mark.parametrize("dtype", [F32, BF], ids=_id)
def test_shifted_sums_conditioning(C, dtype, M, ratio, warm):
    """fwd_stats + apply on channels with mean delta = +-ratio * sigma, once with shift 0 (a
    fresh module) and once with the float64 mean rounded to fp32 (a warmed-up one).  Per
    channel |mean - mean64| <= 2^-16 (|d| + sigma), |var - var64| <= 2^-16 (d^2 + sigma^2),
    d = delta - shift (0 when warm: the header comment's claim).  A fully sequential fp32
    chain over 38,400 rows reaches 6e-6 and 1.7e-5 of those scales on the CPU; the kernel's
    longest chain is a few hundred additions.  The mean is read from the save, the variance
    from running_var with momentum 1 (var * n / (n - 1))."""
    B = C.bn_nhwc
    ch = 64
    g = torch.Generator().manual_seed(977 + ratio)
    sigma = 0.5 + 1.5 * torch.rand(ch, generator=g, dtype=torch.float64)
    delta = ratio * sigma * (torch.randint(0, 2, (ch,), generator=g).double() * 2 - 1)
    x = R.rounded(R.float_rows(M, ch, 13 + M, delta, sigma), dtype)
    mean64, var64, _ = R.batch_moments(x)
    shift = R.rounded(mean64, F32) if warm else torch.zeros(ch, dtype=torch.float64)
    d = torch.zeros_like(delta) if warm else delta
    xd, sh = _act(x, dtype), _f(shift)
    st = _fwd_stats(B, xd, ch, sh)
    rm, rv = sh.clone(), torch.ones(ch, device=DEV)
    nbt = torch.ones(1, dtype=torch.int64, device=DEV)
    save, y = torch.full((2 * ch,), NAN, device=DEV), torch.empty_like(xd)
    one = torch.ones(ch, device=DEV)
    B.apply(xd, None, y, ch, st, one, torch.zeros(ch, device=DEV), rm, rv, nbt, 1.0, R.EPS, True, False, save)
    var = _cpu(rv) * ((M - 1.0) / M)
    tag = f"M={M} delta/sigma={ratio} {'warm' if warm else 'fresh'}"
    _within(save[:ch], mean64, 2.0 ** -16 * (d.abs() + sigma), f"{tag} mean", "c")
    _within(var, var64, 2.0 ** -16 * (d * d + sigma * sigma), f"{tag} var", "c")
    _same(rm, save[:ch].cpu(), f"{tag} running_mean at momentum 1")


# =============================================================================== d
def _pool_ch(dtype):
    return (4, 12) if dtype == F32 else (8, 24)


def _maxpool_ref(x, dy):
    """ATen on the CPU, fp32: output and gradient."""
    x = x.clone().requires_grad_()
    y = F.max_pool2d(x, 3, 2, 1)
    y.backward(dy)
    return y.detach(), x.grad


def _nan_equal(got, want, name):
    got = got.detach().float().cpu()
    assert torch.equal(got.isnan(), want.isnan()), f"{name}: NaN positions"
    ok = ~want.isnan()
    assert torch.equal(got[ok], want[ok]), f"{name}: {int((got[ok] != want[ok]).sum())} of {want.numel()} differ"


def _maxpool_check(B, x, dy, dtype, tag):
    from ddp_practice_amd.ops.bn_nhwc import max_pool_3x3s2

    N, ch, H, W = x.shape
    yr, gr = _maxpool_ref(x, dy)
    xd = x.to(dtype).to(DEV).contiguous(memory_format=CL).requires_grad_()
    y = max_pool_3x3s2(xd)
    y.backward(dy.to(dtype).to(DEV).contiguous(memory_format=CL))
    assert y.shape == yr.shape and y.is_contiguous(memory_format=CL)
    _nan_equal(y, yr, f"{tag} y")
    _nan_equal(xd.grad, gr, f"{tag} dx")
    # the tap the forward kernel returns points at a pixel inside the image, and at the maximum
    OH, OW = yr.shape[2:]
    y2 = torch.empty((N, OH, OW, ch), dtype=dtype, device=DEV)
    idx = torch.full((N, OH, OW, ch), 255, dtype=torch.uint8, device=DEV)
    B.maxpool_fwd(xd.detach().permute(0, 2, 3, 1), y2, idx)
    idx = idx.cpu().long()
    assert int(idx.max()) <= 8
    ih = 2 * torch.arange(OH).view(1, OH, 1, 1) - 1 + idx // 3
    iw = 2 * torch.arange(OW).view(1, 1, OW, 1) - 1 + idx % 3
    assert bool(((ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)).all()), f"{tag}: tap outside the image"
    at = x.permute(0, 2, 3, 1).reshape(N, H * W, ch).gather(1, (ih * W + iw).reshape(N, OH * OW, ch))
    _nan_equal(at.reshape(N, OH, OW, ch).permute(0, 3, 1, 2), yr, f"{tag} value at the tap")


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_maxpool_ties_exact(C, dtype):
    """Post-ReLU integers (most windows tie at 0) and an all-equal tensor: y, the gradient
    (first maximum in scan order takes it; overlapping windows add) and the tap index."""
    g = torch.Generator().manual_seed(5)
    for (H, W), ch in itertools.product([(1, 1), (2, 3), (7, 8), (15, 12)], _pool_ch(dtype)):
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        dy = torch.randint(-3, 4, (2, ch, OH, OW), generator=g).float()
        x = torch.randint(-3, 4, (2, ch, H, W), generator=g).clamp(min=0).float()
        _maxpool_check(C.bn_nhwc, x, dy, dtype, f"maxpool relu-ints {H}x{W} C={ch}")
        _maxpool_check(C.bn_nhwc, torch.full((2, ch, H, W), 2.0), dy, dtype, f"maxpool all-equal {H}x{W} C={ch}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_maxpool_inf_windows_and_nan(C, dtype):
    """A border window and an interior window of -inf (the gradient goes where ATen sends
    it: the first in-bounds pixel of the window) and NaNs, which propagate."""
    g = torch.Generator().manual_seed(6)
    H, W = 7, 8
    for ch in _pool_ch(dtype):
        x = torch.randint(-3, 4, (2, ch, H, W), generator=g).float()
        x[:, :, 0:2, 0:2] = -float("inf")  # output (0, 0): taps 0..2, 3, 6 are padding
        x[:, :, 3:6, 3:6] = -float("inf")  # output (2, 2), interior
        x[1, :, 0:2, 5:8] = -float("inf")  # output (0, 3), top border only: first in-bounds tap 3
        x[0, :, 1:4, 0:2] = -float("inf")  # output (1, 0), left border only: first in-bounds tap 1
        x[0, 1, 6, 6] = NAN
        x[1, 0, 0, 7] = NAN
        x[0, ch - 1, 2, 2] = NAN
        dy = torch.randint(-3, 4, (2, ch, 4, 4), generator=g).float()
        dy[dy == 0] = 1  # every window's gradient is visible
        _maxpool_check(C.bn_nhwc, x, dy, dtype, f"maxpool -inf/NaN C={ch}")


def test_maxpool_grid_stride(C):
    """More than 4096 x 256 vectors, forward (33,489 output pixels x 32) and backward."""
    g = torch.Generator().manual_seed(7)
    N, ch, H = 9, 256, 121
    assert N * 61 * 61 * (ch // 8) > 4096 * THR
    x = torch.randint(-3, 4, (N, ch, H, H), generator=g, dtype=torch.float32).clamp_(min=0)
    dy = torch.randint(-3, 4, (N, ch, 61, 61), generator=g, dtype=torch.float32)
    from ddp_practice_amd.ops.bn_nhwc import max_pool_3x3s2

    yr, gr = _maxpool_ref(x, dy)
    xd = x.to(BF).to(DEV).contiguous(memory_format=CL).requires_grad_()
    y = max_pool_3x3s2(xd)
    y.backward(dy.to(BF).to(DEV).contiguous(memory_format=CL))
    _same(y.float(), yr, "maxpool grid-stride y")
    _same(xd.grad.float(), gr, "maxpool grid-stride dx")


def _avgpool_check(x, dy, dtype, tag):
    from ddp_practice_amd.ops.bn_nhwc import global_avg_pool

    N, ch, H, W = x.shape
    xd = x.to(dtype).to(DEV).contiguous(memory_format=CL).requires_grad_()
    y = global_avg_pool(xd)
    y.backward(dy.to(dtype).to(DEV))
    rel = 2 * R.U32 + R.Q[dtype]
    ref = x.double().mean((2, 3))
    _within(y, ref, rel * ref.abs(), f"{tag} y", "d")
    gref = (dy.double() / (H * W)).view(N, ch, 1, 1).expand(N, ch, H, W)
    _within(xd.grad, gref, rel * gref.abs(), f"{tag} dx", "d")


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_avgpool_exact_sums(C, dtype):
    """Integer inputs: the fp32 sum is exact, so y is the rounding of sum / HW (2 u: the
    reciprocal and the product) and dx that of dy / HW, plus the storage rounding."""
    g = torch.Generator().manual_seed(8)
    for (H, W), ch in itertools.product([(1, 1), (7, 7), (5, 10)], _pool_ch(dtype)):
        x = torch.randint(-3, 4, (3, ch, H, W), generator=g).float()
        dy = torch.randint(-3, 4, (3, ch), generator=g).float()
        _avgpool_check(x, dy, dtype, f"avgpool HW={H * W} C={ch}")


def test_avgpool_bwd_grid_stride(C):
    N, ch = 86, 2048
    assert N * 49 * (ch // 8) > 4096 * THR
    g = torch.Generator().manual_seed(9)
    x = torch.randint(-3, 4, (N, ch, 7, 7), generator=g, dtype=torch.float32)
    dy = torch.randint(-3, 4, (N, ch), generator=g, dtype=torch.float32)
    _avgpool_check(x, dy, BF, "avgpool grid-stride")


@pytest.mark.parametrize("dtype,ch", [(BF, 12), (HF, 20), (F32, 6)], ids=_id)
def test_pools_refuse_partial_vectors(C, dtype, ch):
    """A channel count that is no multiple of the 16-byte vector raises; it must not return
    with the last channels dropped."""
    from ddp_practice_amd.ops.bn_nhwc import global_avg_pool, max_pool_3x3s2

    x = torch.ones(2, ch, 4, 4, device=DEV, dtype=dtype).contiguous(memory_format=CL)
    with pytest.raises(RuntimeError):
        global_avg_pool(x)
    with pytest.raises(RuntimeError):
        max_pool_3x3s2(x)
    with pytest.raises(RuntimeError):
        C.bn_nhwc.avgpool_bwd(torch.ones(2, ch, device=DEV, dtype=dtype),
                              torch.empty(2, 4, 4, ch, device=DEV, dtype=dtype), 16)
    torch.cuda.synchronize()


# =============================================================================== e
def test_graph_replay_matches_eager(C):
    """fwd_stats + apply + bwd_stats + bwd_elemt of a two-level case (147 row blocks) captured
    in a graph and replayed twice: every output bit for bit the eager one, tickets at zero."""
    B = C.bn_nhwc
    ch, blocks = 64, 147
    M = blocks * 32 * U
    assert _geom(M, ch, blocks, BF)[0] == blocks > G1
    t = _int_base(300 * 32 * U, ch)
    dv = _upload(t, BF)
    x, dy = dv["x"][:M], dv["dy"][:M]
    part, tk = _ws(B)
    rm0, rv0 = dv["shift"] * 0.5, torch.full((ch,), 1.5, device=DEV)

    def buffers():
        f = lambda n: torch.full((n,), NAN, device=DEV)  # noqa: E731
        return dict(st=f(3 * ch + 4), save=f(2 * ch), out=f(2 * ch), dgamma=f(ch), dbeta=f(ch), rm=rm0.clone(),
                    rv=rv0.clone(), nbt=torch.zeros(1, dtype=torch.int64, device=DEV), y=torch.full_like(x, NAN),
                    dx=torch.full_like(x, NAN))

    def step(b):
        B.fwd_stats(x, ch, dv["shift"], part, tk, b["st"], b["nbt"])
        B.apply(x, None, b["y"], ch, b["st"], dv["gamma"], dv["beta"], b["rm"], b["rv"], b["nbt"], -1.0, R.EPS, True,
                True, b["save"])
        B.bwd_stats(dy, None, x, ch, 2, b["save"], dv["gamma"], dv["beta"], part, tk, b["out"], b["dgamma"],
                    b["dbeta"])
        B.bwd_elemt(dy, None, x, ch, 2, b["save"], b["out"], b["st"], dv["gamma"], dv["beta"], b["dx"], None)

    def reset(b):
        for k, v in b.items():
            if k == "rm":
                v.copy_(rm0)
            elif k == "rv":
                v.copy_(rv0)
            elif k == "nbt":
                v.zero_()
            else:
                v.fill_(NAN)

    defined = lambda k, v: torch.cat([v[:2 * ch + 1], v[2 * ch + 4:]]) if k == "st" else v  # noqa: E731
    with _targets(B, blocks):
        eager = buffers()
        step(eager)
        torch.cuda.synchronize()
        assert not any(defined(k, v).isnan().any() for k, v in eager.items())
        ref = _int_ref(300 * 32 * U, ch, M)
        _same(eager["st"][:ch], ref["fwd"][0], "eager s1")
        _same(eager["st"][ch:2 * ch], ref["fwd"][1], "eager s2")
        gb = buffers()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step(gb)
        for rep in range(2):
            reset(gb)
            graph.replay()
            torch.cuda.synchronize()
            for k, v in eager.items():
                assert torch.equal(defined(k, gb[k]), defined(k, v)), f"replay {rep}: {k} differs from eager"
            assert int(tk.abs().sum()) == 0, f"replay {rep}: tickets not re-armed"


def test_zz_report_ratios():
    """Largest observed error / bound per section (how much room the derived bounds leave)."""
    for k, (v, name) in sorted(RATIOS.items()):
        print(f"\nerror/bound maximum, section {k}: {v:.4f} ({name})", end="")
    assert all(v <= 1 for v, _ in RATIOS.values())
