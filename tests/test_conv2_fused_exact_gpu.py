"""Exact integer tests of the fused conv2 launches (csrc/kernels/convnet_fused.hip), each called directly
through C.convnet so that a case pins its launch.  Cases and float64 references: tests/_conv2_fused_ref.py
(its conditions: tests/test_conv2_fused_ref_cpu.py).  Every output is prefilled with NaN (0xFF for
bytes) and has a guard region behind it whose bits must survive.

  a  conv2_fwd, training (conv5x5_kernel<T, 16, 32, 14, 14, MODE 0, PRO 1, ..., WR>): y2 element for
     element, p1 / xh1 / idx1, each of the B * fwd2_split slab rows on its own, the fstats2 shift block
     (the other words untouched), BN1's published sums and ONE running-statistics update (what the
     outputs can show of "once per launch": nbt1 == 1 and values within the bound of a single update
     from a start far from the statistics; workgroups that all read the old values before any of them
     writes would store the same bits, which no output distinguishes from one writer); impulse sets;
     a launch after one with large values; reruns bitwise equal
  b  conv2_fwd, eval (MODE 1): the same case through rm1 / rv1, with and without the pooled outputs
  c  a and b in fp32, within K u A with the K_* of _conv2_fused_ref.py (counted there, operation by
     operation); idx1 stays exact
  d  the conv2 weight gradient with BN2's backward on the fly (conv5x5_wgrad_body NSL) through
     conv_wgrad_bn and conv2_bwd at every split allowed: each image's row [dW | db], dg2 / dbe2, the
     launches bitwise equal to each other and run to run; impulse sets for two (output tile,
     input-channel slice) pairs
  e  the fp32 data-gradient role of conv2_bwd / conv2_dgrad: dp1 and the 4 B quarter rows

bf16 / fp16 compare exactly (bound 0); the failure message names the first differing element.
"""
import pytest
import torch

from . import _conv2_fused_ref as X
from . import _convblock_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = R.EPS32
MOM = 0.1
GUARD = 256
IDS = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
DT = pytest.mark.parametrize("dtype", R.DTYPES, ids=[IDS[d] for d in R.DTYPES])
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.uint8: torch.uint8,
        torch.int64: torch.int64}
FWD_CASES = [(1, 11), (3, 13)]  # (B, seed); (3, 17) and (2, 19): the stale-LDS pair
RATIOS = {}


class _Out:
    """An output buffer prefilled with NaN (bytes: 0xFF), with GUARD more elements behind it."""

    def __init__(self, shape, dtype, init=None):
        self.n = int(torch.Size(shape).numel())
        fill = float("nan") if dtype.is_floating_point else (0xFF if dtype == torch.uint8 else -1)
        self.whole = torch.full((self.n + GUARD,), fill, device=DEV, dtype=dtype)
        self.t = self.whole[:self.n].view(shape)
        if init is not None:
            self.t.copy_(init.to(dtype).reshape(shape))
        self.guard0 = self.whole[self.n:].view(BITS[dtype]).clone()

    def bits(self):
        """The written region as integers (CPU); asserts the guard kept its bits."""
        assert torch.equal(self.whole[self.n:].view(BITS[self.whole.dtype]), self.guard0), "guard region written"
        return self.t.reshape(-1).view(BITS[self.whole.dtype]).cpu()


def _collect(o):
    torch.cuda.synchronize()
    return {k: v.bits() for k, v in o.items()}, {k: v.t.cpu() for k, v in o.items()}


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        ne = (a[k] != b[k]).nonzero()
        assert ne.numel() == 0, f"{what}: {k} differs at {ne[:4].flatten().tolist()} ({ne.shape[0]} elements)"


def _cmp(got, want, what, A=None, K=0, key=None):
    """|got - want| <= K u A per element (K = 0: equal); names the first element that is not."""
    got, want = got.double().reshape(want.shape), want.double()
    assert not bool(torch.isnan(got).any()), f"{what}: not written at {torch.isnan(got).nonzero()[:4].tolist()}"
    bnd = torch.zeros_like(want) if K == 0 else K * X.U32 * A.reshape(want.shape)
    err = (got - want).abs()
    if K and key is not None and bool((bnd > 0).any()):
        RATIOS[key] = max(RATIOS.get(key, 0.0), float((err[bnd > 0] / bnd[bnd > 0]).max()))
    bad = ~(err <= bnd)
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} differ, first at {bad.nonzero()[0].tolist()}: "
                                 f"got {got[bad][0].item()!r} want {want[bad][0].item()!r} bound {bnd[bad][0].item():.3e}")


def _k(dtype, K):
    return K if dtype == torch.float32 else 0


def _pack_fwd(w2, dtype):
    """[32][16][5][5] -> the forward LDS tile [32][424], k = tap * 16 + ci, K padding zero."""
    t = torch.zeros(32, 424, dtype=torch.float64)
    t[:, :400] = w2.reshape(32, 16, 25).permute(0, 2, 1).reshape(32, 400)
    return t.reshape(-1).to(dtype)


def _pack_dgrad(w2, dtype):
    """-> the data-gradient tile [16][808], k = (24 - tap) * 32 + co (the flipped transpose)."""
    t = torch.zeros(16, 808, dtype=torch.float64)
    t[:, :800] = w2.reshape(32, 16, 25).flip(2).permute(1, 2, 0).reshape(16, 800)
    return t.reshape(-1).to(dtype)


def _ns(C, dtype):
    return C.convnet.fwd2_split(dtype == torch.float32)


# =============================================================================== forward
def _fwd(C, c, dtype, train=True, outs=True):
    """One conv2_fwd launch on case c: (bits by name, tensors by name)."""
    B, ns, f32 = c["B"], _ns(C, dtype), torch.float32
    dev = lambda t, dt=f32: t.to(dt).to(DEV).contiguous()  # noqa: E731
    nan33 = torch.full((33,), float("nan"), dtype=torch.float64)
    o = dict(y2=_Out((B, 32, 14, 14), dtype), fstats2=_Out((97,), f32),
             fstats1=_Out((49,), f32, torch.cat([nan33, c["shift1"]])),
             rm1=_Out((16,), f32, c["rm0"] if train else c["shift1"]),
             rv1=_Out((16,), f32, c["rv0"] if train else torch.ones(16)),
             nbt1=_Out((1,), torch.int64, torch.tensor([0 if train else 5])))
    if train:
        o["fslab2"] = _Out((B * ns * 65,), f32)
    if outs:
        o.update(p1=_Out((B, 16, 14, 14), dtype), idx1=_Out((B, 16, 14, 14), torch.uint8), xh1=_Out((B, 16, 14, 14), dtype))
    po = [o[k].t if outs else None for k in ("p1", "idx1", "xh1")]
    C.convnet.conv2_fwd(dev(c["y1"], dtype), dev(c["rows1"].reshape(-1)) if train else None, o["fstats1"].t, dev(c["gamma"]),
                        dev(c["beta"]), o["rm1"].t, o["rv1"].t, o["nbt1"].t, MOM, EPS, train, dev(c["w2"]), dev(c["bias2"]),
                        o["y2"].t, o["fslab2"].t if train else None, o["fstats2"].t, dev(c["rm2"]), *po,
                        _pack_fwd(c["w2"], dtype).to(DEV), None)
    return _collect(o)


def _check_fwd(C, c, dtype, bits, t, tag, train=True, outs=True):
    ns = _ns(C, dtype)
    r = X.fwd_ref(c, dtype, ns)
    f = IDS[dtype] + " "
    _cmp(t["y2"], r["y2"], f"{tag} y2", r["A_y2"], _k(dtype, X.K_Y2), f + "y2")
    if outs:
        ne = (t["idx1"] != r["idx1"]).nonzero()
        assert ne.numel() == 0, (f"{tag} idx1: {ne.shape[0]} differ, first at {ne[0].tolist()}: got "
                                 f"{int(t['idx1'][tuple(ne[0])])} want {int(r['idx1'][tuple(ne[0])])}")
        _cmp(t["p1"], r["p1"], f"{tag} p1", r["A_p1"], _k(dtype, X.K_PRO), f + "p1")
        _cmp(t["xh1"], r["xh1"], f"{tag} xh1", r["A_xh1"], _k(dtype, X.K_PRO), f + "xh1")
    nan = torch.full((1,), float("nan")).view(torch.int32).item()
    if train:
        rows, Ar = t["fslab2"].view(-1, 65), r["A_rows"]
        _cmp(rows[:, :32], r["rows"][:, :32], f"{tag} BN2 slab rows (b * {ns} + split, channel), sums", Ar[:, :32],
             _k(dtype, X.K_S1), f + "row sums")
        _cmp(rows[:, 32:64], r["rows"][:, 32:64], f"{tag} BN2 slab rows, sums of squares", Ar[:, 32:64],
             _k(dtype, X.K_S2), f + "row squares")
        _cmp(rows[:, 64], r["rows"][:, 64], f"{tag} BN2 slab rows, counts")
        # fstats2: conv5x5_body (MODE 0) writes the shift block [65, 97) = rm2 from workgroup 0, nothing else
        _cmp(t["fstats2"][65:], c["rm2"], f"{tag} fstats2 shift block")
        assert bool((bits["fstats2"][:65] == nan).all()), f"{tag} fstats2: a word before the shift block was written"
        # fstats1: the leader publishes the column sums [0 | n | n]; the shift block stays
        n = float(c["n"])
        _cmp(t["fstats1"], torch.cat([torch.zeros(16), torch.full((17,), n), c["shift1"].float()]), f"{tag} fstats1")
        st = X.fwd_running(c)
        assert int(t["nbt1"]) == 1, f"{tag} num_batches_tracked {int(t['nbt1'])}"
        for k, a in (("rm", t["rm1"]), ("rv", t["rv1"])):
            bnd = R.B.bound(st["A_" + k], st[k], torch.float32)
            err = (a.double() - st[k]).abs()
            assert bool((err <= bnd).all()), (f"{tag} running {k}: channel {int((err / bnd).argmax())} got "
                                              f"{a[(err / bnd).argmax()].item()} want {st[k][(err / bnd).argmax()].item()}")
    else:
        assert bool((bits["fstats2"] == nan).all()), f"{tag} fstats2 written in eval"
        _cmp(t["fstats1"][33:], c["shift1"], f"{tag} fstats1 shift")
        assert bool((bits["fstats1"][:33] == nan).all()), f"{tag} fstats1 written in eval"
        _cmp(t["rm1"], c["shift1"], f"{tag} rm1 (eval)")
        _cmp(t["rv1"], torch.ones(16), f"{tag} rv1 (eval)")
        assert int(t["nbt1"]) == 5


@DT
@pytest.mark.parametrize("Bn,seed", FWD_CASES)
def test_forward_train(C, Bn, seed, dtype):
    """Sections a / c.  y2 is the exact convolution rounded once (fp32: within K_Y2 u A); every slab
    row is its own workgroup's [sum | sum of squares | count]; BN1's running statistics move once."""
    c = X.fwd_int(Bn, seed)
    bits, t = _fwd(C, c, dtype)
    _check_fwd(C, c, dtype, bits, t, f"B={Bn} {IDS[dtype]}")
    bits2, _ = _fwd(C, c, dtype)
    _same(bits, bits2, "rerun")


@DT
@pytest.mark.parametrize("outs", [True, False], ids=["pooled-outputs", "no-pooled-outputs"])
@pytest.mark.parametrize("Bn,seed", FWD_CASES)
def test_forward_eval(C, Bn, seed, outs, dtype):
    """Section b (c in fp32): MODE 1 with rm1 = shift, rv1 = 1 as the statistics; without the pooled
    outputs it is the call of ops/convnet_fused.py's eval path.  Nothing but y2 (and p1 / idx1 / xh1)
    is written: rm1 / rv1 / nbt1 / fstats1 and a sentinel-filled fstats2 keep their bits."""
    c = X.fwd_int(Bn, seed)
    bits, t = _fwd(C, c, dtype, train=False, outs=outs)
    _check_fwd(C, c, dtype, bits, t, f"eval B={Bn} {IDS[dtype]}", train=False, outs=outs)
    _same(bits, _fwd(C, c, dtype, train=False, outs=outs)[0], "rerun")


@DT
@pytest.mark.parametrize("variant", [0, 1], ids=["range-edge", "image-border"])
def test_forward_impulse(C, variant, dtype):
    """25 images, one tap each (_conv2_fused_ref.fwd_impulse): the image's output is the single weight
    times the single pooled pixel at the single expected place (two where images share a channel)."""
    c, where = X.fwd_impulse(variant, _ns(C, dtype))
    bits, t = _fwd(C, c, dtype)
    _check_fwd(C, c, dtype, bits, t, f"impulse {variant} {IDS[dtype]}")
    y2 = t["y2"].double()
    for i, (co, oh, ow, val) in enumerate(where):
        got = y2[i, co, oh, ow].item()
        # (A / |value| = (v + 1/2) / (v - 1/2) <= 3)
        assert abs(got - val) <= _k(dtype, X.K_Y2) * X.U32 * abs(val) * 3, \
            f"tap {divmod(i, 5)}: y2[{i}][{co}][{oh}][{ow}] = {got}, want {val}"
        assert int((y2[i] != 0).sum()) <= 2, f"tap {divmod(i, 5)}: outputs at {(y2[i] != 0).nonzero().tolist()}"


@DT
def test_forward_after_large_values(C, dtype):
    """A launch with large values, then different data: stale LDS (a row of the image tile left unstaged,
    a halo not zeroed, a statistics partial) would reach an exact sum.  Reruns are bitwise equal."""
    big = dict(X.fwd_int(3, 17))
    sh = big["shift1"].view(1, -1, 1, 1)
    big["y1"], big["w2"] = sh + (big["y1"] - sh).abs() * 16, big["w2"] * 64
    c = X.fwd_int(2, 19)
    _fwd(C, big, dtype)
    bits, t = _fwd(C, c, dtype)
    _check_fwd(C, c, dtype, bits, t, f"after large values, {IDS[dtype]}")
    _fwd(C, big, dtype)
    _same(bits, _fwd(C, c, dtype)[0], "after a launch with large values")


# =============================================================================== backward launches
def _bwd(C, c, dtype, form, split=0):
    """conv2_bwd, conv2_dgrad or conv_wgrad_bn (layer 2) on case c; what a case lacks is zero."""
    cn, B, f32 = C.convnet, c["B"], torch.float32
    dev = lambda t, dt=f32: t.to(dt).to(DEV).contiguous()  # noqa: E731
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
    lsum = dev(c["lsum"].reshape(-1)) if "lsum" in c else None
    y2, dp2, idx2, fst, g2 = dev(c["y2"], dtype), dev(c["dp2"], dtype), c["idx2"].to(DEV), dev(c["fstats2"]), dev(c["gamma"])
    gsum = torch.zeros(B * 64, device=DEV)
    o = {}
    if form != "conv_wgrad_bn":
        o.update(dp1=_Out((B, 16, 14, 14), dtype), bslab1=_Out((cn.dgrad2_rows(B, dtype == f32) * 32,), f32))
        wpk_d = _pack_dgrad(c.get("w2", z(32, 16, 5, 5)), dtype).to(DEV)
        idx1 = c["idx1"].to(DEV) if "idx1" in c else torch.zeros(B, 16, 14, 14, dtype=torch.uint8, device=DEV)
        xh1 = dev(c.get("xh1", z(B, 16, 14, 14)), dtype)
    if form != "conv2_dgrad":
        assert cn.wgrad_bn_rows(2, B) == B
        o.update(wslab2=_Out((B * X.N2,), f32), dg2=_Out((32,), f32), dbe2=_Out((32,), f32))
    if form == "conv2_bwd":
        cn.conv2_bwd(wpk_d, y2, dp2, idx2, fst, gsum, g2, EPS, o["dp1"].t, idx1, xh1, o["bslab1"].t,
                     dev(c["p1"], dtype), o["wslab2"].t, None, lsum, o["dg2"].t, o["dbe2"].t, None, None, None, None,
                     None, split)
    elif form == "conv2_dgrad":
        cn.conv2_dgrad(wpk_d, y2, dp2, idx2, fst, gsum, g2, EPS, o["dp1"].t, idx1, xh1, o["bslab1"].t, None, split)
    else:
        cn.conv_wgrad_bn(dev(c["p1"], dtype), y2, dp2, idx2, fst, gsum, lsum, g2, EPS, o["dg2"].t, o["dbe2"].t,
                         o["wslab2"].t, None)
    bits, t = _collect(o)
    for k, v in t.items():
        nn = torch.isnan(v.float()).nonzero()
        assert nn.numel() == 0, f"{form} {k}: not written at {nn[:4].tolist()}"
    return bits, t


def _wg_launches(dtype):
    return [("conv_wgrad_bn", 0)] + [("conv2_bwd", s) for s in ((0, 4) if dtype == torch.float32 else (0, 2, 4))]


def _check_wgrad(C, c, dtype, tag):
    want, A = X.wgrad_ref(c)
    first = None
    for form, split in _wg_launches(dtype):
        bits, t = _bwd(C, c, dtype, form, split)
        what = f"{tag} {form} split {split}"
        # (image, column): dW[co][ci][kh][kw] at (co * 16 + ci) * 25 + tap, db[co] at 12800 + co
        _cmp(t["wslab2"], want, f"{what}: slab (image, column)", A, _k(dtype, X.K_WG), IDS[dtype] + " wgrad rows")
        _cmp(t["dbe2"], c["lsum"].sum(0)[:32], f"{what} dbe2")
        _cmp(t["dg2"], c["lsum"].sum(0)[32:], f"{what} dg2")
        wg = {k: bits[k] for k in ("wslab2", "dg2", "dbe2")}
        first = wg if first is None else first
        _same(first, wg, f"{what} vs conv_wgrad_bn")
        _same(wg, {k: _bwd(C, c, dtype, form, split)[0][k] for k in wg}, f"{what} rerun")


@DT
@pytest.mark.parametrize("Bn", [1, 2, 3])
def test_wgrad_rows(C, Bn, dtype):
    """Section d: each image's row equals [dW | db] of that image exactly (fp32: K_WG u A), whichever
    launch and split wrote it; dg2 / dbe2 are the exact column sums of lsum."""
    _check_wgrad(C, X.wgrad_int(Bn, 30 + Bn), dtype, f"B={Bn} {IDS[dtype]}")


@DT
@pytest.mark.parametrize("co,ci", [(3, 2), (20, 13)], ids=["tile0-slice0", "tile1-slice1"])
@pytest.mark.parametrize("variant", [0, 1], ids=["dy-on-border", "x-on-border"])
def test_wgrad_impulse(C, variant, co, ci, dtype):
    """One dp2 pixel and one p1 pixel per tap: a tile, slice or tap index that is off writes the value to
    another column, which the message names."""
    c, where = X.wgrad_impulse(variant, co, ci, 5)
    want, A = X.wgrad_ref(c)
    for form in ("conv_wgrad_bn", "conv2_bwd"):
        rows = _bwd(C, c, dtype, form)[1]["wslab2"].view(25, X.N2).double()
        for t, (col, val, dbv) in enumerate(where):
            nz = rows[t].nonzero().flatten().tolist()
            assert nz == [col, 12800 + co], f"{form} tap {divmod(t, 5)}: non-zero columns {nz[:8]}, want {[col, 12800 + co]}"
        _cmp(rows, want, f"{form} impulse rows", A, _k(dtype, X.K_WG))


# =============================================================================== e
@pytest.mark.parametrize("form", ["conv2_bwd", "conv2_dgrad"])
@pytest.mark.parametrize("Bn", [1, 3])
def test_dgrad_fp32(C, Bn, form):
    """Section e: the fp32 instantiation (split 4 only, 16x16x4 MFMA, dynamic LDS in the merged launch)
    on the integer case: dp1 within K_DG u A, each of the 4 B quarter rows within K_Q1 / K_Q2 u A."""
    dtype = torch.float32
    c = X.dgrad_int(Bn, 50 + Bn)
    r = X.dgrad_ref(c)
    bits, t = _bwd(C, c, dtype, form)
    _cmp(t["dp1"], r["dp1"], f"{form} dp1", r["A"], X.K_DG, "fp32 dp1")
    rows = t["bslab1"].view(4 * Bn, 32)
    _cmp(rows[:, :16], r["rows"][:, :16], f"{form} quarter rows (4 b + quarter, channel) S1", r["A_rows"][:, :16],
         X.K_Q1, "fp32 quarter S1")
    _cmp(rows[:, 16:], r["rows"][:, 16:], f"{form} quarter rows S2", r["A_rows"][:, 16:], X.K_Q2, "fp32 quarter S2")
    _same(bits, _bwd(C, c, dtype, form, 4)[0], "rerun at the forced split 4")


def test_zz_report_ratios(C):
    """Largest error / bound of the fp32 sections (how much room the derived K leave)."""
    for k, v in sorted(RATIOS.items()):
        print(f"\nerror/bound maximum, {k}: {v:.4f}", end="")
    assert all(v < 1 for v in RATIOS.values())
