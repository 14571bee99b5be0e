"""The classifier head kernels against tests/_head_ref.py: exact on integer inputs, per
element against float64 elsewhere.

  a. linear_fwd / linear_bwd (csrc/kernels/head.hip): integer operands, bit-for-bit;
  b. the three cross-entropy kernels of head.hip and ce_bwd: loss and gradient per element
     within the derived bounds, label smoothing, ignored rows, bad targets, a -inf column,
     the exact identities of the scaled outputs, the re-armed ticket;
  c. accuracy: exact counts on tied rows;
  d. the ConvNet head: head_fwd / head_bwd / fc_wgrad (csrc/kernels/convnet_fused.hip) and
     head_step (csrc/kernels/convnet_head.hip), its loss word and its graph replay.

Every kernel is called through C.head / C.convnet / C.convnet_head, so each case pins its
path; every output buffer starts as NaN (0xFF for bytes).  The largest error / bound ratio of
each bounded check is kept in RATIOS and printed by the last test (pytest -s).
"""
import itertools
import math

import pytest
import torch

from . import _head_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
DTYPES = list(R.Q)
NAN = float("nan")
INF = float("inf")
S32 = float(torch.tensor(0.1, dtype=F32))  # the smoothing the kernels see for 0.1
SCALE = 1024.0
RATIOS = {}


def _id(v):
    return str(v).replace("torch.", "")


def _nan(shape, dtype=F32):
    if dtype == torch.uint8:
        return torch.full(shape, 0xFF, dtype=dtype, device=DEV)
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def _cpu(t):
    return t.detach().double().cpu()


def _same(got, exp, what):
    """Bit-for-bit (NaN equals NaN), with the first differing index."""
    got, exp = got.detach().cpu(), exp.detach().cpu()
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, exp.dtype, got.shape, exp.shape)
    eq = got == exp
    if got.is_floating_point():
        eq = eq | (got.isnan() & exp.isnan())
    if not bool(eq.all()):
        bad = (~eq).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ, first at {i}: "
                             f"got {got[i].item()}, expected {exp[i].item()}; last at {tuple(bad[-1].tolist())}")


def _within(got, ref, bnd, name, section):
    """|got - ref| <= bnd on every element; NaN fails."""
    ref = torch.as_tensor(ref, dtype=torch.float64)
    err = (_cpu(got).reshape(ref.shape) - ref).abs()
    bnd = torch.as_tensor(bnd, dtype=torch.float64).expand_as(err)
    if err.numel() == 0:
        return
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd.clamp(min=1e-300))
    worst = float(ratio.max()) if not ratio.isnan().any() else INF
    bad = ~(err <= bnd)
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.numel()} outside the bound, error / bound <= {worst:.3g}"
    if worst >= RATIOS.get(section, (0.0, ""))[0]:
        RATIOS[section] = (worst, name)


# =============================================================================== a
@pytest.mark.parametrize("variant", ["full", "nobias", "nodx"])
@pytest.mark.parametrize("M,N,K", R.LIN_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_linear_exact(C, dtype, M, N, K, variant):
    """Integer operands: out, dx (rounded once to the storage type), dw and db bit for bit."""
    t = R.lin_inputs(M, N, K, 7 * M + N)
    bias = variant != "nobias"
    x, dout = t["x"].to(dtype).to(DEV), t["dout"].to(dtype).to(DEV)
    w = t["w"].float().to(DEV)
    b = t["b"].float().to(DEV) if bias else None
    out = _nan((M, N), dtype)
    C.head.linear_fwd(x, w, b, out)
    dx = _nan((M, K), dtype) if variant != "nodx" else None
    dw = _nan((N, K))
    db = _nan((N,)) if bias else None
    C.head.linear_bwd(dout, x, w, dx, dw, db)
    torch.cuda.synchronize()
    tag = f"linear {M}x{N}x{K} {_id(dtype)} {variant}"
    _same(out, R.linear(t["x"], t["w"], t["b"] if bias else None)[0].float().to(dtype), tag + " out")
    rdx, rdw, rdb = R.linear_bwd(t["dout"], t["x"], t["w"])
    if dx is not None:
        _same(dx, rdx.float().to(dtype), tag + " dx")
    _same(dw, rdw.float(), tag + " dw")
    if db is not None:
        _same(db, rdb.float(), tag + " db")


# =============================================================================== b
# (B, N, smoothing, ignored rows (0 | every k-th | "all"), scaled)
CE_CASES = [
    # ce_fwd_kernel<16>
    (1, 1, 0.0, 0, False), (3, 2, 0.1, 0, True), (37, 10, 0.0, 3, True), (37, 10, 0.1, "all", False),
    (64, 16, 0.1, 5, False),
    # ce_fwd_kernel<64>
    (64, 17, 0.0, 0, True), (33, 65, 0.1, 4, False), (5, 1000, 0.1, 0, True), (5, 1000, 0.0, "all", True),
    (65, 1025, 0.0, 7, False), (65, 1025, 0.1, 0, True),
    # ce_fwd_rows_kernel<4> (the last: 1024 workgroups striding, the partial list at CE_MAXG)
    (65, 10, 0.1, 0, True), (130, 256, 0.0, 9, False), (4099, 3, 0.1, 11, True),
    # ce_fwd_rows_kernel<16>
    (67, 257, 0.1, 3, True), (65, 1024, 0.0, "all", False), (65, 1024, 0.1, 0, False),
]


def _multi_wg(Bn, N):
    return Bn > 64 and N <= 1024


def _ce_launch(C, lg64, tgt, dtype, smoothing, scaled):
    """ce_fwd on NaN-filled outputs; a multi-workgroup case runs twice on the per-device
    workspace (its ticket re-arms itself).  Returns CPU (loss[2], dlog, dls | None)."""
    Bn, N = lg64.shape
    lg, t = lg64.to(dtype).to(DEV), tgt.to(DEV)
    scale = torch.tensor([SCALE], device=DEV) if scaled else None
    for _ in range(2 if _multi_wg(Bn, N) else 1):
        loss, dlog = _nan((2,)), _nan((Bn, N))
        dls = _nan((Bn, N), dtype) if scaled else None
        C.head.ce_fwd(lg, t, loss, dlog, -100, smoothing, scale, dls)
    torch.cuda.synchronize()
    return loss.cpu(), dlog.cpu(), (dls.cpu() if scaled else None)


def _ce_check(out, lg64, tgt, dtype, smoothing, scaled, tag, section="b"):
    loss, dlog, dls = out
    s = S32 if smoothing else 0.0
    ref_loss, ref_dlog, A_loss, A_dlog = R.cross_entropy(lg64, tgt, -100, s)
    if not math.isfinite(float(ref_loss)):
        _same(loss[:1], ref_loss.float().reshape(1), tag + " loss")
    else:
        _within(loss[0], ref_loss, R.loss_bound(A_loss), tag + " loss", section + " loss")
    _within(dlog, ref_dlog, R.dlog_bound(A_dlog), tag + " dlog", section + " dlog")
    ign = tgt == -100
    assert not dlog[ign].any(), tag + ": an ignored row's gradient must be exactly 0"
    if scaled:
        _same(loss[1:], loss[:1] * torch.tensor(SCALE), tag + " loss[1] == loss[0] * scale")
        _same(dls, (dlog * torch.tensor(SCALE)).to(dtype), tag + " dls == (dlog * scale).to(dtype)")
    else:
        assert math.isnan(float(loss[1])), tag + ": loss[1] written without a scale"
    return ref_loss


@pytest.mark.parametrize("Bn,N,smoothing,ignored,scaled", CE_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_cross_entropy_per_element(C, dtype, Bn, N, smoothing, ignored, scaled):
    lg64 = R.ce_logits(Bn, N, 100 * Bn + N)
    tgt = R.ce_targets(Bn, N, 100 * Bn + N, ignored)
    tag = f"ce {Bn}x{N} {_id(dtype)} s={smoothing} ign={ignored}"
    out = _ce_launch(C, lg64, tgt, dtype, smoothing, scaled)
    ref_loss = _ce_check(out, lg64, tgt, dtype, smoothing, scaled, tag)
    if ignored == "all":
        assert math.isnan(float(out[0][0])) and math.isnan(float(ref_loss)) and not out[1].any()
    dlog = out[1].to(DEV)
    for g in (1.0, 3.0, SCALE):
        o = _nan((Bn, N), dtype)
        C.head.ce_bwd(dlog, torch.tensor([g], device=DEV), o)
        _same(o, (out[1] * torch.tensor(g)).to(dtype), tag + f" ce_bwd g={g}")


EDGE_SHAPES = [(37, 10), (5, 1000), (130, 256), (67, 257)]  # one per kernel family member


@pytest.mark.parametrize("bad", ["N", "-1"])
@pytest.mark.parametrize("Bn,N", EDGE_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_cross_entropy_bad_target(C, dtype, Bn, N, bad):
    """A counted row with target N or -1: NaN loss, every gradient as the reference (the bad
    row's is (softmax - smoothing / N) / count)."""
    lg64 = R.ce_logits(Bn, N, 100 * Bn + N + 1)
    tgt = R.ce_targets(Bn, N, 100 * Bn + N + 1, 4)
    tgt[2] = N if bad == "N" else -1
    tag = f"ce bad target {bad} {Bn}x{N} {_id(dtype)}"
    out = _ce_launch(C, lg64, tgt, dtype, 0.1, True)
    ref_loss = _ce_check(out, lg64, tgt, dtype, 0.1, True, tag)
    assert math.isnan(float(ref_loss)) and math.isnan(float(out[0][0])) and math.isnan(float(out[0][1]))
    assert bool(out[1][2].isfinite().all()) and bool(out[1][2].any())


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("Bn,N", EDGE_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_cross_entropy_inf_column(C, dtype, Bn, N, smoothing):
    """A masked class (-inf in a column no target names): the loss is finite and within the
    bound at smoothing 0, +inf at smoothing 0.1 (torch's values); the column's gradient is 0
    at smoothing 0.  (While both kernels multiplied the smoothing term by 0 instead of dropping
    it, 0 * inf made the smoothing-0 loss NaN in every case here.)"""
    lg64 = R.ce_logits(Bn, N, 100 * Bn + N + 2)
    col = N // 2
    lg64[:, col] = -INF
    tgt = R.ce_targets(Bn, N, 100 * Bn + N + 2, 5)
    tgt = torch.where(tgt == col, torch.full_like(tgt, col + 1), tgt)
    tag = f"ce -inf column {Bn}x{N} {_id(dtype)} s={smoothing}"
    out = _ce_launch(C, lg64, tgt, dtype, smoothing, False)
    ref_loss = _ce_check(out, lg64, tgt, dtype, smoothing, False, tag)
    if smoothing == 0:
        assert math.isfinite(float(ref_loss)) and math.isfinite(float(out[0][0])), (tag, float(out[0][0]))
        assert not out[1][:, col].any()
    else:
        assert float(ref_loss) == INF and float(out[0][0]) == INF, (tag, float(out[0][0]))


# =============================================================================== c
@pytest.mark.parametrize("Bn,N", R.ACC_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_accuracy_exact_counts(C, dtype, Bn, N):
    """Tied rows (the lowest index wins), a row of -inf, the per-lane loop (N > 64), the
    grid-stride loop (B > 256), and accumulation over two calls."""
    lg64, tgt = R.acc_inputs(Bn, N, 10 * Bn + N)
    rows, hit = R.accuracy(R.rounded(lg64, dtype), tgt)
    lg, t = lg64.to(dtype).to(DEV), tgt.to(DEV)
    counters = torch.zeros(2, device=DEV)
    for call in (1, 2):
        C.head.accuracy(lg, t, counters)
        assert counters.tolist() == [float(call * rows), float(call * hit)], (Bn, N, _id(dtype), call)


# =============================================================================== d
_STATE = {}
_HEAD = {}


def _state():
    if "s" not in _STATE:
        _STATE["s"] = torch.zeros(1, dtype=torch.int64, device=DEV)
    return _STATE["s"]


def _head_case(Bn, N, nrows):
    k = (Bn, N, nrows)
    if k not in _HEAD:
        if len(_HEAD) > 8:
            _HEAD.clear()
        _HEAD[k] = R.head_inputs(Bn, N, R.head_seed(Bn, N), nrows)
    return _HEAD[k]


def _nrows(C, kind, Bn, dtype):
    """Slab row counts: as the op passes; one row; above 3 * 43, the second load batch of
    strided_rowsum in both head kernels (3 lane groups of 24 | 43 rows)."""
    return (Bn * int(C.convnet.fwd2_split(dtype == F32)), 1, 131)[kind % 3]


NBT0 = 4


def _head_buffers(t, dtype, Bn, N):
    f = lambda v: v.float().to(DEV)
    return dict(y2=t["y2"].to(dtype).to(DEV), fslab=f(t["rows"].reshape(-1)),
                fstats=torch.cat([_nan((2 * R.HC + 1,)), f(t["shift"])]), g=f(t["gamma"]), b=f(t["beta"]),
                rm=f(t["rm0"]), rv=f(t["rv0"]), nbt=torch.full((1,), NBT0, dtype=torch.int64, device=DEV),
                wfc=f(t["wfc"]), bfc=f(t["bfc"]), logits=_nan((Bn, N), dtype), p2=_nan((Bn, R.HK), dtype),
                idx2=_nan((Bn, R.HK), torch.uint8), xh2=_nan((Bn, R.HK), dtype))


def _check_forward(d, t, dtype, Bn, N, momentum, tag):
    """d1: statistics, running statistics, p2 / idx2 / xh2 / logits."""
    HC = R.HC
    mom = None if momentum < 0 else R.MOM32
    st = R.bn_from_rows(t["rows"], t["shift"], t["gamma"], t["beta"], t["eps"], t["rm0"], t["rv0"], mom, NBT0 + 1)
    _same(d["fstats"][:2 * HC + 1], st["sums"].float(), tag + " fstats2 column sums")
    _same(d["fstats"][2 * HC + 1:], t["shift"].float(), tag + " fstats2 shift copy")
    assert int(d["nbt"]) == NBT0 + 1, tag
    _within(d["rm"], st["rm"], R.B.bound(st["A_rm"], st["rm"], F32), tag + " running_mean", "d1 running")
    _within(d["rv"], st["rv"], R.B.bound(st["A_rv"], st["rv"], F32), tag + " running_var", "d1 running")
    p, idx, xhat, A_p, A_xh = R.bn_relu_pool(t["y2"], st["mean"], st["invstd"], t["gamma"], t["beta"], dtype)
    _same(d["idx2"], idx, tag + " idx2")
    _within(d["xh2"], xhat, R.B.bound(A_xh, xhat, dtype), tag + " xh2", "d1 xh2")
    w_r = R.rounded(t["wfc"], dtype)
    if dtype != F32:
        _same(d["p2"], p.to(dtype), tag + " p2")
        _same(d["logits"], R.fc(p, w_r, t["bfc"])[0].float().to(dtype), tag + " logits")
    else:
        _within(d["p2"], p, R.B.bound(A_p, p, F32), tag + " p2", "d1 p2 fp32")
        lg, A = R.fc(_cpu(d["p2"]), w_r, t["bfc"])
        _within(d["logits"], lg, R.dot_bound(R.HK, A, lg, F32), tag + " logits", "d1 logits fp32")


FWD_CASES = [(Bn, N, i) for i, (Bn, N) in enumerate(itertools.product(R.HEAD_B, R.HEAD_N + R.HEAD_N_FWD))]


@pytest.mark.parametrize("Bn,N,i", FWD_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_head_fwd(C, dtype, Bn, N, i):
    nrows = _nrows(C, i, Bn, dtype)
    momentum = 0.1 if i % 2 == 0 else -1.0
    t = _head_case(Bn, N, nrows)
    d = _head_buffers(t, dtype, Bn, N)
    C.convnet.head_fwd(d["y2"], d["fslab"], d["fstats"], d["g"], d["b"], d["rm"], d["rv"], d["nbt"], momentum,
                       t["eps"], True, d["wfc"], d["bfc"], d["logits"], d["p2"], d["idx2"], d["xh2"], None)
    torch.cuda.synchronize()
    _check_forward(d, t, dtype, Bn, N, momentum, f"head_fwd B={Bn} N={N} {_id(dtype)} rows={nrows} mom={momentum}")


def _targets(Bn, N, ign, seed):
    tgt = R.ce_targets(Bn, N, seed)
    if ign == "two":
        tgt[0] = tgt[Bn - 1] = -100
    elif ign == "all":
        tgt[:] = -100
    elif ign == "top":
        tgt[Bn - 1] = -100
    return tgt


def _step_buffers(d, tgt, scaled, dtype, Bn, N, chk=True):
    """The NaN-filled outputs of a head_step launch (added to d)."""
    d["tgt"] = tgt.to(DEV)
    d["loss"], d["dlog"] = _nan((2,)), _nan((Bn, N))
    if scaled:
        d["scale"] = torch.tensor([SCALE], device=DEV)
        d["dls"], d["dp2"], d["bsum"] = _nan((Bn, N), dtype), _nan((Bn, R.HK), dtype), _nan((Bn * 2 * R.HC,))
        d["chk"] = torch.full((2,), -1, dtype=torch.int32, device=DEV) if chk else None
    else:
        d["scale"] = d["dls"] = d["dp2"] = d["bsum"] = d["chk"] = None
    d["state"] = _state()


def _step_launch(C, d, t, smoothing, momentum):
    C.convnet_head.head_step(d["y2"], d["fslab"], d["fstats"], d["g"], d["b"], d["rm"], d["rv"], d["nbt"], momentum,
                             t["eps"], d["wfc"], d["bfc"], d["logits"], d["p2"], d["idx2"], d["xh2"], d["tgt"], -100,
                             smoothing, d["scale"], d["state"], d["loss"], d["dlog"], d["dls"], d["dp2"], d["bsum"],
                             None, d["chk"])


def _step(C, d, t, tgt, smoothing, scaled, momentum, dtype, Bn, N, chk=True):
    _step_buffers(d, tgt, scaled, dtype, Bn, N, chk)
    _step_launch(C, d, t, smoothing, momentum)


def _check_loss(d, tgt, smoothing, tag):
    """loss[0] and dlog against the reference on the kernel's own logits."""
    s = S32 if smoothing else 0.0
    ref_loss, ref_dlog, A_loss, A_dlog = R.cross_entropy(_cpu(d["logits"]), tgt, -100, s)
    if math.isnan(float(ref_loss)):
        assert math.isnan(float(d["loss"][0])), tag + ": loss must be NaN"
    else:
        _within(d["loss"][0], ref_loss, R.loss_bound(A_loss, fixed_point=True), tag + " loss", "d3 loss")
    _within(d["dlog"], ref_dlog, R.dlog_bound(A_dlog), tag + " dlog", "d3 dlog")
    assert not d["dlog"].cpu()[tgt == -100].any(), tag + ": an ignored row's gradient must be exactly 0"
    assert int(_state()[0]) == 0, tag + ": the loss word was not re-armed"


def _check_backward(d, t, dtype, Bn, N, tag):
    """d3 with a scale: exact identities, dp2 and the per-image BN2 backward sums from the
    kernel's own dls / dp2 / idx2 / xh2, the gradient-check words."""
    loss, dlog = d["loss"].cpu(), d["dlog"].cpu()
    _same(loss[1:], loss[:1] * torch.tensor(SCALE), tag + " loss[1] == loss[0] * scale")
    _same(d["dls"], (dlog * torch.tensor(SCALE)).to(dtype), tag + " dls == (dlog * scale).to(dtype)")
    w_r, dls = R.rounded(t["wfc"], dtype), _cpu(d["dls"])
    ref, A = dls @ w_r, dls.abs() @ w_r.abs()
    _within(d["dp2"], ref, R.dot_bound(N, A, ref, dtype), tag + " dp2", "d3 dp2")
    g = _cpu(d["dp2"]) * ((d["idx2"].cpu() & 4) != 0).double()
    S1, S2, A1, A2 = R.bn_bwd_rows(g, _cpu(d["xh2"]))
    bsum = _cpu(d["bsum"]).reshape(Bn, 2, R.HC)
    _within(bsum[:, 0], S1, R.DOT(R.HP) * R.U32 * A1, tag + " bsum S1 rows", "d3 bsum")
    _within(bsum[:, 1], S2, R.DOT(R.HP) * R.U32 * A2, tag + " bsum S2 rows", "d3 bsum")
    if d["chk"] is not None:
        chk = d["chk"].cpu()
        assert int(chk[0]) == 0 and int(chk[1]) == int(torch.tensor([SCALE]).view(torch.int32)[0]), (tag, chk.tolist())


def _step_cases():
    out = []
    for i, (Bn, N) in enumerate(itertools.product(R.HEAD_B, R.HEAD_N)):
        igns = ["none", "all"] + (["two"] if Bn >= 3 else []) + (["top"] if Bn == 64 else [])
        for j, ign in enumerate(igns):
            out.append((Bn, N, i + j, 0.0 if (i + j) % 2 else 0.1, ign, (i + j) % 3 != 0))
    return out


@pytest.mark.parametrize("Bn,N,i,smoothing,ign,scaled", _step_cases())
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_head_step(C, dtype, Bn, N, i, smoothing, ign, scaled):
    """d1 on head_step, and d3: loss, dlog, dls, dp2, bsum rows, the check words."""
    nrows = _nrows(C, i, Bn, dtype)
    momentum = 0.1 if (i // 2) % 2 == 0 else -1.0
    t = _head_case(Bn, N, nrows)
    d = _head_buffers(t, dtype, Bn, N)
    tgt = _targets(Bn, N, ign, 100 * Bn + N)
    _step(C, d, t, tgt, smoothing, scaled, momentum, dtype, Bn, N)
    torch.cuda.synchronize()
    tag = f"head_step B={Bn} N={N} {_id(dtype)} rows={nrows} s={smoothing} ign={ign} scaled={scaled}"
    _check_forward(d, t, dtype, Bn, N, momentum, tag)
    _check_loss(d, tgt, smoothing, tag)
    if ign == "all":
        assert not d["dlog"].any()
    if scaled:
        _check_backward(d, t, dtype, Bn, N, tag)


@pytest.mark.parametrize("N", R.HEAD_N)
@pytest.mark.parametrize("Bn", R.HEAD_B)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_head_bwd_and_fc_wgrad_exact(C, dtype, Bn, N):
    """d2: integer inputs, every output of head_bwd bit for bit; fc_wgrad's dw / db equal
    head_bwd's on the same inputs."""
    t = R.head_bwd_inputs(Bn, N, R.head_seed(Bn, N))
    hb = R.head_bwd(t["dl"], t["wfc"], t["p2"], t["idx2"], t["xh2"], dtype)
    a = lambda v: v.to(dtype).to(DEV)
    dl, p2, xh2, idx2, wfc = a(t["dl"]), a(t["p2"]), a(t["xh2"]), t["idx2"].to(DEV), t["wfc"].float().to(DEV)
    dw, db, dg, dbe, bsum = _nan((N, R.HK)), _nan((N,)), _nan((R.HC,)), _nan((R.HC,)), _nan((2 * R.HC,))
    dp2 = _nan((Bn, R.HK), dtype)
    C.convnet.head_bwd(dl, wfc, p2, idx2, xh2, dw, db, dg, dbe, bsum, dp2)
    torch.cuda.synchronize()
    tag = f"head_bwd B={Bn} N={N} {_id(dtype)}"
    _same(dp2, hb["dp2"].float().to(dtype), tag + " dp2")
    _same(dw, hb["dW"].float(), tag + " dwfc")
    _same(db, hb["db"].float(), tag + " dbfc")
    _same(dbe, hb["S1"].float(), tag + " dbeta")
    _same(dg, hb["S2"].float(), tag + " dgamma")
    _same(bsum, torch.cat([hb["S1"], hb["S2"]]).float(), tag + " bsum")
    if Bn in (1, 33, 64) and N in (1, 10, 16):
        dw2, db2 = _nan((N, R.HK)), _nan((N,))
        C.convnet.fc_wgrad(dl, p2, dw2, db2)
        torch.cuda.synchronize()
        _same(dw2, dw.cpu(), f"fc_wgrad B={Bn} N={N} {_id(dtype)} dw")
        _same(db2, db.cpu(), f"fc_wgrad B={Bn} N={N} {_id(dtype)} db")


@pytest.mark.parametrize("bad", ["N", "-1"])
def test_head_step_loss_word(C, bad):
    """The loss word over six launches on one state tensor: ordinary, ordinary, a counted row
    with an out-of-range target (NaN), ordinary (the bad-row bits were cleared by the re-arm),
    a row loss above kRowMax in fp32 (NaN), ordinary; state[0] == 0 after every launch."""
    Bn, N = 3, 10
    t = _head_case(Bn, N, 1)
    good = _targets(Bn, N, "none", 7)
    wrong = good.clone()
    wrong[1] = N if bad == "N" else -1

    def launch(dtype, tgt, bias=None, scaled=True):
        d = _head_buffers(t, dtype, Bn, N)
        if bias is not None:
            d["bfc"] = bias.float().to(DEV)
        _step(C, d, t, tgt, 0.1, scaled, 0.1, dtype, Bn, N, chk=False)
        torch.cuda.synchronize()
        assert int(_state()[0]) == 0, "the loss word was not re-armed"
        return d

    def ordinary(dtype, n):
        d = launch(dtype, good)
        _check_loss(d, good, 0.1, f"loss word, launch {n} ({_id(dtype)})")

    ordinary(BF, 1)
    ordinary(F32, 2)
    d = launch(BF, wrong)
    assert math.isnan(float(d["loss"][0])) and math.isnan(float(d["loss"][1])), "out-of-range target: NaN loss"
    ordinary(BF, 4)
    far = t["bfc"].clone()
    far[int(good[0])] = -2e6
    d = launch(F32, good, bias=far)
    assert math.isnan(float(d["loss"][0])), "a row loss above kRowMax: NaN loss"
    ordinary(F32, 6)


def test_head_step_graph_replay(C):
    """d4: one bf16 head_step captured in a graph and replayed three times on the same buffers:
    every output bit for bit the eager one, the loss word at zero."""
    Bn, N = 33, 10
    t = _head_case(Bn, N, 131)
    tgt = _targets(Bn, N, "two", 9)
    keys = ("logits", "p2", "idx2", "xh2", "loss", "dlog", "dls", "dp2", "bsum")
    eager = _head_buffers(t, BF, Bn, N)
    _step(C, eager, t, tgt, 0.1, True, 0.1, BF, Bn, N)
    torch.cuda.synchronize()
    _check_loss(eager, tgt, 0.1, "graph, eager")
    gb = _head_buffers(t, BF, Bn, N)
    _step_buffers(gb, tgt, True, BF, Bn, N)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _step_launch(C, gb, t, 0.1, 0.1)
    for rep in range(3):
        for k in keys:
            gb[k].fill_(0xFF if k == "idx2" else NAN)
        graph.replay()
        torch.cuda.synchronize()
        for k in keys:
            _same(gb[k], eager[k].cpu(), f"replay {rep}: {k}")
        assert int(_state()[0]) == 0, f"replay {rep}: the loss word was not re-armed"
    assert int(gb["nbt"]) == NBT0 + 3


def test_zz_report_ratios():
    """Largest observed error / bound per check (how much room the derived bounds leave)."""
    for k, (v, name) in sorted(RATIOS.items()):
        print(f"\nerror/bound maximum, {k}: {v:.4f} ({name})", end="")
    assert all(v <= 1 for v, _ in RATIOS.values())
