"""csrc/kernels/conv_igemm.hip and conv_wgrad.hip against tests/_conv_ref.py, EXACTLY.

Integer operands keep every fp32 partial sum an exact integer (tests/_conv_ref.py), so the
float64 CPU reference gives the expected output bit for bit, whatever the tile, the order
or the pixel split: outputs, fused BN statistics, BN backward sums and fp32 weight
gradients are compared with torch.equal.  tests/_conv_cases.py has one case per kernel
variant and edge; each case also asserts the variant that ran (conv_igemm.last_launch())
and, for weight gradients, the pixel split it was designed for, so that a retuned
heuristic fails a case instead of hollowing it out.
"""
import pytest
import torch

from . import _conv_cases as T
from . import _conv_ref as R
from .test_igemm_bits_gpu import knobs

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last


def _cl(t, dtype):
    """float64 CPU integers -> the storage dtype on the device, channels_last (exact)."""
    out = t.to(R.DT[dtype])
    assert torch.equal(out.double(), t), "input not representable"
    return out.to(DEV).contiguous(memory_format=CL)


def _f(t):
    out = t.float()
    assert torch.equal(out.double(), t)
    return out.to(DEV)


def _same(got, exp, what):
    got, exp = got.detach().cpu(), exp.detach().cpu()
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, exp.dtype, got.shape, exp.shape)
    if not torch.equal(got, exp):
        bad = (got != exp).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ, first at {i}: "
                             f"got {got[i].item()}, expected {exp[i].item()}; last at {tuple(bad[-1].tolist())}")


def _launched(C, case, expect=None):
    got = [(f, tuple(v), d) for f, v, d in C.conv_igemm.last_launch()]
    expect = case.expect if expect is None else expect
    want = [(f, tuple(v), "f32" if f.startswith("stat_") else case.dtype) for f, v in expect]
    assert got == want, (case.name, got, want)


def _check_stats(st, exp, K, shift):
    _same(st[:2 * K + 1], exp.float(), "statistics [sum | sumsq | rows]")
    _same(st[2 * K + 4:3 * K + 4], shift.float(), "shift copy")


def _run_fwd(C, case, inp, exp):
    K_ = C.conv_igemm
    N, Cin, H, W, K, Rr, stride, pad = case.shape
    dt = case.dtype
    x, w = _cl(inp["x"], dt), _cl(inp["w"], dt)
    OH, OW = R.out_hw(H, W, Rr, stride, pad)
    if case.op == "fwd+stats":
        M = N * OH * OW
        y = torch.zeros(N, K, OH, OW, dtype=R.DT[dt], device=DEV).contiguous(memory_format=CL)
        part = torch.zeros(K_.stat_part_len(M, K), device=DEV)
        tk = torch.zeros(K_.stat_tickets_len(M, K), dtype=torch.int32, device=DEV)
        st = torch.zeros(3 * K + 4, device=DEV)
        shift = _f(inp["shift"])
        nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
        for _ in range(2):  # the tickets re-arm themselves
            K_.conv_fwd(x, w, y, stride, pad, part, tk, st, shift, nbt)
        _launched(C, case)
        _same(y, exp["y"], "y")
        _check_stats(st, exp["stats"], K, inp["shift"])
        assert int(tk.abs().sum()) == 0 and int(nbt) == 2
        return
    if case.op == "acc":
        y = _cl(inp["old"], dt)
        K_.conv_fwd(x, w, y, stride, pad, accumulate=True)
    elif case.op == "aux":
        y = torch.zeros(N, K, OH, OW, dtype=R.DT[dt], device=DEV).contiguous(memory_format=CL)
        K_.conv_fwd(x, w, y, stride, pad, aux=_cl(inp["aux"], dt))
    else:
        y = torch.zeros(N, K, OH, OW, dtype=R.DT[dt], device=DEV).contiguous(memory_format=CL)
        K_.conv_fwd(x, w, y, stride, pad)
    _launched(C, case)
    _same(y, exp["y"], "y")


def _run_s2t(C, case, inp, exp):
    from ddp_practice_amd.ops.conv_igemm import dgrad_s2

    dy = _cl(inp["dy"], case.dtype)
    wt = _cl(inp["w"].flip(2, 3).transpose(0, 1), case.dtype)
    dx = dgrad_s2(dy, wt, (2 * dy.shape[2], 2 * dy.shape[3]))
    assert dx is not None
    _launched(C, case)
    _same(dx, exp["y"], "dx")


def _run_stem(C, case, inp, exp):
    from ddp_practice_amd.ops import conv_igemm as I

    N, H, W, K = case.shape
    conv = torch.nn.Conv2d(3, K, 7, 2, 3, bias=False)
    with torch.no_grad():
        conv.weight.copy_(inp["w"].float())
    conv = conv.to(DEV)
    bn = torch.nn.BatchNorm2d(K).to(DEV)
    with torch.no_grad():
        bn.running_mean.copy_(_f(inp["shift"]))
    x0 = _f(inp["x"])
    assert I.stem_usable(x0, conv, R.DT[case.dtype])
    for _ in range(2):
        y, st = I.stem_conv(x0, conv, R.DT[case.dtype], bn)
    _launched(C, case)
    assert y.is_contiguous(memory_format=CL)
    _same(y, exp["y"], "y")
    _check_stats(st, exp["stats"], K, inp["shift"])
    OH, OW = y.shape[2:]
    tk = I._StatWS.get(y.device, N * OH * OW, K)[1]
    assert int(tk.abs().sum()) == 0 and int(bn.num_batches_tracked) == 2
    y.backward(_cl(inp["dy"], case.dtype))
    _launched(C, case, [case.extra["wgrad"]])
    _same(conv.weight.grad, exp["dw"], "dW")


def _run_dgrad_bn(C, case, inp, exp):
    from ddp_practice_amd.ops.bn_nhwc import BNTap
    from ddp_practice_amd.ops.conv_igemm import _StatWS, dgrad_bn

    dt, act, Rr = case.dtype, case.extra["act"], case.extra["R"]
    N, K, H, W, Cc = case.shape
    dy, wt, x = _cl(inp["dy"], dt), _cl(inp["wt"], dt), _cl(inp["x"], dt)
    y = _cl(inp["y"], dt) if act == 1 else None
    acc = _cl(inp["acc"], dt) if act == 1 else None
    bt = BNTap()
    bt.bind_tensors(x, y, act, torch.cat([_f(inp["mean"]), _f(inp["invstd"])]), _f(inp["gamma"]), _f(inp["beta"]))
    dx = dgrad_bn(dy, wt, bt, acc, Rr // 2)
    assert dx is not None and bt.matches(dx)
    _launched(C, case)
    _same(dx, exp["y"], "dx")
    out, dgamma, dbeta = bt.sums
    _same(out[:Cc], exp["s1"].float(), "S1 = sum dz")
    _same(out[Cc:], exp["s2"].float(), "S2 = sum dz * xhat")
    assert torch.equal(dbeta, out[:Cc]) and torch.equal(dgamma, out[Cc:])
    assert int(_StatWS.get(dx.device, N * H * W, Cc)[1].abs().sum()) == 0


def _split_geometry(C, shape):
    """(splits, pixels per split, pixels in the last split): conv_igemm.wgrad_splits and
    conv_wgrad's pps = ceil(ceil(M / sp) / 64) * 64."""
    N, Cin, H, W, K, Rr, stride, pad = shape
    OH, OW = R.out_hw(H, W, Rr, stride, pad)
    M = N * OH * OW
    sp = int(C.conv_igemm.wgrad_splits(M, K, Cin, Rr, Rr))
    pps = ((M + sp - 1) // sp + 63) // 64 * 64
    return sp, pps, max(0, M - (sp - 1) * pps)


def _wgrad_raw(C, shape, inp, dtype, reduce=True):
    K_ = C.conv_igemm
    N, Cin, H, W, K, Rr, stride, pad = shape
    sp = _split_geometry(C, shape)[0]
    dy, x = _cl(inp["dy"], dtype), _cl(inp["x"], dtype)
    # NaN-filled: a partial tile or gradient element nobody wrote shows
    slab = torch.full((sp * K * Cin * Rr * Rr,), float("nan"), device=DEV)
    grad = torch.full((K, Cin, Rr, Rr), float("nan"), device=DEV)
    geo = K_.conv_wgrad(dy, x, grad, stride, pad, slab, reduce=reduce)
    return grad, slab, list(geo)


def _run_wgrad(C, case, inp, exp):
    assert _split_geometry(C, case.shape) == tuple(case.splits), (case.name, _split_geometry(C, case.shape))
    for _ in range(2):  # the in-launch reduction's tickets re-arm themselves
        grad, _, _ = _wgrad_raw(C, case.shape, inp, case.dtype)
        _launched(C, case)
        _same(grad, exp["dw"], "dW")


def _run_wgrad_batch(C, case, inps, exps):
    slabs, grads, geos = [], [], []
    for shape, inp in zip(case.shape, inps):
        grad, slab, geo = _wgrad_raw(C, shape, inp, case.dtype, reduce=False)
        slabs.append(slab), grads.append(grad), geos.append(geo)
    C.conv_igemm.wgrad_reduce_batch(slabs, grads, geos)
    for grad, exp in zip(grads, exps):
        _same(grad, exp["dw"], "dW")


RUN = {"fwd": _run_fwd, "fwd+stats": _run_fwd, "acc": _run_fwd, "aux": _run_fwd, "s2t": _run_s2t, "stem": _run_stem,
       "dgrad_bn": _run_dgrad_bn, "wgrad": _run_wgrad, "wgrad_batch": _run_wgrad_batch}


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_exact(C, name):
    case = T.BY_NAME[name]
    inp, exp, pre = R.build(case)
    R.check_preconditions(case, pre)
    with knobs(C, **case.knobs):
        RUN[case.op](C, case, inp, exp)


def test_every_variant_has_an_exact_case(C):
    """The variants the table claims to reach (each claim is asserted by its case through
    last_launch()) == the variants instantiated, read from the dispatch tuples themselves."""
    built = {f: {tuple(v) for v in vs} for f, vs in C.conv_igemm.variants().items()}
    assert sum(len(v) for v in built.values()) > 0
    claimed = T.expected_variants()
    for fam in sorted(set(built) | set(claimed)):
        missing = built.get(fam, set()) - claimed.get(fam, set())
        unknown = claimed.get(fam, set()) - built.get(fam, set())
        assert not missing and not unknown, f"{fam}: no exact case for {sorted(missing)}, not instantiated {sorted(unknown)}"


@pytest.mark.parametrize("wn", ["1x1_m189", "3x3_two_splits_ragged", "3x3_several_splits", "3x3_empty_last_split"])
def test_wgrad_paths_agree_and_replay(C, wn):
    """Register-staged, LDS-DMA 4- and 8-wave, in-launch fixup (twice, and under graph
    replay) and the batched reduction: all equal the integer reference, hence each other."""
    from ddp_practice_amd.ops.conv_igemm import conv_wgrad

    case = T.BY_NAME[f"wgrad_{wn}_fixup-bf16"]
    inp, exp, pre = R.build(case)
    R.check_preconditions(case, pre)
    N, Cin, H, W, K, Rr, stride, pad = case.shape
    dy, x = _cl(inp["dy"], "bf16"), _cl(inp["x"], "bf16")
    for pn, kn, _ in T.WPATHS:
        with knobs(C, **kn):
            for _ in range(2):
                _same(conv_wgrad(dy, x, (K, Cin, Rr, Rr), stride, pad), exp["dw"], f"dW ({pn})")
    with knobs(C, wgrad_fixup=0):
        grad, slab, geo = _wgrad_raw(C, case.shape, inp, "bf16", reduce=False)
        C.conv_igemm.wgrad_reduce_batch([slab], [grad], [geo])
        _same(grad, exp["dw"], "dW (batched reduce)")
    with knobs(C, **case.knobs):
        conv_wgrad(dy, x, (K, Cin, Rr, Rr), stride, pad)  # (the fixup tickets are allocated outside a capture)
        out = torch.empty(K, Cin, Rr, Rr, device=DEV)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            out.copy_(conv_wgrad(dy, x, (K, Cin, Rr, Rr), stride, pad))
        for _ in range(2):
            out.fill_(float("nan"))
            gr.replay()
            torch.cuda.synchronize()
            _same(out, exp["dw"], "dW (graph replay)")


@pytest.mark.parametrize("shape", [(2, 64, 14, 18, 128, 3, 1, 1), (2, 128, 16, 12, 64, 3, 2, 1), (3, 128, 7, 9, 64, 1, 1, 0),
                                   (2, 64, 14, 10, 128, 1, 2, 0)])
def test_ops_level_exact(C, shape):
    """ops.conv_nhwc / ops.conv1x1 forward and backward with integer fp32 master weights
    packed by WeightPack.run() (pack_weights_kernel): the packed forward filter == w.to(dtype)
    and the data-gradient filter == its flipped transpose bit for bit, and y, x.grad, w.grad
    == the reference."""
    from ddp_practice_amd.ops.conv1x1 import conv1x1
    from ddp_practice_amd.ops.conv_igemm import WeightPack
    from ddp_practice_amd.ops.conv_nhwc import conv_nhwc

    N, Cin, H, W, K, Rr, stride, pad = shape
    g = R.gen("ops", shape)
    OH, OW = R.out_hw(H, W, Rr, stride, pad)
    x0, w0 = R.ints((N, Cin, H, W), (-2, -1, 1, 2), g), R.ints((K, Cin, Rr, Rr), (-1, 1), g)
    dy0 = R.ints((N, K, OH, OW), (-1, 1), g)
    y64 = R.conv(x0, w0, stride, pad)
    dx64 = R.dgrad(dy0, w0, x0.shape, stride, pad)
    dw64 = R.wgrad(dy0, x0, w0.shape, stride, pad)
    assert max(float(t.abs().max()) for t in (y64, dx64)) <= R.INT_EXACT["bf16"]
    assert N * OH * OW * 2 < R.F32_EXACT and Rr * Rr * max(Cin, K) * 2 < R.F32_EXACT
    mod = torch.nn.Conv2d(Cin, K, Rr, stride, pad, bias=False)
    with torch.no_grad():
        mod.weight.copy_(w0.float())
    mod = mod.to(DEV)
    packed = WeightPack([(mod, True)], torch.bfloat16).run()[id(mod)]
    wbf = w0.to(torch.bfloat16)
    _same(packed[0], wbf, "packed forward filter")
    assert packed[0].is_contiguous(memory_format=CL) and packed[1].is_contiguous(memory_format=CL)
    _same(packed[1], wbf.flip(2, 3).transpose(0, 1), "packed data-gradient filter")
    for pk in (packed, None):  # the packed filters, and the op's own cast / flip / transpose
        mod.weight.grad = None
        x = _cl(x0, "bf16").requires_grad_()
        if Rr == 1:
            y = conv1x1(x, mod.weight, stride, torch.bfloat16, None, None, pk)
        else:
            y = conv_nhwc(x, mod.weight, (stride, stride), (pad, pad), torch.bfloat16, None, pk)
        y.backward(_cl(dy0, "bf16"))
        _same(y, R.store(y64, "bf16"), "y")
        _same(x.grad.contiguous(), R.store(dx64, "bf16"), "x.grad")
        _same(mod.weight.grad, dw64.float(), "w.grad")
