"""Bit-level net under the ResNet-50 kernels (csrc/kernels/conv_igemm.hip, conv_wgrad.hip,
bn_nhwc.hip statistics trees, head.hip CE loss): every sum in them has a fixed order, so for
one compiler the outputs are a pure function of the inputs.  Each case builds seeded CPU
inputs, runs one kernel path and hashes the raw bytes of every output; the digests in
tests/golden/igemm_bits.json were recorded (scripts/record_igemm_bits.py) from the commit
named in its "meta" and a change that claims to leave behaviour alone must reproduce them.

Bits are promised per compiler, not across compilers: the module is skipped only when
torch.version.hip differs from the recorded one.

Notes on the shapes (smallest that still reach the branch):
  * the 4-wave glds kernels (pixel tile 128 / 256, in-launch tree, 3 / 4 LDS stages) are only
    reached with wide_config(0) once Cout % 128 == 0 (the auto rule then picks an 8-wave
    tile, which always defers its tree): those cases set it;
  * the even-pixel ``aux`` add needs even OH / OW: (2,256,14,14,128,1,2,0) has OH = 7, so the
    accumulate case runs at that shape and the aux case at its stride-1 twin (OH = 14);
  * bn_nhwc row blocks = min(ceil(M / (RP * U)), target) with RP = 256 / (64 / VEC) = 32 rows
    per pass and U = 4 for bf16 at C = 64 (chunk_grid): M = 2*56*56 gives 49 row blocks whatever
    the target -- one level (G1 = 128) -- so the two-level runs take M = 6*56*56 (147 row
    blocks at target 256).  _bn_row_blocks() repeats chunk_grid's arithmetic and each case
    asserts the level count it is named for.
"""
import contextlib
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
BF, HF = torch.bfloat16, torch.float16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "igemm_bits.json")


def digest(tensors) -> str:
    """sha256 over (dtype, shape, raw bytes in memory order) of every tensor."""
    h = hashlib.sha256()
    torch.cuda.synchronize()
    for t in tensors:
        t = t.detach()
        if t.dim() == 4 and t.is_contiguous(memory_format=CL) and not t.is_contiguous():
            t = t.permute(0, 2, 3, 1)
        t = t.contiguous().cpu()
        h.update(f"{t.dtype}{tuple(t.shape)}".encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


@contextlib.contextmanager
def knobs(C, **kw):
    """conv_igemm ``*_config`` settings for one case, restored afterwards."""
    K_ = C.conv_igemm
    prev = {}
    try:
        for name, v in kw.items():
            f = getattr(K_, name + "_config")
            prev[name] = f(*v) if isinstance(v, tuple) else f(v)
        yield
    finally:
        for name, p in prev.items():
            f = getattr(K_, name + "_config")
            f(*p) if isinstance(p, (list, tuple)) else f(p)


def _defined(st, K):
    """[sums | sumsq | rows] and the shift copy (the 3 floats between are padding)."""
    return torch.cat([st[:2 * K + 1], st[2 * K + 4:3 * K + 4]])


def _cl(t, dtype):
    return t.to(DEV, dtype).contiguous(memory_format=CL)


def _conv(C, shape, dtype=BF, stats=True, seed=0):
    """conv_fwd (+ fused statistics, launched twice: the tickets re-arm) -> [y, stats, nbt]."""
    N, Cin, H, W, K, R, stride, pad = shape
    g = torch.Generator().manual_seed(1000 + seed + R * 131 + K + H)
    x = _cl(torch.randn(N, Cin, H, W, generator=g), dtype)
    w = _cl(torch.randn(K, Cin, R, R, generator=g) / (Cin * R * R) ** 0.5, dtype)
    OH, OW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    y = torch.zeros(N, K, OH, OW, dtype=dtype, device=DEV).contiguous(memory_format=CL)
    if not stats:
        C.conv_igemm.conv_fwd(x, w, y, stride, pad)
        return [y]
    M = N * OH * OW
    part = torch.zeros(C.conv_igemm.stat_part_len(M, K), device=DEV)
    tk = torch.zeros(C.conv_igemm.stat_tickets_len(M, K), dtype=torch.int32, device=DEV)
    st = torch.zeros(3 * K + 4, device=DEV)
    shift = (torch.randn(K, generator=g) * 0.1).to(DEV)
    nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
    for _ in range(2):
        C.conv_igemm.conv_fwd(x, w, y, stride, pad, part, tk, st, shift, nbt)
    return [y, _defined(st, K), nbt, tk]


def _acc_aux(C, shape, what):
    N, Cin, H, W, K, R, stride, pad = shape
    g = torch.Generator().manual_seed(77 + K + stride)
    x = _cl(torch.randn(N, Cin, H, W, generator=g), BF)
    w = _cl(torch.randn(K, Cin, R, R, generator=g) / (Cin * R * R) ** 0.5, BF)
    OH = (H + 2 * pad - R) // stride + 1
    y = _cl(torch.randn(N, K, OH, OH, generator=g), BF)
    if what == "acc":
        C.conv_igemm.conv_fwd(x, w, y, stride, pad, accumulate=True)
    else:
        aux = _cl(torch.randn(N, K, OH // 2, OH // 2, generator=g), BF)
        C.conv_igemm.conv_fwd(x, w, y, stride, pad, aux=aux)
    return [y]


def _stem(C, N, H):
    from ddp_practice_amd.ops import conv_igemm as I

    g = torch.Generator().manual_seed(5 + H)
    x0 = torch.rand(N, 3, H, H, generator=g)
    w0 = torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5
    conv = torch.nn.Conv2d(3, 64, 7, 2, 3, bias=False)
    with torch.no_grad():
        conv.weight.copy_(w0)
    conv = conv.to(DEV)
    bn = torch.nn.BatchNorm2d(64).to(DEV)
    y, st = I.stem_conv(x0.to(DEV), conv, BF, bn)
    dy = _cl(torch.randn(y.shape, generator=g), BF)
    y.backward(dy)
    return [y, _defined(st, 64), conv.weight.grad]


def _s2t(C, shape):
    from ddp_practice_amd.ops.conv_igemm import dgrad_s2

    N, Cin, H, W, K = shape
    g = torch.Generator().manual_seed(17)
    dy = _cl(torch.randn(N, K, H // 2, W // 2, generator=g), BF)
    wt = _cl(torch.randn(Cin, K, 3, 3, generator=g) / (K * 9) ** 0.5, BF)
    dx = dgrad_s2(dy, wt, (H, W))
    assert dx is not None
    return [dx]


def _dgrad_bn(C, shape, act, R):
    """Inputs as tests/test_conv_igemm_gpu.py test_dgrad_epilogue_bn_backward_sums builds them."""
    from ddp_practice_amd.ops.bn_nhwc import BNTap
    from ddp_practice_amd.ops.conv_igemm import dgrad_bn

    N, K, H, W, Cc = shape
    g = torch.Generator().manual_seed(41 + act + Cc)
    dy = _cl(torch.randn(N, K, H, W, generator=g), BF)
    wt = _cl(torch.randn(Cc, K, R, R, generator=g) / (K * R * R) ** 0.5, BF)
    x = _cl(torch.randn(N, Cc, H, W, generator=g), BF)
    mean = torch.randn(Cc, generator=g) * 0.1
    invstd = torch.rand(Cc, generator=g) + 0.5
    gamma, beta = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g) * 0.3
    bt = BNTap()
    y = acc = None
    if act == 1:
        y = _cl(torch.randn(N, Cc, H, W, generator=g), BF)
        acc = _cl(torch.randn(N, Cc, H, W, generator=g), BF)
    bt.bind_tensors(x, y, act, torch.cat([mean, invstd]).to(DEV), gamma.to(DEV), beta.to(DEV))
    dx = dgrad_bn(dy, wt, bt, acc, R // 2)
    assert dx is not None and bt.matches(dx)
    out, dgamma, dbeta = bt.sums
    return [dx, out, dgamma, dbeta]


def _wgrad_inputs(shape, seed=11):
    N, Cin, H, W, K, R, stride, pad = shape
    g = torch.Generator().manual_seed(seed)
    x = _cl(torch.randn(N, Cin, H, W, generator=g), BF)
    OH = (H + 2 * pad - R) // stride + 1
    dy = _cl(torch.randn(N, K, OH, OH, generator=g), BF)
    return dy, x


def _wgrad(C, shape):
    from ddp_practice_amd.ops.conv_igemm import conv_wgrad

    N, Cin, H, W, K, R, stride, pad = shape
    dy, x = _wgrad_inputs(shape)
    return [conv_wgrad(dy, x, (K, Cin, R, R), stride, pad)]


def _wgrad_batch(C, shapes):
    K_ = C.conv_igemm
    slabs, grads, geos = [], [], []
    for i, shape in enumerate(shapes):
        N, Cin, H, W, K, R, stride, pad = shape
        dy, x = _wgrad_inputs(shape, seed=13 + i)
        OH = dy.shape[2]
        sp = int(K_.wgrad_splits(N * OH * OH, K, Cin, R, R))
        slab = torch.zeros(sp * K * Cin * R * R, device=DEV)
        grad = torch.zeros(K, Cin, R, R, device=DEV)
        geos.append(list(K_.conv_wgrad(dy, x, grad, stride, pad, slab, reduce=False)))
        slabs.append(slab)
        grads.append(grad)
    K_.wgrad_reduce_batch(slabs, grads, geos)
    return grads


# bn_nhwc statistics trees ------------------------------------------------------------------
BN_G1, BN_MAXGR, BN_U, BN_THR = 128, 1024, 4, 256  # csrc/kernels/bn_nhwc.hip


def _bn_row_blocks(M, Cc, target, vec=8):
    """Row blocks of the statistics kernels (bn_nhwc.hip chunk_grid / stats_grid; bf16: vec 8)."""
    cc = 64
    while cc > vec and not (Cc <= cc or Cc % cc == 0):
        cc //= 2
    ccw = Cc if Cc <= cc else cc
    rp = BN_THR // (ccw // vec)
    gc = Cc // ccw
    by_rows = max(1, (M + rp * BN_U - 1) // (rp * BN_U))
    tgt = target if target > 0 else (128 if M * Cc * 2 < (64 << 20) else 256)
    return min(by_rows, max(1, (tgt + gc - 1) // gc), BN_MAXGR)


def _bn_stats(C, n_img, target, levels, handoff, which):
    B = C.bn_nhwc
    Cc, M = 64, n_img * 56 * 56
    gr = _bn_row_blocks(M, Cc, target)
    assert (gr <= BN_G1) == (levels == 1), (gr, levels)
    g = torch.Generator().manual_seed(61 + n_img)
    x = _cl(torch.randn(n_img, Cc, 56, 56, generator=g), BF)
    part = torch.zeros(int(B.MAX_PARTIAL_ROWS) * 2 * Cc, device=DEV)
    tk = torch.zeros(int(B.MAX_TICKETS), dtype=torch.int32, device=DEV)
    B.set_grid_targets(target, 512, 1024)
    B.set_handoff(handoff)
    try:
        if which == "fwd":
            shift = (torch.randn(Cc, generator=g) * 0.1).to(DEV)
            st = torch.zeros(3 * Cc + 4, device=DEV)
            nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
            for _ in range(2):
                B.fwd_stats(x, Cc, shift, part, tk, st, nbt)
            return [_defined(st, Cc), nbt, tk]
        dy = _cl(torch.randn(n_img, Cc, 56, 56, generator=g), BF)
        y = _cl(torch.randn(n_img, Cc, 56, 56, generator=g), BF)
        save = torch.cat([torch.randn(Cc, generator=g) * 0.1, torch.rand(Cc, generator=g) + 0.5]).to(DEV)
        gamma, beta = torch.randn(Cc, generator=g).to(DEV), (torch.randn(Cc, generator=g) * 0.3).to(DEV)
        out, dgamma, dbeta = torch.zeros(2 * Cc, device=DEV), torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV)
        for _ in range(2):
            B.bwd_stats(dy, y, x, Cc, 1, save, gamma, beta, part, tk, out, dgamma, dbeta)
        return [out, dgamma, dbeta, tk]
    finally:
        B.set_grid_targets(0, 512, 1024)
        B.set_handoff(1)


def _ce(C, B_, N_):
    """CE loss over more than one workgroup (B > 64: ce_fwd_rows_kernel, 4 rows each)."""
    g = torch.Generator().manual_seed(71)
    lg = torch.randn(B_, N_, generator=g).to(DEV, BF)
    tgt = torch.randint(0, N_, (B_,), generator=g).to(DEV)
    tgt[3] = -100
    buf = torch.zeros(2, device=DEV)
    dlog = torch.zeros(B_, N_, device=DEV)
    dls = torch.zeros_like(lg)
    scale = torch.full((1,), 128.0, device=DEV)
    for _ in range(2):  # the ticket re-arms itself
        C.head.ce_fwd(lg, tgt, buf, dlog, -100, 0.1, scale, dls)
    return [buf, dlog, dls]


# the case list ----------------------------------------------------------------------------
CASES = {}


def _case(cid, fn, **kn):
    assert cid not in CASES, cid

    def run(C):
        with knobs(C, **kn):
            return digest(fn(C))

    CASES[cid] = run


def _d(v):
    return "auto" if v is None else str(v).replace("-", "m")


GEN3 = (2, 64, 14, 14, 64, 3, 1, 1)
for dt, dn in ((BF, "bf16"), (HF, "f16")):
    for df in (0, -1):
        _case(f"general_3x3_{dn}_defer{_d(df)}", lambda C, dt=dt: _conv(C, GEN3, dt), g1x1=(0, -1, -1), stat_defer=df)
for df in (0, -1):
    _case(f"general_3x3_s2_bn128_defer{_d(df)}", lambda C: _conv(C, (2, 128, 15, 15, 128, 3, 2, 1)),
          g1x1=(0, -1, -1), stat_defer=df)
for dt, dn in ((BF, "bf16"), (HF, "f16")):
    for bp in (128, 256):
        for df in (0, -1):
            _case(f"glds_1x1_ragged_{dn}_bp{bp}_defer{_d(df)}", lambda C, dt=dt: _conv(C, (3, 64, 7, 7, 256, 1, 1, 0), dt),
                  g1x1=(1, bp, -1), stat_defer=df, wide=0)
_case("glds_1x1_bn64_ragged", lambda C: _conv(C, (2, 128, 9, 9, 64, 1, 1, 0)))
_case("tree_one_level_16_rows", lambda C: _conv(C, (8, 64, 56, 56, 64, 1, 1, 0)), stat_defer=0)
_case("tree_one_level_64_rows", lambda C: _conv(C, (12, 64, 56, 56, 64, 1, 1, 0)), stat_defer=0)
for df in (0, -1):
    _case(f"tree_two_level_defer{_d(df)}", lambda C: _conv(C, (48, 64, 56, 56, 64, 1, 1, 0)), stat_defer=df)
_case("glds_3x3", lambda C: _conv(C, GEN3), g3x3=1)
for R, pad in ((1, 0), (3, 1)):
    for wm in (0, 2, 3, 4, 1):
        _case(f"wide_{R}x{R}_mode{'auto' if wm == 1 else wm}", lambda C, R=R, pad=pad: _conv(C, (2, 256, 14, 14, 256, R, 1, pad)),
              wide=wm)
for ns in (3, 4):
    _case(f"glds_stages{ns}", lambda C: _conv(C, (2, 128, 14, 14, 128, 1, 1, 0)), glds=ns, wide=0)
for on in (1, 0):
    kn = "glds" if on else "general"
    _case(f"accumulate_{kn}", lambda C: _acc_aux(C, (2, 256, 14, 14, 128, 1, 2, 0), "acc"), g1x1=(on, -1, -1), wide=0)
    _case(f"aux_{kn}", lambda C: _acc_aux(C, (2, 256, 14, 14, 128, 1, 1, 0), "aux"), g1x1=(on, -1, -1), wide=0)
_case("stem_fwd_wgrad", lambda C: _stem(C, 3, 23))
_case("s2t_dgrad", lambda C: _s2t(C, (3, 64, 10, 10, 128)))
for act, R in ((1, 1), (2, 1), (2, 3)):
    _case(f"dgrad_bn_act{act}_R{R}", lambda C, act=act, R=R: _dgrad_bn(C, (3, 64, 7, 7, 256), act, R))
    _case(f"dgrad_bn_act{act}_R{R}_wide0", lambda C, act=act, R=R: _dgrad_bn(C, (3, 64, 7, 7, 256), act, R), wide=0)
WG1, WG3 = (3, 256, 7, 7, 128, 1, 1, 0), (2, 64, 14, 14, 64, 3, 1, 1)
for sh, sn in ((WG1, "1x1"), (WG3, "3x3")):
    for gl in (0, 1, 2):
        for wv in (4, 8):
            _case(f"wgrad_{sn}_glds{gl}_waves{wv}", lambda C, sh=sh: _wgrad(C, sh), wgrad=gl, wgrad_waves=wv,
                  wgrad_fixup=0)
_case("wgrad_1x1_fixup8", lambda C: _wgrad(C, WG1), wgrad=2, wgrad_waves=8, wgrad_fixup=8)
_case("wgrad_reduce_batch", lambda C: _wgrad_batch(C, (WG1, WG3)), wgrad_fixup=0)
for which in ("fwd", "bwd"):
    for n_img, target, levels in ((2, 0, 1), (6, 256, 2)):
        for ho in (1, 0):
            _case(f"bn_{which}_stats_levels{levels}_handoff{ho}",
                  lambda C, a=(n_img, target, levels, ho, which): _bn_stats(C, *a))
_case("ce_loss_many_workgroups", lambda C: _ce(C, 300, 10))


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("cid", list(CASES))
def test_bits_match_recorded(C, cid):
    gold = _golden()
    if gold["meta"]["torch_version_hip"] != torch.version.hip:
        pytest.skip(f"digests recorded with HIP {gold['meta']['torch_version_hip']}, this is {torch.version.hip}")
    assert cid in gold["cases"], f"{cid}: no recorded digest (scripts/record_igemm_bits.py)"
    assert CASES[cid](C) == gold["cases"][cid]
