"""The conv2 data gradient at 2 and at 4 workgroups per image (csrc/kernels/convnet_fused.hip
dgrad_split): the BN1 partial-sum slab has one row per image quarter, built by the same
operations at either split (csrc/kernels/conv5x5.h BwdEpi, tests/_dgrad_rows.py), so a launch
with an in-kernel SyncBN site (2) and one without (4) hand the consumer the same bits.

convnet.conv2_bwd (merged launch) and convnet.conv2_dgrad (stand-alone) are called with
split=2 and split=4 on the same inputs, bf16 / fp16, B = 1, 2, 3, 33:

  * every output is bitwise equal between the splits (integer views; NaN-prefilled, so every
    element is written; a guard region behind each buffer keeps its bits);
  * on integer-valued inputs (generators of tests/_convblock_ref.py: every sum below 2^24 in
    units of 1/2, so fp32 arithmetic is exact in any order) each of the 4 B rows equals the
    exact per-quarter sums of the reference, and dp1 the exact data gradient rounded once;
  * reruns are bitwise equal, also right after a launch with large values (a partial left in
    LDS by an earlier workgroup must not reach a row: a 2-way workgroup's second quarter has
    3 or 4 m-tiles, the slot past them is never written by that launch);
  * split=4 on a launch with an exchange site, split=2 in fp32 and any other split are refused;
  * one step (bf16, fp16) of the plain ConvNet and one of DDP + SyncBN at world 1 through the in-kernel
    sites give bitwise equal BN1 gradients (the consumers of the slab).
"""
import copy
import functools
import os
import re

import pytest
import torch

from . import _convblock_ref as R
from . import _dgrad_rows as Q

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = R.EPS32
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
BATCHES = [1, 2, 3, 33]
GUARD = 256
NCLS = 10
FCK = 32 * 49
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def _pack_dgrad(w2, dtype):
    """[32][16][5][5] -> the data-gradient LDS tile [16][808], k = (24 - tap) * 32 + co."""
    t = torch.zeros(16, 808, dtype=torch.float64)
    t[:, :800] = w2.reshape(32, 16, 25).flip(2).permute(1, 2, 0).reshape(16, 800)
    return t.reshape(-1).to(dtype)


# ------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _int_case(B, dtype, seed=0):
    """Integer-valued inputs (CPU, never modified) and the exact reference.  BN2 backward with
    all-zero sums (k1 = k2 = 0), statistics [0 | n (1 - eps) | n | 0] (invstd = 1 to a few
    fp32 ulp) and gamma in {+-1, +-2, +-1/2}: dy = gamma * g is a multiple of 1/2 of magnitude
    <= 6, exact once rounded to bf16 / fp16 (as _convblock_ref.conv1_wgrad_int for layer 1)."""
    seed = 7000 + 100 * B + 10 * DTYPES.index(dtype) + seed
    bc = R.bwd_case(2, B, seed, "int")  # dp2 in [-3, 3], p in {0, 1, 2}, idx in 0..3, y2 in [-4, 4]
    w2 = R.int_dgrad(B, seed + 1)["w"]  # {-1, 0, 1}
    g = R._gen(seed + 2)
    gamma = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5, -0.5], dtype=torch.float64)[torch.randint(0, 6, (32,), generator=g)]
    n = B * 196
    z = torch.zeros(32, dtype=torch.float64)
    fstats2 = R.fstats_of(z, R.rounded(torch.full((32,), n * (1.0 - EPS), dtype=torch.float64), torch.float32), n, z)
    idx2 = (bc["idx"] | (4 * (bc["p"] > 0)).to(torch.uint8)).contiguous()
    dy = R.route(bc["dp"], bc["p"], bc["idx"]) * gamma.view(1, -1, 1, 1)
    dp1, A = R.conv_dgrad(dy, w2)
    assert 2 * A.max().item() < R.EXACT
    idx1 = torch.randint(0, 8, (B, 16, 14, 14), generator=g).to(torch.uint8)
    xh1 = torch.randint(-2, 3, (B, 16, 14, 14), generator=g).double()
    p1 = torch.randint(0, 3, (B, 16, 14, 14), generator=g).double()
    dp1r = R.rounded(dp1, dtype)  # the stored gradient: the exact value rounded once
    g1 = dp1r * ((idx1 & 4) != 0).double()
    rows = Q.quarter_rows(g1, xh1)
    assert 2 * Q.quarter_rows(g1.abs(), xh1.abs()).max().item() < R.EXACT
    return dict(B=B, dtype=dtype, y2=bc["y"].to(dtype), dp2=bc["dp"].to(dtype), idx2=idx2, fstats2=fstats2.float(),
                gsum2=torch.zeros(B, 64), gamma=gamma.float(), idx1=idx1, xh1=xh1.to(dtype), p1=p1.to(dtype),
                wpk_d=_pack_dgrad(w2, dtype), dls=torch.randint(-2, 3, (B, NCLS), generator=g).to(dtype),
                p2=torch.randint(0, 3, (B, FCK), generator=g).to(dtype), dp1_ref=dp1r.to(dtype), rows_ref=rows.float())


@functools.lru_cache(maxsize=None)
def _float_case(B, dtype, seed=0, scale=1.0):
    """Random normal inputs (CPU, never modified): fp32 sums whose bits depend on their order."""
    g = torch.Generator().manual_seed(9000 + 100 * B + 10 * DTYPES.index(dtype) + seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    y2 = (rn(B, 32, 14, 14) * scale).to(dtype)
    yd = y2.double()
    shift = yd.mean((0, 2, 3)).float()
    d = yd - shift.double().view(1, -1, 1, 1)
    fstats2 = torch.cat([d.sum((0, 2, 3)), (d * d).sum((0, 2, 3)), torch.tensor([float(B * 196)], dtype=torch.float64),
                         shift.double()]).float()
    w2 = rn(32, 16, 5, 5).double() * 0.05
    return dict(B=B, dtype=dtype, y2=y2, dp2=(rn(B, 32, 7, 7) * scale).to(dtype),
                idx2=torch.randint(0, 8, (B, 32, 7, 7), generator=g, dtype=torch.uint8), fstats2=fstats2,
                gsum2=(rn(B, 64) * scale).contiguous(), gamma=torch.rand(32, generator=g) + 0.5,
                idx1=torch.randint(0, 8, (B, 16, 14, 14), generator=g, dtype=torch.uint8),
                xh1=rn(B, 16, 14, 14).to(dtype), p1=rn(B, 16, 14, 14).clamp_(min=0).to(dtype),
                wpk_d=_pack_dgrad(w2, dtype), dls=(rn(B, NCLS) * scale).to(dtype),
                p2=rn(B, FCK).clamp_(min=0).to(dtype))


# ------------------------------------------------------------------------------ launches
class _Out:
    """An output buffer prefilled with NaN, with GUARD more elements behind it."""

    def __init__(self, shape, dtype):
        self.n = int(torch.Size(shape).numel())
        self.whole = torch.full((self.n + GUARD,), float("nan"), device=DEV, dtype=dtype)
        self.t = self.whole[:self.n].view(shape)
        self.guard0 = self.whole[self.n:].view(BITS[dtype]).clone()

    def bits(self):
        """The written region as integers (CPU); asserts the guard kept its bits."""
        assert torch.equal(self.whole[self.n:].view(BITS[self.whole.dtype]), self.guard0), "guard region written"
        return self.t.reshape(-1).view(BITS[self.whole.dtype]).cpu()


def _run(C, c, split, merged=True):
    """conv2_bwd (with BN2's gradients and the fc role) or conv2_dgrad at `split`: the outputs
    as integer views, by name."""
    cn = C.convnet
    B, dt = c["B"], c["dtype"]
    dev = lambda k: c[k].to(DEV)  # noqa: E731
    f32 = torch.float32
    assert cn.dgrad2_rows(B, False) == 4 * B
    o = dict(dp1=_Out((B, 16, 14, 14), dt), bslab1=_Out((4 * B * 32,), f32))
    if merged:
        o.update(wslab2=_Out((cn.wgrad_bn_rows(2, B) * (32 * 400 + 32),), f32), dg2=_Out((32,), f32),
                 dbe2=_Out((32,), f32), fc_dw=_Out((NCLS * FCK,), f32), fc_db=_Out((NCLS,), f32))
        cn.conv2_bwd(dev("wpk_d"), dev("y2"), dev("dp2"), dev("idx2"), dev("fstats2"), dev("gsum2"), dev("gamma"), EPS,
                     o["dp1"].t, dev("idx1"), dev("xh1"), o["bslab1"].t, dev("p1"), o["wslab2"].t, None, None,
                     o["dg2"].t, o["dbe2"].t, dev("dls"), dev("p2"), o["fc_dw"].t, o["fc_db"].t, None, split)
    else:
        cn.conv2_dgrad(dev("wpk_d"), dev("y2"), dev("dp2"), dev("idx2"), dev("fstats2"), dev("gsum2"), dev("gamma"), EPS,
                       o["dp1"].t, dev("idx1"), dev("xh1"), o["bslab1"].t, None, split)
    torch.cuda.synchronize()
    res = {k: v.bits() for k, v in o.items()}
    for k, v in o.items():
        assert not bool(torch.isnan(v.t.float()).any()), f"{k}: element not written"
    return res


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        ne = (a[k] != b[k]).nonzero()
        assert ne.numel() == 0, f"{what}: {k} differs at {ne[:4].flatten().tolist()} ({ne.shape[0]} elements)"


FORMS = [True, False]
FORM_IDS = ["conv2_bwd", "conv2_dgrad"]


# ------------------------------------------------------------------------------ tests
def test_row_and_workgroup_counts(C):
    cn = C.convnet
    for B in BATCHES:
        assert cn.dgrad2_rows(B, False) == cn.dgrad2_rows(B, True) == cn.dgrad2_rows(B) == 4 * B
        assert cn.dgrad2_wgs(B, False, False) == 4 * B and cn.dgrad2_wgs(B, False, True) == 2 * B
        assert cn.dgrad2_wgs(B, True, False) == cn.dgrad2_wgs(B, True, True) == 4 * B


@pytest.mark.parametrize("merged", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B", BATCHES)
def test_splits_agree_bitwise(C, B, dtype, merged):
    """dp1, all 4 B rows of bslab1, wslab2, dg2 / dbe2 and the fc gradients at split 2 == at
    split 4, on random inputs (order-sensitive fp32 sums) and on the integer ones; the default
    rule (no site: 4) is one of the two."""
    for c in (_float_case(B, dtype), _int_case(B, dtype)):
        a2, a4 = _run(C, c, 2, merged), _run(C, c, 4, merged)
        _same(a2, a4, "split 2 vs 4")
        _same(_run(C, c, 0, merged), a4, "split by rule vs 4")


@pytest.mark.parametrize("split", [2, 4])
@pytest.mark.parametrize("merged", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B", BATCHES)
def test_rows_are_the_exact_quarter_sums(C, B, dtype, merged, split):
    """Integer inputs: row 4 b + k == [S1 | S2] over the pixels of quarter k of image b, exactly,
    and dp1 == the exact data gradient rounded once -- the rows themselves, not their total."""
    c = _int_case(B, dtype)
    o = _run(C, c, split, merged)
    rows = o["bslab1"].view(torch.float32).view(4 * B, 32)
    ne = (rows != c["rows_ref"]).nonzero()
    assert ne.numel() == 0, (ne[:4].tolist(), rows[ne[0, 0]], c["rows_ref"][ne[0, 0]])
    assert torch.equal(o["dp1"], c["dp1_ref"].reshape(-1).view(BITS[dtype]))


@pytest.mark.parametrize("split", [2, 4])
@pytest.mark.parametrize("merged", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B", BATCHES)
def test_reruns_agree_and_no_stale_partials(C, B, dtype, merged, split):
    """The same inputs twice: bitwise equal.  Then a launch with large values, and the inputs
    again: still the same bits, and on the integer case still the exact rows -- a partial or a
    tile left in LDS by the launch before must not reach an output."""
    big = _float_case(B, dtype, seed=1, scale=64.0)
    for c in (_float_case(B, dtype, seed=2), _int_case(B, dtype, seed=3)):
        a = _run(C, c, split, merged)
        _same(a, _run(C, c, split, merged), "rerun")
        _run(C, big, split, merged)
        b = _run(C, c, split, merged)
        _same(a, b, "after a launch with large values")
        if "rows_ref" in c:
            assert torch.equal(b["bslab1"].view(torch.float32).view(-1, 32), c["rows_ref"])


@pytest.fixture(scope="module")
def forced_w1(C):
    """DDP at world 1 with every collective forced (as tests/test_dist_gpu.py): the
    communicator carries the xGMI engine whose sites the fused ConvNet launches use."""
    import ddp_practice_amd.distributed as dist
    from ddp_practice_amd.parallel import comm as comm_mod

    from ._dist import free_port

    env = dict(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    torch.cuda.set_device(0)
    old = comm_mod.Communicator.force_active
    comm_mod.Communicator.force_active = True
    try:
        yield dist.init_process_group("nccl")
    finally:  # later modules of the tier inherit neither the variables nor the group
        comm_mod.Communicator.force_active = old
        dist.destroy_process_group()
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_refused_splits(C, forced_w1):
    """4 workgroups per image on a launch with an exchange site, 2 in fp32, and any split but
    0 / 2 / 4 are refused on the host, before anything is launched."""
    assert forced_w1.xgmi is not None
    cn = C.convnet
    for merged in FORMS:
        def call(c, xc, split):
            dev = lambda k: c[k].to(DEV)  # noqa: E731
            B, dt = c["B"], c["y2"].dtype
            dp1, bslab1 = torch.zeros(B, 16, 14, 14, device=DEV, dtype=dt), torch.zeros(4 * B * 32, device=DEV)
            head = (dev("wpk_d"), dev("y2"), dev("dp2"), dev("idx2"), dev("fstats2"), dev("gsum2"), dev("gamma"), EPS,
                    dp1, dev("idx1"), dev("xh1"), bslab1)
            if merged:
                wslab2 = torch.zeros(cn.wgrad_bn_rows(2, B) * (32 * 400 + 32), device=DEV)
                cn.conv2_bwd(*head, dev("p1"), wslab2, xc, None, None, None, None, None, None, None, None, split)
            else:
                cn.conv2_dgrad(*head, xc, split)

        c = _float_case(2, torch.bfloat16)
        with pytest.raises(RuntimeError, match="2 workgroups per image"):
            call(c, forced_w1.xgmi, 4)
        for bad in (1, 3, 8, -2):
            with pytest.raises(RuntimeError, match="split is 0"):
                call(c, None, bad)
        c32 = {k: (v.float() if torch.is_tensor(v) and v.dtype == torch.bfloat16 else v) for k, v in c.items()}
        with pytest.raises(RuntimeError, match="fp32 data gradient runs 4"):
            call(c32, None, 2)
    torch.cuda.synchronize()


def _site_handles(x):
    m = re.search(r"site handles ([\d,]+)", x.debug_state(2.0))
    assert m is not None
    return sum(int(v) for v in m.group(1).split(","))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_plain_and_site_steps_give_the_same_bn1_gradients(C, forced_w1, dtype):
    """One bf16 / fp16 step of the plain ConvNet (data gradient at 4, no site) and one of DDP + SyncBN
    at world 1 through the in-kernel sites (data gradient at 2): BN1's weight and bias
    gradients -- the column sums of the slab's rows, taken by the conv1 weight-gradient launch --
    are bitwise equal, and so are conv1's own gradients, which use the same sums."""
    from ddp_practice_amd.amp import GradScaler
    from ddp_practice_amd.models import ConvNet
    from ddp_practice_amd.nn import CrossEntropyLoss
    from ddp_practice_amd.parallel import DistributedDataParallel, convert_sync_batchnorm

    x = forced_w1.xgmi
    assert x is not None and C.convnet.sites_resident(32, dtype)
    torch.manual_seed(3)
    plain = ConvNet(amp_dtype=dtype).cuda()
    with torch.no_grad():
        for bn in (plain.layer1[1], plain.layer2[1]):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)
    ddp = DistributedDataParallel(convert_sync_batchnorm(copy.deepcopy(plain)), device_ids=[0])
    images = torch.rand(32, 1, 28, 28, device=DEV).to(dtype)
    labels = torch.randint(0, 10, (32,), device=DEV)
    crit = CrossEntropyLoss()
    before = _site_handles(x)
    grads = []
    for m in (plain, ddp):
        GradScaler().scale(crit(m(images), labels)).backward()
        torch.cuda.synchronize()
        grads.append({k: p.grad.detach().clone() for k, p in (m.module if m is ddp else m).named_parameters()})
    assert _site_handles(x) > before, "the DDP step did not go through the in-kernel sites"
    assert x.error() == 0
    for k in ("layer1.1.weight", "layer1.1.bias", "layer1.0.weight", "layer1.0.bias"):
        a, b = grads[0][k].float(), grads[1][k].float()
        assert bool(torch.isfinite(a).all())
        ne = (a.view(torch.int32) != b.view(torch.int32)).sum().item()
        print(f"{k}: {ne} of {a.numel()} elements differ, max |diff| {(a - b).abs().max().item():.3e}")
        assert ne == 0, (k, ne)
