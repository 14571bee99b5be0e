"""conv2 weight gradient decomposed by output slice (csrc/kernels/conv5x5_wgrad.h
conv5x5_wgrad_body NSL, convnet_fused.hip conv2_wgrad_role): one slab row per image.

Each row (dW partial | db partial of ONE image) and the column sums are compared with a
float64 reference computed with torch on the CPU: autograd through BN (batch statistics)
-> ReLU -> MaxPool for dy, then the weight gradient of the 5x5 conv.  Bound: the rule of
tests/test_convnet_fused_gpu.py::test_convnet_fused_fwd_bwd -- the error against float64
is at most 2x the error of torch's own computation of the same quantity in the same dtype
(dy rounded to the dtype, a GEMM in that dtype), with that test's floors (1e-5 fp32,
2e-3 bf16 / fp16; the floors matter only where torch's error is ~0).
"""
import copy
import functools
import hashlib
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-5
NW, ROW = 32 * 400, 32 * 400 + 32
DTYPES = [torch.bfloat16, torch.float16, torch.float32]


def _floor(dtype):
    return 1e-5 if dtype == torch.float32 else 2e-3


@functools.lru_cache(maxsize=None)
def _case(B, dtype):
    """Seeded inputs of the layer-2 weight gradient (CPU), the float64 rows and torch's own
    rows in `dtype`.  Computed once per (B, dtype); nothing in it is modified afterwards."""
    g = torch.Generator().manual_seed(1000 * B + DTYPES.index(dtype))
    y2 = torch.randn(B, 32, 14, 14, generator=g).to(dtype)
    p1 = torch.randn(B, 16, 14, 14, generator=g).clamp_(min=0).to(dtype)  # a pooled ReLU output
    dp2 = torch.randn(B, 32, 7, 7, generator=g).to(dtype)
    gamma = torch.rand(32, generator=g) + 0.5
    beta = torch.rand(32, generator=g) * 0.4 - 0.2
    # float64: BN (batch statistics) -> ReLU -> MaxPool and its backward
    y = y2.double().requires_grad_()
    z = F.batch_norm(y, None, None, gamma.double(), beta.double(), training=True, eps=EPS)
    z.retain_grad()
    pool, ind = F.max_pool2d(F.relu(z), 2, 2, return_indices=True)
    pool.backward(dp2.double())
    dy64, gz = y.grad, z.grad
    pos = ((ind // 14) % 2) * 2 + (ind % 14) % 2
    idx2 = (pos + 4 * (pool > 0)).to(torch.uint8)  # argmax in the window | ReLU-open bit
    # forward statistics [sum(y - shift) | sum((y - shift)^2) | n | shift] and the BN backward
    # sums, one [S1 | S2] row per image
    yd = y2.double()
    mean = yd.mean((0, 2, 3))
    var = yd.var((0, 2, 3), unbiased=False)
    shift = mean.float()
    d = yd - shift.double().view(1, -1, 1, 1)
    n = float(B * 196)
    fstats2 = torch.cat([d.sum((0, 2, 3)), (d * d).sum((0, 2, 3)), torch.tensor([n], dtype=torch.float64),
                         shift.double()]).float()
    xhat = (yd - mean.view(1, -1, 1, 1)) * torch.rsqrt(var + EPS).view(1, -1, 1, 1)
    gsum2 = torch.cat([gz.sum((2, 3)), (gz * xhat).sum((2, 3))], 1).float().contiguous()  # [B][64]
    # float64 rows: dW[b] = dy[b] (32 x 196) . unfold(p1[b])^T (196 x 400), db[b] = sum dy[b]
    cols = F.unfold(p1.double(), 5, padding=2)  # [B][(ci, kh, kw)][196]
    rows64 = torch.cat([torch.bmm(dy64.reshape(B, 32, 196), cols.transpose(1, 2)).reshape(B, NW),
                        dy64.sum((2, 3))], 1)
    # the unfold form IS the conv weight gradient
    wref = torch.nn.grad.conv2d_weight(p1.double(), (32, 16, 5, 5), dy64, padding=2)
    assert torch.allclose(rows64[:, :NW].sum(0), wref.reshape(-1), rtol=1e-10, atol=1e-10)
    # torch in `dtype`: dy rounded to the dtype, the same GEMM and sums in that dtype
    dyt = dy64.to(dtype).to(DEV)
    colt = F.unfold(p1.to(DEV), 5, padding=2)
    rows_t = torch.cat([torch.bmm(dyt.reshape(B, 32, 196), colt.transpose(1, 2)).reshape(B, NW),
                        dyt.sum((2, 3))], 1)
    sums_t = torch.cat([(dyt.permute(1, 0, 2, 3).reshape(32, -1) @
                         colt.permute(1, 0, 2).reshape(400, -1).t()).reshape(-1), dyt.sum((0, 2, 3))])
    return dict(B=B, dtype=dtype, y2=y2, p1=p1, dp2=dp2, idx2=idx2, gamma=gamma, fstats2=fstats2, gsum2=gsum2,
                rows64=rows64, rows_t=rows_t.double().cpu(), sums_t=sums_t.double().cpu())


def _run(C, c, merged, fill=None):
    """The slab written by the merged conv2_bwd launch or by conv_wgrad_bn's layer-2 branch."""
    cn = C.convnet
    B, dt = c["B"], c["dtype"]
    y2, p1, dp2, idx2 = (c[k].to(DEV) for k in ("y2", "p1", "dp2", "idx2"))
    fstats2, gsum2, g2 = (c[k].to(DEV) for k in ("fstats2", "gsum2", "gamma"))
    rows = cn.wgrad_bn_rows(2, B)
    assert rows == B  # one slab row per image
    wslab = torch.empty(rows * ROW, device=DEV)
    if fill is not None:
        wslab.fill_(fill)
    if merged:
        g = torch.Generator().manual_seed(7)
        wpk_d = torch.randn(cn.W2D_LEN, generator=g).mul_(0.05).to(DEV, dt)
        dp1 = torch.empty(B, 16, 14, 14, device=DEV, dtype=dt)
        idx1 = torch.randint(0, 8, (B, 16, 14, 14), generator=g, dtype=torch.uint8).to(DEV)
        xh1 = torch.randn(B, 16, 14, 14, generator=g).to(DEV, dt)
        bslab1 = torch.empty(cn.dgrad2_rows(B, dt == torch.float32) * 32, device=DEV)
        cn.conv2_bwd(wpk_d, y2, dp2, idx2, fstats2, gsum2, g2, EPS, dp1, idx1, xh1, bslab1, p1, wslab, None,
                     None, None, None, None, None, None, None, None)
    else:
        cn.conv_wgrad_bn(p1, y2, dp2, idx2, fstats2, gsum2, None, g2, EPS, None, None, wslab, None)
    torch.cuda.synchronize()
    return wslab.view(rows, ROW)


def _rel_rows(a, r):
    return (a - r).norm(dim=-1) / (r.norm(dim=-1) + 1e-12)


@pytest.mark.parametrize("merged", [True, False], ids=["conv2_bwd", "conv_wgrad_bn"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("B", [1, 3, 33])
def test_rows_match_float64(C, B, dtype, merged):
    """Slab row b == the weight / bias gradient of image b alone; the column sums == the
    batch's.  B = 1: a grid of 2 * NSL workgroups; 3: odd; 33: more than 32 images and more
    than two rows per reducing lane."""
    c = _case(B, dtype)
    rows = _run(C, c, merged).double().cpu()
    r64, rt = c["rows64"], c["rows_t"]
    floor = _floor(dtype)
    for what, sl in (("dW", slice(0, NW)), ("db", slice(NW, ROW))):
        if what == "db" and B == 1:
            continue  # the one image is the batch: its bias row IS the column sum (0 analytically), below
        e = _rel_rows(rows[:, sl], r64[:, sl])
        lim = (2.0 * _rel_rows(rt[:, sl], r64[:, sl])).clamp_(min=floor)
        k = int((e / lim).argmax())
        print(f"B={B} {dtype} {what} rows: worst row {k}: err {e[k].item():.3e} limit {lim[k].item():.3e}")
        assert bool((e < lim).all()), (what, k, e[k].item(), lim[k].item())
    s, s64, st = rows.sum(0), r64.sum(0), c["sums_t"]
    e, lim = _rel_rows(s[:NW], s64[:NW]).item(), max(2.0 * _rel_rows(st[:NW], s64[:NW]).item(), floor)
    print(f"B={B} {dtype} dW column sums: err {e:.3e} limit {lim:.3e}")
    assert e < lim, ("dW column sums", e, lim)
    # db2 sums to 0 analytically (a BatchNorm follows the conv): absolute, as the bias rule
    # of test_convnet_fused_fwd_bwd
    lp = dtype != torch.float32
    e = (s[NW:] - s64[NW:]).abs().max().item()
    lim = (4.0 if lp else 2.0) * (st[NW:] - s64[NW:]).abs().max().item() + (1e-2 if lp else 1e-4)
    print(f"B={B} {dtype} db column sums: abs err {e:.3e} limit {lim:.3e}")
    assert e < lim, ("db column sums", e, lim)


@pytest.mark.parametrize("merged", [True, False], ids=["conv2_bwd", "conv_wgrad_bn"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
def test_every_slice_written_and_deterministic(C, dtype, merged):
    """A slab pre-filled with NaN holds no NaN afterwards (every slice of every row, the bias
    columns included, is written), and reruns are bitwise equal (fixed orders, no atomics)."""
    c = _case(3, dtype)
    a = _run(C, c, merged, fill=float("nan"))
    assert not bool(torch.isnan(a).any()), torch.isnan(a).nonzero()[:8]
    assert torch.equal(a, _run(C, c, merged, fill=0.0))
    assert torch.equal(a, _run(C, c, merged, fill=float("nan")))


def _forms_digest(C):
    """sha1 of the slabs of every dtype at B = 3, after checking merged == split bitwise."""
    h = hashlib.sha1()
    for dtype in DTYPES:
        c = _case(3, dtype)
        a, b = _run(C, c, True, fill=float("nan")), _run(C, c, False, fill=float("nan"))
        assert torch.equal(a, b), dtype
        h.update(a.cpu().numpy().tobytes())
    return h.hexdigest()


def _forms_main():  # the child process of test_launch_forms_agree
    from ddp_practice_amd import _ext

    print("DIGEST", _forms_digest(_ext.load()))


@pytest.mark.parametrize("dyn", ["0", "1"], ids=["static-lds", "dynamic-lds"])
def test_launch_forms_agree(C, dyn):
    """The merged conv2_bwd launch and the split conv2 weight-gradient launch write
    identical slabs, with the merged kernel's tiles in static LDS and in dynamic LDS (the
    switches are read once per process: a fresh one per setting)."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, DPA_LP_DYN_BWD=dyn, DPA_FP32_MERGED_BWD=dyn)
    code = (f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; "
            "import test_conv2_wgrad_slices_gpu as t; t._forms_main()")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    digest = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("DIGEST")]
    assert digest == [_forms_digest(C)], (digest, r.stdout[-500:])


@pytest.mark.parametrize("B", [2, 64])
def test_training_step_matches_torch(C, B):
    """One bf16 training step with the GradScaler through the flagship path (paired labels,
    slab sink): the parameters, and the update itself, against a float64 step, within 2x
    the error of the torch step (nn modules under autocast, torch GradScaler / SGD)."""
    from ddp_practice_amd.amp import GradScaler
    from ddp_practice_amd.data import DeviceLoader, synthetic
    from ddp_practice_amd.models import ConvNet
    from ddp_practice_amd.nn import CrossEntropyLoss
    from ddp_practice_amd.optim import SGD

    torch.manual_seed(5)
    m = ConvNet()
    with torch.no_grad():
        for bn in (m.layer1[1], m.layer2[1]):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)
    m = m.to(DEV)
    m64, mt = copy.deepcopy(m).double(), copy.deepcopy(m)
    m64.fused = mt.fused = False
    m.amp_dtype = mt.amp_dtype = torch.bfloat16
    before = {k: v.detach().double().clone() for k, v in m.named_parameters()}
    lr = 0.05
    loader = DeviceLoader(synthetic(B, seed=2), batch_size=B, shuffle=False, device=DEV, dtype=torch.bfloat16)
    images, labels = loader.static_batch()
    loader.start_epoch()
    loader.fill_(images, labels, step=0)
    x32 = images.float()
    # this package's step
    opt, scaler, crit = SGD(m.parameters(), lr=lr), GradScaler(), CrossEntropyLoss()
    assert m.set_slab_sink(opt)
    loss = crit(m(images), labels)
    opt.zero_grad(set_to_none=True)
    scaler.scale(loss).backward()
    scaler.step(opt)
    scaler.update()
    # the torch step
    opt_t, scaler_t = torch.optim.SGD(mt.parameters(), lr=lr), torch.amp.GradScaler("cuda")
    loss_t = F.cross_entropy(mt(x32).float(), labels)
    scaler_t.scale(loss_t).backward()
    scaler_t.step(opt_t)
    scaler_t.update()
    # float64
    opt_r = torch.optim.SGD(m64.parameters(), lr=lr)
    F.cross_entropy(m64(x32.double()), labels).backward()
    opt_r.step()
    torch.cuda.synchronize()
    assert abs(loss.item() - loss_t.item()) < 0.05 * abs(loss_t.item()) + 1e-3
    named_t, named_r = dict(mt.named_parameters()), dict(m64.named_parameters())
    for k, p in m.named_parameters():
        a, t, r = p.detach().double(), named_t[k].detach().double(), named_r[k].detach()
        da, dt_, dr = a - before[k], t - before[k], r - before[k]
        if k.endswith("0.bias"):
            # conv bias gradients are 0 analytically (a BatchNorm follows): noise against noise,
            # absolute, as test_convnet_fused_fwd_bwd (4x torch's + 1e-2 on the gradient)
            e, lim = (da - dr).abs().max().item(), 4.0 * (dt_ - dr).abs().max().item() + lr * 1e-2
            print(f"B={B} {k}: update abs err {e:.3e} limit {lim:.3e}")
            assert e < lim, (k, e, lim)
            continue
        for what, (u, v, w) in (("parameter", (a, t, r)), ("update", (da, dt_, dr))):
            e = ((u - w).norm() / (w.norm() + 1e-12)).item()
            lim = max(2.0 * ((v - w).norm() / (w.norm() + 1e-12)).item(), 2e-3)
            print(f"B={B} {k} {what}: err {e:.3e} limit {lim:.3e}")
            assert e < lim, (k, what, e, lim)
