"""Native channels-last kernels (csrc/kernels/bn_nhwc.hip) vs torch fp32 / float64
references, and the native ResNet-50 path vs the torch module path."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-12)).item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,res,relu", [(64, False, True), (256, True, True), (2048, False, False),
                                        (512, True, False), (24, True, True), (320, False, True)])
def test_bn_act_fwd_bwd(C, res, relu, dtype):
    from ddp_practice_amd.ops.bn_nhwc import bn_act

    torch.manual_seed(0)
    N, H, W = 3, 7, 9
    x = (torch.randn(N, C, H, W, device=DEV) * 2 + 0.5).to(dtype).contiguous(memory_format=torch.channels_last)
    r = torch.randn(N, C, H, W, device=DEV).to(dtype).contiguous(memory_format=torch.channels_last) if res else None
    bn = torch.nn.BatchNorm2d(C).to(DEV)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.3, 0.3)
        bn.running_mean.uniform_(-0.2, 0.2)
    ref = copy.deepcopy(bn).double()
    xs = x.detach().clone().requires_grad_()
    rs = r.detach().clone().requires_grad_() if res else None
    y = bn_act(xs, bn, res=rs, relu=relu)
    x64 = x.double().detach().requires_grad_()
    r64 = r.double().detach().requires_grad_() if res else None
    y64 = ref(x64) + (r64 if res else 0)
    if relu:
        y64 = y64.relu()
    assert y.is_contiguous(memory_format=torch.channels_last) and y.dtype == dtype
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    assert _rel(y, y64) < tol
    assert _rel(bn.running_mean, ref.running_mean) < 1e-5 and _rel(bn.running_var, ref.running_var) < 1e-5
    assert int(bn.num_batches_tracked) == 1
    g = torch.randn_like(y64)
    (y.double() * g).sum().backward()
    (y64 * g).sum().backward()
    gtol = 1e-4 if dtype == torch.float32 else 3e-2
    assert _rel(xs.grad, x64.grad) < gtol
    assert _rel(bn.weight.grad, ref.weight.grad) < gtol and _rel(bn.bias.grad, ref.bias.grad) < gtol
    if res:
        assert _rel(rs.grad, r64.grad) < gtol


@pytest.mark.parametrize("shape,res,relu,dtype", [((32, 64, 28, 28), False, True, torch.bfloat16),
                                                  ((128, 2048, 7, 7), True, True, torch.bfloat16),
                                                  ((16, 1024, 14, 14), False, False, torch.float32),
                                                  ((8, 128, 56, 56), True, False, torch.float32)])
def test_bn_act_large(shape, res, relu, dtype):
    """ResNet-50 row counts, several channel chunks, and cumulative-average running stats
    (momentum=None: num_batches_tracked bumped by the statistics kernel).  With the default
    statistics target every shape here has at most 128 row blocks per chunk, which is ONE
    level of the ticket tree (G1 = 128); the two-level tree is checked against a reference
    in tests/test_bn_nhwc_exact_gpu.py."""
    from ddp_practice_amd.ops.bn_nhwc import bn_act

    torch.manual_seed(2)
    N, C, H, W = shape
    bn = torch.nn.BatchNorm2d(C, momentum=None).to(DEV)
    ref = copy.deepcopy(bn).double()
    for it in range(2):
        x = (torch.randn(N, C, H, W, device=DEV) * 1.5 + 0.3 * it).to(dtype).contiguous(
            memory_format=torch.channels_last)
        r = torch.randn(N, C, H, W, device=DEV).to(dtype).contiguous(memory_format=torch.channels_last) \
            if res else None
        xs = x.detach().clone().requires_grad_()
        rs = r.detach().clone().requires_grad_() if res else None
        y = bn_act(xs, bn, res=rs, relu=relu)
        x64 = x.double().detach().requires_grad_()
        r64 = r.double().detach().requires_grad_() if res else None
        y64 = ref(x64) + (r64 if res else 0)
        if relu:
            y64 = y64.relu()
        tol = 1e-5 if dtype == torch.float32 else 1e-2
        assert _rel(y, y64) < tol
        assert _rel(bn.running_mean, ref.running_mean) < 1e-5 and _rel(bn.running_var, ref.running_var) < 1e-5
        assert int(bn.num_batches_tracked) == it + 1
        g = torch.randn_like(y64)
        (y.double() * g).sum().backward()
        (y64 * g).sum().backward()
        gtol = 1e-4 if dtype == torch.float32 else 3e-2
        assert _rel(xs.grad, x64.grad) < gtol
        if res:
            assert _rel(rs.grad, r64.grad) < gtol
    assert _rel(bn.weight.grad, ref.weight.grad) < gtol and _rel(bn.bias.grad, ref.bias.grad) < gtol


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pools(dtype):
    from ddp_practice_amd.ops.bn_nhwc import global_avg_pool, max_pool_3x3s2

    torch.manual_seed(1)
    x = torch.randn(2, 64, 15, 12, device=DEV).to(dtype).contiguous(memory_format=torch.channels_last)
    xa = x.detach().clone().requires_grad_()
    xb = x.detach().float().clone().requires_grad_()
    y = max_pool_3x3s2(xa)
    yr = F.max_pool2d(xb, 3, 2, 1)
    assert torch.equal(y.float(), yr)
    g = torch.randn_like(yr)
    y.backward(g.to(dtype))
    yr.backward(g)
    assert _rel(xa.grad, xb.grad) < (1e-6 if dtype == torch.float32 else 1e-2)
    x2 = torch.randn(3, 256, 7, 7, device=DEV).to(dtype).contiguous(memory_format=torch.channels_last)
    a = x2.detach().clone().requires_grad_()
    b = x2.detach().float().clone().requires_grad_()
    p = global_avg_pool(a)
    pr = b.mean((2, 3))
    assert _rel(p, pr) < (1e-6 if dtype == torch.float32 else 1e-2)
    gp = torch.randn_like(pr)
    p.backward(gp.to(dtype))
    pr.backward(gp)
    assert _rel(a.grad, b.grad) < (1e-6 if dtype == torch.float32 else 1e-2)


@pytest.mark.parametrize("amp", [None, torch.bfloat16])
def test_resnet50_native_matches_torch_path(C, amp):
    """Native path vs a float64 run of the torch module path: the native error must
    stay within a small factor of the torch path's own error at the same precision
    (fp32 eager, or torch autocast) -- BatchNorm over few elements per channel
    (batch 8, 3x3 maps in layer4) amplifies every rounding difference."""
    from ddp_practice_amd.models import resnet50

    torch.manual_seed(0)
    m = resnet50(num_classes=10, amp_dtype=amp).to(DEV)
    t = copy.deepcopy(m)
    t.fused = False
    t.amp_dtype = None
    r64 = copy.deepcopy(t).double()
    x = torch.rand(8, 3, 96, 96, device=DEV)
    y = torch.randint(0, 10, (8,), device=DEV)
    out = m(x)
    if amp is None:
        ref_t = t(x)
    else:
        with torch.autocast("cuda", dtype=amp):
            ref_t = t(x)
    ref = r64(x.double())
    fac, floor = (4.0, 1e-4) if amp is None else (3.0, 2e-2)
    assert _rel(out, ref) < max(fac * _rel(ref_t, ref), floor), (_rel(out, ref), _rel(ref_t, ref))
    F.cross_entropy(out.float(), y).backward()
    F.cross_entropy(ref_t.float(), y).backward()
    F.cross_entropy(ref, y).backward()
    gt, g64 = dict(t.named_parameters()), dict(r64.named_parameters())
    bad = []
    for n, p in m.named_parameters():
        if n.endswith("bias") and n != "fc.bias" and "bn" not in n and "downsample.1" not in n:
            continue
        e, et = _rel(p.grad, g64[n].grad), _rel(gt[n].grad, g64[n].grad)
        if e > max(fac * et, floor):
            bad.append((n, e, et))
    # one value within an ulp of a ReLU threshold routes differently from float64 and
    # moves every tensor of that bottleneck its gradient passes through (its BN affine
    # grads and convs; layer4 normalises over 72 values per channel here): allow the
    # outliers of at most two blocks, each within 10x torch's error or 0.5 % (a flip
    # moves a BN weight gradient by ~0.2 % while torch's own error there can be ~1e-4:
    # seen once on a fresh box, layer4.2.bn3.weight 1.9e-3 vs 8.5e-5)
    blocks = {".".join(n.split(".")[:2]) for n, _, _ in bad}
    assert len(blocks) <= 2 and len(bad) <= 12 and all(e < 10 * et + 5e-3 for _, e, et in bad), bad[:12]
    for (n, b), (_, bt), (_, r) in zip(m.named_buffers(), t.named_buffers(), r64.named_buffers()):
        if b.dtype.is_floating_point:
            assert _rel(b, r) < max(fac * _rel(bt, r), 1e-3), (n, _rel(b, r), _rel(bt, r))
        else:
            assert torch.equal(b, r.to(b.dtype)), n
    m.eval()
    t.eval()
    r64.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=amp or torch.bfloat16, enabled=amp is not None):
        e_ref = _rel(t(x), r64(x.double()))
    with torch.no_grad():
        e = _rel(m(x), r64(x.double()))
    assert e < max(fac * e_ref, floor), (e, e_ref)


def test_wgrad_batch_matches_per_conv_reduction(monkeypatch):
    """The weight-gradient reductions of a backward pass batched into one end-of-backward
    launch (ops/conv_igemm.WgradBatch) give bitwise the gradients of one reduction per conv,
    are complete when backward() returns, and are skipped when a gradient already exists
    (autograd reads it to accumulate): a second backward accumulates exactly as without."""
    from ddp_practice_amd.models import resnet50
    from ddp_practice_amd.ops import conv_igemm

    torch.manual_seed(0)
    base = resnet50(num_classes=10, amp_dtype=torch.bfloat16).to(DEV)
    x = torch.rand(8, 3, 96, 96, device=DEV)
    y = torch.randint(0, 10, (8,), device=DEV)
    one, two = {}, {}
    for on in (False, True):
        monkeypatch.setattr(conv_igemm.WgradBatch, "enabled", on)
        m = copy.deepcopy(base)
        F.cross_entropy(m(x).float(), y).backward()
        assert not conv_igemm.WgradBatch._pending
        one[on] = {n: p.grad.clone() for n, p in m.named_parameters()}
        F.cross_entropy(m(x).float(), y).backward()
        assert not conv_igemm.WgradBatch._pending
        two[on] = {n: p.grad.clone() for n, p in m.named_parameters()}
    bad1 = [n for n, g in one[False].items() if not torch.equal(g, one[True][n])]
    bad2 = [n for n, g in two[False].items() if not torch.equal(g, two[True][n])]
    assert not bad1 and not bad2, (bad1[:8], bad2[:8])


@pytest.mark.parametrize("C", [256, 64, 24])
def test_bn_res_bn_fwd_bwd(C):
    """relu(bn(x) + bn_r(r)) in one pass (ops/bn_nhwc.bn_res_bn) == float64 torch: output,
    both BNs' running stats, and every gradient (x, r, both BNs' affine parameters)."""
    from ddp_practice_amd.ops.bn_nhwc import bn_res_bn

    torch.manual_seed(1)
    N, H, W = 3, 7, 9
    cl = torch.channels_last
    x = (torch.randn(N, C, H, W, device=DEV) * 2 + 0.5).to(torch.bfloat16).contiguous(memory_format=cl)
    r = (torch.randn(N, C, H, W, device=DEV) - 0.3).to(torch.bfloat16).contiguous(memory_format=cl)
    bn, rbn = torch.nn.BatchNorm2d(C).to(DEV), torch.nn.BatchNorm2d(C).to(DEV)
    with torch.no_grad():
        for m in (bn, rbn):
            m.weight.uniform_(0.5, 1.5)
            m.bias.uniform_(-0.3, 0.3)
            m.running_mean.uniform_(-0.2, 0.2)
    ref, rref = copy.deepcopy(bn).double(), copy.deepcopy(rbn).double()
    xs, rs = x.detach().clone().requires_grad_(), r.detach().clone().requires_grad_()
    y = bn_res_bn(xs, bn, rs, rbn)
    x64, r64 = x.double().detach().requires_grad_(), r.double().detach().requires_grad_()
    y64 = (ref(x64) + rref(r64)).relu()
    assert _rel(y, y64) < 1e-2
    for m, mr in ((bn, ref), (rbn, rref)):
        assert _rel(m.running_mean, mr.running_mean) < 1e-5 and _rel(m.running_var, mr.running_var) < 1e-5
        assert int(m.num_batches_tracked) == 1
    g = torch.randn_like(y64)
    (y.double() * g).sum().backward()
    (y64 * g).sum().backward()
    assert _rel(xs.grad, x64.grad) < 3e-2 and _rel(rs.grad, r64.grad) < 3e-2
    for m, mr in ((bn, ref), (rbn, rref)):
        assert _rel(m.weight.grad, mr.weight.grad) < 3e-2 and _rel(m.bias.grad, mr.bias.grad) < 3e-2
    bn.eval()
    rbn.eval()
    ref.eval()
    rref.eval()
    with torch.no_grad():
        ye = bn_res_bn(x, bn, r, rbn)
        assert _rel(ye, (ref(x.double()) + rref(r.double())).relu()) < 1e-2
