"""The add order of the slab column sums in the BatchNorm coefficient prologues
(csrc/kernels/convblock_bn.h bn_finalize / bn_bwd_coef), pinned bit for bit through the outputs
that expose the sums unchanged:

  bn1_fwd  convnet.conv2_fwd            workgroup 0 writes fstats1[0 .. 32]   (RL 33, G 7)
  bn2_fwd  convnet_head.head_step       workgroup 0 writes fstats2[0 .. 64]   (RL 65, G 3)
  bn2_bwd  convnet.conv2_bwd            dbeta2 | dgamma2                      (RL 64, G 4)
  bn1_bwd  convnet.conv1_wgrad_slab2    dbeta1 | dgamma1                      (RL 32, G 8)
           and convnet.conv_wgrad_bn, the same body in its own launch

The slabs hold the order-sensitive values of tests/_bn_coef_ref.py (mixed magnitudes, fixed
seed; tests/test_bn_coef_ref_cpu.py shows that another order gives other bits) and the outputs
are compared bitwise with its numpy float32 emulation of the documented order.  The backward
launches run twice over: with the parameter gradients taken from the global rows, and from
separate local rows (lsum), which the leader sums behind the coefficients.

Every other input is zero (finite, any shape), so only the prologue decides what is compared.
Batches: 1 (fewer rows than lane groups), 2, 8, 32 (the step's own row counts: one load batch
sized for them), 33 and 64 (the loop behind the first batch).  Each launch runs twice and the
reruns are compared bitwise.
"""
import functools

import numpy as np
import pytest
import torch

from . import _bn_coef_ref as R
from . import test_head_exact_gpu as HX

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-5
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
# every batch in bf16 (the prologues do not depend on the storage type beyond the instantiation),
# the step's batch in all three
CASES = [(B, BF16) for B in R.BATCHES] + [(32, F16), (32, F32)]
PARAMS = pytest.mark.parametrize("B,dtype", CASES, ids=lambda v: str(v).replace("torch.", ""))


@functools.lru_cache(maxsize=None)
def _slab(name, rows, RL, other=False):
    """(device slab, expected column sums) -- computed once, never modified."""
    s = R.case(name, rows, RL)
    if other:  # the local rows of a launch that is given both: other values, same shape
        s = np.ascontiguousarray(s[::-1, ::-1])
    return torch.from_numpy(s.copy()).reshape(-1).to(DEV), torch.from_numpy(R.colsum(s))


def _same(got, want, what):
    got, want = got.detach().cpu().contiguous(), want.contiguous()
    g, w = got.numpy().view(np.uint32), want.numpy().view(np.uint32)
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {g.size} columns differ, first {int(bad[0])}: got "
                           f"{float(got[bad[0]])!r}, documented order gives {float(want[bad[0]])!r}")


def _twice(run, what):
    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x.cpu().view(torch.int32), y.cpu().view(torch.int32)), what + ": reruns differ"
    return a


def _z(*shape, dtype=F32):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


@PARAMS
def test_bn1_finalize_in_conv2_fwd(C, B, dtype):
    cn = C.convnet
    rows = int(C.convblock.fwd_rows(1, 16, 28, 28, B))
    assert rows == R.shapes(B, 4 * B)["bn1_fwd"][0]
    slab, want = _slab("bn1_fwd", rows, 33)
    ns = int(cn.fwd2_split(dtype == F32))

    def run():
        fstats1 = torch.full((49,), float("nan"), device=DEV)
        fstats1[33:] = 0.0  # the shift
        cn.conv2_fwd(_z(B, 16, 28, 28, dtype=dtype), slab, fstats1, torch.ones(16, device=DEV), _z(16), _z(16),
                     torch.ones(16, device=DEV), _z(1, dtype=torch.int64), 0.1, EPS, True, _z(32, 16, 5, 5), _z(32),
                     _z(B, 32, 14, 14, dtype=dtype), _z(B * ns * 65), _z(97), _z(32), _z(B, 16, 14, 14, dtype=dtype),
                     _z(B, 16, 14, 14, dtype=torch.uint8), _z(B, 16, 14, 14, dtype=dtype), _z(32 * 424, dtype=dtype),
                     None)
        torch.cuda.synchronize()
        return (fstats1[:33].clone(),)

    (got,) = _twice(run, "conv2_fwd")
    _same(got, want, f"conv2_fwd fstats1, {rows} rows")


@PARAMS
def test_bn2_finalize_in_head_step(C, B, dtype):
    N = 10
    rows = B * int(C.convnet.fwd2_split(dtype == F32))
    assert rows == R.shapes(B, 4 * B)["bn2_fwd"][0]
    slab, want = _slab("bn2_fwd", rows, 65)
    t = HX._head_case(B, N, rows)

    def run():
        d = HX._head_buffers(t, dtype, B, N)
        d["fslab"] = slab
        HX._step_buffers(d, HX._targets(B, N, "none", 100 * B + N), False, dtype, B, N)
        C.convnet_head.head_step(d["y2"], d["fslab"], d["fstats"], d["g"], d["b"], d["rm"], d["rv"], d["nbt"], 0.1,
                                 t["eps"], d["wfc"], d["bfc"], d["logits"], d["p2"], d["idx2"], d["xh2"], d["tgt"],
                                 -100, 0.0, d["scale"], d["state"], d["loss"], d["dlog"], d["dls"], d["dp2"],
                                 d["bsum"], None, d["chk"], None)
        torch.cuda.synchronize()
        return (d["fstats"][:65].clone(),)

    (got,) = _twice(run, "head_step")
    _same(got, want, f"head_step fstats2, {rows} rows")


@pytest.mark.parametrize("local", [False, True], ids=["global-rows", "local-rows"])
@PARAMS
def test_bn2_bwd_coef_in_conv2_bwd(C, B, dtype, local):
    cn = C.convnet
    rows = R.shapes(B, 4 * B)["bn2_bwd"][0]
    gsum, want = _slab("bn2_bwd", rows, 64)
    lsum = None
    if local:
        lsum, want = _slab("bn2_bwd", rows, 64, other=True)
    fstats2 = _z(97)
    fstats2[32:65] = float(B * 196)  # unit variance, the pixel count

    def run():
        dg, dbe = torch.full((32,), float("nan"), device=DEV), torch.full((32,), float("nan"), device=DEV)
        cn.conv2_bwd(_z(16 * 808, dtype=dtype), _z(B, 32, 14, 14, dtype=dtype), _z(B, 32, 7, 7, dtype=dtype),
                     _z(B, 32, 7, 7, dtype=torch.uint8), fstats2, gsum, torch.ones(32, device=DEV), EPS,
                     _z(B, 16, 14, 14, dtype=dtype), _z(B, 16, 14, 14, dtype=torch.uint8),
                     _z(B, 16, 14, 14, dtype=dtype), _z(int(cn.dgrad2_rows(B, dtype == F32)) * 32),
                     _z(B, 16, 14, 14, dtype=dtype), _z(int(cn.wgrad_bn_rows(2, B)) * (32 * 400 + 32)), None, lsum, dg,
                     dbe, None, None, None, None, None)
        torch.cuda.synchronize()
        return dbe, dg

    dbe, dg = _twice(run, "conv2_bwd")
    _same(dbe, want[:32], f"conv2_bwd dbeta2, {rows} rows")
    _same(dg, want[32:], f"conv2_bwd dgamma2, {rows} rows")


@pytest.mark.parametrize("local", [False, True], ids=["global-rows", "local-rows"])
@pytest.mark.parametrize("which", ["conv1_wgrad_slab2", "conv_wgrad_bn"])
@PARAMS
def test_bn1_bwd_coef_in_conv1_wgrad(C, B, dtype, which, local):
    cn = C.convnet
    rows = int(cn.dgrad2_rows(B, dtype == F32))
    assert rows == R.shapes(B, 4 * B)["bn1_bwd"][0]
    gsum, want = _slab("bn1_bwd", rows, 32)
    lsum = None
    if local:
        lsum, want = _slab("bn1_bwd", rows, 32, other=True)
    fstats1 = _z(49)
    fstats1[16:33] = float(B * 784)
    N1, N2 = 16 * 25 + 16, 32 * 400 + 32

    def run():
        dg, dbe = torch.full((16,), float("nan"), device=DEV), torch.full((16,), float("nan"), device=DEV)
        args = (_z(B, 1, 28, 28, dtype=dtype), _z(B, 16, 28, 28, dtype=dtype), _z(B, 16, 14, 14, dtype=dtype),
                _z(B, 16, 14, 14, dtype=torch.uint8), fstats1, gsum, lsum, torch.ones(16, device=DEV), EPS, dg, dbe,
                _z(int(cn.wgrad_bn_rows(1, B)) * N1))
        if which == "conv_wgrad_bn":
            cn.conv_wgrad_bn(*args, None)
        else:
            cn.conv1_wgrad_slab2(*args, _z(int(cn.wgrad_bn_rows(2, B)) * N2), _z(N2), None, None)
        torch.cuda.synchronize()
        return dbe, dg

    dbe, dg = _twice(run, which)
    _same(dbe, want[:16], f"{which} dbeta1, {rows} rows")
    _same(dg, want[16:], f"{which} dgamma1, {rows} rows")
