"""The BatchNorm coefficient prologues with the slab's row count known at compile time, and the
one-launch head's division-free feature addressing (csrc/kernels/convblock_bn.h
strided_rowsum_n, csrc/kernels/convnet_head.hip head_row_kernel).

a. fstats1 / fstats2 and dbeta / dgamma of both blocks equal, bit for bit, the numpy float32
   emulation of the documented add order (tests/_bn_coef_ref.py: rows g, g + G, ... within a lane
   group from +0, then the groups 0 .. G-1 from +0) on slabs whose values make another order
   visible.  Batch 32 has the step's own row counts (128, 128, 32 and 128 rows): the launches take
   the compile-time form, in bf16, fp16 and fp32.  Batches 1, 31 and 33 keep the runtime form:
   fewer rows than lane groups, one row short of the compile-time count (the same load batch, its
   last rows masked), and one past it (the loop behind the first batch in the forward slabs).
   The launches and comparisons are those of tests/test_bn_coef_order_gpu.py, called here at
   these batches.

b. At batch 32 the head launch's p2, idx2, xh2 and logits equal the three-launch head's
   (convnet.head_fwd) bit for bit, and its dp2 equals convnet.head_bwd's on the head launch's own
   dls.  The inputs are tests/_head_ref.py head_inputs, whose 16-bit logit sums are exact, so the
   two kernels' different lane reductions give the same bits.  head_bwd sums the BN2 backward
   sums over the whole batch, the head launch writes one row per image, so the rows are compared
   with a float32 emulation of the head's own order on those (bitwise equal) dp2 / idx2 / xh2:
   lane j of a channel's 8 adds positions j, j + 8, ... from +0; the 8 lanes are then added as
   ((l0 + l1) + (l2 + l3)) + ((l7 + l6) + (l5 + l4)) (common.h group_sum<8>, seen from lane 0).
   A feature loaded from, stored to or summed at another index changes one of the six.
"""
import functools

import numpy as np
import pytest
import torch

from . import _head_ref as R
from . import test_bn_coef_order_gpu as O
from . import test_head_exact_gpu as HX

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
CASES = [(B, BF16) for B in (1, 31, 32, 33)] + [(32, F16), (32, F32)]
PARAMS = pytest.mark.parametrize("B,dtype", CASES, ids=lambda v: str(v).replace("torch.", ""))


# =============================================================================== a
@PARAMS
def test_bn1_forward_sums(C, B, dtype):
    O.test_bn1_finalize_in_conv2_fwd(C, B, dtype)


@PARAMS
def test_bn2_forward_sums(C, B, dtype):
    O.test_bn2_finalize_in_head_step(C, B, dtype)


@pytest.mark.parametrize("local", [False, True], ids=["global-rows", "local-rows"])
@PARAMS
def test_bn2_backward_sums(C, B, dtype, local):
    O.test_bn2_bwd_coef_in_conv2_bwd(C, B, dtype, local)


@pytest.mark.parametrize("local", [False, True], ids=["global-rows", "local-rows"])
@pytest.mark.parametrize("which", ["conv1_wgrad_slab2", "conv_wgrad_bn"])
@PARAMS
def test_bn1_backward_sums(C, B, dtype, which, local):
    O.test_bn1_bwd_coef_in_conv1_wgrad(C, B, dtype, which, local)


# =============================================================================== b
Bn, N = 32, 10


@functools.lru_cache(maxsize=None)
def _inputs(nrows):
    return R.head_inputs(Bn, N, R.head_seed(Bn, N), nrows)


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _head_rows(v):
    """[B, 32, 49] float32 -> [B, 32]: the head launch's sum over a channel's 49 positions."""
    lane = []
    for j in range(8):
        acc = np.zeros(v.shape[:2], dtype=np.float32)
        for f in range(j, 49, 8):
            acc = _f32(acc + v[..., f])
        lane.append(acc)
    lo = _f32(_f32(lane[0] + lane[1]) + _f32(lane[2] + lane[3]))
    hi = _f32(_f32(lane[7] + lane[6]) + _f32(lane[5] + lane[4]))
    return _f32(lo + hi)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
def test_head_step_equals_three_launch_head(C, dtype):
    nrows = Bn * int(C.convnet.fwd2_split(False))
    t = _inputs(nrows)
    # the three-launch head's forward
    ref = HX._head_buffers(t, dtype, Bn, N)
    C.convnet.head_fwd(ref["y2"], ref["fslab"], ref["fstats"], ref["g"], ref["b"], ref["rm"], ref["rv"], ref["nbt"],
                       0.1, t["eps"], True, ref["wfc"], ref["bfc"], ref["logits"], ref["p2"], ref["idx2"], ref["xh2"],
                       None)
    # the one-launch head (the unpacked kernel; tests/test_head_packed_gpu.py holds the packed one to it)
    d = HX._head_buffers(t, dtype, Bn, N)
    HX._step(C, d, t, HX._targets(Bn, N, "two", 100 * Bn + N), 0.1, True, 0.1, dtype, Bn, N)
    torch.cuda.synchronize()
    tag = f"head_step vs three-launch head, B={Bn} {dtype}"
    for k in ("p2", "idx2", "xh2", "logits"):
        assert not bool(torch.isnan(ref[k].float()).any()), k
        HX._same(d[k], ref[k], f"{tag} {k}")
    # the three-launch head's backward on the same loss gradient
    f = lambda *s: torch.full(s, float("nan"), device=DEV)
    dp2 = torch.full((Bn, R.HK), float("nan"), device=DEV, dtype=dtype)
    C.convnet.head_bwd(d["dls"], ref["wfc"], ref["p2"], ref["idx2"], ref["xh2"], f(N, R.HK), f(N), f(R.HC), f(R.HC),
                       f(2 * R.HC), dp2)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(dp2.float()).any())
    HX._same(d["dp2"], dp2, f"{tag} dp2")
    # the per-image BN2 backward sums in the head's own order, from the three-launch head's tensors
    g = np.where((ref["idx2"].cpu().numpy() & 4) != 0, dp2.float().cpu().numpy(), np.float32(0.0))
    g = _f32(g).reshape(Bn, R.HC, 49)
    gx = _f32(g * ref["xh2"].float().cpu().numpy().reshape(Bn, R.HC, 49))
    want = np.concatenate([_head_rows(g), _head_rows(gx)], axis=1)  # [B][S1(32) | S2(32)]
    HX._same(d["bsum"], torch.from_numpy(want).reshape(-1), f"{tag} bsum rows")
