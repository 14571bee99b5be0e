"""Squeeze-and-excitation with the bottleneck's residual add and ReLU on the hand-written
kernels of csrc/kernels/se.hip: for channels_last bf16 / fp16 ``u`` (bn3's output) and
``identity`` [N, C, H, W] and fp32 ``fc1`` [Cr, C] (+ bias), ``fc2`` [C, Cr] (+ bias),

    p = mean_hw u;  h = relu(fc1 p);  s = sigmoid(fc2 h);  y = relu(u * s + identity)

in three launches, the backward in four; the gate stays fp32 and the master parameters are read
in-kernel.  Supported: C a multiple of 64 in [64, 2048], Cr a multiple of 4 in [4, 128], any
N, H, W >= 1.  Parameter gradients are fp32 in the parameters' own shapes; every reduction has
a fixed order and there are no atomics, so a backward is bit-stable from run to run.

``DPA_SE=0`` sends every SE block of models/resnet.py to :func:`squeeze_excite_torch` (A/B).
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from .._ext import load as _load_ext
from .conv1x1 import GradTap

_CL = torch.channels_last
ENABLED = os.environ.get("DPA_SE", "1") != "0"  # 0: the torch composition (A/B)

# (C, Cr, H * W) of shapes the measurements send to the torch composition; none:
# profiles/se_bench.txt
_LIBRARY_SHAPES: frozenset = frozenset()


def _K():
    return _load_ext().se


def supported(C: int, Cr: int) -> bool:
    return bool(_K().supported(C, Cr))


def usable(u: torch.Tensor, C: int, Cr: int, cdtype: torch.dtype) -> bool:
    """Does the SE block of a [N, C, H, W] ``u`` with ``Cr`` hidden units run on the kernels?"""
    if not (ENABLED and u.is_cuda and u.dim() == 4 and u.shape[1] == C
            and cdtype in (torch.bfloat16, torch.float16) and u.dtype == cdtype):
        return False
    return supported(C, Cr) and (C, Cr, u.shape[2] * u.shape[3]) not in _LIBRARY_SHAPES


def _cl(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous(memory_format=_CL) else t.contiguous(memory_format=_CL)


class SqueezeExciteFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, identity, fc1_w, fc1_b, fc2_w, fc2_b, tap: GradTap | None = None):
        C, Cr = (u.shape[1], fc1_w.shape[0]) if u.dim() == 4 and fc1_w.dim() >= 2 else (0, 0)
        params = (fc1_w, fc1_b, fc2_w, fc2_b)
        if not (u.is_cuda and u.dtype in (torch.bfloat16, torch.float16) and identity.shape == u.shape
                and all(t.dtype == torch.float32 for t in params) and supported(C, Cr)
                and fc1_w.numel() == C * Cr and fc2_w.numel() == C * Cr and fc2_w.shape[0] == C
                and fc1_b.shape == (Cr,) and fc2_b.shape == (C,)):
            raise RuntimeError(f"squeeze_excite: no kernel for u {tuple(u.shape)} {u.dtype}, identity "
                               f"{tuple(identity.shape)}, fc1 {tuple(fc1_w.shape)} {fc1_w.dtype}, fc2 "
                               f"{tuple(fc2_w.shape)} {fc2_w.dtype}")
        u = _cl(u)
        identity = _cl(identity.to(u.dtype))
        w1, b1, w2, b2 = (t.detach().contiguous() for t in params)
        N = u.shape[0]
        f32 = dict(dtype=torch.float32, device=u.device)
        p, h, s = torch.empty(N, C, **f32), torch.empty(N, Cr, **f32), torch.empty(N, C, **f32)
        y = torch.empty_like(u, memory_format=_CL)
        _K().fwd(u, identity, w1, b1, w2, b2, p, h, s, y)
        ctx.save_for_backward(u, y, s, p, h, w1, w2)
        ctx.tap = tap
        return y

    @staticmethod
    def backward(ctx, g):
        u, y, s, p, h, w1, w2 = ctx.saved_tensors
        N, C = p.shape
        Cr = h.shape[1]
        g = _cl(g.to(u.dtype))
        f32 = dict(dtype=torch.float32, device=u.device)
        dz2, dz1 = torch.empty(N, C, **f32), torch.empty(N, Cr, **f32)
        dw1, db1 = torch.empty(w1.shape, **f32), torch.empty(Cr, **f32)
        dw2, db2 = torch.empty(w2.shape, **f32), torch.empty(C, **f32)
        du, did = torch.empty_like(u, memory_format=_CL), torch.empty_like(u, memory_format=_CL)
        _K().bwd(g, y, u, s, p, h, w1, w2, dz2, dz1, dw1, db1, dw2, db2, du, did)
        if ctx.tap is not None:  # d(identity) goes to the consumer's GEMM (ops/conv1x1.py GradTap)
            ctx.tap.grad, did = did, None
        return du, did, dw1, db1, dw2, db2, None


def squeeze_excite(u, identity, fc1_w, fc1_b, fc2_w, fc2_b, tap: GradTap | None = None) -> torch.Tensor:
    """relu(u * sigmoid(fc2(relu(fc1(mean_hw u)))) + identity) on the SE kernels; the weights may be
    2-D or 1x1-conv-shaped.  ``tap``: hand d(identity) to a GradTap instead of returning it, as
    ops/bn_nhwc.bn_act does.  Raises for a shape or dtype outside the supported set."""
    return SqueezeExciteFn.apply(u, identity, fc1_w, fc1_b, fc2_w, fc2_b, tap)


def squeeze_excite_torch(u, identity, fc1_w, fc1_b, fc2_w, fc2_b) -> torch.Tensor:
    """The same math as a torch composition (fp32 gate, one rounding of y): fp32, CPU, unsupported
    shapes and ``DPA_SE=0``."""
    C = u.shape[1]
    uf = u.float()
    h = F.relu(F.linear(uf.mean((2, 3)), fc1_w.reshape(-1, C).float(), fc1_b.float()))
    s = torch.sigmoid(F.linear(h, fc2_w.reshape(C, -1).float(), fc2_b.float()))
    return F.relu(uf * s[:, :, None, None] + identity.float()).to(u.dtype)


def last_launch() -> dict:
    """{family: ([C, Cr], dtype, calls)} of the kernels launched since clear_launches(); families:
    squeeze, fc1, excite (forward), excite_bwd_sums, gate_bwd, gate_wgrad, excite_bwd."""
    return dict(_K().last_launch())


def clear_launches() -> None:
    _K().clear_launches()
