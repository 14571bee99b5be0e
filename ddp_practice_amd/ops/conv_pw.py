"""Pointwise (1x1) convolution on the hand-written MFMA kernels (csrc/kernels/conv_pw.hip):
forward, data gradient and weight gradient of a channels_last bf16 / fp16 activation with the
fp32 master weight read in-kernel (no WeightPack entry, no cast launch).

Supported: 1x1, stride 1, padding 0, groups 1, no bias, C and K multiples of 8 in 8..1024, any
N, H, W >= 1.  The weight gradient is written as the fp32 ``[K, C, 1, 1]`` ``.grad`` (pixel-split
fp32 partials summed in a fixed order: no atomics, bit-stable from run to run).

Routing (``usable``): only the shapes the implicit-GEMM kernel refuses (C or K no multiple of 64),
which until now ran as ``torch.mm`` / ``torch.bmm`` in ops/conv1x1.py; every shape that kernel
serves stays where it is.  Not done: BN statistics in the epilogue (the following BatchNorm takes
its own statistics pass) and the GradTap / BNTap hand-offs (none is consumed).

``DPA_PWCONV=0`` sends every pointwise conv of models/resnet.py::_conv back to ``conv1x1`` (A/B).
"""
from __future__ import annotations

import os

import torch

from .._ext import load as _load_ext
from . import conv_igemm as _igemm
from .conv_igemm import _WgradWS

_CL = torch.channels_last
ENABLED = os.environ.get("DPA_PWCONV", "1") != "0"  # 0: the torch.mm / bmm branch of ops/conv1x1.py (A/B)

# (C, K, P) of shapes the measurements send back to the library (scripts/pwconv_bench.py,
# profiles/pwconv_bench.txt): 256 -> 120 at batch 128, 28 x 28 loses as a conv (155.5 against 104.8 us).
# The unit is a conv: 8 -> 16 / 112 x 112 and 96 -> 96 / 56 x 56 lose their weight gradient alone and win as
# a whole, so they stay.  Follow-up: a per-operation fallback (or a 32- / 96-wide weight-gradient block)
# would save 96 -> 96 about 28 us per step.  No other shape with C or K above 192 was measured.
_LIBRARY_SHAPES: frozenset = frozenset({(256, 120, 128 * 28 * 28)})


def _K():
    return _load_ext().conv_pw


def tile() -> tuple:
    """(pixel rows of a tile, output-channel block of the chunked regime and the weight gradient)."""
    return tuple(int(v) for v in _K().tile())


def supported(C: int, K: int) -> bool:
    return bool(_K().supported(C, K))


def wgrad_splits(P: int, K: int, C: int) -> int:
    """Pixel splits of the weight gradient over ``P`` pixel rows."""
    return int(_K().wgrad_splits(P, K, C))


def tiles_per_workgroup(P: int, Kc: int, Nc: int) -> int:
    """Pixel tiles one workgroup of the forward (Kc = C, Nc = K) / data gradient (Kc = K, Nc = C) walks."""
    return int(_K().tiles_per_workgroup(P, Kc, Nc))


def channel_block(Kc: int, Nc: int) -> int:
    """Output channels one workgroup of the forward (Kc = C, Nc = K) / data gradient (Kc = K, Nc = C) owns."""
    return int(_K().channel_block(Kc, Nc))


def chunk() -> int:
    """Reduction depth staged at once: a deeper conv (Kc above it) runs the chunked regime."""
    return int(_K().K_CHUNK)


def usable(x: torch.Tensor, conv, cdtype: torch.dtype) -> bool:
    """Does ``conv`` (an nn.Conv2d) of ``x`` run on the pointwise kernels?"""
    if not (ENABLED and x.is_cuda and x.dim() == 4 and cdtype in (torch.bfloat16, torch.float16)):
        return False
    if not (conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0) and conv.groups == 1
            and conv.bias is None and conv.weight.dtype == torch.float32):
        return False
    C, K = conv.in_channels, conv.out_channels
    if x.shape[1] != C or not supported(C, K) or bool(_igemm._K().supported(C, K)):
        return False
    return (C, K, x.shape[0] * x.shape[2] * x.shape[3]) not in _LIBRARY_SHAPES


class PointwiseConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, cdtype: torch.dtype):
        if not (x.is_cuda and cdtype in (torch.bfloat16, torch.float16) and weight.dtype == torch.float32
                and weight.dim() == 4 and x.dim() == 4 and tuple(weight.shape[1:]) == (x.shape[1], 1, 1)
                and supported(x.shape[1], weight.shape[0])):
            raise RuntimeError(f"conv_pw: no kernel for x {tuple(x.shape)} {cdtype}, weight "
                               f"{tuple(weight.shape)} {weight.dtype}")
        x = x.to(cdtype)
        x = x if x.is_contiguous(memory_format=_CL) else x.contiguous(memory_format=_CL)
        w = weight.detach().contiguous()
        N, _, H, W = x.shape
        y = torch.empty((N, w.shape[0], H, W), dtype=cdtype, device=x.device, memory_format=_CL)
        _K().fwd(x, w, y)
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.to(x.dtype)
        dy = dy if dy.is_contiguous(memory_format=_CL) else dy.contiguous(memory_format=_CL)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)  # channels_last, as x
            _K().dgrad(dy, w, dx)
        if ctx.needs_input_grad[1]:
            N, K, H, W = dy.shape
            sp = wgrad_splits(N * H * W, K, x.shape[1])
            dw = torch.empty(w.shape, dtype=torch.float32, device=w.device)
            _K().wgrad(dy, x, dw, _WgradWS.get(dy.device, sp * dw.numel()))
        return dx, dw, None


def conv_pw(x: torch.Tensor, weight: torch.Tensor, cdtype: torch.dtype) -> torch.Tensor:
    """Bias-free 1x1 / stride-1 conv of ``x`` with the fp32 ``weight`` [K, C, 1, 1]; returns a
    channels_last tensor in ``cdtype``.  Backward: dx (channels_last, ``cdtype``) and the fp32 OIHW
    weight gradient.  Raises for a shape outside the supported set."""
    return PointwiseConvFn.apply(x, weight, cdtype)


def last_launch() -> dict:
    """{family: ([C, K], dtype, calls)} of the kernels launched since clear_launches();
    families: fwd, dgrad, wgrad."""
    return dict(_K().last_launch())


def clear_launches() -> None:
    _K().clear_launches()
