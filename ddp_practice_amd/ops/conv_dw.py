"""Depthwise 3x3 (MobileNet) and 5x5 (MnasNet) convolution on the hand-written VALU kernels
(csrc/kernels/conv_dw.hip, conv_dw5.hip): forward, data gradient and weight gradient of a
channels_last bf16 / fp16 activation with the fp32 master weight read in-kernel.

Supported: 3x3 / padding 1 or 5x5 / padding 2, dilation 1, no bias, stride 1 or 2, groups == C == K
(channel multiplier 1), C a multiple of 8, any N, H, W >= 1.  The weight gradient is written as the
fp32 ``[C, 1, k, k]`` ``.grad`` (pixel-split fp32 partials summed in a fixed order: no atomics,
bit-stable from run to run).  The following BatchNorm takes its own statistics pass and no
GradTap / BNTap is consumed.

``DPA_DWCONV=0`` sends every depthwise conv of models/resnet.py::_conv to the library branch (A/B).
"""
from __future__ import annotations

import os

import torch

from .._ext import load as _load_ext
from .conv_igemm import _WgradWS

_CL = torch.channels_last
ENABLED = os.environ.get("DPA_DWCONV", "1") != "0"  # 0: library (MIOpen) depthwise conv (A/B)

# (ksize, C, stride, output side) of shapes the measurements send to the library; none:
# profiles/dwconv_bench.txt, profiles/dwconv5_bench.txt
_LIBRARY_SHAPES: frozenset = frozenset()


def _K(ksize: int = 3):
    if ksize not in (3, 5):
        raise RuntimeError(f"conv_dw: no {ksize}x{ksize} kernels")
    ext = _load_ext()
    return ext.conv_dw if ksize == 3 else ext.conv_dw5


def tile(stride: int = 1, ksize: int = 3) -> tuple:
    """(rows, columns) of the ``ksize`` kernels' output tile at ``stride``."""
    return tuple(int(v) for v in _K(ksize).tile(stride))


def supported(C: int, K: int, groups: int) -> bool:
    return bool(_K().supported(C, K, groups))


def wgrad_splits(N: int, OH: int, OW: int, C: int, stride: int, ksize: int = 3) -> int:
    """Pixel splits of the ``ksize`` weight gradient of an [N, C, OH, OW] output gradient."""
    return int(_K(ksize).wgrad_splits(N, OH, OW, C, stride))


def usable(x: torch.Tensor, conv, cdtype: torch.dtype) -> bool:
    """Does ``conv`` (an nn.Conv2d) of ``x`` run on the depthwise kernels?"""
    if not (ENABLED and x.is_cuda and x.dim() == 4 and cdtype in (torch.bfloat16, torch.float16)):
        return False
    k = conv.kernel_size[0]
    if not (conv.groups > 1 and conv.bias is None and conv.kernel_size in ((3, 3), (5, 5))
            and conv.padding == (k // 2, k // 2) and conv.dilation == (1, 1) and conv.stride in ((1, 1), (2, 2)) and conv.padding_mode == "zeros"
            and conv.weight.dtype == torch.float32):
        return False
    C, K, s = conv.in_channels, conv.out_channels, conv.stride[0]
    if x.shape[1] != C or not supported(C, K, conv.groups):
        return False
    return (k, C, s, (x.shape[2] - 1) // s + 1) not in _LIBRARY_SHAPES


class DepthwiseConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, stride: int, cdtype: torch.dtype):
        if not (x.is_cuda and cdtype in (torch.bfloat16, torch.float16) and weight.dtype == torch.float32
                and weight.dim() == 4 and x.dim() == 4 and tuple(weight.shape[1:]) in ((1, 3, 3), (1, 5, 5))
                and stride in (1, 2) and supported(x.shape[1], weight.shape[0], x.shape[1])):
            raise RuntimeError(f"conv_dw: no kernel for x {tuple(x.shape)} {cdtype}, weight "
                               f"{tuple(weight.shape)} {weight.dtype}, stride {stride}")
        x = x.to(cdtype)
        x = x if x.is_contiguous(memory_format=_CL) else x.contiguous(memory_format=_CL)
        w = weight.detach().contiguous()
        N, C, H, W = x.shape
        y = torch.empty((N, C, (H - 1) // stride + 1, (W - 1) // stride + 1), dtype=cdtype, device=x.device,
                        memory_format=_CL)
        _K(w.shape[2]).fwd(x, w, y, stride)
        ctx.save_for_backward(x, w)
        ctx.stride = stride
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        stride, ksize = ctx.stride, w.shape[2]
        dy = dy.to(x.dtype)
        dy = dy if dy.is_contiguous(memory_format=_CL) else dy.contiguous(memory_format=_CL)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)  # channels_last, as x
            _K(ksize).dgrad(dy, w, dx, stride)
        if ctx.needs_input_grad[1]:
            N, C, OH, OW = dy.shape
            sp = wgrad_splits(N, OH, OW, C, stride, ksize)
            dw = torch.empty(w.shape, dtype=torch.float32, device=w.device)
            _K(ksize).wgrad(dy, x, dw, stride, _WgradWS.get(dy.device, sp * dw.numel()))
        return dx, dw, None, None


def conv_dw(x: torch.Tensor, weight: torch.Tensor, stride: int, cdtype: torch.dtype) -> torch.Tensor:
    """Bias-free depthwise 3x3 / padding-1 or 5x5 / padding-2 conv of ``x`` with the fp32 ``weight``
    [C, 1, 3, 3] (conv_dw.hip) or [C, 1, 5, 5] (conv_dw5.hip); returns a channels_last tensor in ``cdtype``.  Backward: dx (channels_last, ``cdtype``) and the
    fp32 OIHW weight gradient.  Raises for a shape outside the supported set."""
    return DepthwiseConvFn.apply(x, weight, int(stride), cdtype)


def last_launch() -> dict:
    """{family: ([stride, C], dtype, calls)} of the kernels launched since clear_launches();
    families: fwd, dgrad, wgrad (3x3) and fwd5, dgrad5, wgrad5 (5x5)."""
    return {**_K(3).last_launch(), **_K(5).last_launch()}


def clear_launches() -> None:
    _K(3).clear_launches()
    _K(5).clear_launches()
