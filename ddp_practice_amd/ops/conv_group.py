"""Grouped 3x3 convolution (ResNeXt) on the hand-written block-diagonal MFMA kernels
(csrc/kernels/conv_group.hip): forward, data gradient and weight gradient of a
channels_last bf16 / fp16 activation with the fp32 master weight read in-kernel.

Supported: 3x3, padding 1, dilation 1, no bias, stride 1 or 2, C == K, groups > 1,
C / groups in {4, 8, 16, 32}, C a multiple of 64, any N, H, W >= 1.  The weight gradient is
written as the fp32 OIHW ``.grad`` (pixel-split fp32 partials summed in a fixed order: no
atomics, bit-stable from run to run).  The following BatchNorm takes its own statistics
pass and no GradTap / BNTap is consumed.

``DPA_GCONV=0`` sends every grouped conv of models/resnet.py to the library branch (A/B).
"""
from __future__ import annotations

import os

import torch

from .._ext import load as _load_ext
from .conv_igemm import _WgradWS

_CL = torch.channels_last
ENABLED = os.environ.get("DPA_GCONV", "1") != "0"  # 0: library (MIOpen) grouped conv (A/B)

# (C, Cg, stride, output side) of shapes the measurements send to the library; none:
# profiles/gconv_bench.txt
_LIBRARY_SHAPES: frozenset = frozenset()


def _K():
    return _load_ext().conv_group


def tile() -> tuple:
    """(rows, pixels per row) of the kernels' output tile."""
    return int(_K().TILE_H), int(_K().TILE_W)


def supported(C: int, K: int, groups: int) -> bool:
    return bool(_K().supported(C, K, groups))


def usable(x: torch.Tensor, conv, cdtype: torch.dtype) -> bool:
    """Does ``conv`` (an nn.Conv2d) of ``x`` run on the grouped kernels?"""
    if not (ENABLED and x.is_cuda and x.dim() == 4 and cdtype in (torch.bfloat16, torch.float16)):
        return False
    if not (conv.groups > 1 and conv.bias is None and conv.kernel_size == (3, 3) and conv.padding == (1, 1)
            and conv.dilation == (1, 1) and conv.stride in ((1, 1), (2, 2)) and conv.padding_mode == "zeros"
            and conv.weight.dtype == torch.float32):
        return False
    C, K, s = conv.in_channels, conv.out_channels, conv.stride[0]
    if x.shape[1] != C or not supported(C, K, conv.groups):
        return False
    return (C, C // conv.groups, s, (x.shape[2] - 1) // s + 1) not in _LIBRARY_SHAPES


class ConvGroupFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, stride: int, groups: int, cdtype: torch.dtype):
        if not (x.is_cuda and cdtype in (torch.bfloat16, torch.float16) and weight.dtype == torch.float32
                and weight.dim() == 4 and x.dim() == 4 and supported(x.shape[1], weight.shape[0], groups)):
            raise RuntimeError(f"conv_group: no kernel for x {tuple(x.shape)} {cdtype}, weight "
                               f"{tuple(weight.shape)} {weight.dtype}, groups {groups}")
        x = x.to(cdtype)
        x = x if x.is_contiguous(memory_format=_CL) else x.contiguous(memory_format=_CL)
        w = weight.detach().contiguous()
        N, C, H, W = x.shape
        y = torch.empty((N, C, (H - 1) // stride + 1, (W - 1) // stride + 1), dtype=cdtype, device=x.device,
                        memory_format=_CL)
        _K().fwd(x, w, y, stride, groups)
        ctx.save_for_backward(x, w)
        ctx.conf = (stride, groups)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        stride, groups = ctx.conf
        dy = dy.to(x.dtype)
        dy = dy if dy.is_contiguous(memory_format=_CL) else dy.contiguous(memory_format=_CL)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)  # channels_last, as x
            _K().dgrad(dy, w, dx, stride, groups)
        if ctx.needs_input_grad[1]:
            N, C, OH, OW = dy.shape
            sp = int(_K().wgrad_splits(N, OH, OW, C, C // groups, stride))
            dw = torch.empty(w.shape, dtype=torch.float32, device=w.device)
            _K().wgrad(dy, x, dw, stride, groups, _WgradWS.get(dy.device, sp * dw.numel()))
        return dx, dw, None, None, None


def conv_group(x: torch.Tensor, weight: torch.Tensor, stride: int, groups: int, cdtype: torch.dtype) -> torch.Tensor:
    """Bias-free grouped 3x3 / padding-1 conv of ``x`` with the fp32 ``weight`` [K, C / groups, 3, 3];
    returns a channels_last tensor in ``cdtype``.  Backward: dx (channels_last, ``cdtype``) and the
    fp32 OIHW weight gradient.  Raises for a shape outside the supported set."""
    return ConvGroupFn.apply(x, weight, int(stride), int(groups), cdtype)


def last_launch() -> dict:
    """{family: ([stride, Cg], dtype, calls)} of the kernels launched since clear_launches();
    families: fwd, dgrad, wgrad."""
    return dict(_K().last_launch())


def clear_launches() -> None:
    _K().clear_launches()
