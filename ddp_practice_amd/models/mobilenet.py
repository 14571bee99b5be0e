"""MobileNetV1 (Howard et al. 2017): a 3x3 / stride-2 stem and 13 depthwise-separable blocks
(depthwise 3x3 + BN + ReLU, pointwise 1x1 + BN + ReLU), global average pool, one linear layer;
4,231,976 parameters at width 1.0 and 1000 classes.  torchvision ships no V1, so the module
tree and the state_dict keys are the project's own: ``stem.0`` (conv) / ``stem.1`` (BN),
``blocks.{i}.dw`` / ``.bn1`` / ``.pw`` / ``.bn2`` and ``fc``.

Execution on a HIP device with bf16 / fp16 (``fused=True``): channels_last end to end;
  * every depthwise conv runs forward, data gradient and weight gradient on the depthwise
    kernels (csrc/kernels/conv_dw.hip, ops/conv_dw.py; DPA_DWCONV=0: library path); its BN takes
    its own statistics pass;
  * every pointwise conv with C and Cout multiples of 64 runs on ``conv1x1`` with the
    following BN's statistics from the conv epilogue, and its data gradient takes the depthwise
    BN's backward sums (ops/bn_nhwc.BNTap), as ``Bottleneck`` does for bn2 -> conv3;
  * every other pointwise conv (32 -> 64 at width 1.0; at ``width_mult`` 0.75 / 0.5 / 0.25 the
    24-, 48-, 96-, 16-, 32-, 8-channel ones) runs forward, data gradient and weight gradient on the
    pointwise kernels (csrc/kernels/conv_pw.hip, ops/conv_pw.py; DPA_PWCONV=0: the torch.mm branch
    of ``ops/conv1x1.py``); its BN takes its own statistics pass and bn1's BNTap is not consumed;
  * the stem (C = 3) goes through the existing fallback of ``models/resnet.py::_conv``;
  * every BN runs on the native NHWC kernels with its ReLU (SyncBatchNorm when converted), the
    pool is the native global average pool and fc runs on the native MFMA linear kernels.
On CPU, or with ``fused=False``, the plain torch modules run (the same math).
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..amp import autocast, compute_dtype
from ..ops import conv_igemm as _igemm
from .resnet import _FUSE_BN_BWD, _PACKS, _comm_of, _conv, _multi_rank

# (output channels, stride) of the 13 depthwise-separable blocks at width 1.0
_BLOCKS = ((64, 1), (128, 2), (128, 1), (256, 2), (256, 1), (512, 2), (512, 1), (512, 1), (512, 1), (512, 1),
           (512, 1), (1024, 2), (1024, 1))


def _width(c: int, mult: float) -> int:
    """``c`` scaled by the width multiplier, to a multiple of 8 (one granule of the depthwise kernels)."""
    return max(8, int(c * mult + 4) // 8 * 8)


class DepthwiseSeparable(nn.Module):
    def __init__(self, cin: int, cout: int, stride: int):
        super().__init__()
        self.dw = nn.Conv2d(cin, cin, kernel_size=3, stride=stride, padding=1, groups=cin, bias=False)
        self.bn1 = nn.BatchNorm2d(cin)
        self.pw = nn.Conv2d(cin, cout, kernel_size=1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = F.relu(self.bn1(self.dw(x)))
        return F.relu(self.bn2(self.pw(x)))

    def forward_native(self, x: torch.Tensor, cdtype: torch.dtype) -> torch.Tensor:
        from ..ops.bn_nhwc import BNTap, bn_act

        train = self.bn1.training and torch.is_grad_enabled()
        # bn1's backward sums taken by the pointwise conv's data-gradient epilogue
        bt = BNTap() if train and _FUSE_BN_BWD else None
        c, st = _conv(x, self.dw, cdtype, self.bn1)
        x = bn_act(c, self.bn1, relu=True, comm=_comm_of(self.bn1), stats=st, btap=bt)
        c, st = _conv(x, self.pw, cdtype, self.bn2, btap=bt)
        return bn_act(c, self.bn2, relu=True, comm=_comm_of(self.bn2), stats=st)


class MobileNetV1(nn.Module):
    def __init__(self, num_classes: int = 1000, amp_dtype: torch.dtype | None = None, fused: bool = True,
                 width_mult: float = 1.0):
        super().__init__()
        c = _width(32, width_mult)
        self.stem = nn.Sequential(nn.Conv2d(3, c, kernel_size=3, stride=2, padding=1, bias=False),
                                  nn.BatchNorm2d(c))
        blocks = []
        for cout, stride in _BLOCKS:
            blocks.append(DepthwiseSeparable(c, _width(cout, width_mult), stride))
            c = _width(cout, width_mult)
        self.blocks = nn.Sequential(*blocks)
        self.fc = nn.Linear(c, num_classes)
        for m in self.modules():  # ResNet's initialisation
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        self.amp_dtype = amp_dtype
        self.fused = fused

    def _native_ok(self, x: torch.Tensor) -> bool:
        if not (self.fused and x.is_cuda and x.dim() == 4):
            return False
        return all(m.affine and m.track_running_stats for m in self.modules()
                   if isinstance(m, nn.modules.batchnorm._BatchNorm))

    def _forward_torch(self, x: torch.Tensor) -> torch.Tensor:
        x = self.blocks(F.relu(self.stem(x)))
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(x, 1), 1))

    def _forward_native(self, x: torch.Tensor) -> torch.Tensor:
        from ..ops.bn_nhwc import bn_act, global_avg_pool

        cdtype = compute_dtype(x) if self.amp_dtype is not None else torch.float32
        _PACKS.clear()
        _igemm.WgradBatch.active = (torch.is_grad_enabled() and not getattr(self, "_dpa_ddp_wrapped", False)
                                    and not _multi_rank())
        if _igemm.ENABLED and cdtype in (torch.bfloat16, torch.float16):
            # the pointwise filters of this step in one launch (ops/conv_igemm.WeightPack), as ResNet
            pack = getattr(self, "_wpack", None)
            if pack is None or pack.cdtype != cdtype:
                convs = [(m, _igemm.dgrad_1x1_here(m.weight.shape[0], 14)) for m in self.modules()
                         if isinstance(m, nn.Conv2d) and m.groups == 1 and m.weight.shape[0] % 64 == 0
                         and m.weight.shape[1] % 64 == 0]
                pack = self._wpack = _igemm.WeightPack(convs, cdtype)
            _PACKS.update(pack.run())
        x = x.to(dtype=cdtype, memory_format=torch.channels_last)
        c, st = _conv(x, self.stem[0], cdtype, self.stem[1])
        x = bn_act(c, self.stem[1], relu=True, comm=_comm_of(self.stem[1]), stats=st)
        for blk in self.blocks:
            x = blk.forward_native(x, cdtype)
        feat = global_avg_pool(x)
        if cdtype in (torch.bfloat16, torch.float16) and os.environ.get("DPA_NATIVE_FC", "1") != "0":
            from ..ops.head import linear

            return linear(feat, self.fc.weight, self.fc.bias, cdtype)
        return F.linear(feat, self.fc.weight.to(cdtype), self.fc.bias.to(cdtype))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        fwd = self._forward_native if self._native_ok(x) else self._forward_torch
        if self.amp_dtype is not None:
            with autocast(dtype=self.amp_dtype, device_type="cuda" if x.is_cuda else "cpu"):
                return fwd(x)
        return fwd(x)


def mobilenet_v1(num_classes: int = 1000, amp_dtype: torch.dtype | None = None, fused: bool = True,
                 width_mult: float = 1.0) -> MobileNetV1:
    return MobileNetV1(num_classes=num_classes, amp_dtype=amp_dtype, fused=fused, width_mult=width_mult)
