"""MnasNet-B1 at depth multiplier 1.0 (Tan et al. 2019) in torchvision's ``mnasnet1_0`` layout
(module tree and state_dict keys): a 3x3 / stride-2 stem, a depthwise-separable layer, six stacks
of inverted residuals (1x1 expand, depthwise 3x3 or 5x5, 1x1 project; the input added when the
shape allows), a 1x1 conv to 1280 channels, global average pool, dropout and one linear layer;
4,383,312 parameters at 1000 classes.  Plain ReLU, no squeeze-and-excitation.

Execution on a HIP device with bf16 / fp16 (``fused=True``): channels_last end to end;
  * the ten 5x5 depthwise convs run forward, data gradient and weight gradient on
    csrc/kernels/conv_dw5.hip, the seven 3x3 ones on conv_dw.hip (ops/conv_dw.py; DPA_DWCONV=0:
    library path); their BNs take their own statistics pass;
  * every 1x1 conv goes through ``models/resnet.py::_conv``: conv1x1 with the following BN's
    statistics from the epilogue where C and Cout are multiples of 64 (and the depthwise BN's
    backward sums through a BNTap), the pointwise kernels (ops/conv_pw.py) for the others;
  * every BN runs on the native NHWC kernels: expand and depthwise BNs with their ReLU, the project
    BN without, and with the block's input as its residual where the block has one;
  * the pool is the native global average pool, the dropout is ``F.dropout`` on the pooled
    [N, 1280] vector and the classifier runs on the native MFMA linear kernels.
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

_BN_MOMENTUM = 1 - 0.9997
# (input channels, output channels, depthwise kernel, stride, expansion, repeats) of the six stacks
_STACKS = ((16, 24, 3, 2, 3, 3), (24, 40, 5, 2, 3, 3), (40, 80, 5, 2, 6, 3), (80, 96, 3, 1, 6, 2),
           (96, 192, 5, 2, 6, 4), (192, 320, 3, 1, 6, 1))


def _bn(c: int) -> nn.BatchNorm2d:
    return nn.BatchNorm2d(c, momentum=_BN_MOMENTUM)


class InvertedResidual(nn.Module):
    def __init__(self, cin: int, cout: int, kernel: int, stride: int, expansion: int):
        super().__init__()
        mid = cin * expansion
        self.apply_residual = cin == cout and stride == 1
        self.layers = nn.Sequential(
            nn.Conv2d(cin, mid, 1, bias=False), _bn(mid), nn.ReLU(inplace=True),
            nn.Conv2d(mid, mid, kernel, padding=kernel // 2, stride=stride, groups=mid, bias=False), _bn(mid),
            nn.ReLU(inplace=True),
            nn.Conv2d(mid, cout, 1, bias=False), _bn(cout))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.layers(x) + x if self.apply_residual else self.layers(x)

    def forward_native(self, x: torch.Tensor, cdtype: torch.dtype) -> torch.Tensor:
        from ..ops.bn_nhwc import BNTap, bn_act

        L = self.layers
        train = L[4].training and torch.is_grad_enabled()
        # the depthwise BN's backward sums taken by the project conv's data-gradient epilogue
        bt = BNTap() if train and _FUSE_BN_BWD else None
        c, st = _conv(x, L[0], cdtype, L[1])
        y = bn_act(c, L[1], relu=True, comm=_comm_of(L[1]), stats=st)
        c, st = _conv(y, L[3], cdtype, L[4])
        y = bn_act(c, L[4], relu=True, comm=_comm_of(L[4]), stats=st, btap=bt)
        c, st = _conv(y, L[6], cdtype, L[7], btap=bt)
        return bn_act(c, L[7], res=x if self.apply_residual else None, relu=False, comm=_comm_of(L[7]), stats=st)


def _stack(cin: int, cout: int, kernel: int, stride: int, expansion: int, repeats: int) -> nn.Sequential:
    blocks = [InvertedResidual(cin, cout, kernel, stride, expansion)]
    blocks += [InvertedResidual(cout, cout, kernel, 1, expansion) for _ in range(repeats - 1)]
    return nn.Sequential(*blocks)


class MNASNet(nn.Module):
    def __init__(self, num_classes: int = 1000, dropout: float = 0.2, amp_dtype: torch.dtype | None = None,
                 fused: bool = True):
        super().__init__()
        layers = [nn.Conv2d(3, 32, 3, padding=1, stride=2, bias=False), _bn(32), nn.ReLU(inplace=True),
                  nn.Conv2d(32, 32, 3, padding=1, stride=1, groups=32, bias=False), _bn(32), nn.ReLU(inplace=True),
                  nn.Conv2d(32, 16, 1, bias=False), _bn(16)]
        layers += [_stack(*s) for s in _STACKS]
        layers += [nn.Conv2d(320, 1280, 1, bias=False), _bn(1280), nn.ReLU(inplace=True)]
        self.layers = nn.Sequential(*layers)
        self.classifier = nn.Sequential(nn.Dropout(p=dropout, inplace=True), nn.Linear(1280, num_classes))
        for m in self.modules():  # as models/mobilenet.py
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
        return self.classifier(self.layers(x).mean([2, 3]))

    def _forward_native(self, x: torch.Tensor) -> torch.Tensor:
        from ..ops.bn_nhwc import BNTap, bn_act, global_avg_pool

        cdtype = compute_dtype(x) if self.amp_dtype is not None else torch.float32
        _PACKS.clear()
        _igemm.WgradBatch.active = (torch.is_grad_enabled() and not getattr(self, "_dpa_ddp_wrapped", False)
                                    and not _multi_rank())
        if _igemm.ENABLED and cdtype in (torch.bfloat16, torch.float16):
            # the 64-multiple pointwise filters of this step in one launch (ops/conv_igemm.WeightPack)
            pack = getattr(self, "_wpack", None)
            if pack is None or pack.cdtype != cdtype:
                convs = [(m, _igemm.dgrad_1x1_here(m.weight.shape[0], 14)) for m in self.modules()
                         if isinstance(m, nn.Conv2d) and m.groups == 1 and m.weight.shape[0] % 64 == 0
                         and m.weight.shape[1] % 64 == 0]
                pack = self._wpack = _igemm.WeightPack(convs, cdtype)
            _PACKS.update(pack.run())
        L = self.layers
        train = L[4].training and torch.is_grad_enabled()
        x = x.to(dtype=cdtype, memory_format=torch.channels_last)
        c, st = _conv(x, L[0], cdtype, L[1])
        x = bn_act(c, L[1], relu=True, comm=_comm_of(L[1]), stats=st)
        bt = BNTap() if train and _FUSE_BN_BWD else None
        c, st = _conv(x, L[3], cdtype, L[4])
        x = bn_act(c, L[4], relu=True, comm=_comm_of(L[4]), stats=st, btap=bt)
        c, st = _conv(x, L[6], cdtype, L[7], btap=bt)
        x = bn_act(c, L[7], relu=False, comm=_comm_of(L[7]), stats=st)
        for stack in L[8:14]:
            for blk in stack:
                x = blk.forward_native(x, cdtype)
        c, st = _conv(x, L[14], cdtype, L[15])
        x = bn_act(c, L[15], relu=True, comm=_comm_of(L[15]), stats=st)
        feat = F.dropout(global_avg_pool(x), p=self.classifier[0].p, training=self.training)
        fc = self.classifier[1]
        if cdtype in (torch.bfloat16, torch.float16) and os.environ.get("DPA_NATIVE_FC", "1") != "0":
            from ..ops.head import linear

            return linear(feat, fc.weight, fc.bias, cdtype)
        return F.linear(feat, fc.weight.to(cdtype), fc.bias.to(cdtype))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        fwd = self._forward_native if self._native_ok(x) else self._forward_torch
        if self.amp_dtype is not None:
            with autocast(dtype=self.amp_dtype, device_type="cuda" if x.is_cuda else "cpu"):
                return fwd(x)
        return fwd(x)


def mnasnet1_0(num_classes: int = 1000, amp_dtype: torch.dtype | None = None, fused: bool = True,
               dropout: float = 0.2) -> MNASNet:
    return MNASNet(num_classes=num_classes, dropout=dropout, amp_dtype=amp_dtype, fused=fused)
