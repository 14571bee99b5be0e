"""ResNet-50 (torchvision layout: same module tree, parameter names and
state_dict keys, 25,557,032 parameters) for the BASELINE.json stress config
"ResNet-50 on synthetic 3x224x224, world_size=8 AMP bf16 (stress MFMA conv +
all-reduce bucket fusion)".  The reference repository has no ResNet; the
architecture is He et al. 2015 with the v1.5 stride placement (stride on the
3x3 conv of each stage's first bottleneck), the variant torchvision ships.

Execution on a HIP device (``fused=True``): activations are bf16/f16/f32
``channels_last`` (NHWC in memory) end to end;
  * forward convolutions (1x1 and 3x3, any stride; C and Cout multiples of 64)
    run on the hand-written NHWC implicit-GEMM MFMA kernel, which also produces
    the following BatchNorm's batch statistics in its epilogue
    (csrc/kernels/conv_igemm.hip, ops/conv_igemm.py; DPA_IGEMM=0: library path);
  * the 7x7 / stride-2 stem (C = 3) runs on the same kernel's stem mode: the image
    is packed to 4-channel NHWC in one launch and the K space is (r, s, c) padded to
    8 x 8 x 4 (forward + statistics, and the weight gradient);
  * backward: every weight gradient and every 3x3 data gradient (stride 1, and
    stride 2 as four output-parity sub-convolutions) run on the implicit-GEMM
    kernel; 1x1 forwards and data gradients run on the glds-staged 1x1 GEMM kernel
    (conv_glds_kernel: 128-pixel tiles, operands global -> LDS by LDS-DMA).  A
    projection block's two input gradients (conv1 and downsample) are combined in
    the conv epilogue instead of by a separate add;
  * every BatchNorm runs on the native NHWC kernels with its ReLU and, for the
    last BN of a bottleneck, the residual add fused in (ops/bn_nhwc.py), as
    SyncBatchNorm when the module was converted (one small all-reduce each way);
  * the grouped 3x3 convs of ResNeXt (``groups`` / ``width_per_group``, resnext50_32x4d) run
    forward, data gradient and weight gradient on the block-diagonal grouped kernels
    (csrc/kernels/conv_group.hip, ops/conv_group.py; DPA_GCONV=0: library path); the BN
    that follows takes its own statistics pass;
  * a stride-1 1x1 conv whose C or Cout is no multiple of 64 (multiples of 8 up to 1024) runs
    forward, data gradient and weight gradient on the pointwise kernels
    (csrc/kernels/conv_pw.hip, ops/conv_pw.py; DPA_PWCONV=0: the torch.mm branch of ops/conv1x1.py);
  * squeeze-and-excitation (``se_reduction``; se_resnet50, se_resnext50_32x4d: Hu et al. 2018,
    timm's ``layerL.B.se.fc{1,2}`` keys): bn3 is applied without ReLU or residual, and the
    pool, the two fp32 gate layers (fp32 MFMA), the sigmoid, the channel scale, the residual add
    and the ReLU run in three launches forward and four backward (csrc/kernels/se.hip,
    ops/se.py; DPA_SE=0: a torch composition of the same math on the same convs).  An identity
    block's d(identity) still goes to conv1's data gradient through the GradTap; the block
    output is not a BN's, so the next block's conv1 takes no BNTap sums;
  * max-pool 3x3/2 and the global average pool are native kernels; fc runs on the
    native MFMA linear kernels (ops/head.py).
On CPU the plain torch modules run (the same math; the CPU test tier).
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..amp import autocast, compute_dtype
from ..ops import conv_dw as _dwconv
from ..ops import conv_group as _gconv
from ..ops import conv_igemm as _igemm
from ..ops import conv_pw as _pwconv
from ..ops import se as _se
from ..ops.conv1x1 import GradTap, conv1x1
from ..ops.conv_nhwc import conv_nhwc


_PACKS: dict = {}  # id(module) -> this forward's packed filters (ops/conv_igemm.WeightPack)
_FUSE_BN_BWD = os.environ.get("DPA_FUSE_BN_BWD", "1") != "0"  # BNTap hand-off (0: own bwd_stats pass, A/B)
# bn1 -> the 3x3 conv2's data gradient: off by default -- the 3x3 epilogue's extra cost
# (+281 us over 13 launches) cancels the bwd_stats pass it removes (-297 us),
# profiles/r3s2h_resnet50_steady_bn1_fused.txt
_FUSE_BN1 = os.environ.get("DPA_FUSE_BN1", "0") == "1"
# a projection block's downsample BN applied inside bn3's residual add (ops/bn_nhwc.bn_res_bn)
_FUSE_DS_BN = os.environ.get("DPA_FUSE_DS_BN", "1") != "0"


def _conv(x: torch.Tensor, conv: nn.Conv2d, cdtype: torch.dtype, bn: nn.Module | None = None, tap=None,
          xtap=None, btap=None):
    """conv(x) -> (output, statistics of the following training BN ``bn`` when the conv
    kernel produced them, else None).  ``btap``: the BNTap of the BN that produced ``x``
    (a 1x1 conv's data gradient then also takes that BN's backward sums)."""
    want = bn if (bn is not None and bn.training) else None
    pk = _PACKS.get(id(conv))
    if tap is None and xtap is None and _pwconv.usable(x, conv, cdtype):
        # 1x1 with C or K no multiple of 64 (the narrow MobileNet widths) on the pointwise MFMA kernels
        # instead of conv1x1's torch.mm branch.  Not done there: BN statistics in the epilogue (the BN
        # takes its own pass) and the BNTap hand-off (``btap`` stays unfilled: the BN runs bwd_stats)
        return _pwconv.conv_pw(x, conv.weight, cdtype), None
    if conv.kernel_size == (1, 1) and conv.padding == (0, 0) and conv.groups == 1 and conv.bias is None:
        if want is None:
            return conv1x1(x, conv.weight, conv.stride[0], cdtype, tap, None, pk, xtap, btap), None
        return conv1x1(x, conv.weight, conv.stride[0], cdtype, tap, want, pk, xtap, btap)
    if conv.bias is None and conv.groups == 1 and conv.dilation == (1, 1):
        if want is None:
            return conv_nhwc(x, conv.weight, conv.stride, conv.padding, cdtype, None, pk, btap), None
        return conv_nhwc(x, conv.weight, conv.stride, conv.padding, cdtype, want, pk, btap)
    if _gconv.usable(x, conv, cdtype):
        # grouped 3x3 (ResNeXt) on the block-diagonal MFMA kernels; the BN takes its own statistics
        return _gconv.conv_group(x, conv.weight, conv.stride[0], conv.groups, cdtype), None
    if _dwconv.usable(x, conv, cdtype):
        # depthwise 3x3 (MobileNet) / 5x5 (MnasNet) on the VALU granule kernels; the BN takes its own statistics
        return _dwconv.conv_dw(x, conv.weight, conv.stride[0], cdtype), None
    w = conv.weight.to(cdtype)
    out = F.conv2d(x, w, None if conv.bias is None else conv.bias.to(cdtype), conv.stride, conv.padding,
                   conv.dilation, conv.groups)
    return (out if out.is_contiguous(memory_format=torch.channels_last) else
            out.contiguous(memory_format=torch.channels_last)), None


def _multi_rank() -> bool:
    import torch.distributed as tdist

    from .. import distributed as ddist

    if tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
        return True
    try:
        return ddist.is_initialized() and ddist.get_world_size() > 1
    except Exception:  # noqa: BLE001 -- no facade state: a single process
        return False


def _comm_of(bn: nn.Module):
    from ..ops.bn_nhwc import bn_comm  # the same lookup the statistics-producing convs use

    return bn_comm(bn)


class SqueezeExcite(nn.Module):
    """x * sigmoid(fc2(relu(fc1(mean_hw x)))): two 1x1 convs with bias on the pooled vector."""

    def __init__(self, channels: int, reduction: int):
        super().__init__()
        self.fc1 = nn.Conv2d(channels, channels // reduction, kernel_size=1)
        self.fc2 = nn.Conv2d(channels // reduction, channels, kernel_size=1)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        s = F.relu(self.fc1(x.mean((2, 3), keepdim=True)))
        return x * torch.sigmoid(self.fc2(s))


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: nn.Module | None = None,
                 groups: int = 1, base_width: int = 64, se_reduction: int = 0):
        super().__init__()
        width = int(planes * base_width / 64) * groups  # torchvision's (ResNeXt: groups x base_width)
        self.conv1 = nn.Conv2d(inplanes, width, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, kernel_size=3, stride=stride, padding=1, groups=groups,
                               bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, planes * self.expansion, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        if se_reduction:
            self.se = SqueezeExcite(planes * self.expansion, se_reduction)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if hasattr(self, "se"):
            out = self.se(out)
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)

    def forward_native(self, x: torch.Tensor, cdtype: torch.dtype, bt_in=None):
        """Native block forward; returns (y, the BNTap of bn3 or None).  ``bt_in``: the
        previous block's bn3 tap (the BN that produced ``x``)."""
        from ..ops.bn_nhwc import BNTap, bn_act

        train = self.bn3.training and torch.is_grad_enabled()
        grad_x = train and x.requires_grad and x.is_contiguous(memory_format=torch.channels_last)
        # identity blocks: conv1's dgrad GEMM accumulates the residual gradient (GradTap);
        # projection blocks: conv1 and the downsample conv share x's gradient (one of them
        # folds the other's product into its own, ops/conv1x1.Conv1x1Fn)
        tap = GradTap() if (grad_x and self.downsample is None) else None
        xtap = GradTap() if (grad_x and self.downsample is not None) else None
        # BN backward sums taken by the consuming conv's data-gradient epilogue
        # (ops/bn_nhwc.BNTap): bn2 -> conv3, and the previous block's bn3 -> this conv1
        # when this is an identity block (its dgrad then holds the whole gradient of x);
        # bn1 -> conv2 (stride 1) with DPA_FUSE_BN1=1
        se = getattr(self, "se", None)
        bt_in = bt_in if (tap is not None and se is None) else None  # (an SE block's x is no BN's output)
        bt1 = BNTap() if train and _FUSE_BN1 and self.conv2.stride == (1, 1) else None
        bt2 = BNTap() if train and _FUSE_BN_BWD else None
        bt3 = BNTap() if train and _FUSE_BN_BWD else None
        # each conv hands the following BN its batch statistics (ops/conv_igemm.py)
        c1, st = _conv(x, self.conv1, cdtype, self.bn1, tap, xtap, bt_in)
        out = bn_act(c1, self.bn1, relu=True, comm=_comm_of(self.bn1), stats=st, btap=bt1)
        c2, st = _conv(out, self.conv2, cdtype, self.bn2, btap=bt1)
        out = bn_act(c2, self.bn2, relu=True, comm=_comm_of(self.bn2), stats=st, btap=bt2)
        identity = x
        cd = std = None
        if self.downsample is not None:
            conv, bn = self.downsample[0], self.downsample[1]
            cd, std = _conv(x, conv, cdtype, bn, None, xtap)
            if not _FUSE_DS_BN or se is not None:
                identity = bn_act(cd, bn, relu=False, comm=_comm_of(bn), stats=std)
        c3, st = _conv(out, self.conv3, cdtype, self.bn3, btap=bt2)
        if se is not None:
            # bn3 without ReLU or residual; the gate, the residual add and the ReLU on the SE kernels
            u = bn_act(c3, self.bn3, relu=False, comm=_comm_of(self.bn3), stats=st)
            gate = (se.fc1.weight, se.fc1.bias, se.fc2.weight, se.fc2.bias)
            if _se.usable(u, se.fc1.in_channels, se.fc1.out_channels, cdtype):
                return _se.squeeze_excite(u, identity, *gate, tap=tap), None
            return _se.squeeze_excite_torch(u, identity, *gate), None
        if cd is not None and _FUSE_DS_BN:
            # downsample BN applied inside the residual add (no normalised identity written)
            from ..ops.bn_nhwc import bn_res_bn

            y = bn_res_bn(c3, self.bn3, cd, self.downsample[1], comm=_comm_of(self.bn3), stats=st, rstats=std,
                          btap=bt3)
        else:
            y = bn_act(c3, self.bn3, res=identity, relu=True, comm=_comm_of(self.bn3), tap=tap, stats=st, btap=bt3)
        return y, bt3


class ResNet(nn.Module):
    def __init__(self, layers=(3, 4, 6, 3), num_classes: int = 1000, amp_dtype: torch.dtype | None = None,
                 fused: bool = True, groups: int = 1, width_per_group: int = 64, se_reduction: int = 0):
        super().__init__()
        self.inplanes = 64
        self.groups = groups
        self.se_reduction = se_reduction
        self.base_width = width_per_group
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(64, layers[0])
        self.layer2 = self._make_layer(128, layers[1], stride=2)
        self.layer3 = self._make_layer(256, layers[2], stride=2)
        self.layer4 = self._make_layer(512, layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512 * Bottleneck.expansion, num_classes)
        for m in self.modules():  # torchvision's initialisation
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        self.amp_dtype = amp_dtype
        self.fused = fused

    def _make_layer(self, planes: int, blocks: int, stride: int = 1) -> nn.Sequential:
        downsample = None
        if stride != 1 or self.inplanes != planes * Bottleneck.expansion:
            downsample = nn.Sequential(
                nn.Conv2d(self.inplanes, planes * Bottleneck.expansion, kernel_size=1, stride=stride, bias=False),
                nn.BatchNorm2d(planes * Bottleneck.expansion),
            )
        layers = [Bottleneck(self.inplanes, planes, stride, downsample, self.groups, self.base_width,
                             self.se_reduction)]
        self.inplanes = planes * Bottleneck.expansion
        layers += [Bottleneck(self.inplanes, planes, groups=self.groups, base_width=self.base_width,
                              se_reduction=self.se_reduction) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    # ------------------------------------------------------------------ paths
    def _native_ok(self, x: torch.Tensor) -> bool:
        if not (self.fused and x.is_cuda and x.dim() == 4):
            return False
        return all(m.affine and m.track_running_stats for m in self.modules()
                   if isinstance(m, nn.modules.batchnorm._BatchNorm))

    def _forward_torch(self, x: torch.Tensor) -> torch.Tensor:
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))

    def _forward_native(self, x: torch.Tensor) -> torch.Tensor:
        from ..ops.bn_nhwc import bn_act, global_avg_pool, max_pool_3x3s2

        cdtype = compute_dtype(x) if self.amp_dtype is not None else torch.float32
        _PACKS.clear()
        # the weight-gradient reductions of this step's backward in one launch, unless a DDP
        # reducer (or a peer rank) may read gradients while the backward still runs
        _igemm.WgradBatch.active = (torch.is_grad_enabled() and not getattr(self, "_dpa_ddp_wrapped", False)
                                    and not _multi_rank())
        if _igemm.ENABLED and cdtype in (torch.bfloat16, torch.float16):
            # every implicit-GEMM conv's filters for this step in one launch (with the flipped
            # transpose where the data gradient runs on the kernels: every 3x3, and the 1x1
            # convs ops/conv_igemm.dgrad_1x1_here selects -- all of them by default)
            pack = getattr(self, "_wpack", None)
            if pack is None or pack.cdtype != cdtype:
                convs = [(m, m.kernel_size == (3, 3) or _igemm.dgrad_1x1_here(m.weight.shape[0], 14))
                         for m in self.modules() if isinstance(m, nn.Conv2d) and m.bias is None and m.groups == 1
                         and m.weight.shape[0] % 64 == 0 and m.weight.shape[1] % 64 == 0]
                pack = self._wpack = _igemm.WeightPack(convs, cdtype)
            _PACKS.update(pack.run())
        if _igemm.stem_usable(x, self.conv1, cdtype):
            # 7x7 stem straight from the NCHW image (packed to 4-channel NHWC in-launch)
            c, st = _igemm.stem_conv(x, self.conv1, cdtype, self.bn1)
        else:
            x = x.to(dtype=cdtype, memory_format=torch.channels_last)
            c, st = _conv(x, self.conv1, cdtype, self.bn1)
        x = bn_act(c, self.bn1, relu=True, comm=_comm_of(self.bn1), stats=st)
        x = max_pool_3x3s2(x)
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            bt = None
            for blk in layer:
                x, bt = blk.forward_native(x, cdtype, bt)
        feat = global_avg_pool(x)
        if cdtype in (torch.bfloat16, torch.float16) and os.environ.get("DPA_NATIVE_FC", "1") != "0":
            # fc on the native MFMA linear kernels (ops/head.py: fp32 master weight read
            # in-kernel, fp32 weight / bias gradients) -- no hipBLASLt GEMM left in the step
            from ..ops.head import linear

            return linear(feat, self.fc.weight, self.fc.bias, cdtype)
        return F.linear(feat, self.fc.weight.to(cdtype), self.fc.bias.to(cdtype))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        native = self._native_ok(x)
        fwd = self._forward_native if native else self._forward_torch
        if self.amp_dtype is not None:
            with autocast(dtype=self.amp_dtype, device_type="cuda" if x.is_cuda else "cpu"):
                return fwd(x)
        return fwd(x)


def resnet50(num_classes: int = 1000, amp_dtype: torch.dtype | None = None, fused: bool = True) -> ResNet:
    return ResNet((3, 4, 6, 3), num_classes=num_classes, amp_dtype=amp_dtype, fused=fused)


def resnext50_32x4d(num_classes: int = 1000, amp_dtype: torch.dtype | None = None, fused: bool = True) -> ResNet:
    """ResNeXt-50 32x4d (Xie et al. 2017; torchvision's module tree and state_dict keys,
    25,028,904 parameters): the 3x3 convs are grouped, 32 groups of 4 / 8 / 16 / 32 channels."""
    return ResNet((3, 4, 6, 3), num_classes=num_classes, amp_dtype=amp_dtype, fused=fused, groups=32,
                  width_per_group=4)


def se_resnet50(num_classes: int = 1000, amp_dtype: torch.dtype | None = None, fused: bool = True) -> ResNet:
    """SE-ResNet-50 (Hu et al. 2018; 28,088,024 parameters): ResNet-50 with a squeeze-and-excitation
    gate of reduction 16 after every bn3, under timm's ``se.fc1`` / ``se.fc2`` keys."""
    return ResNet((3, 4, 6, 3), num_classes=num_classes, amp_dtype=amp_dtype, fused=fused, se_reduction=16)


def se_resnext50_32x4d(num_classes: int = 1000, amp_dtype: torch.dtype | None = None, fused: bool = True) -> ResNet:
    """SE-ResNeXt-50 32x4d (27,559,896 parameters): resnext50_32x4d with the same SE gates."""
    return ResNet((3, 4, 6, 3), num_classes=num_classes, amp_dtype=amp_dtype, fused=fused, groups=32,
                  width_per_group=4, se_reduction=16)
