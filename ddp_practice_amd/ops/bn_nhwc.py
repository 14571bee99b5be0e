"""Channels-last BatchNorm (+ residual add) (+ ReLU), max-pool 3x3/2 and global
average pool on the native kernels of csrc/kernels/bn_nhwc.hip.

Used by the ResNet-50 stress model (models/resnet.py, BASELINE.json config 5).
Activations are NCHW-shaped ``torch.channels_last`` tensors (NHWC in memory),
the layout MIOpen / hipBLASLt consume for the convolutions.  BatchNorm follows
torch semantics (batch stats, biased var for normalisation, unbiased var into
running_var, momentum / cumulative average) and SyncBatchNorm semantics when a
communicator is active: ONE all-reduce of [sum, sum_sq, count] (2C+1 floats)
forward and of [sum dz, sum dz*xhat] (2C) backward, d(gamma) / d(beta) from the
local sums (torch/nn/modules/_functions.py:10-205).  With the communicator's xGMI
engine up (:func:`sync_site`) that all-reduce runs INSIDE the kernel that finishes the
statistics (the last arriver of each channel slice exchanges its slice with the peers,
csrc/comm/xsite.h positioned form): no collective launch between producer and consumer.
"""
from __future__ import annotations

import os
import weakref

import torch

from .._ext import load as _load_ext

_CL = torch.channels_last


def _K():
    return _load_ext().bn_nhwc


class _Workspace:
    """Per-device partial-sum rows + the statistics kernels' tickets (stream-ordered reuse)."""

    _by_dev: dict = {}

    @classmethod
    def get(cls, dev: torch.device, C: int):
        K = _K()
        ws = cls._by_dev.get(dev)
        need = int(K.MAX_PARTIAL_ROWS) * 2 * C
        if ws is None or ws[0].numel() < need:
            part = torch.empty(max(need, int(K.MAX_PARTIAL_ROWS) * 2 * 2048), dtype=torch.float32, device=dev)
            tickets = torch.zeros(int(K.MAX_TICKETS), dtype=torch.int32, device=dev)
            ws = cls._by_dev[dev] = (part, tickets)
        return ws


def bn_comm(bn):
    """The communicator a training BatchNorm module synchronises over (None: local BN)."""
    if not bn.training:
        return None
    if isinstance(bn, torch.nn.SyncBatchNorm):
        from ..parallel.comm import default_comm

        return default_comm()
    return getattr(bn, "comm", None)


def sync_site(comm):
    """The xGMI engine whose wide site (csrc/comm/xsite.h kSiteWide) the statistics
    finishers exchange SyncBN sums through, or None: an all-reduce launch follows each
    statistics launch.  Producer (ops/conv_igemm.conv_fwd, dgrad_bn) and consumer (the BN
    functions here) both decide with this function on the same communicator.

    Only the finisher workgroups of a launch wait for the peers (at most a few dozen), so
    there is no residency condition; ranks sharing one GPU beyond two take the launch path
    unless DPA_FUSED_SYNC=1 (as ops/convnet_fused._fused_site_engine); DPA_FUSED_SYNC=0
    forces the launch path (A/B)."""
    if comm is None or not comm.active:
        return None
    flag = os.environ.get("DPA_FUSED_SYNC")
    if flag == "0":
        return None
    if flag != "1" and os.environ.get("DPA_SHARED_GPU") == "1" and getattr(comm, "world_size", 1) > 2:
        return None
    return getattr(comm, "xgmi", None)


def _cl(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous(memory_format=_CL) else t.contiguous(memory_format=_CL)


class BNTap:
    """Hand-off of a training BatchNorm's backward sums from the 1x1 conv that consumes its
    output (ops/conv1x1.py): that conv's data-gradient kernel produces dy for this BN, and
    its epilogue also takes S1 = sum dz, S2 = sum dz * xhat (csrc/kernels/conv_igemm.hip,
    BS epilogue), so the backward here skips its bwd_stats pass over dy / x (/ y).

    The forward binds the BN's autograd node (``bind``): x and y (act 1: the ReLU follows a
    residual add) are read back from that node's saved tensors through a weak reference, so
    the tap holds no activation and forms no reference cycle with the BN's own output (the
    output -> grad_fn -> tap -> output cycle kept activations alive until the cycle collector
    ran when no backward followed).  The conv's backward sets ``sums`` = (out,
    dgamma, dbeta) and ``grad_ptr`` / ``grad_ver`` = the gradient it wrote and its version;
    the BN backward uses the sums only when dy is that tensor, unmodified (autograd adds a
    second consumer's gradient in place, which keeps the pointer but bumps the version).
    """

    __slots__ = ("_node", "_ix", "_iy", "act", "save", "weight", "bias", "sums", "grad_ptr", "grad_ver", "xc")

    def __init__(self):
        self._node = None
        self._ix = self._iy = -1
        self.save = self.weight = self.bias = self.sums = None
        self.act = 0
        self.grad_ptr = 0
        self.grad_ver = -1
        self.xc = None  # the BN's SyncBN site engine (sync_site): the conv's sums leave global

    def bind(self, ctx, ix: int, iy: int, act: int, save, weight, bias, xc=None) -> None:
        """``ctx``: the BN's autograd node; ``ix`` / ``iy``: positions of x / y in its saved
        tensors (``iy`` -1: y not needed); ``xc``: the BN's :func:`sync_site`."""
        self._node = weakref.ref(ctx)
        self._ix, self._iy = ix, iy
        self.act, self.save, self.weight, self.bias = act, save, weight, bias
        self.sums = None
        self.xc = xc

    def bind_tensors(self, x, y, act: int, save, weight, bias, xc=None) -> None:
        """Direct binding (kernel tests, no autograd node): holds x / y strongly."""
        held = type("_Held", (), {"saved_tensors": (x, y)})()
        self._node = lambda: held
        self._ix, self._iy = 0, (1 if y is not None else -1)
        self.act, self.save, self.weight, self.bias = act, save, weight, bias
        self.sums = None
        self.xc = xc

    def _saved(self, i: int):
        node = self._node() if self._node is not None else None
        if node is None or i < 0:
            return None
        return node.saved_tensors[i]

    @property
    def x(self):
        return self._saved(self._ix)

    @property
    def y(self):
        return self._saved(self._iy)

    def matches(self, dy: torch.Tensor) -> bool:
        """The consumer's sums are valid for ``dy``: same tensor, not modified since."""
        return self.sums is not None and self.grad_ptr == dy.data_ptr() and self.grad_ver == dy._version

    def clear(self):
        self._node = None
        self.save = self.weight = self.bias = self.sums = self.xc = None


def _batch_stats(K, x, C, running_mean, nbt, pre, xc, ws=None):
    """The forward statistics tensor of ``x``: ``pre`` when the producing conv's epilogue already
    computed it (ops/conv_igemm.py), else one fwd_stats launch (``ws``: the workspace, fetched
    when None).  The SyncBN all-reduce (no site exchange, ``xc`` None) is the caller's."""
    if pre is not None:
        return pre
    part, ticket = ws if ws is not None else _Workspace.get(x.device, C)
    stats = torch.empty(3 * C + 4, dtype=torch.float32, device=x.device)
    K.fwd_stats(x, C, running_mean, part, ticket, stats, nbt, xc=xc)
    return stats


def _backward_sums(ctx, K, dy, y, x, act, save, weight, bias):
    """(sums, dgamma, dbeta) of a training BN's backward: the sums its tap holds for this ``dy``
    (taken by the consumer conv's data-gradient epilogue) or one bwd_stats launch; the tap is
    cleared; ``sums`` all-reduced unless the finishers exchanged them (ctx.xc)."""
    C = x.shape[1]
    f32 = dict(dtype=torch.float32, device=x.device)
    bt = getattr(ctx, "btap", None)
    if bt is not None and bt.matches(dy):
        out, dgamma, dbeta = bt.sums
    else:
        part, ticket = _Workspace.get(x.device, C)
        out, dgamma, dbeta = torch.empty(2 * C, **f32), torch.empty(C, **f32), torch.empty(C, **f32)
        K.bwd_stats(dy, y, x, C, act, save, weight, bias, part, ticket, out, dgamma, dbeta, xc=ctx.xc)
    if bt is not None:
        bt.clear()
        ctx.btap = None
    # out is already global when the finishers exchanged it (ctx.xc)
    sums = ctx.comm.all_reduce(out) if (ctx.sync and ctx.xc is None) else out
    return sums, dgamma, dbeta


class BNActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, res, running_mean, running_var, nbt, momentum, eps, training, relu, comm,
                tap=None, pre=None, btap=None):
        K = _K()
        x = _cl(x)
        C = x.shape[1]
        dev = x.device
        y = torch.empty_like(x, memory_format=_CL)
        resc = _cl(res) if res is not None else None
        mom = -1.0 if momentum is None else float(momentum)
        f32 = dict(dtype=torch.float32, device=dev)
        if training:
            sync = comm is not None and comm.active
            xc = sync_site(comm)  # SyncBN inside the statistics finishers (also the producing conv's)
            stats = _batch_stats(K, x, C, running_mean, nbt, pre, xc)
            if sync and xc is None:
                comm.all_reduce_(stats.narrow(0, 0, 2 * C + 1))
            save = torch.empty(2 * C, **f32)
            K.apply(x, resc, y, C, stats, weight, bias, running_mean, running_var, nbt, mom, float(eps), True,
                    relu, save)
            # ReLU derivative: from y after a residual add, else recomputed from x (y not kept)
            ctx.act = (1 if res is not None else 2) if relu else 0
            ctx.save_for_backward(x, y if ctx.act == 1 else None, weight, bias, save, stats)
            ctx.sync, ctx.comm, ctx.xc, ctx.has_res = sync, comm, xc, res is not None
            ctx.tap = tap if res is not None else None
            ctx.btap = btap if ctx.act in (1, 2) else None
            if ctx.btap is not None:
                ctx.btap.bind(ctx, 0, 1 if ctx.act == 1 else -1, ctx.act, save, weight, bias, xc)
        else:
            dummy = torch.empty(2 * C + 1, **f32)
            K.apply(x, resc, y, C, dummy, weight, bias, running_mean, running_var, nbt, mom, float(eps), False,
                    relu, dummy)
            ctx.sync = None
        return y

    @staticmethod
    def backward(ctx, dy):
        if ctx.sync is None:
            raise RuntimeError("BNActFn: backward through an eval-mode BatchNorm is not supported")
        K = _K()
        x, y, weight, bias, save, stats = ctx.saved_tensors
        C = x.shape[1]
        dy = _cl(dy)
        sums, dgamma, dbeta = _backward_sums(ctx, K, dy, y, x, ctx.act, save, weight, bias)
        dx = torch.empty_like(x, memory_format=_CL)
        dres = torch.empty_like(x, memory_format=_CL) if ctx.has_res else None
        K.bwd_elemt(dy, y, x, C, ctx.act, save, sums, stats, weight, bias, dx, dres)
        if ctx.tap is not None:  # d(res) goes to the consumer's GEMM (ops/conv1x1.py GradTap)
            ctx.tap.grad, dres = dres, None
        return dx, dgamma, dbeta, dres, None, None, None, None, None, None, None, None, None, None, None


def bn_act(x, bn, res=None, relu=True, comm=None, tap=None, stats=None, btap=None):
    """BatchNorm module ``bn`` applied to channels_last ``x`` (+ res) (+ ReLU).
    ``tap``: hand d(res) to a GradTap instead of returning it (ops/conv1x1.py).
    ``stats``: the batch statistics already computed by the producing conv
    (ops/conv_igemm.py; training only) -- no statistics pass here.
    ``btap``: a :class:`BNTap` the consuming 1x1 conv fills with this BN's backward sums."""
    return BNActFn.apply(x, bn.weight, bn.bias, res, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                         bn.momentum, bn.eps, bn.training, relu, comm if bn.training else None, tap,
                         stats if bn.training else None, btap if bn.training else None)


# the downsample BN's backward sums inside bn3's elementwise pass: measured slower (14.79-14.80 vs
# 14.69-14.75 ms, profiles/r3s2s_resnet50_rbn_sums_rejected.jsonl), opt-in
_FUSE_RBN_SUMS = os.environ.get("DPA_FUSE_RBN_SUMS", "0") == "1"


class BNResBNFn(torch.autograd.Function):
    """relu(bn(x) + bn_r(r)): a projection bottleneck's last BatchNorm with the downsample
    conv's BatchNorm applied to the residual in the same pass (csrc/kernels/bn_nhwc.hip
    apply_resbn_kernel) -- the normalised identity is never written.  Backward: bn's
    backward (ReLU mask from y) gives dx and dz = d(bn_r output), then bn_r's backward
    (no ReLU) on dz, on the same kernels as two BNActFn backwards."""

    @staticmethod
    def forward(ctx, x, weight, bias, r, rweight, rbias, bn, rbn, comm, pre, rpre, btap):
        K = _K()
        x, r = _cl(x), _cl(r)
        C = x.shape[1]
        dev = x.device
        f32 = dict(dtype=torch.float32, device=dev)
        y = torch.empty_like(x, memory_format=_CL)
        training = bn.training
        stats = rstats = None
        xc = None
        if training:
            sync = comm is not None and comm.active
            xc = sync_site(comm)
            ws = _Workspace.get(dev, C)
            stats = _batch_stats(K, x, C, bn.running_mean, bn.num_batches_tracked, pre, xc, ws)
            rstats = _batch_stats(K, r, C, rbn.running_mean, rbn.num_batches_tracked, rpre, xc, ws)
            if sync and xc is None:
                comm.all_reduce_(stats.narrow(0, 0, 2 * C + 1))
                comm.all_reduce_(rstats.narrow(0, 0, 2 * C + 1))
        else:
            sync = False
            stats = rstats = torch.empty(3 * C + 4, **f32)  # unused in eval
        save, rsave = torch.empty(2 * C, **f32), torch.empty(2 * C, **f32)
        mom = -1.0 if bn.momentum is None else float(bn.momentum)
        rmom = -1.0 if rbn.momentum is None else float(rbn.momentum)
        K.apply_resbn(x, r, y, C, stats, weight, bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, mom,
                      float(bn.eps), save, rstats, rweight, rbias, rbn.running_mean, rbn.running_var,
                      rbn.num_batches_tracked, rmom, float(rbn.eps), rsave, training)
        ctx.training = training
        if training:
            ctx.save_for_backward(x, y, weight, bias, save, stats, r, rweight, rbias, rsave, rstats)
            ctx.sync, ctx.comm, ctx.xc = sync, comm, xc
            ctx.btap = btap
            if btap is not None:
                btap.bind(ctx, 0, 1, 1, save, weight, bias, xc)
        return y

    @staticmethod
    def backward(ctx, dy):
        if not ctx.training:
            raise RuntimeError("BNResBNFn: backward through an eval-mode BatchNorm is not supported")
        K = _K()
        x, y, weight, bias, save, stats, r, rweight, rbias, rsave, rstats = ctx.saved_tensors
        C = x.shape[1]
        dy = _cl(dy)
        f32 = dict(dtype=torch.float32, device=x.device)
        part, ticket = _Workspace.get(x.device, C)
        sums, dgamma, dbeta = _backward_sums(ctx, K, dy, y, x, 1, save, weight, bias)
        dx = torch.empty_like(x, memory_format=_CL)
        dz = torch.empty_like(x, memory_format=_CL)
        # bn's elementwise backward, which also takes the downsample BN's sums of dz
        rout, rdgamma, rdbeta = torch.empty(2 * C, **f32), torch.empty(C, **f32), torch.empty(C, **f32)
        if _FUSE_RBN_SUMS:
            K.bwd_elemt_rbn(dy, y, x, C, save, sums, stats, weight, bias, dx, dz, r, rsave, part, ticket, rout,
                            rdgamma, rdbeta)
        else:  # A/B: the elementwise pass, then the downsample BN's own statistics pass
            K.bwd_elemt(dy, y, x, C, 1, save, sums, stats, weight, bias, dx, dz)
            K.bwd_stats(dz, None, r, C, 0, rsave, rweight, rbias, part, ticket, rout, rdgamma, rdbeta, xc=ctx.xc)
        # the downsample BN (no ReLU) on dz (rout global when bwd_stats exchanged it)
        rsums = ctx.comm.all_reduce(rout) if (ctx.sync and (ctx.xc is None or _FUSE_RBN_SUMS)) else rout
        dr = torch.empty_like(r, memory_format=_CL)
        K.bwd_elemt(dz, None, r, C, 0, rsave, rsums, rstats, rweight, rbias, dr, None)
        return dx, dgamma, dbeta, dr, rdgamma, rdbeta, None, None, None, None, None, None


def bn_res_bn(x, bn, r, rbn, comm=None, stats=None, rstats=None, btap=None):
    """relu(bn(x) + rbn(r)) in one pass (a projection bottleneck's tail; ``bn`` and ``rbn``
    in the same mode).  ``stats`` / ``rstats``: the producing convs' statistics (training);
    ``btap``: as bn_act."""
    if bn.training != rbn.training:
        raise RuntimeError("bn_res_bn: both BatchNorms must be in the same mode")
    return BNResBNFn.apply(x, bn.weight, bn.bias, r, rbn.weight, rbn.bias, bn, rbn, comm if bn.training else None,
                           stats if bn.training else None, rstats if bn.training else None,
                           btap if bn.training else None)


class MaxPoolFn(torch.autograd.Function):
    """MaxPool2d(kernel 3, stride 2, padding 1) on channels_last."""

    @staticmethod
    def forward(ctx, x):
        x = _cl(x)
        N, C, H, W = x.shape
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = torch.empty((N, C, OH, OW), dtype=x.dtype, device=x.device, memory_format=_CL)
        idx = torch.empty((N, OH, OW, C), dtype=torch.uint8, device=x.device)
        _K().maxpool_fwd(x.permute(0, 2, 3, 1), y.permute(0, 2, 3, 1), idx)
        ctx.save_for_backward(idx)
        ctx.shape = (N, C, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        N, C, H, W = ctx.shape
        dy = _cl(dy)
        dx = torch.empty((N, C, H, W), dtype=dy.dtype, device=dy.device, memory_format=_CL)
        _K().maxpool_bwd(dy.permute(0, 2, 3, 1), idx, dx.permute(0, 2, 3, 1))
        return dx


class GlobalAvgPoolFn(torch.autograd.Function):
    """AdaptiveAvgPool2d(1) + flatten on channels_last: [N, C, H, W] -> [N, C]."""

    @staticmethod
    def forward(ctx, x):
        x = _cl(x)
        N, C, H, W = x.shape
        y = torch.empty((N, C), dtype=x.dtype, device=x.device)
        _K().avgpool_fwd(x.permute(0, 2, 3, 1), y, H * W)
        ctx.shape = (N, C, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, C, H, W = ctx.shape
        dx = torch.empty((N, C, H, W), dtype=dy.dtype, device=dy.device, memory_format=_CL)
        _K().avgpool_bwd(dy.contiguous(), dx.permute(0, 2, 3, 1), H * W)
        return dx


def max_pool_3x3s2(x):
    return MaxPoolFn.apply(x)


def global_avg_pool(x):
    return GlobalAvgPoolFn.apply(x)
