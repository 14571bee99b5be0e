"""Global-norm gradient clipping on two HIP launches (csrc/kernels/clip.hip).

``clip_grad_norm_`` has ``torch.nn.utils.clip_grad_norm_``'s signature and semantics.  On
float32 HIP gradients with ``norm_type == 2`` it is one read-only norm launch, whose result is
two device words (the norm, and the coefficient ``min(1, max_norm / (norm + 1e-6))`` with
torch's roundings), and one in-place scale launch whose workgroups return at once on a step
that does not clip.  There is no host sync, so both replay from a hipGraph.  The norm is summed
in a fixed order that does not depend on the launch's grid: the same gradients give the same
bits, eagerly, replayed, and inside ``optim.AdamW``'s fused step (optim/adamw.py
``set_grad_clip``), which reads the coefficient word in its update instead of scaling the
gradients.

Everything else -- CPU tensors, another norm, other dtypes, more than ``LARGE_MAXT``
gradients -- is torch's own function, unchanged.

The norm launch hands its per-chunk partial sums from workgroup to workgroup through a
workspace and a ticket word kept per device, created on the first eager call (a zero-fill must
not become a node of a step graph).  They serve one stream at a time, as the optimizers do.
"""
from __future__ import annotations

import torch

from .._ext import load as _load_ext

_NEED_EAGER = "{}: its device workspace must exist before graph capture (run one eager step first)"
_MIN_PARTIALS = 1 << 14  # 64 KiB: 67 M gradient elements before the workspace has to grow

_workspaces: dict[int, dict] = {}
_tables: dict = {}
_tables_pinned: list = []


def _capturing() -> bool:
    return torch.cuda.is_current_stream_capturing()


def chunks_of(grads) -> int:
    """The norm launch's chunk count: one float32 partial each (csrc/kernels/clip.hip CHUNK)."""
    C = _load_ext().clip
    return max(1, -(-sum((g.numel() + 3) // 4 for g in grads) // (C.THR * C.U)))


def workspace(dev: torch.device, nchunks: int, who: str = "clip_grad_norm_"):
    """(partials, ticket) of ``dev``, at least ``nchunks`` partials.  A workspace that was too
    small stays alive: a captured graph may still write to it."""
    ws = _workspaces.get(dev.index)
    if ws is None or ws["partials"].numel() < nchunks:
        if _capturing():
            raise RuntimeError(_NEED_EAGER.format(who))
        new = {"partials": torch.empty(max(nchunks, _MIN_PARTIALS), dtype=torch.float32, device=dev),
               "ticket": torch.zeros(1, dtype=torch.int32, device=dev) if ws is None else ws["ticket"],
               "retired": [] if ws is None else ws["retired"] + [ws["partials"]]}
        ws = _workspaces[dev.index] = new
    return ws["partials"], ws["ticket"]


def grad_table(cache: dict, pinned: list, grads):
    """The device table of more than MAXT gradients (``adam.adam_table`` with the gradients in
    every column; the clip kernels read the gradient column), cached per set of pointers and
    sizes and kept for good once a graph capture has looked it up, as optim/adamw.py ``_table``."""
    key = tuple((g.data_ptr(), g.numel()) for g in grads)
    t = cache.get(key)
    if t is None:
        t = _load_ext().adam.adam_table(grads, grads, grads, grads)
        if len(cache) >= 8:
            cache.pop(next(iter(cache)))
        cache[key] = t
    if _capturing() and not any(x is t for x in pinned):
        pinned.append(t)
    return t


def launch_args(grads, cache: dict | None = None, pinned: list | None = None):
    """(gradient list, table keywords) of a clip launch: by value up to MAXT tensors, else the table."""
    if len(grads) <= _load_ext().adam.MAXT:
        return grads, {}
    table = grad_table(_tables if cache is None else cache, _tables_pinned if pinned is None else pinned, grads)
    return [], {"table": table, "total_granules": sum((g.numel() + 3) // 4 for g in grads)}


def native_ok(grads, norm_type=2.0) -> bool:
    """The native route: the 2-norm of 1..LARGE_MAXT dense contiguous float32 HIP gradients on one device."""
    try:
        two = float(norm_type) == 2.0
    except (TypeError, ValueError):
        two = False
    if not two or not grads or not grads[0].is_cuda or len(grads) > _load_ext().adam.LARGE_MAXT:
        return False
    dev = grads[0].device
    return all(g.device == dev and g.dtype == torch.float32 and not g.is_sparse and g.layout == torch.strided
               and g.is_contiguous() for g in grads)


def grad_norm_into(grads, max_norm: float, out: torch.Tensor, grad_scale=None, found_inf=None,
                   cache: dict | None = None, pinned: list | None = None, who: str = "clip_grad_norm_") -> None:
    """The norm launch: ``out[0]`` = the norm of ``grads`` (of ``grads / grad_scale`` with a
    scale word), ``out[1]`` = the clipping coefficient; ``found_inf`` is set, never cleared,
    when a gradient is not finite.  The gradients are only read."""
    partials, ticket = workspace(grads[0].device, chunks_of(grads), who)
    lst, kw = launch_args(grads, cache, pinned)
    _load_ext().clip.grad_norm(lst, float(max_norm), out, partials, ticket, grad_scale, found_inf, **kw)


def clip_grads_(grads, max_norm: float, out: torch.Tensor) -> None:
    """Norm and in-place scale of ``grads`` (``native_ok``) through the two words ``out``,
    which the caller owns: ``out[0]`` is the norm after the call."""
    grad_norm_into(grads, max_norm, out)
    lst, kw = launch_args(grads)
    _load_ext().clip.scale_(lst, out[1:2], **kw)


def _nonfinite_error(norm_type) -> RuntimeError:
    return RuntimeError(f"The total norm of order {norm_type} for gradients from `parameters` is non-finite, so it "
                        "cannot be clipped. To disable this error and scale the gradients by the non-finite norm "
                        "anyway, set `error_if_nonfinite=False`")


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None, *, optimizer=None):
    """``torch.nn.utils.clip_grad_norm_`` (same arguments, same result: the total norm, here a
    0-d float32 tensor on the device, never read on the host unless ``error_if_nonfinite``).

    ``optimizer=``: the optimizer these gradients belong to.  Its ``_flush_deferred()`` runs
    first, so that gradients it was left to complete -- the ConvNet's conv1 slab, a deferring
    DDP's average -- are whole before they are read."""
    if optimizer is not None:
        flush = getattr(optimizer, "_flush_deferred", None)
        if flush is not None:
            flush()
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = list(parameters)
    grads = [p.grad for p in params if p.grad is not None]
    if not native_ok(grads, norm_type):
        return torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type, error_if_nonfinite, foreach)
    if error_if_nonfinite and _capturing():
        raise RuntimeError("clip_grad_norm_(error_if_nonfinite=True) reads the norm on the host, which a graph "
                           "capture cannot do; check optimizer.grad_norm or the returned tensor after the replay")
    partials, _ = workspace(grads[0].device, chunks_of(grads))  # before the allocation below: raises inside a capture
    out = torch.empty(2, dtype=torch.float32, device=grads[0].device)
    if error_if_nonfinite:
        grad_norm_into(grads, max_norm, out)
        if not bool(torch.isfinite(out[0])):
            raise _nonfinite_error(norm_type)
        lst, kw = launch_args(grads)
        _load_ext().clip.scale_(lst, out[1:2], **kw)
    else:
        clip_grads_(grads, max_norm, out)
    return out[0]
