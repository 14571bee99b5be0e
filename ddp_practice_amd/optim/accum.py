"""Gradient accumulation on one HIP launch per micro-step (csrc/kernels/accum.hip).

``GradAccumulator(optimizer, steps=K, model=None)`` trains on an effective batch of K
micro-batches per rank.  ``accumulate()`` is called after every ``backward()``:

    for i, (x, y) in enumerate(batches):
        optimizer.zero_grad(set_to_none=True)
        scaler.scale(criterion(model(x), y)).backward()
        if accum.accumulate(last=(i == len(batches) - 1)):
            scaler.step(optimizer); scaler.update()

Every backward writes FRESH gradients (``.grad`` is None when it starts), so the fused producers
of ops/convnet_fused.py stay on and autograd adds nothing.  One launch per micro-step folds
the fresh gradients into float32 accumulators:

    micro-step 0        acc = g                      (no zero-fill anywhere)
    micro-steps 1..K-2  acc = acc + g
    the window's last   g   = (acc + g) * c,  c = float32(1 / K); acc is not written

After a non-final micro-step ``.grad`` is set to None; after the last one ``.grad`` holds the
window's mean and ``accumulate`` returns True: the unchanged optimizer, clip, EMA, schedule and
GradScaler step then run once per window.  The position within a window is a host integer; a
captured window has one node per micro-step with its mode baked in.  ``last=True`` closes a
short window early (an epoch's end); the factor stays ``1 / K`` (a window of a single
micro-step stores ``g * c``).  The scaled gradients of a GradScaler are accumulated as they
are: call ``scaler.update()`` once per window so that a window shares one loss scale.

The accumulator is a gradient reader and writer: before its launch it calls the optimizer's
``flush_slab()`` (a deferred conv1 slab is summed, a producer-side pre-check dropped), but on a
non-final micro-step never ``_flush_deferred()``, which would all-reduce.

DDP (pass the wrapped model as ``model``): ONE gradient average per window.  The order is:
each rank sums its micro-batches in order and scales the sum by ``c`` (the LAST launch), then
the ranks average once.  For power-of-two K and world sizes the order of the two scalings
does not matter bitwise.  The reducer is put in defer mode
(``DistributedDataParallel.defer_grad_sync_for``): a backward leaves the buckets rank-local; a
non-final micro-step accumulates from the bucket views and drops the pending average, the
final one writes the mean into the bucket views and leaves the average to its consumer -- the
fused AMP-SGD exchange when the optimizer owns the deferral, else the reducer's bucket
all-reduces, run here.  A DDP without bucket views or with ``find_unused_parameters`` runs every
micro-step under ``no_sync()`` (``micro_step()`` is that context) and the accumulator
all-reduces the window's mean itself, flat, once.

Fallback: CPU tensors, non-float32 gradients, more than ``LARGE_MAXT`` gradients do the same
arithmetic with torch ops (``acc.copy_(g)``, ``acc.add_(g)``, ``g.copy_((acc + g) * c)``).
"""
from __future__ import annotations

import contextlib

import torch

from .._ext import load as _load_ext


def _capturing(dev: torch.device) -> bool:
    return dev.type == "cuda" and torch.cuda.is_current_stream_capturing()


class GradAccumulator:
    def __init__(self, optimizer, steps: int = 1, model=None):
        if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
            raise ValueError(f"GradAccumulator: steps must be an int >= 1, not {steps!r}")
        if not hasattr(optimizer, "param_groups"):
            raise ValueError("GradAccumulator: optimizer has no param_groups")
        self.optimizer = optimizer
        self.steps = steps
        self.c = 1.0 / steps  # the kernel and the fallback round it to float32
        self.model = model
        self._pos = 0
        self.launches = 0  # accumulate launches issued (native or fallback), for tests
        self._params = [p for g in optimizer.param_groups for p in g["params"] if p.requires_grad]
        if len({id(p) for p in self._params}) != len(self._params):
            raise ValueError("GradAccumulator: a parameter is listed twice")
        self._acc: dict[int, torch.Tensor] = {}
        self._flat: dict[torch.device, torch.Tensor] = {}
        self._rows = None  # the parameters of the open window
        self._tables: dict = {}
        self._tables_pinned: list = []
        # how a DDP model's average is taken: None (no DDP / one rank), "defer" or "no_sync"
        self._ddp = None
        if steps > 1:
            # float32 views, each 16-byte aligned, into one flat buffer per device; allocated
            # here, outside any capture, and never filled
            sizes: dict[torch.device, int] = {}
            for p in self._params:
                sizes[p.device] = sizes.get(p.device, 0) + (p.numel() + 3) // 4 * 4
            for dev, n in sizes.items():
                self._flat[dev] = torch.empty(max(n, 4), dtype=torch.float32, device=dev)
            offs = {dev: 0 for dev in sizes}
            for p in self._params:
                o = offs[p.device]
                self._acc[id(p)] = self._flat[p.device][o:o + p.numel()].view(p.shape)
                offs[p.device] = o + (p.numel() + 3) // 4 * 4
            if model is not None and hasattr(model, "no_sync") and not hasattr(model, "averages_gradients"):
                raise ValueError("GradAccumulator: model= takes this package's DistributedDataParallel (another "
                                 "wrapper would average every micro-step's gradients behind its back)")
            if model is not None and getattr(model, "averages_gradients", False):
                self._ddp = "defer" if model.defer_grad_sync_for(optimizer) else "no_sync"

    # ------------------------------------------------------------------ window
    @property
    def position(self) -> int:
        """Micro-steps accumulated in the open window (a host integer)."""
        return self._pos

    def reset(self) -> None:
        """Drop a half-finished window: the next ``accumulate()`` starts a new one."""
        self._pos = 0
        self._rows = None
        if self._ddp == "defer":
            self.model.drop_deferred_grad_sync()

    def micro_step(self):
        """The context of a micro-step's forward and backward: ``model.no_sync()`` for a DDP
        the reducer's deferral cannot serve (the accumulator averages once itself), else
        nothing."""
        if self._ddp == "no_sync":
            return self.model.no_sync()
        return contextlib.nullcontext()

    def _native_ok(self, accs, grads) -> bool:
        if not grads or len(grads) > _load_ext().accum.LARGE_MAXT:
            return False
        dev = grads[0].device
        return dev.type == "cuda" and all(
            g.device == dev and g.dtype == torch.float32 and g.is_contiguous() and g.layout == torch.strided
            and g.data_ptr() % 4 == 0 for g in grads)

    def _table(self, accs, grads):
        """The device row table of more than MAXT rows, cached per set of gradient pointers and
        sizes (DDP bucket views keep them fixed; freshly allocated gradients may not).  It is
        written by launches on the stream (``accum_table``), never from the host, so one built
        during a graph capture is captured with it; any table a capture looked up stays
        referenced for the life of the accumulator (as optim/adamw.py ``_table``)."""
        key = tuple((g.data_ptr(), g.numel()) for g in grads)
        t = self._tables.get(key)
        if t is None:
            t = _load_ext().accum.accum_table(accs, grads)
            if len(self._tables) >= 8:
                self._tables.pop(next(iter(self._tables)))
            self._tables[key] = t
        if _capturing(grads[0].device) and not any(x is t for x in self._tables_pinned):
            self._tables_pinned.append(t)
        return t

    @torch.no_grad()
    def accumulate(self, last: bool | None = None) -> bool:
        """Fold this micro-step's gradients into the window.  True: the window is complete,
        ``.grad`` holds its mean, run the update.  False: ``.grad`` is None again."""
        if self.steps == 1:
            return True
        final = bool(last) or self._pos == self.steps - 1
        flush = getattr(self.optimizer, "flush_slab", None)
        if flush is not None:
            flush()
        rows = [p for p in self._params if p.grad is not None]
        if self._rows is None:
            self._rows = rows
        elif len(rows) != len(self._rows) or any(a is not b for a, b in zip(rows, self._rows)):
            raise RuntimeError("GradAccumulator: the set of parameters with a gradient changed within a window")
        grads = [p.grad for p in rows]
        accs = [self._acc[id(p)] for p in rows]
        if rows:
            if any(g.is_sparse for g in grads):
                raise RuntimeError("GradAccumulator does not support sparse gradients")
            mode = (3 if final else 0) if self._pos == 0 else (2 if final else 1)
            if self._native_ok(accs, grads):
                A = _load_ext().accum
                kw, lists = {}, (accs, grads)
                if len(grads) > A.MAXT:
                    kw = {"table": self._table(accs, grads),
                          "total_granules": sum((g.numel() + 3) // 4 for g in grads)}
                    lists = ([], [])
                A.accumulate(*lists, mode, self.c, **kw)
            else:
                self._fallback(accs, grads, mode)
            self.launches += 1
        if not final:
            self._pos += 1
            if self._ddp == "defer":
                self.model.drop_deferred_grad_sync()  # this micro-step is not averaged
            for p in self._params:
                p.grad = None
            return False
        self._pos = 0
        self._rows = None
        if self._ddp == "defer":
            # the fused step of an optimizer that owns the deferral averages inside its own
            # launch, and its other gradient readers flush first; nobody else would
            if not self.model.grad_sync_deferred_to(self.optimizer):
                self.model.run_deferred_grad_sync()
        elif self._ddp == "no_sync":
            self._average(grads)
        return True

    def _fallback(self, accs, grads, mode: int) -> None:
        c = torch.tensor(self.c, dtype=torch.float32).item()  # float32(1 / K), as the kernel's
        for a, g in zip(accs, grads):
            if mode == 0:
                a.copy_(g)
            elif mode == 1:
                a.add_(g)
            elif mode == 2:
                g.copy_((a + g) * c)
            else:
                g.copy_(g.to(torch.float32) * c)

    def _average(self, grads) -> None:
        """One flat all-reduce of the window's mean (a DDP whose micro-steps ran under no_sync)."""
        comm = self.model.comm
        by: dict = {}
        for g in grads:
            by.setdefault((g.device, g.dtype), []).append(g)
        for gs in by.values():
            flat = torch.cat([g.reshape(-1) for g in gs])
            comm.all_reduce_(flat, "avg")
            o = 0
            for g in gs:
                g.copy_(flat[o:o + g.numel()].view_as(g))
                o += g.numel()
