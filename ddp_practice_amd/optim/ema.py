"""Exponential moving average of a model's weights on one HIP launch (csrc/kernels/ema.hip).

``EMA(model, decay)`` is the EMA configuration of ``torch.optim.swa_utils.AveragedModel``
(``AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay), use_buffers=...)``), built so
that ``update()`` replays from a hipGraph (``engine.TrainLoop(ema=)``):

* torch's ``update_parameters`` branches on the host (``copy_param = bool(n_averaged == 0)``,
  also a device sync), so a captured graph repeats whichever branch it was captured with.  Here
  ``n_averaged`` is an int64 word on the device that every workgroup of the launch reads first:
  0 copies, anything else averages, and the launch's last workgroup stores ``n + 1``;
* the whole update -- every parameter and every buffer -- is one launch, not a
  ``_foreach_lerp_`` per dtype plus a ``copy_`` per buffer.  The average is
  ``torch._foreach_lerp_(shadow, source, 1 - decay)`` bit for bit (csrc/common.h ``lerp_rule``);
* ``warmup=True`` (torch has no such mode): update n >= 1 uses ``min(decay, (1 + n) / (10 + n))``,
  computed on the device from the count word (a by-value decay would be frozen into the graph).

The class holds clones of the module's parameters and buffers keyed by ``state_dict`` name
(the *shadows*), not a deep copy of the module: the native models hold workspaces, and captured
graphs reference the live tensors.  ``with ema.applied():`` copies the shadows INTO the model's
own tensors for an evaluation and copies the live values back on exit; no pointer is swapped.

``state_dict()`` / ``load_state_dict()`` use ``AveragedModel``'s layout (``n_averaged``,
``module.<name>``): an ``AveragedModel`` of the torch model loads it, and the reverse.

Deviation from torch: **integer buffers (``num_batches_tracked``) are always copied.**  torch
with ``use_buffers=True`` averages them in floating point and truncates.

More than ``LARGE_MAXT`` tensors, CPU tensors and non-float32 parameters take a fallback that
does what ``update_parameters`` does (``_foreach_lerp_`` / ``copy_``) and syncs with the host,
so it cannot be captured; on CPU it equals torch bit for bit, integer buffers aside.
"""
from __future__ import annotations

import contextlib

import torch

from .._ext import load as _load_ext

_NEED_EAGER = "{}: its device words and row table must exist before graph capture (run one eager update first)"


def _capturing(dev: torch.device) -> bool:
    return dev.type == "cuda" and torch.cuda.is_current_stream_capturing()


def warmup_weight(n: int, decay: float) -> float:
    """The lerp weight of update ``n`` >= 1 with warm-up, rounded as csrc/common.h
    ``ema_warmup_weight`` rounds it (the fallback route; float32 arithmetic through torch)."""
    f = lambda x: torch.tensor(x, dtype=torch.float32)  # noqa: E731
    q = (f(1.0) + f(float(n))) / (f(10.0) + f(float(n)))
    if bool(q < f(decay)):
        return float(f(1.0) - q)
    return float(f(1.0 - decay))


class EMA:
    def __init__(self, model, decay: float = 0.999, use_buffers: bool = False, warmup: bool = False):
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"Invalid decay value {decay} provided. Please provide a value in [0,1] range.")
        if type(model).__name__ == "DistributedDataParallel" and hasattr(model, "module"):
            model = model.module
        self.model = model
        self.decay = float(decay)
        self.use_buffers = bool(use_buffers)
        self.warmup = bool(warmup)
        # the live tensors by state_dict name (keep_vars: the Parameter objects themselves)
        self._sources = dict(model.state_dict(keep_vars=True))
        params = {id(p) for p in model.parameters()}
        if not self._sources:
            raise ValueError("EMA: the model has no parameters or buffers")
        self.shadows: dict[str, torch.Tensor] = {}
        self._copy: dict[str, bool] = {}
        for k, v in self._sources.items():
            self.shadows[k] = v.detach().clone(memory_format=torch.contiguous_format)
            averaged = id(v) in params or (self.use_buffers and v.is_floating_point())
            self._copy[k] = not averaged
        devs = {v.device for v in self._sources.values()}
        self.device = next(iter(devs))
        self._one_device = len(devs) == 1
        self._n = torch.zeros((), dtype=torch.int64, device=self.device)
        self._ticket = None
        self._tables: dict = {}
        self._tables_pinned: list = []

    # ------------------------------------------------------------------ state
    @property
    def n_averaged(self) -> torch.Tensor:
        """The number of updates so far: a 0-d int64 tensor on the device, as torch's."""
        return self._n

    def parameters(self):
        """The shadow tensors, in ``state_dict`` order."""
        return list(self.shadows.values())

    def state_dict(self) -> dict:
        sd = {"n_averaged": self._n.detach().clone()}
        for k, v in self.shadows.items():
            sd["module." + k] = v.detach().clone()
        return sd

    def load_state_dict(self, sd: dict) -> None:
        if _capturing(self.device):
            raise RuntimeError("EMA.load_state_dict copies from the host: not under graph capture")
        want = {"n_averaged"} | {"module." + k for k in self.shadows}
        missing, extra = sorted(want - set(sd)), sorted(set(sd) - want)
        if missing or extra:
            raise KeyError(f"EMA.load_state_dict: missing keys {missing}, unexpected keys {extra}")
        with torch.no_grad():
            for k, v in self.shadows.items():
                v.copy_(sd["module." + k])
            self._n.copy_(torch.as_tensor(sd["n_averaged"]).reshape(()))

    # -- engine._snapshot / _restore (the warm-up steps of a capture are undone)
    def _snapshot(self):
        return self._n.clone(), {k: v.clone() for k, v in self.shadows.items()}

    def _restore(self, snap) -> None:
        with torch.no_grad():
            self._n.copy_(snap[0])
            for k, v in self.shadows.items():
                v.copy_(snap[1][k])

    # ------------------------------------------------------------------ update
    def _rows(self):
        """(shadows, sources, copy flags) of the launch, in ``state_dict`` order; raises on an alias."""
        S, X, C = [], [], []
        for k, s in self.shadows.items():
            x = self._sources[k].detach()
            if x.numel() and s.data_ptr() == x.data_ptr():
                raise RuntimeError(f"EMA: the shadow of {k!r} aliases its source")
            if x.shape != s.shape or x.dtype != s.dtype:
                raise RuntimeError(f"EMA: {k!r} changed its shape or dtype since the EMA was created")
            S.append(s)
            X.append(x)
            C.append(self._copy[k])
        return S, X, C

    def _native_ok(self, S, X, C) -> bool:
        if not self._one_device or self.device.type != "cuda" or len(S) > _load_ext().ema.LARGE_MAXT:
            return False
        for s, x, c in zip(S, X, C):
            if not (x.is_cuda and x.device == self.device and x.is_contiguous() and x.layout == torch.strided):
                return False
            if not c and x.dtype != torch.float32:
                return False
            # copy rows move whole 4-byte words
            if c and ((x.numel() * x.element_size()) % 4 or x.data_ptr() % 4 or s.data_ptr() % 4):
                return False
        return True

    def _table(self, S, X, C):
        """The device row table of more than MAXT rows, cached per set of pointers and sizes and
        kept for good once a graph capture has looked it up (as optim/clip.py ``grad_table``)."""
        key = tuple((s.data_ptr(), x.data_ptr(), x.numel() * x.element_size(), c) for s, x, c in zip(S, X, C))
        t = self._tables.get(key)
        if t is None:
            if _capturing(self.device):
                raise RuntimeError(_NEED_EAGER.format("EMA.update"))
            t = _load_ext().ema.ema_table(S, X, C)
            if len(self._tables) >= 8:
                self._tables.pop(next(iter(self._tables)))
            self._tables[key] = t
        if _capturing(self.device) and not any(x is t for x in self._tables_pinned):
            self._tables_pinned.append(t)
        return t

    @torch.no_grad()
    def update(self) -> None:
        """One update from the model's current weights.  On a GPU: one launch, no host sync."""
        S, X, C = self._rows()
        if not self._native_ok(S, X, C):
            return self._fallback(S, X, C)
        E = _load_ext().ema
        if self._ticket is None:
            if _capturing(self.device):
                raise RuntimeError(_NEED_EAGER.format("EMA.update"))
            self._ticket = torch.zeros(1, dtype=torch.int32, device=self.device)
        kw = {}
        lists = (S, X, C)
        if len(S) > E.MAXT:
            kw = {"table": self._table(S, X, C),
                  "total_granules": sum((x.numel() * x.element_size() // 4 + 3) // 4 for x in X)}
            lists = ([], [], [])
        # the weight: float32 of the Python double, as the scalar torch hands to _foreach_lerp_
        E.ema_update(*lists, self._n, self._ticket, 1.0 - self.decay, self.decay, self.warmup, **kw)

    def _fallback(self, S, X, C) -> None:
        if _capturing(self.device):
            raise RuntimeError("EMA.update: this set of tensors takes the torch fallback, which reads n_averaged "
                               "on the host and cannot be captured")
        n = int(self._n)
        X = [x.to(s.device) for s, x in zip(S, X)]
        avg = [(s, x) for s, x, c in zip(S, X, C) if not c]
        if n == 0:
            for s, x in avg:
                s.copy_(x)
        elif avg:
            w = warmup_weight(n, self.decay) if self.warmup else 1.0 - self.decay
            groups: dict = {}
            for s, x in avg:
                groups.setdefault((s.device, s.dtype), ([], []))
                groups[(s.device, s.dtype)][0].append(s)
                groups[(s.device, s.dtype)][1].append(x)
            for ss, xs in groups.values():
                torch._foreach_lerp_(ss, xs, w)
        for s, x, c in zip(S, X, C):
            if c:
                s.copy_(x)
        self._n += 1

    # ------------------------------------------------------------------ evaluation
    @contextlib.contextmanager
    def applied(self):
        """Run the body with the averaged weights in the model's own tensors; the live values
        are copied back on exit, bit for bit.  Eager only."""
        if _capturing(self.device):
            raise RuntimeError("EMA.applied copies whole models: not under graph capture")
        with torch.no_grad():
            live = {k: v.detach().clone() for k, v in self._sources.items()}
            for k, v in self._sources.items():
                v.detach().copy_(self.shadows[k])
        try:
            yield self.model
        finally:
            with torch.no_grad():
                for k, v in self._sources.items():
                    v.detach().copy_(live[k])
