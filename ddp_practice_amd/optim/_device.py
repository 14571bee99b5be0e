"""What the modules of ``optim/`` share about device-resident state: the graph-capture guard,
the refusal to create such state lazily inside a capture, the lifetime policy of the device
tensor tables (``TableCache``) and the common base of the native optimizers."""
from __future__ import annotations

import torch
from torch.optim import Optimizer


def capturing(dev: torch.device) -> bool:
    """The current stream of a ``cuda`` device is capturing a graph (``torch.cuda`` is not
    touched for any other device)."""
    return dev.type == "cuda" and torch.cuda.is_current_stream_capturing()


_NEED_EAGER = "{}: {} must exist before graph capture (run one eager {} first)"


def need_eager(dev: torch.device, who: str, what: str, verb: str = "step") -> None:
    """Called where device state is about to be created lazily: inside a capture its
    allocation and zero-fill would become graph nodes that run again on every replay."""
    if capturing(dev):
        raise RuntimeError(_NEED_EAGER.format(who, what, verb))


class TableCache:
    """The device tensor tables that launches over more than ``MAXT`` tensors read, and how
    long each one lives.

    * ``build()`` writes a table by launches on the stream (``adam_table``, ``amp_sgd_table``,
      ``ema_table``, ``accum_table``), never from the host, so one built during a graph
      capture is captured with it.  Filling the SGD step's table from the host after capture
      was tried and reverted after a fault in the ResNet bench (README, r5aa).
    * A table is cached per key.  The caller's key carries every tensor's pointer (DDP
      bucket-view gradients and optimizer state keep them fixed; freshly allocated gradients
      may not) and its size too: memory reused at the same address for a different size must
      not hit a stale table.
    * At most 8 tables are kept and the oldest is dropped first.  Dropping one that only eager
      launches read is safe: the allocator's stream order keeps its memory from reuse until
      they have run.
    * Any table looked up during graph capture -- built then, or an eager warm-up's table
      reused from the cache -- is appended once to ``pinned``, which is never shrunk: the
      graph reads the table on every replay, long after eviction may have dropped it from
      ``tables``, so it stays referenced for the life of the cache's owner.
    """

    def __init__(self, pinned: list | None = None):
        self.tables: dict = {}
        self.pinned: list = [] if pinned is None else pinned  # two caches of one owner may share it

    def get(self, key, build, dev: torch.device):
        t = self.tables.get(key)
        if t is None:
            t = build()
            if len(self.tables) >= 8:
                self.tables.pop(next(iter(self.tables)))
            self.tables[key] = t
        if capturing(dev) and not any(x is t for x in self.pinned):
            self.pinned.append(t)
        return t


def _undecorated(name):
    """``torch.optim.Optimizer.<name>`` without its ``torch._disable_dynamo`` wrapper.

    The wrapper imports ``torch._dynamo`` on first use (~1.2 s, measured: the largest
    single cost of a 3-epoch CLI run); this framework never traces an optimizer, so the
    plain function is called.
    """
    fn = getattr(Optimizer, name)
    return getattr(fn, "__wrapped__", fn)


class DeviceOptimizer(Optimizer):
    """What ``SGD`` and ``Adam`` share: ``found_inf`` read on the device, the group's rate from
    an attached ``optim.DeviceLR`` and the gradient average a DDP reducer deferred to them."""
    supports_device_found_inf = True

    add_param_group = _undecorated("add_param_group")
    zero_grad = _undecorated("zero_grad")

    def _lr_kw(self, gi: int = 0) -> dict:
        """``lr_dev=`` of group ``gi``'s update launch: its device-resident rate when an
        ``optim.DeviceLR`` is attached (optim/lr.py), else nothing -- the rate goes by value."""
        w = self.__dict__.get("_lr_words")
        return {} if w is None else {"lr_dev": w[gi]}

    def _host_lr(self, gi: int) -> float | None:
        """Group ``gi``'s ``DeviceLR`` word read on the host, for the torch fallback (None: no
        ``DeviceLR`` attached, the group's own ``lr`` holds)."""
        w = self.__dict__.get("_lr_words")
        return None if w is None else float(w[gi])

    def _flush_deferred(self):
        """Average gradients a DDP reducer left to this optimizer (DDP.defer_grad_sync_to hands
        them to any optimizer with ``fused_amp_step``): every gradient reader calls this first."""
        d = getattr(self, "_deferred_ddp", None)
        if d is not None:
            d[0].flush_deferred()
