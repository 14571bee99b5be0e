"""Learning-rate schedules that survive hipGraph replay: the rate lives on the device.

Every update kernel takes the learning rate as a by-value kernel argument, so a captured
step (``runtime.CapturedStep``) replays the rate it was captured with: a
``torch.optim.lr_scheduler`` or a hand edit of ``param_groups[0]["lr"]`` is ignored by
every replayed step.  ``DeviceLR`` keeps one float32 word per param group in device memory
-- the update kernels read it in place of the argument (``lr_dev=``, csrc/kernels/optim.hip)
-- and a table of per-step rates next to it.  ``step()`` is one 64-lane launch
(``lr_advance``): position += 1, words = table row.  No host sync, legal under capture, so
it sits inside the captured step like the loss scale, ``found_inf`` and the data position.

The table is computed on the host, once (``from_torch`` runs any torch scheduler on a
throw-away optimizer), so each rate is float32 of the Python double torch would have passed
to its own foreach SGD -- bit-identical training, and no device ``cos``/``pow`` whose last
bit differs from libm.
"""
from __future__ import annotations

from typing import Callable, Sequence

import torch

from .._ext import load as _load_ext


def _capturing(dev: torch.device) -> bool:
    return dev.type == "cuda" and torch.cuda.is_current_stream_capturing()


class DeviceLR:
    """``lrs[k]`` is the rate used by the update after ``k`` calls of ``step()``: a sequence
    of floats (every group the same) or of per-group rows.  Past the end the last row holds.

    The words are attached to the optimizer as ``optimizer._lr_words`` (one per group), not
    put into ``param_groups``: ``optimizer.state_dict()`` is unchanged.  ``param_groups[i]["lr"]``
    is left alone too and is not what the update uses while a ``DeviceLR`` is attached.
    """

    def __init__(self, optimizer, lrs: Sequence):
        groups = optimizer.param_groups
        G = len(groups)
        rows = []
        for r in lrs:
            row = [float(x) for x in r] if isinstance(r, (list, tuple)) else [float(r)] * G
            if len(row) != G:
                raise ValueError(f"DeviceLR: a row of {len(row)} rates for {G} param groups")
            rows.append(row)
        if not rows:
            raise ValueError("DeviceLR: an empty schedule")
        ps = [p for g in groups for p in g["params"]]
        devs = {p.device for p in ps}
        if len(devs) != 1:
            raise ValueError("DeviceLR: the optimizer's parameters must be on one device")
        self.device = devs.pop()
        if _capturing(self.device):
            raise RuntimeError("DeviceLR: create the schedule outside graph capture")
        self.optimizer = optimizer
        # float32 of the Python double: what torch's foreach SGD rounds its lr to
        self.table = torch.tensor(rows, dtype=torch.float64).to(torch.float32).to(self.device).contiguous()
        self.pos = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.words = self.table[0].clone()
        optimizer._lr_words = tuple(self.words[g:g + 1] for g in range(G))

    @classmethod
    def from_torch(cls, optimizer, make_scheduler: Callable, steps: int) -> "DeviceLR":
        """Compile a torch scheduler into a table of ``steps`` rows: ``make_scheduler(opt)`` is
        run on a throw-away ``torch.optim.SGD`` with the same groups and base rates, on the
        host, recording ``get_last_lr()`` before each of its ``steps`` steps."""
        groups = [{"params": [torch.nn.Parameter(torch.zeros(1))], "lr": float(g.get("initial_lr", g["lr"]))}
                  for g in optimizer.param_groups]
        shadow = torch.optim.SGD(groups, lr=groups[0]["lr"])
        sched = make_scheduler(shadow)
        rows = []
        for k in range(max(1, int(steps))):
            rows.append([float(x) for x in sched.get_last_lr()])
            if k + 1 < steps:
                shadow.step()
                sched.step()
        return cls(optimizer, rows)

    def __len__(self) -> int:
        return self.table.shape[0]

    def step(self) -> None:
        """Advance by one: a single launch on a GPU (no host sync, capturable)."""
        if self.device.type == "cuda":
            _load_ext().optim.lr_advance(self.table, self.pos, self.words)
        else:
            pos = min(int(self.pos) + 1, torch.iinfo(torch.int32).max)  # saturating, as the kernel
            self.pos.fill_(pos)
            self.words.copy_(self.table[min(pos, len(self) - 1)])

    # -- host-syncing methods: each reads from or writes to the device, none under capture
    def _no_capture(self, what: str) -> None:
        if _capturing(self.device):
            raise RuntimeError(f"DeviceLR.{what} synchronises with the host: not under graph capture")

    def get_last_lr(self) -> list[float]:
        """The rates the next update uses (host sync)."""
        self._no_capture("get_last_lr()")
        return [float(x) for x in self.words.tolist()]

    def state_dict(self) -> dict:
        """``{"pos": int}`` (host sync)."""
        self._no_capture("state_dict()")
        return {"pos": int(self.pos.item())}

    def load_state_dict(self, sd: dict) -> None:
        """Set the position and rewrite the words (host-ordered copies)."""
        self._no_capture("load_state_dict()")
        pos = int(sd["pos"])
        if pos < 0:
            raise ValueError("DeviceLR: negative position")
        self.pos.fill_(pos)
        self.words.copy_(self.table[min(pos, len(self) - 1)])

    # -- engine._snapshot / _restore (the warm-up steps of a capture are undone)
    def _snapshot(self):
        return self.pos.clone(), self.words.clone()

    def _restore(self, snap) -> None:
        self.pos.copy_(snap[0])
        self.words.copy_(snap[1])
