"""Adam / AdamW on one multi-tensor HIP launch per param group (csrc/kernels/adam.hip).

Same hyper-parameters, state keys and update rule as ``torch.optim.AdamW`` / ``torch.optim.Adam``
(torch/optim/adam.py, the capturable foreach path ``_multi_tensor_adam``: csrc/common.h
``adam_rule`` follows its op order and rounding), built so that the whole step replays from a
hipGraph (``engine.TrainLoop``):

* the step count of the bias corrections is a float32 word in device memory.  torch's default
  path computes ``1 - beta ** step`` on the host, so a captured graph would replay the
  corrections it was captured with (the by-value trap ``optim.DeviceLR`` removed for the
  learning rate); its capturable path is about twenty foreach launches per step.  Here every
  launch reads the word and the launch's last workgroup advances it;
* ``found_inf`` is read on the device (``supports_device_found_inf``): a skipped step leaves
  the parameters, both moments and the step word untouched, bit for bit;
* the learning rate is read from the ``optim.DeviceLR`` word when one is attached;
* ``set_grad_clip(max_norm)`` clips the global gradient norm inside the step: one read-only
  norm launch over the gradients of every param group (optim/clip.py; under ``GradScaler`` it
  takes the place of the non-finite check, whose pass over the gradients it shares), and the
  update multiplies each gradient by the coefficient word that launch left on the device.
  The gradients are not written, and the result is bitwise what ``unscale_()`` ->
  ``optim.clip_grad_norm_`` -> ``step()`` gives.  The fused route covers at most
  ``LARGE_MAXT`` gradients in total; beyond that ``GradScaler`` takes its explicit route and
  the clip is torch's function.

The one deviation from torch: **the parameters of a group share one step count.**
``state[p]["step"]`` is the same 0-d float32 tensor for every parameter of a group (so
``state_dict()`` and ``engine._snapshot`` cover it), and a step in which some parameters of a
group have a gradient and others have none raises instead of advancing only some counts.
``state_dict()`` writes one copy of the count per parameter, as torch does, and loads into
``torch.optim.AdamW``; ``load_state_dict`` takes torch's and refuses a group whose parameters
disagree on ``step``.

``amsgrad``, complex and sparse parameters are not implemented (the constructor raises).
"""
from __future__ import annotations

import torch
from torch.optim import Optimizer

from .._ext import load as _load_ext
from .sgd import _undecorated


def _capturing(dev: torch.device) -> bool:
    return dev.type == "cuda" and torch.cuda.is_current_stream_capturing()


_NEED_EAGER = "{}: the optimizer state must exist before graph capture (run one eager step first)"


class Adam(Optimizer):
    supports_device_found_inf = True
    _decoupled = False  # torch.optim.Adam: weight decay added to the gradient

    add_param_group = _undecorated("add_param_group")
    zero_grad = _undecorated("zero_grad")
    _base_state_dict = _undecorated("state_dict")
    _base_load_state_dict = _undecorated("load_state_dict")

    def __init__(self, params, lr: float = 1e-3, betas: tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, amsgrad: bool = False, *, maximize: bool = False):
        if isinstance(lr, torch.Tensor):
            raise ValueError("a Tensor lr is not supported: attach an optim.DeviceLR for a device-resident rate")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if amsgrad:
            raise ValueError(f"{type(self).__name__}: amsgrad is not implemented")
        # every key of torch.optim.Adam's groups, so a state_dict loads there and back
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=maximize,
                        foreach=None, capturable=False, differentiable=False, fused=None,
                        decoupled_weight_decay=self._decoupled)
        super().__init__(params, defaults)
        for group in self.param_groups:
            for p in group["params"]:
                if p.is_complex() or p.is_sparse:
                    raise ValueError(f"{type(self).__name__}: complex and sparse parameters are not implemented")
        # the ticket words of the step-count advance (csrc/kernels/adam.hip), zeroed here, outside
        # any graph capture, as SGD's barrier state is (optim/sgd.py)
        self._tickets: dict[int, torch.Tensor] = {}
        for gi, group in enumerate(self.param_groups):
            if group["params"] and group["params"][0].is_cuda and not _capturing(group["params"][0].device):
                self._ticket(gi, group["params"][0].device)
        self._clip: float | None = None

    # ------------------------------------------------------------------ clipping
    def set_grad_clip(self, max_norm: float | None) -> None:
        """Clip the global 2-norm of the gradients of all param groups to ``max_norm`` inside
        every step (None: off).  An attribute, not a param-group key: ``state_dict()`` keeps
        loading into ``torch.optim.AdamW``."""
        if max_norm is not None:
            max_norm = float(max_norm)
            if not max_norm > 0.0:
                raise ValueError(f"Invalid max_norm: {max_norm}")
        self._clip = max_norm

    @property
    def grad_norm(self) -> torch.Tensor | None:
        """The last clipped step's total gradient norm: a 0-d float32 tensor on the device (no
        host sync; a step that found_inf skipped leaves the non-finite norm it saw)."""
        w = self.__dict__.get("_clip_out")
        return None if w is None else w[0]

    def _clip_words(self, dev: torch.device) -> torch.Tensor:
        w = self.__dict__.get("_clip_out")
        if w is None or w.device != dev or w.numel() != 2:
            if _capturing(dev):
                raise RuntimeError(_NEED_EAGER.format(type(self).__name__))
            w = self._clip_out = torch.tensor([0.0, 1.0], dtype=torch.float32, device=dev)
        return w

    def _clip_native(self, groups) -> bool:
        n = sum(len(g[1]) for g in groups)
        devs = {p.device for g in groups for p in g[1]}
        return (0 < n <= _load_ext().adam.LARGE_MAXT and len(devs) == 1
                and all(self._native(*g[1:5]) for g in groups if g[1]))

    def _norm_launch(self, groups, grad_scale=None, found_inf=None) -> torch.Tensor:
        """One norm launch over the gradients of every group, in group order; returns the
        coefficient word the updates read."""
        from . import clip as K

        grads = [g for grp in groups for g in grp[2]]
        out = self._clip_words(grads[0].device)
        K.grad_norm_into(grads, self._clip, out, grad_scale, found_inf,
                         self.__dict__.setdefault("_clip_tables", {}), self.__dict__.setdefault("_tables_pinned", []),
                         type(self).__name__)
        return out[1:2]

    # ------------------------------------------------------------------ state
    def _ticket(self, gi: int, dev: torch.device) -> torch.Tensor:
        t = self._tickets.get(gi)
        if t is None or t.device != dev:
            if _capturing(dev):
                raise RuntimeError(_NEED_EAGER.format(type(self).__name__))
            t = self._tickets[gi] = torch.zeros(1, dtype=torch.int32, device=dev)
        return t

    def _group_word(self, group) -> torch.Tensor | None:
        for p in group["params"]:
            st = self.state.get(p)
            if st:
                return st["step"]
        return None

    def _collect(self):
        """Per group: (group, params, grads, exp_avgs, exp_avg_sqs, step word); state is created
        here, lazily, but never inside a graph capture."""
        out = []
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                out.append((group, [], [], [], [], None))
                continue
            if len(ps) != len(group["params"]):
                raise RuntimeError(f"{type(self).__name__}: {len(group['params']) - len(ps)} of a group's "
                                   f"{len(group['params'])} parameters have no gradient; the group shares one "
                                   "step count, so all of its parameters step together (put parameters that "
                                   "may be unused into a group of their own)")
            word = self._group_word(group)
            ms, vs = [], []
            for p in ps:
                if p.grad.is_sparse:
                    raise RuntimeError(f"{type(self).__name__} does not support sparse gradients")
                st = self.state[p]
                if not st:
                    if _capturing(p.device):
                        raise RuntimeError(_NEED_EAGER.format(type(self).__name__))
                    if word is None:
                        word = torch.zeros((), dtype=torch.float32, device=p.device)
                    st["step"] = word
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                ms.append(st["exp_avg"])
                vs.append(st["exp_avg_sq"])
            out.append((group, ps, [p.grad for p in ps], ms, vs, word))
        return out

    def state_dict(self):
        """torch's layout, with one copy of the group's step count per parameter (a file that
        kept the sharing would make ``torch.optim.AdamW`` advance one tensor once per parameter)."""
        sd = self._base_state_dict()
        sd["state"] = {k: {n: (v.clone() if n == "step" and torch.is_tensor(v) else v) for n, v in st.items()}
                       for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict) -> None:
        kinds = {k for st in state_dict["state"].values() for k in st}
        if kinds and not {"exp_avg", "exp_avg_sq", "step"} <= kinds:
            raise ValueError(f"{type(self).__name__}.load_state_dict: not an Adam state (its per-parameter keys "
                             f"are {sorted(map(str, kinds))}, expected exp_avg, exp_avg_sq, step)")
        if any("betas" not in g for g in state_dict["param_groups"]):
            raise ValueError(f"{type(self).__name__}.load_state_dict: the param groups are not Adam's (no 'betas')")
        if "max_exp_avg_sq" in kinds:
            raise ValueError(f"{type(self).__name__}.load_state_dict: an amsgrad state is not supported")
        self._base_load_state_dict(state_dict)
        # one word per group again: on the parameters' device, float32, shared
        for group in self.param_groups:
            group["amsgrad"] = False
            have = [p for p in group["params"] if self.state.get(p)]
            if not have:
                continue
            if len(have) != len(group["params"]):
                raise ValueError(f"{type(self).__name__}.load_state_dict: a group with state for only some of "
                                 "its parameters (the group shares one step count)")
            steps = [float(self.state[p]["step"]) for p in have]
            if any(s != steps[0] for s in steps):
                raise ValueError(f"{type(self).__name__}.load_state_dict: the parameters of a group disagree on "
                                 f"'step' ({sorted(set(steps))}); the group shares one step count")
            word = torch.full((), steps[0], dtype=torch.float32, device=have[0].device)
            for p in have:
                self.state[p]["step"] = word

    # ------------------------------------------------------------------ step
    def _lr_kw(self, gi: int = 0) -> dict:
        """``lr_dev=`` of group ``gi``'s launch when an ``optim.DeviceLR`` is attached (optim/lr.py)."""
        w = self.__dict__.get("_lr_words")
        return {} if w is None else {"lr_dev": w[gi]}

    def _flush_deferred(self):
        """Average gradients a DDP reducer left to this optimizer (DDP.defer_grad_sync_to hands
        them to any optimizer with ``fused_amp_step``): every gradient reader calls this first."""
        d = getattr(self, "_deferred_ddp", None)
        if d is not None:
            d[0].flush_deferred()

    @staticmethod
    def _native(params, grads, ms, vs) -> bool:
        return params[0].is_cuda and len(params) <= _load_ext().adam.LARGE_MAXT and all(
            t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
            for ts in (params, grads, ms, vs) for t in ts)

    def _table(self, gi, params, grads, ms, vs):
        """Device tensor table of a group of more than MAXT tensors, cached per set of pointers
        (DDP bucket-view grads and the optimizer state keep them fixed; freshly allocated
        grads may not).  Any table looked up during graph capture -- built then, or an
        eager warm-up's table reused from the cache -- stays referenced for the life of
        the optimizer (the graph reads it on every replay).  The key carries every
        tensor's size too: memory reused at the same address for a different size must
        not hit a stale table.  The table is written by launches on the stream
        (``adam_table``), never from the host: filling the SGD step's table from the host
        after capture was tried and reverted after a fault in the ResNet bench (README, r5aa)."""
        key = (gi,) + tuple(tuple((t.data_ptr(), t.numel()) for t in ts) for ts in (params, grads, ms, vs))
        cache = self.__dict__.setdefault("_tables", {})
        t = cache.get(key)
        if t is None:
            t = _load_ext().adam.adam_table(params, grads, ms, vs)
            if len(cache) >= 8:  # eager tables: the allocator's stream order makes freeing safe
                cache.pop(next(iter(cache)))
            cache[key] = t
        if torch.cuda.is_current_stream_capturing():
            pinned = self.__dict__.setdefault("_tables_pinned", [])
            if not any(x is t for x in pinned):
                pinned.append(t)
        return t

    def _launch_args(self, gi, params, grads, ms, vs):
        """(lists or table) of one group's launches: by value up to MAXT tensors, else the table."""
        A = _load_ext().adam
        if len(params) <= A.MAXT:
            return (params, grads, ms, vs), {}
        total = sum((p.numel() + 3) // 4 for p in params)
        return ([], [], [], []), {"table": self._table(gi, params, grads, ms, vs), "total_granules": total}

    def _native_step(self, gi, group, params, grads, ms, vs, word, found_inf, grad_scale, clip_coef=None):
        lists, kw = self._launch_args(gi, params, grads, ms, vs)
        if clip_coef is not None:
            kw["clip_coef"] = clip_coef
        b1, b2 = group["betas"]
        _load_ext().adam.adam_step(*lists, word, group["lr"], b1, b2, group["eps"], group["weight_decay"],
                                   group["decoupled_weight_decay"], group["maximize"], found_inf, grad_scale,
                                   ticket=self._ticket(gi, params[0].device), **self._lr_kw(gi), **kw)

    @torch.no_grad()
    def step(self, closure=None, found_inf: torch.Tensor | None = None):
        self._flush_deferred()
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        groups = self._collect()
        coef = None
        if self.__dict__.get("_clip") is not None and any(g[1] for g in groups):
            if self._clip_native(groups):
                coef = self._norm_launch(groups)
            else:  # torch's clip, in place, as the update below is torch's
                self._clip_out = torch.nn.utils.clip_grad_norm_(
                    [p for g in groups for p in g[1]], self._clip).detach().reshape(1)
        for gi, (group, params, grads, ms, vs, word) in enumerate(groups):
            if not params:
                continue
            if self._native(params, grads, ms, vs):
                self._native_step(gi, group, params, grads, ms, vs, word, found_inf, None, coef)
            else:
                if found_inf is not None and bool(found_inf.item()):
                    continue
                w = self.__dict__.get("_lr_words")
                self._torch_step(group, params, grads, ms, vs, word, None if w is None else float(w[gi]))
        return loss

    @staticmethod
    def _torch_step(group, params, grads, ms, vs, word, lr=None):
        """CPU, non-float32 or non-contiguous tensors: torch's functional Adam on the same state.
        It advances one count per parameter, so each gets a copy and the word takes the result."""
        from torch.optim import adam as _A

        fn = getattr(_A.adam, "__wrapped__", _A.adam)  # no torch._dynamo import (optim/sgd.py _undecorated)
        steps = [word.clone() for _ in params]
        b1, b2 = group["betas"]
        fn(params, grads, ms, vs, [], steps, foreach=None, capturable=False, differentiable=False, fused=None,
           grad_scale=None, found_inf=None, has_complex=False,
           decoupled_weight_decay=group["decoupled_weight_decay"], amsgrad=False, beta1=b1, beta2=b2,
           lr=group["lr"] if lr is None else lr, weight_decay=group["weight_decay"], eps=group["eps"],
           maximize=group["maximize"])
        word.copy_(steps[0])

    # ------------------------------------------------------------------ AMP
    def can_fuse_amp(self) -> bool:
        """GradScaler.step as three barrier-free launches (``fused_amp_step``): every group on
        the native kernel, and its state in place if a capture is under way."""
        seen = False
        total = 0
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            total += len(ps)
            if self.__dict__.get("_clip") is not None and total > _load_ext().adam.LARGE_MAXT:
                return False  # one norm launch covers LARGE_MAXT gradients: the explicit route
            if len(ps) != len(group["params"]) or len(ps) > _load_ext().adam.LARGE_MAXT:
                return False
            if not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and not p.grad.is_sparse
                       and p.grad.dtype == torch.float32 and p.grad.is_contiguous() for p in ps):
                return False
            seen = True
        return seen

    @torch.no_grad()
    def fused_amp_step(self, scale, tracker, found_inf, growth, backoff, interval):
        """unscale + inf check + update + scale update without a host sync or a grid barrier:
        a read-only non-finite check of the (still scaled) gradients into ``found_inf``, the
        update with the unscale folded in (``grad_scale``; the gradients are left as they are),
        and GradScaler's own ``update_scale``, which also re-arms ``found_inf``.  The check only
        ever sets ``found_inf``: it must be zero on entry, as GradScaler keeps it.  With a clip
        set the check is the norm launch's (same pass, same word) and the update also reads
        the coefficient; a skipped step ignores whatever that word holds."""
        self._flush_deferred()
        C = _load_ext()
        groups = [(gi, g) for gi, g in enumerate(self._collect()) if g[1]]
        coef = None
        if self.__dict__.get("_clip") is not None and groups:
            coef = self._norm_launch([g for _, g in groups], scale, found_inf)
        else:
            for gi, (group, params, grads, ms, vs, word) in groups:
                lists, kw = self._launch_args(gi, params, grads, ms, vs)
                C.adam.nonfinite_check(lists[1], found_inf, **kw)
        for gi, (group, params, grads, ms, vs, word) in groups:
            self._native_step(gi, group, params, grads, ms, vs, word, found_inf, scale, coef)
        C.optim.update_scale(scale, tracker, found_inf, growth, backoff, interval)


class AdamW(Adam):
    _decoupled = True  # p *= 1 - lr*wd before the update

    def __init__(self, params, lr: float = 1e-3, betas: tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, amsgrad: bool = False, *, maximize: bool = False):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize=maximize)
