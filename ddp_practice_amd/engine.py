"""Training / evaluation loops shared by the CLIs and the benchmark.

The per-batch semantics are the reference's
(/root/reference/ddp_main.py:83-93 ``train`` and :96-112 ``test``):

    outputs = model(images); loss = criterion(outputs, labels)
    optimizer.zero_grad(); scaler.scale(loss).backward()
    scaler.step(optimizer); scaler.update()

On a HIP device the step for full batches is captured once into a hipGraph
(``runtime.CapturedStep``) and replayed; the batch position lives in a device
counter advanced by the gather kernel, so an epoch is ``n_full / K`` graph
replays plus (if the sampler leaves one) a partial last batch run eagerly.
The warm-up iteration that capture needs is undone (model, buffers,
optimizer and scaler state are snapshotted and restored), so the sequence of
optimizer steps is exactly the reference's.  On CPU the same loop runs eagerly.
"""
from __future__ import annotations

import contextlib

import torch

from .data.loader import DeviceLoader
from .runtime.graph import CapturedStep
from .utils.trace import trace_range


def _snapshot(model, optimizer, scaler, scheduler=None):
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    opt = {id(p): {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}
           for p, st in optimizer.state.items()}
    sc = None
    if scaler is not None and getattr(scaler, "_scale", None) is not None:
        sc = (scaler._scale.clone(), scaler._growth_tracker.clone(), scaler._found_inf.clone())
    # a device-resident schedule (optim.DeviceLR): its position and lr words, which the
    # warm-up steps of a capture advance like everything else
    lr = scheduler._snapshot() if hasattr(scheduler, "_snapshot") else None
    return sd, opt, sc, lr


def _restore(model, optimizer, scaler, snap, scheduler=None):
    sd, opt, sc, lr = snap
    with torch.no_grad():
        for k, v in model.state_dict().items():
            v.copy_(sd[k])
    for p in list(optimizer.state.keys()):
        if id(p) in opt:
            for k, v in opt[id(p)].items():
                if torch.is_tensor(v):
                    optimizer.state[p][k].copy_(v)
                else:
                    optimizer.state[p][k] = v
        else:
            # state created by the warm-up step: keep the tensors (a captured graph
            # may reference them) but reset them
            for k, v in optimizer.state[p].items():
                if torch.is_tensor(v):
                    v.zero_()
    if sc is not None:
        scaler._scale.copy_(sc[0])
        scaler._growth_tracker.copy_(sc[1])
        scaler._found_inf.copy_(sc[2])
    if lr is not None:
        scheduler._restore(lr)


class TrainLoop:
    """Epoch runner: graph-replayed full batches + eager tail batch."""

    def __init__(self, model, criterion, optimizer, loader: DeviceLoader, scaler=None, use_graph: bool = True,
                 steps_per_graph: int = 16, watchdog=None, faults=None, scheduler=None,
                 scheduler_interval: str = "step", clip_grad_norm: float | None = None, ema=None,
                 accum_steps: int = 1, accum_impl: str = "native"):
        self.model = model
        self.criterion = criterion
        self.optimizer = optimizer
        self.loader = loader
        self.scaler = scaler
        # scheduler: optim.DeviceLR (its step() is one launch, captured with the step) or, on
        # an eager loop, any torch scheduler.  "step": stepped after every optimizer update,
        # unconditionally as a torch loop does (a step found_inf skipped still advances);
        # "epoch": once at the end of run_epoch, eagerly
        if scheduler_interval not in ("step", "epoch"):
            raise ValueError(f"scheduler_interval must be 'step' or 'epoch', not {scheduler_interval!r}")
        self.scheduler = scheduler
        self.scheduler_interval = scheduler_interval
        if scheduler is not None and use_graph and loader.device.type == "cuda" and not hasattr(scheduler, "_snapshot"):
            # a host-side scheduler edits param_groups[i]["lr"], which a replayed graph never reads
            raise ValueError("TrainLoop: a captured step replays the learning rate it was captured with; use "
                             "optim.DeviceLR (DeviceLR.from_torch compiles a torch scheduler) or use_graph=False")
        # ema: optim.EMA (its update() is one launch, captured with the step, whose update count
        # lives on the device) or, on an eager loop, torch's AveragedModel.  Updated after every
        # optimizer update, unconditionally as a torch loop that calls update_parameters after
        # scaler.step does (a step found_inf skipped still updates the average)
        self.ema = ema
        if ema is not None and use_graph and loader.device.type == "cuda" and not hasattr(ema, "_snapshot"):
            # torch's update_parameters branches on bool(n_averaged == 0) on the host
            raise ValueError("TrainLoop: a captured step replays the host branch an averaged model took at "
                             "capture (copy or average, forever); use optim.EMA or use_graph=False")
        self.device = loader.device
        self.use_graph = use_graph and self.device.type == "cuda"
        self.spg = max(1, steps_per_graph)
        self.images, self.labels = loader.static_batch()
        self._graphs: dict[int, CapturedStep] = {}
        self.graph_error = None
        self.watchdog = watchdog  # utils.Watchdog: ticked after every chunk of steps
        self.faults = faults if faults else None  # utils.FaultInjector (DPA_FAULT)
        # DDP + fused AMP step: the optimizer kernel averages the gradients over xGMI
        # (parallel/ddp.py defer_grad_sync_to; a no-op without the engine)
        # (fp32 without a scaler: the optimizer's plain step is the same fused launch, optim/sgd.py)
        fused = (getattr(scaler, "_enabled", False) if scaler is not None
                 else getattr(optimizer, "plain_fused", False))
        if fused and hasattr(model, "defer_grad_sync_to"):
            if model.defer_grad_sync_to(optimizer):
                model.set_slab_sink(optimizer)  # and the conv1 slab sums (exchanged in the same launch)
        elif fused and hasattr(model, "set_slab_sink"):
            # no DDP: the fused step also sums the conv1 weight-gradient slab (models/convnet.py)
            model.set_slab_sink(optimizer)
        # clip_grad_norm: the global gradient norm is clipped to it before every update.  The
        # native Adam family does it inside its own step (optim/adamw.py set_grad_clip: nothing
        # changes in _step); optim.SGD through optim.clip_grad_norm_ between unscale_ and step
        # (its unfused route); any other optimizer through torch's function, so the --impl
        # torch runs stay an independent reference
        self.clip_grad_norm = None if clip_grad_norm is None else float(clip_grad_norm)
        self._clip_mode = None
        self._norm_words = None  # [norm, coefficient] of the last step (the two non-fused routes)
        if self.clip_grad_norm is not None:
            if not self.clip_grad_norm > 0.0:
                raise ValueError(f"clip_grad_norm must be positive, not {clip_grad_norm!r}")
            from .optim import SGD

            if hasattr(optimizer, "set_grad_clip"):
                optimizer.set_grad_clip(self.clip_grad_norm)
                self._clip_mode = "fused"
            else:
                self._clip_mode = "native" if isinstance(optimizer, SGD) else "torch"
                self._norm_words = torch.tensor([0.0, 1.0], dtype=torch.float32, device=self.device)
        # accum_steps K > 1: an optimizer update per window of K micro-batches (optim/accum.py).
        # Created after the deferral above: the accumulator asks who owns the DDP average.
        # global_step, the fault steps, the watchdog note, the EMA count, Adam's step word and
        # the DeviceLR position all count optimizer updates, not micro-batches
        if isinstance(accum_steps, bool) or not isinstance(accum_steps, int) or accum_steps < 1:
            raise ValueError(f"accum_steps must be an int >= 1, not {accum_steps!r}")
        if accum_impl not in ("native", "torch"):
            raise ValueError(f"accum_impl must be 'native' or 'torch', not {accum_impl!r}")
        self.accum_steps = accum_steps
        # accum_impl "torch": the textbook idiom instead (loss / K, autograd's accumulation into
        # .grad, no_sync() on the non-final micro-steps), the --impl torch runs' reference
        self.accum = None
        if accum_steps > 1 and accum_impl == "native":
            from .optim import GradAccumulator

            self.accum = GradAccumulator(optimizer, accum_steps, model if hasattr(model, "no_sync") else None)
        self.global_step = 0
        # the model's first kernel gathers the batch itself (no gather launch per step)
        from .data.loader import accepts_deferred

        self._defer = accepts_deferred(model, self.images)

    @property
    def grad_norm(self):
        """The last step's total gradient norm before clipping (a 0-d device tensor; None
        without ``clip_grad_norm``)."""
        if self._clip_mode == "fused":
            return self.optimizer.grad_norm
        return None if self._norm_words is None else self._norm_words[0]

    def _clip(self):
        """Clip the (unscaled, complete) gradients in place; the norm goes to ``_norm_words``."""
        params = [p for g in self.optimizer.param_groups for p in g["params"] if p.grad is not None]
        if self._clip_mode == "native":
            from .optim import clip as K

            grads = [p.grad for p in params]
            if K.native_ok(grads):
                K.clip_grads_(grads, self.clip_grad_norm, self._norm_words)
                return
        norm = torch.nn.utils.clip_grad_norm_(params, self.clip_grad_norm)
        self._norm_words[0].copy_(norm)

    # -- one step on the static buffers (what gets captured)
    def _step(self, images=None, labels=None, fill=True, before_update=None):
        if fill:
            self.loader.fill_(self.images, self.labels, defer=self._defer)
        images = self.images if images is None else images
        labels = self.labels if labels is None else labels
        with trace_range("forward"):
            outputs = self.model(images)
            loss = self.criterion(outputs, labels)
        self.optimizer.zero_grad(set_to_none=True)
        if self.scaler is not None:
            with trace_range("backward"):
                self.scaler.scale(loss).backward()
        else:
            with trace_range("backward"):
                loss.backward()
        self._update(before_update)
        return loss

    def _update(self, before_update=None):
        """The optimizer update over complete gradients: unscale / clip / step / scale update,
        then the weight average and the per-step schedule."""
        if self.scaler is not None:
            if before_update is not None:
                flush = getattr(self.optimizer, "_flush_deferred", None)
                if flush is not None:
                    flush()  # the hook reads .grad
                before_update()
            with trace_range("optimizer"):
                if self._norm_words is not None:
                    self.scaler.unscale_(self.optimizer)  # (the native scaler's flushes first)
                    self._clip()
                self.scaler.step(self.optimizer)
                self.scaler.update()
        else:
            if before_update is not None:
                before_update()
            with trace_range("optimizer"):
                if self._norm_words is not None:
                    flush = getattr(self.optimizer, "_flush_deferred", None)
                    if flush is not None:
                        flush()
                    self._clip()
                self.optimizer.step()
        if self.ema is not None:
            self._ema_update()
        if self.scheduler is not None and self.scheduler_interval == "step":
            self.scheduler.step()

    # -- one window of micro-steps and its update (accum_steps > 1; what gets captured)
    def _window(self, items=None, before_update=None):
        """``items``: one entry per micro-step, None (the next full batch, filled into the static
        buffers) or an (images, labels) pair already filled; default: ``accum_steps`` full
        batches.  The last entry closes the window, however short it is."""
        items = [None] * self.accum_steps if items is None else items
        idiom = self.accum is None
        if idiom:
            self.optimizer.zero_grad(set_to_none=True)
        loss = None
        for i, it in enumerate(items):
            last = i == len(items) - 1
            if it is None:
                self.loader.fill_(self.images, self.labels, defer=self._defer)
                images, labels = self.images, self.labels
            else:
                images, labels = it
            if not idiom:
                ctx = self.accum.micro_step()
            elif not last and hasattr(self.model, "no_sync"):
                ctx = self.model.no_sync()
            else:
                ctx = contextlib.nullcontext()
            with ctx:
                with trace_range("forward"):
                    outputs = self.model(images)
                    loss = self.criterion(outputs, labels)
                if idiom:
                    loss = loss / self.accum_steps
                else:
                    self.optimizer.zero_grad(set_to_none=True)
                with trace_range("backward"):
                    (self.scaler.scale(loss) if self.scaler is not None else loss).backward()
            if not idiom:
                with trace_range("accumulate"):
                    done = self.accum.accumulate(last=last)
                assert done == last
        self._update(before_update)
        return loss

    def _ema_update(self):
        if hasattr(self.ema, "update_parameters"):  # torch.optim.swa_utils.AveragedModel (eager loops)
            m = self.model
            wrapped = type(m).__name__ == "DistributedDataParallel" and hasattr(m, "module")
            self.ema.update_parameters(m.module if wrapped else m)
        else:
            self.ema.update()

    def _snapshot_all(self):
        return (_snapshot(self.model, self.optimizer, self.scaler, self.scheduler),
                self.ema._snapshot() if self.ema is not None else None)

    def _restore_all(self, snap):
        _restore(self.model, self.optimizer, self.scaler, snap[0], self.scheduler)
        if snap[1] is not None:
            self.ema._restore(snap[1])

    def _eager_step(self, images=None, labels=None, fill=True, items=None):
        """One un-captured update (CPU, tail batches, steps with an injected fault): a step, or with
        accum_steps > 1 a window (``items``: see ``_window``)."""
        step = self.global_step
        hook = None
        if self.faults is not None:
            self.faults.before_step(step)
            params = [p for g in self.optimizer.param_groups for p in g["params"]]
            hook = lambda: self.faults.corrupt_grads(step, params)  # noqa: E731
        if self.accum_steps > 1:
            self._window(items, before_update=hook)
        else:
            self._step(images, labels, fill=fill, before_update=hook)
        self.global_step += 1
        self._tick()

    def _tick(self):
        if self.watchdog is not None:
            self.watchdog.note(f"{self.global_step} training steps queued")
            self.watchdog.tick()

    def _graph(self, k: int) -> CapturedStep | None:
        if not self.use_graph:
            return None
        if k in self._graphs:
            return self._graphs[k]
        snap = self._snapshot_all()
        # accum_steps > 1: a graph holds k whole windows
        g = CapturedStep((lambda: self._window()) if self.accum_steps > 1 else (lambda: self._step()),
                         warmup=2, steps_per_graph=k,
                         pre_capture=lambda: self._restore_all(snap))
        ctr = self.loader._ctr.clone() if self.loader._ctr is not None else None
        ok = g.capture()
        # undo the warm-up step's data consumption and parameter update
        self._restore_all(snap)
        if ctr is not None:
            self.loader._ctr.copy_(ctr)
        if not ok:
            self.graph_error = g.capture_error
            self.use_graph = False
            return None
        self._graphs[k] = g
        return g

    def _run_epoch_windows(self) -> None:
        """run_epoch with accum_steps K > 1: ``nfull // K`` whole windows, graph-replayed in
        graphs of ``max(1, steps_per_graph // K)`` windows (about today's micro-steps per
        graph) and then of one; the epoch's last window is short when the batches are no
        multiple of K -- the leftover full batches plus the sampler's partial tail batch --
        and runs eagerly.  A window never spans an epoch."""
        K = self.accum_steps
        sizes = self.loader.batch_sizes()
        B = self.loader.batch_size
        nfull = sum(1 for b in sizes if b == B)
        tail = [b for b in sizes if b != B]
        self.loader.start_epoch()
        if self.accum is not None:
            self.accum.reset()
        nwin, left = divmod(nfull, K)
        wpg = max(1, self.spg // K)
        done = 0
        faults = self.faults
        with trace_range("train_epoch"):
            if self.use_graph and nwin > 0:
                big = self._graph(wpg) if (wpg > 1 and nwin >= wpg) else None
                while big is not None and nwin - done >= wpg:
                    if faults is not None and faults.pending_in(self.global_step, self.global_step + wpg):
                        break  # run the chunk holding the faulty update window by window
                    big.run()
                    done += wpg
                    self.global_step += wpg
                    self._tick()
                if nwin - done > 0:
                    one = self._graph(1)
                    while one is not None and done < nwin:
                        if faults is not None and faults.pending_in(self.global_step, self.global_step + 1):
                            self._eager_step()
                        else:
                            one.run()
                            self.global_step += 1
                            self._tick()
                        done += 1
            while done < nwin:  # eager fallback (CPU, or capture failed)
                self._eager_step()
                done += 1
            items = [None] * left
            for i, b in enumerate(tail):
                imgs, labels = self.loader.static_batch(b)
                self.loader._fill_tail(imgs, labels, nfull + i)
                items.append((imgs, labels))
            for s in range(0, len(items), K):
                self._eager_step(items=items[s:s + K])
        if self.scheduler is not None and self.scheduler_interval == "epoch":
            self.scheduler.step()

    def run_epoch(self) -> None:
        self.model.train()
        if self.accum_steps > 1:
            return self._run_epoch_windows()
        sizes = self.loader.batch_sizes()
        B = self.loader.batch_size
        nfull = sum(1 for b in sizes if b == B)
        tail = [b for b in sizes if b != B]
        self.loader.start_epoch()
        done = 0
        faults = self.faults
        with trace_range("train_epoch"):
            if self.use_graph and nfull > 0:
                big = self._graph(self.spg) if nfull >= self.spg else None
                while big is not None and nfull - done >= self.spg:
                    if faults is not None and faults.pending_in(self.global_step, self.global_step + self.spg):
                        break  # run the chunk holding the fault step by step
                    big.run()
                    done += self.spg
                    self.global_step += self.spg
                    self._tick()
                if nfull - done > 0:
                    one = self._graph(1)
                    while one is not None and done < nfull:
                        if faults is not None and faults.pending_in(self.global_step, self.global_step + 1):
                            self._eager_step()
                        else:
                            one.run()
                            self.global_step += 1
                            self._tick()
                        done += 1
            while done < nfull:  # eager fallback (CPU, or capture failed)
                self._eager_step()
                done += 1
            for i, b in enumerate(tail):
                imgs, labels = self.loader.static_batch(b)
                self.loader._fill_tail(imgs, labels, nfull + i)
                self._eager_step(imgs, labels, fill=False)
        if self.scheduler is not None and self.scheduler_interval == "epoch":
            self.scheduler.step()


@torch.no_grad()
def evaluate(model, loader: DeviceLoader, comm=None, dst: int = 0, native: bool = True):
    """Reference ``test()``: global accuracy reduced to rank ``dst`` (ddp_main.py:96-112).

    Returns (correct, size) as floats on rank ``dst`` (other ranks: their local values).
    ``native=False`` counts with torch ops (the ``--impl torch`` runs).
    """
    model.eval()
    dev = loader.device
    counters = torch.zeros(2, dtype=torch.float32, device=dev)
    native = native and dev.type == "cuda"
    if native:
        from .ops.head import accuracy_
    for images, labels in loader:
        out = model(images)
        if native:
            accuracy_(out, labels, counters)
        else:
            counters[0] += images.shape[0]
            counters[1] += (out.argmax(1) == labels).float().sum()
    if comm is not None and comm.active:
        comm.reduce_(counters, dst, "sum")
    size, correct = counters.tolist()
    return correct, size


@contextlib.contextmanager
def maybe_profile(enabled: bool, path: str):
    if not enabled:
        yield
        return
    from torch.profiler import ProfilerActivity, profile

    acts = [ProfilerActivity.CPU] + ([ProfilerActivity.CUDA] if torch.cuda.is_available() else [])
    with profile(activities=acts) as prof:
        yield
    prof.export_chrome_trace(path)
