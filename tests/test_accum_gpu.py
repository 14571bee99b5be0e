"""csrc/kernels/accum.hip and optim.GradAccumulator on the GPU: every mode at zero tolerance against
the torch ops over the granule space's edge sizes, misaligned pointers and row counts (by value
and through the table) with guard words behind every accumulator and gradient, non-finite values
through the fused AMP step, a whole window against the float64 reference of tests/_accum_ref.py,
graph replay of a captured window, and ``TrainLoop(accum_steps=)`` on the ConvNet."""
import copy
import gc

import pytest
import torch

from . import _accum_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD = 8          # guard words behind every accumulator and every gradient
GUARD = 12345.0  # their value: the kernel must not write a lane past a tensor's end


def _bits(t):
    t = t.detach().contiguous().reshape(-1)
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int64)


def _exact(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, i)
        if not torch.equal(_bits(a), _bits(b)):
            d = (a.double() - b.double()).abs().max().item() if a.is_floating_point() else None
            raise AssertionError(f"{what}: tensor {i} of {tuple(a.shape)} differs (max abs {d})")


def _guarded(x, offset=0):
    """A copy of ``x`` inside a larger buffer: ``offset`` words in, GUARD in front and behind."""
    buf = torch.full((offset + x.numel() + PAD,), GUARD, dtype=torch.float32, device=DEV)
    buf[offset:offset + x.numel()] = x.reshape(-1)
    return buf, buf[offset:offset + x.numel()].view(x.shape)


def _guards_intact(bufs, views, offset):
    for buf, v in zip(bufs, views):
        assert bool((buf[:offset] == GUARD).all()) and bool((buf[offset + v.numel():] == GUARD).all())


def _launch(C, A, G, mode, c=1.0):
    K = C.accum
    if len(A) <= K.MAXT:
        K.accumulate(A, G, mode, c)
    else:
        table = K.accum_table(A, G)
        K.accumulate([], [], mode, c, table=table, total_granules=sum((g.numel() + 3) // 4 for g in G))


def _check_modes(C, sizes, a_off=0, g_off=0, Ks=(2, 3, 7)):
    """FIRST gives acc the bits of g, ADD equals acc + g, LAST equals (acc + g) * c with acc
    untouched and SCALE equals g * c, each against the torch op on the same device."""
    K = C.accum
    gen = torch.Generator().manual_seed(len(sizes) * 7919 + sizes[0])
    a0 = [torch.randn(s, generator=gen).to(DEV) for s in sizes]
    g0 = [torch.randn(s, generator=gen).to(DEV) for s in sizes]
    for g in g0:
        g[0] = -0.0  # FIRST moves bits: the sign of a zero survives
        if g.numel() > 2:
            g[2] = 1e-41  # and a subnormal
    abufs, A = map(list, zip(*[_guarded(x, a_off) for x in a0]))
    gbufs, G = map(list, zip(*[_guarded(x, g_off) for x in g0]))
    if a_off:
        assert all(a.data_ptr() % 16 == 4 * a_off for a in A)
    if g_off:
        assert all(g.data_ptr() % 16 == 4 * g_off for g in G)

    def settle(what):
        torch.cuda.synchronize()
        _guards_intact(abufs, A, a_off)
        _guards_intact(gbufs, G, g_off)

    _launch(C, A, G, K.FIRST)
    settle("first")
    _exact(A, g0, "first: acc has the bits of g")
    _exact(G, g0, "first: g is only read")
    assert all(torch.signbit(a.reshape(-1)[0]) for a in A)
    for a, x in zip(A, a0):
        a.copy_(x)
    _launch(C, A, G, K.ADD)
    settle("add")
    _exact(A, [x + g for x, g in zip(a0, g0)], "add: acc + g")
    _exact(G, g0, "add: g is only read")
    for k in Ks:
        c = torch.tensor(1.0 / k, dtype=torch.float32).item()
        for a, x, g, y in zip(A, a0, G, g0):
            a.copy_(x)
            g.copy_(y)
        _launch(C, A, G, K.LAST, 1.0 / k)
        settle("last")
        _exact(G, [(x + g) * c for x, g in zip(a0, g0)], f"last: (acc + g) * c, K = {k}")
        _exact(A, a0, "last: acc is not written")
        for g, y in zip(G, g0):
            g.copy_(y)
        _launch(C, A, G, K.SCALE, 1.0 / k)
        settle("scale")
        _exact(G, [g * c for g in g0], f"scale: g * c, K = {k}")
        _exact(A, a0, "scale: acc is not touched")


# ---------------------------------------------------------------- 1. the modes, bit for bit
@pytest.mark.parametrize("nt", [False, True], ids=["plain", "nt"])
@pytest.mark.parametrize("u", [0, 2, 4])
def test_edge_sizes_equal_the_torch_ops(C, u, nt):
    """Sizes 1, 3, 4, 5, one chunk, one chunk + 1 and what follows them: with 5 granules in front,
    the chunk-sized tensor straddles the first chunk edge.  u: granules per lane and chunk (0: the
    by-size rule, 1 for a launch this small); nt: non-temporal loads of the accumulator."""
    chunk = C.accum.THR * max(u, 1) * 4  # elements
    C.accum.set_variant(u, nt)
    try:
        _check_modes(C, [1, 3, 4, 5, chunk, chunk + 1, 2 * chunk - 3, 7])
    finally:
        C.accum.set_variant(0, False)


@pytest.mark.parametrize("a_off,g_off", [(1, 1), (1, 0), (0, 1)], ids=["both", "acc-only", "grad-only"])
def test_misaligned_rows_equal_the_torch_ops(C, a_off, g_off):
    """An accumulator and / or a gradient 4 bytes into its storage: every granule moves per element."""
    chunk = C.accum.THR * 4
    _check_modes(C, [1, 3, 4, 5, chunk + 1, 9], a_off, g_off, Ks=(3,))


@pytest.mark.parametrize("rows", [1, 36, 37, 161])
def test_row_counts_equal_the_torch_ops(C, rows):
    """1 / 36 rows by value, 37 / 161 through the device table."""
    assert C.accum.MAXT == 36 and C.accum.LARGE_MAXT == 512
    gen = torch.Generator().manual_seed(rows)
    sizes = [int(torch.randint(1, 70, (1,), generator=gen)) for _ in range(rows)]
    sizes[rows // 2] = C.accum.THR * 4 + 2
    _check_modes(C, sizes, Ks=(3,))


def test_a_launch_of_many_workgroups(C):
    """More chunks than the grid's cap of workgroups: the grid-stride walk covers every granule."""
    numel = C.accum.THR * 4 * 2500 + 13
    gen = torch.Generator().manual_seed(11)
    a, g = torch.randn(numel, generator=gen).to(DEV), torch.randn(numel, generator=gen).to(DEV)
    acc = a.clone()
    _launch(C, [acc], [g], C.accum.ADD)
    _exact([acc], [a + g], "add over 2500 chunks")
    g2 = g.clone()
    _launch(C, [acc], [g2], C.accum.LAST, 1.0 / 3)
    _exact([g2], [((a + g) + g) * torch.tensor(1.0 / 3, dtype=torch.float32).item()], "last over 2500 chunks")


def test_launch_checks(C):
    a, g = torch.zeros(8, device=DEV), torch.zeros(8, device=DEV)
    with pytest.raises(RuntimeError, match="aliases"):
        C.accum.accumulate([a], [a], C.accum.ADD, 1.0)
    with pytest.raises(RuntimeError, match="size"):
        C.accum.accumulate([a], [g[:7]], C.accum.ADD, 1.0)
    with pytest.raises(RuntimeError, match="f32"):
        C.accum.accumulate([a], [g.double()], C.accum.ADD, 1.0)
    with pytest.raises(RuntimeError, match="mode"):
        C.accum.accumulate([a], [g], 4, 1.0)
    with pytest.raises(RuntimeError, match="rows by value"):
        C.accum.accumulate([a] * 37, [g] * 37, C.accum.FIRST, 1.0)


# ---------------------------------------------------------------- 2. the class
class _Bag(torch.nn.Module):
    """``count`` parameters of odd sizes; ``fresh_grads(i)`` is what a backward does: new gradient
    tensors (``.grad`` must be None), from capturable ops that depend on the weights."""

    def __init__(self, count, seed=0):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(5 + 3 * i, generator=gen))
                                          for i in range(count)])

    def fresh_grads(self, i):
        with torch.no_grad():
            gs = torch._foreach_mul(list(self.ps), 0.37 + 0.11 * i)
            torch._foreach_add_(gs, 0.05 * (i + 1))
        for p, g in zip(self.ps, gs):
            assert p.grad is None
            p.grad = g


def test_whole_window_within_the_counted_bound(C):
    """K = 3 on random gradients of mixed magnitude: within the bound counted in tests/_accum_ref.py."""
    from ddp_practice_amd.optim import GradAccumulator

    gen = torch.Generator().manual_seed(3)
    ps = [torch.nn.Parameter(torch.zeros(n, device=DEV)) for n in (2051, 7, 1024)]
    acc = GradAccumulator(torch.optim.SGD(ps, lr=0.1), steps=3)
    seen = []
    for i in range(3):
        gs = [torch.randn(p.shape, generator=gen) * (10.0 ** (i - 1)) for p in ps]
        gs[0][:5] = torch.tensor([1e-30, -1e-38, 0.0, 3e38 if i == 0 else -1e38, 1.0])
        seen.append(gs)
        for p, g in zip(ps, gs):
            p.grad = g.to(DEV)
        done = acc.accumulate()
    torch.cuda.synchronize()
    assert done and acc.launches == 3
    worst = 0.0
    for j, p in enumerate(ps):
        mean, bound, _ = R.window([s[j] for s in seen], 3)
        err = (p.grad.cpu().double() - mean).abs()
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), worst
        _exact([p.grad.cpu()], [R.kernel_loop([s[j] for s in seen], 3)], "the torch ops on the CPU")
    print(f"K = 3 window: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("vals,want", [((float("inf"), 1.0, 2.0), "inf"), ((float("inf"), float("-inf"), 2.0), "nan"),
                                       ((1.0, float("nan"), 2.0), "nan")])
def test_non_finite_values_propagate(C, vals, want):
    from ddp_practice_amd.optim import GradAccumulator

    p = torch.nn.Parameter(torch.zeros(70, device=DEV))
    acc = GradAccumulator(torch.optim.SGD([p], lr=0.1), steps=3)
    for v in vals:
        p.grad = torch.ones(70, device=DEV)
        p.grad[33] = v
        done = acc.accumulate()
    assert done
    x = p.grad[33]
    assert bool(torch.isinf(x)) if want == "inf" else bool(torch.isnan(x))
    assert bool(torch.isfinite(torch.cat([p.grad[:33], p.grad[34:]])).all())


def test_non_finite_window_skips_the_fused_amp_step(C):
    """An inf in micro-step 0 of 3 reaches the fused AMP-SGD step's found_inf: the parameters stay
    as they are and the scale backs off (the fused launch re-arms the found_inf word itself)."""
    from ddp_practice_amd.amp import GradScaler
    from ddp_practice_amd.optim import SGD, GradAccumulator

    gc.collect()
    m = _Bag(5).to(DEV)
    opt = SGD(m.parameters(), lr=0.1)
    acc = GradAccumulator(opt, steps=3)
    scaler = GradScaler(init_scale=4.0)
    scaler._lazy_init(DEV)  # the scale words, as the first scale(loss) creates them
    before = None
    for window, poison in enumerate((False, False, True)):
        if poison:
            before = [p.detach().clone() for p in m.ps]
        for i in range(3):
            opt.zero_grad(set_to_none=True)
            m.fresh_grads(i)
            if i == 0 and poison:
                m.ps[2].grad[4] = float("inf")
            done = acc.accumulate()
        assert done
        if poison:
            assert bool(torch.isinf(m.ps[2].grad[4]))
        scaler.step(opt)
        fused = scaler._fused_done
        scaler.update()
        if window >= 1:
            assert fused  # the one-launch route (from the second iteration on)
    torch.cuda.synchronize()
    assert scaler.get_scale() == 2.0  # backed off once
    _exact([p.detach() for p in m.ps], before, "parameters after the skipped update")


@pytest.mark.parametrize("opt_name", ["AdamW", "SGD"])
@pytest.mark.parametrize("count", [4, 60], ids=["by-value", "table"])
def test_captured_window_replayed_equals_eager(C, opt_name, count):
    """One captured window (K = 2) replayed 4 times == 4 eager windows, bitwise; Adam's step word
    counts 4 updates.  The accumulators exist since the constructor; the row table of 60 rows is
    written by a launch on the stream, so the one a capture builds for its own gradient tensors is
    part of the graph."""
    from ddp_practice_amd import optim

    kw = dict(lr=1e-2, weight_decay=0.01) if opt_name == "AdamW" else dict(lr=1e-2, momentum=0.9)

    def make():
        m = _Bag(count).to(DEV)
        o = getattr(optim, opt_name)(m.parameters(), **kw)
        return m, o, optim.GradAccumulator(o, steps=2)

    def window(m, o, a):
        for i in range(2):
            o.zero_grad(set_to_none=True)
            m.fresh_grads(i)
            done = a.accumulate()
        assert done
        o.step()

    ma, oa, aa = make()
    for _ in range(4):
        window(ma, oa, aa)
    mb, ob, ab = make()
    flat = ab._flat[DEV]
    snap = [p.detach().clone() for p in mb.ps]
    window(mb, ob, ab)  # the optimizer's state and words exist before capture
    with torch.no_grad():
        for p, s in zip(mb.ps, snap):
            p.copy_(s)
        for st in ob.state.values():
            for v in st.values():
                if torch.is_tensor(v):
                    v.zero_()
    ob.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        window(mb, ob, ab)
    assert ab._flat[DEV] is flat and ab.position == 0
    if count > C.accum.MAXT:
        assert len(ab._tables_pinned) >= 1
    _exact([p.detach() for p in mb.ps], snap, "capture runs nothing")
    for _ in range(4):
        graph.replay()
    torch.cuda.synchronize()
    _exact([p.detach() for p in mb.ps], [p.detach() for p in ma.ps], "replayed windows vs eager")
    assert not torch.equal(mb.ps[0].detach(), snap[0])
    if opt_name == "AdamW":
        assert float(ob.state[mb.ps[0]]["step"]) == 4.0 == float(oa.state[ma.ps[0]]["step"])
    del graph


def test_more_rows_than_the_table_holds_take_the_fallback(C, monkeypatch):
    from ddp_practice_amd.optim import GradAccumulator

    count = C.accum.LARGE_MAXT + 1
    m = _Bag(count).to(DEV)
    acc = GradAccumulator(torch.optim.SGD(m.parameters(), lr=0.1), steps=2)

    def no_native(*a, **k):
        raise AssertionError("the native launch with more rows than LARGE_MAXT")

    monkeypatch.setattr(C.accum, "accumulate", no_native)
    seen = []
    for i in range(2):
        for p in m.ps:
            p.grad = None
        m.fresh_grads(i)
        seen.append([p.grad.clone() for p in m.ps])
        done = acc.accumulate()
    assert done
    _exact([p.grad for p in m.ps], [(a + b) * 0.5 for a, b in zip(*seen)], "fallback vs the torch ops")


# ---------------------------------------------------------------- 3. ConvNet through TrainLoop
def _convnet_loop(base, ds, opt_name, amp, use_graph, K, extras=False):
    from ddp_practice_amd import optim
    from ddp_practice_amd.amp import GradScaler
    from ddp_practice_amd.data import DeviceLoader
    from ddp_practice_amd.engine import TrainLoop
    from ddp_practice_amd.nn import CrossEntropyLoss

    model = copy.deepcopy(base)
    loader = DeviceLoader(ds, batch_size=8, shuffle=False, device=DEV, dtype=torch.bfloat16 if amp else torch.float32)
    kw = dict(lr=1e-3, weight_decay=0.01) if opt_name == "AdamW" else dict(lr=1e-2)
    opt = getattr(optim, opt_name)(model.parameters(), **kw)
    more = {}
    if extras:
        more = dict(clip_grad_norm=0.05, ema=optim.EMA(model, decay=0.9),
                    scheduler=optim.DeviceLR.from_torch(
                        opt, lambda o: torch.optim.lr_scheduler.StepLR(o, step_size=1, gamma=0.5), 8))
    loop = TrainLoop(model, CrossEntropyLoss(), opt, loader, GradScaler() if amp else None, use_graph=use_graph,
                     steps_per_graph=4, accum_steps=K, **more)
    return model, opt, loop


def _hand_written_epoch(loop, K, on_window=None):
    """The same epoch by hand on a TrainLoop(accum_steps=1)'s parts: every micro-step's fresh
    ``.grad`` cloned, the window's mean formed with torch ops (``acc = acc + g``, ``* c``) and
    written where the last micro-step's gradients live, then the loop's own update."""
    loader, opt, scaler = loop.loader, loop.optimizer, loop.scaler
    c = torch.tensor(1.0 / K, dtype=torch.float32).item()
    sizes = loader.batch_sizes()
    nfull = sum(1 for b in sizes if b == loader.batch_size)
    loop.model.train()
    loader.start_epoch()
    for s in range(0, len(sizes), K):
        seen = []
        for i in range(s, min(s + K, len(sizes))):
            if i < nfull:
                loader.fill_(loop.images, loop.labels, defer=loop._defer)
                images, labels = loop.images, loop.labels
            else:
                images, labels = loader.static_batch(sizes[i])
                loader._fill_tail(images, labels, i)
            loss = loop.criterion(loop.model(images), labels)
            opt.zero_grad(set_to_none=True)
            (scaler.scale(loss) if scaler is not None else loss).backward()
            flush = getattr(opt, "flush_slab", None)
            if flush is not None:
                flush()  # .grad is read
            seen.append([p.grad.clone() for p in loop.model.parameters()])
        with torch.no_grad():
            for j, p in enumerate(loop.model.parameters()):
                acc = seen[0][j]
                for g in seen[1:]:
                    acc = acc + g[j]
                p.grad.copy_(acc * c)
        if on_window is not None:
            on_window([p.grad.clone() for p in loop.model.parameters()])
        loop._update()
        loop.global_step += 1


def _plain_backward_sinks(base, ds, opt_name, amp):
    """Whether the backward of a plain step (accum_steps=1) leaves the conv1 slab to the optimizer."""
    model, opt, loop = _convnet_loop(base, ds, opt_name, amp, False, 1)
    model.train()
    loop.loader.start_epoch()
    loop.loader.fill_(loop.images, loop.labels, defer=loop._defer)
    loss = loop.criterion(model(loop.images), loop.labels)
    opt.zero_grad(set_to_none=True)
    (loop.scaler.scale(loss) if amp else loss).backward()
    torch.cuda.synchronize()
    return opt.__dict__.get("_pending_slab") is not None


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("opt_name,amp", [("SGD", True), ("SGD", False), ("AdamW", True), ("AdamW", False)],
                         ids=["sgd-bf16", "sgd-fp32", "adamw-bf16", "adamw-fp32"])
def test_convnet_train_loop_graph_equals_eager_equals_hand_written(C, opt_name, amp, K):
    """Batch 8, 2K full batches and a partial tail: two whole windows (graph-replayed) and a short
    one.  The replayed loop == the eager loop == a hand-written eager loop on the same native
    model, bitwise; the fused producers stay on in every micro-step."""
    from ddp_practice_amd.data import synthetic
    from ddp_practice_amd.models import ConvNet

    gc.collect()  # an uncollected GradScaler of an earlier test
    ds = synthetic(8 * 2 * K + 5, seed=5)
    torch.manual_seed(0)
    base = ConvNet(amp_dtype=torch.bfloat16 if amp else None).to(DEV)
    plain_sinks = _plain_backward_sinks(base, ds, opt_name, amp)
    if opt_name == "SGD" and amp:
        assert plain_sinks  # the flagship configuration: its backward runs the fused tail
    out = []
    for use_graph in (False, True):
        model, opt, loop = _convnet_loop(base, ds, opt_name, amp, use_graph, K)
        sunk = []
        if not use_graph and hasattr(opt, "defer_slab"):
            # what every accumulate() finds: the conv1 slab still deferred to the optimizer, i.e.
            # the backward ran its fused tail (ops/convnet_fused.py drops it when .grad exists)
            inner = loop.accum.accumulate

            def spy(last=None, inner=inner, opt=opt, sunk=sunk):
                sunk.append(opt.__dict__.get("_pending_slab") is not None)
                return inner(last)

            loop.accum.accumulate = spy
        loop.run_epoch()
        torch.cuda.synchronize()
        assert loop.graph_error is None, loop.graph_error
        assert loop.global_step == 3 and loop.accum.launches >= 2 * K + 1
        if sunk:  # every micro-step's backward did what a plain step's does
            assert sunk == [plain_sinks] * (2 * K + 1), sunk
        if opt_name == "AdamW":
            assert float(opt.state[next(iter(model.parameters()))]["step"]) == 3.0
        out.append(model.state_dict())
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), k
    assert not torch.equal(out[0]["fc.weight"], base.state_dict()["fc.weight"])
    model, opt, loop = _convnet_loop(base, ds, opt_name, amp, False, 1)
    _hand_written_epoch(loop, K)
    torch.cuda.synchronize()
    assert loop.global_step == 3
    sd = model.state_dict()
    for k in sd:
        assert torch.equal(sd[k], out[1][k]), k


@pytest.mark.parametrize("opt_name", ["SGD", "AdamW"])
def test_convnet_clip_ema_and_schedule_count_windows(C, opt_name):
    """clip_grad_norm, ema and a DeviceLR attached, K = 2, bf16: the clip norm is the norm of the
    window's mean, and n_averaged, Adam's step and the LR position equal the number of windows."""
    from ddp_practice_amd.data import synthetic
    from ddp_practice_amd.models import ConvNet

    gc.collect()
    K = 2
    ds = synthetic(8 * 2 * K + 5, seed=6)
    torch.manual_seed(0)
    base = ConvNet(amp_dtype=torch.bfloat16).to(DEV)
    out = []
    for use_graph in (False, True):
        model, opt, loop = _convnet_loop(base, ds, opt_name, True, use_graph, K, extras=True)
        loop.run_epoch()
        torch.cuda.synchronize()
        assert loop.graph_error is None, loop.graph_error
        assert loop.global_step == 3 and int(loop.ema.n_averaged) == 3
        assert loop.scheduler.state_dict()["pos"] == 3
        if opt_name == "AdamW":
            assert float(opt.state[next(iter(model.parameters()))]["step"]) == 3.0
        out.append((model.state_dict(), float(loop.grad_norm), list(loop.ema.shadows.values())))
    for k in out[0][0]:
        assert torch.equal(out[0][0][k], out[1][0][k]), k
    assert out[0][1] == out[1][1]
    _exact(out[1][2], out[0][2], "shadows, graph vs eager")
    # by hand: the norm of the last window's mean (unscaled), as a torch loop's clip sees it
    model, opt, loop = _convnet_loop(base, ds, opt_name, True, False, 1, extras=True)
    norms = []

    def norm_of(grads, loop=loop):
        inv = 1.0 / loop.scaler.get_scale()
        norms.append(float(torch.linalg.vector_norm(torch.stack(
            [torch.linalg.vector_norm(g.double() * inv) for g in grads]))))

    _hand_written_epoch(loop, K, on_window=norm_of)
    torch.cuda.synchronize()
    assert len(norms) == 3
    assert out[1][1] == pytest.approx(norms[-1], rel=1e-5)  # float32 norm of 29,034 values against float64
    assert float(loop.grad_norm) == out[1][1]
    sd = model.state_dict()
    for k in sd:
        assert torch.equal(sd[k], out[1][0][k]), k


def test_not_zeroing_grad_drops_the_fused_producers(C):
    """The control of the claim above: the route this feature replaces (keeping ``.grad`` between
    backwards) makes ops/convnet_fused.py drop the slab sink in the second backward."""
    from ddp_practice_amd.data import synthetic
    from ddp_practice_amd.models import ConvNet

    gc.collect()
    ds = synthetic(16, seed=5)
    torch.manual_seed(0)
    base = ConvNet(amp_dtype=torch.bfloat16).to(DEV)
    model, opt, loop = _convnet_loop(base, ds, "SGD", True, False, 1)
    model.train()
    loop.loader.start_epoch()
    sunk = []
    opt.zero_grad(set_to_none=True)
    for _ in range(2):
        loop.loader.fill_(loop.images, loop.labels, defer=loop._defer)
        loop.scaler.scale(loop.criterion(model(loop.images), loop.labels)).backward()
        sunk.append(opt.__dict__.get("_pending_slab") is not None)
    torch.cuda.synchronize()
    assert sunk == [True, False]
