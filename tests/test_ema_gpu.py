"""csrc/kernels/ema.hip and optim.EMA on the GPU: the average against ``torch._foreach_lerp_`` at
zero tolerance over the granule space's edge sizes, misaligned pointers and row counts (by value
and through the table), copy rows and integer rows, the device-resident update count, the
warm-up weights against the float64 reference of tests/_ema_ref.py, graph replay (with torch's
``AveragedModel`` as the control), ``TrainLoop(ema=)`` on the ConvNet, and the fallback."""
import copy
import gc

import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

from . import _ema_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD = 8          # guard words behind every shadow
GUARD = 12345.0  # their value: the kernel must not write a lane past a tensor's end


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int64)


def _exact(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, i)
        if not torch.equal(_bits(a), _bits(b)):
            d = (a.double() - b.double()).abs().max().item() if a.is_floating_point() else None
            raise AssertionError(f"{what}: tensor {i} of {tuple(a.shape)} differs (max abs {d})")


def _lerp(a, b, w):
    out = a.clone()
    torch._foreach_lerp_([out], [b], w)
    return out


def _guarded(x, offset=0):
    """A copy of ``x`` inside a larger buffer: ``offset`` words in, GUARD behind it."""
    buf = torch.full((offset + x.numel() + PAD,), GUARD, dtype=torch.float32, device=DEV)
    buf[offset:offset + x.numel()] = x.reshape(-1)
    return buf, buf[offset:offset + x.numel()].view(x.shape)


def _words(dev=DEV, n=0):
    return torch.full((), n, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)


def _launch(C, S, X, copy_flags, n, ticket, decay, warmup=False):
    E = C.ema
    if len(S) <= E.MAXT:
        E.ema_update(S, X, copy_flags, n, ticket, 1.0 - decay, decay, warmup)
    else:
        table = E.ema_table(S, X, copy_flags)
        total = sum((x.numel() * x.element_size() // 4 + 3) // 4 for x in X)
        E.ema_update([], [], [], n, ticket, 1.0 - decay, decay, warmup, table=table, total_granules=total)


def _check_against_foreach_lerp(C, sizes, decay, offset=0, n0=1):
    gen = torch.Generator().manual_seed(len(sizes) * 7919 + sizes[0])
    a = [torch.randn(s, generator=gen).to(DEV) for s in sizes]
    b = [torch.randn(s, generator=gen).to(DEV) for s in sizes]
    bufs, S = zip(*[_guarded(x, offset) for x in a])
    _, X = zip(*[_guarded(x, offset) for x in b])
    S, X = list(S), list(X)
    if offset:
        assert all(s.data_ptr() % 16 == 4 * offset for s in S)
    want = [x.clone() for x in a]
    torch._foreach_lerp_(want, b, 1.0 - decay)
    n, ticket = _words(n=n0)
    _launch(C, S, X, [False] * len(S), n, ticket, decay)
    torch.cuda.synchronize()
    _exact(S, want, f"ema vs _foreach_lerp_ at decay {decay}")
    _exact(X, b, "the sources are only read")
    for buf, s in zip(bufs, S):
        assert bool((buf[:offset] == GUARD).all()) and bool((buf[offset + s.numel():] == GUARD).all())
    assert int(n) == n0 + 1 and int(ticket) == 0
    assert not any(torch.equal(s, x) for s, x in zip(S, X) if s.numel() > 1)


# ---------------------------------------------------------------- 1. the average, bit for bit
@pytest.mark.parametrize("u", [0, 2, 4])
@pytest.mark.parametrize("decay", [0.999, 0.3])
def test_edge_sizes_equal_foreach_lerp(C, decay, u):
    """Sizes 1, 3, 4, 5, one chunk, one chunk + 1 and what follows them: with 5 granules in front,
    the chunk-sized tensor straddles the first chunk edge.  u: granules per lane and chunk (0: the
    by-size rule, 1 for a launch this small)."""
    chunk = C.ema.THR * max(u, 1) * 4  # elements
    C.ema.set_variant(u)
    try:
        _check_against_foreach_lerp(C, [1, 3, 4, 5, chunk, chunk + 1, 2 * chunk - 3, 7], decay)
    finally:
        C.ema.set_variant(0)


@pytest.mark.parametrize("decay", [0.999, 0.3])
def test_misaligned_rows_equal_foreach_lerp(C, decay):
    """A source and a shadow each 4 bytes into their storage: every granule moves per element."""
    chunk = C.ema.THR * 4
    _check_against_foreach_lerp(C, [1, 3, 4, 5, chunk + 1, 9], decay, offset=1)


def test_only_one_side_misaligned(C):
    gen = torch.Generator().manual_seed(3)
    a, b = torch.randn(1029, generator=gen).to(DEV), torch.randn(1029, generator=gen).to(DEV)
    for so, xo in ((1, 0), (0, 1)):
        _, s = _guarded(a, so)
        _, x = _guarded(b, xo)
        want = _lerp(a, b, 1.0 - 0.999)
        n, ticket = _words(n=3)
        _launch(C, [s], [x], [False], n, ticket, 0.999)
        torch.cuda.synchronize()
        _exact([s], [want], f"shadow offset {so}, source offset {xo}")


@pytest.mark.parametrize("rows", [1, 36, 37, 161])
@pytest.mark.parametrize("decay", [0.999, 0.3])
def test_row_counts_equal_foreach_lerp(C, rows, decay):
    """1 / 36 rows by value, 37 / 161 through the device table."""
    assert C.ema.MAXT == 36 and C.ema.LARGE_MAXT == 512
    gen = torch.Generator().manual_seed(rows)
    sizes = [int(torch.randint(1, 70, (1,), generator=gen)) for _ in range(rows)]
    sizes[rows // 2] = C.ema.THR * 4 + 2
    _check_against_foreach_lerp(C, sizes, decay)


def test_a_launch_of_many_workgroups_counts_once(C):
    """300 chunks and more: every workgroup reads the count before the last one advances it, so
    the whole tensor is averaged (not copied) and the count moves by exactly one, launch after launch."""
    numel = C.ema.THR * 4 * 300 + 13
    gen = torch.Generator().manual_seed(11)
    a, b = torch.randn(numel, generator=gen).to(DEV), torch.randn(numel, generator=gen).to(DEV)
    s = a.clone()
    n, ticket = _words(n=0)
    ref = None
    for k in range(4):
        src = b + float(k)
        _launch(C, [s], [src], [False], n, ticket, 0.3)
        ref = src.clone() if k == 0 else _lerp(ref, src, 1.0 - 0.3)  # the first update copies
        torch.cuda.synchronize()
        assert int(n) == k + 1 and int(ticket) == 0
    _exact([s], [ref], "four launches of 300 workgroups")


# ---------------------------------------------------------------- 2. row kinds
def test_average_and_copy_rows_in_one_launch(C):
    """Float rows averaged, a float row copied, an int64 scalar (two words, value 2**33 + 5), an
    int32 row and an int64 row copied exactly -- bit patterns that are NaNs as floats included."""
    gen = torch.Generator().manual_seed(5)
    f = lambda n: torch.randn(n, generator=gen).to(DEV)  # noqa: E731
    a0, a1, c0 = f(37), f(1030), f(21)
    x0, x1, y0 = f(37), f(1030), f(21)
    big = torch.tensor(2 ** 33 + 5, dtype=torch.int64, device=DEV)
    ints = torch.tensor([-1, 0x7FC00001, -0x00400000], dtype=torch.int32, device=DEV)  # NaN payloads as floats
    longs = torch.tensor([-1, 2 ** 40 + 3, 0x7FF0000000000001, 7, -2 ** 62], dtype=torch.int64, device=DEV)
    S = [a0.clone(), c0.clone(), torch.zeros_like(big), a1.clone(), torch.zeros_like(ints), torch.zeros_like(longs)]
    X = [x0, y0, big, x1, ints, longs]
    flags = [False, True, True, False, True, True]
    n, ticket = _words(n=2)
    _launch(C, S, X, flags, n, ticket, 0.999)
    torch.cuda.synchronize()
    _exact([S[0], S[3]], [_lerp(a0, x0, 1.0 - 0.999), _lerp(a1, x1, 1.0 - 0.999)], "averaged rows")
    _exact([S[1], S[2], S[4], S[5]], [y0, big, ints, longs], "copied rows")
    assert int(S[2]) == 2 ** 33 + 5 and S[2].dtype == torch.int64
    assert int(n) == 3
    with pytest.raises(RuntimeError, match="float32"):
        _launch(C, [S[4]], [ints], [False], n, ticket, 0.999)  # an integer row cannot be averaged
    with pytest.raises(RuntimeError, match="aliases"):
        _launch(C, [x0], [x0], [False], n, ticket, 0.999)
    assert int(n) == 3


# ---------------------------------------------------------------- 3. the count word
@pytest.mark.parametrize("rows", [3, 40])
def test_first_update_copies_second_averages(C, rows):
    gen = torch.Generator().manual_seed(rows)
    a = [torch.randn(50 + i, generator=gen).to(DEV) for i in range(rows)]
    b = [torch.randn(50 + i, generator=gen).to(DEV) for i in range(rows)]
    S = [x.clone() for x in a]
    n, ticket = _words(n=0)
    _launch(C, S, b, [False] * rows, n, ticket, 0.999)
    torch.cuda.synchronize()
    assert int(n) == 1 and int(ticket) == 0
    _exact(S, b, "the first update copies")
    b2 = [x * 2 + 1 for x in b]
    want = [x.clone() for x in S]
    torch._foreach_lerp_(want, b2, 1.0 - 0.999)
    _launch(C, S, b2, [False] * rows, n, ticket, 0.999)
    torch.cuda.synchronize()
    assert int(n) == 2 and int(ticket) == 0
    _exact(S, want, "the second update averages")


# ---------------------------------------------------------------- 4. warm-up
@pytest.mark.parametrize("n0", [1, 2, 9, 10_000])
def test_warmup_within_the_counted_bound(C, n0):
    """Update n uses min(decay, (1 + n) / (10 + n)), computed on the device from the count word:
    against the float64 reference within the bound counted in tests/_ema_ref.py."""
    gen = torch.Generator().manual_seed(n0)
    a = torch.randn(2051, generator=gen) * 3
    b = torch.randn(2051, generator=gen) * 3
    b[:7] = a[:7]                      # D = 0
    a[7:9], b[7:9] = 1e-30, -3e-30     # tiny values
    s = a.to(DEV)
    n, ticket = _words(n=n0)
    _launch(C, [s], [b.to(DEV)], [False], n, ticket, 0.999, warmup=True)
    torch.cuda.synchronize()
    ref, bound = R.update(a, b, n0, 0.999, True)
    err = (s.cpu().double() - ref).abs()
    worst = float((err / bound).max())
    print(f"warm-up update {n0}: decay {R.decay_of(n0, 0.999, True):.6f}, worst error / bound {worst:.3f}")
    assert bool((err <= bound).all()), worst
    assert int(n) == n0 + 1
    if n0 == 10_000:  # the constant decay has won: the update without warm-up, bit for bit
        _exact([s], [_lerp(a.to(DEV), b.to(DEV), 1.0 - 0.999)], "after the warm-up")
    else:
        assert not torch.equal(s, _lerp(a.to(DEV), b.to(DEV), 1.0 - 0.999))


def test_warmup_first_update_copies(C):
    a, b = torch.zeros(9, device=DEV), torch.arange(9.0, device=DEV)
    n, ticket = _words(n=0)
    _launch(C, [a], [b], [False], n, ticket, 0.999, warmup=True)
    torch.cuda.synchronize()
    _exact([a], [b], "update 0 with warm-up")
    assert int(n) == 1


# ---------------------------------------------------------------- 5. the class, graph replay
class _Bag(torch.nn.Module):
    """``count`` parameters of odd sizes and a BatchNorm's buffers (float and int64)."""

    def __init__(self, count, seed=0):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(5 + 3 * i, generator=gen))
                                          for i in range(count)])
        self.bn = torch.nn.BatchNorm1d(6)

    def train_step(self):
        """What a step does to the weights, in capturable ops."""
        with torch.no_grad():
            torch._foreach_mul_(list(self.ps), 1.03125)
            torch._foreach_add_(list(self.ps), 0.25)
            self.bn.running_mean.add_(0.5)
            self.bn.num_batches_tracked.add_(1)


@pytest.mark.parametrize("count,use_buffers", [(4, False), (4, True), (60, False)],
                         ids=["by-value", "by-value-buffers", "table"])
def test_graph_replay_from_zero_equals_eager(C, count, use_buffers):
    """One captured update replayed 8 times from n_averaged == 0 == 8 eager updates, bitwise,
    with n_averaged == 8: the first replay copies, the other seven average."""
    from ddp_practice_amd.optim import EMA

    ma, mb = _Bag(count).to(DEV), _Bag(count).to(DEV)
    ea, eb = EMA(ma, decay=0.9, use_buffers=use_buffers), EMA(mb, decay=0.9, use_buffers=use_buffers)
    for _ in range(8):
        ma.train_step()
        ea.update()
    snap_m = {k: v.clone() for k, v in mb.state_dict().items()}
    snap_e = eb._snapshot()
    mb.train_step()
    eb.update()  # the ticket word and (60 rows) the table exist before capture
    eb._restore(snap_e)
    with torch.no_grad():
        for k, v in mb.state_dict().items():
            v.copy_(snap_m[k])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mb.train_step()
        eb.update()
    assert int(eb.n_averaged) == 0  # capture runs nothing
    for _ in range(8):
        graph.replay()
    torch.cuda.synchronize()
    assert int(ea.n_averaged) == 8 and int(eb.n_averaged) == 8
    _exact(list(eb.shadows.values()), list(ea.shadows.values()), "replayed shadows vs eager")
    assert int(eb.shadows["bn.num_batches_tracked"]) == 8
    assert not torch.equal(eb.shadows["ps.0"], mb.state_dict()["ps.0"])
    # and against torch's AveragedModel run eagerly
    mt = _Bag(count).to(DEV)
    t = AveragedModel(mt, multi_avg_fn=get_ema_multi_avg_fn(0.9), use_buffers=use_buffers)
    for _ in range(8):
        mt.train_step()
        t.update_parameters(mt)
    tsd = t.module.state_dict()
    keys = [k for k in tsd if use_buffers is False or tsd[k].is_floating_point()]
    _exact([eb.shadows[k] for k in keys], [tsd[k] for k in keys], "replayed shadows vs torch's AveragedModel")
    del graph


def test_control_torch_averaged_model_replays_its_captured_branch(C):
    """Control: torch's ``AveragedModel`` captured the same way, from n_averaged == 0.  Its
    ``update_parameters`` takes ``bool(n_averaged == 0)`` on the host (the count is a CPU buffer),
    so the capture succeeds in the copy branch and the graph copies forever: after 8 replays the
    shadows are the model's last weights, not the average, and the host's count is 1 -- it ends
    elsewhere than the 8 eager updates."""
    m, me = _Bag(4).to(DEV), _Bag(4).to(DEV)
    t = AveragedModel(m, multi_avg_fn=get_ema_multi_avg_fn(0.9))
    te = AveragedModel(me, multi_avg_fn=get_ema_multi_avg_fn(0.9))
    for _ in range(8):
        me.train_step()
        te.update_parameters(me)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.train_step()
        t.update_parameters(m)
    for _ in range(8):
        graph.replay()
    torch.cuda.synchronize()
    assert int(te.n_averaged) == 8 and int(t.n_averaged) == 1
    for (k, a), b, live in zip(t.module.state_dict().items(), te.module.state_dict().values(),
                               m.state_dict().values()):
        assert torch.equal(a, live), k  # a copy of the weights
        if k.startswith("ps."):
            assert not torch.equal(a, b), k  # not the average
    del graph


def test_words_must_exist_before_capture(C):
    from ddp_practice_amd.optim import EMA

    for count in (3, 50):
        m = _Bag(count).to(DEV)
        e = EMA(m, decay=0.9)
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="run one eager update first"):
            with torch.cuda.graph(graph):
                e.update()
        torch.cuda.synchronize()
        e.update()  # usable afterwards
        torch.cuda.synchronize()
        assert int(e.n_averaged) == 1


def test_applied_and_state_dict_on_the_gpu(C):
    from ddp_practice_amd.optim import EMA

    m = _Bag(40).to(DEV)
    e = EMA(m, decay=0.5)
    for _ in range(3):
        m.train_step()
        e.update()
    live = {k: v.clone() for k, v in m.state_dict().items()}
    with e.applied():
        _exact(list(m.state_dict().values()), list(e.shadows.values()), "applied")
    _exact(list(m.state_dict().values()), list(live.values()), "restored")
    t = AveragedModel(_Bag(40).to(DEV))
    t.load_state_dict(e.state_dict())
    assert int(t.n_averaged) == 3
    e2 = EMA(_Bag(40, seed=1).to(DEV), decay=0.5)
    e2.load_state_dict(t.state_dict())
    _exact(list(e2.shadows.values()), list(e.shadows.values()), "through torch's AveragedModel and back")
    assert int(e2.n_averaged) == 3 and e2.n_averaged.is_cuda


# ---------------------------------------------------------------- 6. the fallback
def test_more_rows_than_the_table_holds_take_the_fallback(C, monkeypatch):
    """More than 512 rows: torch's ops, and torch's result."""
    from ddp_practice_amd.optim import EMA

    count = C.ema.LARGE_MAXT + 1
    m, mt = _Bag(count).to(DEV), _Bag(count).to(DEV)
    e = EMA(m, decay=0.3)
    t = AveragedModel(mt, multi_avg_fn=get_ema_multi_avg_fn(0.3))

    def no_native(*a, **k):
        raise AssertionError("the native launch with more rows than LARGE_MAXT")

    monkeypatch.setattr(C.ema, "ema_update", no_native)
    for _ in range(3):
        m.train_step()
        mt.train_step()
        e.update()
        t.update_parameters(mt)
    torch.cuda.synchronize()
    assert int(e.n_averaged) == 3
    _exact(list(e.shadows.values()), list(t.module.state_dict().values()), "fallback vs torch")


# ---------------------------------------------------------------- 7. ConvNet through TrainLoop
def _convnet_loop(base, ds, opt_name, amp, use_graph, ema_of, attach=True):
    from ddp_practice_amd import optim
    from ddp_practice_amd.amp import GradScaler
    from ddp_practice_amd.data import DeviceLoader
    from ddp_practice_amd.engine import TrainLoop
    from ddp_practice_amd.nn import CrossEntropyLoss

    model = copy.deepcopy(base)
    loader = DeviceLoader(ds, batch_size=32, shuffle=False, device=DEV, dtype=torch.bfloat16 if amp else torch.float32)
    kw = dict(lr=1e-3, weight_decay=0.01) if opt_name == "AdamW" else dict(lr=1e-2)
    opt = getattr(optim, opt_name)(model.parameters(), **kw)
    ema = ema_of(model)
    loop = TrainLoop(model, CrossEntropyLoss(), opt, loader, GradScaler() if amp else None, use_graph=use_graph,
                     steps_per_graph=4, ema=ema if attach else None)
    return model, ema, loop


@pytest.mark.parametrize("opt_name,amp", [("SGD", True), ("SGD", False), ("AdamW", True), ("AdamW", False)],
                         ids=["sgd-bf16", "sgd-fp32", "adamw-bf16", "adamw-fp32"])
def test_convnet_train_loop_graph_equals_eager_equals_torch(C, opt_name, amp):
    """Batch 32, 20 full steps (five replays of a 4-step graph) with ``ema=``: the shadows and
    n_averaged of the replayed loop == the eager loop's == those of a hand-written eager loop that
    calls torch's ``AveragedModel.update_parameters`` on the native model after every step, bitwise.
    The two warm-up steps of the capture leave no trace in the average."""
    from ddp_practice_amd.data import synthetic
    from ddp_practice_amd.models import ConvNet
    from ddp_practice_amd.optim import EMA

    gc.collect()  # an uncollected GradScaler of an earlier test
    ds = synthetic(32 * 20, seed=5)
    torch.manual_seed(0)
    base = ConvNet(amp_dtype=torch.bfloat16 if amp else None).to(DEV)
    out = []
    for use_graph in (False, True):
        model, ema, loop = _convnet_loop(base, ds, opt_name, amp, use_graph, lambda m: EMA(m, decay=0.9))
        loop.run_epoch()
        torch.cuda.synchronize()
        assert loop.graph_error is None, loop.graph_error
        assert loop.global_step == 20 and int(ema.n_averaged) == 20
        out.append((model.state_dict(), ema))
    (sd_e, ema_e), (sd_g, ema_g) = out
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k
    _exact(list(ema_g.shadows.values()), list(ema_e.shadows.values()), "shadows, graph vs eager")
    assert not torch.equal(ema_g.shadows["fc.weight"], sd_g["fc.weight"])
    assert int(ema_g.shadows["layer1.1.num_batches_tracked"]) == 20
    # the hand-written loop: the engine's eager step, then torch's update on the native model
    model, _, loop = _convnet_loop(base, ds, opt_name, amp, False, lambda m: None, attach=False)
    avg = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(0.9))
    model.train()
    loop.loader.start_epoch()
    for _ in range(20):
        loop._eager_step()
        avg.update_parameters(model)
    torch.cuda.synchronize()
    tsd = avg.module.state_dict()
    assert list(tsd) == list(ema_g.shadows) and int(avg.n_averaged) == 20
    _exact(list(ema_g.shadows.values()), list(tsd.values()), "shadows vs torch's AveragedModel")


def test_train_loop_refuses_a_host_side_averaged_model_under_graph(C):
    from ddp_practice_amd.data import synthetic
    from ddp_practice_amd.models import ConvNet

    ds = synthetic(64, seed=5)
    base = ConvNet(amp_dtype=None).to(DEV)
    with pytest.raises(ValueError, match="optim.EMA"):
        _convnet_loop(base, ds, "SGD", False, True, lambda m: AveragedModel(m))
    _convnet_loop(base, ds, "SGD", False, False, lambda m: AveragedModel(m))  # eager: accepted
