"""The device-resident learning rate (optim/lr.py DeviceLR, ``lr_dev=`` of the update kernels)
on the GPU: every update launch follows a per-step schedule bit for bit, eagerly and under
hipGraph replay, where a by-value rate is frozen at capture."""
import copy
import gc

import numpy as np
import pytest
import torch
from torch.optim import lr_scheduler as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
STEPS, EAGER = 8, 3  # steps 0-2 eager, steps 3-7 replays of one captured graph
KW = dict(lr=0.05, momentum=0.9, weight_decay=1e-4)
SMALL_SHAPES = [(400,), (16,), (32, 16, 5, 5), (10, 1568), (7,), (4099,)]


def _one_cycle(o):  # every step's rate differs; the momentum is left alone
    return S.OneCycleLR(o, max_lr=0.2, total_steps=STEPS, cycle_momentum=False)


def _large_sizes():  # tests/test_ops_gpu.py test_large_fused_amp_sgd_matches_unfused
    g = torch.Generator().manual_seed(3)
    sizes = [int(x) for x in torch.randint(1, 90000, (161,), generator=g)]
    sizes[0], sizes[7], sizes[100] = 1, 3, 2_000_001
    return sizes


def _exact(xs, ys, msg):
    """Bit for bit, every tensor of the two lists (one comparison of the concatenations)."""
    a = torch.cat([x.detach().reshape(-1) for x in xs])
    b = torch.cat([y.detach().reshape(-1) for y in ys])
    torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True, msg=lambda m: f"{msg}: {m}")


def _spy(monkeypatch, C, name):
    calls = []
    orig = getattr(C.optim, name)

    def f(*a, **k):
        calls.append(k.get("lr_dev"))
        return orig(*a, **k)

    monkeypatch.setattr(C.optim, name, f)
    return calls


def _run_launch_case(C, monkeypatch, shapes, amp, nesterov, launch, plain_fused=True):
    """optim.SGD + DeviceLR (steps 0-2 eager, 3-7 one replayed graph holding the update and
    scheduler.step()) against torch.optim.SGD(foreach=True) + the real torch scheduler; with
    ``amp`` also against the unfused unscale / sgd_step / update_scale launches given the torch
    scheduler's rate by value, and step 4 carries an inf: skipped, the schedule still advances."""
    from ddp_practice_amd.optim import SGD, DeviceLR, sgd as sgd_mod

    monkeypatch.setattr(sgd_mod, "_PLAIN_FUSED", plain_fused)
    calls = _spy(monkeypatch, C, launch)
    kw = dict(KW, nesterov=nesterov)
    torch.manual_seed(0)
    init = [torch.randn(s, device=DEV) for s in shapes]
    pa = [torch.nn.Parameter(p.clone()) for p in init]
    ga = [torch.empty_like(p) for p in init]
    for p, g in zip(pa, ga):
        p.grad = g
    opt = SGD(pa, **kw)
    dlr = DeviceLR.from_torch(opt, _one_cycle, STEPS)
    pt = [torch.nn.Parameter(p.clone()) for p in init]
    ref = torch.optim.SGD(pt, foreach=True, **kw)
    sched = _one_cycle(ref)
    table = dlr.table.cpu().numpy()[:, 0]
    assert len(set(table.tolist())) == STEPS and opt.param_groups[0]["lr"] not in table.tolist()
    if amp:
        sa, sb = torch.tensor([512.0], device=DEV), torch.tensor([512.0], device=DEV)
        ta, tb = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        fa, fb = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
        pb = [p.clone() for p in init]
        bb = [torch.zeros_like(p) for p in init]
        assert opt._fuse_kind() == {"amp_sgd_fused": "small", "amp_sgd_large": "large"}[launch]

    def one():
        if amp:
            opt.fused_amp_step(sa, ta, fa, 2.0, 0.5, 2)
        else:
            opt.step()
        dlr.step()

    graph = None
    for it in range(STEPS):
        gs = [torch.randn_like(p) * (512.0 if amp else 1.0) for p in init]
        if amp and it == 4:
            gs[it % len(gs)].view(-1)[it % gs[it % len(gs)].numel()] = float("inf")
        for x, g in zip(ga, gs):
            x.copy_(g)
        if it < EAGER:
            one()
        else:
            if graph is None:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    one()
            graph.replay()
        # the references: the rate of this step is the torch scheduler's
        lr_k = sched.get_last_lr()[0]
        assert np.float32(lr_k) == table[it]
        skipped = False
        if amp:
            inv = 1.0 / sb.item()  # a power of two: g * inv is exact, as the kernels' unscale
            skipped = not all(bool(torch.isfinite(g).all()) for g in gs)
            gb = [g.clone() for g in gs]
            C.optim.unscale_check(gb, sb, fb)
            C.optim.sgd_step(pb, gb, bb, lr_k, kw["momentum"], 0.0, kw["weight_decay"], nesterov, False, [], fb, None)
            C.optim.update_scale(sb, tb, fb, 2.0, 0.5, 2)
            gs = [g * inv for g in gs]
        if not skipped:
            for q, g in zip(pt, gs):
                q.grad = g
            ref.step()
        if it + 1 < STEPS:
            sched.step()  # unconditional, as scheduler.step() in the captured step
        torch.cuda.synchronize()
        ba = [opt.state[p]["momentum_buffer"] for p in pa]
        _exact(pa, pt, f"step {it} params vs torch foreach SGD")
        _exact(ba, [ref.state[q]["momentum_buffer"] for q in pt], f"step {it} momentum buffers vs torch foreach SGD")
        if amp:
            _exact(pa + ga + ba, pb + gb + bb, f"step {it} params / grads / buffers vs the unfused launches")
            assert sa.item() == sb.item() and ta.item() == tb.item() and fa.item() == fb.item() == 0.0, it
    if amp:
        assert sb.item() != 512.0 or tb.item() != 0  # the scale machine moved (backoff at step 4)
    assert dlr.state_dict() == {"pos": STEPS} and dlr.get_last_lr() == [float(table[-1])]
    # the launch under test ran (3 eager calls + 1 capture), every time with the device word
    assert len(calls) == EAGER + 1 and all(w is opt._lr_words[0] for w in calls), calls
    return opt


def test_multi_tensor_sgd_step_follows_device_lr(C, monkeypatch):
    _run_launch_case(C, monkeypatch, SMALL_SHAPES, amp=False, nesterov=False, launch="sgd_step", plain_fused=False)


def test_fused_plain_step_follows_device_lr(C, monkeypatch):
    opt = _run_launch_case(C, monkeypatch, [(7,), (3000,), (29034,)], amp=False, nesterov=True,
                           launch="amp_sgd_fused")
    assert int(opt._amp_sync[0]) == 0 and int(opt._amp_sync[3]) == 0  # plain mode: no barrier, no error


@pytest.mark.parametrize("sizes,barrier", [((7, 33, 100), False), ((7, 3000, 29034), True)])
def test_fused_amp_step_follows_device_lr(C, monkeypatch, sizes, barrier):
    opt = _run_launch_case(C, monkeypatch, [(n,) for n in sizes], amp=True, nesterov=False, launch="amp_sgd_fused")
    # one workgroup skips the grid barrier; else one generation per launch (capture runs nothing)
    assert int(opt._amp_sync[0]) == (STEPS if barrier else 0) and int(opt._amp_sync[3]) == 0


def test_large_fused_amp_step_follows_device_lr(C, monkeypatch):
    opt = _run_launch_case(C, monkeypatch, [(n,) for n in _large_sizes()], amp=True, nesterov=False,
                           launch="amp_sgd_large")
    assert int(opt._amp_sync_large[0]) == STEPS and int(opt._amp_sync_large[3]) == 0


@pytest.mark.parametrize("G", [1, 3])
def test_lr_advance_kernel(C, G):
    """4 rows advanced 6 times under one 6-node graph: exact words and position after every
    node, the last row holds, and a second replay moves nothing but the position."""
    rows = torch.tensor([[0.1 * (r + 1) + 0.01 * g for g in range(G)] for r in range(4)], dtype=torch.float64)
    table = rows.to(torch.float32).to(DEV)
    pos = torch.zeros(1, dtype=torch.int32, device=DEV)
    words = table[0].clone()
    log = torch.zeros(6, G, device=DEV)
    plog = torch.zeros(6, dtype=torch.int32, device=DEV)
    C.optim.lr_advance(table, pos, words)  # eager first (and lazy initialisation outside capture)
    torch.cuda.synchronize()
    assert pos.item() == 1 and torch.equal(words, table[1])
    pos.zero_()
    words.copy_(table[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for k in range(6):
            C.optim.lr_advance(table, pos, words)
            log[k].copy_(words)
            plog[k:k + 1].copy_(pos)
    graph.replay()
    torch.cuda.synchronize()
    want = torch.stack([table[min(k + 1, 3)] for k in range(6)])
    assert torch.equal(log, want) and plog.tolist() == [1, 2, 3, 4, 5, 6]
    assert pos.item() == 6 and torch.equal(words, table[3])
    graph.replay()
    torch.cuda.synchronize()
    assert pos.item() == 12 and torch.equal(words, table[3]) and torch.equal(log, want[-1:].expand(6, G))
    # saturating, never wrapping
    big = torch.iinfo(torch.int32).max
    pos.fill_(big - 1)
    C.optim.lr_advance(table, pos, words)
    C.optim.lr_advance(table, pos, words)
    torch.cuda.synchronize()
    assert pos.item() == big and torch.equal(words, table[3])
    # host checks
    with pytest.raises(RuntimeError):
        C.optim.lr_advance(table, pos.long(), words)
    with pytest.raises(RuntimeError):
        C.optim.lr_advance(table.view(-1)[:-1].contiguous() if G > 1 else table.double(), pos, words)
    with pytest.raises(RuntimeError):
        C.optim.lr_advance(table.cpu(), pos, words)


@pytest.mark.parametrize("amp", [True, False], ids=["bf16", "fp32"])
def test_convnet_train_loop_graph_equals_eager_under_schedule(C, amp):
    """ConvNet through TrainLoop (batch 8, 64 samples: two replays of a 4-step graph holding 4
    lr_advance nodes) == the same loop run eagerly, bitwise; the slab-column lanes and the
    pre-checked path read the word, and the capture's two warm-up steps do not shift the schedule."""
    from ddp_practice_amd.amp import GradScaler
    from ddp_practice_amd.data import DeviceLoader, synthetic
    from ddp_practice_amd.engine import TrainLoop
    from ddp_practice_amd.models import ConvNet
    from ddp_practice_amd.nn import CrossEntropyLoss
    from ddp_practice_amd.optim import SGD, DeviceLR

    # an earlier test's GradScaler that is garbage but not yet collected is still the one the
    # native loss pre-scales for (amp/grad_scaler.py _ACTIVE, a weak reference), and a capture
    # collects garbage first (runtime/graph.py gc_paused): without this the eager run and the
    # graph run of the fp32 case would go through different loss kernels
    gc.collect()
    ds = synthetic(64, seed=5)
    torch.manual_seed(0)
    base = ConvNet(amp_dtype=torch.bfloat16 if amp else None).to(DEV)
    out = []
    for use_graph in (False, True):
        model = copy.deepcopy(base)
        loader = DeviceLoader(ds, batch_size=8, shuffle=False, device=DEV,
                              dtype=torch.bfloat16 if amp else torch.float32)
        opt = SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
        dlr = DeviceLR.from_torch(opt, lambda o: S.OneCycleLR(o, max_lr=0.05, total_steps=12, cycle_momentum=False), 12)
        loop = TrainLoop(model, CrossEntropyLoss(), opt, loader, GradScaler() if amp else None, use_graph=use_graph,
                         steps_per_graph=4, scheduler=dlr)
        loop.run_epoch()
        torch.cuda.synchronize()
        assert loop.graph_error is None, loop.graph_error
        assert loop.global_step == 8 and dlr.state_dict() == {"pos": 8}
        assert dlr.get_last_lr() == [float(dlr.table[8, 0])]
        out.append((model.state_dict(), [opt.state[p]["momentum_buffer"] for p in model.parameters()]))
    (sd_e, b_e), (sd_g, b_g) = out
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), (k, (sd_e[k].float() - sd_g[k].float()).abs().max().item())
    for i, (x, y) in enumerate(zip(b_e, b_g)):
        assert torch.equal(x, y), ("momentum_buffer", i)
    assert not torch.equal(sd_e["fc.weight"], base.state_dict()["fc.weight"])


def test_control_host_lr_edit_is_ignored_by_graph_replay(C):
    """The trap this feature removes, in code: without a DeviceLR the captured step keeps the
    rate it was captured with, whatever the host writes into param_groups afterwards."""
    from ddp_practice_amd.optim import SGD

    gen = torch.Generator(device="cpu").manual_seed(0)
    init = [torch.randn(s, generator=gen).to(DEV) for s in SMALL_SHAPES]
    pa = [torch.nn.Parameter(p.clone()) for p in init]
    pt = [torch.nn.Parameter(p.clone()) for p in init]
    for p in pa:
        p.grad = torch.empty_like(p)
    opt, ref = SGD(pa, lr=0.1), torch.optim.SGD(pt, lr=0.1, foreach=True)
    graph = None
    for it in range(4):
        gs = [torch.randn(p.shape, generator=gen).to(DEV) for p in init]
        for p, q, g in zip(pa, pt, gs):
            p.grad.copy_(g)
            q.grad = g
        if it == 0:
            opt.step()
        else:
            if graph is None:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    opt.step()
            graph.replay()
            opt.param_groups[0]["lr"] *= 0.5  # what a host-side scheduler would do
        ref.step()  # the reference's rate is never changed
    torch.cuda.synchronize()
    assert opt.param_groups[0]["lr"] == 0.1 * 0.5 ** 3
    _exact(pa, pt, "replayed steps used the captured rate")


def test_train_loop_refuses_a_host_scheduler_under_graph_replay(C):
    from ddp_practice_amd.data import DeviceLoader, synthetic
    from ddp_practice_amd.engine import TrainLoop
    from ddp_practice_amd.models import ConvNet
    from ddp_practice_amd.nn import CrossEntropyLoss
    from ddp_practice_amd.optim import SGD

    model = ConvNet().to(DEV)
    opt = SGD(model.parameters(), lr=0.01)
    loader = DeviceLoader(synthetic(16, seed=1), batch_size=8, shuffle=False, device=DEV, dtype=torch.float32)
    sched = S.StepLR(opt, step_size=1)
    with pytest.raises(ValueError, match="DeviceLR"):
        TrainLoop(model, CrossEntropyLoss(), opt, loader, None, use_graph=True, scheduler=sched)
    TrainLoop(model, CrossEntropyLoss(), opt, loader, None, use_graph=False, scheduler=sched)  # eager: honoured
