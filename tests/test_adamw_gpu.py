"""optim.AdamW / optim.Adam on the GPU (csrc/kernels/adam.hip): one step per element against
the float64 reference within the counted bounds of tests/_adam_ref.py, a ten-step trajectory
against torch's capturable foreach AdamW, the device-side skip, hipGraph replay of the
device-resident step count (with the by-value trap as the control), DeviceLR, the three-launch
AMP step, and the ConvNet through TrainLoop."""
import copy
import gc
import os

import pytest
import torch
from torch.optim import lr_scheduler as S

from . import _adam_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
EDGE_SIZES = [1, 3, 4, 5, 4095, 4096, 4097]
SHAPES = [(400,), (16,), (32, 16, 5, 5), (7,), (4099,)]


def _sizes(count):
    if count == 1:
        return [4097]
    if count == 161:  # the ResNet-50 tensor count, sizes of its BN vectors and small kernels
        return [(64, 256, 2304)[i % 3] for i in range(161)]
    return [EDGE_SIZES[i % len(EDGE_SIZES)] for i in range(count)]  # 36: by value; 37: the table's first size


def _grad(n, gen):
    """Magnitudes in [2^-3, 2^3] with random sign, plus exact zeros and (from 4 elements) one 1e-20."""
    g = torch.exp2(torch.rand(n, generator=gen) * 6 - 3) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1)
    g[torch.rand(n, generator=gen) < 0.05] = 0.0
    if n >= 4:
        g[int(torch.randint(0, n, (1,), generator=gen))] = 1e-20
    return g


def _group(sizes, t0, seed, offset_first=True):
    """CPU float32 p, g, m, v per tensor; tensor 0 of a multi-tensor group is a view starting 4
    bytes into its storage (made on the device by _to_dev)."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for n in sizes:
        p = torch.randn(n, generator=gen)
        g = _grad(n, gen)
        if t0 == 0:
            m, v = torch.zeros(n), torch.zeros(n)
        else:
            m = torch.randn(n, generator=gen) * 0.1
            v = torch.rand(n, generator=gen)
            v[torch.rand(n, generator=gen) < 0.05] = 0.0
        out.append((p, g, m, v))
    return out


def _to_dev(data, cls, t0, **kw):
    """An optimizer over device copies of ``data`` with its state in place at step count t0."""
    params = []
    for i, (p, g, m, v) in enumerate(data):
        if i == 0 and len(data) > 1:
            store = torch.empty(p.numel() + 1, device=DEV)
            q = store[1:]
            q.copy_(p)
            assert q.data_ptr() % 16 == 4 and q.is_contiguous()
        else:
            q = p.to(DEV)
        q = torch.nn.Parameter(q)
        if i == 0 and len(data) > 1:
            assert q.data_ptr() % 16 == 4
        q.grad = g.to(DEV)
        params.append(q)
    opt = cls(params, **kw)
    word = torch.full((), float(t0), dtype=torch.float32, device=DEV)
    for q, (p, g, m, v) in zip(params, data):
        opt.state[q].update(step=word, exp_avg=m.to(DEV), exp_avg_sq=v.to(DEV))
    return params, opt


def _exact(xs, ys, msg):
    a = torch.cat([x.detach().reshape(-1) for x in xs])
    b = torch.cat([y.detach().reshape(-1) for y in ys])
    torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True, msg=lambda m: f"{msg}: {m}")


def _state(opt, params):
    return ([opt.state[p]["exp_avg"] for p in params], [opt.state[p]["exp_avg_sq"] for p in params])


# ---------------------------------------------------------------- 1. one step, per element
@pytest.mark.parametrize("t0", [0, 1, 999])
@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("name", ["AdamW", "Adam"])
def test_one_step_within_counted_bounds(C, name, wd, maximize, t0):
    from ddp_practice_amd import optim

    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    worst = {}
    for count in (1, 36, 37, 161):
        data = _group(_sizes(count), t0, seed=count)
        params, opt = _to_dev(data, getattr(optim, name), t0, maximize=maximize, **hyper)
        opt.step()
        torch.cuda.synchronize()
        assert float(opt.state[params[0]]["step"]) == t0 + 1
        assert int(opt._tickets[0]) == 0  # the last workgroup reset it
        for i, (q, (p, g, m, v)) in enumerate(zip(params, data)):
            o = R.step(p, g, m, v, t0 + 1, decoupled=name == "AdamW", maximize=maximize, **hyper)
            assert torch.equal(q.grad.cpu(), g), (count, i)  # the gradient is only read
            for key, got in (("p", q), ("m", opt.state[q]["exp_avg"]), ("v", opt.state[q]["exp_avg_sq"])):
                err = (got.detach().cpu().double() - o[key]).abs()
                ratio = float((err / o["b" + key]).max())
                worst[key] = max(worst.get(key, 0.0), ratio)
                assert ratio <= 1.0, (count, i, key, p.numel(), ratio, int((err / o["b" + key]).argmax()))
    print(f"{name} wd={wd} maximize={maximize} t0={t0}: worst error / bound {worst}")


# ---------------------------------------------------------------- 2. ten steps vs torch
def _trajectory_case(name="AdamW", n_steps=10, lrs=None, seed=0, **hyper):
    """(native params/state, torch params/state, float64 trajectory) after n_steps on the same
    gradients; torch is its capturable foreach path, the op order adam_rule follows."""
    from ddp_practice_amd import optim

    hyper = dict(dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01), **hyper)
    gen = torch.Generator().manual_seed(seed)
    init = [torch.randn(s, generator=gen) for s in SHAPES]
    grads = [[_grad(p.numel(), gen).reshape(p.shape) for p in init] for _ in range(n_steps)]
    pa = [torch.nn.Parameter(p.to(DEV)) for p in init]
    pt = [torch.nn.Parameter(p.to(DEV)) for p in init]
    opt = getattr(optim, name)(pa, **hyper)
    ref = getattr(torch.optim, name)(pt, foreach=True, capturable=True, **hyper)
    for k, gs in enumerate(grads):
        if lrs is not None:
            opt.param_groups[0]["lr"] = ref.param_groups[0]["lr"] = float(lrs[k])
        for p, q, g in zip(pa, pt, gs):
            p.grad, q.grad = g.to(DEV), g.to(DEV)
        opt.step()
        ref.step()
    torch.cuda.synchronize()
    f64 = [R.trajectory(p, [gs[i] for gs in grads], decoupled=name == "AdamW", lrs=lrs, **hyper)
           for i, p in enumerate(init)]
    return (pa, opt), (pt, ref), f64, n_steps


def _outputs(params, opt):
    m, v = _state(opt, params)
    return {"p": [p.detach() for p in params], "m": m, "v": v}


def _assert_as_close_as_torch(native, torch_side, f64, n_steps, what):
    """max |native - f64| <= 2 max |torch - f64| + n_steps * 2^-24 * max |x|, per output."""
    a, t = _outputs(*native), _outputs(*torch_side)
    for key in ("p", "m", "v"):
        ref = torch.cat([o[key].reshape(-1) for o in f64])
        ea = float((torch.cat([x.reshape(-1) for x in a[key]]).cpu().double() - ref).abs().max())
        et = float((torch.cat([x.reshape(-1) for x in t[key]]).cpu().double() - ref).abs().max())
        floor = n_steps * R.U32 * float(ref.abs().max())
        print(f"{what} {key}: native err {ea:.3e} torch err {et:.3e} floor {floor:.3e}")
        assert ea <= 2.0 * et + floor, (what, key, ea, et, floor)


def vs_torch_report():
    """(text, largest distance): the largest ulp distance per output to torch's capturable foreach
    path, after ONE step from the same state (which output differs names the op) and after ten."""
    from ddp_practice_amd import optim

    lines = ["optim.AdamW / optim.Adam vs torch.optim.*(foreach=True, capturable=True) on this GPU, "
             f"torch {torch.__version__}: largest distance in ulp per output",
             "one step from identical state (weight_decay 0.01):"]
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    worst = 0
    for name in ("AdamW", "Adam"):
        for t0 in (0, 1, 999):
            data = _group([4097, 400, 7], t0, seed=5)
            params, opt = _to_dev(data, getattr(optim, name), t0, **hyper)
            pt = [torch.nn.Parameter(p.to(DEV)) for p, _, _, _ in data]
            ref = getattr(torch.optim, name)(pt, foreach=True, capturable=True, **hyper)
            for q, (p, g, m, v) in zip(pt, data):
                q.grad = g.to(DEV)
                ref.state[q].update(step=torch.tensor(float(t0), device=DEV), exp_avg=m.to(DEV),
                                    exp_avg_sq=v.to(DEV))
            opt.step()
            ref.step()
            a, t = _outputs(params, opt), _outputs(pt, ref)
            d = {k: max(R.ulp_distance(x, y) for x, y in zip(a[k], t[k])) for k in ("p", "m", "v")}
            lines.append(f"  {name:5s} step {t0 + 1:4d}: p {d['p']}  exp_avg {d['m']}  exp_avg_sq {d['v']}")
            worst = max(worst, *d.values())
    lines.append("ten steps from zero state:")
    for name in ("AdamW", "Adam"):
        native, torch_side, _, _ = _trajectory_case(name)
        a, t = _outputs(*native), _outputs(*torch_side)
        d = {k: max(R.ulp_distance(x, y) for x, y in zip(a[k], t[k])) for k in ("p", "m", "v")}
        lines.append(f"  {name:5s}: p {d['p']}  exp_avg {d['m']}  exp_avg_sq {d['v']}")
        worst = max(worst, *d.values())
    return "\n".join(lines) + "\n", worst


@pytest.mark.parametrize("name", ["AdamW", "Adam"])
def test_ten_steps_as_close_to_float64_as_torch(C, name):
    native, torch_side, f64, n = _trajectory_case(name)
    _assert_as_close_as_torch(native, torch_side, f64, n, name)
    assert float(native[1].state[native[0][0]]["step"]) == 10.0


def test_bitwise_equal_to_torch_capturable_foreach(C):
    """Every output, one step from steps 0 / 1 / 999 and ten steps from zero: 0 ulp from torch's
    capturable foreach path (profiles/adamw_vs_torch.txt is this text from the recorded run;
    DPA_ADAMW_REPORT=path writes it).  Holds for this torch build's foreach kernels: a new
    torch that reorders an op shows up here first, and the float64 tests above still decide."""
    text, worst = vs_torch_report()
    print(text)
    path = os.environ.get("DPA_ADAMW_REPORT")
    if path:
        with open(path, "w") as f:
            f.write(text)
    assert worst == 0, text


# ---------------------------------------------------------------- 3. skip
@pytest.mark.parametrize("count", [3, 37])
def test_found_inf_skips_the_whole_launch(C, count):
    from ddp_practice_amd.optim import AdamW

    data = _group(_sizes(count) if count > 3 else [4097, 5, 64], 7, seed=2)
    params, opt = _to_dev(data, AdamW, 7, lr=1e-3, weight_decay=0.01)
    before = [x.clone() for x in (*[p.detach() for p in params], *sum(_state(opt, params), []))]
    found = torch.ones(1, device=DEV)
    opt.step(found_inf=found)
    torch.cuda.synchronize()
    after = [*[p.detach() for p in params], *sum(_state(opt, params), [])]
    _exact(after, before, "skipped step")
    assert float(opt.state[params[0]]["step"]) == 7.0 and int(opt._tickets[0]) == 0
    found.zero_()
    opt.step(found_inf=found)
    torch.cuda.synchronize()
    assert float(opt.state[params[0]]["step"]) == 8.0 and int(opt._tickets[0]) == 0
    assert not torch.equal(params[1].detach(), before[1])


# ---------------------------------------------------------------- 4. replay
def _replay_setup(count, seed=3):
    from ddp_practice_amd.optim import AdamW

    sizes = _sizes(count) if count > 5 else [s[0] if len(s) == 1 else 12800 for s in SHAPES]
    gen = torch.Generator().manual_seed(seed)
    init = [torch.randn(n, generator=gen) for n in sizes]
    grads = [[_grad(n, gen) for n in sizes] for _ in range(8)]
    out = []
    for _ in range(2):
        ps = [torch.nn.Parameter(p.to(DEV)) for p in init]
        for p in ps:
            p.grad = torch.zeros_like(p)
        out.append((ps, AdamW(ps, lr=1e-3, weight_decay=0.01)))
    return init, grads, out


def _reset(ps, opt, init):
    """Undo the eager warm-up step (the state tensors stay: a graph references them)."""
    for p, x in zip(ps, init):
        p.data.copy_(x)
        opt.state[p]["exp_avg"].zero_()
        opt.state[p]["exp_avg_sq"].zero_()
    opt.state[ps[0]]["step"].zero_()


@pytest.mark.parametrize("count", [5, 161])
def test_graph_replay_advances_the_step_count(C, count):
    """One captured step replayed 8 times == 8 eager steps, bitwise, and the word counts 8.
    Control: the same graph with the count held at its captured value (what a by-value count
    is under replay) ends somewhere else."""
    init, grads, ((pa, oa), (pb, ob)) = _replay_setup(count)
    for g in grads:  # eager
        for p, x in zip(pa, g):
            p.grad.copy_(x)
        oa.step()
    results = []
    for frozen in (False, True):
        ob.step()  # state and (count > 36) the table exist before capture
        _reset(pb, ob, init)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ob.step()
        word = ob.state[pb[0]]["step"]
        for g in grads:
            for p, x in zip(pb, g):
                p.grad.copy_(x)
            if frozen:
                word.zero_()
            graph.replay()
        torch.cuda.synchronize()
        results.append(([p.detach().clone() for p in pb], [x.clone() for x in sum(_state(ob, pb), [])], float(word)))
        del graph
    (p_live, s_live, w_live), (p_frozen, _, w_frozen) = results
    assert float(oa.state[pa[0]]["step"]) == 8.0 and w_live == 8.0 and w_frozen == 1.0
    _exact(p_live, pa, "replayed params vs eager")
    _exact(s_live, sum(_state(oa, pa), []), "replayed moments vs eager")
    assert not torch.equal(torch.cat(p_frozen), torch.cat([p.detach() for p in pa]))


def test_state_must_exist_before_capture(C):
    from ddp_practice_amd.optim import AdamW

    p = torch.nn.Parameter(torch.ones(8, device=DEV))
    p.grad = torch.ones(8, device=DEV)
    opt = AdamW([p])
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="run one eager step first"):
        with torch.cuda.graph(graph):
            opt.step()
    torch.cuda.synchronize()
    opt.step()  # and the optimizer is usable afterwards
    torch.cuda.synchronize()
    assert float(opt.state[p]["step"]) == 1.0


# ---------------------------------------------------------------- 5. DeviceLR
def test_device_lr_eager_equals_replay_and_follows_torch_scheduler(C):
    from ddp_practice_amd.optim import AdamW, DeviceLR

    n = 6
    make = lambda o: S.OneCycleLR(o, max_lr=5e-3, total_steps=n, cycle_momentum=False)  # noqa: E731
    gen = torch.Generator().manual_seed(4)
    init = [torch.randn(s, generator=gen) for s in SHAPES]
    grads = [[_grad(p.numel(), gen).reshape(p.shape) for p in init] for _ in range(n)]
    hyper = dict(lr=1e-3, weight_decay=0.01)
    runs = []
    for replay in (False, True):
        ps = [torch.nn.Parameter(p.to(DEV)) for p in init]
        for p in ps:
            p.grad = torch.zeros_like(p)
        opt = AdamW(ps, **hyper)
        dlr = DeviceLR.from_torch(opt, make, n)
        graph = None
        if replay:
            opt.step()
            _reset(ps, opt, init)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                opt.step()
                dlr.step()
        for gs in grads:
            for p, g in zip(ps, gs):
                p.grad.copy_(g)
            if graph is not None:
                graph.replay()
            else:
                opt.step()
                dlr.step()
        torch.cuda.synchronize()
        assert float(opt.state[ps[0]]["step"]) == n and dlr.state_dict() == {"pos": n}
        runs.append((ps, opt, dlr))
    (pe, oe, dlr), (pr, orr, _) = runs
    _exact(pr, pe, "replayed vs eager params under DeviceLR")
    _exact(sum(_state(orr, pr), []), sum(_state(oe, pe), []), "replayed vs eager moments under DeviceLR")
    # torch AdamW (capturable foreach) under the real scheduler, and the float64 trajectory on its rates
    pt = [torch.nn.Parameter(p.to(DEV)) for p in init]
    ref = torch.optim.AdamW(pt, foreach=True, capturable=True, **hyper)
    sched = make(ref)
    lrs = []
    for k, gs in enumerate(grads):
        lrs.append(sched.get_last_lr()[0])
        for q, g in zip(pt, gs):
            q.grad = g.to(DEV)
        ref.step()
        if k + 1 < n:
            sched.step()
    assert [float(x) for x in dlr.table[:, 0].cpu()] == [float(torch.tensor(x, dtype=torch.float32)) for x in lrs]
    f64 = [R.trajectory(p, [gs[i] for gs in grads], decoupled=True, lrs=lrs, betas=(0.9, 0.999), eps=1e-8, **hyper)
           for i, p in enumerate(init)]
    _assert_as_close_as_torch((pe, oe), (pt, ref), f64, n, "DeviceLR")


# ---------------------------------------------------------------- 6. AMP
@pytest.mark.parametrize("count", [5, 37])
def test_fused_amp_step_equals_unscale_then_step(C, count, monkeypatch):
    from ddp_practice_amd.amp import GradScaler
    from ddp_practice_amd.optim import AdamW

    scale = 65536.0
    sizes = _sizes(count) if count > 5 else [400, 16, 12800, 7, 4099]
    gen = torch.Generator().manual_seed(6)
    init = [torch.randn(n, generator=gen) for n in sizes]
    sides = []
    for fuse in (True, False):
        ps = [torch.nn.Parameter(p.to(DEV)) for p in init]
        opt = AdamW(ps, lr=1e-3, weight_decay=0.01)
        sides.append((ps, opt, GradScaler(init_scale=scale, growth_interval=3, fuse_step=fuse)))
    (pa, oa, sa), (pb, ob, sb) = sides
    fused_calls = []
    orig = oa.fused_amp_step
    monkeypatch.setattr(oa, "fused_amp_step", lambda *a, **k: (fused_calls.append(1), orig(*a, **k))[1])
    for s in (sa, sb):
        s._lazy_init(torch.device(DEV, torch.cuda.current_device()))
    for it in range(5):
        gs = [_grad(n, gen) * float(sa.get_scale()) for n in sizes]  # the scale is a power of two: exact
        if it == 2:
            gs[2][3] = float("inf")  # the last element of the 37-tensor case's third tensor
        for p, q, g in zip(pa, pb, gs):
            p.grad, q.grad = g.to(DEV), g.to(DEV)
        kept = [p.grad.clone() for p in pa]
        before = ([p.detach().clone() for p in pa], float(oa.state[pa[0]]["step"]) if it else 0.0, sa.get_scale())
        sa.step(oa)
        if it >= 1:  # the fused route (GradScaler takes it from its second iteration): g is only read
            _exact([p.grad for p in pa], kept, f"iteration {it}: gradients after fused_amp_step")
        sa.update()
        sb.unscale_(ob)  # the explicit route
        sb.step(ob)
        sb.update()
        torch.cuda.synchronize()
        _exact(pa, pb, f"iteration {it}: params")
        _exact(sum(_state(oa, pa), []), sum(_state(ob, pb), []), f"iteration {it}: moments")
        assert float(oa.state[pa[0]]["step"]) == float(ob.state[pb[0]]["step"])
        assert sa.get_scale() == sb.get_scale() and float(sa._found_inf) == float(sb._found_inf) == 0.0
        if it == 2:  # the injected inf: skipped, scale halved, count unchanged
            _exact(pa, before[0], "skipped iteration")
            assert float(oa.state[pa[0]]["step"]) == before[1] == 2.0 and sa.get_scale() == before[2] * 0.5
    assert len(fused_calls) == 4 and float(oa.state[pa[0]]["step"]) == 4.0
    assert int(oa._tickets[0]) == 0 and int(ob._tickets[0]) == 0


# ---------------------------------------------------------------- 7. ConvNet through TrainLoop
@pytest.mark.parametrize("amp,sched", [(True, False), (False, False), (True, True)], ids=["bf16", "fp32", "bf16-cosine"])
def test_convnet_train_loop_graph_equals_eager(C, amp, sched):
    """Batch 32, 12 full steps (three replays of a 4-step graph) == the same loop run eagerly,
    bitwise: parameters, BN buffers, both moments; the count is 12 whatever the capture's
    warm-up steps did."""
    from ddp_practice_amd.amp import GradScaler
    from ddp_practice_amd.data import DeviceLoader, synthetic
    from ddp_practice_amd.engine import TrainLoop
    from ddp_practice_amd.models import ConvNet
    from ddp_practice_amd.nn import CrossEntropyLoss
    from ddp_practice_amd.optim import AdamW, DeviceLR

    gc.collect()  # an uncollected GradScaler of an earlier test (tests/test_lr_schedule_gpu.py)
    ds = synthetic(32 * 12, seed=5)
    torch.manual_seed(0)
    base = ConvNet(amp_dtype=torch.bfloat16 if amp else None).to(DEV)
    out = []
    for use_graph in (False, True):
        model = copy.deepcopy(base)
        loader = DeviceLoader(ds, batch_size=32, shuffle=False, device=DEV,
                              dtype=torch.bfloat16 if amp else torch.float32)
        opt = AdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
        dlr = None
        if sched:
            dlr = DeviceLR.from_torch(opt, lambda o: S.CosineAnnealingLR(o, T_max=12), 13)
        loop = TrainLoop(model, CrossEntropyLoss(), opt, loader, GradScaler() if amp else None, use_graph=use_graph,
                         steps_per_graph=4, scheduler=dlr)
        loop.run_epoch()
        torch.cuda.synchronize()
        assert loop.graph_error is None, loop.graph_error
        ps = list(model.parameters())
        assert loop.global_step == 12 and float(opt.state[ps[0]]["step"]) == 12.0
        assert all(opt.state[p]["step"] is opt.state[ps[0]]["step"] for p in ps)
        if dlr is not None:
            assert dlr.state_dict() == {"pos": 12}
        out.append((model.state_dict(), sum(_state(opt, ps), [])))
    (sd_e, s_e), (sd_g, s_g) = out
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), (k, (sd_e[k].float() - sd_g[k].float()).abs().max().item())
    _exact(s_g, s_e, "moments, graph vs eager")
    assert not torch.equal(sd_e["fc.weight"], base.state_dict()["fc.weight"])
