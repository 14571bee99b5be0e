"""Global-norm gradient clipping on the GPU (csrc/kernels/clip.hip, optim/clip.py,
optim/adamw.py set_grad_clip): the norm against float64 within the bound tests/_clip_ref.py
counts, its independence of the grid, the coefficient's and the scale's bits against torch,
non-finite gradients, and the fused routes -- AdamW, AdamW under GradScaler, graph replay, the
ConvNet through TrainLoop -- bitwise against the explicit unscale_ -> clip_grad_norm_ -> step."""
import copy
import gc
import math

import pytest
import torch

from . import _clip_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
EDGE_SIZES = [1, 3, 4, 5, 4095, 4096, 4097]


def _sizes(count):
    """tests/test_adamw_gpu.py's tensor sets: 36 go by value, 37 is the table's first size, 161 is
    ResNet-50's tensor count with the sizes of its BN vectors and small kernels."""
    if count == 1:
        return [4097]
    if count == 161:
        return [(64, 256, 2304)[i % 3] for i in range(161)]
    return [EDGE_SIZES[i % len(EDGE_SIZES)] for i in range(count)]


def _draw(n, gen):
    """|g| log-uniform in [1e-6, 1e3] with a random sign: every square is a normal fp32."""
    mag = torch.exp(torch.rand(n, generator=gen, dtype=torch.float64) * math.log(1e9) + math.log(1e-6))
    g = (mag * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1)).float()
    return g.clamp(-1e3, 1e3)


def _grad(n, gen):
    """test_adamw_gpu.py's optimizer gradients: magnitudes in [2^-3, 2^3], random sign, some exact zeros."""
    g = torch.exp2(torch.rand(n, generator=gen) * 6 - 3) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1)
    g[torch.rand(n, generator=gen) < 0.05] = 0.0
    return g


def _on_dev(cpu_grads, offset_first=False):
    out = []
    for i, g in enumerate(cpu_grads):
        if i == 0 and offset_first:
            store = torch.empty(g.numel() + 1, device=DEV)
            t = store[1:]
            t.copy_(g)
            assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        else:
            t = g.to(DEV)
        out.append(t)
    return out


def _norm(grads, max_norm=1.0, **kw):
    from ddp_practice_amd.optim import clip as K

    out = torch.empty(2, device=DEV)
    K.grad_norm_into(grads, max_norm, out, **kw)
    return out


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _exact(xs, ys, msg):
    a = torch.cat([x.detach().reshape(-1) for x in xs])
    b = torch.cat([y.detach().reshape(-1) for y in ys])
    torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True, msg=lambda m: f"{msg}: {m}")


def _cases(C):
    """name -> (sizes, first tensor 4 bytes into its storage)."""
    E = 4 * C.clip.THR * C.clip.U  # elements per chunk
    cases = {f"one tensor of {n}": ([n], False) for n in (1, 3, 4, 5, E - 1, E, E + 1, 2 * E + 1)}
    cases["a tensor straddling a chunk edge"] = ([E - 6, 13], False)
    cases["a padded tail granule, then a tensor"] = ([7, 400], False)
    cases["a gradient 4 bytes into its storage"] = ([E + 3, 5], True)
    for c in (1, 36, 37, 161):
        cases[f"{c} tensors"] = (_sizes(c), False)
    cases["257 chunks"] = ([256 * E + 5], False)
    return cases


_made = {}


def _case(C, name):
    """The case's CPU gradients, device gradients and float64 norm, made once."""
    if name not in _made:
        sizes, off = _cases(C)[name]
        gen = torch.Generator().manual_seed(len(_made) + 1)
        cpu = [_draw(n, gen) for n in sizes]
        _made[name] = (cpu, _on_dev(cpu, off), R.reference(cpu, 1.0)["norm"])
    return _made[name]


def float64_report(C):
    """(text, [(case, relative error, bound)]): the norm of every case against float64."""
    U = C.clip.U
    bound = R.norm_rel_bound(U)
    rows = []
    for name in _cases(C):
        _, dev, ref = _case(C, name)
        got = float(_norm(dev)[0])
        rows.append((name, abs(got - ref) / ref, bound))
    worst = max(r[1] / r[2] for r in rows)
    lines = [f"clip.grad_norm against float64 on this GPU (U = {U} granules per lane, {R.sumsq_roundings(U)} counted "
             f"roundings on the sum of squares): relative error of the norm, the counted bound {bound:.3e}"]
    lines += [f"  {name:40s} {err:.3e}  ({err / b:.3f} of the bound)" for name, err, b in rows]
    lines.append(f"worst: {worst:.3f} of the bound")
    return "\n".join(lines) + "\n", rows


# ---------------------------------------------------------------- 1. the norm
def test_norm_within_the_counted_bound_of_float64(C):
    text, rows = float64_report(C)
    print(text)
    bad = [(n, e, b) for n, e, b in rows if not e <= b]
    assert not bad, bad


def test_same_bits_twice_and_under_every_grid(C):
    try:
        for name in ("257 chunks", "161 tensors"):
            _, dev, _ = _case(C, name)
            C.clip.set_grid_cap(0)
            first = _bits(_norm(dev, 3.0))
            assert torch.equal(_bits(_norm(dev, 3.0)), first), name
            for cap in (1, 3, 0):
                C.clip.set_grid_cap(cap)
                assert torch.equal(_bits(_norm(dev, 3.0)), first), (name, cap)
    finally:
        C.clip.set_grid_cap(0)
    from ddp_practice_amd.optim import clip as K

    assert int(K.workspace(torch.device(DEV, torch.cuda.current_device()), 1)[1]) == 0  # the ticket re-armed itself


def test_coefficient_bits_are_torchs(C):
    _, dev, ref = _case(C, "37 tensors")
    seen = []
    for max_norm in (0.5 * ref, 10.0 * ref, 1.0, 3.7):
        out = _norm(dev, max_norm)
        want = torch.clamp(max_norm / (out[0] + 1e-6), max=1.0)
        assert want.dtype == torch.float32
        assert torch.equal(_bits(out[1]), _bits(want)), (max_norm, float(out[1]), float(want))
        seen.append(float(out[1]))
    assert seen[0] < 1.0 and seen[1] == 1.0


def test_scale_is_the_product_and_one_leaves_the_gradients(C):
    for name in ("37 tensors", "a gradient 4 bytes into its storage", "a padded tail granule, then a tensor"):
        cpu, _, _ = _case(C, name)
        off = _cases(C)[name][1]
        from ddp_practice_amd.optim import clip as K

        for c in (0.37, 1.0):
            grads = _on_dev(cpu, off)
            before = [g.clone() for g in grads]
            coef = torch.tensor([c], device=DEV)
            lst, kw = K.launch_args(grads)
            C.clip.scale_(lst, coef, **kw)
            want = [g * coef[0] for g in before] if c != 1.0 else before
            for g, w in zip(grads, want):
                assert torch.equal(_bits(g), _bits(w)), (name, c)
            assert (c == 1.0) == all(torch.equal(g, b) for g, b in zip(grads, before))


@pytest.mark.parametrize("value", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_non_finite_gradients(C, value):
    from ddp_practice_amd.optim import clip_grad_norm_

    gen = torch.Generator().manual_seed(9)
    cpu = [_grad(n, gen) for n in (400, 7, 4099)]
    cpu[2][4098] = value
    ours = [torch.nn.Parameter(torch.zeros(g.numel(), device=DEV)) for g in cpu]
    theirs = [torch.nn.Parameter(torch.zeros(g.numel(), device=DEV)) for g in cpu]
    for p, q, g in zip(ours, theirs, cpu):
        p.grad, q.grad = g.to(DEV), g.to(DEV)
    # found_inf: set by the norm launch, which only reads
    fi = torch.zeros(1, device=DEV)
    before = [_bits(p.grad) for p in ours]
    _norm([p.grad for p in ours], 1.0, found_inf=fi)
    assert float(fi) == 1.0 and all(torch.equal(_bits(p.grad), b) for p, b in zip(ours, before))
    fi.zero_()
    _norm([p.grad for p in ours[:2]], 1.0, found_inf=fi)
    assert float(fi) == 0.0  # finite gradients leave the word alone
    n_ours = clip_grad_norm_(ours, 1.0)
    n_theirs = torch.nn.utils.clip_grad_norm_(theirs, 1.0, foreach=True)
    _exact([n_ours], [n_theirs], "norm")
    _exact([p.grad for p in ours], [q.grad for q in theirs], "clipped gradients")
    with pytest.raises(RuntimeError, match="non-finite"):
        clip_grad_norm_(ours, 1.0, error_if_nonfinite=True)


def test_clip_grad_norm_against_torch_foreach(C):
    from ddp_practice_amd.optim import clip_grad_norm_

    U = C.clip.U
    cpu, _, ref_norm = _case(C, "37 tensors")
    for factor in (0.5, 10.0):
        max_norm = factor * ref_norm
        ref = R.reference(cpu, max_norm)
        ours = [torch.nn.Parameter(torch.zeros(g.numel(), device=DEV)) for g in cpu]
        theirs = [torch.nn.Parameter(torch.zeros(g.numel(), device=DEV)) for g in cpu]
        for p, q, g in zip(ours, theirs, _on_dev(cpu, True)):
            p.grad, q.grad = g, g.clone()
        n_ours = clip_grad_norm_(ours, max_norm)
        n_theirs = torch.nn.utils.clip_grad_norm_(theirs, max_norm, foreach=True)
        assert n_ours.dim() == 0 and n_ours.dtype == torch.float32 and n_ours.is_cuda
        e_ours, e_theirs = abs(float(n_ours) - ref["norm"]) / ref["norm"], abs(float(n_theirs) - ref["norm"]) / ref["norm"]
        print(f"max_norm {factor} x norm: relative error ours {e_ours:.3e} torch {e_theirs:.3e} "
              f"bound {R.norm_rel_bound(U):.3e}")
        assert e_ours <= R.norm_rel_bound(U) and e_theirs <= R.norm_rel_bound(U)
        for p, c, g in zip(ours, ref["clipped"], cpu):
            err = (p.grad.cpu().double() - c).abs()
            assert bool((err <= c.abs() * R.clipped_rel_bound(U)).all()), float((err / c.abs()).max())
            assert (factor == 0.5) != torch.equal(p.grad.cpu(), g)  # it clipped exactly when it should


# ---------------------------------------------------------------- 2. fused into AdamW
def _two_groups(init, wd=(0.01, 0.1), clip=None):
    from ddp_practice_amd.optim import AdamW

    ps = [torch.nn.Parameter(p.to(DEV)) for p in init]
    opt = AdamW([{"params": ps[:5], "weight_decay": wd[0]}, {"params": ps[5:], "weight_decay": wd[1]}], lr=1e-3)
    opt.set_grad_clip(clip)
    return ps, opt


def _moments(opt, ps):
    return [opt.state[p][k] for p in ps for k in ("exp_avg", "exp_avg_sq")]


def test_adamw_set_grad_clip_equals_clip_then_step(C):
    from ddp_practice_amd.optim import clip_grad_norm_

    sizes = [400, 16, 12800, 7, 4099] + _sizes(37)
    gen = torch.Generator().manual_seed(11)
    init = [torch.randn(n, generator=gen) for n in sizes]
    steps = [[_grad(n, gen) for n in sizes] for _ in range(3)]
    probe = [torch.nn.Parameter(torch.zeros(n, device=DEV)) for n in sizes]
    for p, g in zip(probe, steps[0]):
        p.grad = g.to(DEV)
    norm0 = float(torch.nn.utils.clip_grad_norm_(probe, 1e30, foreach=True))  # the first step's norm, by torch
    assert norm0 > 0.0
    for factor in (0.5, 10.0):
        v = factor * norm0
        (pa, oa), (pb, ob), (pc, oc) = _two_groups(init, clip=v), _two_groups(init), _two_groups(init)
        for k, gs in enumerate(steps):
            for p, q, r, g in zip(pa, pb, pc, gs):
                p.grad, q.grad, r.grad = g.to(DEV), g.to(DEV), g.to(DEV)
            kept = [_bits(p.grad) for p in pa]
            oa.step()
            nb = clip_grad_norm_(pb, v)
            ob.step()
            oc.step()
            assert all(torch.equal(_bits(p.grad), b) for p, b in zip(pa, kept))  # the fused side only reads
            _exact([oa.grad_norm], [nb], f"step {k}: norm")
            _exact(pa, pb, f"step {k}: params, fused vs clip then step")
            _exact(_moments(oa, pa), _moments(ob, pb), f"step {k}: moments")
            if factor == 10.0:  # a clip that never bites is no clip at all
                _exact(pa, pc, f"step {k}: params, loose clip vs none")
                _exact(_moments(oa, pa), _moments(oc, pc), f"step {k}: moments, loose clip vs none")
        if factor == 0.5:
            assert not torch.equal(torch.cat([p.detach() for p in pa]), torch.cat([p.detach() for p in pc]))
        assert all(float(o.state[ps[0]]["step"]) == float(o.state[ps[-1]]["step"]) == 3.0
                   for ps, o in ((pa, oa), (pb, ob), (pc, oc)))


@pytest.mark.parametrize("count", [5, 37])
def test_fused_amp_step_with_clip_equals_unscale_clip_step(C, count, monkeypatch):
    from ddp_practice_amd.amp import GradScaler
    from ddp_practice_amd.optim import AdamW, clip_grad_norm_

    scale = 65536.0
    sizes = _sizes(count) if count > 5 else [400, 16, 12800, 7, 4099]
    gen = torch.Generator().manual_seed(6)
    init = [torch.randn(n, generator=gen) for n in sizes]
    all_gs = [[_grad(n, gen) for n in sizes] for _ in range(5)]
    v = 0.5 * float(torch.cat(all_gs[0]).double().norm())
    sides = []
    for fuse in (True, False):
        ps = [torch.nn.Parameter(p.to(DEV)) for p in init]
        opt = AdamW(ps, lr=1e-3, weight_decay=0.01)
        sides.append((ps, opt, GradScaler(init_scale=scale, growth_interval=3, fuse_step=fuse)))
    (pa, oa, sa), (pb, ob, sb) = sides
    oa.set_grad_clip(v)
    fused_calls = []
    orig = oa.fused_amp_step
    monkeypatch.setattr(oa, "fused_amp_step", lambda *a, **k: (fused_calls.append(1), orig(*a, **k))[1])

    def no_check(*a, **k):
        raise AssertionError("nonfinite_check ran: the norm launch makes the check")

    monkeypatch.setattr(C.adam, "nonfinite_check", no_check)
    for s in (sa, sb):
        s._lazy_init(torch.device(DEV, torch.cuda.current_device()))
    for it in range(5):
        gs = [g * float(sa.get_scale()) for g in all_gs[it]]  # the scale is a power of two: exact
        if it == 2:
            gs[2][3] = float("inf")
        for p, q, g in zip(pa, pb, gs):
            p.grad, q.grad = g.to(DEV), g.to(DEV)
        kept = [p.grad.clone() for p in pa]
        before = ([p.detach().clone() for p in pa], float(oa.state[pa[0]]["step"]) if it else 0.0, sa.get_scale())
        sa.step(oa)
        if it >= 1:  # the fused route (GradScaler takes it from its second iteration): g is only read
            _exact([p.grad for p in pa], kept, f"iteration {it}: gradients after fused_amp_step")
        sa.update()
        sb.unscale_(ob)  # the explicit route
        nb = clip_grad_norm_(pb, v)
        sb.step(ob)
        sb.update()
        torch.cuda.synchronize()
        _exact(pa, pb, f"iteration {it}: params")
        _exact(_moments(oa, pa), _moments(ob, pb), f"iteration {it}: moments")
        _exact([oa.grad_norm], [nb], f"iteration {it}: grad_norm")
        assert float(oa.state[pa[0]]["step"]) == float(ob.state[pb[0]]["step"])
        assert sa.get_scale() == sb.get_scale() and float(sa._found_inf) == float(sb._found_inf) == 0.0
        if it == 2:  # the injected inf: skipped, scale halved, count unchanged
            _exact(pa, before[0], "skipped iteration")
            assert float(oa.state[pa[0]]["step"]) == before[1] == 2.0 and sa.get_scale() == before[2] * 0.5
            assert not math.isfinite(float(oa.grad_norm))
        else:
            assert float(oa.grad_norm) > v  # the clip bit
    assert len(fused_calls) == 4 and float(oa.state[pa[0]]["step"]) == 4.0
    assert int(oa._tickets[0]) == 0 and int(ob._tickets[0]) == 0


# ---------------------------------------------------------------- 3. graph replay
@pytest.mark.parametrize("count", [5, 37])
def test_graph_replay_of_a_clipped_step(C, count):
    from ddp_practice_amd.optim import AdamW

    sizes = _sizes(count) if count > 5 else [400, 16, 12800, 7, 4099]
    gen = torch.Generator().manual_seed(3)
    init = [torch.randn(n, generator=gen) for n in sizes]
    grads = [[_grad(n, gen) * (0.25 + 0.25 * k) for n in sizes] for k in range(8)]  # the norm moves from step to step
    v = 0.5 * float(torch.cat(grads[0]).double().norm())
    sides = []
    for _ in range(2):
        ps = [torch.nn.Parameter(p.to(DEV)) for p in init]
        for p in ps:
            p.grad = torch.zeros_like(p)
        opt = AdamW(ps, lr=1e-3, weight_decay=0.01)
        opt.set_grad_clip(v)
        sides.append((ps, opt))
    (pa, oa), (pb, ob) = sides
    norms = []
    for g in grads:  # eager
        for p, x in zip(pa, g):
            p.grad.copy_(x)
        oa.step()
        norms.append(oa.grad_norm.clone())
    ob.step()  # state, the clip words and (count > 36) both tables exist before capture
    for p, x in zip(pb, init):
        p.data.copy_(x)
        ob.state[p]["exp_avg"].zero_()
        ob.state[p]["exp_avg_sq"].zero_()
    ob.state[pb[0]]["step"].zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ob.step()
    for k, g in enumerate(grads):
        for p, x in zip(pb, g):
            p.grad.copy_(x)
        graph.replay()
        _exact([ob.grad_norm], [norms[k]], f"replay {k}: norm")
    torch.cuda.synchronize()
    assert float(ob.state[pb[0]]["step"]) == 8.0
    assert float(norms[0]) > v and float(norms[0]) != float(norms[7])
    _exact(pb, pa, "replayed params vs eager")
    _exact(_moments(ob, pb), _moments(oa, pa), "replayed moments vs eager")
    del graph


def test_first_call_inside_a_capture_raises(C, monkeypatch):
    from ddp_practice_amd.optim import clip as K
    from ddp_practice_amd.optim import clip_grad_norm_

    monkeypatch.setattr(K, "_workspaces", {})  # a process that has not clipped yet
    p = torch.nn.Parameter(torch.ones(8, device=DEV))
    p.grad = torch.full((8,), 2.0, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="run one eager step first"):
        with torch.cuda.graph(graph):
            clip_grad_norm_([p], 1.0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="graph"):
        with torch.cuda.graph(graph):
            clip_grad_norm_([p], 1.0, error_if_nonfinite=True)
    torch.cuda.synchronize()
    n = clip_grad_norm_([p], 1.0)  # and it is usable afterwards
    assert abs(float(n) - 2.0 * 8 ** 0.5) < 1e-5 and abs(float(p.grad.norm()) - 1.0) < 1e-5


# ---------------------------------------------------------------- 4. ConvNet through TrainLoop
@pytest.mark.parametrize("opt_name,amp", [("AdamW", True), ("AdamW", False), ("SGD", True)],
                         ids=["adamw-bf16", "adamw-fp32", "sgd-bf16"])
def test_convnet_train_loop_clipped_graph_equals_eager(C, opt_name, amp):
    """Batch 32, 12 full steps (three replays of a 4-step graph) == the same loop run eagerly,
    bitwise, with a clip of half the first step's norm; and it is not the unclipped run."""
    from ddp_practice_amd import optim
    from ddp_practice_amd.amp import GradScaler
    from ddp_practice_amd.data import DeviceLoader, synthetic
    from ddp_practice_amd.engine import TrainLoop
    from ddp_practice_amd.models import ConvNet
    from ddp_practice_amd.nn import CrossEntropyLoss

    gc.collect()  # an uncollected GradScaler of an earlier test
    ds = synthetic(32 * 12, seed=5)
    torch.manual_seed(0)
    base = ConvNet(amp_dtype=torch.bfloat16 if amp else None).to(DEV)
    kw = dict(lr=1e-3, weight_decay=0.01) if opt_name == "AdamW" else dict(lr=1e-2)

    def loop_of(use_graph, clip):
        model = copy.deepcopy(base)
        loader = DeviceLoader(ds, batch_size=32, shuffle=False, device=DEV,
                              dtype=torch.bfloat16 if amp else torch.float32)
        opt = getattr(optim, opt_name)(model.parameters(), **kw)
        return model, opt, TrainLoop(model, CrossEntropyLoss(), opt, loader, GradScaler() if amp else None,
                                     use_graph=use_graph, steps_per_graph=4, clip_grad_norm=clip)

    # the first step's norm: one eager step under a clip that cannot bite
    model, _, probe = loop_of(False, 1e30)
    model.train()
    probe.loader.start_epoch()
    probe._eager_step()
    first = float(probe.grad_norm)
    assert math.isfinite(first) and first > 0.0
    v = 0.5 * first
    out = []
    for use_graph, clip in ((False, v), (True, v), (False, None)):
        model, opt, loop = loop_of(use_graph, clip)
        loop.run_epoch()
        torch.cuda.synchronize()
        assert loop.graph_error is None, loop.graph_error
        assert loop.global_step == 12
        state = [t for p in model.parameters() for t in opt.state[p].values() if torch.is_tensor(t) and t.dim() > 0]
        out.append((model.state_dict(), state, None if clip is None else loop.grad_norm.clone()))
    (sd_e, s_e, n_e), (sd_g, s_g, n_g), (sd_u, _, _) = out
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), (k, (sd_e[k].float() - sd_g[k].float()).abs().max().item())
    if s_e:
        _exact(s_g, s_e, "optimizer state, graph vs eager")
    _exact([n_g], [n_e], "the last step's norm, graph vs eager")
    assert not torch.equal(sd_e["fc.weight"], sd_u["fc.weight"])
    assert not torch.equal(sd_e["fc.weight"], base.state_dict()["fc.weight"])
