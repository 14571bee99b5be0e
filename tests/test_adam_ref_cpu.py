"""tests/_adam_ref.py against torch's own Adam / AdamW in float64, and optim.AdamW / optim.Adam
on CPU tensors (constructor, torch delegation, the shared per-group step, state_dict)."""
import copy

import pytest
import torch

from ddp_practice_amd.optim import Adam, AdamW

from . import _adam_ref as R

SHAPES = [(5,), (3, 4), (1,), (17,)]


def _data(steps, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(s, generator=g, dtype=dtype) for s in SHAPES]
    grads = [[torch.randn(s, generator=g, dtype=dtype) for s in SHAPES] for _ in range(steps)]
    return init, grads


@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam"])
def test_reference_matches_torch_float64(decoupled, wd, maximize):
    """Five steps of the reference == torch.optim.AdamW / Adam on float64 tensors, to float64
    rounding (the two differ only in the association of a few float64 operations)."""
    init, grads = _data(5)
    hyper = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    ps = [torch.nn.Parameter(p.double()) for p in init]
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(ps, maximize=maximize, foreach=False, **hyper)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.double()
        opt.step()
    for i, p0 in enumerate(init):
        out = R.trajectory(p0, [gs[i] for gs in grads], decoupled=decoupled, maximize=maximize, **hyper)
        torch.testing.assert_close(out["p"], ps[i].detach(), rtol=1e-12, atol=1e-14)
        torch.testing.assert_close(out["m"], opt.state[ps[i]]["exp_avg"], rtol=1e-12, atol=1e-14)
        torch.testing.assert_close(out["v"], opt.state[ps[i]]["exp_avg_sq"], rtol=1e-12, atol=1e-16)


def test_reference_bounds_hold_for_torch_float32():
    """The counted bounds are bounds: torch's float32 CPU step (another association of the same
    roundings) stays inside them, and they are tight enough to be a test (p within 1e-5 of |p| + lr)."""
    init, grads = _data(1, seed=1)
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    for t0 in (0, 999):
        ps = [torch.nn.Parameter(p.clone()) for p in init]
        opt = torch.optim.AdamW(ps, foreach=False, **hyper)
        ms = [torch.randn_like(p) * 0.1 for p in init]
        vs = [torch.rand_like(p) for p in init]
        for p, g, m, v in zip(ps, grads[0], ms, vs):
            p.grad = g
            opt.state[p].update(step=torch.tensor(float(t0)), exp_avg=m.clone(), exp_avg_sq=v.clone())
        opt.step()
        for p0, p, g, m, v in zip(init, ps, grads[0], ms, vs):
            o = R.step(p0, g, m, v, t0 + 1, decoupled=True, **hyper)
            assert bool(((p.detach().double() - o["p"]).abs() <= o["bp"]).all())
            assert bool(((opt.state[p]["exp_avg"].double() - o["m"]).abs() <= o["bm"]).all())
            assert bool(((opt.state[p]["exp_avg_sq"].double() - o["v"]).abs() <= o["bv"]).all())
            assert bool((o["bp"] <= 1e-5 * (p0.abs().double() + hyper["lr"])).all())


def test_ulp_distance():
    a = torch.tensor([1.0, -1.0, 0.0, 3.0])
    b = torch.tensor([1.0 + 2 ** -23, -1.0, -0.0, 3.0])
    assert R.ulp_distance(a, a) == 0 and R.ulp_distance(a, b) == 1
    assert R.ulp_distance(torch.tensor([2.0 ** -149]), torch.tensor([-(2.0 ** -149)])) == 2


@pytest.mark.parametrize("cls,tcls", [(AdamW, torch.optim.AdamW), (Adam, torch.optim.Adam)])
@pytest.mark.parametrize("maximize", [False, True])
def test_cpu_tensors_bitwise_equal_torch(cls, tcls, maximize):
    init, grads = _data(4, seed=2)
    kw = dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.02, maximize=maximize)
    pa = [torch.nn.Parameter(p.clone()) for p in init]
    pt = [torch.nn.Parameter(p.clone()) for p in init]
    opt, ref = cls(pa, **kw), tcls(pt, **kw)
    for gs in grads:
        for p, q, g in zip(pa, pt, gs):
            p.grad, q.grad = g.clone(), g.clone()
        opt.step()
        ref.step()
    for p, q in zip(pa, pt):
        assert torch.equal(p, q)
        assert torch.equal(opt.state[p]["exp_avg"], ref.state[q]["exp_avg"])
        assert torch.equal(opt.state[p]["exp_avg_sq"], ref.state[q]["exp_avg_sq"])
        assert float(opt.state[p]["step"]) == float(ref.state[q]["step"]) == 4.0
    # the group's one word
    assert all(opt.state[p]["step"] is opt.state[pa[0]]["step"] for p in pa)
    assert opt.state[pa[0]]["step"].dtype == torch.float32 and opt.state[pa[0]]["step"].dim() == 0


def test_defaults_match_torch():
    p = [torch.nn.Parameter(torch.zeros(3))]
    for cls, tcls in ((AdamW, torch.optim.AdamW), (Adam, torch.optim.Adam)):
        a, t = cls(p).param_groups[0], tcls(p).param_groups[0]
        assert {k: v for k, v in a.items() if k != "params"} == {k: v for k, v in t.items() if k != "params"}


def _stepped(cls, init, grads, **kw):
    ps = [torch.nn.Parameter(p.clone()) for p in init]
    opt = cls(ps, **kw)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        opt.step()
    return ps, opt


def test_state_dict_round_trips_with_torch():
    """ours -> torch.optim.AdamW and torch -> ours, each continued for two steps next to the
    optimizer the state came from: bitwise the same parameters."""
    init, grads = _data(5, seed=3)
    kw = dict(lr=2e-3, weight_decay=0.01)
    for src_cls, dst_cls in ((AdamW, torch.optim.AdamW), (torch.optim.AdamW, AdamW)):
        ps, src = _stepped(src_cls, init, grads[:3], **kw)
        sd = copy.deepcopy(src.state_dict())
        assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
        qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
        dst = dst_cls(qs, **kw)
        dst.load_state_dict(sd)
        for gs in grads[3:]:
            for p, q, g in zip(ps, qs, gs):
                p.grad, q.grad = g.clone(), g.clone()
            src.step()
            dst.step()
        for p, q in zip(ps, qs):
            assert torch.equal(p, q)
            assert float(src.state[p]["step"]) == float(dst.state[q]["step"]) == 5.0
    # ours: the loaded counts are one word again; the file holds one copy per parameter
    assert all(dst.state[q]["step"] is dst.state[qs[0]]["step"] for q in qs)
    sd = dst.state_dict()
    assert sd["state"][0]["step"] is not sd["state"][1]["step"]
    # through a file, as cli.py does
    import io

    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    again = AdamW([torch.nn.Parameter(q.detach().clone()) for q in qs], **kw)
    again.load_state_dict(torch.load(buf, weights_only=True))
    assert float(again.state[again.param_groups[0]["params"][0]]["step"]) == 5.0


def test_load_state_dict_refuses_disagreeing_steps_and_other_states():
    init, grads = _data(2, seed=4)
    ps, opt = _stepped(AdamW, init, grads)
    sd = opt.state_dict()
    sd["state"][1]["step"] = torch.tensor(7.0)
    with pytest.raises(ValueError, match="disagree"):
        AdamW([torch.nn.Parameter(p.detach().clone()) for p in ps]).load_state_dict(sd)
    sgd = torch.optim.SGD([torch.nn.Parameter(p.clone()) for p in init], lr=0.1, momentum=0.9)
    for p, g in zip(sgd.param_groups[0]["params"], grads[0]):
        p.grad = g.clone()
    sgd.step()
    with pytest.raises(ValueError, match="not an Adam state"):
        AdamW([torch.nn.Parameter(p.detach().clone()) for p in ps]).load_state_dict(sgd.state_dict())


def test_partial_gradients_raise():
    ps = [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2))]
    opt = AdamW(ps)
    ps[0].grad = torch.ones(3)
    with pytest.raises(RuntimeError, match="share"):
        opt.step()
    # a group of its own may sit a step out
    opt = AdamW([{"params": [ps[0]]}, {"params": [ps[1]]}])
    opt.step()
    assert float(opt.state[ps[0]]["step"]) == 1.0 and ps[1] not in opt.state


def test_found_inf_skips_on_cpu():
    p = torch.nn.Parameter(torch.ones(3))
    p.grad = torch.ones(3)
    opt = AdamW([p])
    opt.step(found_inf=torch.ones(1))
    assert torch.equal(p.detach(), torch.ones(3))
    opt.step(found_inf=torch.zeros(1))
    assert not torch.equal(p.detach(), torch.ones(3)) and float(opt.state[p]["step"]) == 1.0


@pytest.mark.parametrize("kw,match", [
    (dict(lr=-1.0), "Invalid learning rate"), (dict(eps=-1.0), "Invalid epsilon"),
    (dict(betas=(1.0, 0.9)), "index 0"), (dict(betas=(0.9, -0.1)), "index 1"),
    (dict(weight_decay=-1.0), "Invalid weight_decay"), (dict(amsgrad=True), "amsgrad"),
    (dict(lr=torch.tensor(0.1)), "DeviceLR"),
])
def test_constructor_errors(kw, match):
    for cls in (AdamW, Adam):
        with pytest.raises(ValueError, match=match):
            cls([torch.nn.Parameter(torch.zeros(2))], **kw)


def test_complex_parameters_raise():
    with pytest.raises(ValueError, match="complex"):
        AdamW([torch.nn.Parameter(torch.zeros(2, dtype=torch.complex64))])
