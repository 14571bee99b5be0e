"""optim.EMA without a GPU: the float64 reference of tests/_ema_ref.py against torch's
``AveragedModel``, the class on CPU tensors bit for bit against ``AveragedModel`` (both lerp
branches, buffers averaged and copied), the ``state_dict`` round trips in both directions,
``applied()``, the constructor errors, the warm-up weights, and ``TrainLoop(ema=)`` eagerly."""
import copy

import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

from . import _ema_ref as R


def _net(dtype=torch.float32):
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Conv2d(1, 3, 3), torch.nn.BatchNorm2d(3), torch.nn.Flatten(),
                            torch.nn.Linear(3 * 36, 5))
    return m.to(dtype)


def _train_step(m, k):
    """Stand-in for an optimizer step: move every parameter, and a train-mode forward for the BN buffers."""
    g = torch.Generator().manual_seed(100 + k)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(torch.randn(p.shape, generator=g, dtype=p.dtype) * 0.1)
    m.train()
    m(torch.randn(4, 1, 8, 8, generator=g, dtype=next(m.parameters()).dtype))


def _torch_ema(m, decay, use_buffers):
    return AveragedModel(m, multi_avg_fn=get_ema_multi_avg_fn(decay), use_buffers=use_buffers)


@pytest.mark.parametrize("decay", [0.999, 0.3])
def test_reference_equals_torch_in_float64(decay):
    m = _net(torch.float64)
    t = _torch_ema(m, decay, False)
    seen = []
    for k in range(5):
        _train_step(m, k)
        t.update_parameters(m)
        seen.append({n: p.detach().clone() for n, p in m.named_parameters()})
    assert int(t.n_averaged) == 5
    for n, p in t.module.named_parameters():
        ref = R.trajectory([s[n] for s in seen], decay)
        # float64 against float64: a few roundings of 2^-53 per update (ATen's lerp orders them otherwise)
        torch.testing.assert_close(p.detach(), ref, rtol=1e-13, atol=1e-15)


def test_reference_warmup_decays():
    assert R.decay_of(1, 0.999, True) == 2.0 / 11.0
    assert R.decay_of(9, 0.999, True) == 10.0 / 19.0
    assert R.decay_of(10_000, 0.999, True) == 0.999  # (1 + n) / (10 + n) = 0.99910...: the constant wins
    assert R.decay_of(5, 0.999, False) == 0.999
    a, b = torch.tensor([1.0, -2.0]), torch.tensor([3.0, 4.0])
    r, bound = R.update(a, b, 1, 0.999, True)
    assert torch.equal(r, a.double() + (1 - 2.0 / 11.0) * (b.double() - a.double())) and bool((bound > 0).all())
    r0, b0 = R.update(a, b, 0, 0.999, True)
    assert torch.equal(r0, b.double()) and bool((b0 == 0).all())


@pytest.mark.parametrize("use_buffers", [False, True], ids=["copy-buffers", "avg-buffers"])
@pytest.mark.parametrize("decay", [0.999, 0.3])
def test_cpu_bitwise_equal_to_torch_averaged_model(decay, use_buffers):
    from ddp_practice_amd.optim import EMA

    m = _net()
    t = _torch_ema(m, decay, use_buffers)
    e = EMA(m, decay=decay, use_buffers=use_buffers)
    assert int(e.n_averaged) == 0 and e.n_averaged.dtype == torch.int64
    for k in range(5):
        _train_step(m, k)
        t.update_parameters(m)
        e.update()
        assert int(e.n_averaged) == k + 1
    tsd = t.module.state_dict()
    assert list(e.shadows) == list(tsd)
    moved = 0
    for n, s in e.shadows.items():
        if not s.is_floating_point():
            # the stated deviation: integer buffers are copied (torch averages and truncates them
            # when use_buffers is on)
            assert torch.equal(s, m.state_dict()[n]) and int(s) == 5, n
            continue
        assert torch.equal(s, tsd[n]), (n, (s - tsd[n]).abs().max().item())
        moved += int(not torch.equal(s, m.state_dict()[n]))
    assert moved >= 4  # an average, not a copy of the weights


def test_state_dict_round_trips_with_torch():
    from ddp_practice_amd.optim import EMA

    m = _net()
    e = EMA(m, decay=0.9)
    for k in range(3):
        _train_step(m, k)
        e.update()
    sd = e.state_dict()
    t = _torch_ema(_net(), 0.9, False)
    assert list(sd) == list(t.state_dict())
    assert sd["n_averaged"].dtype == torch.int64 and sd["n_averaged"].dim() == 0
    t.load_state_dict(sd)  # strict
    assert int(t.n_averaged) == 3
    for n, v in t.module.state_dict().items():
        assert torch.equal(v, e.shadows[n]), n
    # the copy is detached from the shadows
    sd["module.3.bias"].zero_()
    assert bool(e.shadows["3.bias"].abs().sum() > 0)
    # and the reverse
    _train_step(m, 7)
    t.update_parameters(m)
    e2 = EMA(_net(), decay=0.9)
    e2.load_state_dict(t.state_dict())
    assert int(e2.n_averaged) == 4
    for n, v in t.module.state_dict().items():
        assert torch.equal(v, e2.shadows[n]), n
    bad = dict(t.state_dict())
    bad.pop("module.3.bias")
    with pytest.raises(KeyError, match="3.bias"):
        e2.load_state_dict(bad)


def test_applied_swaps_values_in_and_restores_bitwise():
    from ddp_practice_amd.optim import EMA

    m = _net()
    e = EMA(m, decay=0.5)
    for k in range(2):
        _train_step(m, k)
        e.update()
    live = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ptrs = {k: v.data_ptr() for k, v in m.state_dict().items()}
    with e.applied() as inner:
        assert inner is m
        for k, v in m.state_dict().items():
            assert torch.equal(v, e.shadows[k]), k
        assert not torch.equal(m.state_dict()["3.weight"], live["3.weight"])
    for k, v in m.state_dict().items():
        assert torch.equal(v, live[k]) and v.data_ptr() == ptrs[k], k
    with pytest.raises(ZeroDivisionError):  # restored on an exception too
        with e.applied():
            1 / 0
    for k, v in m.state_dict().items():
        assert torch.equal(v, live[k]), k


def test_constructor_and_update_errors():
    from ddp_practice_amd.optim import EMA

    m = _net()
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="decay"):
            EMA(m, decay=bad)
    EMA(m, decay=0.0)
    EMA(m, decay=1.0)

    class DistributedDataParallel(torch.nn.Module):  # the wrapper's .module is what is averaged
        def __init__(self, module):
            super().__init__()
            self.module = module

    e = EMA(DistributedDataParallel(m), decay=0.9)
    assert e.model is m and list(e.shadows) == list(m.state_dict())
    # no deep copy of the module: tensors only
    assert all(isinstance(v, torch.Tensor) and not isinstance(v, torch.nn.Parameter) for v in e.shadows.values())
    e.shadows["3.bias"] = m.state_dict()["3.bias"]
    with pytest.raises(RuntimeError, match="aliases"):
        e.update()


def test_snapshot_restore():
    from ddp_practice_amd.optim import EMA

    m = _net()
    e = EMA(m, decay=0.9)
    _train_step(m, 0)
    e.update()
    snap = e._snapshot()
    before = {k: v.clone() for k, v in e.shadows.items()}
    _train_step(m, 1)
    e.update()
    e.update()
    assert int(e.n_averaged) == 3
    e._restore(snap)
    assert int(e.n_averaged) == 1
    for k, v in e.shadows.items():
        assert torch.equal(v, before[k]), k


def test_warmup_weights_and_fallback_within_the_counted_bound():
    from ddp_practice_amd.optim import EMA
    from ddp_practice_amd.optim.ema import warmup_weight

    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))  # noqa: E731
    assert warmup_weight(1, 0.999) == f32(1.0 - f32(2.0 / 11.0))
    assert warmup_weight(9, 0.999) == f32(1.0 - f32(10.0 / 19.0))
    assert warmup_weight(10_000, 0.999) == f32(1.0 - 0.999)  # the host's float32 of the double
    m = _net()
    e = EMA(m, decay=0.999, warmup=True)
    plain = EMA(m, decay=0.999)
    for k in range(4):
        _train_step(m, k)
        prev = {n: s.clone() for n, s in e.shadows.items()}
        e.update()
        plain.update()
        for n, p in m.named_parameters():
            r, bound = R.update(prev[n], p, k, 0.999, True)
            err = (e.shadows[n].double() - r).abs()
            assert bool((err <= bound).all()), (k, n, float((err / bound.clamp_min(1e-300)).max()))
    # and it is the warm-up, not the constant decay
    assert not torch.equal(e.shadows["3.weight"], plain.shadows["3.weight"])


@pytest.mark.slow
def test_train_loop_updates_after_every_step_and_equals_torch():
    from ddp_practice_amd import optim as native_optim
    from ddp_practice_amd.data import DeviceLoader, synthetic
    from ddp_practice_amd.engine import TrainLoop
    from ddp_practice_amd.models import ConvNet

    ds = synthetic(32 * 3, seed=7)
    torch.manual_seed(0)
    base = ConvNet(amp_dtype=None, fused=False)
    crit = torch.nn.CrossEntropyLoss()

    ma = copy.deepcopy(base)
    ea = native_optim.EMA(ma, decay=0.9)
    la = DeviceLoader(ds, batch_size=32, shuffle=False, device="cpu", dtype=torch.float32)
    loop = TrainLoop(ma, crit, native_optim.SGD(ma.parameters(), lr=1e-2), la, None, ema=ea)
    loop.run_epoch()
    assert int(ea.n_averaged) == 3

    # the same loop with torch's AveragedModel as ema=, and a hand-written one
    mb = copy.deepcopy(base)
    eb = _torch_ema(mb, 0.9, False)
    lb = DeviceLoader(ds, batch_size=32, shuffle=False, device="cpu", dtype=torch.float32)
    TrainLoop(mb, crit, native_optim.SGD(mb.parameters(), lr=1e-2), lb, None, ema=eb).run_epoch()
    mc = copy.deepcopy(base)
    mc.train()
    ec = _torch_ema(mc, 0.9, False)
    oc = torch.optim.SGD(mc.parameters(), lr=1e-2)
    for x, y in DeviceLoader(ds, batch_size=32, shuffle=False, device="cpu", dtype=torch.float32):
        loss = crit(mc(x), y)
        oc.zero_grad(set_to_none=True)
        loss.backward()
        oc.step()
        ec.update_parameters(mc)
    assert int(eb.n_averaged) == int(ec.n_averaged) == 3
    for k, v in ec.module.state_dict().items():
        assert torch.equal(eb.module.state_dict()[k], v), k
        assert torch.equal(ea.shadows[k], v), k
    assert not torch.equal(ea.shadows["fc.weight"], ma.state_dict()["fc.weight"])
