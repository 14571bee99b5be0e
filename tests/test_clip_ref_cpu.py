"""Gradient clipping without a GPU: the float64 reference of tests/_clip_ref.py against torch,
``optim.clip_grad_norm_``'s fall-through to torch's function, ``TrainLoop(clip_grad_norm=)``
against a hand-written torch loop, and the ``--clip-grad-norm`` flag."""
import copy
import os
import subprocess
import sys

import pytest
import torch

from . import _clip_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "origin_main.py")
DATA = ["--synthetic", "--train-samples", "96", "--test-samples", "32", "--seed", "0", "-e", "1"]  # 3 steps of 32


def _params(sizes, seed, dtype=torch.float32):
    gen = torch.Generator().manual_seed(seed)
    ps = []
    for n in sizes:
        p = torch.nn.Parameter(torch.randn(n, generator=gen).to(dtype))
        p.grad = (torch.randn(n, generator=gen) * 3).to(dtype)
        ps.append(p)
    return ps


@pytest.mark.parametrize("max_norm", [0.5, 1e4])
def test_reference_equals_torch_in_float64(max_norm):
    ps = _params([1, 7, 400, 4099], seed=1, dtype=torch.float64)
    ref = R.reference([p.grad for p in ps], max_norm)
    norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    assert abs(float(norm) - ref["norm"]) <= 1e-14 * ref["norm"]
    assert (ref["coef"] < 1.0) == (max_norm == 0.5)
    for p, c in zip(ps, ref["clipped"]):
        torch.testing.assert_close(p.grad, c, rtol=1e-14, atol=0)


def test_reference_unscales_first():
    ps = _params([33], seed=2)
    a = R.reference([p.grad * 1024.0 for p in ps], 1.0, scale=1024.0)
    b = R.reference([p.grad for p in ps], 1.0)
    assert a["norm"] == b["norm"] and a["coef"] == b["coef"]


def test_counted_roundings():
    # square, 4U - 1 lane adds, six wave levels, three wave-order adds, the final rounding
    assert R.sumsq_roundings(4) == 1 + 15 + 6 + 3 + 1
    assert R.sumsq_roundings(1) == 1 + 3 + 6 + 3 + 1
    assert R.sumsq_roundings(4, unscale=True) == R.sumsq_roundings(4) + 4
    assert R.norm_rel_bound(4) == R.sumsq_roundings(4) * 2.0 ** -24 / 2 + 2.0 ** -24


@pytest.mark.parametrize("norm_type", [2.0, 1.0, float("inf")])
def test_cpu_tensors_take_torchs_function_bitwise(norm_type):
    from ddp_practice_amd.optim import clip_grad_norm_

    a, b = _params([5, 400, 33], seed=3), _params([5, 400, 33], seed=3)
    na = clip_grad_norm_(a, 0.25, norm_type=norm_type)
    nb = torch.nn.utils.clip_grad_norm_(b, 0.25, norm_type=norm_type)
    assert torch.equal(na, nb)
    for p, q in zip(a, b):
        assert torch.equal(p.grad, q.grad)
    assert not torch.equal(a[1].grad, _params([5, 400, 33], seed=3)[1].grad)  # it did clip


def test_empty_list_parameters_without_grad_single_tensor_and_generator():
    from ddp_practice_amd.optim import clip_grad_norm_

    assert float(clip_grad_norm_([], 1.0)) == 0.0
    ps = _params([4, 9], seed=4)
    ps[0].grad = None
    kept = ps[1].grad.clone()
    n = clip_grad_norm_(ps, 1e9)
    assert float(n) == float(kept.norm()) and ps[0].grad is None and torch.equal(ps[1].grad, kept)
    assert float(clip_grad_norm_([torch.nn.Parameter(torch.ones(3))], 1.0)) == 0.0  # none has a gradient
    assert float(clip_grad_norm_(ps[1], 1e9)) == float(n)  # a single tensor
    assert float(clip_grad_norm_((p for p in ps), 1e9)) == float(n)  # a generator
    ps[1].grad[0] = float("inf")
    with pytest.raises(RuntimeError, match="non-finite"):
        clip_grad_norm_(ps, 1.0, error_if_nonfinite=True)


def test_optimizer_keyword_flushes_first():
    from ddp_practice_amd.optim import clip_grad_norm_

    calls = []

    class Opt:
        def _flush_deferred(self):
            calls.append(1)

    ps = _params([8], seed=5)
    clip_grad_norm_(ps, 1.0, optimizer=Opt())
    clip_grad_norm_(ps, 1.0, optimizer=object())  # an optimizer without the hook
    assert calls == [1]


def test_set_grad_clip_is_an_attribute_and_the_cpu_step_clips_with_torch():
    from ddp_practice_amd.optim import AdamW

    a, b = _params([5, 40], seed=6), _params([5, 40], seed=6)
    oa, ob = AdamW(a, lr=1e-2), torch.optim.AdamW(b, lr=1e-2)
    assert oa.grad_norm is None
    with pytest.raises(ValueError):
        oa.set_grad_clip(0.0)
    oa.set_grad_clip(0.5)
    oa.step()
    nb = torch.nn.utils.clip_grad_norm_(b, 0.5)
    ob.step()
    assert float(oa.grad_norm) == float(nb)
    for p, q in zip(a, b):
        assert torch.equal(p, q)
    sd = oa.state_dict()
    assert all("clip" not in k and "max_norm" not in k for g in sd["param_groups"] for k in g)
    ob.load_state_dict(sd)  # still torch.optim.AdamW's layout
    oa.set_grad_clip(None)
    assert oa._clip is None


@pytest.mark.slow
@pytest.mark.parametrize("opt_name", ["SGD", "AdamW"])
def test_train_loop_equals_a_torch_loop_with_torchs_clip(opt_name):
    from ddp_practice_amd import optim as native_optim
    from ddp_practice_amd.data import DeviceLoader, synthetic
    from ddp_practice_amd.engine import TrainLoop
    from ddp_practice_amd.models import ConvNet

    ds = synthetic(32 * 3, seed=7)
    torch.manual_seed(0)
    base = ConvNet(amp_dtype=None, fused=False)
    kw = dict(lr=1e-2)
    # the clip must bite: half of the first step's norm, measured here
    m0 = copy.deepcopy(base)
    crit = torch.nn.CrossEntropyLoss()
    loader0 = DeviceLoader(ds, batch_size=32, shuffle=False, device="cpu", dtype=torch.float32)
    x0, y0 = next(iter(loader0))
    crit(m0(x0), y0).backward()
    v = 0.5 * float(torch.nn.utils.clip_grad_norm_(m0.parameters(), 1e9))
    assert v > 0

    ma = copy.deepcopy(base)
    la = DeviceLoader(ds, batch_size=32, shuffle=False, device="cpu", dtype=torch.float32)
    loop = TrainLoop(ma, crit, getattr(native_optim, opt_name)(ma.parameters(), **kw), la, None, clip_grad_norm=v)
    loop.run_epoch()

    mb = copy.deepcopy(base)
    mb.train()
    ob = getattr(torch.optim, opt_name)(mb.parameters(), **kw)
    lb = DeviceLoader(ds, batch_size=32, shuffle=False, device="cpu", dtype=torch.float32)
    last = None
    for x, y in lb:
        loss = crit(mb(x), y)
        ob.zero_grad(set_to_none=True)
        loss.backward()
        last = torch.nn.utils.clip_grad_norm_(mb.parameters(), v)
        ob.step()
    assert loop.global_step == 3 and float(loop.grad_norm) == float(last)
    for (k, a), b in zip(ma.state_dict().items(), mb.state_dict().values()):
        assert torch.equal(a, b), k

    mc = copy.deepcopy(base)
    lc = DeviceLoader(ds, batch_size=32, shuffle=False, device="cpu", dtype=torch.float32)
    plain = TrainLoop(mc, crit, getattr(native_optim, opt_name)(mc.parameters(), **kw), lc, None)
    plain.run_epoch()
    assert plain.grad_norm is None
    assert not torch.equal(mc.state_dict()["fc.weight"], ma.state_dict()["fc.weight"])


def _run(args, cwd, ok=True):
    env = dict(os.environ)
    env.pop("CUDA_VISIBLE_DEVICES", None)
    r = subprocess.run([sys.executable, MAIN, *args], cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r


@pytest.mark.slow
def test_negative_flag_is_an_error(tmp_path):
    r = _run([*DATA, "--clip-grad-norm", "-1"], tmp_path, ok=False)
    assert "--clip-grad-norm" in r.stderr and not (tmp_path / "origin_checkpoint.pt").exists()


@pytest.mark.slow
def test_clipped_run_saves_its_optimizer_and_resumes(tmp_path):
    import json

    metrics = tmp_path / "m.jsonl"
    _run([*DATA, "--optimizer", "adamw", "--lr", "1e-3", "--clip-grad-norm", "0.5", "--checkpoint", "a.pt",
          "--metrics-file", str(metrics)], tmp_path)
    ck = torch.load(tmp_path / "a.pt", weights_only=True)
    assert list(ck) == ["model", "optimizer"]
    assert all(float(st["step"]) == 3.0 for st in ck["optimizer"]["state"].values())
    row = json.loads(metrics.read_text().splitlines()[0])
    assert row["grad_norm"] > 0.0
    _run([*DATA, "--optimizer", "adamw", "--lr", "1e-3", "--clip-grad-norm", "0.5", "--resume", "a.pt",
          "--start-epoch", "1", "--checkpoint", "b.pt"], tmp_path)
    ck2 = torch.load(tmp_path / "b.pt", weights_only=True)
    assert all(float(st["step"]) == 6.0 for st in ck2["optimizer"]["state"].values())
    # SGD with nothing but the clip flag is a non-default run too: its (empty) optimizer state is saved
    _run([*DATA, "--clip-grad-norm", "0.5", "--checkpoint", "s.pt", "--metrics-file", str(tmp_path / "s.jsonl")],
         tmp_path)
    assert "optimizer" in torch.load(tmp_path / "s.pt", weights_only=True)
    assert json.loads((tmp_path / "s.jsonl").read_text().splitlines()[0])["grad_norm"] > 0.0
    # and a run without the flag has no grad_norm column
    _run([*DATA, "--checkpoint", "d.pt", "--metrics-file", str(tmp_path / "d.jsonl")], tmp_path)
    assert "grad_norm" not in (tmp_path / "d.jsonl").read_text()
