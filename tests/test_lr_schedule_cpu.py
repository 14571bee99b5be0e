"""The device-resident learning-rate schedule (optim/lr.py DeviceLR) on its CPU paths: table
compilation from torch schedulers, SGD parity, hold past the end, resume, TrainLoop, CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch.optim import lr_scheduler as S

from ddp_practice_amd.optim import SGD, DeviceLR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STEPS = 40
SCHEDULERS = {
    "StepLR": lambda o: S.StepLR(o, step_size=7, gamma=0.5),
    "MultiStepLR": lambda o: S.MultiStepLR(o, milestones=[3, 11, 30], gamma=0.3),
    "LambdaLR": lambda o: S.LambdaLR(o, lambda k: 1.0 / (1.0 + 0.37 * k)),
    "OneCycleLR": lambda o: S.OneCycleLR(o, max_lr=[0.3, 0.07], total_steps=STEPS, cycle_momentum=False),
    # the CLI's --lr-schedule cosine
    "SequentialLR": lambda o: S.SequentialLR(
        o, [S.LinearLR(o, start_factor=0.01, total_iters=5), S.CosineAnnealingLR(o, T_max=STEPS - 5)], milestones=[5]),
}


def _params(seed=0):  # tests/test_amp_optim_cpu.py
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=g)) for n in (3, 17, 64)]


def _two_groups(ps, lrs=(0.1, 0.03)):
    return [{"params": ps[:1], "lr": lrs[0]}, {"params": ps[1:], "lr": lrs[1]}]


def _torch_sequence(make, steps):
    """get_last_lr() before each of ``steps`` steps of a real torch loop."""
    opt = torch.optim.SGD(_two_groups(_params()), lr=0.1)
    sched = make(opt)
    rows = []
    for _ in range(steps):
        rows.append(list(sched.get_last_lr()))
        opt.step()
        if len(rows) < steps:
            sched.step()
    return rows


@pytest.mark.parametrize("name", list(SCHEDULERS))
def test_from_torch_table_is_torch_sequence_in_float32(name):
    make = SCHEDULERS[name]
    opt = SGD(_two_groups(_params()), lr=0.1)
    dlr = DeviceLR.from_torch(opt, make, STEPS)
    want = np.asarray(_torch_sequence(make, STEPS), dtype=np.float64).astype(np.float32)
    got = dlr.table.numpy()
    assert got.shape == (STEPS, 2) and got.dtype == np.float32
    assert np.array_equal(got, want), np.abs(got - want).max()
    assert len({float(x) for x in got[:, 0]}) > 1  # a schedule, not a constant
    assert dlr.get_last_lr() == [float(x) for x in want[0]]


@pytest.mark.parametrize("momentum,wd,nesterov,damp", [(0.0, 0.0, False, 0.0), (0.9, 1e-4, False, 0.1),
                                                       (0.9, 0.0, True, 0.0)])
def test_cpu_sgd_with_device_lr_matches_torch_with_scheduler(momentum, wd, nesterov, damp):
    make = lambda o: S.OneCycleLR(o, max_lr=0.3, total_steps=12, cycle_momentum=False)  # noqa: E731
    a, b = _params(), _params()
    kw = dict(lr=0.1, momentum=momentum, weight_decay=wd, nesterov=nesterov, dampening=damp)
    oa, ob = SGD(a, **kw), torch.optim.SGD(b, **kw)
    sa, sb = DeviceLR.from_torch(oa, make, 12), make(ob)
    g = torch.Generator().manual_seed(1)
    for k in range(12):
        for p, q in zip(a, b):
            gr = torch.randn(p.shape, generator=g)
            p.grad, q.grad = gr.clone(), gr.clone()
        assert sa.get_last_lr() == [float(np.float32(x)) for x in sb.get_last_lr()]
        oa.step()
        ob.step()
        sa.step()
        if k < 11:
            sb.step()
    for p, q in zip(a, b):
        torch.testing.assert_close(p, q)


def test_rate_holds_past_the_end_and_rows_are_per_group():
    opt = SGD(_two_groups(_params()), lr=0.1)
    dlr = DeviceLR(opt, [0.5, 0.25, 0.125])
    seen = []
    for _ in range(6):
        seen.append(dlr.get_last_lr())
        dlr.step()
    assert seen == [[0.5, 0.5], [0.25, 0.25], [0.125, 0.125]] + [[0.125, 0.125]] * 3
    assert dlr.state_dict() == {"pos": 6}
    dlr = DeviceLR(opt, [(0.5, 0.1), (0.25, 0.05)])
    dlr.step()
    assert dlr.get_last_lr() == [0.25, float(np.float32(0.05))]
    with pytest.raises(ValueError):
        DeviceLR(opt, [(0.1, 0.2, 0.3)])
    with pytest.raises(ValueError):
        DeviceLR(opt, [])


def _run_steps(first, last, resume_from=None):
    make = lambda o: S.OneCycleLR(o, max_lr=0.3, total_steps=12, cycle_momentum=False)  # noqa: E731
    ps = _params()
    opt = SGD(ps, lr=0.1, momentum=0.9, weight_decay=1e-4)
    dlr = DeviceLR.from_torch(opt, make, 12)
    if resume_from is not None:
        with torch.no_grad():
            for p, q in zip(ps, resume_from["params"]):
                p.copy_(q)
        opt.load_state_dict(resume_from["optimizer"])
        dlr.load_state_dict(resume_from["lr_scheduler"])
    g = torch.Generator().manual_seed(1)
    grads = [[torch.randn(p.shape, generator=g) for p in ps] for _ in range(12)]
    for k in range(first, last):
        for p, gr in zip(ps, grads[k]):
            p.grad = gr.clone()
        opt.step()
        dlr.step()
    return {"params": [p.detach().clone() for p in ps], "optimizer": opt.state_dict(),
            "lr_scheduler": dlr.state_dict()}


def test_state_dict_round_trip_resumes_bitwise():
    whole = _run_steps(0, 12)
    half = _run_steps(0, 5)
    assert half["lr_scheduler"] == {"pos": 5}
    resumed = _run_steps(5, 12, resume_from=half)
    assert resumed["lr_scheduler"] == {"pos": 12}
    for p, q in zip(whole["params"], resumed["params"]):
        assert torch.equal(p, q)


def test_optimizer_state_dict_unchanged_by_device_lr():
    def sd(attach):
        ps = _params()
        opt = SGD(_two_groups(ps), lr=0.1, momentum=0.9)
        dlr = DeviceLR(opt, [0.1, 0.05]) if attach else None
        for p in ps:
            p.grad = torch.ones_like(p)
        opt.step()
        if dlr is not None:
            dlr.step()
        return opt.state_dict()

    a, b = sd(True), sd(False)
    assert a["param_groups"] == b["param_groups"]
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert a["state"][k].keys() == b["state"][k].keys() == {"momentum_buffer"}
        assert torch.equal(a["state"][k]["momentum_buffer"], b["state"][k]["momentum_buffer"])


@pytest.mark.parametrize("interval,want", [("step", 4), ("epoch", 1)])
def test_train_loop_steps_the_scheduler(interval, want):
    from ddp_practice_amd.data import DeviceLoader, synthetic
    from ddp_practice_amd.engine import TrainLoop
    from ddp_practice_amd.models import ConvNet
    from ddp_practice_amd.nn import CrossEntropyLoss

    torch.manual_seed(0)
    model = ConvNet()
    opt = SGD(model.parameters(), 0.1)
    dlr = DeviceLR(opt, [0.1 / (k + 1) for k in range(8)])
    loader = DeviceLoader(synthetic(4 * 8, seed=1), batch_size=8, shuffle=False, device=torch.device("cpu"))
    loop = TrainLoop(model, CrossEntropyLoss(), opt, loader, None, scheduler=dlr, scheduler_interval=interval)
    loop.run_epoch()
    assert loop.global_step == 4 and dlr.state_dict() == {"pos": want}
    assert dlr.get_last_lr() == [float(np.float32(0.1 / (want + 1)))]
    with pytest.raises(ValueError):
        TrainLoop(model, CrossEntropyLoss(), opt, loader, None, scheduler=dlr, scheduler_interval="batch")


def _cli(args, cwd):
    env = dict(os.environ)
    env.pop("CUDA_VISIBLE_DEVICES", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "origin_main.py"), "-e", "1", "--synthetic",
                        "--train-samples", "256", "--test-samples", "64", "--seed", "0", *args],
                       cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.slow
def test_cli_default_checkpoint_has_todays_keys(tmp_path):
    _cli([], tmp_path)
    ck = torch.load(tmp_path / "origin_checkpoint.pt", weights_only=True)
    assert list(ck) == ["model"]


@pytest.mark.slow
def test_cli_cosine_momentum_checkpoint_and_resume(tmp_path):
    import json

    flags = ["--lr", "0.01", "--lr-schedule", "cosine", "--warmup-steps", "3", "--momentum", "0.9"]
    _cli(flags + ["--metrics-file", str(tmp_path / "m.jsonl")], tmp_path)
    ck = torch.load(tmp_path / "origin_checkpoint.pt", weights_only=True)
    assert set(ck) == {"model", "optimizer", "lr_scheduler"}
    steps = int(ck["model"]["layer1.1.num_batches_tracked"])
    assert steps > 3 and ck["lr_scheduler"] == {"pos": steps}
    bufs = [st["momentum_buffer"] for st in ck["optimizer"]["state"].values()]
    assert bufs and all(torch.isfinite(b).all() and b.abs().sum() > 0 for b in bufs)
    # the rate of the metrics line is the schedule's at the end of the epoch: annealed to ~0
    rec = [json.loads(ln) for ln in open(tmp_path / "m.jsonl")]
    assert len(rec) == 1 and 0.0 <= rec[0]["lr"] < 0.01 * 0.05
    _cli(flags + ["--resume", str(tmp_path / "origin_checkpoint.pt"), "--start-epoch", "1", "--checkpoint",
                  str(tmp_path / "b.pt")], tmp_path)
    ck2 = torch.load(tmp_path / "b.pt", weights_only=True)
    assert ck2["lr_scheduler"] == {"pos": 2 * steps}
    assert int(ck2["model"]["layer1.1.num_batches_tracked"]) == 2 * steps
