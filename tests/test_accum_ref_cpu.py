"""optim.GradAccumulator without a GPU: the float64 reference of tests/_accum_ref.py against the
torch idiom, the class on CPU tensors bit for bit against the hand-written loop and against the
real idiom on a small MLP, its window rules (``steps=1``, ``last=True``, ``reset()``, errors),
``TrainLoop(accum_steps=)`` bitwise against a hand-written torch loop, ``--accum-steps`` through
origin_main.py, and DDP + SyncBN on two gloo ranks against one process."""
import copy
import json
import os
import subprocess
import sys

import pytest
import torch

from . import _accum_ref as R
from . import _accum_workers as W
from ._dist import run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "origin_main.py")


def _mlp(dtype=torch.float32):
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(7, 9), torch.nn.Tanh(), torch.nn.Linear(9, 5)).to(dtype)


def _micro(k, dtype=torch.float32):
    g = torch.Generator().manual_seed(50 + k)
    return torch.randn(6, 7, generator=g, dtype=dtype), torch.randint(0, 5, (6,), generator=g)


def _fresh_grads(m, k, dtype=torch.float32):
    x, y = _micro(k, dtype)
    for p in m.parameters():
        p.grad = None
    torch.nn.functional.cross_entropy(m(x), y).backward()
    return [p.grad.detach().clone() for p in m.parameters()]


@pytest.mark.parametrize("K", [2, 3, 7])
def test_reference_equals_torch_idiom_in_float64(K):
    m = _mlp(torch.float64)
    per = [_fresh_grads(m, k, torch.float64) for k in range(K)]
    for p in m.parameters():
        p.grad = None
    for k in range(K):
        x, y = _micro(k, torch.float64)
        (torch.nn.functional.cross_entropy(m(x), y) / K).backward()
    for i, p in enumerate(m.parameters()):
        mean, bound, mag = R.window([g[i] for g in per], K)
        # float64 against float64: K roundings of 2^-53 each way
        torch.testing.assert_close(p.grad, mean, rtol=1e-13, atol=1e-16)
        assert bool((bound > 0).all()) and bool((bound <= 1e-6 * mag + R.ETA).all())


def test_reference_bound_counts_the_roundings():
    assert R.gamma(4) == 4 * R.U32 / (1 - 4 * R.U32)
    g = [torch.tensor([1.0, -2.0]), torch.tensor([3.0, 2.0]), torch.tensor([-0.5, 0.25])]
    mean, bound, mag = R.window(g, 3)
    assert torch.equal(mean, torch.tensor([3.5, 0.25], dtype=torch.float64) / 3)
    assert torch.equal(mag, torch.tensor([4.5, 4.25], dtype=torch.float64) / 3)
    assert torch.equal(bound, R.gamma(4) * mag + R.ETA)
    short, b2, _ = R.window(g[:2], 3)  # a short window keeps 1 / K
    assert torch.equal(short, torch.tensor([4.0, 0.0], dtype=torch.float64) / 3)
    assert torch.equal(b2, R.gamma(3) * torch.tensor([4.0, 4.0], dtype=torch.float64) / 3 + R.ETA)


def _params(shapes, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]


def _set_grads(ps, k):
    g = torch.Generator().manual_seed(1000 + k)
    out = []
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g) * (10.0 ** (k % 3 - 1))
        out.append(p.grad.clone())
    return out


@pytest.mark.parametrize("K", [2, 3, 7])
def test_cpu_bitwise_equal_to_the_hand_written_loop(K):
    from ddp_practice_amd.optim import GradAccumulator

    ps = _params([(1,), (3,), (5, 7), (4, 4), (129,)])
    acc = GradAccumulator(torch.optim.SGD(ps, lr=0.1), steps=K)
    for window in range(2):
        seen = []
        for i in range(K):
            seen.append(_set_grads(ps, 10 * window + i))
            done = acc.accumulate()
            assert done == (i == K - 1) and acc.position == (0 if done else i + 1)
            if not done:
                assert all(p.grad is None for p in ps)
        for j, p in enumerate(ps):
            want = R.kernel_loop([s[j] for s in seen], K)
            assert torch.equal(p.grad, want), (window, j)
            mean, bound, _ = R.window([s[j] for s in seen], K)
            assert bool(((p.grad.double() - mean).abs() <= bound).all())
    assert acc.launches == 2 * K
    # the accumulators: float32, 16-byte aligned views of one flat buffer
    flat = acc._flat[torch.device("cpu")]
    for p in ps:
        a = acc._acc[id(p)]
        assert a.dtype == torch.float32 and a.shape == p.shape and a.data_ptr() % 16 == 0
        assert flat.data_ptr() <= a.data_ptr() < flat.data_ptr() + flat.numel() * 4


@pytest.mark.parametrize("K", [2, 4])
def test_cpu_bitwise_equal_to_the_torch_idiom_on_an_mlp(K):
    """Scaling by a power of two is exact while nothing is subnormal, so autograd's accumulation of
    the ``loss / K`` gradients and ``(g_0 + ... + g_{K-1}) * (1 / K)`` are the same floats."""
    from ddp_practice_amd.optim import GradAccumulator

    m = _mlp()
    ref = copy.deepcopy(m)
    for k in range(K):
        x, y = _micro(k)
        (torch.nn.functional.cross_entropy(ref(x), y) / K).backward()
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    acc = GradAccumulator(opt, steps=K)
    tiny = torch.finfo(torch.float32).tiny
    for k in range(K):
        x, y = _micro(k)
        opt.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(m(x), y).backward()
        for p in m.parameters():  # no subnormal gradients: the premise of the bitwise claim
            nz = p.grad[p.grad != 0]
            assert bool((nz.abs() >= tiny * K * 16).all())
        done = acc.accumulate()
    assert done
    for p, q in zip(m.parameters(), ref.parameters()):
        assert torch.equal(p.grad, q.grad)


def test_steps_one_launches_nothing():
    from ddp_practice_amd.optim import GradAccumulator

    ps = _params([(5,)])
    acc = GradAccumulator(torch.optim.SGD(ps, lr=0.1))
    g = _set_grads(ps, 0)
    assert acc.steps == 1 and acc.accumulate() is True and acc.accumulate(last=False) is True
    assert acc.launches == 0 and not acc._flat and torch.equal(ps[0].grad, g[0])


@pytest.mark.parametrize("steps", [0, -1, 2.0, "2", None, True])
def test_constructor_errors(steps):
    from ddp_practice_amd.optim import GradAccumulator

    with pytest.raises(ValueError, match="steps"):
        GradAccumulator(torch.optim.SGD(_params([(5,)]), lr=0.1), steps=steps)


def test_short_window_and_reset():
    from ddp_practice_amd.optim import GradAccumulator

    ps = _params([(6,), (3, 3)])
    acc = GradAccumulator(torch.optim.SGD(ps, lr=0.1), steps=4)
    # two micro-steps closed early: the factor stays 1 / 4
    a = _set_grads(ps, 0)
    assert acc.accumulate() is False
    b = _set_grads(ps, 1)
    assert acc.accumulate(last=True) is True and acc.position == 0
    for j, p in enumerate(ps):
        assert torch.equal(p.grad, (a[j] + b[j]) * 0.25)
    # a window of a single micro-step
    c = _set_grads(ps, 2)
    assert acc.accumulate(last=True) is True
    for j, p in enumerate(ps):
        assert torch.equal(p.grad, c[j] * 0.25)
    # reset() drops a half-finished window: the next one does not see it
    _set_grads(ps, 3)
    assert acc.accumulate() is False and acc.position == 1
    acc.reset()
    assert acc.position == 0
    seen = []
    for i in range(4):
        seen.append(_set_grads(ps, 4 + i))
        done = acc.accumulate()
    assert done
    for j, p in enumerate(ps):
        assert torch.equal(p.grad, R.kernel_loop([s[j] for s in seen], 4))
    # the set of parameters with a gradient may not change within a window
    _set_grads(ps, 9)
    acc.accumulate()
    _set_grads(ps, 10)
    ps[1].grad = None
    with pytest.raises(RuntimeError, match="changed within a window"):
        acc.accumulate()


def test_non_float32_gradients_take_the_fallback_in_float32():
    from ddp_practice_amd.optim import GradAccumulator

    ps = [torch.nn.Parameter(torch.randn(9, dtype=torch.float64))]
    acc = GradAccumulator(torch.optim.SGD(ps, lr=0.1), steps=2)
    g0 = torch.randn(9, dtype=torch.float64)
    g1 = torch.randn(9, dtype=torch.float64)
    ps[0].grad = g0.clone()
    acc.accumulate()
    ps[0].grad = g1.clone()
    assert acc.accumulate()
    assert ps[0].grad.dtype == torch.float64
    assert torch.equal(ps[0].grad, ((g0.float() + g1) * 0.5))


@pytest.mark.slow
@pytest.mark.parametrize("K", [2, 3])
def test_train_loop_equals_a_hand_written_loop(K):
    from ddp_practice_amd import optim as native_optim
    from ddp_practice_amd.data import DeviceLoader, synthetic
    from ddp_practice_amd.engine import TrainLoop
    from ddp_practice_amd.models import ConvNet

    ds = synthetic(8 * 2 * K + 5, seed=7)  # 2K full batches and a partial tail: 2 windows + a short one
    torch.manual_seed(0)
    base = ConvNet(amp_dtype=None, fused=False)
    crit = torch.nn.CrossEntropyLoss()

    ma = copy.deepcopy(base)
    la = DeviceLoader(ds, batch_size=8, shuffle=False, device="cpu", dtype=torch.float32)
    oa = native_optim.SGD(ma.parameters(), lr=1e-2, momentum=0.9)
    loop = TrainLoop(ma, crit, oa, la, None, accum_steps=K)
    loop.run_epoch()
    assert loop.global_step == 3 and loop.accum.launches == 2 * K + 1

    mb = copy.deepcopy(base)
    mb.train()
    ob = torch.optim.SGD(mb.parameters(), lr=1e-2, momentum=0.9)
    batches = list(DeviceLoader(ds, batch_size=8, shuffle=False, device="cpu", dtype=torch.float32))
    assert len(batches) == 2 * K + 1 and batches[-1][0].shape[0] == 5
    for s in range(0, len(batches), K):
        seen = []
        for x, y in batches[s:s + K]:
            ob.zero_grad(set_to_none=True)
            crit(mb(x), y).backward()
            seen.append([p.grad.clone() for p in mb.parameters()])
        for j, p in enumerate(mb.parameters()):
            p.grad = R.kernel_loop([g[j] for g in seen], K)
        ob.step()
    for (n, p), (_, q) in zip(ma.state_dict().items(), mb.state_dict().items()):
        assert torch.equal(p, q), n

    # the torch idiom (accum_impl="torch": loss / K, autograd's accumulation) on the same loop
    mc = copy.deepcopy(base)
    lc = DeviceLoader(ds, batch_size=8, shuffle=False, device="cpu", dtype=torch.float32)
    lt = TrainLoop(mc, crit, torch.optim.SGD(mc.parameters(), lr=1e-2, momentum=0.9), lc, None, accum_steps=K,
                   accum_impl="torch")
    lt.run_epoch()
    assert lt.global_step == 3 and lt.accum is None
    for (n, p), (_, q) in zip(ma.state_dict().items(), mc.state_dict().items()):
        if K == 2:  # a power of two: the same floats
            assert torch.equal(p, q), n
        else:
            torch.testing.assert_close(p, q, rtol=1e-4, atol=1e-5, msg=n)


@pytest.mark.parametrize("bad", [0, -2, 1.5, True])
def test_train_loop_accum_steps_errors(bad):
    from ddp_practice_amd.data import DeviceLoader, synthetic
    from ddp_practice_amd.engine import TrainLoop

    m = _mlp()
    la = DeviceLoader(synthetic(16, seed=1), batch_size=8, shuffle=False, device="cpu", dtype=torch.float32)
    with pytest.raises(ValueError, match="accum_steps"):
        TrainLoop(m, torch.nn.CrossEntropyLoss(), torch.optim.SGD(m.parameters(), lr=0.1), la, None, accum_steps=bad)


# ------------------------------------------------------------------ CLI
DATA = ["--synthetic", "--train-samples", "168", "--test-samples", "32", "--seed", "0", "-e", "1", "-b", "32"]
# 168 samples: 5 full batches of 32 and a tail of 8 -> with K = 2: 3 updates per epoch


def _run(args, cwd, ok=True):
    env = dict(os.environ)
    env.pop("CUDA_VISIBLE_DEVICES", None)
    r = subprocess.run([sys.executable, MAIN, *args], cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r


@pytest.mark.slow
@pytest.mark.parametrize("k", ["0", "-3"])
def test_cli_flag_errors(tmp_path, k):
    r = _run([*DATA, "--accum-steps", k], tmp_path, ok=False)
    assert "error:" in r.stderr and "--accum-steps" in r.stderr and "Traceback" not in r.stderr
    assert not (tmp_path / "origin_checkpoint.pt").exists()


@pytest.mark.slow
def test_cli_default_run_is_unchanged(tmp_path):
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()  # (the archive records the file's own name: the same name in two folders)
    _run([*DATA, "--metrics-file", "a.jsonl"], tmp_path / "a")
    _run([*DATA, "--accum-steps", "1"], tmp_path / "b")
    assert (tmp_path / "a" / "origin_checkpoint.pt").read_bytes() == (tmp_path / "b" / "origin_checkpoint.pt").read_bytes()
    row = json.loads((tmp_path / "a" / "a.jsonl").read_text().splitlines()[0])
    assert row["updates"] == 6 and row["steps_per_rank"] == 6


@pytest.mark.slow
def test_cli_updates_column_and_torch_route(tmp_path):
    r = _run([*DATA, "--accum-steps", "2", "--lr", "0.01", "--checkpoint", "n.pt", "--metrics-file", "n.jsonl"],
             tmp_path)
    lines = [ln.split(":")[0] if ln.startswith("time elapsed") else ln.split(" is ")[0]
             for ln in r.stdout.splitlines() if ln.strip()]
    assert lines == ["begin training of epoch 1/1", "begin testing", "Accuracy", "time elapsed"], r.stdout
    row = json.loads((tmp_path / "n.jsonl").read_text().splitlines()[0])
    assert row["updates"] == 3 and row["steps_per_rank"] == 6
    _run([*DATA, "--accum-steps", "2", "--lr", "0.01", "--impl", "torch", "--checkpoint", "t.pt", "--metrics-file",
          "t.jsonl"], tmp_path)
    assert json.loads((tmp_path / "t.jsonl").read_text().splitlines()[0])["updates"] == 3
    a = torch.load(tmp_path / "n.pt", weights_only=True)
    b = torch.load(tmp_path / "t.pt", weights_only=True)
    assert list(a) == list(b) and list(a["model"]) == list(b["model"])
    # CPU, fp32, K = 2 (a power of two), same data and order: the two routes are the same arithmetic
    for k, v in a["model"].items():
        assert torch.equal(v, b["model"][k]), k
    base = torch.load(tmp_path / "n.pt", weights_only=True)["model"]
    _run([*DATA, "--lr", "0.01", "--checkpoint", "one.pt"], tmp_path)
    one = torch.load(tmp_path / "one.pt", weights_only=True)["model"]
    assert not torch.equal(base["fc.weight"], one["fc.weight"])  # and it is not the K = 1 run


@pytest.mark.slow
def test_cli_cosine_and_resume_count_updates(tmp_path):
    sched = ["--accum-steps", "2", "--lr", "0.01", "--lr-schedule", "cosine", "--warmup-steps", "2"]
    _run([*DATA, *sched, "--checkpoint", "a.pt", "--metrics-file", "a.jsonl"], tmp_path)
    ck = torch.load(tmp_path / "a.pt", weights_only=True)
    assert ck["lr_scheduler"]["pos"] == 3  # one epoch: 3 updates, not 6 batches
    _run([*DATA, *sched, "--resume", "a.pt", "--start-epoch", "1", "--checkpoint", "b.pt", "--metrics-file",
          "b.jsonl"], tmp_path)
    ck2 = torch.load(tmp_path / "b.pt", weights_only=True)
    assert ck2["lr_scheduler"]["pos"] == 6
    # the cosine over (1 + 1) * 3 updates ends at its last position: rate ~ 0 after the 6th update
    row = json.loads((tmp_path / "b.jsonl").read_text().splitlines()[0])
    assert row["updates"] == 3 and row["lr"] < 0.01 * 0.1
    # resumed without the file's position: start_epoch * updates-per-epoch
    ck.pop("lr_scheduler")
    torch.save(ck, tmp_path / "nopos.pt")
    _run([*DATA, *sched, "--resume", "nopos.pt", "--start-epoch", "1", "--checkpoint", "c.pt"], tmp_path)
    assert torch.load(tmp_path / "c.pt", weights_only=True)["lr_scheduler"]["pos"] == 6


# ------------------------------------------------------------------ DDP (gloo, 2 ranks)
@pytest.mark.slow
@pytest.mark.parametrize("bucket_view", [True, False], ids=["defer", "no_sync"])
def test_ddp_syncbn_window_matches_single_process(bucket_view):
    outs = run(W.ddp_syncbn_accum, world=2, args=(4, 2, bucket_view))
    assert len(outs[0]) == 10 and outs[0] == outs[1]  # the ranks hold identical parameters
