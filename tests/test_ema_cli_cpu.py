"""``--ema-decay`` through origin_main.py on the CPU: the flag errors, the extra stdout line, the
checkpoint's "ema" entry in ``AveragedModel``'s layout (loaded with ``weights_only``),
``--resume`` continuing ``n_averaged``, ``ema_updates`` in the metrics file, the ``--impl torch``
route writing the same layout, and the default run unchanged."""
import json
import os
import subprocess
import sys

import pytest
import torch

from .test_cli_cpu import REF_KEYS, _check_stdout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.slow
MAIN = os.path.join(ROOT, "origin_main.py")
DATA = ["--synthetic", "--train-samples", "96", "--test-samples", "32", "--seed", "0", "-e", "1"]  # 3 steps of 32
EMA_KEYS = ["n_averaged"] + ["module." + k for k in REF_KEYS]


def _run(args, cwd, ok=True):
    env = dict(os.environ)
    env.pop("CUDA_VISIBLE_DEVICES", None)
    r = subprocess.run([sys.executable, MAIN, *args], cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r


def _ema_acc(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("EMA accuracy is ")]
    assert len(lines) == 1 and lines[0].endswith("%"), out
    return float(lines[0][len("EMA accuracy is "):-1])


@pytest.mark.parametrize("flags,word", [
    (["--ema-decay", "1.0"], "--ema-decay"), (["--ema-decay", "-0.1"], "--ema-decay"),
    (["--ema-decay", "1.5"], "--ema-decay"), (["--ema-warmup"], "--ema-decay"), (["--ema-buffers"], "--ema-decay"),
    (["--ema-decay", "0.9", "--ema-warmup", "--impl", "torch"], "--ema-warmup")])
def test_flag_errors(tmp_path, flags, word):
    r = _run([*DATA, *flags], tmp_path, ok=False)
    assert "error:" in r.stderr and word in r.stderr and "Traceback" not in r.stderr
    assert not (tmp_path / "origin_checkpoint.pt").exists()


def test_ema_checkpoint_stdout_metrics_and_resume(tmp_path):
    metrics = tmp_path / "m.jsonl"
    r = _run([*DATA, "--ema-decay", "0.9", "--checkpoint", "a.pt", "--metrics-file", str(metrics)], tmp_path)
    _check_stdout(r.stdout, 1)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    i = [k for k, ln in enumerate(lines) if ln.startswith("Accuracy is ")][0]
    assert lines[i + 1].startswith("EMA accuracy is ")
    assert 0.0 <= _ema_acc(r.stdout) <= 100.0
    ck = torch.load(tmp_path / "a.pt", weights_only=True)
    assert list(ck) == ["model", "ema"] and list(ck["model"]) == REF_KEYS
    assert list(ck["ema"]) == EMA_KEYS
    assert ck["ema"]["n_averaged"].dtype == torch.int64 and int(ck["ema"]["n_averaged"]) == 3
    assert not torch.equal(ck["ema"]["module.fc.weight"], ck["model"]["fc.weight"])
    assert torch.equal(ck["ema"]["module.layer1.1.num_batches_tracked"], ck["model"]["layer1.1.num_batches_tracked"])
    assert json.loads(metrics.read_text().splitlines()[0])["ema_updates"] == 3
    # torch's AveragedModel of the torch model loads the entry
    from torch.optim.swa_utils import AveragedModel

    from ddp_practice_amd.models import ConvNet

    t = AveragedModel(ConvNet(fused=False))
    t.load_state_dict(ck["ema"])
    assert int(t.n_averaged) == 3

    _run([*DATA, "--ema-decay", "0.9", "--resume", "a.pt", "--start-epoch", "1", "--checkpoint", "b.pt"], tmp_path)
    ck2 = torch.load(tmp_path / "b.pt", weights_only=True)
    assert int(ck2["ema"]["n_averaged"]) == 6
    # resumed from a file without "ema": the average starts from the resumed weights at 0
    _run([*DATA, "--checkpoint", "plain.pt"], tmp_path)
    _run([*DATA, "--ema-decay", "0.9", "--ema-buffers", "--ema-warmup", "--resume", "plain.pt", "--checkpoint",
          "c.pt"], tmp_path)
    assert int(torch.load(tmp_path / "c.pt", weights_only=True)["ema"]["n_averaged"]) == 3

    # the same program on torch's AveragedModel writes the same layout and resumes ours
    r = _run([*DATA, "--ema-decay", "0.9", "--impl", "torch", "--resume", "a.pt", "--start-epoch", "1",
              "--checkpoint", "t.pt"], tmp_path)
    _ema_acc(r.stdout)
    ck3 = torch.load(tmp_path / "t.pt", weights_only=True)
    assert list(ck3["ema"]) == EMA_KEYS and int(ck3["ema"]["n_averaged"]) == 6
    # CPU, fp32, same data and order: the two routes are the same arithmetic
    for k in EMA_KEYS:
        assert torch.equal(ck3["ema"][k], ck2["ema"][k]), k


def test_default_run_is_unchanged(tmp_path):
    r = _run([*DATA], tmp_path)
    assert "EMA" not in r.stdout
    lines = [ln.split(":")[0] if ln.startswith("time elapsed") else ln.split(" is ")[0]
             for ln in r.stdout.splitlines() if ln.strip()]
    assert lines == ["begin training of epoch 1/1", "begin testing", "Accuracy", "time elapsed"], r.stdout
    ck = torch.load(tmp_path / "origin_checkpoint.pt", weights_only=True)
    assert list(ck) == ["model"] and list(ck["model"]) == REF_KEYS
