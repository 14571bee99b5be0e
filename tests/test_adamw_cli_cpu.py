"""``--optimizer adamw`` through origin_main.py on the CPU: the checkpoint's "optimizer" entry in
torch's layout, ``--resume`` continuing the step count, the default run's checkpoint unchanged,
and the flag errors."""
import os
import subprocess
import sys

import pytest
import torch

from .test_cli_cpu import REF_KEYS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.slow
MAIN = os.path.join(ROOT, "origin_main.py")
DATA = ["--synthetic", "--train-samples", "96", "--test-samples", "32", "--seed", "0", "-e", "1"]  # 3 steps of 32


def _run(args, cwd, ok=True):
    env = dict(os.environ)
    env.pop("CUDA_VISIBLE_DEVICES", None)
    r = subprocess.run([sys.executable, MAIN, *args], cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r


def test_adamw_checkpoint_and_resume(tmp_path):
    metrics = tmp_path / "m.jsonl"
    _run([*DATA, "--optimizer", "adamw", "--lr", "1e-3", "--weight-decay", "0.01", "--checkpoint", "a.pt",
          "--metrics-file", str(metrics)], tmp_path)
    ck = torch.load(tmp_path / "a.pt", weights_only=True)
    assert list(ck) == ["model", "optimizer"] and list(ck["model"]) == REF_KEYS
    osd = ck["optimizer"]
    assert len(osd["state"]) == 10 and all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in osd["state"].values())
    assert all(float(st["step"]) == 3.0 for st in osd["state"].values())
    g = osd["param_groups"][0]
    assert g["lr"] == 1e-3 and g["betas"] == (0.9, 0.999) and g["weight_decay"] == 0.01
    assert g["decoupled_weight_decay"] is True
    assert metrics.read_text().count("\n") == 1 and '"lr": 0.001' in metrics.read_text()
    # the file's optimizer entry is torch.optim.AdamW's
    from ddp_practice_amd.models import ConvNet

    m = ConvNet(fused=False)
    m.load_state_dict(ck["model"])
    t = torch.optim.AdamW(m.parameters(), lr=1e-3)
    t.load_state_dict(osd)
    assert float(t.state[next(m.parameters())]["step"]) == 3.0

    _run([*DATA, "--optimizer", "adamw", "--lr", "1e-3", "--weight-decay", "0.01", "--resume", "a.pt",
          "--start-epoch", "1", "--checkpoint", "b.pt"], tmp_path)
    ck2 = torch.load(tmp_path / "b.pt", weights_only=True)
    assert all(float(st["step"]) == 6.0 for st in ck2["optimizer"]["state"].values())
    assert not torch.equal(ck2["optimizer"]["state"][0]["exp_avg"], osd["state"][0]["exp_avg"])

    # the same program on torch's optimizer writes the same layout
    _run([*DATA, "--optimizer", "adam", "--betas", "0.8,0.99", "--adam-eps", "1e-6", "--impl", "torch",
          "--checkpoint", "t.pt"], tmp_path)
    ck3 = torch.load(tmp_path / "t.pt", weights_only=True)
    g3 = ck3["optimizer"]["param_groups"][0]
    assert tuple(g3["betas"]) == (0.8, 0.99) and g3["eps"] == 1e-6 and not g3.get("decoupled_weight_decay", False)
    assert all(float(st["step"]) == 3.0 for st in ck3["optimizer"]["state"].values())

    # an SGD momentum state does not resume into AdamW, nor the reverse: named, not a KeyError
    _run([*DATA, "--momentum", "0.9", "--checkpoint", "s.pt"], tmp_path)
    r = _run([*DATA, "--optimizer", "adamw", "--resume", "s.pt"], tmp_path, ok=False)
    assert "SGD optimizer state" in r.stderr and "KeyError" not in r.stderr
    r = _run([*DATA, "--momentum", "0.9", "--resume", "a.pt"], tmp_path, ok=False)
    assert "Adam optimizer state" in r.stderr and "KeyError" not in r.stderr


def test_default_run_checkpoint_is_unchanged(tmp_path):
    _run([*DATA], tmp_path)
    ck = torch.load(tmp_path / "origin_checkpoint.pt", weights_only=True)
    assert list(ck) == ["model"] and list(ck["model"]) == REF_KEYS


def test_momentum_with_adamw_is_an_error(tmp_path):
    r = _run([*DATA, "--momentum", "0.9", "--optimizer", "adamw"], tmp_path, ok=False)
    assert "--momentum" in r.stderr and not (tmp_path / "origin_checkpoint.pt").exists()
    r = _run([*DATA, "--optimizer", "adamw", "--betas", "0.9"], tmp_path, ok=False)
    assert "--betas" in r.stderr
