"""``origin_main.py --ema-decay`` on the GPU: optim.EMA updated inside the graph-replayed step
against the same program on torch's stack (``--impl torch``: torch's ``AveragedModel``, eager) on
identical synthetic data, within the margin tests/test_cli_gpu.py allows between the two routes;
the checkpoint's "ema" entry, ``--resume`` continuing ``n_averaged``, and the default run unchanged."""
import json
import os
import re

import pytest
import torch

from .test_cli_cpu import REF_KEYS, _check_stdout
from .test_cli_gpu import _acc, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
EMA_KEYS = ["n_averaged"] + ["module." + k for k in REF_KEYS]


def _ema_acc(out):
    m = re.findall(r"^EMA accuracy is ([0-9.]+)%$", out, flags=re.M)
    assert len(m) == 1, out
    return float(m[0])


def test_ema_accuracy_parity_with_torch_checkpoint_and_resume(C, tmp_path):
    args = [os.path.join(ROOT, "origin_main.py"), "--gpu", "0", "--synthetic", "--seed", "0", "-e", "1",
            "--train-samples", "8192", "--test-samples", "2048", "--optimizer", "adamw", "--lr", "1e-3",
            "--ema-decay", "0.9"]
    (tmp_path / "n").mkdir()
    (tmp_path / "t").mkdir()
    out = _run(args + ["--metrics-file", str(tmp_path / "n.jsonl")], tmp_path / "n")
    _check_stdout(out, 1)
    lines = [ln for ln in out.splitlines() if ln.strip()]
    i = [k for k, ln in enumerate(lines) if ln.startswith("Accuracy is ")][0]
    assert lines[i + 1].startswith("EMA accuracy is ")
    e_native = _ema_acc(out)
    out_t = _run(args + ["--impl", "torch"], tmp_path / "t")
    e_torch = _ema_acc(out_t)
    print(f"adamw, ema 0.9: native {_acc(out):.2f}% ema {e_native:.2f}%; torch {_acc(out_t):.2f}% ema {e_torch:.2f}%")
    assert abs(e_native - e_torch) <= 1.0, (e_native, e_torch)
    assert abs(_acc(out) - _acc(out_t)) <= 1.0
    ck = torch.load(tmp_path / "n" / "origin_checkpoint.pt", weights_only=True)
    assert list(ck) == ["model", "ema", "optimizer"] and list(ck["ema"]) == EMA_KEYS
    assert int(ck["ema"]["n_averaged"]) == 256  # 8192 / 32, every one replayed from the step graph
    assert int(ck["ema"]["module.layer1.1.num_batches_tracked"]) == 256
    assert not torch.equal(ck["ema"]["module.fc.weight"], ck["model"]["fc.weight"])
    assert json.loads((tmp_path / "n.jsonl").read_text().splitlines()[0])["ema_updates"] == 256
    ck_t = torch.load(tmp_path / "t" / "origin_checkpoint.pt", weights_only=True)
    assert list(ck_t["ema"]) == EMA_KEYS and int(ck_t["ema"]["n_averaged"]) == 256

    out = _run(args + ["--resume", str(tmp_path / "n" / "origin_checkpoint.pt"), "--start-epoch", "1",
                       "--train-samples", "1024", "--test-samples", "256", "--checkpoint", "b.pt"], tmp_path / "n")
    assert int(torch.load(tmp_path / "n" / "b.pt", weights_only=True)["ema"]["n_averaged"]) == 256 + 32


def test_default_run_is_unchanged_on_the_gpu(C, tmp_path):
    out = _run([os.path.join(ROOT, "origin_main.py"), "--gpu", "0", "--synthetic", "--seed", "0", "-e", "1",
                "--train-samples", "1024", "--test-samples", "256"], tmp_path)
    _check_stdout(out, 1)
    assert "EMA" not in out
    ck = torch.load(tmp_path / "origin_checkpoint.pt", weights_only=True)
    assert list(ck) == ["model"] and list(ck["model"]) == REF_KEYS
