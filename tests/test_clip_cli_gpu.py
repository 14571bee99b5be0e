"""``origin_main.py --clip-grad-norm`` on the GPU: AdamW with the clip fused into its graph-replayed
step against the same program on torch's stack (``--impl torch``: torch.optim.AdamW after
``torch.nn.utils.clip_grad_norm_``) on identical synthetic data, within the margin of
tests/test_adamw_cli_gpu.py; and SGD through ``optim.clip_grad_norm_``, with the norm in the
metrics file."""
import json
import os

import pytest
import torch

from .test_cli_cpu import _check_stdout
from .test_cli_gpu import _acc, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_clipped_adamw_accuracy_parity_with_torch(C, tmp_path):
    args = [os.path.join(ROOT, "origin_main.py"), "--gpu", "0", "--synthetic", "--seed", "0", "-e", "1",
            "--train-samples", "8192", "--test-samples", "2048", "--optimizer", "adamw", "--lr", "1e-3",
            "--clip-grad-norm", "1.0"]
    (tmp_path / "n").mkdir()
    (tmp_path / "t").mkdir()
    out = _run(args + ["--metrics-file", str(tmp_path / "n.jsonl")], tmp_path / "n")
    _check_stdout(out, 1)
    a_native = _acc(out)
    a_torch = _acc(_run(args + ["--impl", "torch", "--metrics-file", str(tmp_path / "t.jsonl")], tmp_path / "t"))
    print(f"adamw, clip 1.0: native {a_native:.2f}% torch {a_torch:.2f}%")
    assert abs(a_native - a_torch) <= 1.0, (a_native, a_torch)
    ck = torch.load(tmp_path / "n" / "origin_checkpoint.pt", weights_only=True)
    assert all(float(st["step"]) == 256.0 for st in ck["optimizer"]["state"].values())  # 8192 / 32, all replayed
    for f in ("n.jsonl", "t.jsonl"):
        row = json.loads((tmp_path / f).read_text().splitlines()[0])
        print(f, row)
        assert row["grad_norm"] > 0.0 and row["grad_norm"] == row["grad_norm"]


def test_clipped_sgd_runs_and_reports_the_norm(C, tmp_path):
    args = [os.path.join(ROOT, "origin_main.py"), "--gpu", "0", "--synthetic", "--seed", "0", "-e", "1",
            "--train-samples", "2048", "--test-samples", "512", "--optimizer", "sgd", "--lr", "1e-2",
            "--clip-grad-norm", "1.0", "--metrics-file", str(tmp_path / "m.jsonl")]
    out = _run(args, tmp_path)
    _check_stdout(out, 1)
    row = json.loads((tmp_path / "m.jsonl").read_text().splitlines()[0])
    assert row["grad_norm"] > 0.0 and row["grad_norm"] == row["grad_norm"], row
    assert "optimizer" in torch.load(tmp_path / "origin_checkpoint.pt", weights_only=True)
