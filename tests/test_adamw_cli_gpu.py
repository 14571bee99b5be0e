"""``origin_main.py --optimizer adamw`` on the GPU: the native optimizer under the graph-replayed
step against the same program on torch's stack (``--impl torch``: torch.optim.AdamW) on
identical synthetic data, within the margin of tests/test_cli_gpu.py's SGD parity test."""
import os

import pytest
import torch

from .test_cli_cpu import _check_stdout
from .test_cli_gpu import _acc, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_adamw_accuracy_parity_with_torch(C, tmp_path):
    args = [os.path.join(ROOT, "origin_main.py"), "--gpu", "0", "--synthetic", "--seed", "0", "-e", "1",
            "--train-samples", "8192", "--test-samples", "2048", "--optimizer", "adamw", "--lr", "1e-3"]
    (tmp_path / "n").mkdir()
    (tmp_path / "t").mkdir()
    out = _run(args, tmp_path / "n")
    _check_stdout(out, 1)
    a_native = _acc(out)
    a_torch = _acc(_run(args + ["--impl", "torch"], tmp_path / "t"))
    print(f"adamw: native {a_native:.2f}% torch {a_torch:.2f}%")
    assert abs(a_native - a_torch) <= 1.0, (a_native, a_torch)
    ck = torch.load(tmp_path / "n" / "origin_checkpoint.pt", weights_only=True)
    assert all(float(st["step"]) == 256.0 for st in ck["optimizer"]["state"].values())  # 8192 / 32, all replayed
