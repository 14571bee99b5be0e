"""``origin_main.py --accum-steps 2`` on the GPU: the native windows (graph-replayed) against the
same program on torch's stack (``--impl torch``: the textbook idiom, eager) on identical synthetic
data, within the margin tests/test_cli_gpu.py allows between the two routes, and the ``updates``
column of the metrics file."""
import json
import os

import pytest
import torch

from .test_cli_cpu import REF_KEYS, _check_stdout
from .test_cli_gpu import _acc, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_accum_accuracy_parity_with_torch_and_updates_column(C, tmp_path):
    # 8200 samples: 256 full batches of 32 and a tail of 8 -> 128 whole windows and a short one
    args = [os.path.join(ROOT, "origin_main.py"), "--gpu", "0", "--synthetic", "--seed", "0", "-e", "1",
            "--train-samples", "8200", "--test-samples", "2048", "--optimizer", "adamw", "--lr", "2e-3",
            "--accum-steps", "2"]
    (tmp_path / "n").mkdir()
    (tmp_path / "t").mkdir()
    out = _run(args + ["--metrics-file", str(tmp_path / "n.jsonl")], tmp_path / "n")
    _check_stdout(out, 1)
    out_t = _run(args + ["--impl", "torch", "--metrics-file", str(tmp_path / "t.jsonl")], tmp_path / "t")
    print(f"adamw, accum 2: native {_acc(out):.2f}%; torch {_acc(out_t):.2f}%")
    assert abs(_acc(out) - _acc(out_t)) <= 1.0
    assert _acc(out) > 30.0  # it trained (chance: 10%)
    for name in ("n", "t"):
        row = json.loads((tmp_path / f"{name}.jsonl").read_text().splitlines()[0])
        assert row["updates"] == 129 and row["steps_per_rank"] == 257, row
    ck = torch.load(tmp_path / "n" / "origin_checkpoint.pt", weights_only=True)
    assert list(ck["model"]) == REF_KEYS
    assert int(ck["model"]["layer1.1.num_batches_tracked"]) == 257  # every micro-batch went through the model
