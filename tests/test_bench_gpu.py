"""bench.py contract on the MI355X: exact --steps/--warmup, the measured 3-epoch run,
the same-node torch baseline, the self-launcher with ranks sharing the one GPU, and a
clear refusal of more ranks than GPUs."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(args, timeout=110):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=timeout)
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    return r, recs


def test_bench_one_gpu_contract(C):
    r, recs = _bench(["--steps", "20", "--warmup", "5", "--full", "--baseline-steps", "30"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert len(recs) == 1
    rec = recs[0]
    assert rec["n_gpus"] == 1 and rec["steps"] == 20 and rec["warmup"] == 5 and rec["ranks_seen"] == 1
    assert rec["dtype"] == "bf16" and rec["config"]["hipgraph"] is True
    assert rec["epochs"] == 3 and rec["steps_per_rank_per_epoch"] == 1875
    assert rec["wall_3epoch_s"] > 0 and rec["accuracy"] > 0.5  # trains on the synthetic set
    assert rec["baseline_same_node_img_s"] > 0, rec.get("baseline_error")
    assert rec["vs_baseline"] == pytest.approx(rec["value"] / rec["baseline_same_node_img_s"], rel=1e-2)
    # the other precisions and the steady state, same run
    for dt in ("fp16", "fp32"):
        assert rec[f"value_{dt}"] > 0 and rec[f"ms_per_step_{dt}"] > 0, rec.get(f"error_{dt}")
    assert rec["steady_steps"] >= 1875 and rec["steady_img_s"] > 0
    assert rec["comm_error"] == ""


def test_bench_plain_run_and_dumped_outputs(C, tmp_path):
    """A plain run (no --full) is the headline alone, and --dump-outputs holds the last timed
    step's results, equal from run to run with equal arguments.

    Tolerances from the number format, not from a run.  Two runs execute the same kernels on
    the same seeded inputs; where a reduction's order could differ, a bf16 rounding (8 mantissa
    bits) may flip: logits of magnitude ~1 within a few ulps (4 * 2^-8 = 2^-6), and parameters
    that moved ~30 steps of lr 1e-4 along gradients of magnitude <= ~10 agreeing to those few
    ulps (30 * 1e-4 * 10 * 2^-6 ~ 5e-4; the running statistics are averages of O(1) values
    agreeing likewise).  The loss is the cross entropy of the dumped logits against the labels
    of the batch that the last timed step reads (step warmup + steps of the sampler's order),
    within the logits' own bf16 rounding (2^-8 * |logit| per logit, |logit| < 8: 2^-5)."""
    import numpy as np

    from ddp_practice_amd.data import DistributedSampler, synthetic

    dumps = []
    for name in ("a", "b"):
        d = tmp_path / name
        r, recs = _bench(["--steps", "20", "--warmup", "5", "--dump-outputs", str(d)])
        assert r.returncode == 0, r.stdout + r.stderr
        assert len(recs) == 1
        rec = recs[0]
        assert rec["steps"] == 20 and rec["warmup"] == 5 and rec["dtype"] == "bf16"
        assert rec["config"]["hipgraph"] is True
        assert rec["value"] > 0 and rec["ms_per_step"] == pytest.approx(32 / rec["value"] * 1e3, rel=1e-3)
        for k in ("wall_3epoch_s", "epochs", "steady_img_s", "value_fp16", "value_fp32", "baseline_ms_per_step"):
            assert k not in rec, k
        assert rec["vs_baseline"] is None and rec["comm_error"] == ""
        dumps.append({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))})
    a, b = dumps
    assert sorted(a) == sorted(b)
    assert a["logits"].shape == (32, 10) and a["loss"].size == 1 and a["loss_scale"].item() == 65536.0
    assert sum(v.size for k, v in a.items() if k.startswith("param.")) == 29034
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k in sorted(a):
        assert a[k].dtype in (np.float32, np.float64) and np.isfinite(a[k]).all(), k
        print(f"{k}: max |a - b| = {np.abs(a[k] - b[k]).max():.3e}")
    ds = synthetic(60000, seed=1, name="synthetic-MNIST-train")
    idx = DistributedSampler(ds, num_replicas=1, rank=0).indices()[24 * 32:25 * 32]
    ce = torch.nn.functional.cross_entropy(torch.from_numpy(a["logits"]), ds.labels[idx].long()).item()
    print(f"loss {a['loss'].item():.6f}, cross entropy of the dumped logits {ce:.6f}, "
          f"max |logit| {np.abs(a['logits']).max():.3f}")
    for k in sorted(a):
        atol = 2.0 ** -6 if k in ("logits", "loss") else 0.0 if "num_batches" in k or k == "loss_scale" else 5e-4
        np.testing.assert_allclose(a[k], b[k], rtol=0, atol=atol, err_msg=k)
    assert np.abs(a["logits"]).max() < 8
    assert a["loss"].item() == pytest.approx(ce, abs=2.0 ** -5)


def test_bench_shared_gpu_two_ranks(C):
    r, recs = _bench(["--gpus", "2", "--share-gpu", "--steps", "20", "--warmup", "5", "--full", "--epochs", "1"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert len(recs) == 1
    rec = recs[0]
    assert rec["n_gpus"] == 2 and rec["ranks_seen"] == 2 and rec["steps"] == 20 and rec["warmup"] == 5
    assert rec["config"]["shared_gpu"] is True and rec["config"]["sync_bn"] is True
    assert rec["steps_per_rank_per_epoch"] == 938
    assert rec["comm_error"] == "" and rec["fallback"] is None
    assert "xgmi" in rec["config"]["comm"].lower()


def test_bench_shared_gpu_site_timeout_falls_back(C):
    """Rank 1 stops entering collectives for longer than the exchange timeout at step 3:
    rank 0's in-kernel exchange times out (error word), its watchdog reports and exits, the
    supervisor kills rank 1 and re-runs both as fresh processes on the host-staged
    communicator -> one line with the measured value, ``fallback`` and the original error."""
    env = {"DPA_FAULT": "1:3:slow:6", "DPA_XGMI_TIMEOUT": "1", "DPA_BENCH_WATCHDOG": "20", "DPA_BENCH_GRACE": "3"}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        r, recs = _bench(["--gpus", "2", "--share-gpu", "--steps", "5", "--warmup", "2", "--full", "--epochs", "1",
                          "--train-samples", "2048", "--test-samples", "256", "--extra-dtypes", ""], timeout=110)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert len(recs) == 1
    rec = recs[0]
    assert rec["fallback"] == "host" and rec["value"] > 0
    assert "timeout" in rec["comm_error"] or "watchdog" in rec["comm_error"], rec["comm_error"]
    assert [a["ok"] for a in rec["attempts"]] == [False, True]


def test_bench_refuses_more_ranks_than_gpus(C):
    n = torch.cuda.device_count() + 1
    r, recs = _bench(["--gpus", str(n), "--steps", "1", "--warmup", "0"])
    assert r.returncode == 2 and not recs
    assert "GPU(s) are visible" in r.stderr
