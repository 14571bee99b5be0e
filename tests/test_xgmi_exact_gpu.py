"""The xGMI communication engine bit for bit against tests/_xgmi_ref.py (checked on the CPU by
test_xgmi_ref_cpu.py), with W processes sharing the one GPU (tests/_xgmi_exact_worker.py):

  one-shot   all_reduce: 13 sizes around the lane (8) and workgroup (2048) edges x f32 / bf16 / f16
             x sum / avg / max / min, each in and out of place; SPECIALS (+-0, subnormals, the largest
             normal, +-inf, NaN, overflowing sums) on one rank at the first element, the last
             element of a full lane and the last element
  two-shot   all_reduce_twoshot on a grid of 2: shard edges, an empty and a one-element last
             shard, three chunks per shard, the region's maximum, every dtype and op, sizes
             interleaved; XgmiCollective's routing (one-shot / two-shot / chunked one-shot
             launches, counted from the engine's own issue counters)
  sites      site_probe (two site ids in turn, grids of 1 / 3 / 4, every workgroup's row) and
             wide_probe (1 .. 64 finishers, the count changing from call to call)
  graph      world 2: one single-stream capture of a one-shot, a two-shot and a site exchange,
             replayed four times with fresh inputs
  sgd        amp_sgd_fused(..., xc=x): the DDP gradient average inside the fused AMP/SGD step
             against _sgd_ref.amp_step on the rank-ordered fp32 average -- bitwise on dyadic data
             (W = 2), within _sgd_ref's counted bound on normals, one non-finite value on one
             rank, an overflowing average of finite values, the pre-checked mode's NaN poison,
             the plain mode, the slab source

The contract checked: rank-ordered fp32 accumulation, one multiply by fp32 1/W, one rounding to
the storage type, the same bits on every rank (each rank compares with the reference, and the
parent compares the ranks' bytes).  Every output sits between sentinel guards that are compared
after each call; data is fresh per call and one size per mode is issued three times in a row, so
a granule left over from the call two before (the same parity) gives a wrong value.

In the pre-checked mode a flagged rank pushes NaN in place of its values; the gradients its peers
store in that skipped step are the poisoned averages, left unspecified here and not compared.
The fused step's slab source is bitwise the pre-summed step at W = 2 and 3; that step itself is
bitwise _sgd_ref's at W = 2 only, where the average (by 1/2) is exact.
"""
import pytest

from ._dist import launch
from .conftest import W8

pytestmark = pytest.mark.gpu

TIMEOUT = {"oneshot": 150, "twoshot": 150, "sites": 120, "graph": 120, "sgd": 150}


def _run(world, mode):
    from ._xgmi_exact_worker import worker

    res = launch(worker, world, (mode,), TIMEOUT[mode] * (1 if world <= 4 else 2))
    keys = set(res[0]["out"])
    for r in range(1, world):
        assert set(res[r]["out"]) == keys and res[r]["calls"] == res[0]["calls"]
        for k in sorted(keys):
            assert res[r]["out"][k] == res[0]["out"][k], f"rank {r} differs from rank 0 on {k}"
        assert res[r]["count"] == res[0]["count"]
    print(f"{mode} W={world}: {res[0]['calls']} calls, compared per rank {res[0]['count']}, "
          f"{max(r['seconds'] for r in res):.1f} s in the workers")
    return res


@pytest.mark.parametrize("world", [2, 3, 4, pytest.param(8, marks=W8)])
def test_oneshot_bitwise(C, world):
    res = _run(world, "oneshot")
    assert res[0]["count"]["oneshot"] > 0 and res[0]["count"]["oneshot specials"] > 0


@pytest.mark.parametrize("world", [2, 3, 4, pytest.param(8, marks=W8)])
def test_twoshot_and_routing_bitwise(C, world):
    res = _run(world, "twoshot")
    assert res[0]["count"]["twoshot"] > 0 and res[0]["count"]["routing"] > 0


@pytest.mark.parametrize("world", [2, 3, pytest.param(8, marks=W8)])
def test_sites_bitwise(C, world):
    res = _run(world, "sites")
    assert res[0]["count"]["site"] > 0 and res[0]["count"]["wide"] > 0


def test_graph_replay_bitwise(C):
    res = _run(2, "graph")
    assert res[0]["count"]["graph"] > 0


@pytest.mark.parametrize("world", [2, 3])
def test_fused_step_with_gradient_exchange(C, world):
    res = _run(world, "sgd")
    worst = max((v for r in res for v in r["extra"].values()), default=(0.0, ""))
    print(f"amp_sgd_fused (xgmi) W={world}: largest error / bound = {worst[0]:.3g} ({worst[1]})")
    assert 0.0 < worst[0] <= 1.0
