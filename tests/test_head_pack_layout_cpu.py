"""tests/_head_pack.py pack_layout (the reference layout of the head's packed fc weights used by
tests/test_head_packed_gpu.py) against a plain loop over (lane, class, element)."""
import pytest
import torch

from . import _head_pack as P


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("N", [1, 3, 10, 11, 16])
def test_pack_layout_matches_loop(N, dtype):
    g = torch.Generator().manual_seed(N)
    wfc = torch.randn(N, P.K, generator=g)
    wfc[0, 0], wfc[N - 1, P.K - 1] = -0.0, 1.0 + 2.0 ** -8  # a negative zero, a bf16 rounding tie
    a, b = P.pack_layout(wfc, dtype), P.pack_layout_loop(wfc, dtype)
    assert a.numel() == P.LANES * P.nm_of(N) * P.G
    assert torch.equal(P.bits(a), P.bits(b))
    v = a.view(P.LANES, P.nm_of(N), P.G)
    assert not bool(v[:, :, 7].any()) and not bool(v[:, N:].any())          # element 7, classes >= N
    assert not bool(v[P.K - 6 * P.LANES:, :, 6].any())                       # features >= 1568
    assert torch.equal(P.bits(v[5, N - 1, :7]), P.bits(wfc[N - 1, 5::P.LANES][:7].to(dtype)))
