"""The layout of the head's packed fc weights (csrc/kernels/conv5x5.h pack_fc, read by
convnet_head.hip head_row_kernel PK), built with torch on the CPU for the tests:

    [256 lanes][NM][8] elements of the compute dtype, NM = 10 (N <= 10) or 16,
    entry [tid][n][i] = wfc[n][tid + 256 i] cast to the dtype,
    zero where n >= N, tid + 256 i >= 1568, or i = 7.

tests/test_head_pack_layout_cpu.py checks pack_layout against the plain loop below.
"""
import torch

LANES, K, G = 256, 1568, 8


def nm_of(N):
    return 16 if N > 10 else 10


def pack_layout(wfc, dtype):
    """wfc [N][1568] (fp32, CPU) -> the packed buffer [256 * NM * 8] of `dtype`."""
    N = wfc.shape[0]
    NM = nm_of(N)
    w = torch.zeros(NM, G * LANES, dtype=dtype)
    w[:N, :K] = wfc.to(dtype)
    return w.view(NM, G, LANES).permute(2, 0, 1).contiguous().view(-1)  # [n][i][tid] -> [tid][n][i]


def pack_layout_loop(wfc, dtype):
    """The same, one element at a time."""
    N = wfc.shape[0]
    NM = nm_of(N)
    wt = wfc.to(dtype)
    out = torch.zeros(LANES * NM * G, dtype=dtype)
    for tid in range(LANES):
        for n in range(N):
            for i in range(G - 1):
                k = tid + LANES * i
                if k < K:
                    out[(tid * NM + n) * G + i] = wt[n, k]
    return out


def bits(t):
    """A 16-bit float tensor as int16, for bitwise comparison (-0 and NaN payloads included)."""
    return t.contiguous().view(torch.int16)
