"""The row rule of the conv2 data gradient's BN1 partial sums (csrc/kernels/conv5x5.h BwdEpi),
written once in Python for tests/test_dgrad_rows_layout_cpu.py and test_dgrad_rows_gpu.py.

An image of H x W output pixels is MT = ceil(H W / 16) m-tiles of 16 pixels.  A launch runs
`nsplit` workgroups per image, workgroup sp the m-tiles [MT sp / nsplit, MT (sp + 1) / nsplit),
and wave wv of its NW = 4 waves the m-tiles mt0 + wv, mt0 + wv + NW, ...  The slab has one row
per image QUARTER whatever nsplit is: quarter k is the m-tiles [MT k / 4, MT (k + 1) / 4), and
within it the m-tile mt has slot mt - quarter start.  A row is the slots' partials in slot order.
"""
import torch

H, W, MT, NW, QUARTERS = 14, 14, 13, 4, 4


def split_range(sp, nsplit, mt=MT):
    """The m-tiles [mt0, mt1) of workgroup sp of nsplit."""
    return mt * sp // nsplit, mt * (sp + 1) // nsplit


def quarter_range(k, mt=MT):
    return split_range(k, QUARTERS, mt)


def place(tile, mt=MT):
    """(quarter, slot) of an m-tile."""
    for k in range(QUARTERS):
        lo, hi = quarter_range(k, mt)
        if lo <= tile < hi:
            return k, tile - lo
    raise ValueError(tile)


def wave_tiles(sp, nsplit, wv, mt=MT):
    """The m-tiles wave wv of workgroup sp computes."""
    lo, hi = split_range(sp, nsplit, mt)
    return list(range(lo + wv, hi, NW))


def quarters_of(sp, nsplit):
    """The quarters a workgroup writes the rows of: QUARTERS / nsplit consecutive ones."""
    n = QUARTERS // nsplit
    return list(range(sp * n, sp * n + n))


def quarter_pixels(k, hw=H * W, mt=MT):
    """The output pixels [p0, p1) of quarter k (the last m-tile is clipped at the image)."""
    lo, hi = quarter_range(k, mt)
    return 16 * lo, min(16 * hi, hw)


def quarter_rows(g, xh):
    """Exact rows [4 B][S1(C) | S2(C)] of a full-resolution gradient g and xhat, [B][C][H][W]
    float64: per quarter, S1 = sum g and S2 = sum g * xhat over the quarter's pixels."""
    Bn, C = g.shape[:2]
    gf, pf = g.reshape(Bn, C, -1), (g * xh).reshape(Bn, C, -1)
    rows = torch.empty(Bn, QUARTERS, 2 * C, dtype=g.dtype)
    for k in range(QUARTERS):
        p0, p1 = quarter_pixels(k, gf.shape[-1])
        rows[:, k, :C] = gf[:, :, p0:p1].sum(-1)
        rows[:, k, C:] = pf[:, :, p0:p1].sum(-1)
    return rows.reshape(Bn * QUARTERS, 2 * C)
