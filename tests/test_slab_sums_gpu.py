"""Every implementation of the slab column sum, on integer-valued slabs against int64 sums:

  a  C.convblock.slab_reduce            slab_colsum<16> (csrc/common.h), one and two slabs
  b  the slab source of C.optim.amp_sgd_fused (csrc/kernels/amp_step.h SlabSrc): bitwise the
     result of slab_reduce followed by unscale_check + sgd_step + update_scale

(slab_colsum_chunks<4, 2> / <4, 16>, the third one, is reached through conv1_wgrad_slab2:
tests/test_conv1_wgrad_gpu.py::test_out2_column_sums.)

slab_colsum loads a fixed batch of 16 clamped rows per lane (16 row groups: 256 rows) and
masks the surplus, then walks a tail loop: rows = 16 | 17 (a second row for group 0),
256 | 257 (the tail loop starts), 259, 300; n = 15, 16, 17 (the column clamp of a workgroup's 16
columns), 1, 416 and 12832 (the ConvNet's slabs).  Outputs are views between NaN guards.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
GUARD = 8
NS = (1, 15, 16, 17, 416, 12832)
ROWS = (1, 7, 16, 17, 224, 256, 257, 259, 300)


def _view(n):
    buf = torch.full((n + 2 * GUARD,), NAN, device=DEV)
    return buf, buf.narrow(0, GUARD, n)


def _check(buf, want, name):
    out = buf.cpu()
    assert bool(torch.isnan(out[:GUARD]).all()) and bool(torch.isnan(out[-GUARD:]).all()), f"{name}: guard overwritten"
    got = out[GUARD:-GUARD].double()
    bad = got != want.double()
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} of {bad.numel()} columns differ, first {bad.nonzero()[0].item()}: "
                                 f"got {got[bad][0].item()} want {want[bad][0].item()}")


# =============================================================================== a
@pytest.mark.parametrize("n", NS)
def test_slab_reduce_exact(C, n):
    """One slab, then as the second slab behind a first whose n1 = 17 is no multiple of 16 (the
    second slab's workgroups start after a clamped one), then as the first with that one second."""
    sr = C.convblock.slab_reduce
    g = torch.Generator().manual_seed(n)
    big = torch.randint(-8, 9, (max(ROWS), n), generator=g)
    other = torch.randint(-8, 9, (7, 17), generator=g)
    assert int(big.abs().sum(0).max()) < 2 ** 24
    big_d, other_d = big.float().to(DEV), other.float().to(DEV).reshape(-1)
    for rows in ROWS:
        slab, want = big_d[:rows].reshape(-1), big[:rows].sum(0)
        buf, out = _view(n)
        sr(slab, n, out)
        torch.cuda.synchronize()
        _check(buf, want, f"n {n} rows {rows}")
        for first in (False, True):
            buf, out = _view(n)
            buf2, out2 = _view(17)
            if first:
                sr(slab, n, out, other_d, 17, out2)
            else:
                sr(other_d, 17, out2, slab, n, out)
            torch.cuda.synchronize()
            _check(buf, want, f"n {n} rows {rows} as slab {1 if first else 2}")
            _check(buf2, other.sum(0), f"n {n} rows {rows}: the other slab")


# =============================================================================== b
SIZES = (7, 3000, 33)  # the ordinary tensors next to the slab's 400 + 16
LR, WD = 0.05, 1e-4


def _state(rows, scale, inf_col=None):
    """Initial tensors of one step (CPU): params, momentum buffers, the ordinary (scaled) gradients,
    the integer slab [rows][416]."""
    g = torch.Generator().manual_seed(rows)
    sizes = (400, 16) + SIZES
    ps = [torch.randn(n, generator=g) for n in sizes]
    bs = [torch.randn(n, generator=g) for n in sizes]
    gs = [torch.randint(-64, 65, (n,), generator=g).float() * (scale or 1.0) / 16 for n in SIZES]
    slab = torch.randint(-8, 9, (rows, 416), generator=g).float()
    if inf_col is not None:  # finite rows, a column that sums to +inf
        slab[0, inf_col] = slab[rows - 1, inf_col] = 3.0e38
    return ps, bs, gs, slab


class _Step:
    """Device copies of a state and the two ways to step them."""

    def __init__(self, C, st, scale):
        self.C = C
        ps, bs, gs, slab = st
        self.p = [t.to(DEV) for t in ps]
        self.b = [t.to(DEV) for t in bs]
        self.gout = torch.full((416,), NAN, device=DEV)  # the slab's gradient region: 400 + 16
        self.g = [self.gout.narrow(0, 0, 400), self.gout.narrow(0, 400, 16)] + [t.to(DEV) for t in gs]
        self.slab = slab.to(DEV).reshape(-1)
        self.amp = scale is not None
        self.scale = torch.tensor([scale or 1.0], device=DEV)
        self.tracker = torch.tensor([1], dtype=torch.int32, device=DEV)
        self.found = torch.zeros(1, device=DEV)
        self.sync = torch.zeros(4, dtype=torch.int64, device=DEV)
        self.init = [t.clone() for t in self.tensors()]

    def tensors(self):
        return self.p + self.b + [self.gout] + self.g[2:] + [self.scale, self.tracker, self.found]

    def reset(self):
        for t, s in zip(self.tensors(), self.init):
            t.copy_(s)

    def fused(self, momentum, first):
        a = (self.scale, self.tracker, self.found) if self.amp else (None, None, None)
        self.C.optim.amp_sgd_fused(self.p, self.g, self.b, LR, momentum, 0.0, WD, False, False, [int(first)] * len(self.p),
                                   *a, 2.0, 0.5, 2, self.sync, None, slab=self.slab, slab_out=self.gout)

    def unfused(self, momentum, first):
        o = self.C.optim
        self.C.convblock.slab_reduce(self.slab, 416, self.gout)
        if self.amp:
            o.unscale_check(self.g, self.scale, self.found)
        o.sgd_step(self.p, self.g, self.b, LR, momentum, 0.0, WD, False, False, [int(first)] * len(self.p),
                   self.found if self.amp else None, None)
        if self.amp:
            o.update_scale(self.scale, self.tracker, self.found, 2.0, 0.5, 2)


def _equal(a, b, what):
    for i, (x, y) in enumerate(zip(a.tensors(), b.tensors())):
        same = (x == y) | (x.isnan() & y.isnan()) if x.is_floating_point() else x == y
        assert bool(same.all()), f"{what}: tensor {i} differs at {(~same).nonzero()[:4].flatten().tolist()}"


def _compare(C, rows, scale, inf_col=None):
    st = _state(rows, scale, inf_col)
    a, b = _Step(C, st, scale), _Step(C, st, scale)
    for momentum in (0.0, 0.9):
        for first in (True, False):
            tag = f"rows {rows} scale {scale} momentum {momentum} first {first}"
            a.reset()
            b.reset()
            a.fused(momentum, first)
            b.unfused(momentum, first)
            torch.cuda.synchronize()
            _equal(a, b, tag + " eager")
            graph = torch.cuda.CUDAGraph()
            a.reset()
            with torch.cuda.graph(graph):
                a.fused(momentum, first)
            a.reset()
            graph.replay()
            torch.cuda.synchronize()
            _equal(a, b, tag + " replay")
            yield a, st


@pytest.mark.parametrize("scale", [None, 1.0, 1024.0], ids=["plain", "scale1", "scale1024"])
@pytest.mark.parametrize("rows", [7, 224, 257, 259])
def test_amp_sgd_slab_source_bitwise(C, rows, scale):
    """Params, buffers, the (unscaled) gradients -- the slab's column sums written to slab_out
    among them --, scale, tracker and found_inf after the fused launch == after slab_reduce and the
    unfused kernels, bit for bit; eagerly and replayed from a graph."""
    for a, st in _compare(C, rows, scale):
        want = st[3].double().sum(0) / (scale or 1.0)  # integers over a power of two: exact
        assert torch.equal(a.gout.double().cpu(), want)
        assert int(a.sync[3]) == 0


@pytest.mark.parametrize("rows", [7, 259])
def test_amp_sgd_slab_column_overflow_skips(C, rows):
    """A slab column that sums to inf from finite rows: the step is skipped (parameters and
    buffers untouched), the scale backs off, as the unfused kernels do."""
    for a, st in _compare(C, rows, 1024.0, inf_col=401):
        ps, bs = st[0], st[1]
        assert bool(torch.isinf(a.gout[401])) and bool(torch.isfinite(a.slab).all())
        for x, y in zip(a.p + a.b, ps + bs):
            assert torch.equal(x.cpu(), y)
        assert a.scale.item() == 512.0 and a.tracker.item() == 0 and a.found.item() == 0.0
