"""The first conv of the fused ConvNet step with the batch gather in its prologue
(csrc/kernels/conv5x5.h conv5x5_body PRO 3, convnet_fused.hip conv1_fwd_pack_gather) and the
layer-2 weight packs its launch writes (cb::pack_w2), at every batch size where the launch's
shape differs: one image (4 conv workgroups against 26,496 pack elements), odd counts, 32.

Dataset: 64 images whose pixels name the image, pixel p of image i = (7 i + p) % 256, read
through a seeded permutation.  The step counter is put at 0, at a middle step, at the last
full batch and one step past it (positions past the order's end clamp to its last entry).

Everything is compared bit for bit:
  x, lab_out     with the stand-alone gather op (csrc/kernels/data.hip) at that step;
  y1, fslab1     with conv1_fwd_pack run on that x (every B * 4 row, count column included;
                 rows past them must stay untouched);
  fstats1        its shift block is written;
  wpk_f, wpk_d   with the packs built in torch from w2, padding columns zero;
  ctr            [step + 1, 0] afterwards;
  y1             with the float64 reference.  scale = 1/2 and shift = -64 make every input a
                 multiple of 1/2 of magnitude <= 64 and the weights are +-1, the bias a small
                 integer: every partial sum is a multiple of 1/2 below 2^24 halves, exact in
                 fp32 in any order, so the stored value is ONE rounding of the float64 result
                 (tests/_conv_ref.py store(); its partial-sum limit F32_EXACT is asserted).
Two launches back to back and three launches captured in one graph and replayed twice must
read consecutive batches and advance ctr[0] by the number of launches.
"""
import functools

import pytest
import torch

from . import _conv_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, SPLIT, ROW = 64, 4, 33
SCALE, SHIFT = 0.5, -64.0
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
GUARD = 32  # slab rows behind the launch's B * SPLIT that nothing may write
SENT = -12345.0


@functools.lru_cache(maxsize=None)
def _data():
    """(imgs uint8 [N][28][28], labels, order, float64 images after ToTensor); never modified."""
    i, p = torch.arange(N).view(N, 1), torch.arange(784).view(1, 784)
    imgs = ((7 * i + p) % 256).to(torch.uint8).view(N, 28, 28)
    labels = (3 * torch.arange(N) + 1) % 10
    order = torch.randperm(N, generator=torch.Generator().manual_seed(5))
    x64 = imgs.double() * SCALE + SHIFT
    assert len({bytes(im.numpy().tobytes()) for im in imgs}) == N  # the pixels identify the image
    return imgs, labels, order, x64


@functools.lru_cache(maxsize=None)
def _weights():
    g = torch.Generator().manual_seed(11)
    w1 = R.ints((16, 1, 5, 5), (-1, 1), g)
    b1 = R.ints((16,), (-2, -1, 1, 2), g)
    shift1 = R.ints((16,), (-2, -1, 1, 2), g)
    w2 = (torch.randn(32, 16, 5, 5, generator=g) * 0.05).float()
    return w1, b1, shift1, w2


def _packs(w2, dtype):
    """The two LDS-layout packs of w2: fwd [32][424] (k = tap * 16 + ci), dgrad [16][808]
    (k = (24 - tap) * 32 + co); columns from 400 / 800 on are zero."""
    w = w2.view(32, 16, 25)
    f = torch.zeros(32, 424)
    f[:, :400] = w.permute(0, 2, 1).reshape(32, 400)
    d = torch.zeros(16, 808)
    d[:, :800] = w.flip(2).permute(1, 2, 0).reshape(16, 800)
    return f.reshape(-1).to(dtype), d.reshape(-1).to(dtype)


def _same(got, exp, what):
    got, exp = got.detach().cpu(), exp.detach().cpu()
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, exp.dtype, got.shape, exp.shape)
    if not torch.equal(got, exp):
        bad = (got != exp).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ, first at {i}: "
                             f"got {got[i].item()}, expected {exp[i].item()}")


def _y64(src):
    """float64 conv1 output of the images `src` (indices into the dataset)."""
    w1, b1, _, _ = _weights()
    x = _data()[3][src].view(-1, 1, 28, 28)
    assert 25 * float(x.abs().max()) * float(w1.abs().max()) + float(b1.abs().max()) < R.F32_EXACT
    return R.conv(x, w1, 1, 2) + b1.view(1, -1, 1, 1)


def _stored(y64, dtype):
    y32 = y64.float()
    assert torch.equal(y32.double(), y64), "not an fp32 value"
    return y32.to(dtype)


class _Run:
    """Device tensors of one (B, dtype) and the three launch forms."""

    def __init__(self, C, B, dtype):
        self.C, self.B, self.dtype = C, B, dtype
        imgs, labels, order, _ = _data()
        w1, b1, shift1, w2 = _weights()
        self.imgs, self.labels, self.order = imgs.to(DEV), labels.to(DEV), order.to(DEV)
        self.w1, self.b1, self.shift1 = w1.float().to(DEV), b1.float().to(DEV), shift1.float().to(DEV)
        self.w2 = w2.to(DEV)
        self.ctr = torch.zeros(2, dtype=torch.int32, device=DEV)

    def bufs(self):
        B, dt = self.B, self.dtype
        Z = lambda *s, **k: torch.full(s, SENT, device=DEV, **k)  # noqa: E731
        return dict(x=Z(B, 1, 28, 28, dtype=dt), lab=torch.full((B,), -1, dtype=torch.int64, device=DEV),
                    y1=Z(B, 16, 28, 28, dtype=dt), slab=Z((B * SPLIT + GUARD) * ROW), fstats=Z(49),
                    wf=Z(self.C.convnet.W2F_LEN, dtype=dt), wd=Z(self.C.convnet.W2D_LEN, dtype=dt))

    def gather_conv(self, o):
        self.C.convnet.conv1_fwd_pack_gather(o["x"], self.w1, self.b1, o["y1"], o["slab"][:self.B * SPLIT * ROW],
                                             o["fstats"], self.shift1, self.w2, o["wf"], o["wd"], self.imgs,
                                             self.labels, self.order, self.ctr, o["lab"], SCALE, SHIFT)

    def conv(self, x, o, stats=True):
        a = (o["slab"][:self.B * SPLIT * ROW], o["fstats"], self.shift1) if stats else (None, None, None)
        self.C.convnet.conv1_fwd_pack(x, self.w1, self.b1, o["y1"], *a, self.w2, o["wf"], o["wd"])

    def gather(self, step):
        """The stand-alone gather op at a fixed step."""
        x = torch.empty(self.B, 1, 28, 28, dtype=self.dtype, device=DEV)
        lab = torch.empty(self.B, dtype=torch.int64, device=DEV)
        self.C.data.gather(self.imgs, self.labels, self.order, self.ctr.clone(), step, x, lab, SCALE, SHIFT)
        return x, lab

    def check_packs(self, o, what):
        f, d = _packs(_weights()[3], self.dtype)
        _same(o["wf"], f, f"{what}: wpk_f")
        _same(o["wd"], d, f"{what}: wpk_d")

    def check_batch(self, o, step, what):
        """x / lab_out / y1 of a gather launch that ran at `step`."""
        B = self.B
        xr, labr = self.gather(step)
        _same(o["x"], xr, f"{what}: x")
        _same(o["lab"], labr, f"{what}: lab_out")
        pos = (step * B + torch.arange(B)).clamp(max=N - 1)
        src = _data()[2][pos]
        _same(o["lab"], _data()[1][src], f"{what}: lab_out against the dataset")
        _same(o["y1"], _stored(_y64(src), self.dtype), f"{what}: y1 against float64")
        return xr


def _steps(B):
    nb = N // B
    return sorted({0, nb // 2, nb - 1, nb})


@pytest.mark.parametrize("B", [1, 2, 3, 5, 32])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_conv1_gather_steps(C, B, dt):
    r = _Run(C, B, DTYPES[dt])
    rows = B * SPLIT * ROW
    for step in _steps(B):
        what = f"B={B} {dt} step={step}"
        r.ctr.copy_(torch.tensor([step, 0], dtype=torch.int32))
        o = r.bufs()
        r.gather_conv(o)
        torch.cuda.synchronize()
        _same(r.ctr, torch.tensor([step + 1, 0], dtype=torch.int32), f"{what}: ctr")
        xr = r.check_batch(o, step, what)
        ref = r.bufs()
        r.conv(xr, ref)
        torch.cuda.synchronize()
        _same(o["y1"], ref["y1"], f"{what}: y1 against conv1_fwd_pack")
        _same(o["slab"][:rows], ref["slab"][:rows], f"{what}: fslab1")
        cnt = o["slab"][:rows].view(B * SPLIT, ROW)[:, 32].cpu()
        assert cnt.view(B, SPLIT).sum(1).eq(784).all() and (cnt > 0).all(), (what, cnt)
        for t, name in ((o, "gather"), (ref, "conv1_fwd_pack")):
            assert t["slab"][rows:].eq(SENT).all(), f"{what}: {name} wrote past the B * SPLIT slab rows"
            _same(t["fstats"][33:], r.shift1, f"{what}: {name} fstats1 shift block")
            assert t["fstats"][:33].eq(SENT).all(), f"{what}: {name} wrote fstats1 sums"
            r.check_packs(t, f"{what}: {name}")
    ev = r.bufs()  # the eval form: no statistics, the same packs
    r.conv(xr, ev, stats=False)
    torch.cuda.synchronize()
    _same(ev["y1"], ref["y1"], f"B={B} {dt}: eval y1")
    assert ev["slab"].eq(SENT).all() and ev["fstats"].eq(SENT).all()
    r.check_packs(ev, f"B={B} {dt}: eval")


@pytest.mark.parametrize("dt", list(DTYPES))
def test_conv1_gather_consecutive_launches(C, dt):
    B = 3
    r = _Run(C, B, DTYPES[dt])
    r.ctr.zero_()
    two = [r.bufs(), r.bufs()]
    for o in two:  # back to back, no host synchronisation in between
        r.gather_conv(o)
    torch.cuda.synchronize()
    _same(r.ctr, torch.tensor([2, 0], dtype=torch.int32), f"{dt}: ctr after two launches")
    for step, o in enumerate(two):
        r.check_batch(o, step, f"{dt}: launch {step} of two")
    three = [r.bufs() for _ in range(3)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for o in three:
            r.gather_conv(o)
    torch.cuda.synchronize()
    _same(r.ctr, torch.tensor([2, 0], dtype=torch.int32), f"{dt}: ctr after the capture")
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        _same(r.ctr, torch.tensor([2 + 3 * (rep + 1), 0], dtype=torch.int32), f"{dt}: ctr after replay {rep}")
        for k, o in enumerate(three):
            r.check_batch(o, 2 + 3 * rep + k, f"{dt}: replay {rep} launch {k}")
            r.check_packs(o, f"{dt}: replay {rep} launch {k}")
