"""The batch gather that starts every step (csrc/kernels/data.hip gather) against
tests/_sgd_ref.py ``gather``: every element of the batch and every label compared exactly.

With shift == 0 the one correctly rounded product is required; with a normalising scale / shift
either of the reference's two candidates (one fma, or the product rounded and then the sum) is
accepted, the contraction being the compiler's choice.  Shapes take both pixel loops
(npix % 4 == 0 and not), one pixel, and the grid-stride over images (B > 1024); the step comes
from the argument, from the device counter (eager and graph-replayed), and from past the end of
the order list (the kernel's clamp).
"""
import pytest
import torch

from . import _sgd_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
IDS = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}
DT = pytest.mark.parametrize("dtype", list(IDS), ids=list(IDS.values()))
PLAIN = (1 / 255.0, 0.0)
NORMALISED = (1 / (255 * 0.3081), -0.1307 / 0.3081)
SHAPES = [(784, 1), (784, 5), (30, 1), (30, 5), (9, 1), (9, 5), (9, 1025), (1, 1), (1, 5)]
NIMG = 67


def _set(npix, L, seed):
    g = torch.Generator().manual_seed(seed)
    imgs = torch.randint(0, 256, (NIMG, npix), dtype=torch.uint8, generator=g)
    imgs[0, 0], imgs[1, -1] = 0, 255
    labels = torch.randint(0, 10, (NIMG,), generator=g)
    order = torch.randint(0, NIMG, (L,), generator=g)
    return imgs, labels, order


def _out(B, npix, dtype):
    return (torch.full((B, npix), float("nan"), dtype=dtype, device=DEV),
            torch.full((B,), -1, dtype=torch.long, device=DEV))


def _check(out, lab, cands, want_lab, what):
    got = out.cpu()
    ok = torch.zeros_like(got, dtype=torch.bool)
    for c in cands:
        ok |= got == c  # NaN (an unwritten element) equals nothing
    if not bool(ok.all()):
        i, j = (~ok).nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} differ, first at image {i} pixel {j}: got "
                             f"{got[i, j].item()!r} want {' or '.join(repr(c[i, j].item()) for c in cands)}")
    bad = lab.cpu() != want_lab
    assert not bool(bad.any()), f"{what}: label of image {int(bad.nonzero()[0])} differs"


@pytest.mark.parametrize("scale,shift", [PLAIN, NORMALISED], ids=["plain", "normalised"])
@DT
@pytest.mark.parametrize("npix,B", SHAPES)
def test_gather_fixed_step(C, npix, B, dtype, scale, shift):
    """A fixed step >= 0 reads its batch and leaves the counter alone."""
    imgs, labels, order = _set(npix, 3 * B + 2, npix + B)
    ctr = torch.tensor([7, 0], dtype=torch.int32, device=DEV)
    out, lab = _out(B, npix, dtype)
    C.data.gather(imgs.to(DEV), labels.to(DEV), order.to(DEV), ctr, 2, out, lab, scale, shift)
    torch.cuda.synchronize()
    cands, want_lab = R.gather(imgs, labels, order, 2, B, scale, shift, dtype)
    assert len(cands) == (1 if shift == 0 else 2)
    _check(out, lab, cands, want_lab, "step 2")
    assert ctr.tolist() == [7, 0]


@pytest.mark.parametrize("scale,shift", [PLAIN, NORMALISED], ids=["plain", "normalised"])
@DT
@pytest.mark.parametrize("npix,B", [(784, 5), (30, 5), (9, 1025)])
def test_gather_device_counter_eager_and_replayed(C, npix, B, dtype, scale, shift):
    """Three launches, then three replays of one captured launch: the batches follow the order
    list and the counter ends at [6, 0]."""
    imgs, labels, order = _set(npix, 6 * B, 3 * npix + B)
    di, dl, do = imgs.to(DEV), labels.to(DEV), order.to(DEV)
    ctr = torch.zeros(2, dtype=torch.int32, device=DEV)
    out, lab = _out(B, npix, dtype)
    launch = lambda: C.data.gather(di, dl, do, ctr, -1, out, lab, scale, shift)
    graph = None
    for step in range(6):
        out.fill_(float("nan"))
        lab.fill_(-1)
        if step < 3:
            launch()
        else:
            if graph is None:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    launch()
            graph.replay()
        torch.cuda.synchronize()
        cands, want_lab = R.gather(imgs, labels, order, step, B, scale, shift, dtype)
        _check(out, lab, cands, want_lab, f"step {step}")
        assert ctr.tolist() == [step + 1, 0]
    assert ctr.tolist() == [6, 0]


@DT
def test_gather_positions_past_the_order_list_repeat_the_last_index(C, dtype):
    B, npix = 5, 30
    imgs, labels, order = _set(npix, 2 * B + 2, 99)
    ctr = torch.tensor([2, 0], dtype=torch.int32, device=DEV)
    for step in (2, -1):  # positions 10 .. 14 of 12: the last three clamp to 11
        out, lab = _out(B, npix, dtype)
        C.data.gather(imgs.to(DEV), labels.to(DEV), order.to(DEV), ctr, step, out, lab, *NORMALISED)
        torch.cuda.synchronize()
        cands, want_lab = R.gather(imgs, labels, order, 2, B, *NORMALISED, dtype)
        _check(out, lab, cands, want_lab, f"step {step}")
        assert bool((want_lab[2:] == labels[order[-1]]).all())
    assert ctr.tolist() == [3, 0]
