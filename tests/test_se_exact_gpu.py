"""ops/se.py on integer cases, bit for bit against float64 (tests/_se_ref.py).  W1 = W2 = 0, b2 = 0 and
b1 in {0, 1, 2} make the gate exactly 0.5 and h = b1; u, identity are integers in [-2, 2] and g is
+-1, so y (a multiple of 1/2 up to 3, with exact zeros that exercise the y > 0 rule), du = gm / 2,
d_identity = gm, ds (an integer), dz2 = ds / 4, db2, dW2 = dz2^T h and dW1 = db1 = 0 are all exactly
representable: any wrong, missing or repeated term changes a value.  665 pixels are past the 256-pixel
range of the elementwise kernels by a non-multiple."""
import pytest
import torch

from . import _se_ref as R

pytestmark = pytest.mark.gpu
SHAPES = [(2, 7, 7), (3, 13, 9), (17, 5, 5), (1, 19, 35)]
CASES = [(C, Cr, s) for C, Cr in [(64, 4), (128, 8), (256, 16)] for s in SHAPES] + [(2048, 128, (2, 7, 7))]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("C,Cr,shape", CASES, ids=[f"{C}x{Cr}-{'x'.join(map(str, s))}" for C, Cr, s in CASES])
def test_integer_case_is_exact(C, Cr, shape, dtype):
    from ddp_practice_amd.ops import se as S
    (N, H, W), gen = shape, torch.Generator().manual_seed(C + 7 * shape[0])
    ints = lambda lo, hi, *sz: torch.randint(lo, hi + 1, sz, generator=gen).float()
    u, idn = ints(-2, 2, N, C, H, W), ints(-2, 2, N, C, H, W)
    g = ints(0, 1, N, C, H, W) * 2 - 1
    w1, b1, w2, b2 = torch.zeros(Cr, C, 1, 1), ints(0, 2, Cr), torch.zeros(C, Cr), torch.zeros(C)
    f = R.forward(u, idn, w1, b1, w2, b2)
    b = R.backward(g, f["y"], u, w1, w2, f)
    want = dict(y=f["y"], du=b["du"], d_identity=b["d_identity"], dw1=b["dw1"].view_as(w1), db1=b["db1"],
                dw2=b["dw2"], db2=b["db2"])
    for k, v in want.items():  # exactly representable: storage dtype / fp32 quarters below 2^24
        if k in ("y", "du", "d_identity"):
            assert torch.equal(v.to(dtype).double(), v), k
        else:
            assert torch.equal((4 * v).round(), 4 * v) and (4 * v).abs().max() < 2 ** 24, k
    assert (f["y"] == 0).any() and (b["dz2"] != 0).any() and (b["dw2"] != 0).any()

    cl = lambda t: t.cuda().to(dtype).contiguous(memory_format=torch.channels_last).requires_grad_()
    ud, idd = cl(u), cl(idn)
    params = [t.cuda().requires_grad_() for t in (w1, b1, w2, b2)]
    S.clear_launches()
    y = S.squeeze_excite(ud, idd, *params)
    bwd = lambda: torch.autograd.grad(y, [ud, idd, *params], cl(g).detach(), retain_graph=True)
    grads, rec = [bwd()], S.last_launch()
    assert {k: r[2] for k, r in rec.items()} == dict.fromkeys(
        ["squeeze", "fc1", "excite", "excite_bwd_sums", "gate_bwd", "gate_wgrad", "excite_bwd"], 1), rec
    assert all(r[0] == [C, Cr] and r[1] == ("bf16" if dtype == torch.bfloat16 else "f16") for r in rec.values())
    got = dict(zip(["du", "d_identity", "dw1", "db1", "dw2", "db2"], grads[0]), y=y)
    for k, v in want.items():
        assert got[k].shape == v.shape and got[k].dtype == (dtype if v.dim() == 4 and k[:2] != "dw" else torch.float32)
        assert torch.equal(got[k].detach().double().cpu(), v), k
    assert all(torch.equal(a, c) for a, c in zip(grads[0], bwd())), "a second backward gives other bits"
