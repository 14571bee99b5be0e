"""ops/se.py with random gates against float64 (tests/_se_ref.py), elementwise, plus the GradTap hand-off,
hipGraph replay and the refusal of an unsupported shape.  Inputs: u (never 0), identity, g multiples of 1/4 in
[-2, 2], W2 ~ U(-1, 1) / sqrt(Cr), b2 ~ U(-1, 1), W1 ~ U(-1, 1) * 4 / C and b1 = +-1/2 alternating, so the
h > 0 mask cannot depend on rounding (asserted with a margin of 100); the y > 0 mask of the backward is
taken from the stored y itself, so it is an input, not a result.
Bounds (``bounds``), derived, not tuned: e = 2^-24, r = 2^-8 (bf16) or 2^-11 (fp16).  A sum of T fp32
terms in any order (MFMA 4-term groups included) plus its bias add and one more operation is within
(T + 2) e sum|terms| of the exact sum; the error of each operand enters to first order, through
|sigmoid'| <= 1/4 and |(s (1 - s))'| <= 1:
  p    (HW + 2) e mean|u|                              h   (C + 2) e (|p| |W1|^T + |b1|) + e_p |W1|^T
  s    ((Cr + 2) e (h |W2|^T + |b2|) + e_h |W2|^T) / 4 + 4 e   (exp, add, divide: 4 roundings of s <= 1)
  y    r |y| + |u| e_s + 2 e (|u| s + |identity|)      d_identity = g [y > 0] is a copy: exact
  ds   (HW + 2) e sum|gm u|                            dz2  e_ds / 4 + |ds| e_s + 3 e |dz2|
  db2  (N + 2) e sum_n|dz2| + sum_n e_dz2              dW2  (N + 2) e |dz2|^T h + e_dz2^T h + |dz2|^T e_h
  dz1  (C + 2) e |dz2| |W2| + e_dz2 |W2|   (masked)     db1, dW1  as db2, dW2 with dz1 and p
  du   r |du| + |gm| e_s + ((Cr + 2) e |dz1| |W1| + e_dz1 |W1|) / HW + 2 e (|gm| s + |dp| / HW)
Each line is one rounding to storage plus the accumulation bounds of the reductions that feed the output,
each once.  That they bind: a dropped pixel moves p by >= 1 / (4 HW) >= 2.1e-3 (e_p <= 1.4e-5) and ds by
|gm u| >= 1/16 wherever y > 0 (e_ds <= 7e-6 * 117 * 4); a dropped batch row n removes dz2[n, c] from db2[c] and
dz1[n, j] from db1[j], and every row has one of each above twice that bound (asserted)."""
import functools

import pytest
import torch

from . import _se_ref as R

E = 2.0 ** -24
ROWS = [(64, 4), (128, 8), (256, 16), (2048, 128)]
CASES = [(C, Cr, s, dt) for C, Cr in ROWS for s in [(3, 13, 9), (17, 5, 5)] for dt in (torch.bfloat16, torch.float16)]
IDS = [f"{C}x{Cr}-{'x'.join(map(str, s))}-{'bf16' if dt == torch.bfloat16 else 'f16'}" for C, Cr, s, dt in CASES]


@functools.lru_cache(None)
def case(C, Cr, shape, dtype):
    # (inputs, float64 forward) of a case, computed once; nobody modifies them
    (N, H, W), gen = shape, torch.Generator().manual_seed(C + shape[0])
    uni = lambda *sz: torch.rand(sz, generator=gen) * 2 - 1
    grid = lambda: torch.randint(-8, 9, (N, C, H, W), generator=gen).float() / 4
    u, idn, g = grid(), grid(), grid()
    u[u == 0] = 0.25
    x = dict(u=u.to(dtype), idn=idn.to(dtype), g=g.to(dtype), w1=uni(Cr, C, 1, 1) * 4 / C,
             b1=0.5 - torch.arange(Cr).float() % 2, w2=uni(C, Cr) / Cr ** 0.5, b2=uni(C))
    return x, R.forward(x["u"], x["idn"], x["w1"], x["b1"], x["w2"], x["b2"])


def bounds(x, f, b, dtype):
    r = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    u, idn, w1, w2 = x["u"].double(), x["idn"].double(), x["w1"].double().flatten(1).abs(), x["w2"].double().abs()
    (N, C, H, W), Cr, HW = u.shape, w1.shape[0], u.shape[2] * u.shape[3]
    bc = lambda t: t[:, :, None, None]
    p, h, s, gm = f["p"].abs(), f["h"], f["s"], b["gm"].abs()
    e_p = (HW + 2) * E * u.abs().mean((2, 3))
    e_h = (C + 2) * E * (p @ w1.t() + x["b1"].abs()) + e_p @ w1.t()
    e_s = ((Cr + 2) * E * (h @ w2.t() + x["b2"].abs()) + e_h @ w2.t()) / 4 + 4 * E
    e_ds = (HW + 2) * E * (gm * u.abs()).sum((2, 3))
    dz2, dz1 = b["dz2"].abs(), b["dz1"].abs()
    e_dz2 = e_ds / 4 + b["ds"].abs() * e_s + 3 * E * dz2
    e_dz1 = ((C + 2) * E * dz2 @ w2 + e_dz2 @ w2) * (h > 0)
    e_dp = ((Cr + 2) * E * dz1 @ w1 + e_dz1 @ w1) / HW
    return dict(
        y=r * f["y"] + u.abs() * bc(e_s) + 2 * E * (u.abs() * bc(s) + idn.abs()), d_identity=torch.zeros_like(u),
        du=r * b["du"].abs() + gm * bc(e_s) + bc(e_dp) + 2 * E * (gm * bc(s) + bc(b["dp"].abs()) / HW),
        db2=(N + 2) * E * dz2.sum(0) + e_dz2.sum(0), dw2=(N + 2) * E * dz2.t() @ h + e_dz2.t() @ h + dz2.t() @ e_h,
        db1=(N + 2) * E * dz1.sum(0) + e_dz1.sum(0), dw1=(N + 2) * E * dz1.t() @ p + e_dz1.t() @ p + dz1.t() @ e_p,
        e_h=e_h)


def check(got, x, f, dtype):
    b = R.backward(x["g"], got["y"], x["u"], x["w1"], x["w2"], f)
    tol = bounds(x, f, b, dtype)
    for k in ("y", "du", "d_identity", "dw1", "db1", "dw2", "db2"):
        err = (got[k].detach().double().cpu().reshape(tol[k].shape) - (f[k] if k == "y" else b[k])).abs()
        print(f"{k}: max err {err.max():.3e}, max err / bound {(err / tol[k].clamp_min(1e-300)).max():.3f}")
        assert (err <= tol[k]).all(), k
    return b, tol


def put(x, dev):
    cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last)
    return [cl(x["u"]), cl(x["idn"]), *(x[k].to(dev) for k in ("w1", "b1", "w2", "b2"))], cl(x["g"])

def run(fn, x, dev, tap=None, ins=None):
    leaves, g = ins or put(x, dev)  # (ins: already on the device, for a capture)
    leaves = [t.detach().requires_grad_() for t in leaves]
    y = fn(*leaves, tap) if tap is not None else fn(*leaves)
    grads = torch.autograd.grad(y, leaves, g, allow_unused=tap is not None)
    return dict(zip(["du", "d_identity", "dw1", "db1", "dw2", "db2"], grads), y=y)


@pytest.mark.parametrize("dev", ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)])
@pytest.mark.parametrize("C,Cr,shape,dtype", CASES, ids=IDS)
def test_every_output_meets_its_bound(C, Cr, shape, dtype, dev):
    """cuda: the kernels.  cpu: the float32 torch composition -- the condition on the inputs."""
    from ddp_practice_amd.ops import se as S
    x, f = case(C, Cr, shape, dtype)
    b, tol = check(run(S.squeeze_excite if dev == "cuda" else S.squeeze_excite_torch, x, dev), x, f, dtype)
    z1 = (f["p"] @ x["w1"].double().flatten(1).t() + x["b1"]).abs()
    assert (z1 > 100 * tol["e_h"]).all()  # the h > 0 mask is certain
    for dz, db in ((b["dz2"], tol["db2"]), (b["dz1"], tol["db1"])):  # a dropped batch row shows in db2 and db1
        assert ((dz.abs() > 2 * db).any(1)).all()


@pytest.mark.gpu
def test_tap_graph_replay_and_refusal():
    from ddp_practice_amd.ops.conv1x1 import GradTap
    from ddp_practice_amd.ops.se import squeeze_excite
    x, _ = case(128, 8, (3, 13, 9), torch.bfloat16)
    eager, tap = run(squeeze_excite, x, "cuda"), GradTap()
    assert run(squeeze_excite, x, "cuda", tap)["d_identity"] is None and torch.equal(tap.grad, eager["d_identity"])

    ins, stream, graph = put(x, "cuda"), torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        run(squeeze_excite, x, "cuda", ins=ins)  # warm-up on the capture stream
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            out = run(squeeze_excite, x, "cuda", ins=ins)
    for _ in range(2):
        for t in out.values():
            t.detach().fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(out[k], eager[k]) for k in eager)

    bad = torch.zeros(2, 96, 4, 4, device="cuda", dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="squeeze_excite: no kernel for u"):
        squeeze_excite(bad, bad, *(torch.zeros(s, device="cuda") for s in [(8, 96), (8,), (96, 8), (96,)]))
