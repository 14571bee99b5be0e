"""The head's fc weights packed once per step by the conv1 launch (csrc/kernels/conv5x5.h
pack_fc) and read by the one-launch head (convnet_head.hip head_row_kernel PK), bf16 / fp16.

  a  the pack: conv1_fwd_pack / conv1_fwd_pack_gather at batch 1 write, into a buffer prefilled
     with 0xFFFF, bitwise the layout of tests/_head_pack.py built from wfc.to(dtype) -- padding
     zero included -- on weights with rounding ties, +-0, subnormals and the largest finite
     values; the launch's other outputs are what the launch without the pack writes
  b  head_step with wfc_pk against head_step without: every output bitwise, with and without
     the scaler / speculative backward; one integer case against tests/_head_ref.py
  c  control: after fc.weight changes in place, the head given the OLD pack reproduces the old
     results, not the unpacked head's new ones -- the pack is what it reads
  d  the model: five SGD steps through TrainLoop at batch 8, graph-replayed == eager and
     pack on == pack off, bitwise (the pack is refreshed by every step's conv1 launch)
"""
import copy
import functools
import gc

import pytest
import torch

from . import _head_pack as P
from . import _head_ref as R
from . import test_head_exact_gpu as HX

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
DTYPES = [torch.bfloat16, torch.float16]
DT = pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
OUTS = ("logits", "p2", "idx2", "xh2", "loss", "dlog", "dls", "dp2", "bsum", "fstats", "rm", "rv", "nbt")


def _special_wfc(N, dtype, seed):
    """fp32 fc weights with the values a cast can get wrong in the first columns of every row."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, P.K, generator=g) * 0.05
    u = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11  # half an ulp at 1: ties
    tiny = 2.0 ** -133 if dtype == torch.bfloat16 else 2.0 ** -20  # a subnormal of the dtype
    big = 3.38e38 if dtype == torch.bfloat16 else 65504.0
    sp = [1.0 + u, 1.0 + 3 * u, -(1.0 + u), 0.0, -0.0, tiny, -tiny, 1.5 * tiny, 1e-40, big, -big, 1.0 + u + 2.0 ** -23,
          1.0 + u - 2.0 ** -24]
    for n in range(N):
        w[n, :len(sp)] = torch.tensor(sp)
        w[n, P.K - len(sp):] = torch.tensor(sp).flip(0)  # the last feature row (lanes >= 32 pad there)
    return w


def _conv1_args(dtype, B=1):
    g = torch.Generator().manual_seed(3)
    x = torch.rand(B, 1, 28, 28, generator=g).to(DEV, dtype)
    w1 = (torch.randn(16, 1, 5, 5, generator=g) * 0.2).to(DEV)
    b1 = (torch.randn(16, generator=g) * 0.1).to(DEV)
    w2 = (torch.randn(32, 16, 5, 5, generator=g) * 0.05).to(DEV)
    return x, w1, b1, w2


def _conv1_pack(C, dtype, wfc, gather, with_pack=True):
    """One conv1 launch at batch 1; returns (y1, wpk_f, wpk_d, wfc_pk) on the CPU."""
    cn, cb = C.convnet, C.convblock
    x, w1, b1, w2 = _conv1_args(dtype)
    y1 = torch.full((1, 16, 28, 28), NAN, device=DEV, dtype=dtype)
    wpk_f = torch.full((cn.W2F_LEN,), NAN, device=DEV, dtype=dtype)
    wpk_d = torch.full((cn.W2D_LEN,), NAN, device=DEV, dtype=dtype)
    pk = torch.full((P.LANES * P.nm_of(wfc.shape[0]) * P.G,), -1, dtype=torch.int16, device=DEV).view(dtype)
    extra = (wfc.to(DEV), pk) if with_pack else ()
    fslab1 = torch.empty(cb.fwd_rows(1, 16, 28, 28, 1) * cb.fslab_row(16), device=DEV)
    fstats1, shift1 = torch.empty(cb.stats_len(16), device=DEV), torch.zeros(16, device=DEV)
    if gather:
        imgs = (x[:, 0].float() * 255).round().to(torch.uint8).repeat(3, 1, 1).contiguous()
        labels = torch.arange(3, device=DEV)
        order = torch.tensor([2, 0, 1], device=DEV)
        ctr = torch.zeros(2, dtype=torch.int32, device=DEV)
        lab_out = torch.full((1,), -1, dtype=torch.int64, device=DEV)
        xg = torch.full_like(x, NAN)
        cn.conv1_fwd_pack_gather(xg, w1, b1, y1, fslab1, fstats1, shift1, w2, wpk_f, wpk_d, imgs, labels, order, ctr,
                                 lab_out, 1.0 / 255, 0.0, *extra)
        torch.cuda.synchronize()
        assert ctr.tolist() == [1, 0] and int(lab_out[0]) == 2  # the gather ran and advanced the step
    else:
        cn.conv1_fwd_pack(x, w1, b1, y1, fslab1, fstats1, shift1, w2, wpk_f, wpk_d, *extra)
        torch.cuda.synchronize()
    return y1.cpu(), wpk_f.cpu(), wpk_d.cpu(), pk.cpu()


# =============================================================================== a
@pytest.mark.parametrize("gather", [False, True], ids=["conv1_fwd_pack", "conv1_fwd_pack_gather"])
@pytest.mark.parametrize("N", [3, 10, 16])
@DT
def test_pack_layout(C, dtype, N, gather):
    wfc = _special_wfc(N, dtype, N)
    y1, wf, wd, pk = _conv1_pack(C, dtype, wfc, gather)
    want = P.pack_layout(wfc, dtype)
    got, exp = P.bits(pk), P.bits(want)
    bad = (got != exp).nonzero()
    assert bad.numel() == 0, (f"{len(bad)} of {got.numel()} elements differ, first at (lane, class, element) "
                              f"{[(int(i) // (P.nm_of(N) * 8), int(i) // 8 % P.nm_of(N), int(i) % 8) for i in bad[:4, 0]]}")
    # the conv role and the conv2 packs do not depend on the extra workgroups
    y0, wf0, wd0, pk0 = _conv1_pack(C, dtype, wfc, gather, with_pack=False)
    assert bool((P.bits(pk0) == -1).all())  # no buffer given: nothing written
    for a, b, what in ((y1, y0, "y1"), (wf, wf0, "wpk_f"), (wd, wd0, "wpk_d")):
        assert not bool(torch.isnan(a.float()).any()), what
        assert torch.equal(P.bits(a), P.bits(b)), what


@DT
def test_pack_refused(C, dtype):
    x, w1, b1, w2 = _conv1_args(dtype)
    cn = C.convnet
    y1 = torch.empty(1, 16, 28, 28, device=DEV, dtype=dtype)
    wf, wd = torch.empty(cn.W2F_LEN, device=DEV, dtype=dtype), torch.empty(cn.W2D_LEN, device=DEV, dtype=dtype)
    wfc = torch.zeros(10, P.K, device=DEV)
    with pytest.raises(RuntimeError, match="wfc_pk"):  # the 16-class size for 10 classes
        cn.conv1_fwd_pack(x, w1, b1, y1, None, None, None, w2, wf, wd, wfc, torch.empty(256 * 16 * 8, device=DEV, dtype=dtype))
    with pytest.raises(RuntimeError, match="go together"):
        cn.conv1_fwd_pack(x, w1, b1, y1, None, None, None, w2, wf, wd, None, torch.empty(256 * 10 * 8, device=DEV, dtype=dtype))
    torch.cuda.synchronize()


# =============================================================================== b
@functools.lru_cache(maxsize=None)
def _case(C, Bn, N, dtype):
    """The inputs of tests/_head_ref.py head_inputs with random float fc weights and bias."""
    t = dict(R.head_inputs(Bn, N, R.head_seed(Bn, N), Bn * int(C.convnet.fwd2_split(False))))
    g = torch.Generator().manual_seed(50 * Bn + N)
    t["wfc"] = (torch.randn(N, P.K, generator=g) * 0.05).double()
    t["wfc"][:, :5] = torch.tensor([0.0, -0.0, 1.0 + 2.0 ** -8, 2.0 ** -133, -(2.0 ** -20)], dtype=torch.float64)
    t["bfc"] = torch.randn(N, generator=g).double()
    return t


def _pack_of(C, wfc_dev, dtype):
    """wfc_pk as the conv1 launch writes it."""
    return _conv1_pack(C, dtype, wfc_dev.cpu(), gather=False)[3].to(DEV)


def _head(C, t, dtype, Bn, N, scaled, pk, wfc=None, smoothing=0.1):
    d = HX._head_buffers(t, dtype, Bn, N)
    if wfc is not None:
        d["wfc"] = wfc
    HX._step_buffers(d, HX._targets(Bn, N, "two" if Bn >= 3 else "none", 100 * Bn + N), scaled, dtype, Bn, N)
    C.convnet_head.head_step(d["y2"], d["fslab"], d["fstats"], d["g"], d["b"], d["rm"], d["rv"], d["nbt"], 0.1, t["eps"],
                             d["wfc"], d["bfc"], d["logits"], d["p2"], d["idx2"], d["xh2"], d["tgt"], -100, smoothing,
                             d["scale"], d["state"], d["loss"], d["dlog"], d["dls"], d["dp2"], d["bsum"], None, d["chk"],
                             pk)
    torch.cuda.synchronize()
    return d


def _assert_same(a, b, tag):
    for k in OUTS:
        if a[k] is None:
            assert b[k] is None
            continue
        HX._same(a[k], b[k], f"{tag} {k}")  # bit for bit, NaN == NaN


@pytest.mark.parametrize("scaled", [True, False], ids=["scaler+backward", "forward+loss"])
@pytest.mark.parametrize("N", [3, 10, 16])
@pytest.mark.parametrize("Bn", [1, 3, 32])
@DT
def test_packed_head_equals_unpacked(C, dtype, Bn, N, scaled):
    t = _case(C, Bn, N, dtype)
    wfc = t["wfc"].float().to(DEV)
    plain = _head(C, t, dtype, Bn, N, scaled, None)
    packed = _head(C, t, dtype, Bn, N, scaled, _pack_of(C, wfc, dtype))
    for k in ("logits", "p2", "xh2", "dlog"):
        assert not bool(torch.isnan(plain[k].float()).any()), k
    _assert_same(packed, plain, f"B={Bn} N={N} {dtype} scaled={scaled}")


@DT
def test_packed_head_integer_case(C, dtype):
    """The exact checks of tests/test_head_exact_gpu.py::test_head_step on the packed head."""
    Bn, N = 3, 10
    t = R.head_inputs(Bn, N, R.head_seed(Bn, N), Bn * int(C.convnet.fwd2_split(False)))
    d = _head(C, t, dtype, Bn, N, True, _pack_of(C, t["wfc"].float().to(DEV), dtype))
    tag = f"packed head_step B={Bn} N={N} {dtype}"
    HX._check_forward(d, t, dtype, Bn, N, 0.1, tag)
    HX._check_loss(d, d["tgt"].cpu(), 0.1, tag)
    HX._check_backward(d, t, dtype, Bn, N, tag)


@DT
def test_wrong_pack_size_refused(C, dtype):
    t = _case(C, 1, 10, dtype)
    with pytest.raises(RuntimeError, match="wfc_pk"):
        _head(C, t, dtype, 1, 10, True, torch.zeros(256 * 16 * 8, device=DEV, dtype=dtype))
    with pytest.raises(RuntimeError, match="wfc_pk"):
        _head(C, t, dtype, 1, 10, True, torch.zeros(256 * 10 * 8, device=DEV, dtype=torch.float32))


# =============================================================================== c
@DT
def test_stale_pack_is_what_is_read(C, dtype):
    Bn, N = 3, 10
    t = _case(C, Bn, N, dtype)
    wfc = t["wfc"].float().to(DEV)
    old_pk = _pack_of(C, wfc, dtype)
    old = _head(C, t, dtype, Bn, N, True, None)
    wfc.mul_(-1.5)  # in place: fc.weight after an optimizer step
    new = _head(C, t, dtype, Bn, N, True, None, wfc=wfc)
    stale = _head(C, t, dtype, Bn, N, True, old_pk, wfc=wfc)
    _assert_same(stale, old, "stale pack")
    assert not torch.equal(stale["logits"], new["logits"]) and not torch.equal(stale["dp2"], new["dp2"])
    _assert_same(_head(C, t, dtype, Bn, N, True, _pack_of(C, wfc, dtype), wfc=wfc), new, "fresh pack")


# =============================================================================== d
def _five_steps(base, dtype, use_graph):
    from ddp_practice_amd.amp import GradScaler
    from ddp_practice_amd.data import DeviceLoader, synthetic
    from ddp_practice_amd.engine import TrainLoop
    from ddp_practice_amd.nn import CrossEntropyLoss
    from ddp_practice_amd.optim import SGD

    model = copy.deepcopy(base)
    loader = DeviceLoader(synthetic(8 * 5, seed=7), batch_size=8, shuffle=False, device=DEV, dtype=dtype)
    opt = SGD(model.parameters(), lr=0.05)
    loop = TrainLoop(model, CrossEntropyLoss(), opt, loader, GradScaler(), use_graph=use_graph, steps_per_graph=4)
    loop.run_epoch()
    torch.cuda.synchronize()
    assert loop.graph_error is None, loop.graph_error
    assert loop.global_step == 5
    return {k: v.clone() for k, v in model.state_dict().items()}


@DT
def test_model_graph_eager_pack_on_off(C, dtype, monkeypatch):
    from ddp_practice_amd.models import ConvNet
    from ddp_practice_amd.ops import convnet_fused as op

    gc.collect()
    torch.manual_seed(0)
    base = ConvNet(amp_dtype=dtype).to(DEV)
    calls = []
    real = C.convnet_head.head_step

    class Spy:  # the head launches, with or without a pack
        def __getattr__(self, k):
            return getattr(C.convnet_head, k)

        @staticmethod
        def head_step(*a):
            calls.append(a[-1] is not None)
            return real(*a)

    class Ext:
        def __getattr__(self, k):
            return Spy() if k == "convnet_head" else getattr(C, k)

    monkeypatch.setattr(op, "_load_ext", lambda: Ext())
    monkeypatch.setattr(op, "_HEAD_PACK", True)
    on_eager = _five_steps(base, dtype, False)
    assert calls and all(calls), "the training path did not hand the head a pack"
    on_graph = _five_steps(base, dtype, True)
    del calls[:]
    monkeypatch.setattr(op, "_HEAD_PACK", False)
    off_eager = _five_steps(base, dtype, False)
    assert calls and not any(calls)
    for k in on_eager:
        assert torch.equal(on_eager[k], on_graph[k]), ("graph vs eager", k)
        assert torch.equal(on_eager[k], off_eager[k]), ("pack on vs off", k)
    assert not torch.equal(on_eager["fc.weight"], base.state_dict()["fc.weight"])
