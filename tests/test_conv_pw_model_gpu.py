"""The pointwise kernels (ops/conv_pw.py) inside models/mobilenet.py.

Block test: DepthwiseSeparable(24, 48, 2) on a 4 x 24 x 9 x 9 bf16 input in training mode through
forward_native, forward and backward, against the same block in float64 on the CPU.  The native
pointwise path's relative L2 error per tensor may be at most 2x that of the same pipeline with
ops.conv_pw.ENABLED off (ops/conv1x1.py's torch.mm branch): the factor of
tests/test_mobilenet_gpu.py, for the same reason -- two bf16 pipelines that differ only in the
order of fp32 sums.  The measured ratios are in profiles/pwconv_model_test.txt.

Routing test: one bf16 training step of mobilenet_v1 at width 0.75 (and 1.0) runs every pointwise
conv the implicit-GEMM kernel refuses -- counted from the module tree -- forward, data gradient
and weight gradient on csrc/kernels/conv_pw.hip; the loss and every gradient are finite, fp32 and
of the parameter's shape.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
CL = torch.channels_last


def _rel(got, ref):
    return float((got.double().cpu() - ref).norm() / ref.norm())


def test_block_matches_float64_as_well_as_the_fallback_path(monkeypatch):
    from ddp_practice_amd.models.mobilenet import DepthwiseSeparable
    from ddp_practice_amd.models.resnet import _PACKS
    from ddp_practice_amd.ops import conv_pw as G

    torch.manual_seed(0)
    ref = DepthwiseSeparable(24, 48, 2).double().train()
    for p in ref.parameters():  # (BN weights of 1 and biases of 0 would hide their own terms)
        p.data = torch.randn_like(p) * 0.5 + (1.0 if p.dim() == 1 else 0.0)
    x64 = torch.randn(4, 24, 9, 9, dtype=torch.float64).to(torch.bfloat16).double().requires_grad_()
    y64 = ref(x64)
    dy64 = torch.randn_like(y64).to(torch.bfloat16).double()
    y64.backward(dy64)
    want = [y64.detach(), x64.grad] + [p.grad for p in ref.parameters()]
    names = ["y", "dx"] + [n for n, _ in ref.named_parameters()]

    def run(enabled):
        monkeypatch.setattr(G, "ENABLED", enabled)
        _PACKS.clear()
        G.clear_launches()
        blk = copy.deepcopy(ref).float().cuda().train()
        for p in blk.parameters():
            p.grad = None
        x = x64.detach().to(torch.bfloat16).cuda().contiguous(memory_format=CL).requires_grad_()
        y = blk.forward_native(x, torch.bfloat16)
        y.backward(dy64.to(torch.bfloat16).cuda().contiguous(memory_format=CL))
        assert {f: r[2] for f, r in G.last_launch().items()} == ({"fwd": 1, "dgrad": 1, "wgrad": 1} if enabled else {})
        return [_rel(t, w) for t, w in zip([y.detach(), x.grad] + [p.grad for p in blk.parameters()], want)]

    lib, nat = run(False), run(True)
    for n, a, b in zip(names, nat, lib):
        print(f"{n:>12}: native {a:.3e} fallback {b:.3e} ratio {a / b:.3f}")
    for n, a, b in zip(names, nat, lib):
        assert a <= 2 * b, (n, a, b)


@pytest.mark.parametrize("width", [0.75, 1.0])
def test_mobilenet_step_runs_the_pointwise_kernels(width):
    from ddp_practice_amd.models import mobilenet_v1
    from ddp_practice_amd.ops import conv_igemm, conv_pw as G

    torch.manual_seed(0)
    m = mobilenet_v1(num_classes=16, amp_dtype=torch.bfloat16, width_mult=width).cuda().train()
    n = sum(not conv_igemm._K().supported(b.pw.in_channels, b.pw.out_channels) for b in m.blocks)
    assert n >= 1
    if width == 1.0:
        assert n == 1
    x = torch.randn(4, 3, 64, 64, device="cuda")
    G.clear_launches()
    loss = torch.nn.functional.cross_entropy(m(x).float(), torch.tensor([1, 7, 0, 15], device="cuda"))
    loss.backward()
    torch.cuda.synchronize()
    rec = G.last_launch()
    assert {f: r[2] for f, r in rec.items()} == {"fwd": n, "dgrad": n, "wgrad": n}, rec
    assert all(r[1] == "bf16" for r in rec.values()), rec
    assert torch.isfinite(loss)
    for name, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        assert p.grad.dtype == torch.float32 and p.grad.shape == p.shape, name
