"""models/mnasnet.py on the native path.

Block test: one inverted residual (40 -> 40, 5x5 depthwise, stride 1, expansion 3: the residual is
live; input 4 x 40 x 9 x 9, bf16, training mode) forward and backward against the same block in
float64 on the CPU.  The native depthwise path's relative L2 error per tensor (output, dx, every
parameter gradient) may be at most 2x that of the same pipeline with the library depthwise conv
(ops.conv_dw.ENABLED off): two bf16 pipelines that differ only in the order of 25-term fp32 sums.
The measured ratios are in profiles/dwconv5_model_test.txt.

Routing test: one bf16 training step of mnasnet1_0 runs its ten 5x5 depthwise convs on
csrc/kernels/conv_dw5.hip and its seven 3x3 ones on conv_dw.hip, forward, data gradient and
weight gradient (launch record); the loss and every gradient are finite, fp32 and of the
parameter's shape.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
CL = torch.channels_last


def _rel(got, ref):
    return float((got.double().cpu() - ref).norm() / ref.norm())


def test_block_matches_float64_as_well_as_the_library_path(monkeypatch):
    from ddp_practice_amd.models.mnasnet import InvertedResidual
    from ddp_practice_amd.models.resnet import _PACKS
    from ddp_practice_amd.ops import conv_dw as G

    torch.manual_seed(0)
    ref = InvertedResidual(40, 40, 5, 1, 3).double().train()
    assert ref.apply_residual
    for p in ref.parameters():  # (BN weights of 1 and biases of 0 would hide their own terms)
        p.data = torch.randn_like(p) * 0.5 + (1.0 if p.dim() == 1 else 0.0)
    x64 = torch.randn(4, 40, 9, 9, dtype=torch.float64).to(torch.bfloat16).double().requires_grad_()
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
        assert {f: r[2] for f, r in G.last_launch().items()} == ({"fwd5": 1, "dgrad5": 1, "wgrad5": 1} if enabled else {})
        return [_rel(t, w) for t, w in zip([y.detach(), x.grad] + [p.grad for p in blk.parameters()], want)]

    lib, nat = run(False), run(True)
    for n, a, b in zip(names, nat, lib):
        print(f"{n:>18}: native {a:.3e} library {b:.3e} ratio {a / max(b, 1e-300):.3f}")
    for n, a, b in zip(names, nat, lib):
        assert a <= 2 * b, (n, a, b)


def test_mnasnet_step_runs_both_depthwise_families():
    from ddp_practice_amd.models import mnasnet1_0
    from ddp_practice_amd.ops import conv_dw as G

    torch.manual_seed(0)
    m = mnasnet1_0(num_classes=16, amp_dtype=torch.bfloat16, dropout=0.0).cuda().train()
    x = torch.randn(4, 3, 64, 64, device="cuda")
    G.clear_launches()
    loss = torch.nn.functional.cross_entropy(m(x).float(), torch.tensor([1, 7, 0, 15], device="cuda"))
    loss.backward()
    torch.cuda.synchronize()
    rec = G.last_launch()
    want = {**{f: 7 for f in ("fwd", "dgrad", "wgrad")}, **{f: 10 for f in ("fwd5", "dgrad5", "wgrad5")}}
    assert {f: r[2] for f, r in rec.items()} == want, rec
    assert all(r[1] == "bf16" for r in rec.values()), rec
    assert torch.isfinite(loss)
    for name, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        assert p.grad.dtype == torch.float32 and p.grad.shape == p.shape, name
