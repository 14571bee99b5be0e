"""One bf16 training step of a one-block-per-stage ResNeXt (32 groups of 4 / 8 / 16 / 32
channels) through the native path: the four grouped 3x3 convs run forward, data gradient and
weight gradient on csrc/kernels/conv_group.hip (launch record), the loss and every gradient
are finite, and the grouped gradients are fp32 of the parameters' shape."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_resnext_step_runs_the_grouped_kernels():
    from ddp_practice_amd.models import ResNet
    from ddp_practice_amd.ops import conv_group as G

    torch.manual_seed(0)
    m = ResNet((1, 1, 1, 1), num_classes=10, amp_dtype=torch.bfloat16, groups=32, width_per_group=4).cuda().train()
    x = torch.randn(2, 3, 64, 64, device="cuda")
    G.clear_launches()
    loss = torch.nn.functional.cross_entropy(m(x).float(), torch.tensor([1, 7], device="cuda"))
    loss.backward()
    torch.cuda.synchronize()
    rec = G.last_launch()
    assert {f: r[2] for f, r in rec.items()} == {"fwd": 4, "dgrad": 4, "wgrad": 4}, rec
    assert all(r[1] == "bf16" for r in rec.values()), rec
    assert torch.isfinite(loss)
    for name, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    grouped = [c for c in m.modules() if isinstance(c, torch.nn.Conv2d) and c.groups > 1]
    assert [c.weight.shape[1] for c in grouped] == [4, 8, 16, 32]
    for c in grouped:
        assert c.weight.grad.dtype == torch.float32 and c.weight.grad.shape == c.weight.shape
