"""One bf16 training step of a one-block-per-stage SE-ResNeXt through the native path: every family of
csrc/kernels/se.hip runs 4 times, the loss and all gradients are finite, the SE gradients are fp32 of the
parameters' shapes, and the logits agree with the same weights on the torch composition of the gate
(ops.se.ENABLED = False, what DPA_SE=0 sets; the convs and BNs stay native).

Bound on the logits: both paths round the same fp32 gate output once, so an SE output differs by at most
one bf16 ulp, 2 r |y| with the op test's r = 2^-8 (tests/test_se_gpu.py).  A relative perturbation passes
a following bottleneck with a gain of at most 2 (its BatchNorms renormalise; the residual adds it once
more), so the four blocks' perturbations reach the logits as at most 2 r (8 + 4 + 2 + 1) = 15 * 2^-7 of
the largest logit.  Measured on an MI355X against the composition: max |diff| 1.17e-2 with a largest logit
of 0.789, bound 9.25e-2: a margin of 7.9."""
import pytest
import torch

pytestmark = pytest.mark.gpu
FAMILIES = ["squeeze", "fc1", "excite", "excite_bwd_sums", "gate_bwd", "gate_wgrad", "excite_bwd"]


def test_se_resnext_step_runs_the_se_kernels(monkeypatch):
    from ddp_practice_amd.models import ResNet
    from ddp_practice_amd.ops import se as S
    torch.manual_seed(0)
    m = ResNet((1, 1, 1, 1), num_classes=10, amp_dtype=torch.bfloat16, groups=32, width_per_group=4,
               se_reduction=16).cuda().train()
    x = torch.randn(2, 3, 64, 64, device="cuda")
    state = {k: v.clone() for k, v in m.state_dict().items()}
    S.clear_launches()
    logits = m(x).float()
    loss = torch.nn.functional.cross_entropy(logits, torch.tensor([1, 7], device="cuda"))
    loss.backward()
    torch.cuda.synchronize()
    rec = S.last_launch()
    assert {f: r[1:] for f, r in rec.items()} == dict.fromkeys(FAMILIES, ("bf16", 4)), rec
    assert torch.isfinite(loss)
    for name, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        if ".se." in name:
            assert p.grad.dtype == torch.float32 and p.grad.shape == p.shape, name

    m.load_state_dict(state)  # the running statistics of the first pass undone
    monkeypatch.setattr(S, "ENABLED", False)
    S.clear_launches()
    ref = m(x).float().detach()
    assert S.last_launch() == {}
    diff, scale = float((logits.detach() - ref).abs().max()), float(ref.abs().max())
    print(f"native vs composition logits: max |diff| {diff:.4e}, largest logit {scale:.4e}, "
          f"bound {15 * 2.0 ** -7 * scale:.4e}")
    assert diff <= 15 * 2.0 ** -7 * scale
