"""ResNeXt-50 32x4d (models/resnet.py): torchvision's parameter count, grouped weight shapes
and state_dict keys; a small instance trains on the CPU; ResNet-50 is unchanged; the CLI choice."""
import argparse

import torch

from ddp_practice_amd.cli import add_run_args
from ddp_practice_amd.models import ResNet, resnet50, resnext50_32x4d


def _count(m):
    return sum(p.numel() for p in m.parameters())


def test_resnext50_parameters_and_keys():
    m, r = resnext50_32x4d(), resnet50()
    assert _count(m) == 25_028_904 and _count(r) == 25_557_032
    grouped = {tuple(c.weight.shape) for c in m.modules() if isinstance(c, torch.nn.Conv2d) and c.groups > 1}
    assert grouped == {(128, 4, 3, 3), (256, 8, 3, 3), (512, 16, 3, 3), (1024, 32, 3, 3)}
    assert sum(c.groups == 32 for c in m.modules() if isinstance(c, torch.nn.Conv2d)) == 16
    assert list(m.state_dict()) == list(r.state_dict())


def test_small_resnext_trains_on_cpu():
    torch.manual_seed(0)
    m = ResNet((1, 1, 1, 1), num_classes=10, groups=32, width_per_group=4)
    loss = torch.nn.functional.cross_entropy(m(torch.randn(2, 3, 32, 32)), torch.tensor([1, 7]))
    loss.backward()
    assert torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in m.parameters())


def test_cli_model_choice():
    p = argparse.ArgumentParser()
    add_run_args(p, amp_default="fp32", checkpoint="c.pt", distributed=False)
    assert p.parse_args(["--model", "resnext50_32x4d"]).model == "resnext50_32x4d"
