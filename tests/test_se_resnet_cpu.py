"""SE-ResNet-50 and SE-ResNeXt-50 32x4d (models/resnet.py): parameter counts, timm's ``se.fc{1,2}``
keys on top of the parent model's, a small instance trains on the CPU, and the CLI choices."""
import argparse

import pytest
import torch

from ddp_practice_amd.cli import add_run_args
from ddp_practice_amd.models import ResNet, resnet50, resnext50_32x4d, se_resnet50, se_resnext50_32x4d


@pytest.mark.parametrize("se,parent,count", [(se_resnet50, resnet50, 28_088_024),
                                             (se_resnext50_32x4d, resnext50_32x4d, 27_559_896)])
def test_parameters_and_keys(se, parent, count):
    m, r = se(), parent()
    n = lambda net: sum(p.numel() for p in net.parameters())
    assert n(m) == count == n(r) + 2_530_992
    blocks = [f"layer{i + 1}.{b}" for i, k in enumerate((3, 4, 6, 3)) for b in range(k)]
    gate = {f"{b}.se.{fc}.{t}" for b in blocks for fc in ("fc1", "fc2") for t in ("weight", "bias")}
    keys = list(m.state_dict())
    assert set(keys) == set(r.state_dict()) | gate and len(keys) == len(r.state_dict()) + 64


def test_small_se_resnet_trains_on_cpu():
    torch.manual_seed(0)
    m = ResNet((1, 1, 1, 1), num_classes=10, se_reduction=16)
    opt, x, losses = torch.optim.SGD(m.parameters(), lr=0.05), torch.randn(2, 3, 32, 32), []
    for _ in range(3):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(m(x), torch.tensor([1, 7]))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[0] > losses[1] > losses[2], losses


@pytest.mark.parametrize("name", ["se_resnet50", "se_resnext50_32x4d"])
def test_cli_model_choice(name):
    p = argparse.ArgumentParser()
    add_run_args(p, amp_default="fp32", checkpoint="c.pt", distributed=False)
    assert p.parse_args(["--model", name]).model == name
