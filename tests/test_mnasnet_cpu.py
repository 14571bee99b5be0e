"""models/mnasnet.py on the CPU: size, torchvision's keys, the depthwise layers, the CLI choice, a forward."""
import argparse

import torch

from ddp_practice_amd.cli import add_run_args
from ddp_practice_amd.models import mnasnet1_0

STACKS = ((16, 24, 3, 2, 3, 3), (24, 40, 5, 2, 3, 3), (40, 80, 5, 2, 6, 3), (80, 96, 3, 1, 6, 2),
          (96, 192, 5, 2, 6, 4), (192, 320, 3, 1, 6, 1))
DEPTHWISE = [(32, 3, 1), (48, 3, 2), (72, 3, 1), (72, 3, 1), (72, 5, 2), (120, 5, 1), (120, 5, 1), (240, 5, 2),
             (480, 5, 1), (480, 5, 1), (480, 3, 1), (576, 3, 1), (576, 5, 2), (1152, 5, 1), (1152, 5, 1),
             (1152, 5, 1), (1152, 3, 1)]


def test_parameters_keys_and_depthwise_layers():
    m = mnasnet1_0()
    assert sum(p.numel() for p in m.parameters()) == 4_383_312
    want = {f"layers.{i}" for i in (0, 1, 3, 4, 6, 7, 14, 15)} | {"classifier.1"}
    want |= {f"layers.{8 + s}.{b}.layers.{i}" for s, st in enumerate(STACKS) for b in range(st[5])
             for i in (0, 1, 3, 4, 6, 7)}
    assert {k.rsplit(".", 1)[0] for k in m.state_dict()} == want
    dw = [(c.in_channels, c.kernel_size[0], c.stride[0]) for c in m.modules()
          if isinstance(c, torch.nn.Conv2d) and c.groups > 1]
    assert dw == DEPTHWISE
    assert all(c.groups == c.in_channels == c.out_channels and c.padding[0] == c.kernel_size[0] // 2
               for c in m.modules() if isinstance(c, torch.nn.Conv2d) and c.groups > 1)


def test_cli_model_choice():
    p = argparse.ArgumentParser()
    add_run_args(p, amp_default="fp32", checkpoint="c.pt", distributed=False)
    assert p.parse_args(["--model", "mnasnet1_0"]).model == "mnasnet1_0"


def test_cpu_forward():
    torch.manual_seed(0)
    assert mnasnet1_0(num_classes=10)(torch.randn(2, 3, 32, 32)).shape == (2, 10)
