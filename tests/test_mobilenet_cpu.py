"""models/mobilenet.py on the CPU: size and keys, the CLI choice, a forward, the width multiplier."""
import argparse

import torch

from ddp_practice_amd.cli import add_run_args
from ddp_practice_amd.models import mobilenet_v1


def test_parameters_and_keys():
    m = mobilenet_v1()
    assert sum(p.numel() for p in m.parameters()) == 4_231_976
    heads = {k.rsplit(".", 1)[0] for k in m.state_dict()}
    want = {"stem.0", "stem.1", "fc"} | {f"blocks.{i}.{n}" for i in range(13) for n in ("dw", "bn1", "pw", "bn2")}
    assert heads == want
    assert all(b.dw.groups == b.dw.in_channels == b.dw.out_channels for b in m.blocks)


def test_cli_model_choice():
    p = argparse.ArgumentParser()
    add_run_args(p, amp_default="fp32", checkpoint="c.pt", distributed=False)
    assert p.parse_args(["--model", "mobilenet_v1"]).model == "mobilenet_v1"


def test_cpu_forward_and_width_multiplier():
    torch.manual_seed(0)
    assert mobilenet_v1(num_classes=10)(torch.randn(2, 3, 32, 32)).shape == (2, 10)
    m = mobilenet_v1(num_classes=10, width_mult=0.5)
    assert all(c.in_channels % 8 == 0 and c.out_channels % 8 == 0 for b in m.blocks for c in (b.dw, b.pw))
    assert m.blocks[0].dw.in_channels == 16 and m.fc.in_features == 512
