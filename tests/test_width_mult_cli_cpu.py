"""``--width-mult`` (ddp_practice_amd/cli.py): mobilenet_v1 only, default 1.0."""
import argparse

import pytest

from ddp_practice_amd.cli import add_run_args, build_model


def _parse(*argv):
    p = argparse.ArgumentParser()
    add_run_args(p, amp_default="fp32", checkpoint="c.pt", distributed=False)
    return p.parse_args(list(argv))


def test_width_mult_reaches_the_model():
    m = build_model(_parse("--model", "mobilenet_v1", "--width-mult", "0.5", "--num-classes", "10"))
    assert m.blocks[0].dw.in_channels == 16 and m.blocks[0].pw.out_channels == 32


def test_width_mult_is_mobilenets_only():
    with pytest.raises(SystemExit, match="--width-mult"):
        build_model(_parse("--model", "resnet50", "--width-mult", "0.5"))


def test_default_is_one():
    assert _parse().width_mult == 1.0 and _parse("--model", "mobilenet_v1").width_mult == 1.0
