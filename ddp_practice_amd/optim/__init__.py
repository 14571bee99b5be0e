"""Optimizers (multi-tensor HIP kernels), gradient clipping, gradient accumulation, weight averaging
and the device-resident learning-rate schedule."""
from .accum import GradAccumulator  # noqa: F401
from .adamw import Adam, AdamW  # noqa: F401
from .clip import clip_grad_norm_  # noqa: F401
from .ema import EMA  # noqa: F401
from .lr import DeviceLR  # noqa: F401
from .sgd import SGD  # noqa: F401
