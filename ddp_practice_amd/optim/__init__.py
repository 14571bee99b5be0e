"""Optimizers (multi-tensor HIP kernels), gradient clipping, weight averaging and the device-resident
learning-rate schedule."""
from .adamw import Adam, AdamW  # noqa: F401
from .clip import clip_grad_norm_  # noqa: F401
from .ema import EMA  # noqa: F401
from .lr import DeviceLR  # noqa: F401
from .sgd import SGD  # noqa: F401
