"""Model zoo: the reference ConvNet, the ResNet-50 stress config and ResNeXt-50 32x4d."""
from .convnet import ConvNet  # noqa: F401
from .resnet import ResNet, resnet50, resnext50_32x4d  # noqa: F401
