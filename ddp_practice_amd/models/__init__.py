"""Model zoo: the reference ConvNet, the ResNet-50 stress config, ResNeXt-50 32x4d, their
squeeze-and-excitation variants, MobileNetV1 and MnasNet-B1."""
from .convnet import ConvNet  # noqa: F401
from .mnasnet import MNASNet, mnasnet1_0  # noqa: F401
from .mobilenet import MobileNetV1, mobilenet_v1  # noqa: F401
from .resnet import ResNet, resnet50, resnext50_32x4d, se_resnet50, se_resnext50_32x4d  # noqa: F401
