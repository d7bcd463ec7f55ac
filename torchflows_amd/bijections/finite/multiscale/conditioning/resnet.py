"""Residual conditioner for image couplings (reference ``multiscale/conditioning/resnet.py``:
blocks :11-59, ``ResNet`` :62-118, ``ResNetConditioner`` :121-139).

A ``ConvModifier`` brings the conditioner image to ``(4, 32, 32)``; three stages follow, each
``x + relu(bn2(conv2(relu(bn1(conv1(x))))))`` with 16 hidden channels and a stride-2 convolution behind
it that doubles the channels and halves the frame: (4, 32, 32) -> (8, 16, 16) -> (16, 8, 8) ->
(32, 4, 4) = 512 features, then ``Linear(512, 100)``, ``leaky_relu``, ``Linear(100, n_outputs)`` and the
(-2, 2) sigmoid bound.  BatchNorm sits in front of the ReLU, so at inference it folds into the convolution
and a whole coupling with this conditioner is one launch (image_program.py, csrc/tfk_glow_resnet.hip:
kinds 4 and 6 of ``tfk_glow_coupling``).  Training, float64 and host tensors run the modules below on
ATen.  Module and attribute names match the reference so state dicts carry over.
"""
from __future__ import annotations

from typing import Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from torchflows_amd.bijections.finite.autoregressive.conditioning.transforms import (
    TensorConditionerTransform)
from torchflows_amd.bijections.finite.multiscale.conditioning.classic import ConvModifier


class BasicResidualBlock(nn.Module):
    """``x + relu(bn2(conv2(relu(bn1(conv1(x))))))``; height and width are kept."""

    def __init__(self, in_channels: int, hidden_channels: int):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels, hidden_channels, kernel_size=3, padding=1)
        self.bn1 = nn.BatchNorm2d(hidden_channels)
        self.conv2 = nn.Conv2d(hidden_channels, in_channels, kernel_size=3, padding=1)
        self.bn2 = nn.BatchNorm2d(in_channels)

    def h(self, x):
        hidden = F.relu(self.bn1(self.conv1(x)))
        return F.relu(self.bn2(self.conv2(hidden)))

    def forward(self, x):
        return x + self.h(x)


class BasicResidualBlockGroup(nn.Module):
    def __init__(self, in_channels: int, n_blocks: int, hidden_channels: int = 16):
        super().__init__()
        self.blocks = nn.ModuleList(BasicResidualBlock(in_channels, hidden_channels) for _ in range(n_blocks))

    def forward(self, x):
        for block in self.blocks:
            x = block(x)
        return x


class BottleneckBlock(nn.Module):
    """Stride-2 convolution: twice the channels, half the height and width."""

    def __init__(self, in_channels: int):
        super().__init__()
        self.conv2d = nn.Conv2d(in_channels, 2 * in_channels, kernel_size=3, stride=2, padding=1)

    def forward(self, x):
        return self.conv2d(x)


class ResNet(nn.Module):
    def __init__(self, c: int, h: int, w: int, hidden_size: int = 100, n_outputs: int = 10,
                 n_blocks: Tuple[int, int, int] = (1, 1, 1)):
        super().__init__()
        self.modifier = ConvModifier((c, h, w), c_target=4, h_target=32, w_target=32)
        self.stage1 = BasicResidualBlockGroup(4, n_blocks=n_blocks[0])
        self.down1 = BottleneckBlock(4)
        self.stage2 = BasicResidualBlockGroup(8, n_blocks=n_blocks[1])
        self.down2 = BottleneckBlock(8)
        self.stage3 = BasicResidualBlockGroup(16, n_blocks=n_blocks[2])
        self.down3 = BottleneckBlock(16)
        self.linear1 = nn.Linear(32 * 4 * 4, hidden_size)
        self.linear2 = nn.Linear(hidden_size, n_outputs)

    def forward(self, x):
        lead = x.shape[:-3]
        out = self.modifier(x.reshape(-1, *x.shape[-3:]))        # conv2d wants exactly one batch axis
        out = self.down1(self.stage1(out))
        out = self.down2(self.stage2(out))
        out = self.down3(self.stage3(out))
        out = F.leaky_relu(self.linear1(out.reshape(*lead, 512)))
        return self.linear2(out)


class ResNetConditioner(TensorConditionerTransform):
    def __init__(self, input_event_shape, parameter_shape, **kwargs):
        super().__init__(input_event_shape=input_event_shape, parameter_shape=parameter_shape,
                         output_lower_bound=-2.0, output_upper_bound=2.0, **kwargs)
        self.network = ResNet(*input_event_shape, n_outputs=self.n_transformer_parameters)

    def predict_theta_flat(self, x: torch.Tensor, context: torch.Tensor = None) -> torch.Tensor:
        return self.network(x)
