"""Plain-torch statement of FNet3D (the 3-D U-Net of Ounkomol et al. 2018 as ``viscy_models.unet.Unet3d`` builds it): the CPU
yardstick of viscy_amd.unet3d, pinned against tests/golden/fnet3d.pt.  Same parameter names as the reference, so state dicts
move between the three freely."""

from __future__ import annotations

import torch
from torch import Tensor, nn


class ConvBnRelu(nn.Module):
    def __init__(self, cin: int, cout: int):
        super().__init__()
        self.proj = nn.Conv3d(cin, cout, 3, padding=1)
        self.norm = nn.BatchNorm3d(cout)

    def forward(self, x: Tensor) -> Tensor:
        return torch.relu(self.norm(self.proj(x)))


class DoubleConv(nn.Module):
    def __init__(self, cin: int, cout: int):
        super().__init__()
        self.block1 = ConvBnRelu(cin, cout)
        self.block2 = ConvBnRelu(cout, cout)

    def forward(self, x: Tensor) -> Tensor:
        return self.block2(self.block1(x))


class Bottleneck(nn.Module):
    def __init__(self, c: int):
        super().__init__()
        self.block = DoubleConv(c, c)

    def forward(self, x: Tensor) -> Tensor:
        return self.block(x)


class FNet3D(nn.Module):
    def __init__(self, in_channels: int = 1, out_channels: int = 1, depth: int = 4, mult_chan: int = 32):
        super().__init__()
        dims = [mult_chan * 2 ** i for i in range(depth + 1)]
        self.depth = depth
        self.inconv = nn.Conv3d(in_channels, dims[0], 3, padding=1)
        self._encoder_blocks = nn.ModuleList(nn.ModuleList([DoubleConv(dims[i], dims[i])]) for i in range(depth))
        self._downsamples = nn.ModuleList(nn.Conv3d(dims[i], dims[i + 1], 3, stride=2, padding=1) for i in range(depth))
        self.bottleneck = Bottleneck(dims[-1])
        self._upsamples = nn.ModuleList(
            nn.ConvTranspose3d(dims[i + 1], dims[i], 3, stride=2, padding=1, output_padding=1) for i in reversed(range(depth)))
        self._decoder_blocks = nn.ModuleList(nn.ModuleList([DoubleConv(2 * dims[i], dims[i])]) for i in reversed(range(depth)))
        self.outconv = nn.Conv3d(dims[0], out_channels, 3, padding=1)

    def forward(self, x: Tensor) -> Tensor:
        h = self.inconv(x)
        skips = []
        for blocks, down in zip(self._encoder_blocks, self._downsamples):
            h = blocks[0](h)
            skips.append(h)
            h = down(h)
        h = self.bottleneck(h)
        for up, blocks in zip(self._upsamples, self._decoder_blocks):
            h = blocks[0](torch.cat([up(h), skips.pop()], dim=1))
        return self.outconv(h)
