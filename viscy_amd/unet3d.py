"""FNet3D on MI355X: drop-in for ``viscy_models.unet.Unet3d`` (the 3-D U-Net of Ounkomol et al. 2018, the cytoland
``architecture: FNet3D``; reference ``viscy_models/unet/{unet3d.py, unet3d_base.py, blocks.py}``).

Same constructor, attributes (``num_blocks``, ``downsamples_z``, ``in_stack_depth``, ``out_stack_depth``), divisibility
``ValueError``, initialisation and ``state_dict()`` keys.  The ``nn.Conv3d`` / ``nn.BatchNorm3d`` / ``nn.ConvTranspose3d``
modules only HOLD parameters and running statistics; every forward and backward is a fixed schedule of the HIP kernels of
``csrc/conv3d.hip`` driven by ``Engine``:

  * activations are channels-last ``[B*D*H*W, C]`` matrices in bf16 (production) or fp32 (parity mode);
  * the decoder's ``cat([up, skip])`` is one ``[M, 2C]`` buffer: the encoder block's BatchNorm + ReLU writes the skip into
    columns [C, 2C), the downsampling convolution reads that slice, the transposed convolution writes columns [0, C);
  * BatchNorm statistics come from the convolution epilogue; running statistics are updated on the device.

There is no eager / CPU fallback: ``forward`` raises unless the input is on a HIP device and libvsx.so is loadable.
"""

from __future__ import annotations

import torch
from torch import Tensor, nn

from .flat import NativeModule


def _fnet_weights_init(m: nn.Module) -> None:
    """F-Net initialisation: conv / transposed-conv weights N(0, 0.02), BatchNorm weight N(1, 0.02) and bias 0; conv biases
    keep torch's default (uniform +-1/sqrt(fan_in))"""
    if isinstance(m, (nn.Conv3d, nn.ConvTranspose3d)):
        nn.init.normal_(m.weight, 0.0, 0.02)
    elif isinstance(m, nn.BatchNorm3d):
        nn.init.normal_(m.weight, 1.0, 0.02)
        nn.init.constant_(m.bias, 0)


class _Block(nn.Module):
    """Conv3d(3, padding 1) -> BatchNorm3d -> ReLU (parameter holder)"""

    def __init__(self, cin: int, cout: int):
        super().__init__()
        self.proj = nn.Conv3d(cin, cout, 3, padding=1)
        self.norm = nn.BatchNorm3d(cout)


class _DoubleBlock(nn.Module):
    """the reference's non-residual ResnetBlock: block2(block1(x))"""

    def __init__(self, cin: int, cout: int):
        super().__init__()
        self.block1 = _Block(cin, cout)
        self.block2 = _Block(cout, cout)


class _Bottleneck(nn.Module):
    def __init__(self, c: int):
        super().__init__()
        self.block = _DoubleBlock(c, c)


class Unet3d(NativeModule, nn.Module):
    """MI355X-native FNet3D (see module docstring).  ``compute_dtype``: None -> bf16 under ``torch.autocast(bfloat16)``, fp32
    otherwise; or force ``torch.bfloat16`` / ``torch.float32``.  All of D, H and W must be divisible by ``2**depth``."""

    def __init__(self, in_channels: int = 1, out_channels: int = 1, depth: int = 4, mult_chan: int = 32,
                 in_stack_depth: int | None = None) -> None:
        super().__init__()
        if depth < 1:
            raise ValueError(f"depth must be >= 1, got {depth}")
        dims = [mult_chan * 2 ** i for i in range(depth + 1)]
        self.dims = dims
        self.in_channels, self.out_channels = in_channels, out_channels
        self._divisor = 2 ** depth
        self.downsamples_z = True
        self.inconv = nn.Conv3d(in_channels, dims[0], 3, padding=1)
        self._encoder_blocks = nn.ModuleList(nn.ModuleList([_DoubleBlock(dims[i], dims[i])]) for i in range(depth))
        self._downsamples = nn.ModuleList(nn.Conv3d(dims[i], dims[i + 1], 3, stride=2, padding=1) for i in range(depth))
        self.bottleneck = _Bottleneck(dims[-1])
        self._upsamples = nn.ModuleList(
            nn.ConvTranspose3d(dims[i + 1], dims[i], 3, stride=2, padding=1, output_padding=1) for i in reversed(range(depth)))
        self._decoder_blocks = nn.ModuleList(nn.ModuleList([_DoubleBlock(2 * dims[i], dims[i])]) for i in reversed(range(depth)))
        self.outconv = nn.Conv3d(dims[0], out_channels, 3, padding=1)
        self.in_stack_depth = in_stack_depth
        self.out_stack_depth = in_stack_depth
        self.apply(_fnet_weights_init)

    @property
    def num_blocks(self) -> int:
        """number of spatial downsampling stages"""
        return len(self._encoder_blocks)

    def check_input(self, x: Tensor) -> None:
        for name, size in zip(("D", "H", "W"), x.shape[2:]):
            if size % self._divisor != 0:
                raise ValueError(f"Spatial dim {name}={size} must be divisible by {self._divisor} (2^{self.num_blocks} levels).")

    def _engine_class(self):
        from .engine_unet3d import Engine

        return Engine

    def forward(self, x: Tensor) -> Tensor:
        if x.ndim != 5:
            raise ValueError(f"Expected input with 5 dimensions (B, C, D, H, W), got {tuple(x.shape)}")
        self.check_input(x)
        self._require_hip(x)
        from .engine_unet3d import unet3d_apply

        return unet3d_apply(self, x)
