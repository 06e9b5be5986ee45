"""ESRGAN generator (RRDBNet) -- interface of torchsr/esrgan/generator.py:32-81."""

import torch
from torch import nn, Tensor

from .. import _dev
from .. import functional as F
from ..layers import ACT_LRELU, Conv2d, Marker, Unshuffle2Conv2d
from .residual import ResidualInResidualDenseBlock

NUM_RESIDUAL = 23  # torchsr/esrgan/generator.py:20


class Generator(nn.Module):
    """``Generator(num_rrdb_blocks=23, scale_factor=4)``; ``forward([N,3,h,w]) -> [N,3,4h,4w]``.

    No BatchNorm, no PixelShuffle: two nearest-neighbour x2 upsamples, each followed by a
    conv + LeakyReLU; the upsampled tensors are never written (the conv gathers pixel (h >> 1, w >> 1))
    and the LeakyReLU is the conv's epilogue.

    ``scale_factor=2`` is RRDBNet at x2 (``RealESRGAN_x2plus``): the same trunk behind ``pixel_unshuffle(x, 2)``, so ``conv1``
    takes 12 channels at half the resolution (``weight`` [64, 12, 3, 3], RRDBNet's own shape) and the two x2 stages end at
    ``[N,3,2h,2w]``.  The unshuffle is the gather of ``conv1``'s kernel (``layers.Unshuffle2Conv2d``); an odd h or w (at least 3)
    is padded there by one reflected row / column at the bottom / right, as ``RealESRGANer.pre_process`` pads, and the result is
    cropped back to ``[2h, 2w]``.  By default x2 is inference-only: a training-mode or autograd-enabled forward raises
    ``RuntimeError``.  ``trainable=True`` builds ``conv1`` with its weight gradient (``Unshuffle2Conv2d(trainable=True)``) and
    lifts that refusal; at ``scale_factor=4`` the flag is accepted and changes nothing.
    """

    # tiled inference (torchsr_amd/test.py): the true receptive field radius is ~350 low-resolution pixels, more than a
    # tile can carry, so ESRGAN tiling is approximate near tile borders
    halo = 64

    def __init__(self, num_rrdb_blocks: int = NUM_RESIDUAL, scale_factor: int = 4, trainable: bool = False) -> None:
        super().__init__()
        if scale_factor not in (2, 4):
            raise ValueError(f'esrgan.Generator: scale_factor must be 4 or 2 (RRDBNet behind pixel_unshuffle(2)), got {scale_factor!r}')
        self.scale_factor, self.trainable = scale_factor, bool(trainable)
        if scale_factor == 2:
            # tiles of the image: the trunk's 64 pixels of halo are 128 of the image's, and even tile origins keep a tile's
            # unshuffle phase the whole image's (test.upscale rounds tile sizes and the halo up to multiples of tile_align)
            self.halo, self.tile_align = 128, 2
            self.conv1 = Unshuffle2Conv2d(self.trainable)
        else:
            self.conv1 = Conv2d(3, 64, kernel_size=3, stride=1, padding=1)
        self.blocks = nn.Sequential(*[ResidualInResidualDenseBlock(channels=64, growth_channels=32, scale_ratio=0.2)
                                      for _ in range(num_rrdb_blocks)])
        self.conv2 = Conv2d(64, 64, kernel_size=3, stride=1, padding=1)
        self.upsample1 = Conv2d(64, 64, kernel_size=3, stride=1, padding=1, act=ACT_LRELU, slope=0.2, up=2)
        self.upsample2 = Conv2d(64, 64, kernel_size=3, stride=1, padding=1, act=ACT_LRELU, slope=0.2, up=2)
        self.conv3 = nn.Sequential(Conv2d(64, 64, kernel_size=3, stride=1, padding=1, act=ACT_LRELU, slope=0.2),
                                   Marker('LeakyReLU(0.2) (conv epilogue)'))
        self.conv4 = Conv2d(64, 3, kernel_size=3, stride=1, padding=1)

    def forward_nhwc(self, x4: Tensor) -> Tensor:
        conv1 = self.conv1(x4)
        # the RRDB chain is one autograd node (functional._RRDBTrunk): every dense block finds its input where the
        # block before wrote it; the modules in self.blocks hold the parameters (and run one by one when called alone)
        conv2 = self.conv2(F.rrdb_trunk(conv1, list(self.blocks)))   # :70
        out = F.axpby(conv1, conv2, 1.0, 1.0)                       # torch.add, generator.py:72
        out = F.cut_point('g.tail', out)                            # data parallel: upsample* / conv3 / conv4 gradients go out first
        out = self.upsample1(out)                                   # :73-75 (nearest x2 in the conv's gather)
        # upsample2's LeakyReLU backward rides in conv3's data gradient (its output feeds conv3 and nothing else)
        fold = torch.is_grad_enabled() and self.upsample2._st.act == ACT_LRELU and not _dev.NO_ACT_FOLD
        token = F.ActFold(ACT_LRELU, self.upsample2._st.slope) if fold else None  # producer skips, consumer masks
        out = self.upsample2(out, act_bwd_folded=token)             # :76-78
        return self.conv4(self.conv3[0](out, in_act=token))         # :79-80

    def forward(self, x: Tensor) -> Tensor:
        if self.scale_factor == 2:
            if not self.trainable and not F.inference_mode(self):
                raise RuntimeError('esrgan.Generator(scale_factor=2) is inference-only (eval mode, no autograd) unless it is built '
                                   'with trainable=True; the default training path is x4')
            h, w = int(x.shape[-2]), int(x.shape[-1])
            if (h & 1 and h < 3) or (w & 1 and w < 3):
                raise RuntimeError(f'esrgan.Generator(scale_factor=2): an odd height or width is padded by reflection and must be '
                                   f'at least 3, got {h} x {w}')
            out = F.to_nchw(self.forward_nhwc(F.to_nhwc(x, 4)), 3)  # [N, 3, 2 (h + (h & 1)), 2 (w + (w & 1))]
            return out if not (h & 1 or w & 1) else out[:, :, :2 * h, :2 * w].contiguous()
        return F.to_nchw(self.forward_nhwc(F.to_nhwc(x, 4)), 3)
