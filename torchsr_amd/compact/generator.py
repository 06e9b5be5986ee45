"""Compact generator: Real-ESRGAN's SRVGGNetCompact (``realesr-general-x4v3``: 32 body convs, ``realesr-animevideov3``: 16).

A plain chain at low resolution, no BatchNorm, no dense blocks::

    conv3x3(3 -> F) + PReLU(F)
    num_conv x [conv3x3(F -> F) + PReLU(F)]
    conv3x3(F -> 3 s^2), PixelShuffle(s), + nearest-enlarged input

Every PReLU has one slope per channel.  The module list and the ``state_dict`` keys are SRVGGNetCompact's (``body.0.weight``,
``body.1.weight`` of shape ``[F]``, ... ``body.{2 num_conv + 2}.weight`` of shape ``[3 s^2, F, 3, 3]``), so published
checkpoints load key for key.
"""
import torch
from torch import nn, Tensor

from .. import _dev
from .. import functional as F
from ..layers import Conv2d, PReLU

NUM_CONV = 32  # realesr-general-x4v3


def tail_index(num_conv: int) -> int:
    """Index in ``body`` of the conv that opens the generator's tail gradient bucket: the second half of the body convs and
    the output conv.  Autograd completes their gradients first; a data-parallel trainer puts them on the wire while the
    first half's backward still runs (``ddp.py``)."""
    return 2 * ((num_conv + 1) // 2) + 2


class Generator(nn.Module):
    """``Generator(scale_factor=4, num_feat=64, num_conv=32)``; ``forward([N,3,h,w]) -> [N,3,s*h,s*w]`` (unclamped)."""

    def __init__(self, scale_factor: int = 4, num_feat: int = 64, num_conv: int = NUM_CONV) -> None:
        super().__init__()
        if scale_factor not in (2, 3, 4):
            raise ValueError(f'compact.Generator: scale_factor must be 2, 3 or 4, got {scale_factor!r}')
        if num_conv < 1 or num_feat < 4 or num_feat % 4:
            raise ValueError(f'compact.Generator: num_conv >= 1 and num_feat a positive multiple of 4, got {num_conv!r}, {num_feat!r}')
        self.scale_factor, self.num_feat, self.num_conv = int(scale_factor), int(num_feat), int(num_conv)
        body = [Conv2d(3, num_feat, kernel_size=3, stride=1, padding=1), PReLU(num_parameters=num_feat)]
        for _ in range(num_conv):
            body += [Conv2d(num_feat, num_feat, kernel_size=3, stride=1, padding=1), PReLU(num_parameters=num_feat)]
        body.append(Conv2d(num_feat, 3 * scale_factor ** 2, kernel_size=3, stride=1, padding=1))
        self.body = nn.ModuleList(body)
        # low-resolution pixels a tile must see beyond its border for tiled inference to equal the untiled result: the
        # receptive field radius (num_conv + 2 convs of radius 1), rounded up to a multiple of 8
        self.halo = -(-(num_conv + 2) // 8) * 8
        self._tail = tail_index(num_conv)

    def native16(self):
        """The storage dtype of the 16-bit-native inference chain, or None (see ``srgan.Generator.native16``): with bf16 or
        fp16 products the 64-channel activations stay in 16 bits from the first PReLU to the tail kernel."""
        if _dev.NO_C64 or not F.inference_mode(self) or self.num_feat != 64:
            return None
        return {1: torch.bfloat16, F.PRECISION_F16: torch.float16}.get(self.body[2]._st.precision)

    def _infer_nhwc(self, x4: Tensor) -> Tensor:
        f = self.__dict__.get('_folded')
        if f is None:
            n = len(self.body)
            f = [F.FoldedConv(self.body[i], None, self.body[i + 1]) for i in range(0, n - 1, 2)]
            f.append(F.FoldedConv(self.body[n - 1], pad16=True))
            f = self.__dict__.setdefault('_folded', f)
        out = f[0](x4)
        dt = self.native16()
        if dt is not None:
            out = F.to_bf16(out) if dt == torch.bfloat16 else F.to_f16(out)
        for layer in f[1:]:
            out = layer(out)
        return F.shuffle_add_nearest(out, x4, self.scale_factor)

    def forward_nhwc(self, x4: Tensor) -> Tensor:
        """NHWC ``[N,h,w,4]`` -> NHWC ``[N,s*h,s*w,4]`` (4th channel zero)."""
        if F.inference_mode(self):
            return self._infer_nhwc(x4)
        if self.body[0]._st.precision == F.PRECISION_F16:
            raise RuntimeError('compact.Generator: fp16 precision (3) is inference-only (eval mode, no autograd)')
        out = x4
        for i, m in enumerate(self.body):
            if i == self._tail:
                out = F.cut_point('g.tail', out)  # data parallel: body.{tail ..} gradients go out first
            out = m(out)  # training: each PReLU is a pass of its own (srx_prelu_channels_*), not a conv epilogue
        return F.shuffle_add_nearest(out, x4, self.scale_factor)

    def forward(self, x: Tensor) -> Tensor:
        return F.to_nchw(self.forward_nhwc(F.to_nhwc(x, 4)), 3)
