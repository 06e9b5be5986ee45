"""A torch CPU restatement of RRDBNet, written from its architecture description:

    [scale 2: reflect-pad an odd axis by one row / column at the bottom / right, pixel_unshuffle(2)]
    conv_first 3x3 (3 or 12 -> 64);  num_block x RRDB;  conv_body 3x3;  + conv_first's output
    nearest x2, conv_up1 3x3, LeakyReLU(0.2);  nearest x2, conv_up2 3x3, LeakyReLU(0.2)
    conv_hr 3x3, LeakyReLU(0.2);  conv_last 3x3 (64 -> 3)        [scale 2: crop to 2h x 2w]

    RRDB: x + 0.2 rdb3(rdb2(rdb1(x)));   dense block: convk sees cat(x, x1 .. x(k-1)), k <= 4 with LeakyReLU(0.2) and 32
    outputs, conv5 64 outputs, result x + 0.2 conv5(...)

Stock ``torch.nn`` modules only, under BasicSR's module names -- ``state_dict()`` is a published-format state (the keys of
``RealESRGAN_x4plus.pth``'s ``params_ema``) -- so it runs in fp32 and, after ``.double()``, in fp64: the tests' reference and
the measure of fp32's own distance from fp64.
"""
from collections import OrderedDict

import torch
import torch.nn.functional as TF
from torch import nn


class _DenseBlock(nn.Module):
    def __init__(self, num_feat=64, num_grow_ch=32):
        super().__init__()
        for k in range(1, 5):
            setattr(self, f'conv{k}', nn.Conv2d(num_feat + (k - 1) * num_grow_ch, num_grow_ch, 3, 1, 1))
        self.conv5 = nn.Conv2d(num_feat + 4 * num_grow_ch, num_feat, 3, 1, 1)

    def forward(self, x):
        feats = [x]
        for k in range(1, 5):
            feats.append(TF.leaky_relu(getattr(self, f'conv{k}')(torch.cat(feats, 1)), 0.2))
        return x + 0.2 * self.conv5(torch.cat(feats, 1))


class _RRDB(nn.Module):
    def __init__(self, num_feat=64, num_grow_ch=32):
        super().__init__()
        self.rdb1, self.rdb2, self.rdb3 = (_DenseBlock(num_feat, num_grow_ch) for _ in range(3))

    def forward(self, x):
        return x + 0.2 * self.rdb3(self.rdb2(self.rdb1(x)))


class RRDBNetRef(nn.Module):
    def __init__(self, num_block: int = 23, scale: int = 4, num_feat: int = 64, num_grow_ch: int = 32):
        super().__init__()
        self.scale = scale
        self.conv_first = nn.Conv2d(3 * (4 // scale) ** 2, num_feat, 3, 1, 1)
        self.body = nn.Sequential(*[_RRDB(num_feat, num_grow_ch) for _ in range(num_block)])
        self.conv_body = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_up1 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_up2 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_hr = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_last = nn.Conv2d(num_feat, 3, 3, 1, 1)

    def forward(self, x):
        h, w = x.shape[-2:]
        if self.scale == 2:
            x = TF.pixel_unshuffle(TF.pad(x, (0, w & 1, 0, h & 1), mode='reflect'), 2)
        feat = self.conv_first(x)
        feat = feat + self.conv_body(self.body(feat))
        feat = TF.leaky_relu(self.conv_up1(TF.interpolate(feat, scale_factor=2, mode='nearest')), 0.2)
        feat = TF.leaky_relu(self.conv_up2(TF.interpolate(feat, scale_factor=2, mode='nearest')), 0.2)
        out = self.conv_last(TF.leaky_relu(self.conv_hr(feat), 0.2))
        return out[..., :h * self.scale, :w * self.scale]


def seeded_state(ref: nn.Module, seed: int = 0) -> OrderedDict:
    """Non-degenerate weights and biases: conv weights at He scale -- the dense blocks' at 0.1 x that, so that the 0.2-scaled
    residuals neither vanish nor explode -- and biases spread over [-0.1, 0.1] (zero biases would hide a bias read from the
    wrong channel)."""
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for k, v in ref.state_dict().items():
        if v.dim() == 4:
            gain = 0.1 if '.rdb' in k else 1.0
            sd[k] = torch.randn(v.shape, generator=g) * gain * (2.0 / (1.04 * v.shape[1] * 9)) ** 0.5
        else:
            sd[k] = (torch.rand(v.shape, generator=g) - 0.5) * 0.2
    return sd


def xinntao_names(state) -> OrderedDict:
    """The same tensors under the key names of xinntao/ESRGAN's "new arch" files."""
    ren = {'conv_body': 'trunk_conv', 'conv_up1': 'upconv1', 'conv_up2': 'upconv2', 'conv_hr': 'HRconv'}
    out = OrderedDict()
    for k, v in state.items():
        p = k.split('.')
        if p[0] == 'body':
            p = ['RRDB_trunk', p[1], p[2].upper()] + p[3:]
        else:
            p[0] = ren.get(p[0], p[0])
        out['.'.join(p)] = v
    return out
