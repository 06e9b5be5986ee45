"""A torch CPU restatement of the compact generator (SRVGGNetCompact), written from its architecture description:

    conv3x3(3 -> F) + PReLU(F);  num_conv x [conv3x3(F -> F) + PReLU(F)];  conv3x3(F -> 3 s^2), PixelShuffle(s), + nearest x s (input)

Stock ``torch.nn`` modules only, so it runs in fp32 and, after ``.double()``, in fp64: the tests' reference and the measure
of fp32's own distance from fp64.  ``rounded_forward`` restates the 16-bit inference chain: weights and stored activations
rounded to bf16 / fp16, sums exact (fp64).
"""
import torch
import torch.nn.functional as TF
from torch import nn


class CompactRef(nn.Module):
    def __init__(self, scale_factor: int = 4, num_feat: int = 64, num_conv: int = 32):
        super().__init__()
        self.scale_factor = scale_factor
        body = [nn.Conv2d(3, num_feat, 3, 1, 1), nn.PReLU(num_parameters=num_feat)]
        for _ in range(num_conv):
            body += [nn.Conv2d(num_feat, num_feat, 3, 1, 1), nn.PReLU(num_parameters=num_feat)]
        body.append(nn.Conv2d(num_feat, 3 * scale_factor ** 2, 3, 1, 1))
        self.body = nn.ModuleList(body)

    def forward(self, x):
        out = x
        for m in self.body:
            out = m(out)
        return TF.pixel_shuffle(out, self.scale_factor) + TF.interpolate(x, scale_factor=self.scale_factor, mode='nearest')


def seeded_state(ref: nn.Module, seed: int = 0):
    """A state with conv weights at He scale and slopes spread over [-0.2, 0.6] (some negative, some above 0.5) -- the default
    initialisation's equal slopes 0.25 would hide a slope read from the wrong channel."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in ref.state_dict().items():
        if v.dim() == 4:
            sd[k] = torch.randn(v.shape, generator=g) * (2.0 / (1.1 * v.shape[1] * 9)) ** 0.5
        elif k.endswith('.bias'):
            sd[k] = (torch.rand(v.shape, generator=g) - 0.5) * 0.2
        else:
            sd[k] = torch.rand(v.shape, generator=g) * 0.8 - 0.2
    return sd


def rounded_forward(sd, x, scale: int, rnd):
    """The 16-bit inference chain in fp64: ``rnd`` rounds to the storage type (``lambda t: t.bfloat16().double()`` or
    ``.half()``).  The first conv multiplies the rounded image by its rounded weights (what the 3x3 input conv does at either
    16-bit precision) into an fp32 tensor that is activated in fp32 and rounded once; every later layer rounds once behind bias and activation; the last conv's rounded output meets the fp32
    image in the tail."""
    n = max(int(k.split('.')[1]) for k in sd)
    d = {k: v.double() for k, v in sd.items()}
    out = x.double()
    for i in range(0, n, 2):
        z = TF.conv2d(rnd(out), rnd(d[f'body.{i}.weight']), d[f'body.{i}.bias'], 1, 1)
        if i == 0:
            z = z.float().double()
        a = d[f'body.{i + 1}.weight'].view(1, -1, 1, 1)
        out = rnd(torch.where(z > 0, z, a * z))
    z = rnd(TF.conv2d(out, rnd(d[f'body.{n}.weight']), d[f'body.{n}.bias'], 1, 1))
    return TF.pixel_shuffle(z, scale) + TF.interpolate(x.double(), scale_factor=scale, mode='nearest')
