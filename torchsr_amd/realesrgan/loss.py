"""Real-ESRGAN's perceptual loss (``train --perceptual realesrgan``).

BasicSR's ``PerceptualLoss`` with the options of Real-ESRGAN's ``train_realesrgan_x4plus.yml``: VGG19 features of the
ImageNet-normalised images at ``conv1_2, conv2_2, conv3_4, conv4_4, conv5_4`` BEFORE their ReLU, weighted 0.1, 0.1, 1, 1, 1, L1
criterion, perceptual weight 1, no style term.  The graph is ``vgg19.features[:35]`` -- it ends at ``conv5_4`` with no ReLU
behind it -- with torchvision's child indices, loaded from the same ``vgg19-dcbb9e9d.pth`` as ``srgan.loss.VGGLoss``.

The whole term is one autograd node (``functional.frozen_tap_stack``): in cfg 'E' every tap but the last is the conv in front
of a max-pool, ReLU and max commute, so a tap conv writes its pre-activation once and the pool behind it applies the ReLU and
sums ``|fs - ft|`` on the way.
"""
import warnings
from typing import List, Optional

import torch
from torch import nn, Tensor

from .. import functional as F
from ..layers import ACT_NONE, ACT_RELU, Conv2d, Marker
from ..srgan.loss import VGG19_CFG, VGG19_FILE, MaxPool2x2, _find_weights

LAYER_WEIGHTS = {'conv1_2': 0.1, 'conv2_2': 0.1, 'conv3_4': 1.0, 'conv4_4': 1.0, 'conv5_4': 1.0}
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def vgg19_conv_names() -> List[str]:
    """``conv1_1 .. conv5_4`` in cfg 'E' order."""
    names, block, k = [], 1, 0
    for v in VGG19_CFG:
        if v == 'M':
            block, k = block + 1, 0
        else:
            k += 1
            names.append(f'conv{block}_{k}')
    return names


def make_vgg19_tap_features(layer_weights=None) -> nn.Sequential:
    """``vgg19().features[:35]`` with the same child indices (conv at 0, 2, 5, ..., 34): a conv named in ``layer_weights``
    writes its pre-activation (act NONE; the ``Marker`` behind it stands for the ReLU the pool applies), every other conv keeps
    the fused ReLU."""
    taps = LAYER_WEIGHTS if layer_weights is None else layer_weights
    names, layers, cin = iter(vgg19_conv_names()), [], 3
    for v in VGG19_CFG:
        if v == 'M':
            layers.append(MaxPool2x2())
        else:
            tap = next(names) in taps
            layers += [Conv2d(cin, v, kernel_size=3, stride=1, padding=1, act=ACT_NONE if tap else ACT_RELU),
                       Marker('ReLU (in the pool behind a tap)' if tap else 'ReLU (conv epilogue)')]
            cin = v
    return nn.Sequential(*layers[:35])


class PerceptualLoss(nn.Module):
    """``PerceptualLoss()``; ``forward(source, target) -> 0-dim loss``: ``sum_k w_k * l1(f_k(norm(source)), f_k(norm(target)))``.

    The features are frozen and in eval mode; ``weights`` / ``seed`` are ``VGGLoss``'s: a path to ``vgg19-dcbb9e9d.pth`` (default:
    ``$TORCHSR_VGG19_WEIGHTS``, then the torch hub cache), or ``'random'`` for seeded random features."""

    layer_weights = LAYER_WEIGHTS
    mean, std = IMAGENET_MEAN, IMAGENET_STD

    def __init__(self, weights: Optional[str] = None, seed: int = 1234) -> None:
        super().__init__()
        self.features = make_vgg19_tap_features(self.layer_weights).eval()
        path = None if weights == 'random' else _find_weights(weights)
        if path is not None:
            state = torch.load(path, map_location='cpu')
            own = self.features.state_dict()
            picked = {k[len('features.'):]: v for k, v in state.items()
                      if k.startswith('features.') and k[len('features.'):] in own}
            self.features.load_state_dict(picked, strict=True)
            self.pretrained = True
        else:
            if weights != 'random':  # 'random' is the explicit opt-in of benchmarks, tests and `--vgg-weights random`
                warnings.warn(f'{VGG19_FILE} not found (pass weights=, or set TORCHSR_VGG19_WEIGHTS): PerceptualLoss uses '
                              'seeded random features', stacklevel=2)
            g = torch.Generator().manual_seed(seed)
            for m in self.features:
                if isinstance(m, Conv2d):
                    fan_out = m.out_channels * m.kernel_size[0] * m.kernel_size[1]
                    with torch.no_grad():
                        m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_out) ** 0.5)
                        m.bias.zero_()
            self.pretrained = False
        for _, param in self.features.named_parameters():
            param.requires_grad = False

    def _stack(self):
        """``(layers, taps)`` of ``functional.frozen_tap_stack``: the stack without its markers, tap position -> weight."""
        layers = [('pool', None) if isinstance(m, MaxPool2x2) else ('conv', m) for m in self.features if not isinstance(m, Marker)]
        convs = [i for i, (kind, _) in enumerate(layers) if kind == 'conv']
        taps = {convs[j]: self.layer_weights[name] for j, name in enumerate(vgg19_conv_names()[:len(convs)])
                if name in self.layer_weights}
        return layers, taps

    @torch.no_grad()
    def target_features(self, target: Tensor) -> List[Tensor]:
        """The five pre-ReLU features of the detached branch, shallow to deep, NHWC; no autograd state."""
        layers, taps = self._stack()
        return F.frozen_tap_features(F.to_nhwc(target, 4), layers, taps, self.mean, self.std)

    def forward(self, source: Tensor, target: Tensor = None, target_features: List[Tensor] = None) -> Tensor:
        """The loss of NCHW images in [0, 1].  ``target_features`` may carry ``target_features(target)`` in place of ``target``."""
        with torch.no_grad():
            tgt4 = None if target is None else F.to_nhwc(target, 4)
        return self.forward_nhwc(F.to_nhwc(source, 4), tgt4, target_features)

    def forward_nhwc(self, src4: Tensor, tgt4: Tensor = None, target_features: List[Tensor] = None) -> Tensor:
        """``forward`` on NHWC ``[N,H,W,4]`` images (4th channel zero), as the trainers call it."""
        layers, taps = self._stack()
        if target_features is not None:
            return F.frozen_tap_stack(src4, None, layers, taps, self.mean, self.std, target_features=target_features)
        return F.frozen_tap_stack(src4, tgt4.detach(), layers, taps, self.mean, self.std)
