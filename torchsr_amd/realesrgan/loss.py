"""Real-ESRGAN's perceptual loss (``train --perceptual realesrgan``).

BasicSR's ``PerceptualLoss`` with the options of Real-ESRGAN's ``train_realesrgan_x4plus.yml``: VGG19 features of the
ImageNet-normalised images at ``conv1_2, conv2_2, conv3_4, conv4_4, conv5_4`` BEFORE their ReLU, weighted 0.1, 0.1, 1, 1, 1, L1
criterion, perceptual weight 1, no style term.  The graph is ``vgg19.features[:35]`` -- it ends at ``conv5_4`` with no ReLU
behind it -- with torchvision's child indices, loaded from the same ``vgg19-dcbb9e9d.pth`` as ``srgan.loss.VGGLoss``.

The whole term is one autograd node (``functional.frozen_tap_stack``): in cfg 'E' every tap but the last is the conv in front
of a max-pool, ReLU and max commute, so a tap conv writes its pre-activation once and the pool behind it applies the ReLU and
sums ``|fs - ft|`` on the way.
"""
from typing import List, Optional

import torch
from torch import nn, Tensor

from .. import functional as F
from ..srgan.loss import load_frozen_vgg19, stack_layers, vgg19_conv_names, vgg19_layers

LAYER_WEIGHTS = {'conv1_2': 0.1, 'conv2_2': 0.1, 'conv3_4': 1.0, 'conv4_4': 1.0, 'conv5_4': 1.0}
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def make_vgg19_tap_features(layer_weights=None) -> nn.Sequential:
    """``vgg19().features[:35]`` with the same child indices (conv at 0, 2, 5, ..., 34): a conv named in ``layer_weights``
    writes its pre-activation, every other conv keeps the fused ReLU (``srgan.loss.vgg19_layers``)."""
    return nn.Sequential(*vgg19_layers(LAYER_WEIGHTS if layer_weights is None else layer_weights)[:35])


class PerceptualLoss(nn.Module):
    """``PerceptualLoss()``; ``forward(source, target) -> 0-dim loss``: ``sum_k w_k * l1(f_k(norm(source)), f_k(norm(target)))``.

    The features are frozen and in eval mode; ``weights`` / ``seed`` are ``VGGLoss``'s: a path to ``vgg19-dcbb9e9d.pth`` (default:
    ``$TORCHSR_VGG19_WEIGHTS``, then the torch hub cache), or ``'random'`` for seeded random features."""

    layer_weights = LAYER_WEIGHTS
    mean, std = IMAGENET_MEAN, IMAGENET_STD

    def __init__(self, weights: Optional[str] = None, seed: int = 1234) -> None:
        super().__init__()
        self.features = make_vgg19_tap_features(self.layer_weights).eval()
        self.pretrained = load_frozen_vgg19(self.features, weights, seed, 'PerceptualLoss')

    def _stack(self):
        """``(layers, taps)`` of ``functional.frozen_tap_stack``: the stack without its markers, tap position -> weight."""
        layers = stack_layers(self.features)
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
