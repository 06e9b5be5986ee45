"""Parameter-holding layers with the reference's ``state_dict`` schema.

Each class subclasses the stock ``torch.nn`` module the reference instantiates, so
parameter names, shapes, creation order (and therefore seeded default init) are
identical to roclark/torchsr, while ``forward`` runs the MI355X HIP kernels on NHWC
activations.  These layers are the internal (NHWC) building blocks; the public
``Generator`` / ``Discriminator`` / ``VGGLoss`` modules accept and return NCHW like
the reference.
"""
import contextlib

import torch
from torch import nn, Tensor

from . import functional as F
from ._lib import ACT_LRELU, ACT_NONE, ACT_RELU


_frozen = [False]


@contextlib.contextmanager
def no_weight_grad():
    """Run forwards whose parameters take no gradient while activations still do.

    Used for the discriminator pass inside the generator update (torchsr/srgan/trainer.py:456):
    the reference lets autograd compute -- and DDP all-reduce -- discriminator weight gradients
    there that are zeroed before anyone reads them.  Skipping them
    changes no result and removes 28 GFLOP and 94 MB of all-reduce per step.
    """
    old = _frozen[0]
    _frozen[0] = True
    try:
        yield
    finally:
        _frozen[0] = old


def _w(p):
    return p.detach() if (_frozen[0] and p is not None) else p


class Conv2d(nn.Conv2d):
    """nn.Conv2d on NHWC activations with an optional fused epilogue.

    ``act``: fused ReLU / LeakyReLU after the bias; ``shuffle=2`` fuses the
    ``nn.PixelShuffle(2)`` that follows the conv in srgan/residual.py:27-28; ``up=2`` fuses the
    ``F.interpolate(scale_factor=2, mode='nearest')`` that precedes it in esrgan/generator.py:73-78.
    """

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, act=ACT_NONE,
                 slope=0.0, shuffle=0, up=0):
        super().__init__(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=padding,
                         bias=bias)
        self._st = F.ConvState(in_channels, out_channels, kernel_size, stride, padding, shuffle=shuffle, act=act,
                               slope=slope, up=up)

    def forward(self, x: Tensor, want_stats: bool = False, in_act=None, act_bwd_folded=None):
        """``in_act`` / ``act_bwd_folded``: a consumer / producer pair of flags that moves the backward of the producer's
        fused activation into the consumer's data gradient (``functional._Conv2d.forward``)."""
        if self._st.precision == F.PRECISION_F16 and not F.inference_mode(self):
            raise RuntimeError('Conv2d: fp16 precision (3) is inference-only (eval mode, no autograd); '
                               "train with 'fp32' or 'bf16'")
        y, part = F.conv2d(x, _w(self.weight), _w(self.bias), self._st, want_stats, self.weight, in_act, act_bwd_folded)
        return (y, part) if want_stats else y

    def __deepcopy__(self, memo):
        new = Conv2d(self.in_channels, self.out_channels, self.kernel_size[0], self.stride[0], self.padding[0],
                     self.bias is not None, self._st.act, self._st.slope, self._st.shuffle, self._st.up)
        new.load_state_dict(self.state_dict())
        return new


class Unshuffle2Conv2d(Conv2d):
    """RRDBNet's input layer at x2: ``nn.Conv2d(12, 64, 3, 1, 1)`` behind ``pixel_unshuffle(x, 2)``, with that module's
    ``weight`` [64, 12, 3, 3] and ``bias`` -- a published x2 state_dict loads key for key.  ``forward`` takes the NHWC-4 IMAGE
    [N,H,W,4] and returns [N,Hp/2,Wp/2,64] from one launch that gathers the unshuffled (and, for an odd H / W, reflect-padded)
    pixels itself (``functional.unshuffle2_conv``).  By default inference only: training mode or autograd raises.
    ``trainable=True`` asks for the training path: with autograd on the layer is an autograd node with a weight and a bias
    gradient (``srx_unshuffle2_conv_bwd_weight``) and no input gradient -- the input is the image."""

    def __init__(self, trainable: bool = False):
        super().__init__(12, 64, kernel_size=3, stride=1, padding=1)
        self.trainable = bool(trainable)
        if self.trainable:
            self._st.own_pack = None  # packs on every autograd forward; pack tables leave it out (functional.PackTable)

    def forward(self, x4: Tensor) -> Tensor:
        if not self.trainable and not F.inference_mode(self):
            raise RuntimeError('Unshuffle2Conv2d: the x2 input layer is inference-only (eval mode, no autograd) unless it is built '
                               'with trainable=True; the default training path is x4')
        return F.unshuffle2_conv(x4, _w(self.weight), _w(self.bias), self._st, self.trainable)

    def __deepcopy__(self, memo):
        new = Unshuffle2Conv2d(self.trainable)
        new.load_state_dict(self.state_dict())
        return new


class SNConv2d(nn.Module):
    """A bias-free conv under ``torch.nn.utils.spectral_norm`` (one power iteration, eps 1e-12) with that wrapper's
    ``state_dict`` keys: ``weight_orig`` (the Parameter), ``weight_u`` and ``weight_v`` (buffers, updated by every training-mode
    forward).  ``functional.spectral_norm`` writes the normalised weight into one persistent buffer per layer, which the conv
    packs from on every call (``functional.SNConvState``); the conv's weight gradient goes back to autograd as a tensor, and the
    normalisation's backward accumulates into ``weight_orig.grad``.

    One buffer per layer means one live forward per layer: ``D(a); D(b); (la + lb).backward()`` in training mode would take the
    first call's input gradient through the second call's weight, so the conv's backward raises when the layer has run forward
    again since (torch's wrapper keeps a weight per call).  Run the two inputs as one batch, as ``pair_loss_nhwc`` does, or
    finish a call's backward before the next forward, as the trainer's phases do."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, act=ACT_NONE, slope=0.0):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        self.stride, self.padding = stride, padding
        conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding, bias=False)  # torch's default init
        self.weight_orig = nn.Parameter(conv.weight.detach().clone())
        rows, cols = out_channels, in_channels * kernel_size * kernel_size
        # (torch.nn.utils.spectral_norm's start: u ~ N(0, 1) normalised, v = normalize(W^T u))
        u = nn.functional.normalize(torch.randn(rows), dim=0, eps=1e-12)
        v = nn.functional.normalize(self.weight_orig.detach().reshape(rows, cols).t().mv(u), dim=0, eps=1e-12)
        self.register_buffer('weight_u', u)
        self.register_buffer('weight_v', v)
        self._st = F.SNConvState(in_channels, out_channels, kernel_size, stride, padding, act=act, slope=slope)
        self._w_sn = None

    def normalised_weight(self) -> Tensor:
        """One ``functional.spectral_norm`` call (training mode: with its power iteration) into the layer's buffer."""
        w = self.weight_orig
        if self._w_sn is None or self._w_sn.device != w.device:
            self._w_sn = torch.empty(w.shape, dtype=torch.float32, device=w.device)
        self._st.sn_calls += 1
        return F.spectral_norm(_w(w), self.weight_u, self.weight_v, self._w_sn, self.training, w)

    def forward(self, x: Tensor) -> Tensor:
        w_sn = self.normalised_weight()
        return F.conv2d(x, w_sn, None, self._st, False, w_sn)[0]

    def extra_repr(self) -> str:
        return (f'{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, '
                f'padding={self.padding}, spectral norm')


def set_conv_precision(module: nn.Module, precision: str) -> None:
    """``'bf16'``: every conv of ``module`` multiplies bf16-rounded operands and accumulates in fp32 (forward
    and stride-1 data gradient) -- this package's reading of the reference's ``autocast`` region
    (srgan/trainer.py:379-383).  ``'fp32'`` restores exact fp32."""
    p = {'fp32': 0, 'bf16': 1}[precision]
    for m in module.modules():
        if isinstance(m, (Conv2d, SNConv2d)):
            m._st.precision = p


class BatchNorm2d(nn.BatchNorm2d):
    """nn.BatchNorm2d parameter holder; applied through ``functional.bn_act``."""

    def forward(self, y: Tensor, part=None, act=ACT_NONE, slope=0.0, prelu=None, residual=None, groups: int = 1) -> Tensor:
        return F.bn_act(y, part, self, act=act, slope=slope, prelu=_w(prelu), residual=residual, frozen=_frozen[0],
                        groups=groups)


class PReLU(nn.PReLU):
    def forward(self, x: Tensor) -> Tensor:
        if self.weight.numel() > 1:  # nn.PReLU(C): one slope per channel (the compact generator)
            return F.prelu_channels(x, _w(self.weight))
        return F.prelu(x, _w(self.weight))


class LeakyReLU(nn.LeakyReLU):
    def forward(self, x: Tensor) -> Tensor:
        return F.leaky_relu(x, self.negative_slope)


class Linear(nn.Linear):
    def forward(self, x: Tensor, act=ACT_NONE, slope=0.0) -> Tensor:
        return F.linear(x, _w(self.weight), _w(self.bias), act, slope)


class Marker(nn.Module):
    """Placeholder keeping ``nn.Sequential`` indices equal to the reference's when the op it
    stands for (ReLU / LeakyReLU / Sigmoid / PixelShuffle) is fused into a neighbouring kernel."""

    def __init__(self, what: str):
        super().__init__()
        self.what = what

    def extra_repr(self) -> str:
        return f'fused {self.what}'

    def forward(self, x):
        return x


__all__ = ['no_weight_grad', 'Conv2d', 'Unshuffle2Conv2d', 'SNConv2d', 'BatchNorm2d', 'PReLU', 'LeakyReLU', 'Linear', 'Marker', 'ACT_NONE',
           'ACT_RELU', 'ACT_LRELU']
