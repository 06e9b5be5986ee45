"""Real-ESRGAN's U-Net discriminator with spectral normalisation (``UNetDiscriminatorSN``): one realness logit per pixel.

Three stride-2 4x4 convs down, three bilinear x2 steps up with additive skips, two more 3x3 convs and a 64 -> 1 output conv;
every conv but the first and the last is spectrally normalised and has no bias, every activation is LeakyReLU(0.2), and there
is no BatchNorm.  ``state_dict()`` has the keys of torch's ``spectral_norm`` wrapper (``convK.weight_orig`` / ``weight_u`` /
``weight_v``), so Real-ESRGAN's published ``*_netD.pth`` files load key for key.  It is trained with the plain GAN loss.
"""
import torch
from torch import nn, Tensor

from .. import functional as F
from ..layers import ACT_LRELU, Conv2d, SNConv2d


class UNetDiscriminatorSN(nn.Module):
    """``UNetDiscriminatorSN(num_in_ch=3, num_feat=64, skip_connection=True)``; ``forward([N,3,H,W]) -> [N,1,H,W]`` logits.
    H and W must be multiples of 8."""

    def __init__(self, num_in_ch: int = 3, num_feat: int = 64, skip_connection: bool = True) -> None:
        super().__init__()
        self.skip_connection = skip_connection
        f = num_feat
        lrelu = {'act': ACT_LRELU, 'slope': 0.2}
        self.conv0 = Conv2d(num_in_ch, f, kernel_size=3, stride=1, padding=1, **lrelu)
        self.conv1 = SNConv2d(f, f * 2, 4, 2, 1, **lrelu)
        self.conv2 = SNConv2d(f * 2, f * 4, 4, 2, 1, **lrelu)
        self.conv3 = SNConv2d(f * 4, f * 8, 4, 2, 1, **lrelu)
        self.conv4 = SNConv2d(f * 8, f * 4, 3, 1, 1, **lrelu)
        self.conv5 = SNConv2d(f * 4, f * 2, 3, 1, 1, **lrelu)
        self.conv6 = SNConv2d(f * 2, f, 3, 1, 1, **lrelu)
        self.conv7 = SNConv2d(f, f, 3, 1, 1, **lrelu)
        self.conv8 = SNConv2d(f, f, 3, 1, 1, **lrelu)
        self.conv9 = Conv2d(f, 1, kernel_size=3, stride=1, padding=1)

    def forward_nhwc(self, x4: Tensor) -> Tensor:
        """NHWC ``[N,H,W,4]`` in, ``[N,H,W,4]`` out: channel 0 is the logit, the other three are padding."""
        n, h, w, _ = x4.shape
        if h % 8 or w % 8:
            raise ValueError(f'UNetDiscriminatorSN: height and width must be multiples of 8 (three stride-2 levels whose skips '
                             f'have to line up), got {h} x {w}')
        skip = (lambda up, down: F.axpby(up, down, 1.0, 1.0)) if self.skip_connection else (lambda up, down: up)
        x0 = self.conv0(x4)
        x1 = self.conv1(x0)
        x2 = self.conv2(x1)
        x3 = self.conv3(x2)
        x4_ = skip(self.conv4(F.upsample_bilinear2x(x3)), x2)
        x5 = skip(self.conv5(F.upsample_bilinear2x(x4_)), x1)
        x6 = skip(self.conv6(F.upsample_bilinear2x(x5)), x0)
        x6 = F.cut_point('d.head', x6)  # data parallel: conv7 .. conv9 complete first in the backward pass
        out = self.conv8(self.conv7(x6))
        return self.conv9(out)

    def logits_nhwc(self, x4: Tensor) -> Tensor:
        """``[N,1,H,W]`` logits: the padding channels of the 1-channel output never reach a loss."""
        return F.to_nchw(self.forward_nhwc(x4), 1)

    def forward(self, x: Tensor) -> Tensor:
        if x.dim() != 4 or x.shape[2] % 8 or x.shape[3] % 8:
            raise ValueError(f'UNetDiscriminatorSN: expected [N, C, H, W] with H and W multiples of 8, got {tuple(x.shape)}')
        return self.logits_nhwc(F.to_nhwc(x, F.round4(x.shape[1])))

    # ---- what the trainer calls (the plain, non-relativistic GAN loss of Real-ESRGAN); same surface as esrgan/discriminator.py
    def pair_loss_nhwc(self, real4: Tensor, fake4: Tensor):
        """``BCEWithLogits(D(real), 1) + BCEWithLogits(D(fake), 0)``, each a mean over all N*H*W logits; ``(loss, aux)``.  Real
        and fake run as ONE batch of 2N (no BatchNorm: nothing couples the samples), so a training-mode call is ONE power
        iteration of every normalised layer, where two separate calls would be two."""
        n = real4.shape[0]
        if fake4.shape != real4.shape:
            raise ValueError(f'pair_loss_nhwc: real {tuple(real4.shape)} and fake {tuple(fake4.shape)} batches differ in shape')
        real, fake = F.split_batch(self.logits_nhwc(torch.cat([real4, fake4], dim=0)), n)
        loss_real, loss_fake = F.bce_with_logits(real, 1.0), F.bce_with_logits(fake, 0.0)
        return F.axpby(loss_real, loss_fake, 1.0, 1.0), (loss_real.detach(), loss_fake.detach())

    def adversarial_loss_nhwc(self, fake4: Tensor, addend: Tensor, weight: float):
        """``addend + weight * BCEWithLogits(D(fake), 1)``; ``(loss, (None, adversarial term))``."""
        adv = F.bce_with_logits(self.logits_nhwc(fake4), 1.0)
        return F.axpby(addend, adv, 1.0, float(weight)), (None, adv.detach())
