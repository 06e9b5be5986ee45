"""GAN training against Real-ESRGAN's U-Net discriminator (``train --discriminator unet``).

A mixin over ``ESRGANTrainer`` / ``CompactTrainer``: the generator, the content terms (``0.01 L1 + VGG``), the amp phases, the
flat Adam and the hipGraph capture stay the base trainer's.  What changes is the critic and its loss: ``UNetDiscriminatorSN``
returns one logit per pixel and is trained with the plain GAN loss, so the relativistic ``mean(D(real))`` forward of the
generator phase is gone and the adversarial weight is Real-ESRGAN's 0.1.  The order of updates stays this package's -- D first,
then G against the updated D -- so every step runs two training-mode forwards of D (the 2N batch, then the fake batch) and
therefore two power iterations of every normalised layer, as torch's ``spectral_norm`` does per training-mode forward.
"""
from ..compact.trainer import CompactTrainer
from ..esrgan.trainer import ESRGANTrainer
from ..layers import no_weight_grad
from .discriminator import UNetDiscriminatorSN


class UNetDiscriminatorMixin:
    discriminator_cls = UNetDiscriminatorSN
    adversarial_weight = 0.1  # Real-ESRGAN's gan_opt loss_weight for the vanilla loss

    def __init__(self, device, args, train_loader, test_loader, train_len, test_len, distributed: bool = False) -> None:
        if distributed:
            # (not attempted: disc_head_bucket = 'conv7.weight_orig' may be all that is missing, but nothing has run it -- DESIGN.md 7)
            raise RuntimeError('--discriminator unet does not run under a process group yet: its gradient bucket (conv7 .. conv9 '
                               'behind the "d.head" cut) has not been wired into the bucketed exchange or tested; train it on one GPU')
        super().__init__(device, args, train_loader, test_loader, train_len, test_len, distributed)

    # (_phase_disc_loss is the base trainer's: it calls ``discriminator.pair_loss_nhwc``, here BCE(D(real), 1) + BCE(D(fake), 0))

    def _phase_gen(self) -> None:
        """D update, then ``gen_loss = 0.01 L1 + VGG + 0.1 BCEWithLogits(D(fake), 1)`` against the updated D."""
        self.disc_optimizer.step()
        with no_weight_grad():
            gen_loss, aux = self.discriminator.adversarial_loss_nhwc(self._super_res, self._content, self.adversarial_weight)
        self._backward(gen_loss)
        self._losses['gan/adversarial-loss'] = aux[1]
        self._losses['gan/train-loss'] = gen_loss.detach()
        self._super_res = self._content = self._high4 = None


class UNetESRGANTrainer(UNetDiscriminatorMixin, ESRGANTrainer):
    pass


class UNetCompactTrainer(UNetDiscriminatorMixin, CompactTrainer):
    pass
