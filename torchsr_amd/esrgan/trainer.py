"""ESRGAN trainer on MI355X -- interface of torchsr/esrgan/trainer.py:39-560.

Same skeleton as the SRGAN trainer (shared host loop, checkpoints, PSNR test, hipGraph capture,
flat Adam, bucketed RCCL gradient exchange); differences follow the reference:

* pre-training minimises L1 instead of MSE (esrgan/trainer.py:163,385);
* relativistic-average GAN losses on logits, ``BCEWithLogits(real - mean(fake), 1)`` etc.
  (:451-453,468), ``disc_loss = (real + fake) / 2``;
* ``gen_loss = 0.01 * L1 + 1 * VGG + 0.005 * adversarial`` (:469); the reference's second generator forward
  (:462) recomputes the first bit for bit and is not repeated here;
* BOTH phases sit inside ``amp.autocast`` (:384,446,461), so without ``--disable-amp`` the generator,
  the discriminator and VGG19 all multiply bf16-rounded operands with fp32 accumulation in both
  phases (``amp_phases``; BASELINE config 4).  ``--disable-amp`` gives exact fp32.
"""
import functools

import torch

from .. import functional as F
from ..layers import no_weight_grad
from ..srgan.trainer import SRGANTrainer
from .discriminator import Discriminator
from .generator import Generator


class ESRGANTrainer(SRGANTrainer):
    phase_prefix = 'esrgan'
    # three gradients meet at the generator's output (pixel, perceptual, adversarial): summing them in another order than autograd
    # moves last bits, and the backward on the side stream bought nothing here (10.14 vs 10.13 ms): forward only
    deep_overlap = False
    generator_cls = Generator
    discriminator_cls = Discriminator
    amp_phases = ('psnr', 'gan')          # esrgan/trainer.py:384 and :446,461
    gen_tail_bucket = 'upsample1.weight'  # data parallel: upsample1/2, conv3, conv4 gradients complete first
    finetune = True

    def __init__(self, device, args, *rest, **kw) -> None:
        self.scale = read_scale(args)  # train --scale: 4, or 2 (RRDBNet behind pixel_unshuffle(2); the compact net with 12 outputs)
        self._set_scale()
        super().__init__(device, args, *rest, **kw)

    def _set_scale(self) -> None:
        if self.scale != 4:  # (instance attribute: the class keeps describing the default network)
            cls = self.generator_cls
            self.generator_cls = functools.partial(getattr(cls, 'func', cls), **{**getattr(cls, 'keywords', {}),
                                                                                'scale_factor': self.scale, 'trainable': True})

    def _init_generator_state(self, path: str) -> dict:
        """``train --init-generator``: every RRDBNet file ``test --weights`` takes, in either published naming or this package's;
        the generator is built at the file's depth (23 blocks, or 6 for the anime model).  The file's scale must be the run's."""
        from ..rrdbnet import rrdbnet_geometry, rrdbnet_to_generator_state
        from ..test import load_generator_state
        state = rrdbnet_to_generator_state(load_generator_state(path))
        num_blocks, scale = rrdbnet_geometry(state)
        if scale != self.scale:
            raise RuntimeError(scale_conflict(f'--init-generator {path}', 'RRDBNet', scale, self.scale))
        cls = self.generator_cls  # (instance attribute: the class keeps describing the default network)
        self.generator_cls = functools.partial(getattr(cls, 'func', cls), **{**getattr(cls, 'keywords', {}),
                                                                            'num_rrdb_blocks': num_blocks})
        return state

    def _state_scale(self, state: dict):
        """The scale a generator state_dict was trained at (``None``: not readable off it)."""
        w = state.get('conv1.weight')
        return {3: 4, 12: 2}.get(int(w.shape[1])) if w is not None and w.dim() == 4 else None

    def _load_generator_state(self, state: dict, path: str) -> None:
        """A checkpoint's generator: one clear error when it was trained at the other scale."""
        scale = self._state_scale(state)
        if scale is not None and scale != self.scale:
            raise RuntimeError(scale_conflict(f'checkpoint {path}', 'generator', scale, self.scale))
        super()._load_generator_state(state, path)

    def _initialize_loss(self) -> None:
        """esrgan/trainer.py:159-165."""
        super()._initialize_loss()
        self.l1_loss = F.l1_loss
        self.pixel_loss = F.l1_loss
        self.bce_loss = F.bce_with_logits

    def _perceptual_loss(self):
        """``--perceptual single``: the reference's ``VGGLoss``; ``realesrgan``: Real-ESRGAN's five-layer pre-ReLU term
        under the same name and call (it holds no trainable parameter and no state either)."""
        if self.perceptual == 'realesrgan':
            from ..realesrgan.loss import PerceptualLoss
            return PerceptualLoss(weights=self.vgg_weights)
        if self.perceptual != 'single':
            raise RuntimeError(f'perceptual loss "{self.perceptual}" not supported. Please choose from: single, realesrgan')
        return super()._perceptual_loss()

    def _phase_disc(self) -> None:
        """esrgan/trainer.py:444-455 (optimizer step is issued by ``_phase_gen`` after the all-reduce)."""
        self._phase_disc_gen()
        self._phase_disc_loss()

    def _phase_disc_gen(self) -> None:
        # the three networks exchange NHWC tensors (as in the SRGAN trainer): the batch is converted once, the super-resolved
        # image never goes through the NCHW module boundary
        with torch.no_grad():
            low4 = F.to_nhwc(self._static['low_res'], 4)
            self._high4 = F.to_nhwc(self._static['high_res'], 4)
        self.disc_optimizer.zero_grad()                                          # :444
        # The reference runs the generator twice per step (:447 and again at :462) on the same input with the same
        # weights -- only the discriminator is updated in between, and RRDBNet has no BatchNorm, dropout or other
        # state -- so the second forward reproduces the first bit for bit.  It is run once, with its graph kept for
        # the generator update (as the reference's own SRGAN loop does, srgan/trainer.py:444,455-456): 587 GFLOP and
        # ~700 launches per step that change no result.
        self._super_res = self.generator.forward_nhwc(low4)                      # :447 (and :462)

    def _phase_disc_loss(self) -> None:
        # :448-453 -- D(real), D(fake) as one batch; both relativistic terms and their mean in the head's launch
        disc_loss, _ = self.discriminator.pair_loss_nhwc(self._high4, self._super_res.detach())
        self._backward(disc_loss)                                                # :455
        self._losses['gan/disc-loss'] = disc_loss.detach()

    def _phase_content(self) -> None:
        """esrgan/trainer.py:459-467: pixel and perceptual terms (the generator output of ``_phase_disc`` is reused)."""
        self.gen_optimizer.zero_grad()                                           # :459
        # :466 -- the 4th NHWC channel is zero on both sides: the mean runs over the 3 real ones
        pixel = self.l1_loss(self._super_res, self._high4, count=self._high4.numel() // 4 * 3)
        content = self.vgg_loss.forward_nhwc(self._super_res, self._high4)       # :467
        self._content = F.axpby(pixel, content, self.pixel_weight, 1.0)  # train --pixel-weight: 0.01 (:469), Real-ESRGAN 1.0
        self._losses['gan/pixel-loss'] = pixel.detach()
        self._losses['gan/content-loss'] = content.detach()

    def _phase_gen(self) -> None:
        """esrgan/trainer.py:456,463-480: D update, relativistic adversarial term, G backward."""
        self.disc_optimizer.step()                                               # :456
        with no_weight_grad():
            with torch.no_grad():  # mean(real_output) carries no gradient to the generator
                real_mean = F.mean(self.discriminator.forward_nhwc(self._high4))  # :463
            # :464,468-469 -- gen_loss = 0.01 * pixel + content + 0.005 * BCEWithLogits(D(fake) - mean(D(real)), 1)
            gen_loss, aux = self.discriminator.adversarial_loss_nhwc(self._super_res, real_mean, self._content, 0.005)
        self._backward(gen_loss)                                                 # :480
        self._losses['gan/adversarial-loss'] = aux[1]
        self._losses['gan/train-loss'] = gen_loss.detach()
        self._super_res = self._content = self._high4 = None


def read_scale(args) -> int:
    scale = int(getattr(args, 'scale', None) or 4)
    if scale not in (2, 4):
        raise RuntimeError(f'--scale {scale}: the trainers run at x4 and x2')
    return scale


def scale_conflict(what: str, kind: str, scale: int, run_scale: int) -> str:
    """The message for a file whose scale is not the run's (``--init-generator`` and resumed checkpoints)."""
    if scale == 2:
        return (f'{what}: an x2 {kind} file in a run at x{run_scale}; x2 is inference-only unless the run is started with '
                f'--scale 2 (test --weights runs the file as it is)')
    return f'{what}: an x{scale} {kind} file in a run started with --scale {run_scale}; start the run with --scale {scale}'
