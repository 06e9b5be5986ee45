"""Trainer of the compact generator (Real-ESRGAN's SRVGGNetCompact).

The discriminator, the losses (L1 pre-training; relativistic-average GAN, ``0.01 L1 + VGG + 0.005 adversarial``), the amp
phases and the hipGraph capture are ESRGAN's, unchanged; only the generator differs.  (``train --discriminator unet`` swaps the
critic and its loss: ``realesrgan/trainer.py``.)  ``args.num_conv`` (``train --num-conv``)
sets the number of body convs.
"""
import functools

from ..esrgan.trainer import ESRGANTrainer
from .generator import NUM_CONV, Generator, tail_index


class CompactTrainer(ESRGANTrainer):
    phase_prefix = 'compact'
    generator_cls = Generator
    # data parallel: the second half of the body and the output conv complete first (``Generator.forward_nhwc``'s 'g.tail' cut)
    gen_tail_bucket = f'body.{tail_index(NUM_CONV)}.weight'

    def __init__(self, device, args, *rest, **kw) -> None:
        num_conv = int(getattr(args, 'num_conv', None) or NUM_CONV)
        if num_conv != NUM_CONV:  # (instance attributes: the class keeps describing the default network)
            self.generator_cls = functools.partial(Generator, num_conv=num_conv)
            self.gen_tail_bucket = f'body.{tail_index(num_conv)}.weight'
        super().__init__(device, args, *rest, **kw)
