"""Trainer of the compact generator (Real-ESRGAN's SRVGGNetCompact).

The discriminator, the losses (L1 pre-training; relativistic-average GAN, ``0.01 L1 + VGG + 0.005 adversarial``), the amp
phases and the hipGraph capture are ESRGAN's, unchanged; only the generator differs.  (``train --discriminator unet`` swaps the
critic and its loss: ``realesrgan/trainer.py``.)  ``args.num_conv`` (``train --num-conv``)
sets the number of body convs.
"""
import functools

from ..esrgan.trainer import ESRGANTrainer, read_scale, scale_conflict
from .generator import NUM_CONV, Generator, tail_index


class CompactTrainer(ESRGANTrainer):
    phase_prefix = 'compact'
    generator_cls = Generator
    # data parallel: the second half of the body and the output conv complete first (``Generator.forward_nhwc``'s 'g.tail' cut)
    gen_tail_bucket = f'body.{tail_index(NUM_CONV)}.weight'

    def __init__(self, device, args, *rest, **kw) -> None:
        self._num_conv_given = getattr(args, 'num_conv', None)  # None: the default, or the depth of --init-generator's file
        self.scale = read_scale(args)
        self._set_num_conv(int(self._num_conv_given or NUM_CONV))
        super().__init__(device, args, *rest, **kw)

    def _set_num_conv(self, num_conv: int) -> None:
        if num_conv != NUM_CONV or self.scale != 4:  # (instance attributes: the class keeps describing the default network)
            self.generator_cls = functools.partial(Generator, scale_factor=self.scale, num_conv=num_conv)
            self.gen_tail_bucket = f'body.{tail_index(num_conv)}.weight'

    def _set_scale(self) -> None:
        pass  # (``_set_num_conv`` builds the generator class from the depth and the scale)

    def _state_scale(self, state: dict):
        from ..test import compact_scale
        try:
            return compact_scale(state)
        except RuntimeError:
            return None

    def _init_generator_state(self, path: str) -> dict:
        """``train --init-generator``: every SRVGGNetCompact file ``test --weights`` takes; the depth is the file's, and the
        scale (read off the last conv's output channels) must be the run's."""
        from ..test import compact_num_conv, compact_scale, load_generator_state
        state = load_generator_state(path)
        depth = compact_num_conv(state)
        scale = compact_scale(state, path)
        if scale != self.scale:
            raise RuntimeError(scale_conflict(f'--init-generator {path}', 'SRVGGNetCompact', scale, self.scale))
        if self._num_conv_given is not None and int(self._num_conv_given) != depth:
            raise RuntimeError(num_conv_conflict(int(self._num_conv_given), depth, path))
        self.__dict__.pop('generator_cls', None)
        self.__dict__.pop('gen_tail_bucket', None)
        self._set_num_conv(depth)
        return state


def num_conv_conflict(given: int, depth: int, path: str) -> str:
    """The message for a ``--num-conv`` that disagrees with ``--init-generator``'s file (the command line and the trainer)."""
    return (f'--num-conv {given} does not fit --init-generator {path}, which holds {depth} body convs: drop --num-conv (the '
            f'depth is read off the file) or pass --num-conv {depth}')
