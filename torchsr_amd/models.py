"""Model registry -- interface of torchsr/models.py:10-82 (same dict names, same selectors,
same RuntimeError on unknown models).

``MODELS`` / ``CROP_SIZE`` hold the reference's two entries and stay exactly that (tests/test_cpu.py pins them); what this
package adds beyond the reference -- the compact generator -- is registered in ``EXTRA_MODELS`` / ``EXTRA_CROP_SIZE``, and
the selectors and the command line (``model_names``) look in both."""
from argparse import Namespace
from typing import Tuple

from torchsr_amd.compact.generator import Generator as CompactGen
from torchsr_amd.compact.trainer import CompactTrainer
from torchsr_amd.esrgan.generator import Generator as ESRGANGen
from torchsr_amd.esrgan.trainer import ESRGANTrainer
from torchsr_amd.srgan.generator import Generator as SRGANGen
from torchsr_amd.srgan.trainer import SRGANTrainer

MODELS = {
    'esrgan': ESRGANTrainer,
    'srgan': SRGANTrainer
}

CROP_SIZE = {
    'esrgan': 128,
    'srgan': 96
}

EXTRA_MODELS = {
    'compact': CompactTrainer
}

EXTRA_CROP_SIZE = {
    'compact': 128
}

GENERATORS = {
    'compact': CompactGen,
    'esrgan': ESRGANGen,
    'srgan': SRGANGen
}


DISCRIMINATORS = ('vgg', 'unet')  # train --discriminator: the model's own VGG-style critic, or Real-ESRGAN's U-Net


def _unet_trainers() -> dict:
    from torchsr_amd.realesrgan.trainer import UNetCompactTrainer, UNetESRGANTrainer
    return {'esrgan': UNetESRGANTrainer, 'compact': UNetCompactTrainer}


def model_names() -> Tuple[str, ...]:
    """Every ``--model`` the command line accepts."""
    return tuple(sorted({**MODELS, **EXTRA_MODELS}))


def select_trainer_model(args: Namespace) -> Tuple[object, int]:
    """Trainer class and crop size for ``args.model`` (case-insensitive), models.py:26-53."""
    name = args.model.lower()
    disc = (getattr(args, 'discriminator', None) or 'vgg').lower()
    if disc not in DISCRIMINATORS:
        raise RuntimeError(f'discriminator {disc} not supported. Please choose from: {DISCRIMINATORS}')
    if disc == 'unet':
        trainers = _unet_trainers()
        if name not in trainers:
            raise RuntimeError(f'--discriminator unet trains with --model {" or ".join(sorted(trainers))}; --model {args.model} '
                               'keeps its own discriminator')
        return trainers[name], {**CROP_SIZE, **EXTRA_CROP_SIZE}[name]
    if name in MODELS:
        return MODELS[name], CROP_SIZE[name]
    if name in EXTRA_MODELS:
        return EXTRA_MODELS[name], EXTRA_CROP_SIZE[name]
    raise RuntimeError(f'{args.model} not supported. Please choose from: {model_names()}')


def select_test_model(args: Namespace) -> object:
    """Generator class for ``args.model``, models.py:56-82."""
    name = args.model.lower()
    if name in GENERATORS:
        return GENERATORS[name]
    raise RuntimeError(f'{args.model} not supported. Please choose from: {GENERATORS.keys()}')
