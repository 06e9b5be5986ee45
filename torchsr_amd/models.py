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


def model_names() -> Tuple[str, ...]:
    """Every ``--model`` the command line accepts."""
    return tuple(sorted({**MODELS, **EXTRA_MODELS}))


def select_trainer_model(args: Namespace) -> Tuple[object, int]:
    """Trainer class and crop size for ``args.model`` (case-insensitive), models.py:26-53."""
    name = args.model.lower()
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
