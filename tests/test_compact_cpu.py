"""The compact generator (SRVGGNetCompact) without a GPU: its state_dict schema against the restatement in
``tests/compact_ref.py``, the registry, the command line (``--model compact``, ``--num-conv``, ``--weights``), the checkpoint
layouts ``load_generator_state`` unwraps, and the tiling halo."""
import pytest
import torch

from compact_ref import CompactRef


@pytest.mark.parametrize('num_conv', [16, 32])
def test_state_dict_schema_is_srvggnetcompact(num_conv):
    from torchsr_amd.compact.generator import Generator
    got = Generator(num_conv=num_conv).state_dict()
    want = CompactRef(num_conv=num_conv).state_dict()
    assert list(got) == list(want)
    assert {k: tuple(v.shape) for k, v in got.items()} == {k: tuple(v.shape) for k, v in want.items()}
    last = 2 * num_conv + 2
    assert tuple(got['body.0.weight'].shape) == (64, 3, 3, 3) and tuple(got['body.1.weight'].shape) == (64,)
    assert tuple(got[f'body.{last}.weight'].shape) == (48, 64, 3, 3) and tuple(got[f'body.{last}.bias'].shape) == (48,)
    assert len(got) == 2 * (num_conv + 2) + (num_conv + 1)  # weight + bias per conv, one slope vector per PReLU
    Generator(num_conv=num_conv).load_state_dict(want)  # key for key, strict


def test_other_scales_and_refusals():
    from torchsr_amd.compact.generator import Generator
    assert tuple(Generator(scale_factor=2, num_conv=2).state_dict()['body.6.weight'].shape) == (12, 64, 3, 3)
    for bad in ({'scale_factor': 5}, {'num_conv': 0}, {'num_feat': 30}):
        with pytest.raises(ValueError):
            Generator(**bad)


def test_halo_is_the_receptive_field_rounded_up_to_8():
    from torchsr_amd.compact.generator import Generator
    assert Generator(num_conv=16).halo == 24
    assert Generator(num_conv=32).halo == 40
    assert Generator(num_conv=3).halo == 8
    assert 'halo' in Generator(num_conv=3).__dict__  # an instance attribute: it depends on the depth


def test_registry_knows_compact():
    from argparse import Namespace
    from torchsr_amd import models
    from torchsr_amd.compact.generator import Generator
    from torchsr_amd.compact.trainer import CompactTrainer
    from torchsr_amd.esrgan.trainer import ESRGANTrainer
    # MODELS / CROP_SIZE stay the reference's two entries (tests/test_cpu.py pins them); the additions sit next to them
    assert models.EXTRA_MODELS['compact'] is CompactTrainer and models.GENERATORS['compact'] is Generator
    assert models.EXTRA_CROP_SIZE['compact'] == 128 and set(models.EXTRA_MODELS) == set(models.EXTRA_CROP_SIZE)
    assert models.model_names() == ('compact', 'esrgan', 'srgan')
    with pytest.raises(RuntimeError, match='not supported'):
        models.select_trainer_model(Namespace(model='nope'))
    assert models.select_trainer_model(Namespace(model='Compact')) == (CompactTrainer, 128)
    assert models.select_test_model(Namespace(model='compact')) is Generator
    assert issubclass(CompactTrainer, ESRGANTrainer) and CompactTrainer.phase_prefix == 'compact'
    assert CompactTrainer.generator_cls is Generator
    # the tail bucket names a parameter that exists, at the default depth and at any other
    from torchsr_amd.compact.generator import tail_index
    assert CompactTrainer.gen_tail_bucket in Generator().state_dict()
    for n in (1, 2, 3, 16):
        assert f'body.{tail_index(n)}.weight' in Generator(num_conv=n).state_dict()
        assert Generator(num_conv=n).state_dict()[f'body.{tail_index(n)}.weight'].dim() == 4  # a conv, not a slope vector


def test_cli_accepts_compact_num_conv_and_weights(capsys):
    from torchsr_amd.torchsr import parse_args
    a = parse_args(['train', '--model', 'compact', '--num-conv', '16'])
    assert a.model == 'compact' and a.num_conv == 16
    assert parse_args(['train', '--model', 'compact']).num_conv == 32
    t = parse_args(['test', 'x.png', '--model', 'compact', '--weights', 'realesr-general-x4v3.pth', '--precision', 'fp16'])
    assert t.weights == 'realesr-general-x4v3.pth' and t.model == 'compact' and t.precision == 'fp16'
    assert parse_args(['test', 'x.png', '--model', 'srgan', '--weights', 'w.pth']).weights == 'w.pth'  # for any model
    assert parse_args(['test', 'x.png']).weights is None  # default: <model>-gan-best.pth
    for bad in (['train', '--model', 'srgan', '--num-conv', '16'], ['train', '--model', 'esrgan', '--num-conv', '32'],
                ['train', '--model', 'compact', '--num-conv', '0'], ['train', '--model', 'compact', '--num-conv', 'x']):
        with pytest.raises(SystemExit):
            parse_args(bad)
    assert '--num-conv' in capsys.readouterr().err


def test_load_generator_state_unwraps_every_layout(tmp_path):
    from torchsr_amd.test import compact_num_conv, load_generator_state
    sd = CompactRef(num_conv=2).state_dict()
    other = {k: v + 1 for k, v in sd.items()}
    cases = {
        'ema.pth': {'params_ema': sd},
        'both.pth': {'params': other, 'params_ema': sd},  # Real-ESRGAN files carry both: the averaged weights win
        'params.pth': {'params': sd},
        'state.pth': {'epoch': 3, 'phase': 'compact-gan', 'state': sd},
        'bare.pth': dict(sd),
        'ddp.pth': {'params_ema': {'module.' + k: v for k, v in sd.items()}},
    }
    for name, obj in cases.items():
        torch.save(obj, tmp_path / name)
        got = load_generator_state(str(tmp_path / name))
        assert list(got) == list(sd), name
        assert all(torch.equal(got[k], sd[k]) for k in sd), name
        assert compact_num_conv(got) == 2
    assert compact_num_conv(CompactRef(num_conv=16).state_dict()) == 16
    assert compact_num_conv(CompactRef(num_conv=32).state_dict()) == 32
    with pytest.raises(RuntimeError):
        compact_num_conv({'conv1.0.weight': torch.zeros(1)})


def test_restatement_is_the_architecture():
    """The restatement against a hand-written evaluation of the description: conv + per-channel PReLU chain, PixelShuffle,
    nearest-enlarged input -- in fp64, where both are exact to rounding."""
    import torch.nn.functional as TF
    from compact_ref import seeded_state
    ref = CompactRef(scale_factor=2, num_feat=8, num_conv=1).double()
    sd = {k: v.double() for k, v in seeded_state(ref, 1).items()}
    ref.load_state_dict(sd)
    x = torch.rand(1, 3, 4, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        y = ref(x)
    t = x
    for i in (0, 2):
        t = TF.conv2d(t, sd[f'body.{i}.weight'], sd[f'body.{i}.bias'], padding=1)
        t = torch.where(t > 0, t, t * sd[f'body.{i + 1}.weight'].view(1, -1, 1, 1))
    t = TF.conv2d(t, sd['body.4.weight'], sd['body.4.bias'], padding=1)
    want = torch.empty(1, 3, 8, 10, dtype=torch.float64)
    for c in range(3):
        for i in range(2):
            for j in range(2):
                want[0, c, i::2, j::2] = t[0, c * 4 + i * 2 + j] + x[0, c]
    assert torch.allclose(y, want, rtol=0, atol=1e-13)
