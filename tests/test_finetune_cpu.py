"""Fine-tuning without a GPU: the command line of ``train --init-generator / --init-discriminator / --ema-decay /
--pixel-weight`` and ``test --ema``, the loaders behind them, and the argument checks of ``srx_ema_update``."""
import pytest
import torch

import compact_ref
import unet_ref


def _compact_file(tmp_path, num_conv: int, name: str = 'compact.pth') -> str:
    path = str(tmp_path / name)
    torch.save({'params_ema': compact_ref.CompactRef(num_conv=num_conv).state_dict()}, path)
    return path


@pytest.mark.parametrize('flag', [['--init-generator', 'g.pth'], ['--init-discriminator', 'd.pth'], ['--ema-decay', '0.999'],
                                  ['--pixel-weight', '1.0']])
def test_each_new_flag_is_refused_for_srgan(flag, capsys):
    from torchsr_amd.torchsr import parse_args
    with pytest.raises(SystemExit):
        parse_args(['train', '--model', 'srgan'] + flag)
    assert f'{flag[0]} trains with --model esrgan or --model compact; --model srgan' in capsys.readouterr().err


def test_flags_parse_for_esrgan_and_compact_and_default_to_off(tmp_path):
    from torchsr_amd.torchsr import parse_args
    path = _compact_file(tmp_path, 2)
    for model in ('esrgan', 'compact'):
        off = parse_args(['train', '--model', model])
        assert (off.init_generator, off.init_discriminator, off.ema_decay, off.pixel_weight) == (None, None, None, None)
        on = parse_args(['train', '--model', model, '--ema-decay', '0.999', '--pixel-weight', '1.0', '--init-discriminator', path])
        assert on.ema_decay == 0.999 and on.pixel_weight == 1.0 and on.init_discriminator == path
    assert parse_args(['train', '--model', 'esrgan', '--ema-decay', '0']).ema_decay == 0.0
    assert parse_args(['train', '--model', 'compact']).num_conv == 32
    assert parse_args(['test', 'x.png', '--ema']).ema is True and parse_args(['test', 'x.png']).ema is False


@pytest.mark.parametrize('value', ['1', '-0.1', 'nan', '1.5', 'inf', 'x'])
def test_ema_decay_outside_the_half_open_interval_is_refused(value, capsys):
    from torchsr_amd.torchsr import parse_args
    with pytest.raises(SystemExit):
        parse_args(['train', '--model', 'esrgan', f'--ema-decay={value}'])
    assert '--ema-decay' in capsys.readouterr().err


def test_num_conv_comes_from_the_file_and_a_conflict_names_both_numbers(tmp_path, capsys):
    from torchsr_amd.torchsr import parse_args
    path = _compact_file(tmp_path, 2)
    assert parse_args(['train', '--model', 'compact', '--init-generator', path]).num_conv == 2
    assert parse_args(['train', '--model', 'compact', '--init-generator', path, '--num-conv', '2']).num_conv == 2
    with pytest.raises(SystemExit):
        parse_args(['train', '--model', 'compact', '--init-generator', path, '--num-conv', '16'])
    err = capsys.readouterr().err
    assert '--num-conv 16' in err and 'holds 2 body convs' in err
    with pytest.raises(SystemExit):
        parse_args(['train', '--model', 'compact', '--init-generator', str(tmp_path / 'absent.pth')])
    assert 'no such file' in capsys.readouterr().err
    torch.save({'params': unet_ref.UNetRef().state_dict()}, str(tmp_path / 'd.pth'))  # not a compact generator
    with pytest.raises(SystemExit):
        parse_args(['train', '--model', 'compact', '--init-generator', str(tmp_path / 'd.pth')])
    assert 'not a compact' in capsys.readouterr().err


def test_load_generator_state_ema(tmp_path):
    from torchsr_amd.test import load_generator_state
    live = {'body.0.weight': torch.zeros(2), 'module.body.0.bias': torch.zeros(1)}
    average = {'body.0.weight': torch.ones(2), 'module.body.0.bias': torch.ones(1)}
    both, only = str(tmp_path / 'both.pth'), str(tmp_path / 'only.pth')
    torch.save({'epoch': 1, 'phase': 'compact-gan', 'state': live, 'params_ema': average}, both)
    torch.save({'epoch': 1, 'phase': 'compact-gan', 'state': live}, only)
    got = load_generator_state(both, ema=True)
    assert list(got) == ['body.0.weight', 'body.0.bias'] and all(bool((v == 1).all()) for v in got.values())
    assert all(bool((v == 0).all()) for v in load_generator_state(both).values())  # without the flag: 'state' first, as before
    with pytest.raises(RuntimeError, match=r'holds no averaged weights.*epoch.*phase.*state'):
        load_generator_state(only, ema=True)
    assert all(bool((v == 0).all()) for v in load_generator_state(only).values())


def test_init_discriminator_loads_strictly_and_names_the_kind(tmp_path):
    from torchsr_amd.esrgan.discriminator import Discriminator
    from torchsr_amd.realesrgan.discriminator import UNetDiscriminatorSN
    from torchsr_amd.srgan.trainer import load_discriminator_init
    want = unet_ref.seeded_state(unet_ref.UNetRef(), 5)
    unet_path, vgg_path, own_path = (str(tmp_path / n) for n in ('unet.pth', 'vgg.pth', 'own.pth'))
    torch.save({'params': want}, unet_path)
    torch.manual_seed(0)
    disc = UNetDiscriminatorSN()
    load_discriminator_init(disc, unet_path)
    got = disc.state_dict()
    assert list(got) == list(want)
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    # one of this package's checkpoints: its resume.discriminator entry; DDP's prefix is dropped
    torch.save({'epoch': 1, 'phase': 'x', 'state': {}, 'resume': {'discriminator': {'module.' + k: v + 1 for k, v in want.items()}}},
               own_path)
    load_discriminator_init(disc, own_path)
    assert all(torch.equal(disc.state_dict()[k], v + 1) for k, v in want.items())
    vgg = Discriminator()
    torch.save(vgg.state_dict(), vgg_path)
    with pytest.raises(RuntimeError, match='holds a "vgg" discriminator, this run trains a "unet" one'):
        load_discriminator_init(disc, vgg_path)
    with pytest.raises(RuntimeError, match='holds a "unet" discriminator, this run trains a "vgg" one'):
        load_discriminator_init(vgg, unet_path)
    short = dict(want)
    short.pop('conv9.bias')
    torch.save(short, unet_path)
    with pytest.raises(RuntimeError, match="does not fit this run's"):
        load_discriminator_init(disc, unet_path)


def test_flat_ema_refuses_a_decay_outside_the_interval():
    from torchsr_amd.optim import FlatEMA, FlatParams
    flat = FlatParams(torch.nn.Linear(3, 2))
    for bad in (1.0, -0.1, float('nan'), 2.0):
        with pytest.raises(ValueError, match='decay must be in'):
            FlatEMA(flat, bad)
    ema = FlatEMA(flat, 0.999)
    assert ema.one_minus_decay == 1.0 - 0.999 and ema.data.data_ptr() != flat.data.data_ptr()
    assert torch.equal(ema.data, flat.data) and flat.numel == 12  # 6 -> 8 and 2 -> 4 floats: the gaps are part of the buffer


def test_abi_refuses_bad_ema_arguments_without_a_gpu():
    """``srx_ema_update`` refuses what would read or write where it must not -- before anything is launched, so the checks run
    here with fake pointers, on the CPU."""
    import ctypes as C
    from torchsr_amd import _lib
    if torch.cuda.is_available():
        pytest.skip('fake pointers: argument validation is exercised where a missed check cannot reach a device')
    lib = _lib.lib()
    a, b = 0x10000, 0x20000  # never dereferenced: the calls below must fail in argument validation

    def err():
        buf = C.create_string_buffer(256)
        lib.srx_last_error(buf, 256)
        return buf.value.decode()

    assert lib.srx_ema_update(None, b, 16, 0.5, 0.5, None) != 0 and 'bad argument' in err()
    assert lib.srx_ema_update(a, None, 16, 0.5, 0.5, None) != 0 and 'bad argument' in err()
    assert lib.srx_ema_update(a, b, 0, 0.5, 0.5, None) != 0 and 'bad argument' in err()
    assert lib.srx_ema_update(a, b, -4, 0.5, 0.5, None) != 0 and 'bad argument' in err()
    assert lib.srx_ema_update(a + 4, b, 16, 0.5, 0.5, None) != 0 and '16-byte aligned' in err()
    assert lib.srx_ema_update(a, b + 8, 16, 0.5, 0.5, None) != 0 and '16-byte aligned' in err()
    assert lib.srx_ema_update(a, a, 16, 0.5, 0.5, None) != 0 and 'same buffer' in err()
    for decay in (1.0, -0.1, 1.5, float('nan'), float('inf'), -float('inf')):
        assert lib.srx_ema_update(a, b, 16, decay, 0.5, None) != 0 and 'decay must be in [0, 1)' in err(), decay
    for omd in (0.0, -0.5, 1.5, float('nan'), float('inf')):
        assert lib.srx_ema_update(a, b, 16, 0.5, omd, None) != 0 and 'one_minus_decay must be in (0, 1]' in err(), omd
