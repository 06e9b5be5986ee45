"""Fine-tuning on the MI355X: ``srx_ema_update`` through the C ABI, ``optim.FlatEMA``, and the trainers with
``--ema-decay``, ``--init-generator``, ``--init-discriminator`` and ``--pixel-weight``.

The bound of every comparison of an average is derived, not fitted.  One update forms two fp32 products and one fp32 sum, each
rounded once (the kernel never contracts them), from the fp32 constants ``d = fl(decay)`` and ``w = fl(1 - decay)`` (the difference
formed in double, rounded once): with ``u = 2^-24`` the result is within ``(2 u + u^2) (|d ema| + |w p|) < 3 u (|d ema| + |w p|)``
of the exact ``d ema + w p``, elementwise.  An error already in ``ema`` is multiplied by ``d < 1``, so after k updates the error is
at most the sum of the k per-update bounds (``_recurrence`` adds them up, on the fp64 values).  ``d = 0`` gives ``0 * ema + 1 * p``:
``p``, bit for bit.  Everything else here is equality of bits: the same kernels on the same operands.
"""
import functools
import os
import socket
import warnings
from argparse import Namespace
from math import log10

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as TF

import compact_ref
import rrdbnet_ref
import unet_ref
from guarded import SENTINEL, Guarded, within

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GRID_CAP = 4096 * 256  # quads one pass of the grid covers: stream_blocks() in csrc/optim.hip caps the grid at 4096 workgroups of 256


def _consts(decay: float):
    """The two fp32 constants the kernel multiplies by, as doubles."""
    return float(np.float32(decay)), float(np.float32(1.0 - decay))


def _recurrence(ema0, weights, decay: float):
    """fp64 recurrence over the recorded live weights and the summed per-update bounds."""
    d, w = _consts(decay)
    ema, bound = ema0.double(), torch.zeros_like(ema0, dtype=torch.float64)
    for p in weights:
        a, b = d * ema, w * p.double()
        ema = a + b
        bound = bound + 3.0 * U * (a.abs() + b.abs())
    return ema, bound


def _update(ema, p, n, decay):
    from torchsr_amd import _lib
    _lib.call('srx_ema_update', ema.ptr(), p.ptr(), n, decay, 1.0 - decay, torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------ 1. the kernel through the C ABI
# n = 1, 3: the scalar tail alone; 4: one quad; 5, 1027: quads and a tail, more than one workgroup at 1027 (257 quads);
# 4 * GRID_CAP + 15: threads 0 .. 2 of the first workgroup take a second grid-stride iteration, then a 3-element tail
SIZES = [1, 3, 4, 5, 1027, 4 * GRID_CAP + 15]


@pytest.fixture(scope='module')
def kernel_inputs():
    g = torch.Generator().manual_seed(20)
    n = max(SIZES)
    return torch.randn(n, generator=g), torch.randn(n, generator=g)


@pytest.mark.parametrize('decay', [0.0, 0.5, 0.999])
def test_ema_update_kernel_against_fp64(dev, decay, kernel_inputs):
    d, w = _consts(decay)
    for n in SIZES:
        e0, p0 = kernel_inputs[0][:n], kernel_inputs[1][:n]
        ema = Guarded(dev, (n,), src=e0, margin=SENTINEL, margin_floats=64)
        p = Guarded(dev, (n,), src=p0, margin_floats=64)
        _update(ema, p, n, decay)
        torch.cuda.synchronize()
        got = ema.t.cpu()
        a, b = d * e0.double(), w * p0.double()
        err = (got.double() - (a + b)).abs()
        bound = 3.0 * U * (a.abs() + b.abs())
        print(f'decay {decay} n {n}: worst error / bound {(err / bound).max().item():.3f}')
        within(got, a + b, bound, f'ema decay {decay} n {n}')
        assert ema.margins_unchanged() and p.margins_unchanged(), (decay, n)
        assert torch.equal(p.t.cpu(), p0), (decay, n)
        if decay == 0.0:
            assert torch.equal(got.view(torch.int32), p0.view(torch.int32)), n


def test_ema_update_refusals_on_device_buffers(dev):
    """The refusals again with real buffers (a missed check could only touch memory the test owns); nothing is written."""
    from torchsr_amd import _lib
    lib = _lib.lib()
    ema = Guarded(dev, (16,), src=torch.ones(16), margin=SENTINEL, margin_floats=64)
    p = Guarded(dev, (16,), src=torch.full((16,), 2.0), margin_floats=64)
    e, q = ema.t.data_ptr(), p.t.data_ptr()
    for args in ((e, q, 0, 0.5, 0.5), (e, e, 16, 0.5, 0.5), (e + 4, q, 8, 0.5, 0.5), (e, q + 4, 8, 0.5, 0.5), (e, q, 16, 1.0, 0.5),
                 (e, q, 16, float('nan'), 0.5), (e, q, 16, -0.1, 0.5), (None, q, 16, 0.5, 0.5), (e, None, 16, 0.5, 0.5)):
        assert lib.srx_ema_update(*args, None) != 0, args
    torch.cuda.synchronize()
    assert bool((ema.t == 1).all()) and bool((p.t == 2).all()) and ema.margins_unchanged()


# ------------------------------------------------------------------ 2. FlatEMA
def _gap_mask(flat):
    mask = torch.ones(flat.numel, dtype=torch.bool)
    for p, o in zip(flat.params, flat.offsets):
        mask[o:o + p.numel()] = False
    return mask


@pytest.mark.parametrize('which', ['compact num_conv=1', 'ragged stack'])
def test_flat_ema_three_updates_against_the_recurrence(dev, which):
    from torchsr_amd.compact.generator import Generator
    from torchsr_amd.optim import FlatEMA, FlatParams
    torch.manual_seed(4)
    if which == 'ragged stack':  # 15, 5, 15 and 3 floats: a gap behind every parameter
        module = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.Linear(5, 3)).to(dev)
    else:
        module = Generator(num_conv=1).to(dev)
    flat = FlatParams(module)
    gaps = _gap_mask(flat)
    assert (int(gaps.sum()) > 0) == (which == 'ragged stack')
    ema = FlatEMA(flat, 0.9)
    assert torch.equal(ema.data, flat.data) and ema.data.data_ptr() != flat.data.data_ptr()
    ema0, weights = ema.data.cpu(), []
    g = torch.Generator().manual_seed(5)
    for _ in range(3):
        with torch.no_grad():
            for p in module.parameters():  # (through the views: the gaps are nobody's)
                p.add_((torch.randn(p.shape, generator=g) * 0.05).to(dev))
        weights.append(flat.data.cpu())
        ema.update()
    want, bound = _recurrence(ema0, weights, 0.9)
    got = ema.data.cpu()
    within(got, want, bound, f'FlatEMA {which}')
    assert not torch.equal(got, weights[-1])
    assert bool((got[gaps] == 0).all()) and bool((flat.data.cpu()[gaps] == 0).all())
    # the averaged weights under the module's names, and back
    sd = ema.state_dict(module)
    assert list(sd) == list(module.state_dict())
    for (k, v), (o, p) in zip(sd.items(), zip(flat.offsets, flat.params)):
        assert v.device.type == 'cpu' and torch.equal(v.reshape(-1), got[o:o + p.numel()]), k
    ema.reset()
    assert torch.equal(ema.data, flat.data)
    ema.load_state_dict(module, sd)
    assert torch.equal(ema.data.cpu(), got)


# ------------------------------------------------------------------ 3. the trainers
def _trainer(dev, model: str, graphs: bool, seed: int = 3, amp: bool = True, disc: str = 'unet', prepare: bool = True, blocks: int = 2,
             **extra):
    """A two-block ESRGAN / two-conv compact trainer against the U-Net critic on 32 x 32 crops (tests/test_unet_disc_gpu.py)."""
    from oracle.weights import closed_form_state
    from torchsr_amd.esrgan.generator import Generator
    from torchsr_amd.models import select_trainer_model
    args = Namespace(disable_amp=not amp, batch_size=2, epochs=8, gan_checkpoint=None, local_rank=0, pretrain_epochs=1,
                     psnr_checkpoint=None, skip_image_save=True, world_size=1, rank=-1, use_graphs=graphs, vgg_weights='random',
                     num_conv=2, model=model, discriminator=disc, **extra)
    cls, _crop = select_trainer_model(args)
    if model == 'esrgan':
        cls = type('Small' + cls.__name__, (cls,), {'generator_cls': functools.partial(Generator, num_rrdb_blocks=blocks)})
    torch.manual_seed(seed)
    t = cls(dev, args, [], [], 2, 2, distributed=False)
    if prepare:
        if disc == 'unet' and not extra.get('init_discriminator'):
            t.discriminator.load_state_dict(unet_ref.seeded_state(unet_ref.UNetRef(), 11))
        t.vgg_loss.features.load_state_dict(closed_form_state(t.vgg_loss.features.state_dict(), prefix='features.'))
    t.generator.train()
    t.discriminator.train()
    return t


def _batch(dev, seed=31):
    g = torch.Generator().manual_seed(seed)
    hr = torch.rand(2, 3, 32, 32, generator=g).to(dev)
    return TF.avg_pool2d(hr, 4), hr


def _items(losses):
    return [(k, v.item()) for k, v in sorted(losses.items())]


def _same_bits(a, b, what):
    assert list(a) == list(b), what
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize('model', ['esrgan', 'compact'])
def test_ema_does_not_disturb_training_and_follows_the_recurrence(dev, model):
    """5 GAN steps (two eager, the capture, two replays), then 5 pre-training steps (the eager one after the phase switch, two
    more, the capture, a replay), with --ema-decay 0.5 and without it: the same losses and live weights, bit for bit; the average
    is the fp64 recurrence over the live weights recorded after every step; and an eager step of either phase launches what it
    launches without the average, plus one ``ema_update_kernel``."""
    import step_layers
    lr, hr = _batch(dev)
    off, on = _trainer(dev, model, True), _trainer(dev, model, True, ema_decay=0.5)
    assert off.gen_ema is None and off.ema_generator is None
    ema0, weights = on.gen_ema.data.cpu(), []
    assert torch.equal(ema0, on.gen_flat.data.cpu())
    for step in range(10):
        if step < 5:
            a, b = _items(off.gan_step(lr, hr)), _items(on.gan_step(lr, hr))
        else:
            a, b = off.pretrain_step(lr, hr).item(), on.pretrain_step(lr, hr).item()
        assert a == b and np.all(np.isfinite([v for _k, v in a] if step < 5 else [a])), (step, a, b)
        weights.append(on.gen_flat.data.cpu())
        assert torch.equal(off.gen_flat.data.cpu(), weights[-1]), step
    for t in (off, on):
        assert {'gan.all', 'psnr.all'} <= set(t._graphs)
    _same_bits(off.discriminator.state_dict(), on.discriminator.state_dict(), 'D')
    want, bound = _recurrence(ema0, weights, 0.5)
    within(on.gen_ema.data.cpu(), want, bound, f'{model}: the average after 10 steps')
    assert not torch.equal(on.gen_ema.data, on.gen_flat.data)
    assert bool((on.gen_ema.data.cpu()[_gap_mask(on.gen_flat)] == 0).all())
    # one eager step of each phase under the launch records
    for t in (off, on):
        t.use_graphs = False
    for phase, run in (('gan', lambda t: t.gan_step(lr, hr)), ('psnr', lambda t: t.pretrain_step(lr, hr))):
        names = [step_layers.prof_launches(functools.partial(run, t)) for t in (off, on)]
        assert len(names[0]) >= 8 and not any('ema' in n for n in names[0]), phase  # (the two-conv generator: 4 convs, forward and backward)
        assert [n for n in names[1] if 'ema' in n] == ['ema_update_kernel'], phase
        assert [n for n in names[1] if 'ema' not in n] == names[0], phase
        assert torch.equal(off.gen_flat.data, on.gen_flat.data), phase


def _psnr(generator, lr, hr):
    from torchsr_amd import functional as F
    with torch.no_grad():
        return 10 * log10(1 / F.mse_loss(generator.eval()(lr), hr).item())


def test_validation_checkpoints_resume_and_test_ema(dev, tmp_path, monkeypatch, capsys):
    from PIL import Image
    from torchsr_amd.compact.generator import Generator
    from torchsr_amd.srgan.trainer import save_image
    from torchsr_amd.test import load_generator_state, upscale
    from torchsr_amd.torchsr import main
    monkeypatch.chdir(tmp_path)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'LOCAL_WORLD_SIZE', 'SLURM_NTASKS'):
        monkeypatch.delenv(k, raising=False)
    lr, hr = _batch(dev)
    whole = _trainer(dev, 'compact', False, ema_decay=0.5)
    for _ in range(4):
        whole.gan_step(lr, hr)
    first = _trainer(dev, 'compact', False, ema_decay=0.5)
    first.test_loader = [(lr, None, hr)]
    for _ in range(2):
        first.gan_step(lr, hr)
    # ---- _test evaluates the average: the logged PSNR is that of a fresh generator holding params_ema
    logged = []
    first._log_wandb = lambda contents, step=None: logged.append(contents)
    live_before = first.gen_flat.data.clone()
    first._test(1, 'compact-gan', 0)
    assert torch.equal(first.gen_flat.data, live_before) and first.generator.training
    ckpt = torch.load('compact-gan-latest.pth', map_location='cpu')
    assert set(ckpt) == {'epoch', 'phase', 'state', 'resume', 'params_ema'}
    assert set(torch.load('compact-gan-best.pth', map_location='cpu')) == set(ckpt)
    assert list(ckpt['params_ema']) == list(ckpt['state'])
    assert all(v.device.type == 'cpu' and v.shape == ckpt['state'][k].shape for k, v in ckpt['params_ema'].items())
    _same_bits(ckpt['state'], {k: v.cpu() for k, v in first.generator.state_dict().items()}, 'state stays the live weights')
    assert not any(torch.equal(v, ckpt['state'][k]) for k, v in ckpt['params_ema'].items())
    fresh = Generator(num_conv=2).to(dev)
    fresh.load_state_dict(ckpt['params_ema'])
    psnr_ema = _psnr(fresh, lr, hr)
    fresh.load_state_dict(ckpt['state'])
    psnr_live = _psnr(fresh, lr, hr)
    print(f'PSNR of the average {psnr_ema!r}, of the live weights {psnr_live!r}, logged {logged[0]["gan/PSNR"]!r}')
    assert logged[0]['gan/PSNR'] == psnr_ema and psnr_ema != psnr_live
    assert f'PSNR: {round(psnr_ema, 3)},' in capsys.readouterr().out
    # a second evaluation after more steps sees the new average (the copy's packed weights follow its own epoch)
    first.gan_step(lr, hr)
    logged.clear()
    first._test(2, 'compact-gan', 0)
    fresh.load_state_dict(torch.load('compact-gan-latest.pth', map_location='cpu')['params_ema'])
    assert logged[0]['gan/PSNR'] == _psnr(fresh, lr, hr) != psnr_ema
    # ---- 2 + 2 steps through save -> new trainer -> resume: the average of 4 straight steps, bit for bit
    path = str(tmp_path / 'two.pth')
    torch.save(ckpt, path)
    second = _trainer(dev, 'compact', False, seed=99, ema_decay=0.5)
    loaded = second._load_checkpoint(path)
    second.generator.load_state_dict(loaded['state'])
    assert second._restore_resume_state(loaded)
    for _ in range(2):
        second.gan_step(lr, hr)
    assert torch.equal(second.gen_ema.data, whole.gen_ema.data) and torch.equal(second.gen_flat.data, whole.gen_flat.data)
    # a checkpoint without an average: the average starts at the loaded weights
    loaded.pop('params_ema')
    second.generator.load_state_dict(loaded['state'])
    assert second._restore_resume_state(loaded)
    assert torch.equal(second.gen_ema.data, second.gen_flat.data)
    # ---- with the average off the file's keys are the old ones
    plain = _trainer(dev, 'compact', False)
    plain.gan_step(lr, hr)
    state = plain._model_state(1, 'compact-gan')
    assert set(state) == {'epoch', 'phase', 'state', 'resume'}
    torch.save(state, str(tmp_path / 'plain.pth'))
    # ---- test --ema through the command line
    image = (np.random.RandomState(2).rand(12, 20, 3) * 255).astype('uint8')
    Image.fromarray(image).save('lr.png')
    low = torch.from_numpy(image.astype('float32') / 255.0).permute(2, 0, 1).unsqueeze(0).contiguous().to(dev)
    for flags, key in ((['--ema'], 'params_ema'), ([], 'state')):
        main(['test', 'lr.png', '--model', 'compact', '--weights', path] + flags)
        got = np.asarray(Image.open('upres-lr.png')).copy()
        assert load_generator_state(path, ema=bool(flags)).keys() == ckpt[key].keys()
        fresh.load_state_dict(ckpt[key])
        save_image(upscale(fresh, low, scale=4, precision='fp32'), 'want.png')
        assert got.shape == (48, 80, 3) and np.array_equal(got, np.asarray(Image.open('want.png'))), key
        os.remove('upres-lr.png')
    with pytest.raises(SystemExit, match='holds no averaged weights'):
        main(['test', 'lr.png', '--model', 'compact', '--weights', str(tmp_path / 'plain.pth'), '--ema'])
    assert not os.path.exists('upres-lr.png')


# ------------------------------------------------------------------ 4. init files
def _generator_file(tmp_path, kind: str):
    """(path, the state in the trainer's generator's key names)"""
    from torchsr_amd.rrdbnet import rrdbnet_to_generator_state
    path = str(tmp_path / f'{kind}.pth')
    if kind == 'compact':
        state = compact_ref.seeded_state(compact_ref.CompactRef(num_conv=2), 21)
        torch.save({'params_ema': state, 'params': {k: v + 1 for k, v in state.items()}}, path)
        return path, state
    state = rrdbnet_ref.seeded_state(rrdbnet_ref.RRDBNetRef(num_block=2), 22)
    torch.save({'params_ema': rrdbnet_ref.xinntao_names(state) if kind == 'xinntao' else state}, path)
    return path, rrdbnet_to_generator_state(state)


def _disc_file(tmp_path, seed=23):
    path, state = str(tmp_path / 'netD.pth'), unet_ref.seeded_state(unet_ref.UNetRef(), seed)
    torch.save({'params': state}, path)
    return path, state


@pytest.mark.parametrize('kind', ['basicsr', 'xinntao', 'compact'])
def test_init_files_are_the_trainers_weights_bit_for_bit(dev, tmp_path, kind):
    gpath, gstate = _generator_file(tmp_path, kind)
    dpath, dstate = _disc_file(tmp_path)
    model = 'compact' if kind == 'compact' else 'esrgan'
    t = _trainer(dev, model, True, prepare=False, blocks=1, init_generator=gpath, init_discriminator=dpath, ema_decay=0.5)
    _same_bits({k: v.cpu() for k, v in t.generator.state_dict().items()}, dict(gstate), 'G')
    _same_bits({k: v.cpu() for k, v in t.discriminator.state_dict().items()}, dstate, 'D (weight_u, weight_v included)')
    if model == 'esrgan':
        assert len(t.generator.blocks) == 2  # the file's depth, not the trainer's default (1 here)
    assert torch.equal(t.gen_ema.data, t.gen_flat.data)
    for p, o in zip(t.gen_flat.params, t.gen_flat.offsets):  # the parameters are views into the flat buffer that holds the file
        assert p.data_ptr() == t.gen_flat.data.data_ptr() + 4 * o
    for opt in (t.psnr_optimizer, t.gen_optimizer, t.disc_optimizer):  # optimiser states start at zero
        assert int(opt.step_count) == 0 and not bool(opt.exp_avg.any()) and not bool(opt.exp_avg_sq.any())


def test_init_refusals(dev, tmp_path):
    x2 = str(tmp_path / 'x2.pth')
    torch.save({'params_ema': rrdbnet_ref.seeded_state(rrdbnet_ref.RRDBNetRef(num_block=1, scale=2), 1)}, x2)
    with pytest.raises(RuntimeError, match='x2 is inference-only'):
        _trainer(dev, 'esrgan', True, prepare=False, init_generator=x2)
    gpath, _ = _generator_file(tmp_path, 'compact')
    with pytest.raises(RuntimeError, match='RRDBNet'):  # (a compact file: rrdbnet_to_generator_state refuses it)
        _trainer(dev, 'esrgan', True, prepare=False, init_generator=gpath)
    three = str(tmp_path / 'three.pth')
    torch.save(compact_ref.CompactRef(num_conv=3).state_dict(), three)
    with pytest.raises(RuntimeError, match='--num-conv 2 does not fit .* holds 3 body convs'):
        _trainer(dev, 'compact', True, prepare=False, init_generator=three)
    dpath, _ = _disc_file(tmp_path)
    with pytest.raises(RuntimeError, match='holds a "unet" discriminator, this run trains a "vgg" one'):
        _trainer(dev, 'compact', True, prepare=False, disc='vgg', init_discriminator=dpath)
    from torchsr_amd.srgan.trainer import SRGANTrainer
    args = Namespace(disable_amp=True, batch_size=2, epochs=8, gan_checkpoint=None, local_rank=0, pretrain_epochs=1,
                     psnr_checkpoint=None, skip_image_save=True, world_size=1, rank=-1, vgg_weights='random', ema_decay=0.5)
    with pytest.raises(RuntimeError, match='--model esrgan or --model compact'):
        SRGANTrainer(dev, args, [], [], 2, 2)


def test_init_precedence(dev, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    gpath, gstate = _generator_file(tmp_path, 'compact')
    dpath, dstate = _disc_file(tmp_path)
    other = _trainer(dev, 'compact', True, seed=7, prepare=False, ema_decay=0.5)
    other.discriminator.load_state_dict(unet_ref.seeded_state(unet_ref.UNetRef(), 12))
    other.gen_ema.data.mul_(0.5)  # (an average that is not the weights)
    saved = other._model_state(3, 'compact-gan')
    assert not torch.equal(saved['params_ema']['body.0.weight'], saved['state']['body.0.weight'])
    live = lambda t: {k: v.cpu() for k, v in t.generator.state_dict().items()}  # noqa: E731
    # a stray compact-psnr-latest.pth and --pretrain-epochs 0: the init files win, in both phases' loaders
    torch.save(saved, 'compact-psnr-latest.pth')
    t = _trainer(dev, 'compact', True, prepare=False, init_generator=gpath, init_discriminator=dpath, ema_decay=0.5)
    t.pre_epochs = t.epochs = 0  # (no epoch runs: what is checked is which file each phase starts from)
    t._pretrain()
    t._gan_train()
    _same_bits(live(t), dict(gstate), 'G after both phases looked for checkpoints')
    _same_bits({k: v.cpu() for k, v in t.discriminator.state_dict().items()}, dstate, 'D')
    assert torch.equal(t.gen_ema.data, t.gen_flat.data)
    assert 'not used' not in capsys.readouterr().out
    # with pre-training epochs the pre-training phase resumes from its checkpoint, as it always did, and says so
    t = _trainer(dev, 'compact', True, prepare=False, init_generator=gpath, ema_decay=0.5)
    t.pre_epochs = t.epochs = 0
    t.pre_epochs = 1
    saved_epoch = dict(saved, epoch=1)  # (resumed: continues with epoch 2 > pre_epochs, so no epoch runs)
    torch.save(saved_epoch, 'compact-psnr-latest.pth')
    t._pretrain()
    _same_bits(live(t), saved['state'], 'G resumed from compact-psnr-latest.pth')
    out = capsys.readouterr().out
    assert out.count('not used') == 1 and f'--init-generator {gpath} not used' in out
    os.remove('compact-psnr-latest.pth')
    # a compact-gan-latest.pth: that checkpoint wins, the average it holds included, and one line says so
    torch.save(saved, 'compact-gan-latest.pth')
    t = _trainer(dev, 'compact', True, prepare=False, init_generator=gpath, init_discriminator=dpath, ema_decay=0.5)
    t.pre_epochs = t.epochs = 0
    t._pretrain()
    t._gan_train()
    _same_bits(live(t), saved['state'], 'G resumed from compact-gan-latest.pth')
    _same_bits({k: v.cpu() for k, v in t.discriminator.state_dict().items()}, saved['resume']['discriminator'], 'D resumed')
    _same_bits(t.gen_ema.state_dict(t.generator), saved['params_ema'], 'the average resumed')
    out = capsys.readouterr().out
    assert out.count('not used') == 1
    assert f'Resuming from compact-gan-latest.pth: --init-generator {gpath} and --init-discriminator {dpath} not used' in out


# ------------------------------------------------------------------ 5. --pixel-weight
def test_pixel_weight(dev):
    """``gan/train-loss = w pixel + content + 0.1 adversarial`` from the logged components.  The step forms it in two launches of
    two products and a sum each: at most six roundings of partial results no larger than the sum of the terms' magnitudes, so the
    fp64 value of the fp32 components is within 6 u of that sum; 8 u is asserted."""
    lr, hr = _batch(dev)
    losses = {}
    for name, extra in (('absent', {}), ('default', {'pixel_weight': 0.01}), ('one', {'pixel_weight': 1.0})):
        t = _trainer(dev, 'compact', False, **extra)
        assert t.pixel_weight == (1.0 if name == 'one' else 0.01)
        first = {k: v.item() for k, v in t.gan_step(lr, hr).items()}
        t.gan_step(lr, hr)
        losses[name] = (first, t.gen_flat.data.clone(), t.adversarial_weight)
    for name, w in (('default', float(np.float32(0.01))), ('one', 1.0)):
        first, _flat, adv_w = losses[name]
        terms = [w * first['gan/pixel-loss'], first['gan/content-loss'], float(np.float32(adv_w)) * first['gan/adversarial-loss']]
        err, bound = abs(first['gan/train-loss'] - sum(terms)), 8 * U * sum(abs(x) for x in terms)
        print(f'pixel weight {w}: train loss {first["gan/train-loss"]!r}, from its terms {sum(terms)!r}, error {err:.3e}, bound {bound:.3e}')
        assert err <= bound, (name, err, bound)
    assert losses['absent'][0] == losses['default'][0] and torch.equal(losses['absent'][1], losses['default'][1])
    assert losses['one'][0]['gan/pixel-loss'] == losses['default'][0]['gan/pixel-loss']  # the first step's terms are the same ...
    assert losses['one'][0]['gan/train-loss'] != losses['default'][0]['gan/train-loss']  # ... their sum is not
    assert not torch.equal(losses['one'][1], losses['default'][1])


# ------------------------------------------------------------------ 6. two ranks
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _ddp_worker(rank, world, port, gpath, out):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY='0')
    import hashlib
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from oracle.weights import closed_form_state, seeded_input, step_state
        from torchsr_amd.esrgan.trainer import ESRGANTrainer
        dev = torch.device('cuda', 0)
        torch.cuda.set_device(dev)
        args = Namespace(disable_amp=True, batch_size=2, epochs=8, gan_checkpoint=None, local_rank=0, pretrain_epochs=1,
                         psnr_checkpoint=None, skip_image_save=True, world_size=world, rank=rank, use_graphs=False,
                         vgg_weights='random', ema_decay=0.5, init_generator=gpath)
        torch.manual_seed(100 + rank)  # (different starts: the init file and the broadcast make the ranks equal)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            t = ESRGANTrainer(dev, args, [], [], 2, 2, distributed=True)
        t.discriminator.load_state_dict(step_state(t.discriminator.state_dict(), 'esrgan.D'))
        t.vgg_loss.features.load_state_dict(closed_form_state(t.vgg_loss.features.state_dict(), prefix='features.'))
        t.generator.train()
        t.discriminator.train()
        lr, hr = seeded_input((2, 3, 32, 32), 270 + rank).to(dev), seeded_input((2, 3, 128, 128), 280 + rank).to(dev)
        ema0, weights = t.gen_ema.data.cpu(), []
        for _ in range(2):
            t.gan_step(lr, hr)
            weights.append(t.gen_flat.data.cpu())
        got = t.gen_ema.data.cpu()
        want, bound = _recurrence(ema0, weights, 0.5)
        ratio = ((got.double() - want).abs() / bound.clamp_min(1e-300)).max().item()
        digest = lambda x: hashlib.sha256(x.numpy().tobytes()).hexdigest()  # noqa: E731
        out[rank] = {'blocks': len(t.generator.blocks), 'ema': digest(got), 'live': digest(weights[-1]), 'ema0': digest(ema0),
                     'ratio': ratio, 'finite': bool(torch.isfinite(got).all()), 'moved': not torch.equal(got, weights[-1])}
        torch.cuda.synchronize()
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_hold_the_same_average(dev, tmp_path):
    """Two ranks on one GPU over gloo (tests/test_ddp_gpu.py): 2 segmented GAN steps of a two-block ESRGAN trainer started from
    --init-generator with --ema-decay 0.5.  Every rank averages the same weights, so the buffers are equal without a collective."""
    gpath = str(tmp_path / 'g.pth')
    torch.save({'params_ema': rrdbnet_ref.seeded_state(rrdbnet_ref.RRDBNetRef(num_block=2), 24)}, gpath)
    world, port = 2, _free_port()
    mgr = mp.get_context('spawn').Manager()
    out = mgr.dict()
    mp.spawn(_ddp_worker, args=(world, port, gpath, out), nprocs=world, join=True)
    assert len(out) == world
    print({r: (out[r]['ratio'], out[r]['ema'][:12]) for r in range(world)})
    for rank in range(world):
        rep = out[rank]
        assert rep['blocks'] == 2 and rep['finite'] and rep['moved'], (rank, rep)
        assert rep['ratio'] <= 1.0, (rank, rep)
    assert out[0]['ema'] == out[1]['ema'] and out[0]['live'] == out[1]['live'] and out[0]['ema0'] == out[1]['ema0']
