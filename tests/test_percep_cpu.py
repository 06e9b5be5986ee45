"""``train --perceptual realesrgan`` without a GPU: the command line, the module's layout and weight loading, and the reference
(tests/percep_ref.py) against an independent formulation of itself."""
import warnings

import pytest
import torch

import percep_ref as R
from oracle.weights import closed_form_state


def test_cli_perceptual_flag():
    from torchsr_amd.torchsr import parse_args
    base = ['train', '--train-dir', 'synthetic:8']
    assert parse_args(base).perceptual == 'single'
    for model in ('esrgan', 'compact'):
        for disc in ('vgg', 'unet'):
            args = parse_args(base + ['--model', model, '--discriminator', disc, '--perceptual', 'realesrgan'])
            assert args.perceptual == 'realesrgan'
    assert parse_args(base + ['--model', 'srgan', '--perceptual', 'single']).perceptual == 'single'
    with pytest.raises(SystemExit):
        parse_args(base + ['--model', 'srgan', '--perceptual', 'realesrgan'])
    with pytest.raises(SystemExit):
        parse_args(base + ['--model', 'esrgan', '--perceptual', 'five'])


def test_perceptual_loss_layout_and_freeze():
    from torchsr_amd.layers import ACT_NONE, ACT_RELU, Conv2d
    from torchsr_amd.realesrgan.loss import PerceptualLoss, vgg19_conv_names
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        p = PerceptualLoss()
    assert any('seeded random features' in str(w.message) for w in seen)   # VGGLoss's warning; 'random' is the opt-in
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        PerceptualLoss(weights='random')
    convs = [m for m in p.features if isinstance(m, Conv2d)]
    assert len(convs) == 16 and len(p.features) == 35 and isinstance(p.features[-1], Conv2d)
    assert list(p.features.state_dict()) == [f'{i}.{k}' for i in R.CONV_INDICES for k in ('weight', 'bias')]
    assert list(p.state_dict()) == [f'features.{i}.{k}' for i in R.CONV_INDICES for k in ('weight', 'bias')]
    assert sum(q.numel() for q in p.parameters()) == 20024384
    assert not any(q.requires_grad for q in p.parameters()) and not p.features.training
    assert p.layer_weights == R.LAYER_WEIGHTS and p.mean == R.MEAN and p.std == R.STD
    names = vgg19_conv_names()
    assert names == [name for _, kind, name in R.layout() if kind == 'conv']
    for name, m in zip(names, convs):
        assert m._st.act == (ACT_NONE if name in R.LAYER_WEIGHTS else ACT_RELU), name
    layers, taps = p._stack()
    assert [kind for kind, _ in layers].count('pool') == 4 and len(layers) == 20
    assert taps == {1: 0.1, 4: 0.1, 9: 1.0, 14: 1.0, 19: 1.0}
    # the seeded random features are VGGLoss's own draws (same generator, same order), and the reference's copy of them
    from torchsr_amd.srgan.loss import VGGLoss
    sd, ref = p.features.state_dict(), R.random_state()
    for k, v in VGGLoss(weights='random').features.state_dict().items():
        assert torch.equal(sd[k], v) and torch.equal(ref[k], v), k


def test_perceptual_loss_loads_a_torchvision_shaped_state_dict(tmp_path, monkeypatch):
    from torchsr_amd.realesrgan.loss import PerceptualLoss
    from torchsr_amd.srgan.loss import make_vgg19_features
    own = make_vgg19_features(36).state_dict()
    full = {f'features.{k}': v for k, v in closed_form_state(own, prefix='features.').items()}
    for i in (0, 3, 6):
        full[f'classifier.{i}.weight'], full[f'classifier.{i}.bias'] = torch.ones(4, 4), torch.ones(4)
    path = tmp_path / 'vgg19-dcbb9e9d.pth'
    torch.save(full, path)
    p = PerceptualLoss(weights=str(path))
    assert p.pretrained and not p.features.training and not any(q.requires_grad for q in p.parameters())
    got = p.features.state_dict()
    assert list(got) == list(own)
    for k, t in got.items():
        assert torch.equal(t, full['features.' + k]), k
    monkeypatch.setenv('TORCHSR_VGG19_WEIGHTS', str(path))
    assert PerceptualLoss().pretrained
    torch.save({k: v for k, v in full.items() if not k.startswith('features.34')}, tmp_path / 'short.pth')
    with pytest.raises(RuntimeError, match='Missing key'):
        PerceptualLoss(weights=str(tmp_path / 'short.pth'))


def test_trainer_refuses_realesrgan_for_srgan_and_unknown_names():
    """The choice is made in ``_perceptual_loss``; called here on bare instances (the trainers themselves need the GPU)."""
    from torchsr_amd.esrgan.trainer import ESRGANTrainer
    from torchsr_amd.realesrgan.loss import PerceptualLoss
    from torchsr_amd.srgan.loss import VGGLoss
    from torchsr_amd.srgan.trainer import SRGANTrainer
    t = SRGANTrainer.__new__(SRGANTrainer)
    t.vgg_weights, t.perceptual = 'random', 'realesrgan'
    with pytest.raises(RuntimeError, match='SRGAN trainer keeps'):
        t._perceptual_loss()
    e = ESRGANTrainer.__new__(ESRGANTrainer)
    e.vgg_weights, e.perceptual = 'random', 'realesrgan'
    assert type(e._perceptual_loss()) is PerceptualLoss
    e.perceptual = 'single'
    assert type(e._perceptual_loss()) is VGGLoss
    e.perceptual = 'five'
    with pytest.raises(RuntimeError, match='not supported'):
        e._perceptual_loss()


def _inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g), torch.rand(shape, generator=g)


def test_reference_equals_hooked_formulation_fp64():
    sd = R.random_state(dtype=torch.float64)
    for shape, seed in (((2, 3, 16, 16), 3), ((1, 3, 32, 48), 4)):
        src, tgt = (t.double() for t in _inputs(shape, seed))
        a, b = R.perceptual_loss(sd, src, tgt).item(), R.hooked_loss(sd, src, tgt).item()
        assert a > 0 and abs(a - b) <= 1e-12 * abs(b), (shape, a, b)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_relu_and_pool_commute_bit_for_bit(dtype):
    """``maxpool(relu(x)) == relu(maxpool(x))``: both orders of the reference give the same bits, features, loss and gradient."""
    sd = R.random_state(dtype=dtype)
    src, tgt = (t.to(dtype) for t in _inputs((2, 3, 16, 32), 5))
    fa, fb = R.features(sd, src), R.features(sd, src, pool_first=True)
    assert list(fa) == list(R.LAYER_WEIGHTS) and all(torch.equal(fa[k], fb[k]) for k in fa)
    grads = []
    for pool_first in (False, True):
        x = src.clone().requires_grad_(True)
        loss = R.perceptual_loss(sd, x, tgt, pool_first=pool_first)
        loss.backward()
        grads.append((loss.detach(), x.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    x = torch.randn(3, 8, 6, 10, dtype=dtype)
    assert torch.equal(torch.nn.functional.max_pool2d(torch.relu(x), 2, 2), torch.relu(torch.nn.functional.max_pool2d(x, 2, 2)))


def test_bf16_mode_rounds_conv_operands():
    """The bf16-products mode: storing the inter-conv activations as bf16 changes nothing (their consumers round them anyway),
    and the result differs from fp32 by bf16-sized, not fp32-sized, amounts."""
    sd = R.random_state(dtype=torch.float64)
    src, tgt = (t.double() for t in _inputs((1, 3, 16, 16), 6))
    exact, b16 = R.perceptual_loss(sd, src, tgt).item(), R.perceptual_loss(sd, src, tgt, bf16=True).item()
    assert 1e-6 < abs(b16 - exact) / exact < 5e-2
    assert R.perceptual_loss(sd, src, tgt, bf16=True, pool_first=True).item() == b16
