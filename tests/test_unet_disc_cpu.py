"""``--discriminator unet`` without a GPU: the closed forms the kernels implement against torch autograd in fp64, the module's
state-dict schema against the reference restatement (tests/unet_ref.py), the command line, and the refusals of the new ABI."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import unet_ref as R


@pytest.mark.parametrize('rows,cols,k', [(8, 36, 2), (64, 576, 3)])
def test_closed_form_sn_backward_equals_autograd_through_spectral_norm(rows, cols, k):
    """dW = (G - <G, W_sn> u v^T) / sigma, u and v the (constant) vectors of the forward: equal to autograd through
    torch.nn.utils.spectral_norm's training forward in fp64, to rounding."""
    cin = cols // (k * k)
    g = torch.Generator().manual_seed(rows)
    conv = torch.nn.utils.spectral_norm(torch.nn.Conv2d(cin, rows, k, bias=False)).double()
    w = conv.weight_orig.detach().numpy().reshape(rows, cols).copy()
    u0, v0 = conv.weight_u.numpy().copy(), conv.weight_v.numpy().copy()
    x = torch.randn(2, cin, k + 2, k + 3, generator=g, dtype=torch.float64)
    y = conv(x)
    go = torch.randn(y.shape, generator=g, dtype=torch.float64)
    # G = dL/dW_sn of the same loss, from a plain conv on the normalised weight
    w_sn, sigma, u, v = R.sn_forward(w, u0, v0, train=True)
    np.testing.assert_allclose(u, conv.weight_u.numpy(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(v, conv.weight_v.numpy(), rtol=0, atol=1e-13)
    wt = torch.from_numpy(w_sn.reshape(rows, cin, k, k)).requires_grad_(True)
    np.testing.assert_allclose(TF.conv2d(x, wt).detach().numpy(), y.detach().numpy(), rtol=0, atol=1e-12)
    (TF.conv2d(x, wt) * go).sum().backward()
    (y * go).sum().backward()
    mine = R.sn_backward(wt.grad.numpy().reshape(rows, cols), w_sn, u, v, sigma)
    want = conv.weight_orig.grad.numpy().reshape(rows, cols)
    assert np.abs(mine - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_eval_forward_takes_sigma_from_the_stored_vectors():
    g = np.random.default_rng(0)
    w, u, v = g.standard_normal((8, 36)), g.standard_normal(8), g.standard_normal(36)
    w_sn, sigma, u1, v1 = R.sn_forward(w, u, v, train=False)
    assert u1 is u and v1 is v and sigma == u @ (w @ v)
    np.testing.assert_array_equal(w_sn, w / sigma)


@pytest.mark.parametrize('h,w', [(1, 1), (2, 3), (5, 7)])
def test_bilinear_tables_and_their_transpose_equal_interpolate_and_its_autograd(h, w):
    g = torch.Generator().manual_seed(h * 10 + w)
    x = torch.randn(2, 3, h, w, generator=g, dtype=torch.float64, requires_grad=True)
    y = TF.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    np.testing.assert_allclose(R.bilinear2x_forward(x.detach().numpy()), y.detach().numpy(), rtol=0, atol=1e-14)
    np.testing.assert_allclose(R.bilinear2x_backward(dy.numpy()), x.grad.numpy(), rtol=0, atol=1e-14)
    t = R.bilinear2x_table(h)
    assert (t.sum(1) == 1).all() and (np.count_nonzero(t, axis=0) <= 4).all()  # an input row feeds at most four output rows


def test_state_dict_keys_and_shapes_equal_the_reference_in_order():
    from torchsr_amd.realesrgan.discriminator import UNetDiscriminatorSN
    mine, ref = UNetDiscriminatorSN().state_dict(), R.UNetRef().state_dict()
    assert [(k, tuple(v.shape)) for k, v in mine.items()] == [(k, tuple(v.shape)) for k, v in ref.items()]
    assert list(mine)[:5] == ['conv0.weight', 'conv0.bias', 'conv1.weight_orig', 'conv1.weight_u', 'conv1.weight_v']
    m = UNetDiscriminatorSN()
    assert isinstance(m.conv1.weight_orig, torch.nn.Parameter) and not isinstance(m.conv1.weight_u, torch.nn.Parameter)
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in R.UNetRef().named_parameters()]
    m.load_state_dict(R.seeded_state(R.UNetRef(), 3), strict=True)  # a state the reference module made loads key for key
    small = UNetDiscriminatorSN(num_feat=8, skip_connection=False).state_dict()
    assert tuple(small['conv3.weight_orig'].shape) == (64, 32, 4, 4) and tuple(small['conv3.weight_v'].shape) == (512,)


def test_cli_accepts_unet_for_esrgan_and_compact_refuses_srgan_and_defaults_to_vgg(capsys):
    from torchsr_amd.models import select_trainer_model
    from torchsr_amd.realesrgan.trainer import UNetCompactTrainer, UNetESRGANTrainer
    from torchsr_amd.compact.trainer import CompactTrainer
    from torchsr_amd.esrgan.trainer import ESRGANTrainer
    from torchsr_amd.realesrgan.discriminator import UNetDiscriminatorSN
    from torchsr_amd.torchsr import parse_args
    for model, plain, unet in (('esrgan', ESRGANTrainer, UNetESRGANTrainer), ('compact', CompactTrainer, UNetCompactTrainer)):
        args = parse_args(['train', '--model', model])
        assert args.discriminator == 'vgg' and select_trainer_model(args) == (plain, 128)
        assert select_trainer_model(parse_args(['train', '--model', model, '--discriminator', 'vgg'])) == (plain, 128)
        args = parse_args(['train', '--model', model, '--discriminator', 'unet'])
        cls, crop = select_trainer_model(args)
        assert cls is unet and issubclass(cls, plain) and crop == 128 and cls.discriminator_cls is UNetDiscriminatorSN
        assert plain.discriminator_cls is not UNetDiscriminatorSN
    with pytest.raises(SystemExit):
        parse_args(['train', '--model', 'srgan', '--discriminator', 'unet'])
    assert '--discriminator unet trains with --model esrgan or --model compact' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(['train', '--model', 'esrgan', '--discriminator', 'patch'])
    ns = parse_args(['train', '--model', 'esrgan'])
    ns.model, ns.discriminator = 'srgan', 'unet'  # (a caller that builds the namespace itself)
    with pytest.raises(RuntimeError, match='--discriminator unet trains with'):
        select_trainer_model(ns)


def test_sizes_that_are_no_multiple_of_8_are_refused_before_anything_runs():
    from torchsr_amd.realesrgan.discriminator import UNetDiscriminatorSN
    m = UNetDiscriminatorSN(num_feat=8)
    for shape in ((1, 3, 12, 16), (1, 3, 16, 20), (1, 3, 7, 8)):
        with pytest.raises(ValueError, match='multiples of 8'):
            m(torch.zeros(shape))  # (a CPU tensor: the refusal comes before the first device check)
    with pytest.raises(ValueError, match='multiples of 8'):
        m.forward_nhwc(torch.zeros(1, 12, 16, 4))


def test_trainer_refuses_a_process_group_with_a_message():
    from argparse import Namespace
    from torchsr_amd.realesrgan.trainer import UNetESRGANTrainer
    with pytest.raises(RuntimeError, match='does not run under a process group'):
        UNetESRGANTrainer('cuda', Namespace(), None, None, 0, 0, distributed=True)


def test_abi_refuses_bad_spectral_norm_and_bilinear_arguments():
    """Null or misaligned pointers, cols that are no multiple of 4, rows * cols >= 2^31 and a short workspace are refused with
    a status code BEFORE anything is launched -- so the checks run with fake pointers that are never dereferenced."""
    from torchsr_amd import _lib
    lib = _lib.lib()
    fake = 0x10000

    def err():
        buf = C.create_string_buffer(256)
        lib.srx_last_error(buf, 256)
        return buf.value.decode()

    nws = lib.srx_spectral_norm_ws_floats(64, 576)
    assert nws >= 576 + 64
    fwd = lambda **kw: lib.srx_spectral_norm_fwd(*[kw.get(k, d) for k, d in (  # noqa: E731
        ('W', fake), ('u', fake + 0x100000), ('v', fake + 0x200000), ('out', fake + 0x300000), ('sigma', fake + 0x400000),
        ('keep', None), ('rows', 64), ('cols', 576), ('train', 1), ('ws', fake + 0x500000), ('nws', nws), ('stream', None))])
    assert fwd(W=None) != 0 and 'null' in err()
    assert fwd(ws=None) != 0 and 'null' in err()
    assert fwd(W=fake + 4) != 0 and 'aligned' in err()
    assert fwd(v=fake + 8) != 0 and 'aligned' in err()
    assert fwd(keep=fake + 4) != 0 and 'aligned' in err()
    assert fwd(out=fake) != 0 and 'must not be W' in err()
    assert fwd(cols=578) != 0 and 'multiple of 4' in err()
    assert fwd(rows=0) != 0
    assert fwd(rows=1 << 16, cols=1 << 15) != 0 and '2^31' in err()
    assert fwd(nws=nws - 1) != 0 and 'workspace' in err()
    bwd = lambda **kw: lib.srx_spectral_norm_bwd(*[kw.get(k, d) for k, d in (  # noqa: E731
        ('G', fake), ('W', fake + 0x100000), ('u', fake + 0x200000), ('v', fake + 0x300000), ('sigma', fake + 0x400000),
        ('dW', fake + 0x500000), ('acc', 0), ('rows', 64), ('cols', 576), ('ws', fake + 0x600000), ('nws', nws), ('stream', None))])
    assert bwd(G=None) != 0 and 'null' in err()
    assert bwd(dW=fake + 0x500004) != 0 and 'aligned' in err()
    assert bwd(cols=2) != 0 and 'multiple of 4' in err()
    assert bwd(rows=1 << 16, cols=1 << 15) != 0 and '2^31' in err()
    assert bwd(nws=0) != 0 and 'workspace' in err()
    for name in ('srx_upsample_bilinear2x_fwd', 'srx_upsample_bilinear2x_bwd'):
        fn = getattr(lib, name)
        assert fn(None, fake, 1, 2, 2, 4, 4, None) != 0 and 'null' in err()
        assert fn(fake, fake, 1, 2, 2, 4, 4, None) != 0 and 'aliased' in err()
        assert fn(fake, fake + 0x100004, 1, 2, 2, 4, 4, None) != 0 and 'aligned' in err()
        assert fn(fake, fake + 0x100000, 1, 2, 2, 4, 6, None) != 0 and 'multiple of 4' in err()
        assert fn(fake, fake + 0x100000, 1, 2, 2, 6, 4, None) != 0  # six channels do not fit a stride of four
        assert fn(fake, fake + 0x100000, 1, 0, 2, 4, 4, None) != 0
