"""CPU-side tests (no GPU): the oracle against the golden vectors captured from the reference,
the C-ABI library's exports, host logic (registry, flat buffers, schedulers, schema)."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from oracle import srgan as O
from oracle.weights import closed_form_state, step_state, tensor_digest


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


# ------------------------------------------------------------------ oracle pinned by the goldens
@pytest.mark.parametrize('tag', ['a', 'b'])
def test_oracle_generator_matches_reference_golden(tag):
    from torchsr_amd.srgan.generator import Generator
    gold = np.load(os.path.join(GOLDEN, 'srgan_generator.npz'))
    sd = closed_form_state(Generator().state_dict())
    leaves = O._leaves(sd)
    x = torch.from_numpy(gold[f'{tag}_x']).requires_grad_(True)
    y = O.generator_forward(sd, x, True)
    assert rel(y, gold[f'{tag}_y_train']) < 1e-5
    y.square().mean().backward()
    assert rel(x.grad, gold[f'{tag}_dx']) < 1e-4
    names = [k for k, v in sd.items() if v.is_floating_point() and 'running_' not in k]
    dig = dict(zip((str(k) for k in gold[f'{tag}_grad_keys']), gold[f'{tag}_grad_digest']))
    for k, leaf in zip(names, leaves):
        d = tensor_digest(leaf.grad)
        assert abs(d[0] - dig[k][0]) <= 1e-4 * max(dig[k][1], 1e-12), k
    ye = O.generator_forward(sd, x.detach(), False)
    assert rel(ye, gold[f'{tag}_y_eval']) < 1e-5


@pytest.mark.parametrize('tag,size', [('s32', 32), ('s96', 96)])
def test_oracle_discriminator_matches_reference_golden(tag, size):
    from torchsr_amd.srgan.discriminator import Discriminator
    gold = np.load(os.path.join(GOLDEN, 'srgan_discriminator.npz'))
    sd = closed_form_state(Discriminator(image_size=size).state_dict())
    p = O.discriminator_forward(sd, torch.from_numpy(gold[f'{tag}_x']), True)
    assert rel(p, gold[f'{tag}_p_train']) < 1e-5
    pe = O.discriminator_forward(sd, torch.from_numpy(gold[f'{tag}_x']), False)
    assert rel(pe, gold[f'{tag}_p_eval']) < 1e-5


def test_oracle_vgg_matches_reference_golden():
    from torchsr_amd.srgan.loss import make_vgg19_features
    gold = np.load(os.path.join(GOLDEN, 'vgg19.npz'))
    sd = closed_form_state(make_vgg19_features().state_dict(), prefix='features.')
    feat = O.vgg_features(sd, torch.from_numpy(gold['src']))
    assert rel(feat, gold['features']) < 1e-5
    loss = O.vgg_loss(sd, torch.from_numpy(gold['src']), torch.from_numpy(gold['tgt']))
    assert abs(loss.item() - float(gold['loss'])) < 1e-5 * float(gold['loss'])


def test_oracle_gan_steps_match_reference_trainer_golden():
    """Two consecutive steps: the fixtures start from ``step_state`` weights, which keep the discriminator out of
    saturation, so the second step pins arithmetic as well as the first."""
    from torchsr_amd.srgan.discriminator import Discriminator
    from torchsr_amd.srgan.generator import Generator
    from torchsr_amd.srgan.loss import make_vgg19_features
    gold = np.load(os.path.join(GOLDEN, 'srgan_steps.npz'))
    torch.set_num_threads(8)
    orc = O.SRGANStepOracle(step_state(Generator().state_dict(), 'srgan.G'), step_state(Discriminator().state_dict(), 'srgan.D'),
                            closed_form_state(make_vgg19_features().state_dict(), prefix='features.'))
    keys = [str(k) for k in gold['g_keys']]
    assert 0.5 < gold['gan_losses'][2][0] < 2.0  # disc-loss is still O(1) at the third step
    for step in range(2):
        out = orc.gan_step(torch.from_numpy(gold['low_res']), torch.from_numpy(gold['high_res']))
        assert np.allclose(out, gold['gan_losses'][step], rtol=1e-5)
        assert abs(out[3] - gold['gan_ref_gen_losses'][step]) < 2e-5 * out[3]
        for k, dg in zip(keys, gold['gan_g_digest'][step]):
            d = tensor_digest(orc.g[k].detach())
            assert abs(d[1] - dg[1]) <= 1e-5 * max(dg[1], 1e-9), (step, k)


def test_oracle_esrgan_matches_reference_golden():
    from oracle import esrgan as OE
    from torchsr_amd.esrgan.discriminator import Discriminator
    from torchsr_amd.esrgan.generator import Generator
    gold = np.load(os.path.join(GOLDEN, 'esrgan.npz'))
    sd = closed_form_state(Generator(num_rrdb_blocks=2).state_dict())
    assert rel(OE.generator_forward(sd, torch.from_numpy(gold['g_x'])), gold['g_y']) < 1e-5
    sd = closed_form_state(Discriminator(image_size=64).state_dict())
    assert rel(OE.discriminator_forward(sd, torch.from_numpy(gold['d_x']), True), gold['d_logits']) < 1e-5
    assert len(Generator().state_dict()) == 702 and len(Discriminator().state_dict()) == 60
    assert 0.3 < gold['gan_losses'][2][0] < 1.0 and gold['gan_losses'][0][1] < 5.0  # un-saturated D, O(1) image


# ------------------------------------------------------------------ C ABI
def test_library_exports_every_declared_symbol():
    from torchsr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    handle = _lib.load_handle(_lib.LIB_PATH)   # (on a GPU box: after torch has initialised HIP)
    header = open(os.path.join(ROOT, 'include', 'srx.h')).read()
    declared = set(re.findall(r'\b(srx_[a-z0-9_]+)\s*\(', header))
    assert declared, 'no declarations found'
    for name in declared:
        assert hasattr(handle, name), f'{name} declared in include/srx.h but not exported'
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    assert handle.srx_version() == 100


def test_size_queries_and_error_reporting_without_gpu():
    from torchsr_amd import _lib
    L = _lib.lib()
    d = _lib.Conv2dDesc(16, 24, 24, 64, 64, 64, 64, 3, 3, 1, 1, 0, 0, 0.0, 0)
    assert L.srx_conv2d_packed_fwd_floats(ctypes.byref(d)) == 64 * 576
    assert L.srx_conv2d_packed_bwd_floats(ctypes.byref(d)) == 64 * 576
    d2 = _lib.Conv2dDesc(16, 96, 96, 64, 64, 64, 64, 3, 3, 2, 1, 0, 0, 0.0, 0)
    # stride 2: four parity classes with 1+2+2+4 = 9 taps in total, no wasted work
    assert L.srx_conv2d_packed_bwd_floats(ctypes.byref(d2)) == 64 * 64 * 9
    bad = _lib.Conv2dDesc(16, 24, 24, 64, 62, 64, 64, 3, 3, 1, 1, 0, 0, 0.0, 0)
    assert L.srx_conv2d_packed_fwd_floats(ctypes.byref(bad)) == 0
    assert 'Cin_s' in _lib.last_error()
    with pytest.raises(RuntimeError, match='bad argument'):
        _lib.call('srx_nchw_to_nhwc', None, None, 1, 3, 4, 4, 4, None)


def test_ops_refuse_cpu_tensors():
    from torchsr_amd import functional as F
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.to_nhwc(torch.rand(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.mse_loss(torch.rand(4), torch.rand(4))


# ------------------------------------------------------------------ host logic
def test_state_dict_schema_and_seeded_init_match_reference_counts():
    from torchsr_amd.srgan.discriminator import Discriminator
    from torchsr_amd.srgan.generator import Generator
    g, d = Generator(), Discriminator()
    assert len(g.state_dict()) == 225 and len(d.state_dict()) == 48
    assert sum(p.numel() for p in g.parameters()) == 1547350
    assert sum(p.numel() for p in d.parameters()) == 23563649
    assert g.state_dict()['conv_layers.1.conv.weight'].shape == (256, 64, 3, 3)
    assert d.state_dict()['classifier.0.weight'].shape == (1024, 18432)
    assert Discriminator(image_size=32).classifier[0].in_features == 2048
    assert len(Generator(scale_factor=2).conv_layers) == 1


def test_vgg_layout_and_freeze():
    from torchsr_amd.srgan.loss import VGGLoss, make_vgg19_features
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        v = VGGLoss()
    keys = list(v.features.state_dict().keys())
    convs = [0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28, 30, 32, 34]
    assert keys == [f'{i}.{p}' for i in convs for p in ('weight', 'bias')]
    assert len(v.features) == 36 and sum(p.numel() for p in v.parameters()) == 20024384
    assert not any(p.requires_grad for p in v.parameters()) and not v.features.training
    assert [i for i, k in O.vgg_feature_layout() if k == 'conv'] == convs
    with pytest.raises(RuntimeError):
        make_vgg19_features(1)


def test_flat_params_views_and_zero_grad():
    from torchsr_amd.optim import FlatParams
    m = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 2))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    f = FlatParams(m)
    assert f.numel == 16 + 4 + 8 + 4  # each tensor padded to 4 floats
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k])
    m(torch.rand(4, 5)).sum().backward()
    assert f.grad.abs().sum() > 0 and m[0].weight.grad.data_ptr() == f.grad.data_ptr()
    f.zero_grad()
    assert f.grad.abs().sum() == 0
    with torch.no_grad():
        f.data.add_(1.0)
    assert torch.allclose(m[1].bias, before['1.bias'] + 1.0)
    m.load_state_dict(before)
    assert torch.equal(f.data[:15], before['0.weight'].flatten())


def test_vgg19_cfg_is_torchvision_cfg_e():
    """A literal copy of torchvision.models.vgg cfgs['E'] (public definition), written out here so that a typo
    shared by oracle.srgan.VGG19_CFG, the golden-fixture stub and the product cannot pass unnoticed."""
    from torchsr_amd.srgan.loss import VGG19_CFG
    cfg_e = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 256, 'M', 512, 512, 512, 512, 'M', 512, 512, 512, 512, 'M']
    assert VGG19_CFG == cfg_e and O.VGG19_CFG == cfg_e
    assert sum(1 for v in cfg_e if v != 'M') == 16 and len(cfg_e) + 16 == 37  # features[:36] drops the 5th max-pool


def test_steplr_values_match_torch():
    """optim.StepLR against torch.optim.lr_scheduler.StepLR for the reference's settings
    (step_size = epochs // 8, gamma 0.6, stepped once per epoch: torchsr/srgan/trainer.py:186-195,528-529)."""
    from torchsr_amd.optim import StepLR

    class Opt:  # the slice of FlatAdam that StepLR touches; no device needed
        def __init__(self, lr):
            self._lr = lr

        lr = property(lambda self: self._lr)

        def set_lr(self, lr):
            self._lr = float(lr)

    for epochs in (8, 20, 64, 1000):
        mine_opt = Opt(1e-4)
        mine = StepLR(mine_opt, step_size=epochs // 8, gamma=0.6)
        p = torch.nn.Parameter(torch.zeros(1))
        ref_opt = torch.optim.Adam([p], lr=1e-4)
        ref = torch.optim.lr_scheduler.StepLR(ref_opt, step_size=epochs // 8, gamma=0.6)
        for epoch in range(min(epochs, 40)):
            ref_opt.step()
            ref.step()
            mine.step()
            assert mine.get_last_lr()[0] == pytest.approx(ref.get_last_lr()[0], rel=1e-12), (epochs, epoch)
        sd = mine.state_dict()
        again = StepLR(Opt(1e-4), step_size=epochs // 8, gamma=0.6)
        again.load_state_dict(sd)
        assert again.get_last_lr() == mine.get_last_lr()
    assert StepLR(Opt(1e-4), step_size=0, gamma=0.6).step_size == 1  # --epochs < 8: the reference divides by zero


def test_cli_refuses_to_train_against_random_vgg_features(monkeypatch, tmp_path):
    """`torchsr train` without the pretrained VGG19 file must not silently optimise a meaningless perceptual
    loss (the reference always loads vgg19(pretrained=True), torchsr/srgan/loss.py:30)."""
    from torchsr_amd.torchsr import main
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv('TORCHSR_VGG19_WEIGHTS', raising=False)
    monkeypatch.setenv('TORCH_HOME', str(tmp_path))
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'LOCAL_WORLD_SIZE', 'SLURM_NTASKS'):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(SystemExit, match='vgg19-dcbb9e9d.pth not found'):
        main(['train', '--model', 'srgan', '--train-dir', 'synthetic:8', '--batch-size', '2'])


def test_backward_cuts_pause_and_resume():
    """ddp.BackwardCuts: a cut splits backward() into two calls whose combined effect is the plain backward."""
    from torchsr_amd import functional as F
    from torchsr_amd.ddp import BackwardCuts
    torch.manual_seed(3)
    a, b = torch.nn.Linear(4, 4), torch.nn.Linear(4, 2)
    x = torch.rand(5, 4)

    def loss_of():  # the body runs twice per step, as the discriminator does (real and fake batch)
        h1, h2 = F.cut_point('mid', torch.tanh(a(x))), F.cut_point('mid', torch.tanh(a(2 * x)))
        return (b(h1) - b(h2)).square().mean()

    loss_of().backward()
    want = [p.grad.clone() for p in list(a.parameters()) + list(b.parameters())]
    for p in list(a.parameters()) + list(b.parameters()):
        p.grad = None
    cuts = BackwardCuts(('mid',))
    F.cut_hook[0] = cuts
    try:
        loss_of().backward()
        assert a.weight.grad is None and b.weight.grad is not None and len(cuts.pairs['mid']) == 2
        cuts.resume('mid')
        with torch.no_grad():  # nothing to cut where nothing is differentiated
            assert F.cut_point('mid', a(x)).requires_grad is False and not cuts.pending('mid')
        cuts.names = set()     # un-armed names pass through
        t = a(x)
        assert F.cut_point('mid', t) is t
    finally:
        F.cut_hook[0] = None
    got = [p.grad for p in list(a.parameters()) + list(b.parameters())]
    for g, w in zip(got, want):
        assert torch.allclose(g, w, rtol=1e-6, atol=1e-8)


def test_steplr_and_registry():
    from argparse import Namespace
    from torchsr_amd import models
    cls, crop = models.select_trainer_model(Namespace(model='SRGAN'))
    assert crop == 96 and cls.__name__ == 'SRGANTrainer'
    assert models.select_test_model(Namespace(model='srgan')).__name__ == 'Generator'
    with pytest.raises(RuntimeError, match='not supported'):
        models.select_trainer_model(Namespace(model='nope'))
    assert set(models.MODELS) == {'esrgan', 'srgan'} and models.CROP_SIZE == {'esrgan': 128, 'srgan': 96}


def test_descriptor_validation_without_a_gpu():
    """Host-side argument checking of the C ABI needs no device: limits and unsupported configurations are
    reported through the status code + srx_last_error, never by aborting."""
    import ctypes as C
    from torchsr_amd import _lib
    lib = _lib.lib()
    out = (C.c_int * 6)()

    def plan_error(*fields):
        d = _lib.Conv2dDesc(*fields)
        rc = lib.srx_conv2d_plan(C.byref(d), 0, out)
        buf = C.create_string_buffer(256)
        lib.srx_last_error(buf, 256)
        return rc, buf.value.decode()

    ok = (16, 24, 24, 64, 64, 64, 64, 3, 3, 1, 1, 0, 0, 0.0, 0, 0)
    assert plan_error(*ok)[0] == 0 and list(out)[:2] == [36, 64]
    # > 2^24 pixels: a whole-frame call (round 4: 64-bit tile bases, exact index division) on 128-row tiles
    assert plan_error(1, 5000, 5000, 64, 64, 64, 64, 3, 3, 1, 1, 0, 0, 0.0, 0, 0)[0] == 0 and out[0] == 128
    rc, msg = plan_error(1, 50000, 50000, 64, 64, 64, 64, 3, 3, 1, 1, 0, 0, 0.0, 0, 0)        # > 2^31 pixels
    assert rc != 0 and 'tile the image' in msg
    rc, msg = plan_error(16, 24, 24, 64, 62, 64, 64, 3, 3, 1, 1, 0, 0, 0.0, 0, 0)              # stride < channels
    assert rc != 0 and 'Cin_s' in msg
    rc, msg = plan_error(16, 24, 24, 64, 64, 60, 60, 3, 3, 1, 1, 2, 0, 0.0, 0, 0)              # shuffle needs Cout % 16
    assert rc != 0 and 'shuffle' in msg
    rc, msg = plan_error(16, 24, 24, 64, 64, 64, 64, 3, 3, 1, 1, 0, 0, 0.0, 3, 0)              # upsample factor
    assert rc != 0 and 'up must be' in msg
    rc, msg = plan_error(16, 24, 24, 64, 64, 64, 64, 3, 3, 2, 1, 0, 0, 0.0, 2, 0)              # fused upsample: stride 1 only
    assert rc != 0 and 'up = 2' in msg
    assert plan_error(16, 24, 24, 64, 64, 64, 64, 3, 3, 1, 1, 0, 0, 0.0, 2, 0)[0] == 0 and out[3] >= 256  # 48x48 output rows
    rc, msg = plan_error(16, 24, 24, 64, 64, 64, 64, 3, 3, 1, 1, 0, 0, 0.0, 0, 7)              # precision
    assert rc != 0 and 'precision' in msg
    rc, msg = plan_error(16, 2, 2, 64, 64, 64, 64, 5, 5, 1, 0, 0, 0, 0.0, 0, 0)                # empty output
    assert rc != 0 and 'empty output' in msg
    d = _lib.Conv2dDesc(*ok)
    assert lib.srx_conv2d_packed_fwd_floats(C.byref(d)) == 64 * 576
    assert lib.srx_conv2d_packed_bwd_floats(C.byref(d)) == 64 * 576
    assert lib.srx_conv2d_stat_rows(C.byref(d)) == 256


def test_abi_refuses_out_of_range_addends_slices_and_scales_without_a_gpu():
    """The three entry points added for the RRDB trunk (round 2) address tensors through caller-supplied strides, channel
    ranges and a host array; every combination that would read or write outside a row is refused with a status code
    BEFORE anything is launched ('the esr17 fault') -- so the checks run here, with fake pointers, on CPU."""
    import ctypes as C
    from torchsr_amd import _lib
    if torch.cuda.is_available():
        pytest.skip('fake pointers: argument validation is exercised where a missed check cannot reach a device')
    lib = _lib.lib()
    fake = 0x10000  # never dereferenced: the calls below must fail in argument validation

    def err():
        buf = C.create_string_buffer(256)
        lib.srx_last_error(buf, 256)
        return buf.value.decode()

    # conv5 of a dense block: 192 input channels (row stride 192), dy dense 64 channels
    d = _lib.Conv2dDesc(2, 8, 8, 192, 192, 64, 64, 3, 3, 1, 1, 0, 0, 0.0, 0, 0)
    e = _lib.DgradEpilogue()
    e.addend, e.addend_ld, e.addend_channels, e.addend_scale, e.out_scale = fake, 64, 0, 1.0, 0.2  # 192 channels from 64-float rows
    rc = lib.srx_conv2d_bwd_data_ex(C.byref(d), fake, fake, fake + 4096, C.byref(e), None, 0, None)
    assert rc != 0 and 'row stride' in err()
    e.addend_channels = 128                                                                       # still wider than the row
    assert lib.srx_conv2d_bwd_data_ex(C.byref(d), fake, fake, fake + 4096, C.byref(e), None, 0, None) != 0 and 'row stride' in err()
    e.addend_ld, e.addend_channels = 62, 60                                                       # not whole quads
    assert lib.srx_conv2d_bwd_data_ex(C.byref(d), fake, fake, fake + 4096, C.byref(e), None, 0, None) != 0 and 'quads' in err()
    e = _lib.DgradEpilogue()
    e.addend, e.addend_scale = fake + 4096, 0.5                                                   # the addend IS the output
    assert lib.srx_conv2d_bwd_data_ex(C.byref(d), fake, fake, fake + 4096, C.byref(e), None, 0, None) != 0 and 'of its own' in err()
    e = _lib.DgradEpilogue()
    e.accumulate, e.out_scale = 1, 0.2                                                            # scaled output + accumulate
    assert lib.srx_conv2d_bwd_data_ex(C.byref(d), fake, fake, fake + 4096, C.byref(e), None, 0, None) != 0
    e = _lib.DgradEpilogue()
    e.act_out, e.act_slope, e.c_lo, e.c_hi = fake, 0.2, 192, 224                                  # mask beyond the row
    assert lib.srx_conv2d_bwd_data_ex(C.byref(d), fake, fake, fake + 4096, C.byref(e), None, 0, None) != 0 and 'masked' in err()
    e.c_lo, e.c_hi = 160, 150                                                                     # empty / unaligned range
    assert lib.srx_conv2d_bwd_data_ex(C.byref(d), fake, fake, fake + 4096, C.byref(e), None, 0, None) != 0 and 'masked' in err()

    # channel slices of srx_axpby_channels / srx_copy_channels
    assert lib.srx_axpby_channels(fake, 192, 160, fake, 192, 0, fake, 64, 0, 64, 128, 0.2, 1.0, None) != 0 and 'out of range' in err()
    assert lib.srx_axpby_channels(fake, 192, 0, fake, 192, 0, fake, 64, 32, 64, 128, 0.2, 1.0, None) != 0 and 'out of range' in err()
    assert lib.srx_axpby_channels(fake, 192, -4, fake, 192, 0, fake, 64, 0, 64, 128, 0.2, 1.0, None) != 0 and 'out of range' in err()
    assert lib.srx_axpby_channels(fake, 192, 2, fake, 192, 0, fake, 64, 0, 64, 128, 0.2, 1.0, None) != 0 and 'multiples of 4' in err()
    assert lib.srx_copy_channels(fake, 64, 0, fake, 192, 160, 64, 128, 0, None) != 0 and 'out of range' in err()

    # grouped / scaled / paired weight gradients
    arr = lambda *v: (C.c_void_p * len(v))(*v)  # noqa: E731
    nws = lib.srx_conv2d_bwd_weight_multi_ws_floats(C.byref(d), 2)
    assert nws > 0
    bad = (C.c_float * 2)(1.0, float('nan'))
    rc = lib.srx_conv2d_bwd_weight_multi_scaled(C.byref(d), 2, 1, arr(fake, fake), arr(fake, fake), arr(fake, fake), 1, None, bad,
                                                fake, nws, None)
    assert rc != 0 and 'not finite' in err()
    ok = (C.c_float * 2)(1.0, 0.2)
    rc = lib.srx_conv2d_bwd_weight_multi_scaled(C.byref(d), 2, 1, arr(fake, fake), arr(fake, fake), arr(fake, fake), 1, None, ok,
                                                fake, 4, None)
    assert rc != 0 and 'workspace' in err()                                                      # short workspace
    rc = lib.srx_conv2d_bwd_weight_multi_scaled(C.byref(d), 3, 2, arr(fake, fake, fake), arr(fake, fake, fake), arr(fake, fake), 1,
                                                None, ok, fake, 1 << 40, None)
    assert rc != 0 and 'whole number of outputs' in err()
    rc = lib.srx_conv2d_bwd_weight_multi_scaled(C.byref(d), 2, 1, arr(fake, None), arr(fake, fake), arr(fake, fake), 1, None, ok,
                                                fake, nws, None)
    assert rc != 0 and 'null tensor' in err()
    dp = _lib.Conv2dDesc(2, 8, 8, 96, 192, 64, 192, 3, 3, 1, 1, 0, 0, 0.0, 0, 0)                  # conv1 + conv2 of a dense block
    rc = lib.srx_conv2d_bwd_weight_multi_pair(C.byref(dp), 1, arr(fake), arr(fake), arr(fake), arr(fake), 128, 1, None, None,
                                              fake, 1 << 40, None)
    assert rc != 0 and 'cin_lo' in err()                                                         # first conv wider than the second
    rc = lib.srx_conv2d_bwd_weight_multi_pair(C.byref(dp), 1, arr(fake), arr(fake), arr(fake), arr(fake), 62, 1, None, None,
                                              fake, 1 << 40, None)
    assert rc != 0 and 'quads' in err()
    rc = lib.srx_conv2d_bwd_weight_multi_pair(C.byref(dp), 1, arr(fake), arr(fake), arr(fake), arr(fake), 64, 1, arr(fake), None,
                                              fake, 1 << 40, None)
    assert rc != 0 and 'both convs or neither' in err()

    # the fused dense block: its output never is the block buffer itself, its second addend never the output
    biases = arr(fake, fake, fake, fake, fake)
    rc = lib.srx_rdb_fwd(1, 8, 8, fake, 192, fake, biases, 0.2, 0.2, 1.0, None, 0, fake, 192, None)
    assert rc != 0 and 'alias' in err()
    rc = lib.srx_rdb_fwd(1, 8, 8, fake, 192, fake, biases, 0.2, 0.2, 0.2, fake + 4096, 192, fake + 4096, 192, None)
    assert rc != 0 and 'of its own' in err()


def test_library_carries_the_digest_of_its_sources(tmp_path):
    """A build is identified by the sha256 of its sources, compiled into the binary (``srx_build_info``): a stale library
    next to newer sources is detected by content, not by file times the builder controls."""
    import ctypes as C
    from torchsr_amd import _lib
    want = _lib.source_digest()
    assert len(want) == 64 and _lib.built_digest() == want
    buf = C.create_string_buffer(80)
    assert _lib.lib().srx_build_info(buf, 80) == 0 and buf.value.decode() == want
    # a binary built from other sources is told apart whatever its mtime
    blob = open(_lib.LIB_PATH, 'rb').read().replace(want.encode(), b'0' * 64)
    other = tmp_path / 'libsrx_other.so'
    other.write_bytes(blob)
    assert _lib.built_digest(str(other)) == '0' * 64 != want


def test_plans_follow_the_reserved_compute_units_without_a_gpu():
    """``srx_set_reserved_cus``: the residual tower's row tile cuts 16 x 24 x 24 pixels into 256 workgroups of 36 pixels on a
    free chip and into 192 of 48 once CUs are held by a collective's channel kernels; the generic planner sizes its rounds
    for the same count.  Plans are host code: no GPU needed (without one the library assumes 256 CUs)."""
    import ctypes as C
    from torchsr_amd import _lib
    if torch.cuda.is_available():
        pytest.skip('plan arithmetic for a 256-CU part; on a GPU box the count is the device\'s')
    lib = _lib.lib()
    d = _lib.Conv2dDesc(16, 24, 24, 64, 64, 64, 64, 3, 3, 1, 1, 0, 0, 0.0, 0, 0)
    out = (C.c_int * 6)()
    try:
        assert lib.srx_plan_cus() == 256
        assert lib.srx_conv2d_plan(C.byref(d), 0, out) == 0 and (out[0], out[3]) == (36, 256)
        assert lib.srx_conv2d_stat_rows(C.byref(d)) == 256
        assert lib.srx_set_reserved_cus(16) == 0 and lib.srx_plan_cus() == 240
        assert lib.srx_conv2d_plan(C.byref(d), 0, out) == 0 and (out[0], out[3]) == (48, 192)
        assert lib.srx_conv2d_stat_rows(C.byref(d)) == 192
        # a VGG layer (M = 18432 pixels, 256 channels): whole rounds of 240 CUs, the rest K-split
        v = _lib.Conv2dDesc(32, 24, 24, 256, 256, 256, 256, 3, 3, 1, 1, 0, 1, 0.0, 0, 0)
        assert lib.srx_conv2d_plan(C.byref(v), 0, out) == 0
        full_rounds = (out[3] // 240) * 240
        assert out[3] >= full_rounds and out[3] != 256
        assert lib.srx_set_reserved_cus(500) != 0
    finally:
        lib.srx_set_reserved_cus(0)
    assert lib.srx_plan_cus() == 256


def test_vgg_loss_loads_a_torchvision_shaped_state_dict(tmp_path):
    """The pretrained branch of ``VGGLoss.__init__`` (torchsr/srgan/loss.py:30: ``vgg19(pretrained=True)``): the file
    torchvision downloads is a full VGG19 state dict -- ``features.N.{weight,bias}`` for the 16 convs plus the three
    ``classifier`` layers -- of which ``features[:36]`` is kept.  The real values are not available offline, so the file is
    written here with the closed-form fill (and token-sized classifier tensors: they are dropped unread)."""
    from torchsr_amd.srgan.loss import VGGLoss, make_vgg19_features
    own = make_vgg19_features(36).state_dict()
    full = {f'features.{k}': v for k, v in closed_form_state(own, prefix='features.').items()}
    for i in (0, 3, 6):
        full[f'classifier.{i}.weight'], full[f'classifier.{i}.bias'] = torch.ones(4, 4), torch.ones(4)
    path = tmp_path / 'vgg19-dcbb9e9d.pth'
    torch.save(full, path)
    v = VGGLoss(weights=str(path))
    assert v.pretrained and not v.features.training and not any(p.requires_grad for p in v.parameters())
    got = v.features.state_dict()
    assert list(got) == list(own)
    for k, t in got.items():
        assert torch.equal(t, full['features.' + k]), k
    # found through the environment variable too; a file without the feature tensors is an error, not a silent random init
    import os
    os.environ['TORCHSR_VGG19_WEIGHTS'] = str(path)
    try:
        assert VGGLoss().pretrained
    finally:
        del os.environ['TORCHSR_VGG19_WEIGHTS']
    torch.save({k: v for k, v in full.items() if not k.startswith('features.34')}, tmp_path / 'short.pth')
    with pytest.raises(RuntimeError, match='Missing key'):
        VGGLoss(weights=str(tmp_path / 'short.pth'))


@pytest.mark.parametrize('model', ['srgan', 'esrgan'])
def test_loaders_read_what_the_reference_trainer_writes(tmp_path, model):
    """tests/golden/checkpoint.npz: the keys and per-entry digests of ``_model_state`` of the reference's own trainers
    (srgan/trainer.py:233-258), plain and with the ``module.`` prefix a wrapped generator gives.  A file rebuilt from
    them must load through the trainer's ``_load_checkpoint`` and through ``test.load_generator_state`` into this
    package's generator, entry for entry."""
    import importlib
    from torchsr_amd.srgan.trainer import SRGANTrainer
    from torchsr_amd.test import load_generator_state
    gold = np.load(os.path.join(GOLDEN, 'checkpoint.npz'))
    assert list(gold[f'{model}_top_keys']) == ['epoch', 'phase', 'state']
    gen = importlib.import_module(f'torchsr_amd.{model}.generator').Generator()
    keys = [str(k) for k in gold[f'{model}_state_keys']]
    assert keys == list(gen.state_dict().keys())  # the checkpoint ABI: same names, same order
    values = step_state(gen.state_dict(), f'{model}.G')
    for k, dg in zip(keys, gold[f'{model}_state_digest']):
        assert np.allclose(tensor_digest(values[k].float()), dg, rtol=1e-12, atol=1e-12), k  # what the reference held
    prefixes = ['', 'module.'] if model == 'srgan' else ['']
    if model == 'srgan':
        assert [str(k) for k in gold['srgan_wrapped_state_keys']] == ['module.' + k for k in keys]
    for prefix in prefixes:
        path = str(tmp_path / f'{model}-gan-best{len(prefix)}.pth')
        torch.save({'epoch': 3, 'phase': f'{model}-gan', 'state': {prefix + k: values[k] for k in keys}}, path)
        ck = SRGANTrainer._load_checkpoint(None, path)
        assert ck['epoch'] == 3 and ck['phase'] == f'{model}-gan' and list(ck['state']) == keys
        for state in (ck['state'], load_generator_state(path)):
            fresh = importlib.import_module(f'torchsr_amd.{model}.generator').Generator()
            fresh.load_state_dict(state, strict=True)
            for k, v in fresh.state_dict().items():
                assert torch.equal(v, values[k]), (prefix, k)
    # a bare state dict (no wrapper) is accepted as well
    bare = str(tmp_path / 'bare.pth')
    torch.save({k: values[k] for k in keys}, bare)
    assert list(load_generator_state(bare)) == keys and list(SRGANTrainer._load_checkpoint(None, bare)['state']) == keys


def test_device_loader_shards_have_equal_length_on_every_rank():
    """Uneven shards would leave one rank in a collective alone: every rank must see the same number of
    train batches and a non-empty test shard, like the reference's DistributedSampler (torchsr/dataset.py:279,343-360)."""
    from torchsr_amd.dataset import DeviceLoader
    images = [torch.zeros(8, 8, 3, dtype=torch.uint8) for _ in range(127)]
    for world, batch, n in ((8, 16, 127), (8, 4, 33), (3, 2, 7), (2, 5, 11), (8, 16, 1)):
        for test in (False, True):
            loaders = [DeviceLoader(images[:n], 'cpu', batch, 8, 4, test, 0, 1, rank, world) for rank in range(world)]
            lens = [len(ld) for ld in loaders]
            assert len(set(lens)) == 1, (world, batch, n, test, lens)
            shards = [ld._shard(list(ld.order)) for ld in loaders]
            assert len({len(s) for s in shards}) == 1 and all(len(s) >= 1 for s in shards)
            assert set(i for s in shards for i in s) == set(range(n))  # every sample is somewhere
            if test:
                assert lens[0] >= 1
            # what __iter__ slices must exist on every rank
            assert all(lens[0] * batch - len(s) < batch for s in shards) if test else all(lens[0] * batch <= len(s) for s in shards)


def test_bf16_native_conv_chunks_stay_inside_32_bit_offsets():
    """srx_conv3x3_c64_bf16_fwd addresses a chunk's rows by 32-bit byte offsets from the chunk's first row: the planner must
    cut chunks so that rows per chunk (+ the rows in flight around it) x W x 128 bytes stays below 4 GiB, whatever H is
    (round-4 advice: rows_per_chunk could grow to H and the offsets wrapped silently).  Host only: nothing is launched."""
    import ctypes as C
    from torchsr_amd import _lib
    lib = _lib.lib()
    out = (C.c_int * 3)()
    for n, h, w in ((1, 1080, 1920), (1, 4320, 7680), (1, 400000, 5000), (1, 40000, 50000), (2, 9000, 200000), (1, 64, 24)):
        if n * h * w >= 2 ** 31:
            continue
        assert lib.srx_conv3x3_c64_bf16_plan(n, h, w, 64, out) == 0, (n, h, w)
        rpc, chunks, strips = out[0], out[1], out[2]
        rw = 4 if w <= 32 else (2 if w <= 64 else 1)
        assert rpc >= rw and rpc % rw == 0 and rpc * chunks >= h and strips >= 1
        assert (rpc + 2 + 3 * rw + 1) * w * 128 < 2 ** 32, (n, h, w, rpc)
    assert lib.srx_conv3x3_c64_bf16_plan(1, 16, 300000, 64, out) != 0  # one row of the window alone is past the range


def test_comm_configuration_is_decided_before_the_process_group(monkeypatch):
    """torchsr/torchsr.py:257-258 + srgan/trainer.py:142-157 (DistributedDataParallel): at world size > 1 the RCCL channel count
    is bounded and the launch plans are told how many CUs the channel kernels get while a large bucket is on the wire -- by
    default, not through a hand-set switch -- and a user's own NCCL_* values win."""
    from torchsr_amd import ddp
    for k in ('NCCL_MIN_NCHANNELS', 'NCCL_MAX_NCHANNELS', 'SRX_NCCL_CHANNELS', 'SRX_COMM_RESERVED_CUS'):
        monkeypatch.delenv(k, raising=False)
    one = ddp.configure_comm(1, 'nccl')
    assert one['reserved_cus_in_comm_window'] == 0 and 'NCCL_MAX_NCHANNELS' not in os.environ
    gloo = ddp.configure_comm(2, 'gloo')
    assert gloo['reserved_cus_in_comm_window'] == 0 and 'NCCL_MAX_NCHANNELS' not in os.environ
    eight = ddp.configure_comm(8, 'nccl')
    assert os.environ['NCCL_MAX_NCHANNELS'] == os.environ['NCCL_MIN_NCHANNELS'] == str(ddp.DEFAULT_CHANNELS)
    assert eight['reserved_cus_in_comm_window'] == ddp.DEFAULT_CHANNELS and eight['nccl_max_nchannels'] == str(ddp.DEFAULT_CHANNELS)
    monkeypatch.setenv('NCCL_MAX_NCHANNELS', '4')
    monkeypatch.setenv('NCCL_MIN_NCHANNELS', '2')
    mine = ddp.configure_comm(8, 'nccl')
    assert mine['nccl_max_nchannels'] == '4' and mine['nccl_min_nchannels'] == '2' and mine['reserved_cus_in_comm_window'] == 4
    monkeypatch.setenv('SRX_COMM_RESERVED_CUS', '12')
    assert ddp.configure_comm(8, 'nccl')['reserved_cus_in_comm_window'] == 12


def test_bench_fractions_are_shares_of_a_peak():
    """bench.py's ``frac`` fields are executed MFMA FLOPs over a hardware peak: a Winograd F(2x2, 3x3) kernel books 16/36 of
    the direct convolution's multiplications, its direct-form rate travels as ``algorithmic_tflops``, and no line with a
    fraction above 1 is printed."""
    import bench
    r = bench.rates('wino_kernel<64>', 380.5e9, 1.881, bench.PEAK_TFLOPS)  # round 5's dominant kernel, per replay
    assert abs(r['algorithmic_tflops'] - 202.3) < 0.1 and abs(r['tflops'] - 89.9) < 0.1 and abs(r['frac'] - 0.5716) < 1e-3
    assert r['algorithmic_speedup'] == 2.25
    d = bench.rates('gconv_kernel<128, 64, 32, 32, 1, 16, 0>', 41.448e9, 0.4631, bench.PEAK_TFLOPS)
    assert d['tflops'] == d['algorithmic_tflops'] and 'algorithmic_speedup' not in d
    leg = bench.leg_rates(9199.0, 62.43e-3, bench.PEAK_TFLOPS, {'gflop_not_executed': 9199.0 * 0.9 * 20 / 36})
    assert leg['frac'] < 1.0 and leg['algorithmic_tflops'] > leg['tflops']
    bench.assert_fracs({'roofline': {'frac': 0.57, 'step_frac_of_fp32_mfma_peak': 0.41, 'by_shape': [{'frac': 0.6}]}})
    for bad in ({'roofline': {'frac': 1.1218}}, {'x': [{'dominant_kernel': {'frac': 1.03}}]}, {'step_frac_of_fp32_mfma_peak': 1.2}):
        with pytest.raises(AssertionError):
            bench.assert_fracs(bad)


def test_bench_dump_outputs_are_float32_fixed_and_within_64_mb(tmp_path):
    """``bench.py --dump-outputs DIR``: the losses of the last step and the networks' states as float32 .npy files, at most 64 MB
    in all (the 23.6 M-element discriminator as a fixed sample), the same positions on every call."""
    import bench
    from torchsr_amd.srgan.discriminator import Discriminator
    from torchsr_amd.srgan.generator import Generator
    torch.manual_seed(0)
    states = {'generator': Generator().state_dict(), 'discriminator': Discriminator().state_dict()}
    losses = {'gan/disc-loss': torch.tensor(1.25), 'gan/train-loss': torch.tensor(0.5)}
    shapes = bench.dump_outputs(str(tmp_path / 'a'), losses, states)
    bench.dump_outputs(str(tmp_path / 'b'), losses, states)
    assert shapes == {'gan_disc_loss': [], 'gan_train_loss': [], 'generator_state': [1551574],
                      'discriminator_state': [bench.DUMP_SAMPLE]}
    total = 0
    for name in shapes:
        a, b = np.load(tmp_path / 'a' / f'{name}.npy'), np.load(tmp_path / 'b' / f'{name}.npy')
        assert a.dtype == np.float32 and np.array_equal(a, b), name
        total += os.path.getsize(tmp_path / 'a' / f'{name}.npy')
    assert total <= 64 << 20
    assert float(np.load(tmp_path / 'a' / 'gan_train_loss.npy')) == 0.5
    assert np.array_equal(np.load(tmp_path / 'a' / 'generator_state.npy'), bench.flat_state(states['generator']).numpy())
    flat_d = bench.flat_state(states['discriminator']).numpy()
    assert np.isin(np.load(tmp_path / 'a' / 'discriminator_state.npy')[:1000], flat_d).all()


def test_forced_plans_change_the_reported_plan_and_reset_restores_the_model_without_a_gpu():
    """``srx_conv2d_force_plan`` / ``srx_conv2d_force_s2`` / ``srx_wgrad_force`` (plan arithmetic only, host code): each changes
    what ``srx_conv2d_plan`` and the workspace queries report as specified, a forced form a layer has no kernel for is refused
    with a message, and zeros hand the choice back to the cost model exactly.  The default plans of the discriminators'
    strided layers are pinned, so that a cost-model change shows up as a deliberate edit here."""
    import ctypes as C
    from torchsr_amd import _lib
    lib = _lib.lib()
    if lib.srx_plan_cus() != 256:
        pytest.skip('the pinned plans are those of a 256-CU part')
    out = (C.c_int * 6)()

    def desc(n, h, w, cin, cout, stride=2, prec=0, k=3):
        return _lib.Conv2dDesc(n, h, w, cin, (cin + 3) // 4 * 4, cout, (cout + 3) // 4 * 4, k, k, stride, k // 2, 0, 0, 0.0, 0, prec)

    def plan(d, which=1):
        rc = lib.srx_conv2d_plan(C.byref(d), which, out)
        return list(out) if rc == 0 else (rc, _lib.last_error())

    d96, d128, d12 = desc(16, 96, 96, 64, 64), desc(16, 128, 128, 64, 64), desc(16, 12, 12, 512, 512)
    d96b, d128b = desc(16, 96, 96, 64, 64, prec=1), desc(16, 128, 128, 64, 64, prec=1)
    small, s1 = desc(3, 26, 30, 64, 64), desc(2, 24, 24, 128, 128, stride=1)
    pinned = {  # {BM, BN, split, workgroups, KS, multi (1 gconv_multi_kernel, 2 gconv_s2f_kernel)}
        'd96': [144, 64, 1, 256, 1, 2], 'd128': [128, 64, 1, 512, 1, 2], 'd12': [64, 64, 1, 288, 2, 1],
        'd96b': [128, 64, 1, 1152, 1, 1], 'd128b': [128, 64, 1, 512, 1, 2], 'small': [64, 64, 1, 40, 1, 1],
        's1': [64, 64, 6, 216, 2, 0]}
    layers = {'d96': d96, 'd128': d128, 'd12': d12, 'd96b': d96b, 'd128b': d128b, 'small': small, 's1': s1}

    def defaults():
        return {k: plan(d, 0 if k == 's1' else 1) for k, d in layers.items()}

    wl = desc(2, 12, 20, 64, 64, stride=1)   # 480 rows: at most 4 row splits of >= 128 rows
    ws_default = lib.srx_conv2d_bwd_weight_multi_ws_floats(C.byref(wl), 1)
    try:
        assert defaults() == pinned
        # the fused kernel on a forced tile (also one the model never picks), and back on gconv_multi_kernel at the model's tile
        assert lib.srx_conv2d_force_s2(2, 128, 128) == 0 and plan(desc(2, 22, 18, 128, 128)) == [128, 128, 1, 2, 1, 2]
        assert lib.srx_conv2d_force_s2(2, 64, 64) == 0
        assert plan(small) == [64, 64, 1, 10, 1, 2] and plan(d96) == [64, 64, 1, 576, 1, 2]
        assert lib.srx_conv2d_force_s2(2, 0, 0) == 0 and plan(d96b) == [128, 64, 1, 288, 1, 2]   # (the model's fused tile)
        assert lib.srx_conv2d_force_s2(1, 0, 0) == 0
        assert plan(d96) == [144, 64, 1, 1024, 1, 1] and plan(d12) == pinned['d12']
        # ... and on a forced tile: KS = 2 where asked, the 144-row tile fp32 only, tiles gconv_multi_kernel lacks refused
        assert lib.srx_conv2d_force_plan(64, 64, 1, 2) == 0 and plan(d96) == [64, 64, 1, 2304, 2, 1]
        assert lib.srx_conv2d_force_plan(144, 64, 1, 1) == 0 and plan(small) == [144, 64, 1, 20, 1, 1]
        rc, msg = plan(desc(3, 26, 30, 64, 64, prec=1))
        assert rc == 2 and 'no 144-row tile' in msg
        assert lib.srx_conv2d_force_plan(64, 32, 1, 1) == 0
        rc, msg = plan(small)
        assert rc == 2 and 'gconv_multi_kernel' in msg and 'no instantiation' in msg
        # the forward and stride-1 data gradient: the forced tile with its K split, KS implied by 64 x 32
        assert plan(s1, 0) == [64, 32, 1, 72, 2, 0] and plan(s1, 1)[:5] == [64, 32, 1, 72, 2]
        assert lib.srx_conv2d_force_plan(144, 128, 3, 1) == 0 and plan(s1, 0) == [144, 128, 3, 24, 1, 0]
        assert lib.srx_conv2d_fwd_ws_floats(C.byref(s1)) == 8 * 3 * 144 * 128   # (every tile K-split: one partial per split)
        rc, msg = plan(desc(2, 24, 24, 128, 128, stride=1, prec=1), 0)
        assert rc == 2 and 'no 144-row tile' in msg
        rc, msg = plan(desc(2, 24, 24, 64, 64, stride=1, k=5), 1)   # (64 padded columns)
        assert rc == 2 and 'do not divide' in msg
        assert lib.srx_conv2d_fwd_ws_floats(C.byref(desc(2, 24, 24, 64, 64, stride=1, k=5))) == 0
        # the fused kernel where it cannot run: odd extent, Cin = 32, Cout = 48, a tile without a bf16 instantiation
        assert lib.srx_conv2d_force_plan(0, 0, 0, 0) == 0 and lib.srx_conv2d_force_s2(2, 64, 64) == 0
        for bad in (desc(2, 13, 18, 64, 64), desc(2, 14, 18, 32, 64), desc(2, 14, 18, 64, 48)):
            rc, msg = plan(bad)
            assert rc == 2 and 'gconv_s2f_kernel refused' in msg
        assert lib.srx_conv2d_force_s2(2, 144, 64) == 0
        rc, msg = plan(d96b)
        assert rc == 2 and 'no instantiation' in msg
        # the weight gradient's row splits (its workspace holds one slab per split)
        assert lib.srx_wgrad_force(-1, 2) == 0
        assert lib.srx_conv2d_bwd_weight_multi_ws_floats(C.byref(wl), 1) == 64 * 577 * 2
        assert lib.srx_wgrad_force(0, 5) == 0
        assert lib.srx_conv2d_bwd_weight_multi_ws_floats(C.byref(wl), 1) == 0 and 'row splits refused' in _lib.last_error()
        # arguments out of range are refused by the setters themselves
        for fn, args in (('srx_conv2d_force_plan', (144, 64, 0, 1)), ('srx_conv2d_force_plan', (96, 64, 1, 1)),
                         ('srx_conv2d_force_plan', (64, 64, 1, 3)), ('srx_conv2d_force_s2', (3, 0, 0)),
                         ('srx_conv2d_force_s2', (2, 144, 32)), ('srx_conv2d_force_s2', (1, 64, 64)),
                         ('srx_wgrad_force', (2, 0)), ('srx_wgrad_force', (-1, 65))):
            with pytest.raises(RuntimeError, match=fn[4:]):
                _lib.call(fn, *args)
    finally:
        lib.srx_conv2d_force_plan(0, 0, 0, 0)
        lib.srx_conv2d_force_s2(0, 0, 0)
        lib.srx_wgrad_force(-1, 0)
    assert defaults() == pinned
    assert lib.srx_conv2d_bwd_weight_multi_ws_floats(C.byref(wl), 1) == ws_default


def test_step_ops_integer_cases_stay_exact():
    """The exact checks of test_step_ops_gpu.py rest on one precondition: for every output of every integer case of
    step_layers.STEP_OPS the sum of the ABSOLUTE values of its terms -- counted in the smallest unit present, quarters where the
    slope 0.25 multiplies -- stays below 2^24.  Then every partial sum, in whatever order a kernel takes it, is a whole number
    of units below 2^24 and so an fp32 number: nothing rounds, and the kernel's result must equal the int64 truth.  (A bound on
    the signed sum would not do: a partial sum may exceed the total.)  Every case is built here and counted in int64."""
    from step_layers import STEP_OPS, int_abs_sums, int_inputs
    ids = [c['id'] for c in STEP_OPS]
    assert len(ids) == len(set(ids))
    built = 0
    for case in STEP_OPS:
        d = int_inputs(case)
        if d is None:
            continue
        built += 1
        for arr in d.values():
            assert arr.dtype.kind == 'i' and np.abs(arr).max() > 0, case['id']
        for what, s in int_abs_sums(case, d).items():
            assert 0 < s < 2 ** 24, (case['id'], what, s)
        # non-zeros everywhere a kernel could lose them: per row block for the row reductions, per 1024 elements and in the last
        # element (the n & 3 tail) for the flat ones
        if case['op'] == 'bn':  # 32 rows: the smallest row block
            for name in ('y', 'dout'):
                rows = np.abs(d[name].astype(np.int64)).sum(1)
                assert np.add.reduceat(rows, np.arange(0, case['M'], 32)).min() > 0 and rows[-1] > 0, (case['id'], name)
        elif case['op'] == 'colsum':  # 16 rows: the smallest partial block
            rows = np.abs(d['x'].astype(np.int64)[:, :case['C']]).sum(1)
            assert np.add.reduceat(rows, np.arange(0, case['M'], 16)).min() > 0 and rows[-1] > 0, case['id']
        elif case['op'] == 'bn_finish':
            assert np.abs(d['table']).sum(1).min() > 0, case['id']  # every table row
        else:
            for name, arr in d.items():
                flat = np.abs(arr.reshape(-1).astype(np.int64))
                assert flat[-1] > 0 and np.add.reduceat(flat, np.arange(0, flat.size, 1024)).min() > 0, (case['id'], name)
    assert built >= 60


def test_abi_refuses_bad_batchnorm_groups_and_channels_without_a_gpu():
    """srx_bn_*: `groups` must divide the rows (and the partial-table rows), a row block must not straddle two groups, C is a
    multiple of 4 in [4, 1024] -- refused with a status code before anything is launched (fake pointers, CPU only)."""
    import ctypes as C
    from torchsr_amd import _lib
    if torch.cuda.is_available():
        pytest.skip('fake pointers: argument validation is exercised where a missed check cannot reach a device')
    lib = _lib.lib()
    fake = 0x10000

    def err():
        buf = C.create_string_buffer(256)
        lib.srx_last_error(buf, 256)
        return buf.value.decode()

    def train_fwd(rows, m, c, groups):
        return lib.srx_bn_train_fwd(fake, fake, rows, m, c, groups, 1e-5, 0.1, fake, fake, None, fake, 0, 0.0, None, fake, fake,
                                    None, None, None, None)

    def act_bwd(m, c, groups):
        return lib.srx_bn_act_bwd(fake, fake, fake, fake, fake, fake, fake, fake, m, c, groups, 0, 0.0, None, 1, None, None, None,
                                  fake, 1 << 30, None)

    assert train_fwd(36, 1153, 64, 2) != 0 and 'do not split' in err()          # rows % groups
    assert train_fwd(37, 1152, 64, 2) != 0 and 'partial rows' in err()          # table rows % groups
    assert train_fwd(36, 1152, 64, 0) != 0 and 'groups' in err()
    assert train_fwd(36, 1152, 64, 65) != 0 and 'groups' in err()
    assert act_bwd(1153, 64, 2) != 0 and 'do not split' in err()
    assert act_bwd(1152 + 32, 64, 2) != 0 and 'straddle' in err()               # 592 rows per group: not whole 32-row blocks
    assert act_bwd(65536 + 128, 64, 2) != 0 and 'straddle' in err()             # 128-row blocks, 32832 rows per group
    for c in (0, 2, 6, 1028, 2048, -4):
        assert train_fwd(36, 1152, c, 1) != 0 and 'multiple of 4' in err(), c
        assert act_bwd(1152, c, 1) != 0 and 'multiple of 4' in err(), c
        assert lib.srx_bn_partial_stats(fake, fake, 1152, c, None) != 0 and 'multiple of 4' in err(), c
        assert lib.srx_bn_act_fwd(fake, fake, fake, fake, fake, None, fake, 1152, c, 0, 0.0, None, None) != 0 and 'multiple of 4' in err(), c
        assert lib.srx_bn_act_bwd_reduce(fake, fake, fake, fake, fake, fake, fake, 1152, c, 0, 0.0, None, None, None, None, fake,
                                         1 << 30, None) != 0 and 'multiple of 4' in err(), c
        assert lib.srx_bn_act_bwd_apply(fake, fake, fake, fake, fake, fake, fake, fake, 1152, c, 0, 0.0, None, 1, None) != 0 and 'multiple of 4' in err(), c
        assert lib.srx_bn_act_bwd_finish(fake, fake, fake, fake, fake, fake, fake, 36, 1, fake, fake, 1152, c, 0, 0.0, None, None, None,
                                         None, None) != 0 and 'multiple of 4' in err(), c
    # the row-block regimes the tests' bounds and the group check rest on
    assert [lib.srx_bn_rows_per_block(m) for m in (1, 32767, 32768, 131071, 131072, 1 << 22)] == [32, 32, 128, 128, 512, 512]
    assert lib.srx_bn_stat_rows(32767) == 1024 and lib.srx_bn_stat_rows(32768) == 256 and lib.srx_bn_stat_rows(131072) == 256


# ------------------------------------------------------------------ the ESRGAN step's conv table (test_esrgan_layers_gpu.py)
def test_esrgan_step_conv_table_holds_the_models_geometry():
    """Generator (16 x 32 x 32 crops), Discriminator(128) and the VGG19 features (16 and 32 crops of 128 x 128) walked layer by
    layer through ``ConvState.out_shape``: every distinct conv problem is the shape of a row of ESRGAN_STEP_CONVS, and no row has
    a shape the models do not produce."""
    from step_layers import ESRGAN_STEP_CONVS, esrgan_case_shapes
    from torchsr_amd.esrgan.discriminator import Discriminator
    from torchsr_amd.esrgan.generator import Generator
    from torchsr_amd.esrgan.loss import make_vgg19_features
    from torchsr_amd.layers import Conv2d
    seen = set()

    def through(conv, shape):
        n, h, w, c = shape
        st = conv._st
        assert c == st.cin_s, (shape, st.cin)
        seen.add((n, h, w, st.cin, st.cout, st.k, st.stride, st.pad, st.up))
        return st.out_shape(n, h, w)

    gen = Generator()
    trunk_in = through(gen.conv1, (16, 32, 32, 4))
    for rrdb in gen.blocks:
        for rdb in (rrdb.RDB1, rrdb.RDB2, rrdb.RDB3):
            for k, conv in enumerate((rdb.conv1[0], rdb.conv2[0], rdb.conv3[0], rdb.conv4[0], rdb.conv5)):
                out = through(conv, trunk_in[:3] + (64 + 32 * k,))   # (its first channels of the block's 192-wide buffer)
                assert out[:3] == trunk_in[:3] and out[3] == (64 if k == 4 else 32)
    shape = trunk_in
    for conv in (gen.conv2, gen.upsample1, gen.upsample2, gen.conv3[0], gen.conv4):
        shape = through(conv, shape)
    assert shape == (16, 128, 128, 4)
    for n in (32, 16):   # the pair pass on real + fake, the adversarial pass; source + target, the source's gradient
        shape = (n, 128, 128, 4)
        for m in Discriminator(128).features:
            if isinstance(m, Conv2d):
                shape = through(m, shape)
        assert shape == (n, 4, 4, 512)
        shape = (n, 128, 128, 4)
        for m in make_vgg19_features(36):
            if isinstance(m, Conv2d):
                shape = through(m, shape)
            elif type(m).__name__ == 'MaxPool2x2':
                shape = (shape[0], shape[1] // 2, shape[2] // 2, shape[3])
        assert shape == (n, 8, 8, 512)
    rows = set()
    for case in ESRGAN_STEP_CONVS:
        assert case['precisions'] and set(case['precisions']) <= {'fp32', 'bf16'} and set(case['kernels']) == set(case['precisions']), case['id']
        assert all(case['kernels'][p] for p in case['precisions']), case['id']   # every row names the form it is there to test
        rows |= esrgan_case_shapes(case)
    assert not seen - rows, sorted(seen - rows)
    assert not rows - seen, sorted(rows - seen)
    for precision in ('fp32', 'bf16'):   # ... and each precision's rows hold every shape
        have = set().union(*[esrgan_case_shapes(c) for c in ESRGAN_STEP_CONVS if precision in c['precisions']])
        assert have == seen, (precision, sorted(seen - have))
    assert len({c['id'] for c in ESRGAN_STEP_CONVS}) == len(ESRGAN_STEP_CONVS)


@pytest.mark.parametrize('cfg', [(2, 9, 7, 3, 64, 1, 0, 3), (2, 9, 7, 64, 32, 2, 0, 64), (1, 6, 5, 64, 16, 1, 2, 64), (2, 8, 8, 96, 32, 1, 0, 192)],
                         ids=['cin3', 'stride2', 'up2', 'cin96of192'])
def test_bf16_conv_reference_bound_separates_right_from_wrong(cfg):
    """``step_layers.conv_refs`` before it judges a kernel: a plain fp32 torch convolution of the bf16-rounded operands lies
    inside the elementwise bound gamma_K (|r(a)| conv |r(b)|) around the float64 value and inside the statistical budget
    (F = 1.5 of its own distance), for the forward, the data gradient and the weight gradient -- and a result with one tap or
    one input channel dropped lies outside the bound."""
    from step_layers import bf16_round, conv_refs
    n, h, w, cin, cout, stride, up, width = cfg
    g = torch.Generator().manual_seed(cin * 7 + stride + up)
    buf = torch.nn.functional.leaky_relu(torch.randn((n, width, h, w), generator=g), 0.2)
    x = buf[:, :cin]                                    # (96 of 192: a dense block's conv reads the head of a wider buffer)
    wt = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (cin * 9)) ** 0.5
    b = torch.randn((cout,), generator=g) * 0.1
    y64, y32, by = conv_refs('y', x, wt, x.shape, wt.shape, stride, 1, up, b, rounded=True)
    dy = torch.randn(y64.shape, generator=g)
    w_cut = wt.clone()
    w_cut[:, :, 1, 2] = 0.0                             # one tap dropped
    x_cut = x.clone()
    x_cut[:, cin // 2] = 0.0                            # one input channel dropped
    wrong = {'y': conv_refs('y', x, w_cut, x.shape, wt.shape, stride, 1, up, b, rounded=True)[1],
             'dx': conv_refs('dx', dy, w_cut, x.shape, wt.shape, stride, 1, up, None, rounded=True)[1],
             'dW': conv_refs('dW', x_cut, dy, x.shape, wt.shape, stride, 1, up, None, rounded=True)[1]}
    also_wrong = conv_refs('y', x_cut, wt, x.shape, wt.shape, stride, 1, up, b, rounded=True)[1]
    for what, a, bb, bias in (('y', x, wt, b), ('dx', dy, wt, None), ('dW', x, dy, None)):
        r64, r32, bound = conv_refs(what, a, bb, x.shape, wt.shape, stride, 1, up, bias, rounded=True)
        assert r64.dtype == torch.float64 and r32.dtype == torch.float32 and r64.shape == r32.shape == bound.shape
        expect = {'y': y64.shape, 'dx': x.shape, 'dW': wt.shape}[what]
        assert tuple(r64.shape) == tuple(expect), what
        # the float64 value is the convolution of the ROUNDED operands, not of the operands
        plain = conv_refs(what, a, bb, x.shape, wt.shape, stride, 1, up, bias, rounded=False)[0]
        assert torch.equal(r64, conv_refs(what, bf16_round(a), bf16_round(bb), x.shape, wt.shape, stride, 1, up, bias)[0])
        assert ((plain - r64).abs() > bound).any(), what
        err = (r32.double() - r64).abs()
        assert (err <= bound).all(), (what, (err / bound.clamp_min(1e-300)).max().item())
        dist = ((r32.double() - r64).norm() / r64.norm()).item()
        assert dist <= 1.5 * dist + 1e-7 and dist < 1e-6, (what, dist)
        bad = (wrong[what].double() - r64).abs()
        assert (bad > bound).any(), what
        assert (bad > bound).double().mean().item() > 0.01, what   # (not one element: the whole tap / channel is missing)
    assert ((also_wrong.double() - y64).abs() > by).any()
