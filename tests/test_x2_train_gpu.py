"""Training at x2 on the MI355X: the weight gradient of RRDBNet's x2 input layer through the C ABI
(``srx_unshuffle2_conv_bwd_weight``), its autograd node, the two generators against their fp64 restatements, and the trainers.

Bounds.  The kernel multiplies and adds in fp32 and nothing else: on small integers every partial sum is an integer below 2^24,
so the result is the fp64 one bit for bit in any order of summation.  On random data the bound is ``TOL_WGRAD`` of
test_thin_forms_gpu.py (2e-4 as a relative L2 distance; the same scheme and arithmetic as ``thin_wgrad_kernel``).  The generators
follow test_compact_gpu.py::test_generator_vs_fp64_restatement: at most 4x the fp32 CPU restatement's own distance from fp64.
The 16-bit compact chain follows test_generator_16bit_chain_vs_rounded_restatement: five stored layers, 10 u of the range.
Everything about trainers is equality of bits."""
import functools
import os
import socket
import warnings
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as TF

import compact_ref
import rrdbnet_ref
import unet_ref
import x2_ref
from guarded import SENTINEL, Guarded
from test_thin_forms_gpu import TOL_WGRAD

pytestmark = pytest.mark.gpu


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------ 1. the kernel through the C ABI
def _buffers(dev, shape, kind, prefill=None):
    n, h, w = shape
    x, dy, want = x2_ref.operands(shape, kind)
    x4, dy4 = x2_ref.nhwc(x, 4), x2_ref.nhwc(dy, 64)
    gx, gdy = Guarded(dev, tuple(x4.shape), src=x4), Guarded(dev, tuple(dy4.shape), src=dy4)
    gdw = Guarded(dev, (64, 12, 3, 3), src=prefill, margin=SENTINEL)
    nws = x2_ref.ws_floats(shape)
    gws = Guarded(dev, (nws,), margin=SENTINEL, margin_floats=256)
    return (x4, dy4, want), (gx, gdy, gdw, gws), nws


def _run(shape, bufs, nws, accumulate):
    from torchsr_amd import _lib
    gx, gdy, gdw, gws = bufs
    _lib.call('srx_unshuffle2_conv_bwd_weight', *shape, gx.ptr(), gdy.ptr(), gdw.ptr(), accumulate, gws.ptr(), nws, _stream())
    torch.cuda.synchronize()


def _untouched(bufs, x4, dy4, what):
    gx, gdy, gdw, gws = bufs
    assert gdw.margins_unchanged() and gws.margins_unchanged(), what
    assert gx.margins_unchanged() and gdy.margins_unchanged(), what
    assert torch.equal(gx.t.cpu(), x4) and torch.equal(gdy.t.cpu(), dy4), what


@pytest.mark.parametrize('shape', x2_ref.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_weight_gradient_is_exact_on_integers(dev, shape):
    p = x2_ref.plan(shape)
    if shape in x2_ref.STEP_SHAPES:
        assert p['slabs'] > 1 and p['segs_per_range'] > 1, p
    if shape == x2_ref.RAGGED_SHAPE:
        assert p['ranges'] % 4 != 0 or p['segments'] % p['segs_per_range'] != 0, p
    (x4, dy4, want), bufs, nws = _buffers(dev, shape, 'int')
    assert float(want.abs().max()) < 2 ** 24
    _run(shape, bufs, nws, 0)
    got = bufs[2].t.cpu()
    assert torch.equal(got.double(), want), (shape, p, int((got.double() != want).sum()))
    _untouched(bufs, x4, dy4, shape)
    # accumulate onto an integer prefill: still exact
    g = torch.Generator().manual_seed(5)
    prefill = torch.randint(-50, 51, (64, 12, 3, 3), generator=g).float()
    (x4, dy4, want), bufs, nws = _buffers(dev, shape, 'int', prefill)
    _run(shape, bufs, nws, 1)
    assert torch.equal(bufs[2].t.cpu().double(), want + prefill.double()), shape
    _untouched(bufs, x4, dy4, shape)


@pytest.mark.parametrize('shape', x2_ref.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_weight_gradient_is_bounded_on_random_data(dev, shape):
    (x4, dy4, want), bufs, nws = _buffers(dev, shape, 'rand')
    _run(shape, bufs, nws, 0)
    e = x2_ref.rel_l2(bufs[2].t, want)
    print(f'X2 wgrad {shape}: relative L2 distance from fp64 {e:.3e} of {TOL_WGRAD:g} ({x2_ref.plan(shape)})')
    assert e <= TOL_WGRAD, (shape, e)
    _untouched(bufs, x4, dy4, shape)


def test_refusals_launch_nothing(dev):
    from torchsr_amd import _lib
    L = _lib.lib()
    shape = (2, 8, 32)
    (x4, dy4, _), bufs, nws = _buffers(dev, shape, 'int', torch.full((64, 12, 3, 3), 7.0))
    gx, gdy, gdw, gws = bufs
    gws.t.fill_(3.0)
    x, dy, dw, ws = (b.t.data_ptr() for b in bufs)
    s = _stream()
    cases = [((2, 8, 32), (None, dy, dw, ws), nws), ((2, 8, 32), (x, None, dw, ws), nws), ((2, 8, 32), (x, dy, None, ws), nws),
             ((2, 8, 32), (x, dy, dw, None), nws), ((0, 8, 32), (x, dy, dw, ws), nws), ((2, -8, 32), (x, dy, dw, ws), nws),
             ((2, 8, 0), (x, dy, dw, ws), nws), ((2, 1, 32), (x, dy, dw, ws), nws), ((2, 8, 1), (x, dy, dw, ws), nws),
             ((1, 4096, 4096), (x, dy, dw, ws), 1 << 30), ((2, 8, 32), (x, dy, dw, ws), nws - 1), ((2, 8, 32), (x, dy, dw, ws), 0)]
    for shp, (a, b, c, d), n in cases:
        for acc in (0, 1):
            rc = L.srx_unshuffle2_conv_bwd_weight(*shp, a, b, c, acc, d, n, s)
            assert rc != 0 and _lib.last_error(), (shp, n, rc)
    torch.cuda.synchronize()
    assert bool((gdw.t == 7).all()) and bool((gws.t == 3).all())
    _untouched(bufs, x4, dy4, 'refusals')


# ------------------------------------------------------------------ 2. the autograd node
def _layer_case(shape, seed=3):
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, h, w, generator=g)
    wt = torch.randn(64, 12, 3, 3, generator=g) * (2.0 / (12 * 9)) ** 0.5
    b = (torch.rand(64, generator=g) - 0.5) * 0.2
    r = torch.randn(n, 64, *x2_ref.out_hw(h, w), generator=g)
    ref = {}
    for name, dt in (('f64', torch.float64), ('f32', torch.float32)):
        wr, br = wt.to(dt).requires_grad_(), b.to(dt).requires_grad_()
        y = x2_ref.layer(x.to(dt), wr, br)
        (y * r.to(dt)).sum().backward()
        ref[name] = (y.detach(), wr.grad, br.grad)
    return x, wt, b, r, ref


def _module(dev, wt, b):
    from torchsr_amd.layers import Unshuffle2Conv2d
    m = Unshuffle2Conv2d(trainable=True).to(dev).train()
    with torch.no_grad():
        m.weight.copy_(wt)
        m.bias.copy_(b)
    return m


@pytest.mark.parametrize('shape', [(2, 8, 12), (1, 7, 9)], ids=lambda s: 'x'.join(map(str, s)))
def test_trainable_layer_gradients_with_and_without_sinks(dev, shape):
    from torchsr_amd import functional as F
    x, wt, b, r, ref = _layer_case(shape)
    y64, dw64, db64 = ref['f64']
    x4 = F.to_nhwc(x.to(dev), 4)
    r4 = x2_ref.nhwc(r, 64).to(dev)
    old = F.direct_grads[0]
    try:
        for sinks in (False, True):
            F.direct_grads[0] = sinks
            m = _module(dev, wt, b)
            if sinks:  # a gradient sink is .grad itself: the kernels accumulate onto what it holds
                m.weight.grad, m.bias.grad = torch.full_like(m.weight, 2.0), torch.full_like(m.bias, -1.0)
            y = m(x4)
            assert y.requires_grad and tuple(y.shape) == (shape[0], *x2_ref.out_hw(*shape[1:]), 64)
            (y * r4).sum().backward()
            off_w, off_b = (2.0, -1.0) if sinks else (0.0, 0.0)
            for name, got, want, own in (('forward', y.detach().permute(0, 3, 1, 2), y64, ref['f32'][0]),
                                         ('dw', m.weight.grad - off_w, dw64, ref['f32'][1]),
                                         ('db', m.bias.grad - off_b, db64, ref['f32'][2])):
                e, e0 = x2_ref.rel_l2(got, want), x2_ref.rel_l2(own, want)
                print(f'X2 layer {shape} sinks {sinks} {name}: GPU {e:.3e}, fp32 CPU {e0:.3e} from fp64 (relative L2)')
                assert e <= TOL_WGRAD, (name, sinks, e)
            # no_weight_grad and needs_input_grad: nothing is computed for a detached or frozen parameter
            from torchsr_amd.layers import no_weight_grad
            m.zero_grad(set_to_none=True)
            with no_weight_grad():
                assert not m(x4).requires_grad
            m.bias.requires_grad_(False)
            (m(x4) * r4).sum().backward()
            assert m.bias.grad is None and x2_ref.rel_l2(m.weight.grad, dw64) <= TOL_WGRAD
    finally:
        F.direct_grads[0] = old


def test_a_changed_weight_is_repacked_by_the_next_training_forward(dev):
    """The stale-pack check: the weight changes in place -- through a raw view, so that no version counter moves, as the flat
    Adam step changes it -- between two train-mode forwards; the second equals a fresh module's, bit for bit."""
    from torchsr_amd import functional as F
    x, wt, b, _r, _ref = _layer_case((2, 8, 12))
    x4 = F.to_nhwc(x.to(dev), 4)
    m = _module(dev, wt, b)
    first = m(x4).detach().clone()
    m.weight.data.view(-1).detach().mul_(1.5)
    m.bias.data.add_(0.25)
    second = m(x4).detach()
    fresh = _module(dev, wt * 1.5, b + 0.25)(x4).detach()
    assert torch.equal(second, fresh) and not torch.equal(second, first)
    with torch.no_grad():  # and without autograd the cached pack follows the key
        assert torch.equal(m.eval()(x4), _module(dev, wt * 1.5, b + 0.25).eval()(x4))


def test_an_image_with_requires_grad_raises(dev):
    from torchsr_amd import functional as F
    x, wt, b, _r, _ref = _layer_case((1, 7, 9))
    m = _module(dev, wt, b)
    with pytest.raises(RuntimeError, match='no input gradient'):
        m(F.to_nhwc(x.to(dev), 4).requires_grad_())


# ------------------------------------------------------------------ 3. the generators
def _restatements(make, sd, x, r):
    out = {}
    for name, dt in (('f64', torch.float64), ('f32', torch.float32)):
        m = make().to(dt)
        m.load_state_dict({k: v.to(dt) for k, v in sd.items()})
        y = m(x.to(dt))
        (y * r.to(dt)).sum().backward()
        out[name] = (y.detach(), {k: p.grad.clone() for k, p in m.named_parameters()})
    return out


def _hold_all(gen, y, refs, rename, tag):
    y64, g64 = refs['f64']
    y32, g32 = refs['f32']
    worst = {'train forward': (x2_ref.rel_l2(y, y64), x2_ref.rel_l2(y32, y64))}
    for k, p in gen.named_parameters():
        assert p.grad is not None, k
        worst[k] = (x2_ref.rel_l2(p.grad, g64[rename(k)]), x2_ref.rel_l2(g32[rename(k)], g64[rename(k)]))
    for k, (e, e0) in worst.items():
        print(f'X2 {tag} {k}: GPU {e:.3e}, fp32 CPU {e0:.3e} from fp64 (relative L2); ratio {e / e0:.3f}')
    bad = {k: v for k, v in worst.items() if not v[0] <= 4 * v[1]}
    assert not bad, bad


@pytest.mark.parametrize('hw', [(12, 20), (7, 9)], ids=lambda s: 'x'.join(map(str, s)))
def test_esrgan_x2_generator_vs_fp64_restatement(dev, hw):
    from torchsr_amd.esrgan.generator import Generator
    from torchsr_amd.rrdbnet import rrdbnet_to_generator_state
    make = functools.partial(rrdbnet_ref.RRDBNetRef, num_block=1, scale=2)
    sd = rrdbnet_ref.seeded_state(make(), 6)
    g = torch.Generator().manual_seed(8)
    x = torch.rand(2, 3, *hw, generator=g)
    r = torch.randn(2, 3, 2 * hw[0], 2 * hw[1], generator=g)
    refs = _restatements(make, sd, x, r)
    gen = Generator(1, scale_factor=2, trainable=True).to(dev).train()
    own = rrdbnet_to_generator_state(sd)
    gen.load_state_dict(own)
    by_ptr = {v.data_ptr(): k for k, v in sd.items()}  # (the conversion hands the file's tensors on)
    names = {k: by_ptr[v.data_ptr()] for k, v in own.items()}  # this package's key -> the published one
    y = gen(x.to(dev))
    assert tuple(y.shape) == tuple(r.shape)
    (y * r.to(dev)).sum().backward()
    _hold_all(gen, y.detach(), refs, lambda k: names[k], f'esrgan {hw}')


@pytest.fixture(scope='module')
def compact_refs():
    make = functools.partial(compact_ref.CompactRef, scale_factor=2, num_conv=3)
    sd = compact_ref.seeded_state(make(), 4)
    g = torch.Generator().manual_seed(9)
    x = torch.rand(2, 3, 12, 20, generator=g)
    r = torch.randn(2, 3, 24, 40, generator=g)
    return {'sd': sd, 'x': x, 'r': r, **_restatements(make, sd, x, r)}


def _compact(dev, sd):
    from torchsr_amd.compact.generator import Generator
    gen = Generator(scale_factor=2, num_conv=3).to(dev)
    gen.load_state_dict(sd)
    return gen


def test_compact_x2_generator_vs_fp64_restatement(dev, compact_refs):
    from torchsr_amd.test import upscale
    gen = _compact(dev, compact_refs['sd']).train()
    y = gen(compact_refs['x'].to(dev))
    (y * compact_refs['r'].to(dev)).sum().backward()
    _hold_all(gen, y.detach(), compact_refs, lambda k: k, 'compact')
    with torch.no_grad():
        ye = upscale(gen.eval(), compact_refs['x'].to(dev), scale=2, precision='fp32')
    e, e0 = x2_ref.rel_l2(ye, compact_refs['f64'][0]), x2_ref.rel_l2(compact_refs['f32'][0], compact_refs['f64'][0])
    print(f'X2 compact upscale fp32: GPU {e:.3e}, fp32 CPU {e0:.3e} from fp64 (relative L2); ratio {e / e0:.3f}')
    assert tuple(ye.shape) == (2, 3, 24, 40) and e <= 4 * e0


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_compact_x2_upscale_in_16_bits(dev, compact_refs, precision):
    from torchsr_amd.test import upscale
    dt, u = (torch.bfloat16, 2.0 ** -8) if precision == 'bf16' else (torch.float16, 2.0 ** -11)
    gen = _compact(dev, compact_refs['sd']).eval()
    out = upscale(gen, compact_refs['x'].to(dev), scale=2, precision=precision)
    assert tuple(out.shape) == (2, 3, 24, 40) and bool(torch.isfinite(out).all())
    ref = compact_ref.rounded_forward(compact_refs['sd'], compact_refs['x'], 2, lambda v: v.to(dt).double())
    e = ((out.cpu().double() - ref).abs().max() / ref.abs().max()).item()
    print(f'X2 compact {precision} upscale vs the rounded restatement: max error {e:.3e} of the range = {e / u:.2f} u')
    assert e <= 10 * u, e


# ------------------------------------------------------------------ 4. the trainers
def _trainer(dev, model: str, graphs: bool, seed: int = 3, prepare: bool = True, distributed: bool = False, disc: str = 'unet',
             **extra):
    """A one-block ESRGAN / two-conv compact trainer against the U-Net critic at scale 2, as tests/test_ema_gpu.py builds them."""
    from oracle.weights import closed_form_state
    from torchsr_amd.esrgan.generator import Generator
    from torchsr_amd.models import select_trainer_model
    extra.setdefault('scale', 2)
    args = Namespace(disable_amp=False, batch_size=2, epochs=8, gan_checkpoint=None, local_rank=0, pretrain_epochs=1,
                     psnr_checkpoint=None, skip_image_save=True, world_size=1, rank=0 if distributed else -1, use_graphs=graphs,
                     vgg_weights='random', num_conv=2, model=model, discriminator=disc, **extra)
    cls, _crop = select_trainer_model(args)
    if model == 'esrgan':
        cls = type('Small' + cls.__name__, (cls,), {'generator_cls': functools.partial(Generator, num_rrdb_blocks=1)})
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        t = cls(dev, args, [], [], 2, 2, distributed=distributed)
    if prepare:
        if disc == 'unet' and not extra.get('init_discriminator'):
            t.discriminator.load_state_dict(unet_ref.seeded_state(unet_ref.UNetRef(), 11))
        t.vgg_loss.features.load_state_dict(closed_form_state(t.vgg_loss.features.state_dict(), prefix='features.'))
    t.generator.train()
    t.discriminator.train()
    return t


def _batch(dev, seed=31, size=32):
    g = torch.Generator().manual_seed(seed)
    hr = torch.rand(2, 3, size, size, generator=g).to(dev)
    return TF.avg_pool2d(hr, 2), hr


@pytest.mark.parametrize('model', ['esrgan', 'compact'])
def test_three_captured_x2_gan_steps_equal_three_eager_ones(dev, model):
    """Two eager warm-ups, the capture and three replays against six eager steps: losses and weights bit for bit (a replay that
    read a pack of the input layer from before its Adam update would part from the eager run at once)."""
    lr, hr = _batch(dev)
    eager, graph = _trainer(dev, model, False), _trainer(dev, model, True)
    assert eager.scale == 2 and eager.generator.scale_factor == 2
    if model == 'esrgan':
        assert eager.generator.trainable and len(eager.generator.blocks) == 1
    before = graph.gen_flat.data.clone()
    for step in range(6):
        a = {k: v.item() for k, v in eager.gan_step(lr, hr).items()}
        b = {k: v.item() for k, v in graph.gan_step(lr, hr).items()}
        assert a == b and np.all(np.isfinite(list(a.values()))), (step, a, b)
        assert torch.equal(eager.gen_flat.data, graph.gen_flat.data), step
    assert 'gan.all' in graph._graphs and not eager._graphs
    assert torch.equal(eager.disc_flat.data, graph.disc_flat.data)
    first = 'conv1.weight' if model == 'esrgan' else 'body.0.weight'
    moved = dict(graph.generator.named_parameters())[first]
    assert not torch.equal(graph.gen_flat.data, before) and bool(moved.grad.abs().sum() > 0)
    # the pre-training phase too: the eager step after the switch, the capture, a replay
    for step in range(5):
        a, b = eager.pretrain_step(lr, hr).item(), graph.pretrain_step(lr, hr).item()
        assert a == b and np.isfinite(a), (step, a, b)
        assert torch.equal(eager.gen_flat.data, graph.gen_flat.data), step


def test_init_files_and_checkpoints_of_the_other_scale(dev, tmp_path):
    from oracle.weights import closed_form_state
    from torchsr_amd.rrdbnet import rrdbnet_to_generator_state
    files = {}
    for s in (2, 4):
        files[s] = str(tmp_path / f'rrdb-x{s}.pth')
        state = rrdbnet_ref.seeded_state(rrdbnet_ref.RRDBNetRef(num_block=2, scale=s), 20 + s)
        torch.save({'params_ema': state}, files[s])
        if s == 2:
            want = rrdbnet_to_generator_state(state)
    t = _trainer(dev, 'esrgan', True, prepare=False, init_generator=files[2], ema_decay=0.5)
    assert len(t.generator.blocks) == 2 and t.generator.scale_factor == 2 and t.generator.trainable  # the file's depth, x2
    assert t.ema_generator.trainable and t.ema_generator.conv1.trainable
    got = {k: v.cpu() for k, v in t.generator.state_dict().items()}
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in got)
    lr, hr = _batch(dev)
    t.vgg_loss.features.load_state_dict(closed_form_state(t.vgg_loss.features.state_dict(), prefix='features.'))
    losses = {k: v.item() for k, v in t.gan_step(lr, hr).items()}
    assert np.all(np.isfinite(list(losses.values()))), losses
    with pytest.raises(RuntimeError, match='an x4 RRDBNet file in a run started with --scale 2'):
        _trainer(dev, 'esrgan', True, prepare=False, init_generator=files[4])
    with pytest.raises(RuntimeError, match='x2 is inference-only unless the run is started with --scale 2'):
        _trainer(dev, 'esrgan', True, prepare=False, init_generator=files[2], scale=4)
    cfiles = {}
    for s in (2, 4):
        cfiles[s] = str(tmp_path / f'compact-x{s}.pth')
        torch.save({'params_ema': compact_ref.seeded_state(compact_ref.CompactRef(scale_factor=s, num_conv=2), 30 + s)}, cfiles[s])
    c = _trainer(dev, 'compact', True, prepare=False, init_generator=cfiles[2])
    assert c.generator.scale_factor == 2 and tuple(c.generator.body[-1].weight.shape) == (12, 64, 3, 3)
    with pytest.raises(RuntimeError, match='an x4 SRVGGNetCompact file in a run started with --scale 2'):
        _trainer(dev, 'compact', True, prepare=False, init_generator=cfiles[4])
    with pytest.raises(RuntimeError, match='x2 is inference-only unless'):
        _trainer(dev, 'compact', True, prepare=False, init_generator=cfiles[2], scale=4)
    # resuming a checkpoint of the other scale: one clear error, not a size mismatch of load_state_dict
    for trainer, state in ((t, {'conv1.weight': torch.zeros(64, 3, 3, 3)}),
                           (c, compact_ref.CompactRef(scale_factor=4, num_conv=2).state_dict())):
        with pytest.raises(RuntimeError, match='checkpoint other.pth: an x4 generator file in a run started with --scale 2'):
            trainer._load_generator_state(state, 'other.pth')


@pytest.mark.parametrize('model', ['esrgan', 'compact'])
def test_train_scale_2_then_test_writes_an_image_twice_the_size(dev, model, tmp_path, monkeypatch):
    from PIL import Image
    from torchsr_amd.torchsr import main
    monkeypatch.chdir(tmp_path)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'LOCAL_WORLD_SIZE', 'SLURM_NTASKS'):
        monkeypatch.delenv(k, raising=False)
    depth = ['--num-conv', '2'] if model == 'compact' else []
    main(['train', '--model', model, '--scale', '2', '--train-dir', 'synthetic:8', '--batch-size', '2', '--epochs', '1',
          '--pretrain-epochs', '1', '--seed', '7', '--vgg-weights', 'random', '--skip-image-save', '--device-data'] + depth)
    ckpt = torch.load(f'{model}-gan-latest.pth', map_location='cpu')
    assert all(torch.isfinite(v).all() for v in ckpt['state'].values() if v.is_floating_point())
    first, last = ('conv1.weight', 'conv4.weight') if model == 'esrgan' else ('body.0.weight', 'body.6.weight')
    assert tuple(ckpt['state'][first].shape)[:2] == ((64, 12) if model == 'esrgan' else (64, 3))
    assert ckpt['state'][last].shape[0] == (3 if model == 'esrgan' else 12)
    Image.fromarray((np.random.RandomState(1).rand(18, 23, 3) * 255).astype('uint8')).save('lr.png')
    main(['test', 'lr.png', '--model', model])  # the scale is the file's
    out = np.asarray(Image.open('upres-lr.png'))
    assert out.shape == (36, 46, 3) and out.std() > 0


# ------------------------------------------------------------------ 5. data parallel, world size 1
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _ddp_worker(rank, port, out):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1', LOCAL_RANK='0',
                      HSA_ENABLE_IPC_MODE_LEGACY='0')
    import torch.distributed as dist
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    dist.init_process_group('gloo', rank=0, world_size=1)
    try:
        lr, hr = _batch(dev, size=128)  # (the VGG-style critic's crop: the U-Net critic does not run under a process group)
        fused = _trainer(dev, 'esrgan', True, disc='vgg')
        seg = _trainer(dev, 'esrgan', True, distributed=True, disc='vgg', force_collectives=True)
        rep = {'loss_gap': 0.0, 'buckets': (len(seg.gen_sync), len(seg.disc_sync))}
        for _step in range(5):
            lf, ls = fused.gan_step(lr, hr), seg.gan_step(lr, hr)
            for k in lf:
                a, b = lf[k].item(), ls[k].item()
                rep['loss_gap'] = max(rep['loss_gap'], abs(a - b) / max(abs(a), 1e-3))
        gap = 0.0
        for (k, a), (_, b) in zip(fused.generator.state_dict().items(), seg.generator.state_dict().items()):
            gap = max(gap, ((a - b).abs().max() / a.abs().max().clamp_min(1e-6)).item())
        rep['param_gap'] = gap
        rep['issued'] = seg.gen_sync.issued + seg.disc_sync.issued
        # conv1.weight sits in the body bucket, which goes out last
        names = [k for k, _ in seg.generator.named_parameters()]
        rep['conv1_in_body'] = names.index('conv1.weight') < names.index(seg.gen_tail_bucket)
        out[0] = rep
        torch.cuda.synchronize()
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_segmented_x2_step_tracks_the_single_graph_step_at_world_size_one(dev):
    """tests/test_rccl_gpu.py's equality at world size 1, for the x2 ESRGAN step (gloo: the sums are no-ops, the backward is cut
    at 'g.tail' / 'd.head' and every bucket goes through the collective): the same bounds."""
    port = _free_port()
    mgr = mp.get_context('spawn').Manager()
    out = mgr.dict()
    mp.spawn(_ddp_worker, args=(port, out), nprocs=1, join=True)
    rep = out[0]
    assert rep['buckets'] == (2, 2) and rep['issued'] == 4 * 5 and rep['conv1_in_body'], rep
    assert rep['loss_gap'] < 1e-5 and rep['param_gap'] < 1e-4, rep
