"""Published RRDBNet checkpoints on the GPU (restatement: ``tests/rrdbnet_ref.py``):

1. every launch form of unshuffle2_conv_fwd_kernel (csrc/unshuffle.hip) through the C ABI against fp64 on the CPU of the same
   arithmetic, ``conv2d(pixel_unshuffle(pad_reflect(x)), w, b, 1, 1)`` -- for precision 1 with x and w rounded to bf16 first: one
   output pixel that is all padding, one odd axis each, both odd with a tile across the image boundary, a ragged third tile, and a
   shape cut from the launch plan under a reservation at which waves walk a second tile; with and without bias; outputs inside
   NaN-filled allocations whose guards must survive; the launch name and the plan asserted; every refusal.  Bound: 2e-5 of the
   tensor's largest value -- TOL_FWD of test_thin_forms_gpu.py, the project's bound for the first-layer kernel against a reference
   that rounds as the kernel does.  K is 108 here, not 27: the worst ratio met is printed (profiles/rrdbnet_tests_times.txt).
2. ``esrgan.Generator`` loaded through the key map against the restatement: x4 and x2, even and odd sizes, fp32 by the rule of
   test_compact_gpu.py's test_generator_vs_fp64_restatement (relative L2 distance from fp64 at most 4x the fp32 CPU restatement's
   own), bf16 products within 2e-2 of the fp32 result's largest value (the bound test_cli_gpu.py's
   test_1080p_inference_bf16_products_vs_oracle sets for bf16 inference against the exact result), x2 refused in training mode
   and under autograd.
3. tiled == untiled at x2 with an odd bottom edge, by the bound of test_cli_gpu.py's test_tiled_inference_equals_untiled (1e-4).
4. the command line on published-format files: a 2-block x2 and a 6-block x4 ``{'params_ema': ...}``; the same with
   --self-ensemble, --color-fix and --outscale.
5. the x4 generator: same keys, same launches as before, ``scale_factor=4`` given or not.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from guarded import Guarded
from rrdbnet_ref import RRDBNetRef, seeded_state
from step_layers import prof_launches

pytestmark = pytest.mark.gpu

NAN = float('nan')
TOL_FWD = 2e-5      # test_thin_forms_gpu.py
TOL_BF16 = 2e-2     # test_cli_gpu.py::test_1080p_inference_bf16_products_vs_oracle
TOL_TILED = 1e-4    # test_cli_gpu.py::test_tiled_inference_equals_untiled


def _L():
    from torchsr_amd import _lib
    return _lib, _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(autouse=True)
def _overrides_reset(dev):
    """No other test sees a reservation of this module."""
    lib, L = _L()
    try:
        yield
    finally:
        lib.call('srx_set_reserved_cus', 0)
        assert L.srx_plan_cus() == L.srx_device_cus()


def _rel_l2(a, ref):
    a, ref = a.double().cpu(), ref.double().cpu()
    return ((a - ref).square().sum().sqrt() / ref.square().sum().sqrt().clamp_min(1e-300)).item()


# ------------------------------------------------------------------------------------------------ 1. the kernel's forms
@pytest.fixture(scope='module')
def layer():
    """One weight and bias for every shape; the fp64 references are computed once per shape (``_reference``)."""
    g = torch.Generator().manual_seed(5)
    w = (torch.rand(64, 12, 3, 3, generator=g) * 2 - 1) * (1.0 / 108) ** 0.5
    b = torch.rand(64, generator=g) - 0.5
    return w, b, {}


def _reference(layer, shape):
    """x [N,3,H,W] and the two fp64 results without bias, NHWC: exact operands, bf16-rounded operands."""
    w, _, cache = layer
    if shape not in cache:
        n, h, wd = shape
        x = torch.rand(n, 3, h, wd, generator=torch.Generator().manual_seed(h * 1000 + wd)) * 2 - 1
        out = []
        for r in (lambda t: t.double(), lambda t: t.bfloat16().double()):
            xp = TF.pad(r(x), (0, wd & 1, 0, h & 1), mode='reflect')
            out.append(TF.conv2d(TF.pixel_unshuffle(xp, 2), r(w), None, 1, 1).permute(0, 2, 3, 1).contiguous())
        cache[shape] = (x, out[0], out[1])
    return cache[shape]


def _image4(x, dev):
    n, c, h, w = x.shape
    x4 = torch.zeros(n, h, w, 4)
    x4[..., :3] = x.permute(0, 2, 3, 1)
    x4[..., 3] = 7.0  # the stored fourth channel is not an operand: the pack has no weight for it
    return x4.contiguous().to(dev)


def _plan(n, h, w):
    lib, _ = _L()
    out = (C.c_int * 2)()
    lib.call('srx_unshuffle2_conv_plan', n, h, w, out)
    return list(out)


def _packed(w, dev):
    lib, L = _L()
    assert L.srx_unshuffle2_conv_packed_floats() == 108 * 64
    wpk = Guarded(dev, (108, 64))
    wd = w.to(dev)
    lib.call('srx_unshuffle2_conv_pack', wd.data_ptr(), wpk.t.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert wpk.margins_unchanged() and bool(torch.isfinite(wpk.t).all())
    return wpk


def _run_forms(dev, layer, shape, reserved=0):
    lib, L = _L()
    w, b, _ = layer
    n, h, wd = shape
    x, exact, rounded = _reference(layer, shape)
    ho, wo = (h + 1) // 2, (wd + 1) // 2
    m = n * ho * wo
    assert exact.shape == (n, ho, wo, 64)
    lib.call('srx_set_reserved_cus', reserved)
    ntiles, wgs = _plan(n, h, wd)
    assert ntiles == -(-m // 32) and wgs == min(-(-ntiles // 4), 4 * L.srx_plan_cus())
    x4, bg, wpk = _image4(x, dev), b.to(dev), _packed(w, dev)
    worst = 0.0
    for prec in (0, 1):
        for bias in (False, True):
            y = Guarded(dev, (n, ho, wo, 64), margin=NAN)
            run = lambda: lib.call('srx_unshuffle2_conv_fwd', n, h, wd, x4.data_ptr(), wpk.t.data_ptr(),  # noqa: E731
                                   bg.data_ptr() if bias else None, y.t.data_ptr(), prec, _stream())
            assert prof_launches(run) == ['unshuffle2_conv_fwd_kernel<%d> MxNxK=%dx64x108' % (prec, m)]
            assert y.margins_unchanged(), (shape, prec, bias, 'wrote outside its output')
            want = (rounded if prec else exact) + (b.double() if bias else 0.0)
            got = y.t.cpu()
            assert bool(torch.isfinite(got).all()), (shape, prec, bias)
            e = ((got.double() - want).abs().max() / want.abs().max()).item()
            print('RRDBNET unshuffle2 %s prec %d bias %d: ratio %.3e of %.0e' % (shape, prec, bias, e, TOL_FWD))
            assert e < TOL_FWD, (shape, prec, bias, e)
            worst = max(worst, e)
    return worst, ntiles, wgs


@pytest.mark.parametrize('shape', [(1, 2, 2), (1, 3, 2), (1, 2, 3), (2, 7, 9), (1, 5, 34), (1, 10, 26)], ids=str)
def test_unshuffle_conv_forms(dev, layer, shape):
    worst, ntiles, wgs = _run_forms(dev, layer, shape)
    assert ntiles <= 4 * wgs  # one tile per wave at the most
    print('RRDBNET unshuffle2 %s worst ratio %.3e of %.0e (%d tiles, %d workgroups)' % (shape, worst, TOL_FWD, ntiles, wgs))


def test_unshuffle_conv_waves_walk_a_second_tile(dev, layer):
    """The smallest odd-sized image whose tiles outnumber the waves of the plan cut for the largest reservation."""
    lib, L = _L()
    lib.call('srx_set_reserved_cus', 128)
    waves = 4 * L.srx_plan_cus() * 4
    ho = 129
    wo = -(-(32 * waves + 1) // ho)
    shape = (1, 2 * ho - 1, 2 * wo - 1)
    assert _plan(*shape) == [-(-ho * wo // 32), waves // 4] and ho * wo > 32 * waves
    worst, ntiles, wgs = _run_forms(dev, layer, shape, reserved=128)
    assert 4 * wgs < ntiles < 8 * wgs  # some waves walk two tiles, some one
    print('RRDBNET unshuffle2 %s worst ratio %.3e of %.0e (%d tiles on %d waves)' % (shape, worst, TOL_FWD, ntiles, 4 * wgs))


def test_unshuffle_conv_refusals(dev, layer):
    """Refused with a non-zero code and a message, nothing launched, the NaN-filled output untouched."""
    lib, L = _L()
    w, b, _ = layer
    wpk = _packed(w, dev)
    x4 = torch.zeros(1, 8, 8, 4, device=dev)
    y = Guarded(dev, (1, 4, 4, 64), margin=NAN)
    X, W, Y = x4.data_ptr(), wpk.t.data_ptr(), y.t.data_ptr()
    cases = [('null x', (1, 8, 8, None, W, None, Y, 0)), ('null weights', (1, 8, 8, X, None, None, Y, 0)),
             ('null y', (1, 8, 8, X, W, None, None, 0)), ('H = 1', (1, 1, 8, X, W, None, Y, 0)),
             ('W = 1', (1, 8, 1, X, W, None, Y, 0)), ('H = 0', (1, 0, 8, X, W, None, Y, 0)), ('N = 0', (0, 8, 8, X, W, None, Y, 0)),
             ('2^24 pixels', (1, 4096, 4096, X, W, None, Y, 0)), ('2^24 padded pixels', (1, 4095, 4096, X, W, None, Y, 0)),
             ('precision 2', (1, 8, 8, X, W, None, Y, 2)), ('precision -1', (1, 8, 8, X, W, None, Y, -1))]
    for what, args in cases:
        rc = []
        assert prof_launches(lambda: rc.append(L.srx_unshuffle2_conv_fwd(*args, _stream()))) == [], what
        assert rc[0] != 0 and 'unshuffle2_conv' in lib.last_error(), (what, rc, lib.last_error())
        assert bool(torch.isnan(y.buf).all()), what
    out = (C.c_int * 2)()
    for n, h, wd in ((1, 1, 8), (1, 8, 1), (1, 4096, 4096), (0, 8, 8)):
        assert L.srx_unshuffle2_conv_plan(n, h, wd, out) != 0
    assert L.srx_unshuffle2_conv_plan(1, 8, 8, None) != 0
    assert L.srx_unshuffle2_conv_pack(None, W, _stream()) != 0 and L.srx_unshuffle2_conv_pack(X, None, _stream()) != 0
    # the largest call that is not refused by the pixel limit plans (host only)
    assert L.srx_unshuffle2_conv_plan(1, 4095, 4094, out) == 0 and out[0] == 2048 * 2047 // 32


# ------------------------------------------------------------------------------------------------ 2. generator vs restatement
def _gpu_generator(dev, pub, blocks, scale):
    from torchsr_amd.esrgan.generator import Generator
    from torchsr_amd.test import rrdbnet_geometry, rrdbnet_to_generator_state
    assert rrdbnet_geometry(pub) == (blocks, scale)
    gen = Generator(blocks, scale_factor=scale).to(dev)
    gen.load_state_dict(rrdbnet_to_generator_state(pub))
    return gen.eval()


@pytest.fixture(scope='module')
def nets():
    """Published-format states of 2-block nets at x4 and x2, the restatements that hold them (fp32 and fp64), inputs."""
    out = {}
    for scale in (4, 2):
        ref = RRDBNetRef(num_block=2, scale=scale)
        pub = seeded_state(ref, seed=10 + scale)
        ref.load_state_dict(pub)
        ref.eval()
        ref64 = RRDBNetRef(num_block=2, scale=scale).double()
        ref64.load_state_dict({k: v.double() for k, v in pub.items()})
        out[scale] = (pub, ref, ref64.eval())
    return out


@pytest.mark.parametrize('scale,shape', [(4, (2, 3, 12, 20)), (2, (1, 3, 7, 10)), (2, (2, 3, 12, 20))], ids=str)
def test_generator_vs_fp64_restatement(dev, nets, scale, shape):
    from torchsr_amd.test import upscale
    pub, ref32, ref64 = nets[scale]
    x = torch.rand(shape, generator=torch.Generator().manual_seed(shape[2]))
    with torch.no_grad():
        y64, y32 = ref64(x.double()), ref32(x)
    assert y64.shape == (shape[0], 3, scale * shape[2], scale * shape[3])
    gen = _gpu_generator(dev, pub, 2, scale)
    y = upscale(gen, x.to(dev), scale=scale, precision='fp32')
    assert y.shape == y64.shape and y.is_contiguous()
    e, e0 = _rel_l2(y, y64), _rel_l2(y32, y64)
    print(f'RRDBNET generator x{scale} {shape}: GPU {e:.3e}, fp32 CPU {e0:.3e} from fp64 (relative L2); ratio {e / e0:.3f} of 4')
    assert e <= 4 * e0, (e, e0)
    y16 = upscale(gen, x.to(dev), scale=scale, precision='bf16')
    assert y16.shape == y.shape and bool(torch.isfinite(y16).all())
    e16 = ((y16 - y).abs().max() / y.abs().max()).item()
    print(f'RRDBNET generator x{scale} {shape}: bf16 products {e16:.3e} of the fp32 result\'s largest value, bound {TOL_BF16:.0e}')
    assert 0 < e16 <= TOL_BF16, e16
    again = upscale(gen, x.to(dev), scale=scale, precision='fp32')  # the precision is restored
    assert torch.equal(again, y)
    with pytest.raises(ValueError, match='fp16'):
        upscale(gen, x.to(dev), scale=scale, precision='fp16')


def test_x2_is_inference_only(dev, nets):
    gen = _gpu_generator(dev, nets[2][0], 2, 2)
    x = torch.rand(1, 3, 8, 8, device=dev)
    with pytest.raises(RuntimeError, match='inference-only'):
        gen.eval()(x)  # autograd enabled
    with torch.no_grad(), pytest.raises(RuntimeError, match='inference-only'):
        gen.train()(x)
    with torch.no_grad(), pytest.raises(RuntimeError, match='at least 3'):
        gen.eval()(torch.rand(1, 3, 8, 1, device=dev))
    with torch.no_grad():
        assert gen.eval()(x).shape == (1, 3, 16, 16)


# ------------------------------------------------------------------------------------------------ 3. tiled == untiled at x2
def test_x2_tiled_inference_equals_untiled(dev):
    """One RRDB (receptive radius under 40 input pixels at x2: the 17 convs at trunk resolution reach 34, the four
    high-resolution convs 3 more), a 97 x 140 image -- the bottom edge is odd, so the last row of tiles reflects -- halo 40."""
    from torchsr_amd.test import tile_plan, upscale
    ref = RRDBNetRef(num_block=1, scale=2)
    gen = _gpu_generator(dev, seeded_state(ref, seed=21), 1, 2)
    lr = torch.rand(1, 3, 97, 140, generator=torch.Generator().manual_seed(22)).to(dev)
    th, tw, halo, tiles = tile_plan(97, 140, 40, 3000, gen.tile_align)
    assert len({t[0] for t in tiles}) >= 2 and len({t[2] for t in tiles}) >= 2 and halo == 40  # at least a 2 x 2 grid
    whole = upscale(gen, lr, scale=2, max_tile_pixels=10 ** 9, precision='fp32')
    tiled = upscale(gen, lr, halo=40, scale=2, max_tile_pixels=3000, precision='fp32')
    assert whole.shape == tiled.shape == (1, 3, 194, 280)
    err = (whole - tiled).abs().max().item() / whole.abs().max().item()
    print(f'RRDBNET x2 tiled vs whole ({len(tiles)} tiles of {th} x {tw}): {err:.3e} of the largest value, bound {TOL_TILED:.0e}')
    assert err <= TOL_TILED


# ------------------------------------------------------------------------------------------------ 4. the command line
@pytest.mark.parametrize('blocks,scale', [(2, 2), (6, 4)])
def test_cli_on_published_format_files(dev, tmp_path, monkeypatch, blocks, scale):
    from PIL import Image
    from torchsr_amd.srgan.trainer import save_image
    from torchsr_amd.test import upscale
    from torchsr_amd.torchsr import main
    monkeypatch.chdir(tmp_path)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'LOCAL_WORLD_SIZE', 'SLURM_NTASKS'):
        monkeypatch.delenv(k, raising=False)
    pub = seeded_state(RRDBNetRef(num_block=blocks, scale=scale), seed=30 + blocks)
    torch.save({'params': {k: torch.zeros_like(v) for k, v in pub.items()}, 'params_ema': pub}, 'published.pth')
    h, w = 21, 28  # an odd height
    rgb = (np.random.RandomState(3).rand(h, w, 3) * 255).astype('uint8')
    Image.fromarray(rgb).save('lr.png')
    main(['test', 'lr.png', '--model', 'esrgan', '--weights', 'published.pth'])
    got = np.asarray(Image.open('upres-lr.png'))
    assert got.shape == (scale * h, scale * w, 3)
    gen = _gpu_generator(dev, pub, blocks, scale)
    low_res = torch.from_numpy(rgb.astype('float32') / 255.0).permute(2, 0, 1).unsqueeze(0).contiguous().to(dev)
    save_image(upscale(gen, low_res, scale=scale, precision='fp32'), 'by-hand.png')
    assert np.array_equal(got, np.asarray(Image.open('by-hand.png')))
    assert got.std() > 1.0  # a picture, not a constant
    main(['test', 'lr.png', '--model', 'esrgan', '--weights', 'published.pth', '--self-ensemble', '4', '--color-fix', 'adain',
          '--outscale', '1.5'])
    got = np.asarray(Image.open('upres-lr.png'))
    assert got.shape == (int(h * 1.5 + 0.5), int(w * 1.5 + 0.5), 3)
    save_image(upscale(gen, low_res, scale=scale, precision='fp32', self_ensemble=4, color_fix='adain', outscale=1.5), 'by-hand.png')
    assert np.array_equal(got, np.asarray(Image.open('by-hand.png')))


def test_x2_composes_with_ensemble_color_fix_and_outscale(dev, nets):
    """All three take their ratio from the shapes: at x2, on an odd-sized image, each is what it is at x4 -- the 8-variant
    ensemble (transposes included: a 7 x 10 and a 10 x 7 image pad different axes) is the mean of the mapped-back variants."""
    from torchsr_amd import functional as F
    from torchsr_amd.test import upscale
    gen = _gpu_generator(dev, nets[2][0], 2, 2)
    x = torch.rand(1, 3, 7, 10, generator=torch.Generator().manual_seed(40)).to(dev)
    ens = upscale(gen, x, scale=2, precision='fp32', self_ensemble=8)
    assert ens.shape == (1, 3, 14, 20)
    acc = torch.zeros_like(ens, dtype=torch.float64)
    for k in range(8):
        y_k = upscale(gen, x if k == 0 else F.dihedral(x, k), scale=2, precision='fp32')
        acc += (y_k if k == 0 else F.dihedral(y_k, F.dihedral_inverse(k))).double()
    assert (ens.double() - acc / 8).abs().max().item() <= 1e-6 * ens.abs().max().item()
    plain = upscale(gen, x, scale=2, precision='fp32')
    for fix in ('wavelet', 'adain'):
        fixed = upscale(gen, x, scale=2, precision='fp32', color_fix=fix)
        want = (F.color_fix_wavelet if fix == 'wavelet' else F.color_fix_adain)(plain, x)
        assert fixed.shape == plain.shape and torch.equal(fixed, want)
    assert torch.equal(upscale(gen, x, scale=2, precision='fp32', outscale=2), plain)  # the model's own scale: untouched
    out3 = upscale(gen, x, scale=2, precision='fp32', outscale=3)
    assert out3.shape == (1, 3, 21, 30) and torch.equal(out3, F.resize_bicubic_aa(plain, (21, 30)))


# ------------------------------------------------------------------------------------------------ 5. unchanged ground
def test_x4_generator_is_unchanged(dev):
    from torchsr_amd.esrgan.generator import Generator
    torch.manual_seed(50)
    a = Generator(2).to(dev).eval()
    b = Generator(2, scale_factor=4).to(dev).eval()
    b.load_state_dict(a.state_dict())
    ref = RRDBNetRef(num_block=2, scale=4)
    from torchsr_amd.test import rrdbnet_to_generator_state
    assert list(a.state_dict()) == list(b.state_dict()) == list(rrdbnet_to_generator_state(ref.state_dict()))
    assert len(a.state_dict()) == 2 * (6 + 2 * 15)
    x = torch.rand(1, 3, 12, 20, device=dev)
    out = {}
    with torch.no_grad():
        a(x), b(x)  # weight packs
        la = prof_launches(lambda: out.setdefault('a', a(x)))
        lb = prof_launches(lambda: out.setdefault('b', b(x)))
    assert la == lb and torch.equal(out['a'], out['b'])
    assert not any('unshuffle' in name for name in la) and len(la) >= 6
