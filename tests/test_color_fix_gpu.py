"""``--color-fix`` on the GPU: the a-trous level kernel (``srx_color_fix_wavelet_level``, ``F.color_fix_wavelet``) against its
fp32 restatement bit for bit -- reproducibility, plane independence, guard bands, unaligned operands --, the plane moments
and the AdaIN map against fp64 with the derived bound, ``upscale(color_fix=)`` against its restatement bit for bit, the fp16
overflow report and the CLI."""
import numpy as np
import pytest
import torch

import colorfix_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64  # floats of NaN on either side of a guarded buffer (a multiple of 4: the 16-byte alignment stays)

# planes, sr (H, W), lr (h, w): one element; every radius beyond the plane; N = 2; odd width, non-integer ratio (the scalar
# form); x2; several workgroups per plane (the 16-byte form: 130 quads per row, 280 = 17 * 16 + 8 rows) and a tail
SHAPES = [(3, 1, 1, 1, 1), (3, 8, 12, 2, 3), (6, 36, 68, 9, 17), (3, 37, 53, 9, 13), (3, 10, 14, 5, 7), (3, 280, 520, 70, 130)]


def _offset_view(t):
    """A contiguous copy of ``t`` whose base is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _guarded(shape, dev, offset=0, dtype=torch.float32):
    """A NaN-filled buffer and the view of ``shape`` in its middle (``offset`` elements off the 16-byte alignment)."""
    n = int(np.prod(shape))
    buf = torch.full((GUARD + offset + n + GUARD,), float('nan'), device=dev, dtype=dtype)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD + offset:GUARD + offset + n].view(shape)


def _band_kept(buf, view):
    n, lo = view.numel(), (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + n:]).all())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def abi_wavelet(sr, u, levels, offset=0):
    """The levels through ``srx_color_fix_wavelet_level`` itself, as ``F.color_fix_wavelet`` chains them, the result and both
    workspaces inside NaN guard bands that must survive (``offset`` floats off the 16-byte alignment)."""
    from torchsr_amd import _lib
    n, c, h, w = sr.shape
    bufs = [_guarded(sr.shape, sr.device, offset) for _ in range(3)]
    src = u
    for i in range(levels):
        last = i == levels - 1
        dst = bufs[2][1] if last else bufs[i & 1][1]
        _lib.call('srx_color_fix_wavelet_level', src.data_ptr(), sr.data_ptr() if i == 0 else None, sr.data_ptr() if last else None,
                  dst.data_ptr(), n * c, h, w, 1 << i, _stream())
        src = dst
    for i, (buf, view) in enumerate(bufs):
        assert _band_kept(buf, view), f'a level wrote outside buffer {i}'
        written = i == 2 or i < levels - 1
        assert bool(torch.isnan(view).any()) != written, f'buffer {i}: an element was left unwritten (or a spare buffer touched)'
    return bufs[2][1]


def _frames(planes, H, W, h, w, dev, lo=-0.1, span=1.2):
    g = torch.Generator().manual_seed(1000 * H + W)
    sr = (torch.rand(planes // 3, 3, H, W, generator=g) * span + lo).to(dev)
    lr = (torch.rand(planes // 3, 3, h, w, generator=g) * span + lo).to(dev)
    return sr, lr


@pytest.mark.parametrize('planes,H,W,h,w', SHAPES)
def test_wavelet_kernel_equals_its_restatement_bitwise(dev, planes, H, W, h, w):
    from torchsr_amd import functional as F
    sr, lr = _frames(planes, H, W, h, w, dev)
    sr0, lr0 = sr.clone(), lr.clone()
    with torch.no_grad():
        u = F.resize_bicubic_aa(lr, (H, W))  # the device's own enlargement (lr itself for equal sizes)
        for levels in (1, 3, 5):
            want = torch.from_numpy(R.wavelet32(sr.cpu().numpy(), u.cpu().numpy(), levels))
            got = abi_wavelet(sr, u, levels)
            diff = (got.cpu().double() - want.double()).abs().max().item()
            print(f'{(planes, H, W)} levels {levels}: max |kernel - restatement| = {diff:.3e}')
            assert torch.equal(got.cpu(), want), (levels, diff)
            assert torch.equal(abi_wavelet(sr, u, levels), got)                     # the same bits from a second call
            for p in {0, planes - 1}:                                               # a plane alone: the bits it has in the batch
                one = lambda t: t.view(1, planes, H, W)[:, p:p + 1].contiguous()    # noqa: E731
                assert torch.equal(abi_wavelet(one(sr), one(u), levels), got.view(1, planes, H, W)[:, p:p + 1]), (levels, p)
            # 4 bytes off the 16-byte alignment: operands, result and workspaces, together and one side at a time
            assert torch.equal(abi_wavelet(_offset_view(sr), _offset_view(u), levels, offset=1), got), levels
            assert torch.equal(abi_wavelet(_offset_view(sr), u, levels), got), levels
            assert torch.equal(abi_wavelet(sr, u, levels, offset=3), got), levels
            op = F.color_fix_wavelet(sr, lr, levels=levels)                         # the operator: the same chain behind the resize
            assert op.shape == sr.shape and torch.equal(op, got), levels
            out = torch.full_like(sr, float('nan'))
            assert F.color_fix_wavelet(sr, lr, levels=levels, out=out) is out and torch.equal(out, got)
        assert torch.equal(F.color_fix_wavelet(sr, lr), F.color_fix_wavelet(sr, lr, levels=5))
        assert torch.equal(F.color_fix_wavelet(u, lr), u)                           # sr == U: sr itself, bit for bit
        with pytest.raises(RuntimeError, match='overlap'):
            F.color_fix_wavelet(sr, lr, out=sr)
    assert torch.equal(sr, sr0) and torch.equal(lr, lr0)                            # the workspaces left the inputs alone


def abi_adain(sr, lr, offset=0):
    """``srx_plane_moments`` twice and ``srx_color_fix_adain_apply``, the partial sums, the statistics and the result inside NaN
    guard bands that must survive.  Returns the result and the two [planes][2] statistics."""
    from torchsr_amd import _lib
    lib = _lib.lib()
    stats = []
    for x in (sr, lr):
        n, c, h, w = x.shape
        blocks = lib.srx_plane_moments_blocks(h, w)
        assert blocks >= 1
        pbuf, part = _guarded((n * c, blocks, 2), x.device, dtype=torch.float64)
        sbuf, st = _guarded((n * c, 2), x.device, dtype=torch.float64)
        _lib.call('srx_plane_moments', x.data_ptr(), n * c, h, w, part.data_ptr(), part.numel(), st.data_ptr(), _stream())
        assert _band_kept(pbuf, part) and _band_kept(sbuf, st), 'the moments wrote outside their buffers'
        assert not torch.isnan(part).any() and not torch.isnan(st).any(), 'a partial sum or a statistic was left unwritten'
        stats.append(st)
    n, c, h, w = sr.shape
    dbuf, dst = _guarded(sr.shape, sr.device, offset)
    _lib.call('srx_color_fix_adain_apply', sr.data_ptr(), dst.data_ptr(), n * c, h, w, stats[0].data_ptr(), stats[1].data_ptr(), _stream())
    assert _band_kept(dbuf, dst), 'the map wrote outside dst'
    assert not torch.isnan(dst).any(), 'an element was left unwritten'
    return dst, stats[0], stats[1]


@pytest.mark.parametrize('planes,H,W,h,w', SHAPES)
def test_moments_and_adain_against_fp64(dev, planes, H, W, h, w):
    """Image-like values with one constant plane of ``sr`` (variance 0 must map to mean_lr): the statistics against numpy's
    fp64, the result within ``4 * 2^-24 * (|sr| s + |b|)`` of the fp64 value, reproducible, the same for a plane alone and
    for unaligned operands."""
    from torchsr_amd import functional as F
    sr, lr = _frames(planes, H, W, h, w, dev)
    sr[0, 1] = 0.37
    with torch.no_grad():
        got, st_sr, st_lr = abi_adain(sr, lr)
        for st, x in ((st_sr, sr), (st_lr, lr)):
            mean, var = R.moments64(x.cpu().numpy().reshape(planes, *x.shape[2:]))
            # fp64 sums of at most 145,600 terms: far inside 1e-11 relative (of the second moment for the variance)
            assert np.allclose(st[:, 0].cpu().numpy(), mean, rtol=1e-11, atol=0)
            assert (np.abs(st[:, 1].cpu().numpy() - var) <= 1e-11 * (var + mean * mean)).all()
        assert st_sr[1, 1].item() == 0.0 and st_sr[1, 0].item() == float(np.float32(0.37))   # exactly: sums of x - x[0]
        if H * W == 1:
            assert (st_sr[:, 1] == 0).all() and (st_lr[:, 1] == 0).all()
        want, (s, b), bound = R.adain_ref(sr.cpu().numpy(), lr.cpu().numpy())
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        print(f'{(planes, H, W)} <- {(h, w)}: max err {err.max():.3e}, at most {(err / bound).max():.3f} of the bound')
        assert (err <= bound).all()
        mean_lr = R.moments64(lr.cpu().numpy())[0]
        assert (np.abs(got.cpu().numpy()[0, 1].astype(np.float64) - mean_lr[0, 1]) <= bound[0, 1]).all()  # the constant plane
        assert torch.equal(abi_adain(sr, lr)[0], got)                                  # the same bits from a second call
        assert torch.equal(F.color_fix_adain(sr, lr), got)
        out = torch.full_like(sr, float('nan'))
        assert F.color_fix_adain(sr, lr, out=out) is out and torch.equal(out, got)
        assert torch.equal(F.plane_moments(sr).view(planes, 2), st_sr)
        for p in {0, planes - 1}:                                                      # a plane alone
            one = lambda t: t.view(1, planes, *t.shape[2:])[:, p:p + 1].contiguous()   # noqa: E731
            assert torch.equal(abi_adain(one(sr), one(lr))[0], got.view(1, planes, H, W)[:, p:p + 1]), p
        assert torch.equal(abi_adain(_offset_view(sr), _offset_view(lr), offset=1)[0], got)
        assert torch.equal(abi_adain(sr, lr, offset=3)[0], got)


@pytest.mark.parametrize('planes,H,W,h,w', SHAPES)
def test_adain_result_has_the_moments_of_the_input(dev, planes, H, W, h, w):
    """The result's own per-plane mean and standard deviation equal lr's to 1e-5 relative.  The map's 1e-5 under the roots
    moves the standard deviation by 0.5e-5 |1 / var_lr - 1 / var_sr| relative, so the values here span 16 (variances near 20
    and 10): that term stays below 2e-6 (asserted on the inputs) and what is checked is the kernels' arithmetic.  A one-pixel
    plane has no standard deviation; its mean is checked."""
    from torchsr_amd import functional as F
    sr, lr = _frames(planes, H, W, h, w, dev, lo=-2.0, span=16.0)
    lr = lr * 0.7 + 1.0
    with torch.no_grad():
        got = F.color_fix_adain(sr, lr).cpu().numpy()
    (m, v), (ml, vl), (_, vs) = R.moments64(got), R.moments64(lr.cpu().numpy()), R.moments64(sr.cpu().numpy())
    print(f'{(planes, H, W)}: mean off by {np.abs(m / ml - 1).max():.2e} relative')
    assert (np.abs(m - ml) <= 1e-5 * np.abs(ml)).all()
    if H * W > 1 and h * w > 1:
        assert (0.5e-5 * np.abs(1 / vl - 1 / vs) < 2e-6).all()
        print(f'{(planes, H, W)}: std off by {np.abs(np.sqrt(v / vl) - 1).max():.2e} relative')
        assert (np.abs(np.sqrt(v) - np.sqrt(vl)) <= 1e-5 * np.sqrt(vl)).all()


# ------------------------------------------------------------------------------------------------ upscale(color_fix=)
def _srgan_state():
    """``closed_form_state`` with ``blocks.i.bn2`` halved, as the fp16 inference tests do: the activations stay near 1e2,
    inside fp16's range."""
    from oracle.weights import closed_form_state
    from torchsr_amd.srgan.generator import Generator
    sd = closed_form_state(Generator().state_dict())
    for i in range(16):
        for key in ('weight', 'bias'):
            sd[f'blocks.{i}.bn2.{key}'] = sd[f'blocks.{i}.bn2.{key}'] * 0.5
    return sd


def _srgan(dev):
    from torchsr_amd.srgan.generator import Generator
    gen = Generator().to(dev)
    gen.load_state_dict(_srgan_state())
    return gen


def _esrgan(dev):
    from torchsr_amd.esrgan.generator import Generator
    torch.manual_seed(3)
    return Generator(num_rrdb_blocks=1).to(dev)


def _conv_precisions(gen):
    from torchsr_amd.layers import Conv2d
    return [m._st.precision for m in gen.modules() if isinstance(m, Conv2d)]


CASES = [
    ('srgan', (2, 3, 24, 40), dict(precision='fp32')),
    ('srgan', (2, 3, 24, 40), dict(precision='bf16')),
    ('srgan', (2, 3, 24, 40), dict(precision='fp16')),
    ('esrgan', (1, 3, 16, 24), dict(precision='fp32')),
    ('srgan', (2, 3, 24, 40), dict(max_tile_pixels=24 * 20, staged=False)),   # halo tiling
]


@pytest.mark.parametrize('model,shape,kw', CASES, ids=[f'{m}-' + '-'.join(f'{a}={b}' for a, b in kw.items()) for m, _, kw in CASES])
def test_upscale_color_fix_equals_its_restatement_bitwise(dev, model, shape, kw):
    """``upscale(color_fix=m)`` is the colour fix of ``upscale()`` against the original input; with the self-ensemble and an
    ``outscale`` it is ``resize(color_fix(ensemble))``; ``None`` is the path of before."""
    from torchsr_amd import functional as F
    from torchsr_amd.test import upscale
    gen = _srgan(dev) if model == 'srgan' else _esrgan(dev)
    before = _conv_precisions(gen)
    lr = torch.rand(*shape, generator=torch.Generator().manual_seed(7)).to(dev)
    size = (2 * shape[2], 2 * shape[3])
    plain = upscale(gen, lr, **kw)
    mean4 = upscale(gen, lr, self_ensemble=4, **kw)
    assert plain.shape == (shape[0], 3, 4 * shape[2], 4 * shape[3]) and torch.isfinite(plain).all()
    assert torch.equal(upscale(gen, lr, color_fix=None, **kw), plain)
    for mode, fix in (('wavelet', F.color_fix_wavelet), ('adain', F.color_fix_adain)):
        got = upscale(gen, lr, color_fix=mode, **kw)
        assert _conv_precisions(gen) == before
        with torch.no_grad():
            want = fix(plain, lr)
        assert got.shape == plain.shape and torch.equal(got, want), (mode, (got - want).abs().max().item())
        assert torch.isfinite(got).all() and not torch.equal(got, plain)
        got = upscale(gen, lr, color_fix=mode, self_ensemble=4, outscale=2, **kw)
        with torch.no_grad():
            want = F.resize_bicubic_aa(fix(mean4, lr), size)
        assert got.shape == (shape[0], 3) + size and torch.equal(got, want), (mode, (got - want).abs().max().item())
    assert _conv_precisions(gen) == before
    assert torch.equal(upscale(gen, lr, **kw), plain)


def test_color_fix_reports_fp16_overflow(dev):
    """A non-finite fp16 frame still raises and never reaches the colour fix."""
    from torchsr_amd import functional as F
    from torchsr_amd.test import upscale
    gen = _srgan(dev)
    with torch.no_grad():
        gen.conv1[0].weight.mul_(1e8)
    lr = torch.rand(1, 3, 32, 40, generator=torch.Generator().manual_seed(9)).to(dev)
    before = _conv_precisions(gen)
    calls = []
    real = F.color_fix_wavelet, F.color_fix_adain
    F.color_fix_wavelet = lambda *a, **k: calls.append(a) or real[0](*a, **k)
    F.color_fix_adain = lambda *a, **k: calls.append(a) or real[1](*a, **k)
    try:
        for mode in ('wavelet', 'adain'):
            with pytest.raises(FloatingPointError, match='65504'):
                upscale(gen, lr, precision='fp16', color_fix=mode)
            assert not calls and _conv_precisions(gen) == before
            with pytest.raises(FloatingPointError, match='65504'):
                upscale(gen, lr, precision='fp16', color_fix=mode, self_ensemble=4, outscale=2)
            assert not calls and _conv_precisions(gen) == before
        out = upscale(gen, lr, precision='fp32', color_fix='adain')
        assert len(calls) == 1 and out.shape == (1, 3, 128, 160) and torch.isfinite(out).all()
    finally:
        F.color_fix_wavelet, F.color_fix_adain = real
    assert _conv_precisions(gen) == before


def test_cli_color_fix(dev, tmp_path, monkeypatch):
    """``torchsr test lr.png --model srgan --color-fix wavelet`` writes what ``upscale(..., color_fix='wavelet')`` gives, byte for
    byte the ``save_image`` of the API result; the file keeps its name."""
    from PIL import Image
    from torchsr_amd.srgan.trainer import save_image
    from torchsr_amd.test import upscale
    from torchsr_amd.torchsr import main
    monkeypatch.chdir(tmp_path)
    torch.save({'epoch': 1, 'phase': 'srgan-gan', 'state': _srgan_state()}, 'srgan-gan-best.pth')
    img = (np.random.RandomState(2).rand(24, 40, 3) * 255).astype('uint8')
    Image.fromarray(img).save('lr.png')
    low_res = torch.from_numpy(img.astype('float32') / 255.0).permute(2, 0, 1).unsqueeze(0).contiguous().to(dev)
    main(['test', 'lr.png', '--model', 'srgan', '--color-fix', 'wavelet'])
    with Image.open('upres-lr.png') as f:
        assert f.size == (160, 96)
    save_image(upscale(_srgan(dev), low_res, precision='fp32', color_fix='wavelet'), 'want.png')
    save_image(upscale(_srgan(dev), low_res, precision='fp32'), 'plain.png')
    with open('upres-lr.png', 'rb') as a, open('want.png', 'rb') as b, open('plain.png', 'rb') as c:
        fixed = a.read()
        assert fixed == b.read() and fixed != c.read()
