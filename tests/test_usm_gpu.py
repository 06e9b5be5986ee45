"""``--gt-usm`` on the GPU: ``srx_usm_sharpen`` against its float64 restatement (usm_ref.py) with the bounds of DESIGN.md,
'Sharpened targets', its exact identities, ``functional.usm_sharpen`` against the raw call, the ``gt_usm`` DeviceLoader against
the plain one and the chains of calls made by hand, and the CLI."""
import functools
import os

import numpy as np
import pytest
import torch

import usm_ref as U

pytestmark = pytest.mark.gpu

GUARD = 64  # floats of NaN on either side of every output: a store outside the tensor shows


def _guarded(shape, dev):
    n = int(np.prod(shape))
    buf = torch.full((GUARD + n + GUARD,), float('nan'), device=dev)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _band_kept(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def gpu_usm(x, ksize, sigma, weight, threshold, dev):
    """The raw ABI call on NaN-guarded outputs: ``(out, blur, mask)`` on the device."""
    from torchsr_amd import _lib
    from torchsr_amd import functional as F
    xd = torch.as_tensor(x, dtype=torch.float32).to(dev).contiguous()
    n, c, h, w = xd.shape
    taps = torch.from_numpy(F.usm_taps(ksize, sigma)).to(dev)
    bufs, outs = zip(*(_guarded(xd.shape, dev) for _ in range(3)))
    _lib.call('srx_usm_sharpen', xd.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), taps.data_ptr(), ksize,
              n * c, h, w, weight, threshold, _stream())
    torch.cuda.synchronize()
    assert all(_band_kept(b) for b in bufs)
    assert not any(bool(torch.isnan(o).any()) for o in outs)   # every element was written
    return outs


# ---------------------------------------------------------------------------------------------------------------- the operation
CASES = {
    # the smallest legal plane: every tap but the centre column's is reflected, on both sides within one tile
    'smallest-plane': ((26, 26), 51, 8.0, 0.5, 10.0),
    # odd sizes; W crosses a tile edge while both borders still reflect into the same staged rows
    'odd-27x61': ((27, 61), 51, 8.0, 0.5, 10.0),
    # the training crop: nine tiles, the middle one with a halo that never reflects
    'crop-96': ((96, 96), 51, 8.0, 0.5, 10.0),
    'crop-96-threshold-25': ((96, 96), 51, 8.0, 0.5, 25.0),
    # other parameters; the clamp of sharp is active
    'k21-weight-1': ((40, 72), 21, 2.5, 1.0, 4.0),
    # one pixel past a tile in each axis, short kernel
    'k7-one-past-a-tile': ((33, 35), 7, 1.7, 0.5, 10.0),
}
DELTA = 4e-3            # grey levels: 2.5 x the blur bound at k = 51, 255 * 6.2e-6 = 1.6e-3
UNDECIDED_MAX = 0.005   # of a case's elements


@functools.lru_cache(maxsize=None)
def _case(case):
    """A case's image and float64 results, computed once: ``(x, g, out, blur, mask, t)``."""
    (h, w), k, sigma, weight, threshold = CASES[case]
    x = U.images(2, h, w)
    g = U.taps64(k, sigma)
    return (x, g) + U.usm(x, g, weight, threshold)


@pytest.mark.parametrize('case', list(CASES))
def test_usm_against_float64(dev, case):
    (h, w), k, sigma, weight, threshold = CASES[case]
    x, g, _, blur64, mask64, t = _case(case)
    assert 0.1 < float(mask64.mean()) < 0.9                       # neither branch of the mask is vacuous
    out, blur, mask = (o.cpu() for o in gpu_usm(x, k, sigma, weight, threshold, dev))
    # blur: two passes of k products and sums on positive weights of sum 1, inputs in [0, 1]
    blur_tol = (2 * k + 2) * 2.0 ** -24
    blur_err = float((blur.double() - blur64).abs().max())
    print(f'{case}: max |blur err| = {blur_err:.3e} (bound {blur_tol:.3e})')
    assert blur_err <= blur_tol
    # mask: exactly 0 or 1; equal to the reference's wherever the residual is not within DELTA grey levels of the threshold
    assert bool(((mask == 0) | (mask == 1)).all())
    decided = (t - threshold).abs() >= DELTA
    undecided = 1.0 - float(decided.double().mean())
    flipped = int((mask.double() != mask64).sum())
    print(f'{case}: mask mean {float(mask64.mean()):.3f}, undecided {100 * undecided:.4f} %, flipped {flipped}')
    assert torch.equal(mask.double()[decided], mask64[decided])
    assert undecided <= UNDECIDED_MAX
    # out: the float64 formula with the DEVICE's mask, everywhere
    want = U.blend(x, blur64, mask.double(), g, weight)
    out_tol = (2 * k + 8) * 2.0 ** -24
    out_err = float((out.double() - want).abs().max())
    print(f'{case}: max |out err| = {out_err:.3e} (bound {out_tol:.3e}); sharpening moved the image by '
          f'{float((want - torch.from_numpy(x)).abs().max()):.3f}')
    assert out_err <= out_tol
    assert float((want - torch.from_numpy(x)).abs().max()) > 100 * out_tol   # the case sharpens something
    if case == 'k21-weight-1':
        xs = torch.from_numpy(x).double()
        raw = xs + weight * (xs - blur64)
        assert bool(((raw < 0) | (raw > 1)).any())                # the clamp of sharp is active


def test_usm_exact_identities(dev):
    x = U.images(2, 96, 96)
    xd = torch.from_numpy(x).to(dev)
    out, _, mask = gpu_usm(x, 51, 8.0, 0.0, 10.0, dev)            # weight 0: sharp is x
    assert torch.equal(out, xd) and 0.1 < float(mask.mean()) < 0.9
    out, _, mask = gpu_usm(x, 51, 8.0, 0.5, 300.0, dev)           # no residual reaches 300 grey levels
    assert torch.equal(out, xd) and float(mask.sum()) == 0
    flat = np.full((2, 3, 61, 45), 0.37, dtype=np.float32)
    out, blur, mask = gpu_usm(flat, 51, 8.0, 0.5, 10.0, dev)
    assert torch.equal(out, torch.from_numpy(flat).to(dev)) and float(mask.sum()) == 0
    assert float((blur - 0.37).abs().max()) <= 104 * 2.0 ** -24


def test_usm_is_deterministic(dev):
    x = U.images(2, 27, 61)
    first = gpu_usm(x, 51, 8.0, 0.5, 10.0, dev)
    again = gpu_usm(x, 51, 8.0, 0.5, 10.0, dev)
    assert all(torch.equal(a, b) for a, b in zip(first, again))


def test_functional_usm_sharpen(dev):
    from torchsr_amd import functional as F
    x = U.images(2, 40, 72)
    xd = torch.from_numpy(x).to(dev)
    raw = gpu_usm(x, 51, 8.0, 0.5, 10.0, dev)
    with torch.no_grad():
        out = F.usm_sharpen(xd)
        staged = F.usm_sharpen(xd, return_stages=True)
    assert out is not xd and torch.equal(xd, torch.from_numpy(x).to(dev))      # a new tensor; the input is untouched
    assert torch.equal(out, raw[0])
    assert len(staged) == 3 and all(torch.equal(a, b) for a, b in zip(staged, raw))
    raw21 = gpu_usm(x, 21, 2.5, 1.0, 4.0, dev)
    assert all(torch.equal(a, b) for a, b in zip(F.usm_sharpen(xd, 21, 2.5, 1.0, 4.0, return_stages=True), raw21))
    assert not torch.equal(raw21[0], raw[0])
    assert torch.equal(F.usm_sharpen(xd.transpose(2, 3)), F.usm_sharpen(xd.transpose(2, 3).contiguous()))  # strided input
    with pytest.raises(RuntimeError, match='no backward'):
        F.usm_sharpen(xd.clone().requires_grad_())
    with torch.no_grad():
        assert torch.equal(F.usm_sharpen(xd.clone().requires_grad_()), out)   # refused under grad mode only
    with pytest.raises(ValueError):
        F.usm_sharpen(torch.zeros((1, 3, 25, 40), device=dev))
    with pytest.raises(ValueError):
        F.usm_sharpen(torch.zeros((1, 3, 40, 25), device=dev))
    with torch.no_grad():
        assert F.usm_sharpen(torch.zeros((1, 3, 26, 26), device=dev)).abs().max() == 0


# ---------------------------------------------------------------------------------------------------------------- loader
SIZES = [(120, 150), (97, 96), (200, 130), (96, 96), (140, 101), (60, 80), (128, 128), (110, 99), (100, 100), (150, 97)]
LOADER_SEED = 1


@pytest.fixture(scope='module')
def image_dir(tmp_path_factory):
    """The ten random PNGs of test_degrade2_gpu.py."""
    from PIL import Image
    d = tmp_path_factory.mktemp('usm') / 'imgs'
    os.makedirs(d)
    rng = np.random.RandomState(0)
    for i, (h, w) in enumerate(SIZES):
        Image.fromarray((rng.rand(h, w, 3) * 255).astype('uint8')).save(str(d / f'{i}.png'))
    return str(d)


def _loaders(image_dir, dev, degradation, **kw):
    from torchsr_amd.dataset import initialize_device_datasets
    return initialize_device_datasets(image_dir, dev, batch_size=4, crop_size=96, seed=LOADER_SEED, degradation=degradation, **kw)[:2]


def bicubic_by_hand(hr, dev):
    from torchsr_amd import _lib
    lr = torch.empty((hr.shape[0], 3, 24, 24), device=dev)
    _lib.call('srx_bicubic_down', hr.data_ptr(), lr.data_ptr(), hr.shape[0], 3, 96, 96, 4, 1, _stream())
    return lr


def blind_by_hand(hr, deg, dev):
    """The four ABI calls of one ``blind`` batch, from what the loader kept."""
    from torchsr_amd import _lib
    s, n = _stream(), hr.shape[0]
    dv = {k: torch.from_numpy(deg[k]).to(dev) for k in ('parm', 'ksize', 'sigma_n', 'gray', 'quality')}
    a = torch.empty_like(hr)
    b, c, d = (torch.empty((n, 3, 24, 24), device=dev) for _ in range(3))
    _lib.call('srx_blur_aniso', hr.data_ptr(), a.data_ptr(), dv['parm'].data_ptr(), dv['ksize'].data_ptr(), n, 3, 96, 96, s)
    _lib.call('srx_bicubic_down', a.data_ptr(), b.data_ptr(), n, 3, 96, 96, 4, 0, s)
    _lib.call('srx_add_gaussian_noise', b.data_ptr(), c.data_ptr(), dv['sigma_n'].data_ptr(), dv['gray'].data_ptr(),
              deg['seed'] & 0xFFFFFFFF, deg['seed'] >> 32, n, 24, 24, 1, s)
    _lib.call('srx_jpeg_sim', c.data_ptr(), d.data_ptr(), dv['quality'].data_ptr(), n, 24, 24, 1, s)
    return d


def blind2_by_hand(hr, deg, dev):
    """The chain of ABI / ``functional.resize`` calls of one ``blind2`` batch, from what the loader kept (``by_hand`` of
    test_degrade2_gpu.py)."""
    from torchsr_amd import _lib
    from torchsr_amd import functional as F
    s, n = _stream(), hr.shape[0]
    dv = {k: torch.from_numpy(deg[k]).to(dev) for k in ('weights', 'ksize', 'sigma_n', 'gray', 'quality')}
    (s1, s2, lc), modes = deg['sizes'], deg['modes']

    def filt(x, stage, quantize):
        out = torch.empty_like(x)
        _lib.call('srx_filter2d', x.data_ptr(), out.data_ptr(), dv['weights'][stage].data_ptr(), dv['ksize'][stage].data_ptr(), n, 3,
                  x.shape[2], x.shape[3], quantize, s)
        return out

    def noise(x, stage, seed):
        out = torch.empty_like(x)
        _lib.call('srx_add_gaussian_noise', x.data_ptr(), out.data_ptr(), dv['sigma_n'][stage].data_ptr(), dv['gray'][stage].data_ptr(),
                  seed & 0xFFFFFFFF, seed >> 32, n, x.shape[2], x.shape[3], 1, s)
        return out

    def jpeg(x, stage):
        out = torch.empty_like(x)
        _lib.call('srx_jpeg_sim', x.data_ptr(), out.data_ptr(), dv['quality'][stage].data_ptr(), n, x.shape[2], x.shape[3], 1, s)
        return out

    with torch.no_grad():
        a = filt(hr, 0, 0)
        b = F.resize(a, (s1, s1), modes[0])
        c = noise(b, 0, deg['seed1'])
        d = jpeg(c, 0)
        e = filt(d, 1, 0)
        f = F.resize(e, (s2, s2), modes[1])
        g = noise(f, 1, deg['seed2'])
        assert tuple(d.shape) == (n, 3, s1, s1) and tuple(g.shape) == (n, 3, s2, s2)
        if deg['order'] == 'A':
            return jpeg(filt(F.resize(g, (lc, lc), modes[2]), 2, 0), 1)
        return filt(F.resize(jpeg(g, 1), (lc, lc), modes[2]), 2, 1)


def _same_draws(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize('degradation', ['bicubic', 'blind', 'blind2'])
def test_gt_usm_loader(dev, image_dir, degradation):
    from torchsr_amd import functional as F
    (usm, usm_test), (plain, plain_test) = _loaders(image_dir, dev, degradation, gt_usm=True), _loaders(image_dir, dev, degradation)
    assert usm.gt_usm is True and plain.gt_usm is False and usm_test.gt_usm is False and len(usm) == 2
    batches = 0
    for _ in range(2):  # epochs
        for (lr, hr), (lr_p, hr_p) in zip(usm, plain):
            assert lr.shape == (4, 3, 24, 24) and hr.shape == (4, 3, 96, 96)
            with torch.no_grad():
                assert torch.equal(hr, F.usm_sharpen(hr_p)) and not torch.equal(hr, hr_p)   # the plain crop, sharpened
            levels = lr.double() * 255
            assert float(lr.min()) >= 0 and float(lr.max()) <= 1 and float((levels - levels.round()).abs().max()) < 1e-4
            if degradation == 'bicubic':
                assert usm.last_degradation is None
                assert torch.equal(lr, bicubic_by_hand(hr, dev))
            else:
                _same_draws(usm.last_degradation, plain.last_degradation)                   # it consumed no random numbers
                by_hand = blind_by_hand if degradation == 'blind' else blind2_by_hand
                assert torch.equal(lr, by_hand(hr, usm.last_degradation, dev))
            assert not torch.equal(lr, lr_p)                                                # the degradation saw the sharpened crop
            batches += 1
    assert batches == 4
    # the test loader is untouched
    seen = 0
    for a, b in zip(usm_test, plain_test):
        assert len(a) == 3 and all(torch.equal(u, v) for u, v in zip(a, b))
        seen += 1
    assert seen == len(plain_test) >= 1


@pytest.mark.parametrize('degradation', ['bicubic', 'blind2'])
def test_gt_usm_false_changes_nothing(dev, image_dir, degradation):
    """``gt_usm=False`` and a loader built without the argument: the same bits, train and test."""
    for off, default in zip(_loaders(image_dir, dev, degradation, gt_usm=False), _loaders(image_dir, dev, degradation)):
        n = 0
        for _ in range(2):
            for a, b in zip(off, default):
                assert len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))
                n += 1
        assert n == 2 * len(default)


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_gt_usm_cli(dev, image_dir, tmp_path, monkeypatch):
    """The command of test_blind2_degradation_cli with ``--gt-usm``: one pre-training and one GAN epoch."""
    from torchsr_amd.torchsr import main
    monkeypatch.chdir(tmp_path)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'LOCAL_WORLD_SIZE', 'SLURM_NTASKS'):
        monkeypatch.delenv(k, raising=False)
    main(['train', '--model', 'srgan', '--train-dir', image_dir, '--batch-size', '4', '--epochs', '1',
          '--pretrain-epochs', '1', '--disable-amp', '--seed', '5', '--device-data', '--skip-image-save',
          '--vgg-weights', 'random', '--degradation', 'blind2', '--gt-usm'])
    assert os.path.exists('srgan-gan-latest.pth')
    ckpt = torch.load('srgan-gan-latest.pth', map_location='cpu')
    assert all(torch.isfinite(v).all() for v in ckpt['state'].values() if v.is_floating_point())
