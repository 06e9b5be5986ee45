"""``--degradation blind`` on the GPU: ``srx_blur_aniso``, ``srx_add_gaussian_noise`` and ``srx_jpeg_sim`` against their
float64 restatements (degrade_ref.py) with derived bounds, the real JPEG codec, ``functional``'s launchers of the data path
against the raw calls, the ``blind`` DeviceLoader against the four ABI calls made by hand (degrade_chain.py) and against the
``bicubic`` loader, and the CLI."""
import os

import numpy as np
import pytest
import torch

import degrade_ref as R
from degrade_chain import bicubic_by_hand, blind_by_hand, write_images
from guarded import _band_kept, _guarded, _stream

pytestmark = pytest.mark.gpu


def gpu_blur(x, parm, ksize, dev):
    from torchsr_amd import _lib
    n, c, h, w = x.shape
    xd = x.to(dev).contiguous()
    pd = torch.tensor(parm, dtype=torch.float32).reshape(n, 4).to(dev)
    kd = torch.tensor(ksize, dtype=torch.int32).to(dev)
    buf, out = _guarded(x.shape, dev)
    _lib.call('srx_blur_aniso', xd.data_ptr(), out.data_ptr(), pd.data_ptr(), kd.data_ptr(), n, c, h, w, _stream())
    torch.cuda.synchronize()
    assert _band_kept(buf)
    return out.cpu()


def gpu_noise(x, sigma, gray, seed, quantize, dev):
    from torchsr_amd import _lib
    n, _, h, w = x.shape
    xd = x.to(dev).contiguous()
    sd = torch.tensor(sigma, dtype=torch.float32).to(dev)
    gd = torch.tensor(gray, dtype=torch.int32).to(dev)
    buf, out = _guarded(x.shape, dev)
    _lib.call('srx_add_gaussian_noise', xd.data_ptr(), out.data_ptr(), sd.data_ptr(), gd.data_ptr(), seed & 0xFFFFFFFF,
              seed >> 32, n, h, w, quantize, _stream())
    torch.cuda.synchronize()
    assert _band_kept(buf)
    return out.cpu()


def gpu_jpeg(x, quality, quantize, dev):
    from torchsr_amd import _lib
    n, _, h, w = x.shape
    xd = x.to(dev).contiguous()
    qd = torch.tensor(quality, dtype=torch.int32).to(dev)
    buf, out = _guarded(x.shape, dev)
    _lib.call('srx_jpeg_sim', xd.data_ptr(), out.data_ptr(), qd.data_ptr(), n, h, w, quantize, _stream())
    torch.cuda.synchronize()
    assert _band_kept(buf)
    return out.cpu()


# ---------------------------------------------------------------------------------------------------------------- blur
# max |err| <= 3e-5: 441 products and sums in fp32 on weights that are positive and sum to 1 and inputs in [0, 1] give
# 443 * 2^-24 = 2.7e-5; the rounding of the weights themselves (expf, one division) adds under 1e-6
BLUR_TOL = 3e-5
ORIENTED = (3.0, 0.5, 0.6, 0.0)  # sigma_x, sigma_y, theta: a kernel that is neither symmetric in x <-> y nor in theta <-> -theta

BLUR_CASES = {
    # the smallest legal plane: every output touches reflected taps on both sides
    'smallest-plane-21-taps': ((2, 3, 11, 13), [ORIENTED, (1.7, 1.7, 0.0, 0.0)], [21, 21]),
    # per-sample sizes, a sample that is copied, tiles that are not whole (24 x 40 in 32 x 32 tiles)
    'per-sample-sizes-and-a-copy': ((3, 3, 24, 40), [(0.4, 2.5, -2.0, 0.0), ORIENTED, ORIENTED], [7, 0, 13]),
    # the training crop: nine whole tiles, interior tiles without a reflected tap
    'crop-96-21-taps': ((2, 3, 96, 96), [(2.9, 1.1, 2.4, 0.0), ORIENTED], [21, 21]),
}


@pytest.mark.parametrize('case', list(BLUR_CASES))
def test_blur_against_float64(dev, case):
    shape, parm, ksize = BLUR_CASES[case]
    x = torch.rand(shape, generator=torch.Generator().manual_seed(len(case)))
    want = R.blur(x, parm, ksize)
    # the reference can tell a transposed or mirrored kernel from the right one, by far more than the tolerance
    for n, p in enumerate(parm):
        if p == ORIENTED and ksize[n]:
            swapped = [q if i != n else (p[1], p[0], p[2], 0.0) for i, q in enumerate(parm)]
            mirrored = [q if i != n else (p[0], p[1], -p[2], 0.0) for i, q in enumerate(parm)]
            for wrong in (swapped, mirrored):
                assert float((R.blur(x, wrong, ksize)[n] - want[n]).abs().max()) > 100 * BLUR_TOL
    got = gpu_blur(x, parm, ksize, dev)
    err = float((got.double() - want).abs().max())
    print(f'{case}: max |err| = {err:.3e} (bound {BLUR_TOL:.0e})')
    assert err <= BLUR_TOL
    for n, k in enumerate(ksize):
        if k == 0:
            assert torch.equal(got[n], x[n])  # bit for bit


def test_blur_clamps_illegal_sizes(dev):
    """The kernel size is read on the device: whatever it finds there is clamped to the legal set (<= 0 copies, even sizes go
    to the next odd one, more than 21 is 21) -- the restatement does the same."""
    x = torch.rand((5, 3, 16, 19), generator=torch.Generator().manual_seed(4))
    parm, ksize = [(1.5, 0.8, 0.3, 0.0)] * 5, [-7, 8, 22, 1 << 30, 1]
    got, want = gpu_blur(x, parm, ksize, dev), R.blur(x, parm, ksize)
    assert float((got.double() - want).abs().max()) <= BLUR_TOL
    assert torch.equal(got[0], x[0]) and torch.equal(got[4], x[4])  # no blur, and one tap of weight 1


# ---------------------------------------------------------------------------------------------------------------- noise
# |z| <= sqrt(-2 ln 2^-25) = 5.9 times an angle rounding of 2 pi 2^-24 is 2.4e-6; the tolerance is 4 x that
NOISE_TOL = 1e-5
SEED = 0x9E3779B97F4A7C15


@pytest.mark.parametrize('shape', [(2, 3, 5, 7), (4, 3, 24, 32)])
def test_noise_against_float64(dev, shape):
    n, _, h, w = shape
    gray = [i % 2 for i in range(n)]
    x = torch.zeros(shape)
    got = gpu_noise(x, [1.0] * n, gray, SEED, 0, dev)
    want = R.gaussian_z(n, h, w, SEED & 0xFFFFFFFF, SEED >> 32, gray)
    err = float(np.abs(got.double().numpy() - want).max())
    print(f'{shape}: max |z - z64| = {err:.3e} (bound {NOISE_TOL:.0e}), max |z| = {np.abs(want).max():.2f}')
    assert err <= NOISE_TOL
    for i in range(n):
        if gray[i]:
            assert torch.equal(got[i, 0], got[i, 1]) and torch.equal(got[i, 0], got[i, 2])
        else:
            assert not torch.equal(got[i, 0], got[i, 1]) and not torch.equal(got[i, 0], got[i, 2])
    assert torch.equal(got, gpu_noise(x, [1.0] * n, gray, SEED, 0, dev))            # the same seed: the same bits
    assert not torch.equal(got, gpu_noise(x, [1.0] * n, gray, SEED + 1, 0, dev))    # another low word
    assert not torch.equal(got, gpu_noise(x, [1.0] * n, gray, SEED + (1 << 32), 0, dev))  # another high word
    assert not torch.equal(got[0, 0], got[2 if n > 2 else 1, 0])                    # another sample index (same grey flag if n > 2)
    if n == 4:  # the moments of the 2 * 3 * 768 independent deviates of the two coloured samples
        z = got[0::2].double()
        assert abs(float(z.mean())) < 0.06 and abs(float(z.std()) - 1) < 0.05


def test_noise_quantised(dev):
    """An 8-bit valued image, sigma 1/255 and 30/255: equal to the restatement except where the float64 value before the
    rounding lies within 1e-3 of a half step (expected share 0.2 %, at most 1 %), where it may differ by one step."""
    shape = (4, 3, 24, 32)
    x = torch.from_numpy(R.jpeg_images(4, 24, 32, seed=9))
    sigma = np.array([1 / 255, 30 / 255, 30 / 255, 1 / 255], dtype=np.float32)
    gray = [0, 0, 1, 1]
    want, pre = R.add_gaussian_noise(x.numpy(), sigma, gray, SEED & 0xFFFFFFFF, SEED >> 32, 1)
    near = np.abs(pre - np.floor(pre) - 0.5) < 1e-3
    assert near.mean() <= 0.01
    got = gpu_noise(x, sigma.tolist(), gray, SEED, 1, dev).numpy()
    levels = got.astype(np.float64) * 255
    assert np.abs(levels - np.rint(levels)).max() < 1e-4 and got.min() >= 0 and got.max() <= 1   # 8-bit valued
    diff = np.rint(levels) - np.rint(want * 255)
    print(f'{shape}: {near.mean():.3%} of the pixels near a half step, {int((diff != 0).sum())} differ')
    assert (diff[~near] == 0).all() and np.abs(diff[near]).max(initial=0) <= 1
    assert (got == 0).any() or (got == 1).any()  # sigma = 30 / 255 on an image that reaches 0.9: the clamp is exercised


# ---------------------------------------------------------------------------------------------------------------- JPEG
JPEG_CASES = {(1, 3, 8, 8): [50], (2, 3, 16, 24): [0, 95], (10, 3, 24, 32): [0, 30, 49, 50, 75, 95, 30, 49, 75, 95]}
TIE_DELTA = 2e-4   # a block is tie-prone if one of its 192 values coefficient / step lies this near a half-integer
FP32_FACTOR = 8    # tolerance = 8 x the largest |float32 numpy restatement - float64| outside tie-prone blocks, on these inputs;
#                    measured: 3.1e-5, 3.7e-5 and 3.7e-5 grey levels for the three cases, so about 3e-4 / 255


@pytest.fixture(scope='module')
def jpeg_refs():
    """Per case: the images, the float64 result, the tie-prone blocks and the tolerance -- computed once, on the CPU."""
    refs = {}
    for shape, quality in JPEG_CASES.items():
        imgs = R.jpeg_images(shape[0], shape[2], shape[3], seed=0)
        o64, t = R.jpeg_sim(imgs, quality, 0)
        o32, _ = R.jpeg_sim(imgs, quality, 0, dtype=np.float32)
        ties = R.tie_prone_blocks(t, TIE_DELTA)
        coded = np.array([1 <= q <= 100 for q in quality])
        assert ties[coded].mean() <= 0.25  # on the reference alone, before any GPU result
        fp32_err = np.abs(R._blocks(o32.astype(np.float64) - o64)).max(axis=(1, 4, 5))[~ties].max()
        refs[shape] = imgs, o64, ties, FP32_FACTOR * fp32_err
    return refs


@pytest.mark.parametrize('shape', list(JPEG_CASES))
def test_jpeg_against_float64(dev, jpeg_refs, shape):
    imgs, want, ties, tol = jpeg_refs[shape]
    quality = JPEG_CASES[shape]
    got = gpu_jpeg(torch.from_numpy(imgs), quality, 0, dev).numpy()
    assert np.isfinite(got).all() and got.min() >= 0 and got.max() <= 1
    err = np.abs(R._blocks(got.astype(np.float64) - want)).max(axis=(1, 4, 5))  # per block [N][H/8][W/8]
    print(f'{shape}: {ties.mean():.1%} tie-prone blocks; elsewhere max |err| = {err[~ties].max() * 255:.2e} grey levels '
          f'(tolerance {tol * 255:.2e}); in tie-prone blocks {err[ties].max(initial=0) * 255:.2e}')
    assert err[~ties].max() <= tol
    for n, q in enumerate(quality):
        if not 1 <= q <= 100:
            assert np.array_equal(got[n], imgs[n])  # bit for bit


@pytest.mark.parametrize('shape', list(JPEG_CASES))
def test_jpeg_quantised_lies_near_the_real_codec(dev, shape):
    """The CPU test's ratio on the GPU result, factor 3 (fp32 ties fall differently): mse(PIL, source) >= 3 mse(result, PIL)."""
    quality = JPEG_CASES[shape]
    imgs = R.jpeg_images(shape[0], shape[2], shape[3], seed=0)
    got = gpu_jpeg(torch.from_numpy(imgs), quality, 1, dev).numpy()
    levels = got.astype(np.float64) * 255
    assert np.abs(levels - np.rint(levels)).max() < 1e-4 and got.min() >= 0 and got.max() <= 1
    for n, q in enumerate(quality):
        if 1 <= q <= 100:
            ratio = R.pil_ratio(got[n], imgs[n], q)
            print(f'{shape} sample {n} quality {q}: mse(PIL, source) / mse(result, PIL) = {ratio:.1f}')
            assert ratio >= 3.0
        else:
            assert np.array_equal(got[n], imgs[n])


def test_jpeg_quantised_at_the_cpu_tests_qualities(dev):
    """The same ratio on the CPU test's own images and qualities (24 x 32; 30, 50, 75, 90, 95), factor 3."""
    quality = [30, 50, 75, 90, 95] * 2
    imgs = R.jpeg_images(10, 24, 32, seed=21)
    got = gpu_jpeg(torch.from_numpy(imgs), quality, 1, dev).numpy()
    ratios = [R.pil_ratio(got[n], imgs[n], q) for n, q in enumerate(quality)]
    print('mse(PIL, source) / mse(result, PIL):', ' '.join(f'{q}: {r:.1f}' for q, r in zip(quality, ratios)))
    assert min(ratios) >= 3.0


# ---------------------------------------------------------------------------------------------------------------- functional
# The launchers of torchsr_amd.functional against the raw ABI call on the same inputs, bit for bit, at the smallest legal shapes.
def test_functional_blur_aniso(dev):
    from torchsr_amd import functional as F
    x = torch.rand((2, 3, 12, 16), generator=torch.Generator().manual_seed(1))     # more than 10 rows, not square
    parm, ksize = [ORIENTED, (1.7, 1.7, 0.0, 0.0)], [7, 21]
    got = F.blur_aniso(x.to(dev), torch.tensor(parm, dtype=torch.float32).to(dev), torch.tensor(ksize, dtype=torch.int32).to(dev))
    want = gpu_blur(x, parm, ksize, dev)
    assert torch.equal(got.cpu(), want) and not torch.equal(want, x)


@pytest.mark.parametrize('quantize', [False, True])
def test_functional_bicubic_down(dev, quantize):
    from torchsr_amd import _lib
    from torchsr_amd import functional as F
    x = torch.rand((2, 3, 32, 48), generator=torch.Generator().manual_seed(2)).to(dev)
    buf, want = _guarded((2, 3, 8, 12), dev)
    _lib.call('srx_bicubic_down', x.data_ptr(), want.data_ptr(), 2, 3, 32, 48, 4, int(quantize), _stream())
    got = F.bicubic_down(x, 4, quantize)
    torch.cuda.synchronize()
    assert _band_kept(buf) and got.shape == (2, 3, 8, 12) and torch.equal(got, want)
    levels = got.double() * 255
    assert (float((levels - levels.round()).abs().max()) < 1e-4) == quantize


def test_functional_add_gaussian_noise(dev):
    from torchsr_amd import functional as F
    assert SEED & 0xFFFFFFFF and SEED >> 32                                        # both halves of the key count
    x = torch.from_numpy(R.jpeg_images(2, 8, 16, seed=3))
    sigma, gray = [10 / 255, 25 / 255], [1, 0]                                     # one grey and one colour sample
    sd, gd = torch.tensor(sigma, dtype=torch.float32).to(dev), torch.tensor(gray, dtype=torch.int32).to(dev)
    quantised = F.add_gaussian_noise(x.to(dev), sd, gd, SEED)
    assert torch.equal(quantised.cpu(), gpu_noise(x, sigma, gray, SEED, 1, dev))
    raw = F.add_gaussian_noise(x.to(dev), sd, gd, SEED, quantize=False)
    assert torch.equal(raw.cpu(), gpu_noise(x, sigma, gray, SEED, 0, dev)) and not torch.equal(raw, quantised)
    assert not torch.equal(F.add_gaussian_noise(x.to(dev), sd, gd, SEED ^ (1 << 40)), quantised)


@pytest.mark.parametrize('shape', [(2, 3, 8, 16), (2, 3, 16, 8)])
def test_functional_jpeg_sim(dev, shape, monkeypatch):
    """``chroma420`` None: exactly one ``srx_jpeg_sim`` call; given -- all 0 or mixed -- ``srx_jpeg_sim2`` on a workspace of the
    size the library asks for."""
    from step_layers import record_op_calls
    from torchsr_amd import _lib
    from torchsr_amd import functional as F
    n, _, h, w = shape
    quality = [30, 95]
    x = torch.from_numpy(R.jpeg_images(n, h, w, seed=4))
    xd, qd = x.to(dev), torch.tensor(quality, dtype=torch.int32).to(dev)
    got = {}
    calls = record_op_calls(monkeypatch, lambda: got.update(plain=F.jpeg_sim(xd, qd)))
    assert calls == [('srx_jpeg_sim', (n, h, w, 1))]
    assert torch.equal(got['plain'].cpu(), gpu_jpeg(x, quality, 1, dev))
    assert torch.equal(F.jpeg_sim(xd, qd, quantize=False).cpu(), gpu_jpeg(x, quality, 0, dev))
    nbytes = _lib.call('srx_jpeg_sim2_workspace', n, h, w)
    for flags in ([0, 0], [0, 1]):
        fd = torch.tensor(flags, dtype=torch.int32).to(dev)
        calls = record_op_calls(monkeypatch, lambda: got.update(sub=F.jpeg_sim(xd, qd, fd)))
        assert [name for name, _ in calls] == ['srx_jpeg_sim2_workspace', 'srx_jpeg_sim2']
        buf, want = _guarded(shape, dev)
        wbuf, ws = _guarded((nbytes // 4,), dev)
        _lib.call('srx_jpeg_sim2', xd.data_ptr(), want.data_ptr(), qd.data_ptr(), fd.data_ptr(), n, h, w, 1, ws.data_ptr(), nbytes,
                  None, _stream())
        torch.cuda.synchronize()
        assert _band_kept(buf) and _band_kept(wbuf) and torch.equal(got['sub'], want)
        assert torch.equal(got['sub'], got['plain']) == (not any(flags))           # no flag set: srx_jpeg_sim's bits


def test_functional_crop_flip(dev):
    from torchsr_amd import _lib
    from torchsr_amd import functional as F
    g = torch.Generator().manual_seed(5)
    images = [torch.randint(0, 256, s, generator=g, dtype=torch.uint8).to(dev) for s in ((20, 31, 3), (40, 17, 3))]
    meta = [[20, 31, 3, 9, 1, 0], [40, 17, 24, 1, 0, 1]]                           # one flipped each way; the second crop ends at H
    ptrs = torch.tensor([im.data_ptr() for im in images], dtype=torch.int64).to(dev)
    meta_t = torch.tensor(meta, dtype=torch.int32).to(dev)
    buf, want = _guarded((2, 3, 16, 16), dev)
    _lib.call('srx_crop_flip_u8', ptrs.data_ptr(), meta_t.data_ptr(), want.data_ptr(), 2, 16, _stream())
    got = F.crop_flip(images, meta, 16)
    torch.cuda.synchronize()
    assert _band_kept(buf) and got.shape == (2, 3, 16, 16) and torch.equal(got, want)
    crop = images[0][3:19, 9:25].flip(1).permute(2, 0, 1)                          # hflip: the columns reversed
    assert torch.equal((got[0] * 255).round().to(torch.uint8), crop)
    assert torch.equal((got[1] * 255).round().to(torch.uint8), images[1][24:40, 1:17].flip(0).permute(2, 0, 1))


# ---------------------------------------------------------------------------------------------------------------- loader
@pytest.fixture(scope='module')
def image_dir(tmp_path_factory):
    return write_images(tmp_path_factory.mktemp('degrade') / 'imgs')


def _train_loader(image_dir, dev, degradation, seed=5):
    from torchsr_amd.dataset import initialize_device_datasets
    return initialize_device_datasets(image_dir, dev, batch_size=4, crop_size=96, seed=seed, degradation=degradation)[0]


def test_blind_loader(dev, image_dir):
    blind, twin, plain = (_train_loader(image_dir, dev, d) for d in ('blind', 'blind', 'bicubic'))
    assert len(blind) == 2 and plain.last_degradation is None
    seen = []
    for _ in range(2):  # epochs
        for (lr, hr), (lr2, hr2), (lr_p, hr_p) in zip(blind, twin, plain):
            assert lr.shape == (4, 3, 24, 24) and hr.shape == (4, 3, 96, 96)
            assert torch.equal(hr, hr_p) and not torch.equal(lr, lr_p)     # the target is never degraded
            assert torch.equal(lr, lr2) and torch.equal(hr, hr2)          # same seed: the same bits
            levels = lr.double() * 255
            assert float(lr.min()) >= 0 and float(lr.max()) <= 1 and float((levels - levels.round()).abs().max()) < 1e-4
            # the four ABI calls by hand with the parameters the loader kept (every stage does something: asserted there)
            deg = blind.last_degradation
            assert torch.equal(lr, blind_by_hand(hr, deg, dev))
            seen.append(deg['seed'])
    assert len(set(seen)) == 4  # a fresh noise seed per batch
    assert not any(torch.equal(x, y) for x, y in zip(next(iter(_train_loader(image_dir, dev, 'blind', seed=6))), (lr, hr)))


def test_bicubic_loader_did_not_move(dev, image_dir):
    """The default path: ``lr`` equals ``srx_crop_flip_u8`` + ``srx_bicubic_down(quantize=1)`` called by hand with the rows a
    twin loader's host side draws, bit for bit."""
    from torchsr_amd import _lib
    loader, twin = _train_loader(image_dir, dev, 'bicubic'), _train_loader(image_dir, dev, 'bicubic')
    s = _stream()
    batches = 0
    for (lr, hr), (idx, meta, deg) in zip(loader, twin._plan()):
        assert deg is None
        ptrs = torch.tensor([twin.images[i].data_ptr() for i in idx], dtype=torch.int64).to(dev)
        meta_t = torch.tensor(meta, dtype=torch.int32).to(dev)
        hr2 = torch.empty_like(hr)
        _lib.call('srx_crop_flip_u8', ptrs.data_ptr(), meta_t.data_ptr(), hr2.data_ptr(), 4, 96, s)
        assert torch.equal(hr, hr2) and torch.equal(lr, bicubic_by_hand(hr2, 4, dev))
        batches += 1
    assert batches == 2 and loader.last_degradation is None


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_blind_degradation_cli(dev, image_dir, tmp_path, monkeypatch):
    """The command of test_device_data_pipeline_cli plus ``--degradation blind``: one pre-training and one GAN epoch."""
    from torchsr_amd.torchsr import main
    monkeypatch.chdir(tmp_path)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'LOCAL_WORLD_SIZE', 'SLURM_NTASKS'):
        monkeypatch.delenv(k, raising=False)
    main(['train', '--model', 'srgan', '--train-dir', image_dir, '--batch-size', '4', '--epochs', '1',
          '--pretrain-epochs', '1', '--disable-amp', '--seed', '5', '--device-data', '--skip-image-save',
          '--vgg-weights', 'random', '--degradation', 'blind'])
    assert os.path.exists('srgan-gan-latest.pth')
    ckpt = torch.load('srgan-gan-latest.pth', map_location='cpu')
    assert all(torch.isfinite(v).all() for v in ckpt['state'].values() if v.is_floating_point())
