"""``--degradation blind2`` on the GPU: ``srx_filter2d`` against its float64 restatement (degrade2_ref.py) with derived bounds
and against ``srx_blur_aniso``, ``functional.resize`` against torch's ``interpolate`` in float64, the ``blind2`` DeviceLoader
against the chain of calls made by hand and against the ``bicubic`` loader, and the CLI."""
import math
import os

import numpy as np
import pytest
import torch

import degrade2_ref as R2
import degrade_ref as R
from degrade_chain import blind2_by_hand, write_images
from guarded import _band_kept, _guarded, _stream

pytestmark = pytest.mark.gpu


def gpu_filter(x, slots, ksize, quantize, dev):
    from torchsr_amd import _lib
    n, c, h, w = x.shape
    xd = torch.as_tensor(x, dtype=torch.float32).to(dev).contiguous()
    wd = torch.as_tensor(np.ascontiguousarray(slots), dtype=torch.float32).reshape(n, 21, 21).to(dev)
    kd = torch.tensor(ksize, dtype=torch.int32).to(dev)
    buf, out = _guarded(x.shape, dev)
    _lib.call('srx_filter2d', xd.data_ptr(), out.data_ptr(), wd.data_ptr(), kd.data_ptr(), n, c, h, w, quantize, _stream())
    torch.cuda.synchronize()
    assert _band_kept(buf)
    return out.cpu()


def _slots(names):
    from torchsr_amd.degradation import kernel_slot, kernel_weights
    make = {'sinc21': lambda: kernel_weights('sinc', 21, omega_c=math.pi), 'sinc7': lambda: kernel_weights('sinc', 7, omega_c=1.3),
            'plateau13': lambda: kernel_weights('plateau', 13, 2.6, 0.7, 0.6, beta=1.4), 'none': lambda: None}
    size = {'sinc21': 21, 'sinc7': 7, 'plateau13': 13, 'none': 0}
    return np.stack([kernel_slot(make[k]()) for k in names]), [size[k] for k in names]


# ---------------------------------------------------------------------------------------------------------------- filter2d
FILTER_CASES = {
    # the smallest legal plane: with 21 taps every read but the centre column's is reflected
    'smallest-plane': ((3, 3, 11, 11), ['sinc21', 'none', 'sinc7']),
    # one pixel past a 32 x 32 tile in both axes: four workgroups per plane, three of them nearly empty
    'one-past-a-tile': ((2, 3, 33, 37), ['plateau13', 'sinc21']),
    # the training crop: nine whole tiles; four different kernels in one batch, so a wrong sample index shows
    'crop-96': ((4, 3, 96, 96), ['sinc21', 'sinc7', 'plateau13', 'none']),
}


@pytest.mark.parametrize('case', list(FILTER_CASES))
def test_filter2d_against_float64(dev, case):
    shape, names = FILTER_CASES[case]
    slots, ksize = _slots(names)
    x = torch.rand(shape, generator=torch.Generator().manual_seed(len(case))).numpy()
    want = R2.filter2d(x, slots, ksize)
    tol = R2.filter2d_tolerance(slots, ksize, float(np.abs(x).max()))   # (ks^2 + 2) 2^-24 sum |w| max |x|, from the case's table
    # the reference tells a neighbouring sample's kernel from the right one by far more than the tolerance
    rolled = R2.filter2d(x, np.roll(slots, 1, axis=0), np.roll(ksize, 1))
    assert all(np.abs(rolled[n] - want[n]).max() > 100 * tol for n in range(shape[0]))
    got = gpu_filter(x, slots, ksize, 0, dev).numpy()
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f'{case}: max |err| = {err:.3e} (bound {tol:.3e}), overshoot: {want.min():.3f} .. {want.max():.3f}')
    assert err <= tol
    for n, k in enumerate(ksize):
        if k == 0:
            assert np.array_equal(got[n], x[n])  # bit for bit
    assert np.array_equal(got, gpu_filter(x, slots, ksize, 0, dev).numpy())   # no device state: the same bits again


# srx_blur_aniso's own bound against float64 (test_degrade_gpu.py): 443 * 2^-24 = 2.7e-5 for positive weights of sum 1 on [0, 1]
BLUR_TOL = 3e-5


def test_filter2d_with_gaussian_tables_is_blur_aniso(dev):
    """The fp32-rounded tables of ``blur_weights`` in ``srx_filter2d`` against ``srx_blur_aniso`` computing its own weights:
    each lies within BLUR_TOL of the float64 result, so they lie within twice that of each other."""
    from torchsr_amd import _lib
    from torchsr_amd.degradation import kernel_slot
    parm = [(3.0, 0.5, 0.6, 0.0), (1.7, 1.7, 0.0, 0.0), (0.4, 2.5, -2.0, 0.0)]
    ksize = [21, 7, 13]
    x = torch.rand((3, 3, 40, 45), generator=torch.Generator().manual_seed(8))
    slots = np.stack([kernel_slot(R.blur_weights(p[0], p[1], p[2], k).numpy()) for p, k in zip(parm, ksize)])
    got = gpu_filter(x.numpy(), slots, ksize, 0, dev)
    xd, pd, kd = x.to(dev), torch.tensor(parm, dtype=torch.float32).to(dev), torch.tensor(ksize, dtype=torch.int32).to(dev)
    blurred = torch.empty_like(xd)
    _lib.call('srx_blur_aniso', xd.data_ptr(), blurred.data_ptr(), pd.data_ptr(), kd.data_ptr(), 3, 3, 40, 45, _stream())
    diff = float((got - blurred.cpu()).abs().max())
    print(f'max |filter2d(gaussian tables) - blur_aniso| = {diff:.3e} (bound {2 * BLUR_TOL:.0e})')
    assert diff <= 2 * BLUR_TOL
    assert float((got.double() - R.blur(x, parm, ksize)).abs().max()) <= BLUR_TOL


def test_filter2d_copy_quantize_and_illegal_sizes(dev):
    slots, _ = _slots(['sinc21'] * 3)
    x = (torch.rand((3, 3, 17, 35), generator=torch.Generator().manual_seed(2)) * 2 - 0.5).numpy()   # values in [-0.5, 1.5)
    assert x.min() < -0.4 and x.max() > 1.4
    # ksize 0: a copy, bit for bit; with quantize the copy is clamped and rounded to 8 bits
    assert np.array_equal(gpu_filter(x, slots, [0, 0, 0], 0, dev).numpy(), x)
    q0 = gpu_filter(x, slots, [0, 0, 0], 1, dev).numpy()
    assert np.array_equal(q0, (np.rint(np.clip(x, 0, 1) * np.float32(255)) * np.float32(1 / 255)).astype(np.float32))
    # quantize = 1 after a filter: 8-bit valued in [0, 1], and the rounding of the unquantised result
    plain = gpu_filter(x, slots, [21, 7, 13], 0, dev).numpy()
    q = gpu_filter(x, slots, [21, 7, 13], 1, dev).numpy()
    levels = q.astype(np.float64) * 255
    assert q.min() >= 0 and q.max() <= 1 and np.abs(levels - np.rint(levels)).max() < 1e-4 and (q == 0).any() and (q == 1).any()
    assert np.array_equal(q, (np.rint(np.clip(plain, 0, 1) * np.float32(255)) * np.float32(1 / 255)).astype(np.float32))
    # the size is read on the device and clamped: -3, 4, 40 behave as 0, 5, 21 -- the same bits, and the restatement's values
    bad, legal = gpu_filter(x, slots, [-3, 4, 40], 0, dev).numpy(), gpu_filter(x, slots, [0, 5, 21], 0, dev).numpy()
    assert np.array_equal(bad, legal) and np.array_equal(bad[0], x[0])
    want = R2.filter2d(x, slots, [-3, 4, 40])
    assert np.abs(bad.astype(np.float64) - want).max() <= R2.filter2d_tolerance(slots, [0, 5, 21], float(np.abs(x).max()))
    assert np.abs(want[1] - x[1]).max() > 1e-2   # the unnormalised 5 x 5 window of the sinc did something


def test_filter2d_reads_only_the_centred_window(dev):
    slots, ksize = _slots(['sinc7', 'sinc7'])
    x = torch.rand((2, 3, 20, 33), generator=torch.Generator().manual_seed(6)).numpy()
    clean = gpu_filter(x, slots, ksize, 0, dev).numpy()
    dirty = np.full((2, 21, 21), 1e6, dtype=np.float32)
    dirty[1] = float('nan')
    dirty[:, 7:14, 7:14] = slots[:, 7:14, 7:14]
    assert np.array_equal(gpu_filter(x, dirty, ksize, 0, dev).numpy(), clean)
    assert np.abs(clean.astype(np.float64) - R2.filter2d(x, slots, ksize)).max() <= R2.filter2d_tolerance(slots, ksize, 1.0)


@pytest.mark.parametrize('quantize', [False, True])
def test_functional_filter2d(dev, quantize):
    """The launcher against the raw call, bit for bit: [2, 3, 12, 16] with sizes 7 and 21, then 21 and a copy."""
    from torchsr_amd import functional as F
    slots, _ = _slots(['sinc7', 'sinc21'])
    x = torch.rand((2, 3, 12, 16), generator=torch.Generator().manual_seed(3)).numpy()
    for ksize in ([7, 21], [21, 0]):
        got = F.filter2d(torch.from_numpy(x).to(dev), torch.from_numpy(slots).to(dev), torch.tensor(ksize, dtype=torch.int32).to(dev),
                         quantize)
        want = gpu_filter(x, slots, ksize, int(quantize), dev)
        assert torch.equal(got.cpu(), want) and not np.array_equal(want[0].numpy(), x[0])


# ---------------------------------------------------------------------------------------------------------------- resize
RESIZE_CASES = [((2, 3, 24, 40), (16, 56)), ((1, 3, 96, 96), (144, 16)), ((2, 3, 17, 11), (17, 11))]


@pytest.mark.parametrize('mode', R2.MODES)
@pytest.mark.parametrize('shape,size', RESIZE_CASES)
def test_resize_against_interpolate(dev, shape, size, mode):
    from torchsr_amd import functional as F
    x = torch.rand(shape, generator=torch.Generator().manual_seed(size[0]))
    want = R2.interpolate64(x.numpy(), size, mode)
    tol = R2.resize_tolerance(F.resize_tables(shape[2], size[0], mode), F.resize_tables(shape[3], size[1], mode), float(x.abs().max()))
    xd = x.to(dev)
    buf, out = _guarded(shape[:2] + size, dev)
    with torch.no_grad():
        got = F.resize(xd, size, mode, out=out)
        again = F.resize(xd, size, mode)
    torch.cuda.synchronize()
    assert got is out and _band_kept(buf) and tuple(again.shape) == shape[:2] + size
    err = float(np.abs(got.cpu().double().numpy() - want).max())
    print(f'{shape} -> {size} {mode}: max |err| = {err:.3e} (bound {tol:.3e})')
    assert err <= tol
    assert torch.equal(got, again)   # two calls: equal bits
    if size == shape[2:]:
        assert again is xd and torch.equal(got, xd)


# ---------------------------------------------------------------------------------------------------------------- loader
# chosen on the CPU (the draw is host-only): the smallest seed whose six batches of three epochs hold everything below
LOADER_SEED = 1


@pytest.fixture(scope='module')
def image_dir(tmp_path_factory):
    return write_images(tmp_path_factory.mktemp('degrade2') / 'imgs')


def _train_loader(image_dir, dev, degradation, seed=LOADER_SEED):
    from torchsr_amd.dataset import initialize_device_datasets
    return initialize_device_datasets(image_dir, dev, batch_size=4, crop_size=96, seed=seed, degradation=degradation)[0]


def test_blind2_loader(dev, image_dir):
    blind2, twin, plain = (_train_loader(image_dir, dev, d) for d in ('blind2', 'blind2', 'bicubic'))
    assert len(blind2) == 2 and plain.last_degradation is None
    seen = []
    for _ in range(3):  # epochs
        for (lr, hr), (lr2, hr2), (lr_p, hr_p) in zip(blind2, twin, plain):
            assert lr.shape == (4, 3, 24, 24) and hr.shape == (4, 3, 96, 96)
            assert torch.equal(hr, hr_p) and not torch.equal(lr, lr_p)     # the target is never degraded
            assert torch.equal(lr, lr2) and torch.equal(hr, hr2)          # same seed: the same bits
            levels = lr.double() * 255
            assert float(lr.min()) >= 0 and float(lr.max()) <= 1 and float((levels - levels.round()).abs().max()) < 1e-4
            deg = blind2.last_degradation
            assert torch.equal(lr, blind2_by_hand(hr, deg, dev))
            seen.append(deg)
    # what the seed was chosen for -- a changed draw order is noticed here
    assert len(seen) == 6 and {d['order'] for d in seen} == {'A', 'B'}
    assert any(d['sizes'][0] > 96 for d in seen) and any(d['sizes'][0] < 96 for d in seen)
    assert any('sinc' in d['kinds'][0] + d['kinds'][1] for d in seen)
    assert any('skip' in d['kinds'][1] and 0 in d['ksize'][1] for d in seen)
    assert any('pulse' in d['kinds'][2] and 0 in d['ksize'][2] for d in seen)
    assert len({d['seed1'] for d in seen} | {d['seed2'] for d in seen}) == 12   # fresh noise seeds per batch and pass
    other = next(iter(_train_loader(image_dir, dev, 'blind2', seed=LOADER_SEED + 1)))
    assert not any(torch.equal(x, y) for x, y in zip(other, (lr, hr)))


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_blind2_degradation_cli(dev, image_dir, tmp_path, monkeypatch):
    """The command of test_blind_degradation_cli with ``--degradation blind2``: one pre-training and one GAN epoch."""
    from torchsr_amd.torchsr import main
    monkeypatch.chdir(tmp_path)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'LOCAL_WORLD_SIZE', 'SLURM_NTASKS'):
        monkeypatch.delenv(k, raising=False)
    main(['train', '--model', 'srgan', '--train-dir', image_dir, '--batch-size', '4', '--epochs', '1',
          '--pretrain-epochs', '1', '--disable-amp', '--seed', '5', '--device-data', '--skip-image-save',
          '--vgg-weights', 'random', '--degradation', 'blind2'])
    assert os.path.exists('srgan-gan-latest.pth')
    ckpt = torch.load('srgan-gan-latest.pth', map_location='cpu')
    assert all(torch.isfinite(v).all() for v in ckpt['state'].values() if v.is_floating_point())
