"""``--gt-usm`` on the GPU: ``srx_usm_sharpen`` against its float64 restatement (usm_ref.py) with the bounds of DESIGN.md,
'Sharpened targets', its exact identities, ``functional.usm_sharpen`` against the raw call, the ``gt_usm`` DeviceLoader against
the plain one and the chains of calls made by hand, and the CLI."""
import functools
import os

import numpy as np
import pytest
import torch

import usm_ref as U
from degrade_chain import bicubic_by_hand, blind2_by_hand, blind_by_hand, same_draws, write_images
from guarded import _band_kept, _guarded, _stream

pytestmark = pytest.mark.gpu


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
LOADER_SEED = 1


@pytest.fixture(scope='module')
def image_dir(tmp_path_factory):
    return write_images(tmp_path_factory.mktemp('usm') / 'imgs')


def _loaders(image_dir, dev, degradation, **kw):
    from torchsr_amd.dataset import initialize_device_datasets
    return initialize_device_datasets(image_dir, dev, batch_size=4, crop_size=96, seed=LOADER_SEED, degradation=degradation, **kw)[:2]


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
                assert torch.equal(lr, bicubic_by_hand(hr, 4, dev))
            else:
                same_draws(usm.last_degradation, plain.last_degradation)                   # it consumed no random numbers
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
