"""``--poisson-noise-prob`` on the GPU: ``srx_add_poisson_noise`` against its restatement (poisson_ref.py) -- the level masks bit
for bit, every integer draw exactly, the result within the bound of its three fp32 roundings -- its copies, grey samples,
moments, determinism and ``quantize``; the ``poisson_prob`` DeviceLoader against the chain of calls made by hand; and the CLI."""
import functools
import os

import numpy as np
import pytest
import torch

import poisson_ref as P
from degrade_chain import blind2_by_hand, blind_by_hand, same_draws
from guarded import _stream

pytestmark = pytest.mark.gpu

GUARD = 64  # floats of NaN on either side of the output: a store outside the tensor shows


def gpu_poisson(x, scale, gray, seed, dev, quantize=0):
    """The raw ABI call on a NaN-guarded output and a guarded mask: ``(out, levels)`` as numpy arrays."""
    from torchsr_amd import _lib
    from torchsr_amd import functional as F
    xd = torch.as_tensor(np.asarray(x), dtype=torch.float32).to(dev).contiguous()
    n, _, h, w = xd.shape
    sd, gd = torch.as_tensor(np.asarray(scale), dtype=torch.float32).to(dev), torch.as_tensor(np.asarray(gray), dtype=torch.int32).to(dev)
    buf = torch.full((GUARD + xd.numel() + GUARD,), float('nan'), device=dev)
    out = buf[GUARD:GUARD + xd.numel()].view(xd.shape)
    lbuf = torch.full((8 + n * 8 + 8,), 0x5A5A5A5A, dtype=torch.int32, device=dev)   # stale words: the call must clear its part
    levels = lbuf[8:8 + n * 8].view(n, 8)
    _lib.call('srx_add_poisson_noise', xd.data_ptr(), out.data_ptr(), sd.data_ptr(), gd.data_ptr(), F.poisson_tables(dev).data_ptr(),
              levels.data_ptr(), seed & 0xFFFFFFFF, seed >> 32, n, h, w, quantize, _stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())
    assert bool((lbuf[:8] == 0x5A5A5A5A).all()) and bool((lbuf[-8:] == 0x5A5A5A5A).all())
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), np.asarray(x, dtype=np.float32).view(np.uint32))   # the input is untouched
    return out.cpu().numpy(), levels.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(case):
    """A case's inputs and restated results, computed once: ``(x, scale, gray, seed, masks, k, q, vals)``."""
    x, scale, gray, seed = P.level_images()[case]
    return (x, scale, gray, seed, P.level_masks(x, scale, gray)) + P.draws(x, scale, gray, seed)


@functools.lru_cache(maxsize=None)
def _device(case):
    x, scale, gray, seed = _reference(case)[:4]
    return gpu_poisson(x, scale, gray, seed, torch.device('cuda:0'))


CASES = list(P.level_images())


# ---------------------------------------------------------------------------------------------------------------- the operation
@pytest.mark.parametrize('case', CASES)
def test_levels_are_exact(dev, case):
    x, scale, gray, _, masks, _, _, vals = _reference(case)
    _, levels = _device(case)
    assert levels.dtype == np.int32 and np.array_equal(levels, masks)
    print(f'{case}: vals {vals.tolist()}, grey {np.asarray(gray).tolist()}')
    if case == 'constant-8x8':
        assert vals.tolist() == [1]
    if case == '128-and-129-levels':
        assert vals.tolist() == [128, 256]


@pytest.mark.parametrize('case', CASES)
def test_draws_are_exact(dev, case):
    x, scale, gray, _, _, k, q, vals = _reference(case)
    live = np.asarray(scale) != 0
    want, bound = P.result64(x, scale, k, q, vals), P.result_bound(x, scale, k, q, vals)
    # the recovery is unambiguous: an output within the bound moves the recovered value by far less than 1/2
    per_sample = (vals[live] / np.abs(np.asarray(scale, dtype=np.float64)[live]))[:, None, None, None]
    assert (bound[live] * per_sample).max() < 0.01 and np.array_equal(P.recover_k(want, x, scale, q, vals), k)
    out, _ = _device(case)
    assert not np.isnan(out).any()                                        # every element was written
    got = P.recover_k(out, x, scale, q, vals)
    assert np.array_equal(got, k), f'{int((got != k).sum())} of {k.size} draws differ'
    err = np.abs(out.astype(np.float64) - want)
    print(f'{case}: max |out err| = {err.max():.3e} (bound at that element {bound.reshape(-1)[err.argmax()]:.3e}, largest bound '
          f'{bound.max():.3e}); k up to {int(k.max())}, noise up to {np.abs(want - x).max():.3f}')
    assert (err <= bound).all()
    assert k[live].max() > 0 and np.abs(want - x)[live].max() > 1e3 * bound.max()   # the case adds noise


def test_copies_and_grey_samples(dev):
    x, scale, gray, _, _, k, q, vals = _reference('odd-17x29')
    out, _ = _device('odd-17x29')
    assert scale[2] == 0 and np.array_equal(out[2].view(np.uint32), x[2].view(np.uint32))           # a bit copy
    assert gray[1] == 1 and gray[0] == 0
    bound = P.result_bound(x, scale, k, q, vals)
    d = out.astype(np.float64) - x.astype(np.float64)
    spread = np.abs(d[1] - d[1][:1]).max()
    print(f'grey sample: channels\' out - in differ by at most {spread:.3e} (allowed {2 * bound[1].max():.3e}); colour sample: '
          f'{np.abs(d[0] - d[0][:1]).max():.3f}')
    assert (np.abs(d[1] - d[1][:1]) <= bound[1] + bound[1][:1]).all()                                # one k per pixel
    assert np.abs(d[0] - d[0][:1]).max() > 0.1                                                       # three in a colour sample
    # a NaN has level 0 and stays a NaN; negative zero and a copied sample's NaN pass through bit for bit
    y = x[:2].copy()
    y[0, 0, 0, 0], y[1, 1, 2, 3], y[1, 0, 0, 0] = np.nan, np.nan, -0.0
    out2, lv2 = gpu_poisson(y, [1.0, 0.0], [0, 0], 77, dev)
    assert np.isnan(out2[0, 0, 0, 0]) and np.array_equal(out2[1].view(np.uint32), y[1].view(np.uint32))
    assert np.array_equal(lv2, P.level_masks(y, [1.0, 0.0], [0, 0])) and (lv2[1] == 0).all()


def test_it_is_poisson(dev):
    """All 256 levels, 192 draws on each, vals 256: the pooled first two moments, which know nothing of the tables."""
    k_ref, q, vals = P.cycle_draws()
    z_mean, z_var, lam = P.moment_scores(k_ref, q)
    assert abs(z_mean) <= 3 and abs(z_var) <= 3                           # the restatement alone, for this seed
    x = P.cycle_image()
    out, levels = gpu_poisson(x, [1.0], [0], P.CYCLE_SEED, dev)
    assert (levels.view(np.uint32) == 0xFFFFFFFF).all()
    k = P.recover_k(out, x, [1.0], q, vals)
    g_mean, g_var, _ = P.moment_scores(k, q)
    print(f'mean of k - lambda: {g_mean:+.2f} standard errors (restatement {z_mean:+.2f}); mean of (k - lambda)^2 / lambda - 1: '
          f'{g_var:+.2f} (restatement {z_var:+.2f}); lambda up to {lam.max():.1f}, k up to {int(k.max())}')
    assert abs(g_mean) <= 5 and abs(g_var) <= 5
    assert np.array_equal(k, k_ref)


def test_determinism_and_seeds(dev):
    x, scale, gray, seed = _reference('odd-17x29')[:4]
    first, again = _device('odd-17x29'), gpu_poisson(x, scale, gray, seed, dev)
    assert np.array_equal(first[0].view(np.uint32), again[0].view(np.uint32)) and np.array_equal(first[1], again[1])
    other, lv = gpu_poisson(x, scale, gray, seed + 1, dev)
    assert np.array_equal(lv, first[1])                                   # the masks do not depend on the seed
    assert not np.array_equal(other[:2], first[0][:2]) and np.array_equal(other[2], first[0][2])
    hi, _ = gpu_poisson(x, scale, gray, seed ^ (1 << 40), dev)            # the upper key word counts
    assert not np.array_equal(hi[:2], first[0][:2])
    # not the Gaussian kernel's stream: with its counter (p, n, 0, 0) the restated draws differ nearly everywhere
    from degrade_ref import philox4x32_10
    n_s, _, h, w = x.shape
    p, n = np.arange(h * w, dtype=np.uint64)[None, :], np.arange(n_s, dtype=np.uint64)[:, None]
    theirs = np.stack(philox4x32_10((p, n, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))[:3], 1).reshape(n_s, 3, h, w)
    ours = P.words(n_s, h, w, seed)
    assert (theirs != ours).mean() > 0.99
    _, _, _, _, _, k, q, vals = _reference('odd-17x29')
    from torchsr_amd.degradation import poisson_thresholds
    t = poisson_thresholds(int(vals[0])).astype(np.int64)
    k_theirs = np.array([np.searchsorted(t[lv], u, side='right') for lv, u in zip(q[0].reshape(-1), (theirs[0] >> np.uint32(1)).reshape(-1).astype(np.int64))])
    assert (k_theirs != P.recover_k(first[0], x, scale, q, vals)[0].reshape(-1)).mean() > 0.5


def test_quantize(dev):
    x, scale, gray, seed, _, k, q, vals = _reference('128-and-129-levels')
    out, levels = gpu_poisson(x, scale, gray, seed, dev, quantize=1)
    assert np.array_equal(levels, _device('128-and-129-levels')[1])
    assert out.min() >= 0 and out.max() <= 1 and out.min() == 0 and out.max() == 1      # scales 2 and 3 reach both clamps
    lv = out.astype(np.float64) * 255
    assert np.abs(lv - np.rint(lv)).max() < 1e-4
    # the rounded value of the unquantised result, wherever that is not within its bound of a tie
    raw = _device('128-and-129-levels')[0].astype(np.float64)
    pre = np.clip(raw, 0, 1) * 255
    # (scale 2 on 128 levels puts every 64th k exactly on a tie: 255 * 2 k / 128 = 4 k - k / 64)
    decided = np.abs(pre - np.floor(pre) - 0.5) > 1e-3
    assert decided.mean() > 0.95 and np.array_equal(np.rint(lv)[decided], np.rint(pre)[decided])


def test_functional_add_poisson_noise(dev):
    from torchsr_amd import functional as F
    x, scale, gray, seed = _reference('odd-17x29')[:4]
    xd = torch.from_numpy(x).to(dev)
    raw_out, raw_levels = _device('odd-17x29')
    with torch.no_grad():
        out, levels = F.add_poisson_noise(xd, scale.tolist(), gray.tolist(), seed)
        out_t, _ = F.add_poisson_noise(xd, torch.from_numpy(scale).to(dev), torch.from_numpy(gray).to(dev), seed)
        out_q, _ = F.add_poisson_noise(xd, scale, gray, seed, quantize=True)
    assert out is not xd and torch.equal(xd.cpu(), torch.from_numpy(x)) and levels.dtype == torch.int32 and levels.shape == (3, 8)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), raw_out.view(np.uint32)) and torch.equal(out, out_t)
    assert np.array_equal(levels.cpu().numpy(), raw_levels)
    assert np.array_equal(out_q.cpu().numpy(), gpu_poisson(x, scale, gray, seed, dev, quantize=1)[0])
    tables = F.poisson_tables(dev)
    assert tables is F.poisson_tables(dev) and tables.dtype == torch.int32 and tables.is_cuda
    from torchsr_amd.degradation import poisson_table_words
    assert np.array_equal(tables.cpu().numpy(), poisson_table_words())
    with pytest.raises(RuntimeError, match='no backward'):
        F.add_poisson_noise(xd.clone().requires_grad_(), scale, gray, seed)
    with pytest.raises(ValueError):
        F.add_poisson_noise(xd, scale[:2], gray, seed)


# ---------------------------------------------------------------------------------------------------------------- loader
LOADER_SEED = 1


def _loaders(dev, degradation, **kw):
    from torchsr_amd.dataset import initialize_device_datasets
    return initialize_device_datasets('synthetic:16', dev, batch_size=4, crop_size=96, seed=LOADER_SEED, degradation=degradation, **kw)[:2]


@pytest.mark.parametrize('prob', [0.5, 1.0])
@pytest.mark.parametrize('degradation', ['blind', 'blind2'])
def test_poisson_loader(dev, degradation, prob):
    (noisy, noisy_test), (plain, plain_test) = _loaders(dev, degradation, poisson_prob=prob), _loaders(dev, degradation)
    assert noisy.poisson_prob == prob and plain.poisson_prob == 0.0 and noisy_test.poisson_prob == 0.0 and len(noisy) == 4
    by_hand = blind_by_hand if degradation == 'blind' else blind2_by_hand
    batches = chosen = differ = 0
    for (lr, hr), (lr_p, hr_p) in zip(noisy, plain):
        assert lr.shape == (4, 3, 24, 24) and torch.equal(hr, hr_p)        # the target is the plain loader's
        deg, deg_p = noisy.last_degradation, plain.last_degradation
        assert deg.keys() == deg_p.keys() | {'poisson_scale'}
        same_draws(deg, deg_p, but=('sigma_n', 'poisson_scale'))
        assert np.array_equal(deg['sigma_n'], np.where(deg['poisson_scale'] > 0, 0, deg_p['sigma_n']))
        assert torch.equal(lr, by_hand(hr, deg, dev))
        levels = lr.double() * 255
        assert float(lr.min()) >= 0 and float(lr.max()) <= 1 and float((levels - levels.round()).abs().max()) < 1e-4
        chosen += int((deg['poisson_scale'] > 0).sum())
        differ += int(not torch.equal(lr, lr_p))
        batches += 1
    stages = 1 if degradation == 'blind' else 2
    assert batches == 4 and differ >= 3 and (chosen == 16 * stages if prob == 1.0 else 0 < chosen < 16 * stages)
    seen = 0
    for a, b in zip(noisy_test, plain_test):                               # the test loader is untouched
        assert len(a) == 3 and all(torch.equal(u, v) for u, v in zip(a, b))
        seen += 1
    assert seen == len(plain_test) >= 1


@pytest.mark.parametrize('degradation', ['blind', 'blind2'])
def test_poisson_prob_zero_changes_nothing(dev, degradation, monkeypatch):
    """``poisson_prob=0``: the calls of a loader built without the argument -- no ``srx_add_poisson_noise`` -- and the same bits."""
    from step_layers import record_op_calls
    off, default = _loaders(dev, degradation, poisson_prob=0.0)[0], _loaders(dev, degradation)[0]
    assert off.poi_rng is None
    got, want = {}, {}
    calls_off = record_op_calls(monkeypatch, lambda: got.update(enumerate(off)))
    calls_default = record_op_calls(monkeypatch, lambda: want.update(enumerate(default)))
    names = [name for name, _ in calls_off]
    assert calls_off == calls_default and 'srx_add_poisson_noise' not in names
    assert names.count('srx_add_gaussian_noise') == 4 * (1 if degradation == 'blind' else 2) and names.count('srx_crop_flip_u8') == 4
    assert len(got) == len(want) == 4 and all(torch.equal(u, v) for i in got for u, v in zip(got[i], want[i]))
    assert 'poisson_scale' not in off.last_degradation
    # and with the flag the call is there, once per stage in which a sample drew Poisson
    on = _loaders(dev, degradation, poisson_prob=1.0)[0]
    names_on = [name for name, _ in record_op_calls(monkeypatch, lambda: [None for _ in on])]
    assert names_on.count('srx_add_poisson_noise') == names_on.count('srx_add_gaussian_noise') == names.count('srx_add_gaussian_noise')
    without = [name for name in names_on if name != 'srx_add_poisson_noise']
    assert without == names


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_poisson_noise_prob_cli(dev, tmp_path, monkeypatch):
    """The command of test_blind2_degradation_cli on synthetic images with ``--poisson-noise-prob 0.5``: one pre-training and one GAN
    epoch."""
    from torchsr_amd.torchsr import main
    monkeypatch.chdir(tmp_path)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'LOCAL_WORLD_SIZE', 'SLURM_NTASKS'):
        monkeypatch.delenv(k, raising=False)
    main(['train', '--model', 'srgan', '--train-dir', 'synthetic:16', '--batch-size', '4', '--epochs', '1',
          '--pretrain-epochs', '1', '--disable-amp', '--seed', '5', '--device-data', '--skip-image-save',
          '--vgg-weights', 'random', '--degradation', 'blind2', '--poisson-noise-prob', '0.5'])
    assert os.path.exists('srgan-gan-latest.pth')
    ckpt = torch.load('srgan-gan-latest.pth', map_location='cpu')
    assert all(torch.isfinite(v).all() for v in ckpt['state'].values() if v.is_floating_point())
