"""``--jpeg-420-prob`` on the GPU: ``srx_jpeg_sim2`` against its float64 restatement (jpeg420_ref.py), half by half with derived
bounds, against the real 4:2:0 codec and, bit for bit, against ``srx_jpeg_sim``; its refusals; the ``blind`` and ``blind2``
DeviceLoader with the flag; the pair pool; the command line."""
import os

import numpy as np
import pytest
import torch

import jpeg420_ref as J
from degrade_chain import blind2_by_hand, blind_by_hand, write_images
from guarded import _stream

pytestmark = pytest.mark.gpu

GUARD = 64  # floats of NaN on either side of every buffer the kernels write: a store outside it shows


def _guarded(n, dev, fill=float('nan')):
    buf = torch.full((GUARD + n + GUARD,), float('nan'), device=dev)
    buf[GUARD:GUARD + n] = fill
    return buf, buf[GUARD:GUARD + n]


def _band_kept(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def gpu_jpeg2(x, quality, flags, quantize, dev, ws_fill=float('nan'), with_quot=True):
    """``srx_jpeg_sim2`` on a batch: (out [N][3][H][W], quot [N][3][H W] or None), on the host.  The output, the workspace -- of
    exactly the size the library asks for, holding ``ws_fill`` (a float, or a tensor of that many floats) -- and ``quot_out``
    (zeros, so that what the kernel leaves untouched compares equal to the restatement's zeros) lie between NaN guards."""
    from torchsr_amd import _lib
    n, _, h, w = x.shape
    xd = torch.as_tensor(x).to(dev).contiguous()
    qd = torch.tensor(quality, dtype=torch.int32).to(dev)
    fd = torch.tensor(flags, dtype=torch.int32).to(dev)
    nbytes = _lib.call('srx_jpeg_sim2_workspace', n, h, w)
    assert nbytes == n * 2 * J.chroma_blocks(h) * 8 * J.chroma_blocks(w) * 8 * 4
    obuf, out = _guarded(xd.numel(), dev)
    wbuf, ws = _guarded(nbytes // 4, dev, ws_fill)
    qbuf, quot = _guarded(xd.numel(), dev, 0.0)
    _lib.call('srx_jpeg_sim2', xd.data_ptr(), out.data_ptr(), qd.data_ptr(), fd.data_ptr(), n, h, w, quantize, ws.data_ptr(),
              nbytes, quot.data_ptr() if with_quot else None, _stream())
    torch.cuda.synchronize()
    assert _band_kept(obuf) and _band_kept(wbuf) and _band_kept(qbuf)
    if not with_quot:
        assert not bool(quot.any())
    return out.view(x.shape).cpu().numpy(), quot.view(n, 3, h * w).cpu().numpy() if with_quot else None


def gpu_jpeg(x, quality, quantize, dev):
    from torchsr_amd import _lib
    n, _, h, w = x.shape
    xd = torch.as_tensor(x).to(dev).contiguous()
    qd = torch.tensor(quality, dtype=torch.int32).to(dev)
    out = torch.empty_like(xd)
    _lib.call('srx_jpeg_sim', xd.data_ptr(), out.data_ptr(), qd.data_ptr(), n, h, w, quantize, _stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- the kernel
SHAPES = [(8, 8), (16, 16), (24, 40), (32, 48)]   # one block; one whole MCU; a partial MCU on both axes; several MCUs
QUALITY = [30, 0, 50, 75, 101, 95]                # N = 6: two samples are copied, one with its flag set
FLAGS = [1, 1, 0, 2, 0, -1]                       # any value but 0 is 4:2:0
FP32_FACTOR = 8
# Both tolerances are 8 x the largest |float32 numpy restatement - float64| of that half on these inputs (the rule of
# test_degrade_gpu.py), derived on the CPU before any GPU result is looked at.  The restatement's own distances, for the four
# shapes in order -- encode half, in quotients coefficient / step (up to 294 in size): 2.1e-5, 5.2e-5, 3.1e-5, 2.6e-5, so
# tolerances of 1.7e-4, 4.2e-4, 2.4e-4, 2.1e-4; decode half, in grey levels: 4.1e-5, 4.3e-5, 3.8e-5, 4.1e-5, so tolerances of
# 3.3e-4, 3.5e-4, 3.0e-4, 3.3e-4.  The kernel, measured on the MI355X: 2.1e-5, 5.2e-5, 3.1e-5,
# 2.6e-5 in quotients and 3.5e-5, 3.7e-5, 4.6e-5, 4.1e-5 grey levels.
# In the two larger cases a float64 quotient lies within 1e-15 of a half-integer (a chroma block whose coefficient is an exact
# multiple of half a step), which is why the decode half is fed the kernel's own rounding.


@pytest.fixture(scope='module')
def refs():
    """Per shape: the images, the float64 quotients with their tolerance, and the decode half's tolerance -- CPU only."""
    out = {}
    for h, w in SHAPES:
        imgs = J.jpeg_images(len(QUALITY), h, w, seed=h + w)
        q64 = J.encode(imgs, QUALITY, FLAGS)
        q32 = J.encode(imgs, QUALITY, FLAGS, dtype=np.float32)
        tol_q = FP32_FACTOR * np.abs(q32.astype(np.float64) - q64).max()
        d64 = J.decode(np.rint(q64), imgs, QUALITY, FLAGS, 0)
        d32 = J.decode(np.rint(q64), imgs, QUALITY, FLAGS, 0, dtype=np.float32)
        tol_d = FP32_FACTOR * np.abs(d32.astype(np.float64) - d64).max()
        assert 0 < tol_q < 2e-3 and 0 < tol_d * 255 < 2e-3           # far below half a quantiser step and half a grey level
        out[h, w] = imgs, q64, tol_q, tol_d
    return out


@pytest.fixture(scope='module')
def runs(dev, refs):
    """Per shape: the kernel's unquantised result and its quotients -- one call each, shared by the tests below."""
    return {s: gpu_jpeg2(refs[s][0], QUALITY, FLAGS, 0, dev) for s in SHAPES}


@pytest.mark.parametrize('shape', SHAPES)
def test_encode_half_against_float64(refs, runs, shape):
    """``quot_out`` equals the float64 quotients everywhere -- every block of every plane, the untouched words (zero) included."""
    _, q64, tol, _ = refs[shape]
    _, quot = runs[shape]
    err = np.abs(quot.astype(np.float64) - q64).max()
    print(f'{shape}: max |quot_out - float64| = {err:.2e} (tolerance {tol:.2e})')
    assert np.isfinite(quot).all() and err <= tol
    for n, q in enumerate(QUALITY):
        if not J.coded(q):
            assert not quot[n].any()


@pytest.mark.parametrize('shape', SHAPES)
def test_decode_half_against_float64(refs, runs, shape):
    """The kernel's RGB against the restatement's decode half fed the rounding of the kernel's OWN quotients: every pixel, no tie
    excluded.  The copied samples are the input's bits."""
    imgs, _, _, tol = refs[shape]
    got, quot = runs[shape]
    want = J.decode(np.rint(quot.astype(np.float64)), imgs, QUALITY, FLAGS, 0)
    err = np.abs(got.astype(np.float64) - want).max()
    print(f'{shape}: max |RGB - float64 decode of the kernel\'s quotients| = {err * 255:.2e} grey levels (tolerance {tol * 255:.2e})')
    assert np.isfinite(got).all() and got.min() >= 0 and got.max() <= 1 and err <= tol
    for n, q in enumerate(QUALITY):
        if not J.coded(q):
            assert np.array_equal(got[n], imgs[n])


@pytest.mark.parametrize('quantize', [0, 1])
@pytest.mark.parametrize('shape', SHAPES)
def test_flag_0_samples_are_srx_jpeg_sim_bit_for_bit(dev, refs, shape, quantize):
    imgs = refs[shape][0]
    got, _ = gpu_jpeg2(imgs, QUALITY, FLAGS, quantize, dev, with_quot=False)
    old = gpu_jpeg(imgs, QUALITY, quantize, dev)
    none, _ = gpu_jpeg2(imgs, QUALITY, [0] * len(QUALITY), quantize, dev)
    assert np.array_equal(none, old)                                     # no flag set: the whole batch
    for n, (q, f) in enumerate(zip(QUALITY, FLAGS)):
        if f == 0 or not J.coded(q):
            assert np.array_equal(got[n], old[n]), n
        else:
            assert not np.array_equal(got[n], old[n]), n                 # and 4:2:0 is something else


@pytest.mark.parametrize('shape', SHAPES)
def test_result_depends_on_nothing_but_its_arguments(dev, refs, runs, shape):
    """Two calls, a workspace that held NaN and one that held other garbage, ``quot_out`` given or null: the same bits."""
    imgs = refs[shape][0]
    first, quot = runs[shape]                                            # workspace of NaN, quot_out given
    again, quot2 = gpu_jpeg2(imgs, QUALITY, FLAGS, 0, dev)
    assert np.array_equal(first, again) and np.array_equal(quot, quot2)
    n_ws = len(QUALITY) * 2 * J.chroma_blocks(shape[0]) * 8 * J.chroma_blocks(shape[1]) * 8
    garbage = torch.from_numpy(np.random.RandomState(1).uniform(-1e30, 1e30, n_ws).astype(np.float32)).to(dev)
    other, quot3 = gpu_jpeg2(imgs, QUALITY, FLAGS, 0, dev, ws_fill=garbage)
    assert np.array_equal(first, other) and np.array_equal(quot, quot3)
    bare, _ = gpu_jpeg2(imgs, QUALITY, FLAGS, 0, dev, ws_fill=-7.0, with_quot=False)
    assert np.array_equal(first, bare)


def test_quantised_lies_near_the_real_420_codec(dev):
    """The CPU test's ratio on the GPU result with ``quantize=1``, on 24 x 32 images at the five qualities, factor 3 (fp32 ties
    fall differently): mse(PIL 4:2:0, source) >= 3 mse(result, PIL 4:2:0) -- the floor the 4:4:4 kernel is held to."""
    quality = [30, 50, 75, 90, 95] * 2
    imgs = J.jpeg_images(10, 24, 32, seed=21)
    got, _ = gpu_jpeg2(imgs, quality, [1] * 10, 1, dev, with_quot=False)
    levels = got.astype(np.float64) * 255
    assert np.abs(levels - np.rint(levels)).max() < 1e-4 and got.min() >= 0 and got.max() <= 1
    ratios = [J.pil_ratio420(got[n], imgs[n], q) for n, q in enumerate(quality)]
    print('mse(PIL 4:2:0, source) / mse(result, PIL 4:2:0):', ' '.join(f'{q}: {r:.1f}' for q, r in zip(quality, ratios)))
    assert min(ratios) >= 3.0


def test_refusals_launch_nothing(dev):
    """H = 12, a null pointer, a workspace one byte short: an error, and the output keeps what it held."""
    from torchsr_amd import _lib
    n, h, w = 2, 24, 40
    x = torch.from_numpy(J.jpeg_images(n, h, w, seed=2)).to(dev)
    q = torch.tensor([50, 75], dtype=torch.int32, device=dev)
    f = torch.tensor([1, 1], dtype=torch.int32, device=dev)
    nbytes = _lib.call('srx_jpeg_sim2_workspace', n, h, w)
    ws = torch.zeros(nbytes // 4, device=dev)
    out = torch.full_like(x, float('nan'))
    ok = dict(x=x.data_ptr(), out=out.data_ptr(), q=q.data_ptr(), f=f.data_ptr(), h=h, ws=ws.data_ptr(), nbytes=nbytes)

    def run(**kw):
        a = {**ok, **kw}
        _lib.call('srx_jpeg_sim2', a['x'], a['out'], a['q'], a['f'], n, a['h'], w, 1, a['ws'], a['nbytes'], None, _stream())

    for kw, word in ((dict(h=12), 'whole 8 x 8 blocks'), (dict(x=None), 'null pointer'), (dict(out=None), 'null pointer'),
                     (dict(q=None), 'null pointer'), (dict(f=None), 'null pointer'), (dict(ws=None), 'null pointer'),
                     (dict(nbytes=nbytes - 1), 'workspace')):
        with pytest.raises(RuntimeError, match=word):
            run(**kw)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and not bool(ws.any()), kw
    run()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())


# ---------------------------------------------------------------------------------------------------------------- loader
@pytest.fixture(scope='module')
def image_dir(tmp_path_factory):
    return write_images(tmp_path_factory.mktemp('jpeg420') / 'imgs')


def _train_loader(image_dir, dev, degradation, seed=5, **kw):
    from torchsr_amd.dataset import initialize_device_datasets
    return initialize_device_datasets(image_dir, dev, batch_size=4, crop_size=96, seed=seed, degradation=degradation, **kw)[0]


@pytest.mark.parametrize('degradation', ['blind', 'blind2'])
def test_loader(dev, image_dir, degradation):
    """Crop 96 / x4, batch 4.  Probability 0: the batches of a loader without the argument, bit for bit.  Probability 1: the same
    ``hr``, every flag set and another ``lr``, which is the chain of calls made by hand with the recorded parameters, bit for bit;
    for ``blind`` that ``lr`` is also the restatement of the chain's last step on what the first three kernels, called by hand,
    hand to it -- within the 8-bit step."""
    plain, off, one = (_train_loader(image_dir, dev, degradation, **kw) for kw in ({}, {'jpeg420_prob': 0.0}, {'jpeg420_prob': 1.0}))
    batches = 0
    for (lr_p, hr_p), (lr_0, hr_0), (lr_1, hr_1) in zip(plain, off, one):
        assert torch.equal(lr_p, lr_0) and torch.equal(hr_p, hr_0) and 'chroma420' not in off.last_degradation
        assert torch.equal(hr_1, hr_p) and not torch.equal(lr_1, lr_p)
        deg = one.last_degradation
        assert deg['chroma420'].dtype == np.int32 and deg['chroma420'].shape == deg['quality'].shape and (deg['chroma420'] == 1).all()
        assert np.array_equal(deg['quality'], plain.last_degradation['quality'])
        levels = lr_1.double() * 255
        assert lr_1.shape == (4, 3, 24, 24) and float(lr_1.min()) >= 0 and float(lr_1.max()) <= 1
        assert float((levels - levels.round()).abs().max()) < 1e-4
        if degradation == 'blind':
            _, _, c, d = blind_by_hand(hr_1, deg, dev, stages=True)
            assert torch.equal(lr_1, d)
            want, _ = J.jpeg420_sim(c.cpu().numpy(), deg['quality'], deg['chroma420'], 1)
            err = np.abs(lr_1.cpu().numpy().astype(np.float64) - want).max() * 255
            print(f'blind lr against the restatement on the kernel chain\'s input: {err:.3f} grey levels at most')
            assert err <= 1 + 1e-4
        else:
            assert torch.equal(lr_1, blind2_by_hand(hr_1, deg, dev))
        batches += 1
    assert batches == 2


def test_pair_pool_batches(dev, image_dir):
    """``--pair-pool`` composes: a pool of two batches fills, then exchanges; every batch is a clean 8-bit one."""
    loader = _train_loader(image_dir, dev, 'blind2', pair_pool=8, jpeg420_prob=1.0)
    seen = 0
    for _ in range(2):  # epochs: two stores, then two exchanges
        for lr, hr in loader:
            assert lr.shape == (4, 3, 24, 24) and hr.shape == (4, 3, 96, 96) and (loader.last_degradation['chroma420'] == 1).all()
            levels = lr.double() * 255
            assert bool(torch.isfinite(lr).all()) and float(lr.min()) >= 0 and float(lr.max()) <= 1
            assert float((levels - levels.round()).abs().max()) < 1e-4
            seen += 1
    assert seen == 4 and loader.pool_filled == 8


def test_jpeg_420_prob_cli(dev, image_dir, tmp_path, monkeypatch):
    """The command of test_device_data_pipeline_cli plus ``--degradation blind2 --jpeg-420-prob 1``: one pre-training and one GAN
    epoch."""
    from torchsr_amd.torchsr import main
    monkeypatch.chdir(tmp_path)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'LOCAL_WORLD_SIZE', 'SLURM_NTASKS'):
        monkeypatch.delenv(k, raising=False)
    main(['train', '--model', 'srgan', '--train-dir', image_dir, '--batch-size', '4', '--epochs', '1',
          '--pretrain-epochs', '1', '--disable-amp', '--seed', '5', '--device-data', '--skip-image-save',
          '--vgg-weights', 'random', '--degradation', 'blind2', '--jpeg-420-prob', '1'])
    assert os.path.exists('srgan-gan-latest.pth')
    ckpt = torch.load('srgan-gan-latest.pth', map_location='cpu')
    assert all(torch.isfinite(v).all() for v in ckpt['state'].values() if v.is_floating_point())
