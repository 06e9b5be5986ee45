"""``--degradation blind`` without a GPU: the restatements the GPU tests compare against (Philox known answers, the JPEG
model against PIL's codec), the host-side parameter draw and its random streams, the CLI flag and the ABI's refusals."""
import math
import random

import numpy as np
import pytest
import torch

import degrade_ref as R


# ------------------------------------------------------------------------------------------------------- the restatements
def test_philox_restatement_known_answers():
    """Philox4x32-10 against the known-answer vectors of its authors' test suite (zeros, ones, digits of pi)."""
    cases = [((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
             ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')]
    for counter, key, want in cases:
        assert ' '.join('%08x' % int(v) for v in R.philox4x32_10(counter, key)) == want
    # vectorised over the counter, as the noise restatement uses it
    r = R.philox4x32_10((np.array([0, 1], dtype=np.uint64), 0, 0, 0), (0, 0))
    assert '%08x' % int(r[0][0]) == '6627e8d5' and int(r[0][1]) != int(r[0][0])


@pytest.mark.parametrize('quality', [30, 49, 50, 75, 95])
def test_jpeg_tables_are_the_codecs(quality):
    """The scaled Annex K tables equal those PIL's libjpeg writes into a file saved with this quality."""
    img = R.jpeg_images(1, 24, 32, seed=quality)[0]
    _, tables = R.pil_jpeg(np.rint(img * 255).astype(np.uint8), quality)
    luma, chroma = R.jpeg_tables(quality)
    assert (tables[0] == luma).all() and (tables[1] == chroma).all()


@pytest.mark.parametrize('quality', [30, 50, 75, 90, 95])
def test_jpeg_restatement_lies_near_the_real_codec(quality):
    """mse(PIL, source) >= 4 mse(restatement rounded to 8 bits, PIL) for every image: the model lies several times nearer to
    what libjpeg-turbo decodes than the compression moves the picture.  The rest (0.9 - 1.4 grey levels rms) is the codec's
    integer DCT and its rounding of the decoded samples.  Measured over 80 images per quality: smallest ratio 5.8 at 95,
    11.4 at 90, 15 - 19 at 30 .. 75."""
    imgs = R.jpeg_images(8, 24, 32, seed=1000 + quality)
    out, _ = R.jpeg_sim(imgs, [quality] * len(imgs), quantize=1)
    ratios = [R.pil_ratio(out[i], imgs[i], quality) for i in range(len(imgs))]
    print(f'quality {quality}: mse(PIL, source) / mse(restatement, PIL) = {min(ratios):.2f} .. {max(ratios):.2f}')
    assert min(ratios) >= 4.0, ratios


def test_jpeg_restatement_edges():
    """A quality outside 1..100 passes the sample through; quality 100 (all steps 1) leaves only the roundings of the colour
    conversion and of the coefficients, each uniform in half a unit: under one grey level rms."""
    imgs = R.jpeg_images(3, 16, 16, seed=3)
    out, t = R.jpeg_sim(imgs, [0, 101, 100], quantize=0)
    assert (out[0] == imgs[0]).all() and (out[1] == imgs[1]).all() and not t[:2].any()
    assert (R.jpeg_tables(100)[0] == 1).all() and np.sqrt(((out[2] - imgs[2]) ** 2).mean()) * 255 < 1.0


def test_blur_restatement_is_a_normalised_oriented_gaussian():
    w = R.blur_weights(3.0, 0.5, 0.6, 21)
    assert abs(float(w.sum()) - 1) < 1e-12 and w.argmax() == 10 * 21 + 10
    # the long axis points along (cos theta, sin theta) = (x, y): the tap at v = 4 (cos, sin) outweighs the one at 4 (-sin, cos)
    assert w[10 + 2, 10 + 3] > 10 * w[10 + 3, 10 - 2]
    assert torch.equal(R.blur_weights(1.3, 1.3, 0.0, 7), R.blur_weights(1.3, 1.3, 0.0, 7).T)
    assert [R.legal_ksize(k) for k in (-3, 0, 1, 6, 7, 20, 21, 22, 1000)] == [0, 0, 1, 7, 7, 21, 21, 21, 21]


# ------------------------------------------------------------------------------------------------------- the host-side draw
def _loader(degradation, seed=11, sizes=((120, 150), (97, 96), (200, 130), (96, 96), (140, 101)), batch=2, rank=0):
    from torchsr_amd.dataset import DeviceLoader
    images = [torch.zeros(h, w, 3, dtype=torch.uint8) for h, w in sizes]
    return DeviceLoader(images, torch.device('cpu'), batch, 96, 4, False, seed, 5, rank, 1, degradation=degradation)


def test_draw_degradation_ranges_and_branches():
    d = _loader('blind')._draw_degradation(10000)
    assert d['parm'].shape == (10000, 4) and d['parm'].dtype == np.float32
    assert all(d[k].shape == (10000,) and d[k].dtype == np.int32 for k in ('ksize', 'gray', 'quality'))
    assert d['sigma_n'].shape == (10000,) and d['sigma_n'].dtype == np.float32
    sx, sy, theta = d['parm'][:, 0], d['parm'][:, 1], d['parm'][:, 2]
    assert set(np.unique(d['ksize'])) == set(range(7, 22, 2))
    lo, hi = np.float32(0.2), np.float32(3.0)
    assert sx.min() >= lo and sx.max() <= hi and sy.min() >= lo and sy.max() <= hi
    assert theta.min() >= np.float32(-math.pi) and theta.max() <= np.float32(math.pi) and (d['parm'][:, 3] == 0).all()
    iso = (sx == sy) & (theta == 0)
    assert 0.45 < iso.mean() < 0.55 and (theta[~iso] != 0).all() and (theta[~iso] < 0).any() and (theta[~iso] > 0).any()
    assert d['sigma_n'].min() >= np.float32(1 / 255) and d['sigma_n'].max() <= np.float32(30 / 255)
    assert d['sigma_n'].min() < 2 / 255 and d['sigma_n'].max() > 29 / 255
    assert set(np.unique(d['gray'])) == {0, 1} and 0.35 < d['gray'].mean() < 0.45
    assert set(np.unique(d['quality'])) == set(range(30, 96))
    assert 0 <= d['seed'] < 2 ** 64


def test_draw_degradation_is_reproducible_and_per_rank():
    a, b, c, d = _loader('blind'), _loader('blind'), _loader('blind', seed=12), _loader('blind', rank=1)
    for _ in range(3):  # successive batches: equal between equal loaders, different from batch to batch
        da, db = a._draw_degradation(16), b._draw_degradation(16)
        assert all(np.array_equal(da[k], db[k]) for k in ('parm', 'ksize', 'sigma_n', 'gray', 'quality')) and da['seed'] == db['seed']
    first = _loader('blind')._draw_degradation(16)
    assert da['seed'] != first['seed'] and not np.array_equal(da['parm'], first['parm'])
    for other in (c, d):
        do = other._draw_degradation(16)
        assert do['seed'] != first['seed'] and not np.array_equal(do['parm'], first['parm'])


def test_crop_and_flip_stream_is_the_same_in_both_modes():
    """The first 50 (top, left, hflip, vflip) of a seed: equal between a ``bicubic`` and a ``blind`` loader, and equal to the
    draws of the loader before the flag existed (``random.Random(seed * 7919 + rank)``: two randints and two uniforms per
    sample, in the shuffled order) -- a ``bicubic`` loader consumes exactly those numbers and draws no degradation."""
    plain, blind = _loader('bicubic'), _loader('blind')
    rows = {}
    for name, loader in (('bicubic', plain), ('blind', blind)):
        got = []
        for _ in range(3):  # epochs: 25 samples, 12 batches of 2
            for idx, meta, deg in loader._plan():
                assert (deg is None) == (name == 'bicubic') and len(meta) == len(idx) == 2
                got += [tuple(m) for m in meta]
        rows[name] = got[:50]
    assert rows['bicubic'] == rows['blind'] and len(rows['bicubic']) == 50
    rng, want = random.Random(11 * 7919 + 0), []
    for epoch in range(3):
        order = list(plain.order)
        random.Random(epoch * 104729 + 17).shuffle(order)
        for i in order[:24]:
            h, w = plain.sizes[i]
            top, left = rng.randint(0, h - 96), rng.randint(0, w - 96)
            want.append((h, w, top, left, int(rng.random() < 0.5), int(rng.random() < 0.5)))
    assert rows['bicubic'] == want[:50]
    assert {r[4] for r in want} == {0, 1} and {r[5] for r in want} == {0, 1}
    # the degradation stream of the bicubic loader was never touched
    assert plain.deg_rng.getstate() == _loader('bicubic').deg_rng.getstate()
    assert blind.deg_rng.getstate() != plain.deg_rng.getstate()


def test_test_loader_stays_bicubic_and_bad_modes_are_refused():
    from torchsr_amd.dataset import DeviceLoader
    images = [torch.zeros(100, 100, 3, dtype=torch.uint8)] * 3
    test = DeviceLoader(images, torch.device('cpu'), 2, 96, 4, True, 3, degradation='blind')
    assert all(deg is None for _, _, deg in test._plan())
    with pytest.raises(ValueError, match='degradation'):
        DeviceLoader(images, torch.device('cpu'), 2, 96, 4, False, 3, degradation='sinc')
    with pytest.raises(ValueError, match='multiple of 8'):
        DeviceLoader(images, torch.device('cpu'), 2, 100, 4, False, 3, degradation='blind')
    import inspect
    from torchsr_amd.dataset import initialize_device_datasets
    for fn in (DeviceLoader.__init__, initialize_device_datasets):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == 'degradation' and last.default == 'bicubic'


# ------------------------------------------------------------------------------------------------------- the CLI
def test_cli_degradation_flag(capsys):
    from torchsr_amd.torchsr import parse_args
    assert parse_args(['train']).degradation == 'bicubic'
    assert parse_args(['train', '--device-data']).degradation == 'bicubic'
    assert parse_args(['train', '--device-data', '--degradation', 'blind']).degradation == 'blind'
    assert parse_args(['train', '--degradation', 'bicubic']).degradation == 'bicubic'
    with pytest.raises(SystemExit) as exc:
        parse_args(['train', '--degradation', 'blind'])
    assert exc.value.code == 2 and '--device-data' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(['train', '--device-data', '--degradation', 'sinc'])


# ------------------------------------------------------------------------------------------------------- the launchers
def _launcher_cases():
    """Per launcher of the device data path: legal arguments (on the CPU), and argument lists a ValueError refuses."""
    x = torch.zeros(2, 3, 16, 16)
    f, i = (lambda *s: torch.zeros(s)), (lambda *s: torch.zeros(s, dtype=torch.int32))
    return {
        'bicubic_down': ((x, 4, True), [(x[0], 4, True), (x, 0, True), (x, 1.5, True), (x, True, True)]),
        'blur_aniso': ((x, f(2, 4), i(2)), [(x[0], f(2, 4), i(2)), (x[:, :2], f(2, 4), i(2)), (x, f(2, 3), i(2)), (x, f(3, 4), i(2)),
                                            (x, f(2, 4), i(3)), (x, i(2, 4), i(2)), (x, f(2, 4), f(2)), (x, f(4, 2).t(), i(2))]),
        'filter2d': ((x, f(2, 21, 21), i(2), False), [(x[:, :1], f(2, 21, 21), i(2), False), (x, f(2, 7, 7), i(2), False),
                                                     (x, f(3, 2, 21, 21)[0, :, :, :20], i(2), False), (x, f(2, 21, 21), i(2, 1), False),
                                                     (x, f(2, 21, 21).double(), i(2), False)]),
        'add_gaussian_noise': ((x, f(2), i(2), 5), [(x[0], f(2), i(2), 5), (x, f(1), i(2), 5), (x, f(2), i(2, 2), 5), (x, f(2), f(2), 5),
                                                    (x, i(2), i(2), 5), (x, f(2), i(2), -1), (x, f(2), i(2), 1 << 64),
                                                    (x, f(2), i(2), 0.5), (x, f(2), i(2), True)]),
        'jpeg_sim': ((x, i(2), i(2)), [(x[:, :2], i(2)), (x, i(3)), (x, f(2)), (x, i(2), i(1)), (x, i(2), f(2)), (x, i(2, 2)[:, 0])]),
    }


@pytest.mark.parametrize('name', ['bicubic_down', 'blur_aniso', 'filter2d', 'add_gaussian_noise', 'jpeg_sim'])
def test_functional_launchers_check_arguments_before_the_device(name, monkeypatch):
    from torchsr_amd import functional as F
    monkeypatch.setattr(F, 'call', lambda *a: pytest.fail(f'{name} reached the library: {a[0]}'))
    fn, (ok, bad) = getattr(F, name), _launcher_cases()[name]
    for args in bad:
        with pytest.raises(ValueError, match=name):
            fn(*args)
    grad = (ok[0].clone().requires_grad_(),) + ok[1:]
    with pytest.raises(RuntimeError, match='no backward'):
        fn(*grad)
    with torch.no_grad(), pytest.raises(RuntimeError, match='no CPU fallback'):   # refused under grad mode only
        fn(*grad)
    with pytest.raises(RuntimeError, match='no CPU fallback'):   # legal arguments: the tensor's device is what is refused
        fn(*ok)


def test_functional_crop_flip_checks_arguments_before_the_device(monkeypatch):
    from torchsr_amd import functional as F
    monkeypatch.setattr(F, 'call', lambda *a: pytest.fail(f'crop_flip reached the library: {a[0]}'))
    images = [torch.zeros((20, 31, 3), dtype=torch.uint8), torch.zeros((40, 17, 3), dtype=torch.uint8)]
    meta = [[20, 31, 4, 15, 1, 0], [40, 17, 24, 1, 0, 1]]                   # both crops of 16 touch an edge of their image
    edit = lambda n, k, v: [row if j != n else row[:k] + [v] + row[k + 1:] for j, row in enumerate(meta)]  # noqa: E731
    for im, rows, crop in (([], [], 16), (images, meta[:1], 16), (images[:1], meta, 16), (images, [row[:5] for row in meta], 16),
                           (images, edit(0, 2, 5), 16), (images, edit(0, 2, -1), 16), (images, edit(1, 3, 2), 16), (images, meta, 18),
                           (images, edit(0, 0, 21), 16), (images, edit(1, 1, 16), 16), ([images[0], images[1].float()], meta, 16),
                           ([images[0], images[1].transpose(0, 1)], [meta[0], [17, 40, 1, 24, 0, 1]], 16)):   # not contiguous
        with pytest.raises(ValueError, match='crop_flip'):
            F.crop_flip(im, rows, crop)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.crop_flip(images, meta, 16)


# ------------------------------------------------------------------------------------------------------- the ABI
def test_abi_refuses_bad_degradation_arguments_without_a_gpu():
    """srx_blur_aniso / srx_add_gaussian_noise / srx_jpeg_sim refuse null pointers and the shapes their kernels are not
    written for with a status code BEFORE anything is launched -- so the checks run here, with fake pointers, on CPU."""
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

    def blur(i=fake, o=fake + 4096, p=fake, k=fake, n=2, c=3, h=96, w=96):
        return lib.srx_blur_aniso(i, o, p, k, n, c, h, w, None)

    def noise(i=fake, o=fake, s=fake, g=fake, n=2, h=24, w=24):
        return lib.srx_add_gaussian_noise(i, o, s, g, 1, 2, n, h, w, 1, None)

    def jpeg(i=fake, o=fake, q=fake, n=2, h=24, w=24):
        return lib.srx_jpeg_sim(i, o, q, n, h, w, 1, None)

    for arg in ('i', 'o', 'p', 'k'):
        assert blur(**{arg: None}) != 0 and 'null' in err(), arg
    for arg in ('i', 'o', 's', 'g'):
        assert noise(**{arg: None}) != 0 and 'null' in err(), arg
    for arg in ('i', 'o', 'q'):
        assert jpeg(**{arg: None}) != 0 and 'null' in err(), arg
    assert blur(o=fake) != 0 and 'must not be the input' in err()
    for bad in ({'n': 0}, {'n': -1}, {'n': 65536}, {'h': 0}, {'w': -5}):
        assert blur(**bad) != 0 and 'bad shape' in err(), bad
    for c in (0, 1, 2, 4, -3):
        assert blur(c=c) != 0 and '3 channels' in err(), c
    for bad in ({'h': 10}, {'w': 10}, {'h': 1, 'w': 1}):
        assert blur(**bad) != 0 and '11 rows' in err(), bad
    for bad in ({'n': 0}, {'h': 0}, {'w': -1}):
        assert noise(**bad) != 0 and 'bad shape' in err(), bad
        assert jpeg(**bad) != 0 and 'bad shape' in err(), bad
    assert noise(h=65536, w=65536) != 0 and 'too large' in err()
    for bad in ({'h': 12}, {'w': 12}, {'h': 7, 'w': 7}, {'h': 20, 'w': 24}):
        assert jpeg(**bad) != 0 and '8 x 8 blocks' in err(), bad
    assert jpeg(n=65536) != 0 and 'bad shape' in err()
