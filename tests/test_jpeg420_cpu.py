"""``--jpeg-420-prob`` without a GPU: the 4:2:0 restatement (jpeg420_ref.py) against the real codec and against the 4:4:4 model,
its edge cases, the loader's fifth random stream, the CLI flag's and the loader's refusals, and the ABI's refusals."""
import numpy as np
import pytest
import torch

import degrade_ref as R
import jpeg420_ref as J

QUALITIES = (30, 50, 75, 90, 95)


# ------------------------------------------------------------------------------------------------------- the real codec
@pytest.mark.parametrize('quality', QUALITIES)
@pytest.mark.parametrize('size', [(24, 32), (40, 56)])
def test_restatement_lies_near_the_real_codec_and_the_444_model_does_not(size, quality):
    """Against PIL's file saved with subsampling=2, for each of 40 images: the 4:2:0 restatement rounded to 8 bits scores
    mse(PIL, source) / mse(result, PIL) >= 4, the floor the 4:4:4 restatement is held to against its own file, and today's
    4:4:4 ``jpeg_sim`` scores below it; the chrominance table in the file is ``jpeg_tables``'."""
    imgs = J.jpeg_images(40, size[0], size[1], seed=quality)
    out, _ = J.jpeg420_sim(imgs, [quality] * 40, [1] * 40, quantize=1)
    old, _ = R.jpeg_sim(imgs, [quality] * 40, quantize=1)
    ratios, old_ratios = [], []
    for i in range(40):
        pil, tables = J.pil_jpeg420(np.rint(imgs[i] * 255).astype(np.uint8), quality)
        luma, chroma = J.jpeg_tables(quality)
        assert (tables[0] == luma).all() and (tables[1] == chroma).all()
        ratios.append(J.pil_ratio420(out[i], imgs[i], quality, pil))
        old_ratios.append(J.pil_ratio420(old[i], imgs[i], quality, pil))
    print(f'{size[0]} x {size[1]} quality {quality}: mse(PIL 4:2:0, source) / mse(result, PIL 4:2:0) = {min(ratios):.1f} .. '
          f'{max(ratios):.1f} for the 4:2:0 restatement, {min(old_ratios):.2f} .. {max(old_ratios):.2f} for the 4:4:4 one')
    assert min(ratios) >= 4.0, ratios
    assert all(o < r for o, r in zip(old_ratios, ratios))


# ------------------------------------------------------------------------------------------------------- edge cases
def test_an_8x8_image_has_one_padded_chroma_block():
    """H = W = 8: the chroma plane is 4 x 4, replicated to one 8 x 8 block; the result is built from its 4 x 4 samples alone."""
    img = J.jpeg_images(1, 8, 8, seed=3)
    out, quot = J.jpeg420_sim(img, [75], [1], quantize=0)
    assert J.chroma_blocks(8) == 1 and quot.shape == (1, 3, 64) and np.isfinite(out).all() and out.shape == img.shape
    small = J.downsample(J.ycc_levels(img[0])[1:])
    assert small.shape == (2, 4, 4)
    padded = J.pad_edge(small)
    assert padded.shape == (2, 8, 8) and (padded[:, :4, :4] == small).all()
    assert (padded[:, 4:, :4] == small[:, 3:, :]).all() and (padded[:, :, 4:] == padded[:, :, 3:4]).all()
    # the quotients are those of the padded block, by the DCT written out as a sum
    k = np.arange(8)
    basis = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * np.where(k == 0, np.sqrt(1 / 8), 0.5)[:, None]  # [freq][sample]
    want = np.einsum('um,pmn,vn->puv', basis, padded - 128.0, basis) / J.jpeg_tables(75)[1]
    assert np.abs(quot[0, 1:].reshape(2, 8, 8) - want).max() < 1e-9
    # the decoder reads the 4 x 4 plane only: the corner pixels carry the corner samples themselves
    dec = J.decode_ycc(np.rint(quot[0]), 8, 8, 75, 1)
    d = J.dct_matrix()
    plane = (d.T @ (np.rint(quot[0, 1:].reshape(2, 8, 8)) * J.jpeg_tables(75)[1]) @ d)[:, :4, :4]
    assert np.abs(dec[1:, 0, 0] - plane[:, 0, 0]).max() < 1e-12 and np.abs(dec[1:, 7, 7] - plane[:, 3, 3]).max() < 1e-12
    assert np.abs(dec[1:, 7, 0] - plane[:, 3, 0]).max() < 1e-12
    assert np.abs(dec[1:, 1, 1] - (9 * plane[:, 0, 0] + 3 * plane[:, 1, 0] + 3 * plane[:, 0, 1] + plane[:, 1, 1]) / 16).max() < 1e-12


@pytest.mark.parametrize('size', [(24, 40), (32, 48), (8, 8)])
@pytest.mark.parametrize('quality', [30, 75, 95])
def test_a_picture_constant_per_mcu_keeps_its_chroma(size, quality):
    """Every 16 x 16 MCU, the partial ones at the right and bottom too, holds one colour.  Its chroma blocks are then constant
    -- a partial MCU's because its padding replicates -- so only their DC is coded: the decoded chroma planes miss the source's by
    at most the DC's quantisation, step / 2 in the coefficient = step / 16 in every sample, and so does every pixel whose
    four upsampling taps lie in its own MCU (all but the ring of one pixel along the MCU borders inside the image)."""
    h, w = size
    rng = np.random.RandomState(quality)
    colours = rng.randint(0, 256, (3, J.chroma_blocks(h), J.chroma_blocks(w)))
    img = (np.kron(colours, np.ones((16, 16)))[:, :h, :w] / 255).astype(np.float32)[None]
    _, quot = J.jpeg420_sim(img, [quality], [1], quantize=0)
    blocks = quot[0, 1:, :J.chroma_blocks(h) * J.chroma_blocks(w) * 64].reshape(2, -1, 64)
    assert np.abs(blocks[:, :, 1:]).max() < 1e-9                       # no AC: zero padding would put some here
    dec = J.decode_ycc(np.rint(quot[0]), h, w, quality, 1)
    src = J.ycc_levels(img[0]) - 128.0
    bound = J.jpeg_tables(quality)[1][0, 0] / 16 + 1e-9
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    ring = ((y % 16 == 0) & (y > 0)) | ((y % 16 == 15) & (y < h - 1)) | ((x % 16 == 0) & (x > 0)) | ((x % 16 == 15) & (x < w - 1))
    err = np.abs(dec[1:] - src[1:])
    print(f'{h} x {w} quality {quality}: chroma error {err[:, ~ring].max():.3f} inside the MCUs (bound {bound:.3f}), '
          f'{err[:, ring].max(initial=0):.3f} on their borders')
    assert err[:, ~ring].max() <= bound


def test_flags_0_and_pass_through_qualities():
    """All flags 0: ``jpeg_sim``, exactly, quotients included.  Qualities 0 and 101 copy the sample whatever its flag."""
    imgs = J.jpeg_images(4, 24, 40, seed=7)
    quality = [30, 50, 75, 95]
    for quantize in (0, 1):
        out, quot = J.jpeg420_sim(imgs, quality, [0] * 4, quantize)
        want, t = R.jpeg_sim(imgs, quality, quantize)
        assert np.array_equal(out, want) and np.array_equal(quot, t.reshape(4, 3, -1))
    out, quot = J.jpeg420_sim(imgs, [0, 101, 0, 101], [1, 1, 0, 0], 1)
    assert np.array_equal(out, imgs) and not quot.any()
    mixed, _ = J.jpeg420_sim(imgs, quality, [0, 1, 0, 1], 0)
    want, _ = R.jpeg_sim(imgs, quality, 0)
    assert np.array_equal(mixed[0], want[0]) and np.array_equal(mixed[2], want[2])
    assert not np.array_equal(mixed[1], want[1]) and not np.array_equal(mixed[3], want[3])


def test_upsample_is_the_triangle_filter():
    p = np.arange(12, dtype=np.float64).reshape(3, 4) ** 2
    up = J.upsample(p)
    assert up.shape == (6, 8)
    far = lambda i, n: min(max(i // 2 + (1 if i & 1 else -1), 0), n - 1)  # noqa: E731
    rows = np.stack([(3 * p[i // 2] + p[far(i, 3)]) / 4 for i in range(6)])               # the vertical pass alone
    want = np.stack([(3 * rows[:, j // 2] + rows[:, far(j, 4)]) / 4 for j in range(8)], axis=1)
    assert np.abs(up - want).max() < 1e-12
    assert np.abs(J.upsample(np.full((2, 5, 3), 7.0)) - 7.0).max() == 0     # the weights sum to one
    assert np.array_equal(J.downsample(np.array([[1, 2, 3, 3], [2, 2, 3, 4]])), np.array([[2, 3]]))  # (7 + 1) >> 2, (13 + 2) >> 2


# ------------------------------------------------------------------------------------------------------- the CLI
def test_cli_jpeg_420_prob_flag(capsys):
    from torchsr_amd.torchsr import parse_args
    assert parse_args(['train']).jpeg_420_prob == 0.0
    assert parse_args(['train', '--device-data', '--degradation', 'blind', '--jpeg-420-prob', '0.5']).jpeg_420_prob == 0.5
    assert parse_args(['train', '--device-data', '--degradation', 'blind2', '--jpeg-420-prob', '1']).jpeg_420_prob == 1.0
    assert parse_args(['train', '--jpeg-420-prob', '0']).jpeg_420_prob == 0.0                    # off: nothing to refuse
    for argv in (['train', '--jpeg-420-prob', '0.5'],
                 ['train', '--degradation', 'blind2', '--jpeg-420-prob', '0.5'],                 # without --device-data
                 ['train', '--device-data', '--jpeg-420-prob', '0.5'],                           # bicubic
                 ['train', '--device-data', '--degradation', 'bicubic', '--jpeg-420-prob', '0.5']):
        with pytest.raises(SystemExit) as exc:
            parse_args(argv)
        err = capsys.readouterr().err
        assert exc.value.code == 2 and '--jpeg-420-prob' in err and '--device-data' in err, argv
        assert '--degradation blind' in err and 'blind2' in err, argv
    for bad in ('1.5', '-0.1', 'nan', 'inf', 'half'):
        with pytest.raises(SystemExit) as exc:
            parse_args(['train', '--device-data', '--degradation', 'blind', '--jpeg-420-prob', bad])
        assert exc.value.code == 2 and '--jpeg-420-prob' in capsys.readouterr().err, bad


# ------------------------------------------------------------------------------------------------------- the loader
def _loader(degradation, batch=4, n_images=9, **kw):
    from torchsr_amd.dataset import DeviceLoader
    images = [torch.zeros((120 + i % 9, 130, 3), dtype=torch.uint8) for i in range(n_images)]
    return DeviceLoader(images, torch.device('cpu'), batch, 96, 4, False, 3, degradation=degradation, **kw)


@pytest.mark.parametrize('bad', [-0.1, 1.5, float('nan'), float('inf'), None, '0.5', True, [0.5]])
def test_device_loader_refuses_bad_jpeg420_prob(bad):
    with pytest.raises(ValueError, match='jpeg420_prob'):
        _loader('blind', jpeg420_prob=bad)


def test_device_loader_jpeg420_prob_argument():
    import inspect
    from torchsr_amd.dataset import DeviceLoader, initialize_device_datasets
    with pytest.raises(ValueError, match='jpeg420_prob'):
        _loader('bicubic', jpeg420_prob=0.5)
    assert _loader('bicubic', jpeg420_prob=0.0).jpeg420_prob == 0.0 and _loader('bicubic', jpeg420_prob=0).j420_rng is None
    assert _loader('blind', jpeg420_prob=1).jpeg420_prob == 1.0 and _loader('blind2', jpeg420_prob=0.5).j420_rng is not None
    for fn in (DeviceLoader.__init__, initialize_device_datasets):
        assert inspect.signature(fn).parameters['jpeg420_prob'].default == 0.0


def _same(a, b, but=()):
    assert a.keys() - set(but) == b.keys() - set(but)
    for k in a:
        if k in but:
            continue
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize('kw', [{}, {'poisson_prob': 0.5}])
@pytest.mark.parametrize('degradation', ['blind', 'blind2'])
def test_probability_0_plans_what_no_argument_plans(degradation, kw):
    """Key for key and bit for bit: the rows and every array of ``deg``; no stream is created."""
    plain, off = _loader(degradation, **kw), _loader(degradation, jpeg420_prob=0.0, **kw)
    assert off.j420_rng is None and plain.j420_rng is None
    batches = 0
    for _ in range(2):  # epochs
        for (ip, mp, dp), (i0, m0, d0) in zip(plain._plan(), off._plan()):
            assert ip == i0 and mp == m0 and 'chroma420' not in d0
            _same(dp, d0)
            batches += 1
    assert batches == 4
    assert off.rng.getstate() == plain.rng.getstate() and off.deg_rng.getstate() == plain.deg_rng.getstate()


@pytest.mark.parametrize('degradation', ['blind', 'blind2'])
def test_jpeg420_draw(degradation):
    """2 000 draws at probability 0.5 with one seed: the rows and every other array of ``deg`` are what the loader without the
    argument plans; the flags are the stream's uniforms, drawn again by hand -- one per sample and JPEG stage, sample-major; their
    frequency lies within 4 sigma of 0.5 (sigma = sqrt(2000 / 4) = 22.4 draws); probability 1 sets every flag from the same
    stream position; the other streams end where they end without the argument."""
    import random
    stages = 1 if degradation == 'blind' else 2
    batch = 50
    make = lambda **kw: _loader(degradation, batch=batch, n_images=100, **kw)  # noqa: E731
    plain, half, one = make(), make(jpeg420_prob=0.5), make(jpeg420_prob=1.0)
    replay = random.Random(3 * 67867967 + 0 + 236887691)
    flags_set = draws = 0
    for _ in range(2000 // (100 * stages)):  # epochs
        for (ip, mp, dp), (ih, mh, dh), (i1, m1, d1) in zip(plain._plan(), half._plan(), one._plan()):
            assert ip == ih == i1 and mp == mh == m1                      # the rows: every hr batch
            _same(dp, dh, but=('chroma420',))
            _same(dp, d1, but=('chroma420',))
            fl = dh['chroma420']
            assert fl.dtype == np.int32 and fl.shape == dp['quality'].shape and (d1['chroma420'] == 1).all()
            want = np.array([[int(replay.random() < 0.5) for _ in range(stages)] for _ in range(batch)], dtype=np.int32).T
            assert np.array_equal(fl.reshape(stages, batch), want)
            flags_set += int(fl.sum())
            draws += fl.size
    print(f'{degradation}: {flags_set} of {draws} flags set')
    assert draws == 2000 and abs(flags_set - 1000) <= 4 * np.sqrt(2000 * 0.25)
    assert half.j420_rng.getstate() == one.j420_rng.getstate() == replay.getstate()
    assert half.deg_rng.getstate() == plain.deg_rng.getstate() and half.rng.getstate() == plain.rng.getstate()


def test_jpeg420_draw_follows_the_poisson_draw():
    """Both flags: each stream is the one it is alone, and ``deg`` carries both keys."""
    both, poi, j420 = (_loader('blind2', **kw) for kw in ({'poisson_prob': 0.5, 'jpeg420_prob': 0.5}, {'poisson_prob': 0.5},
                                                          {'jpeg420_prob': 0.5}))
    for (_, _, db), (_, _, dp), (_, _, dj) in zip(both._plan(), poi._plan(), j420._plan()):
        _same(db, dp, but=('chroma420',))
        assert np.array_equal(db['chroma420'], dj['chroma420'])
    assert both.j420_rng.getstate() == j420.j420_rng.getstate() and both.poi_rng.getstate() == poi.poi_rng.getstate()


# ------------------------------------------------------------------------------------------------------- the ABI
def test_workspace_size():
    from torchsr_amd import _lib
    lib = _lib.lib()
    for n, h, w in ((1, 8, 8), (6, 24, 40), (16, 32, 32), (4, 128, 136)):
        assert lib.srx_jpeg_sim2_workspace(n, h, w) == n * 2 * J.chroma_blocks(h) * 8 * J.chroma_blocks(w) * 8 * 4
    assert lib.srx_jpeg_sim2_workspace(0, 8, 8) == 0 and lib.srx_jpeg_sim2_workspace(1, -8, 8) == 0


def test_abi_refuses_bad_jpeg_sim2_arguments_without_a_gpu():
    """srx_jpeg_sim2 refuses with a status code BEFORE either launch -- so the checks run here, with fake pointers, on CPU."""
    import ctypes as C
    from torchsr_amd import _lib
    if torch.cuda.is_available():
        pytest.skip('fake pointers: argument validation is exercised where a missed check cannot reach a device')
    lib = _lib.lib()
    x, out, quality, flags, ws, quot = (0x1000000 + i * 0x100000 for i in range(6))  # never dereferenced

    def err():
        buf = C.create_string_buffer(256)
        lib.srx_last_error(buf, 256)
        return buf.value.decode()

    def refused(word, x=x, out=out, quality=quality, flags=flags, ws=ws, quot=quot, n=2, h=24, w=40, ws_bytes=None):
        ws_bytes = lib.srx_jpeg_sim2_workspace(n, h, w) if ws_bytes is None else ws_bytes
        rc = lib.srx_jpeg_sim2(x, out, quality, flags, n, h, w, 1, ws, ws_bytes, quot, None)
        return rc != 0 and 'jpeg_sim2' in err() and word in err()

    for name in ('x', 'out', 'quality', 'flags', 'ws'):
        assert refused('null pointer', **{name: None}), name
    assert refused('bad shape', n=0) and refused('bad shape', n=65536) and refused('bad shape', h=0) and refused('bad shape', w=-8)
    assert refused('whole 8 x 8 blocks', h=12) and refused('whole 8 x 8 blocks', w=20) and refused('whole 8 x 8 blocks', h=4)
    assert refused('too large', h=1 << 16, w=1 << 15) and refused('too large', h=8 * 65536, w=8)
    need = lib.srx_jpeg_sim2_workspace(2, 24, 40)
    assert refused('workspace', ws_bytes=need - 1) and refused('workspace', ws_bytes=0)
