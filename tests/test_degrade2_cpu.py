"""``--degradation blind2`` without a GPU: J1 and the kernel tables, the resize tables against torch's ``interpolate``, the
restatement of ``srx_filter2d`` the GPU tests compare against, the host-side draw and its random streams, the CLI flag and the
ABI's refusals."""
import math
import random

import numpy as np
import pytest
import torch

import degrade2_ref as R2
import degrade_ref as R


# ------------------------------------------------------------------------------------------------------- J1 and the kernels
def test_bessel_j1_known_values():
    from torchsr_amd.degradation import bessel_j1
    assert abs(float(bessel_j1(1.0)) - 0.44005058574493355) < 1e-15
    assert abs(float(bessel_j1(10.0)) - 0.04347274616886144) < 1e-15
    assert abs(float(bessel_j1(3.8317059702075125))) < 1e-14          # the first zero
    assert abs(float(bessel_j1(0.0))) < 1e-15 and bessel_j1(np.linspace(0, 45, 7)).shape == (7,)


def test_bessel_j1_against_scipy():
    special = pytest.importorskip('scipy.special')
    from torchsr_amd.degradation import bessel_j1
    x = np.linspace(0.0, 45.0, 2001)
    err = float(np.abs(bessel_j1(x) - special.j1(x)).max())
    print(f'max |J1 - scipy| on [0, 45] = {err:.2e}')
    assert err <= 1e-14


KERNELS = {'gauss': dict(sigma_x=3.0, sigma_y=0.5, theta=0.6), 'generalized': dict(sigma_x=2.0, sigma_y=0.7, theta=-1.1, beta=0.8),
           'plateau': dict(sigma_x=1.5, sigma_y=2.5, theta=2.0, beta=1.7), 'sinc': dict(omega_c=math.pi / 2)}


@pytest.mark.parametrize('kind', list(KERNELS))
@pytest.mark.parametrize('ksize', [7, 13, 21])
def test_kernel_weights_sum_to_one(kind, ksize):
    from torchsr_amd.degradation import kernel_weights
    w = kernel_weights(kind, ksize, **KERNELS[kind])
    assert w.shape == (ksize, ksize) and w.dtype == np.float64 and abs(w.sum() - 1) < 1e-12
    assert np.unravel_index(np.abs(w).argmax(), w.shape) == (ksize // 2, ksize // 2)


def test_kernel_weights_families():
    from torchsr_amd.degradation import bessel_j1, kernel_weights
    # gauss is srx_blur_aniso's kernel
    for sx, sy, theta, ks in ((3.0, 0.5, 0.6, 21), (0.2, 0.2, 0.0, 7), (1.3, 2.9, -3.0, 13)):
        assert np.abs(kernel_weights('gauss', ks, sx, sy, theta) - R.blur_weights(sx, sy, theta, ks).numpy()).max() <= 1e-15
    # beta = 1: the generalised Gaussian is the Gaussian; the plateau is 1 / (1 + q) up to its sum
    g = kernel_weights('gauss', 9, 1.2, 0.6, 0.4)
    assert np.abs(kernel_weights('generalized', 9, 1.2, 0.6, 0.4, beta=1.0) - g).max() < 1e-15
    p = kernel_weights('plateau', 9, 1.2, 0.6, 0.4, beta=1.0)
    q = -2.0 * np.log(g / g[4, 4])
    assert np.abs(p / p[4, 4] - 1.0 / (1.0 + q)).max() < 1e-12
    # beta changes the shape
    assert np.abs(kernel_weights('generalized', 9, 1.2, 0.6, 0.4, beta=3.0) - g).max() > 1e-3
    # sinc: the formula at a tap, its symmetry group, its negative lobes
    for ks, omega in ((21, math.pi), (7, math.pi / 3), (13, 1.0)):
        w = kernel_weights('sinc', ks, omega_c=omega)
        r = ks // 2
        rho = math.hypot(2, 3)
        ratio = (omega * float(bessel_j1(omega * rho)) / (2 * math.pi * rho)) / (omega * omega / (4 * math.pi))
        assert abs(w[r + 3, r + 2] / w[r, r] - ratio) < 1e-13
        for k in range(4):
            assert np.array_equal(np.rot90(w, k), w) and np.array_equal(np.rot90(w, k).T, w)   # the 8 flips and transposes
    assert (kernel_weights('sinc', 21, omega_c=math.pi) < 0).any() and (kernel_weights('sinc', 7, omega_c=math.pi) < 0).any()
    assert np.abs(kernel_weights('sinc', 21, omega_c=math.pi)).sum() < 4.95   # what the ABI comment quotes
    with pytest.raises(ValueError):
        kernel_weights('box', 7)
    for bad in (0, 8, 23, -3):
        with pytest.raises(ValueError):
            kernel_weights('gauss', bad)


def test_kernel_slot_is_centred():
    from torchsr_amd.degradation import KERNEL_SLOT, kernel_slot, kernel_weights
    assert KERNEL_SLOT == R2.SLOT == R.BLUR_MAX_K
    for ks in (1, 7, 21):
        w = kernel_weights('plateau', ks, 1.5, 0.7, 0.3, beta=1.5)
        slot = kernel_slot(w)
        assert slot.shape == (21, 21) and slot.dtype == np.float32
        assert np.array_equal(R2.window(slot, ks), w.astype(np.float32))
        assert slot[10, 10] == np.float32(w[ks // 2, ks // 2])
        outside = slot.copy()
        o = 10 - ks // 2
        outside[o:o + ks, o:o + ks] = 0
        assert not outside.any()
    assert not kernel_slot(None).any()


# ------------------------------------------------------------------------------------------------------- the resize tables
@pytest.mark.parametrize('mode', R2.MODES)
def test_resize_tables_against_interpolate(mode):
    from torchsr_amd.functional import resize_tables
    rng = np.random.RandomState(7)
    worst = 0.0
    for n_in, n_out in R2.RESIZE_PAIRS:
        start, weight, k = resize_tables(n_in, n_out, mode, dtype='float64')
        assert start.dtype == np.int32 and start.shape == (n_out,) and weight.shape == (n_out, k) and weight.dtype == np.float64
        assert start.min() >= 0 and start.max() <= n_in - 1 and 1 <= k <= 66
        assert np.abs(weight.sum(axis=1) - 1).max() < 1e-12
        x = rng.rand(2, 3, n_in, 5)
        err_y = np.abs(R2.apply_tables(x, start, weight, 2) - R2.interpolate64(x, (n_out, 5), mode)).max()
        xt = np.ascontiguousarray(x.transpose(0, 1, 3, 2))
        err_x = np.abs(R2.apply_tables(xt, start, weight, 3) - R2.interpolate64(xt, (5, n_out), mode)).max()
        worst = max(worst, err_y, err_x)
        assert err_y <= 1e-12 and err_x <= 1e-12, (n_in, n_out, err_y, err_x)
        s32, w32, k32 = resize_tables(n_in, n_out, mode)
        assert w32.dtype == np.float32 and k32 == k and np.array_equal(s32, start) and np.array_equal(w32, weight.astype(np.float32))
    print(f'{mode}: max |tables - F.interpolate| in float64 = {worst:.2e}')


@pytest.mark.parametrize('mode', R2.MODES)
def test_resize_tables_identity_and_refusals(mode):
    from torchsr_amd.functional import resize_tables
    x = np.random.RandomState(1).rand(1, 1, 24, 3)
    for n in (1, 11, 24):
        start, weight, _ = resize_tables(n, n, mode, dtype='float64')
        assert np.array_equal(R2.apply_tables(x[:, :, :n], start, weight, 2), x[:, :, :n])
    with pytest.raises(ValueError, match='16:1'):
        resize_tables(17 * 4, 4, mode)
    resize_tables(16 * 4, 4, mode)
    for bad in ((0, 4), (4, 0), (True, 4), (4.0, 4)):
        with pytest.raises(ValueError):
            resize_tables(*bad, mode)
    with pytest.raises(ValueError, match='mode'):
        resize_tables(8, 4, 'nearest')


def test_resize_refuses_before_the_device():
    """The argument checks of ``resize`` come before anything touches a device: they answer on CPU tensors."""
    from torchsr_amd.functional import resize
    x = torch.zeros(1, 3, 170, 20)
    with pytest.raises(ValueError, match='16:1'):
        resize(x, (10, 20), 'area')
    with pytest.raises(ValueError, match='mode'):
        resize(x, (20, 20), 'nearest')
    with pytest.raises(ValueError, match='NCHW'):
        resize(x[0], (20, 20), 'area')
    with pytest.raises(ValueError, match='positive int'):
        resize(x, (0, 20), 'area')
    with pytest.raises(RuntimeError, match='no backward'):
        resize(x.requires_grad_(True), (20, 20), 'area')


# ------------------------------------------------------------------------------------------------------- the filter restatement
def test_filter2d_restatement_is_a_reflected_correlation():
    from torchsr_amd.degradation import kernel_slot, kernel_weights
    rng = np.random.RandomState(3)
    x = rng.rand(4, 3, 13, 17) * 3 - 1
    slots = np.stack([kernel_slot(kernel_weights('sinc', 21, omega_c=math.pi)), kernel_slot(kernel_weights('sinc', 7, omega_c=1.2)),
                      kernel_slot(kernel_weights('plateau', 13, 2.0, 0.6, 0.7, beta=1.3)), kernel_slot(None)])
    slots[1, 0, :] = 9.0  # outside the 7 x 7 window: never read
    ksize = [21, 7, 13, 0]
    got = R2.filter2d(x, slots, ksize)
    want = R2.filter2d_conv(x, slots, ksize).numpy()
    err = float(np.abs(got - want).max())
    print(f'max |restatement - conv2d| = {err:.2e}')
    assert err <= 1e-12 and np.array_equal(got[3], x[3])
    # an oriented kernel: a transposed window is told apart
    assert np.abs(R2.filter2d(x, slots.transpose(0, 2, 1), ksize)[2] - got[2]).max() > 1e-3
    q = R2.filter2d(x, slots, ksize, quantize=1)
    assert q.min() >= 0 and q.max() <= 1 and np.abs(q * 255 - np.rint(q * 255)).max() < 1e-12
    assert np.array_equal(q[3], R2.quantize8(x[3])) and (q == 0).any() and (q == 1).any()
    assert [R.legal_ksize(k) for k in (-3, 4, 40)] == [0, 5, 21]


# ------------------------------------------------------------------------------------------------------- the host-side draw
def _loader(degradation, seed=11, sizes=((120, 150), (97, 96), (200, 130), (96, 96), (140, 101)), batch=2, rank=0, crop=96):
    from torchsr_amd.dataset import DeviceLoader
    images = [torch.zeros(max(h, crop), max(w, crop), 3, dtype=torch.uint8) for h, w in sizes]
    return DeviceLoader(images, torch.device('cpu'), batch, crop, 4, False, seed, 5, rank, 1, degradation=degradation)


ARRAYS = ('weights', 'ksize', 'sigma_n', 'gray', 'quality')
SCALARS = ('sizes', 'modes', 'order', 'seed1', 'seed2', 'kinds')


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ARRAYS) and all(a[k] == b[k] for k in SCALARS)


def test_draw2_is_reproducible_and_per_seed_and_rank():
    a, b, c, d = _loader('blind2'), _loader('blind2'), _loader('blind2', seed=12), _loader('blind2', rank=1)
    for _ in range(3):
        da, db = a._draw_degradation2(4), b._draw_degradation2(4)
        assert _same(da, db)
    first = _loader('blind2')._draw_degradation2(4)
    assert not _same(da, first) and da['seed1'] != first['seed1'] and first['seed1'] != first['seed2']
    for other in (c, d):
        do = other._draw_degradation2(4)
        assert do['seed1'] != first['seed1'] and not np.array_equal(do['weights'], first['weights'])
    # through _plan: train batches carry a blind2 draw, the test loader none
    plans = list(_loader('blind2')._plan())
    assert len(plans) == 12 and all(deg is not None and 'order' in deg for _, _, deg in plans)
    assert _same(plans[0][2], _loader('blind2')._draw_degradation2(2))   # the loader's batch size
    from torchsr_amd.dataset import DeviceLoader
    test = DeviceLoader([torch.zeros(100, 100, 3, dtype=torch.uint8)] * 3, torch.device('cpu'), 2, 96, 4, True, 3, degradation='blind2')
    assert all(deg is None for _, _, deg in test._plan())


def test_draw2_layout():
    d = _loader('blind2')._draw_degradation2(5)
    assert d['weights'].shape == (3, 5, 21, 21) and d['weights'].dtype == np.float32 and d['weights'].flags['C_CONTIGUOUS']
    assert d['ksize'].shape == (3, 5) and d['ksize'].dtype == np.int32
    assert d['sigma_n'].shape == (2, 5) and d['sigma_n'].dtype == np.float32
    assert all(d[k].shape == (2, 5) and d[k].dtype == np.int32 for k in ('gray', 'quality'))
    assert len(d['sizes']) == 3 and d['sizes'][2] == 24 and len(d['modes']) == 3 and d['order'] in ('A', 'B')
    assert 0 <= d['seed1'] < 2 ** 64 and 0 <= d['seed2'] < 2 ** 64
    for stage in range(3):
        for i in range(5):
            ks, slot = int(d['ksize'][stage, i]), d['weights'][stage, i]
            if ks == 0:
                assert d['kinds'][stage][i] in ('skip', 'pulse') and not slot.any()
            else:
                assert ks % 2 == 1 and 7 <= ks <= 21 and abs(float(R2.window(slot, ks).astype(np.float64).sum()) - 1) < 1e-5
                outside = slot.copy()
                outside[10 - ks // 2:11 + ks // 2, 10 - ks // 2:11 + ks // 2] = 0
                assert not outside.any()


def test_crop_and_flip_stream_is_the_same_in_all_modes():
    rows = {}
    for name in ('bicubic', 'blind2'):
        loader, got = _loader(name), []
        for _ in range(3):
            for idx, meta, deg in loader._plan():
                assert (deg is None) == (name == 'bicubic')
                got += [tuple(m[2:]) for m in meta]
        rows[name] = got
    assert rows['bicubic'] == rows['blind2'] and len(rows['bicubic']) == 72
    assert _loader('bicubic').deg_rng.getstate() == random.Random(11 * 15485863 + 0 + 982451653).getstate()


def test_blind_did_not_move():
    """The first three ``blind`` batches of a seed, re-derived here from the degradation stream as the first-order recipe draws
    it: size, one uniform for isotropic, sigma(s) and theta, noise sigma, grey flag, quality per sample, then the seed."""
    seed, rank, n = 11, 0, 2
    loader = _loader('blind', seed=seed, rank=rank)
    plans = [deg for _, _, deg in loader._plan()][:3]
    rng = random.Random(seed * 15485863 + rank + 982451653)
    for deg in plans:
        parm, ksize = np.zeros((n, 4), dtype=np.float32), np.zeros(n, dtype=np.int32)
        sigma_n, gray, quality = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        for i in range(n):
            ksize[i] = 2 * rng.randint(3, 10) + 1
            if rng.random() < 0.5:
                sx = sy = rng.uniform(0.2, 3.0)
                theta = 0.0
            else:
                sx, sy = rng.uniform(0.2, 3.0), rng.uniform(0.2, 3.0)
                theta = -math.pi + 2.0 * math.pi * rng.random()
            parm[i, :3] = sx, sy, theta
            sigma_n[i] = rng.uniform(1.0, 30.0) / 255.0
            gray[i] = int(rng.random() < 0.4)
            quality[i] = rng.randint(30, 95)
        want = {'parm': parm, 'ksize': ksize, 'sigma_n': sigma_n, 'gray': gray, 'quality': quality}
        assert set(deg) == set(want) | {'seed'}
        assert all(np.array_equal(deg[k], want[k]) for k in want) and deg['seed'] == rng.getrandbits(64)


def test_draw2_sizes_and_branches():
    from torchsr_amd.dataset import BLIND2_KINDS, BLIND2_MODES
    for crop in (96, 128):
        loader = _loader('blind2', crop=crop, seed=crop)
        lc = crop // 4
        kinds, modes, orders, s1s, s2s = [set(), set(), set()], [set(), set(), set()], set(), set(), set()
        for _ in range(2000):
            d = loader._draw_degradation2(2)
            s1, s2, last = d['sizes']
            assert last == lc and s1 % 8 == 0 and s2 % 8 == 0 and s1 >= 16 and s2 >= 16
            assert s1 <= 8 * int(1.5 * crop / 8 + 0.5) and s2 <= 8 * int(1.2 * lc / 8 + 0.5)
            assert crop <= 16 * s1 and s1 <= 16 * s2                    # what functional.resize admits
            s1s.add(s1), s2s.add(s2), orders.add(d['order'])
            for stage in range(3):
                kinds[stage].update(d['kinds'][stage])
                modes[stage].add(d['modes'][stage])
            assert d['sigma_n'][0].min() >= np.float32(1 / 255) and d['sigma_n'][0].max() <= np.float32(30 / 255)
            assert d['sigma_n'][1].min() >= np.float32(1 / 255) and d['sigma_n'][1].max() <= np.float32(25 / 255)
            assert d['quality'].min() >= 30 and d['quality'].max() <= 95 and set(np.unique(d['gray'])) <= {0, 1}
        assert kinds[0] == set(BLIND2_KINDS) | {'sinc'}
        assert kinds[1] == set(BLIND2_KINDS) | {'sinc', 'skip'}       # the skipped second blur
        assert kinds[2] == {'sinc', 'pulse'}                           # the final sinc, or the pulse
        assert all(m == set(BLIND2_MODES) for m in modes) and orders == {'A', 'B'}
        assert min(s1s) < crop < max(s1s) and crop in s1s and min(s2s) < lc < max(s2s) and lc in s2s


def test_blind2_constructor_checks():
    from torchsr_amd.dataset import DEGRADATIONS, DeviceLoader
    assert DEGRADATIONS == ('bicubic', 'blind', 'blind2')
    images = [torch.zeros(300, 300, 3, dtype=torch.uint8)] * 3
    with pytest.raises(ValueError, match='degradation'):
        DeviceLoader(images, torch.device('cpu'), 2, 96, 4, False, 3, degradation='sinc')
    with pytest.raises(ValueError, match='multiple of 8'):
        DeviceLoader(images, torch.device('cpu'), 2, 100, 4, False, 3, degradation='blind2')
    with pytest.raises(ValueError, match='more than 10 pixels'):      # an 8 x 8 low-resolution side: the final filter needs 11 rows
        DeviceLoader(images, torch.device('cpu'), 2, 32, 4, False, 3, degradation='blind2')
    with pytest.raises(ValueError, match='16:1'):                     # 288 * 1.5 = 432 -> 24 would be 18:1
        DeviceLoader(images, torch.device('cpu'), 2, 288, 4, False, 3, degradation='blind2')
    DeviceLoader(images, torch.device('cpu'), 2, 32, 4, False, 3, degradation='blind')   # blind itself keeps its check
    DeviceLoader(images, torch.device('cpu'), 2, 128, 4, False, 3, degradation='blind2')


# ------------------------------------------------------------------------------------------------------- the CLI
def test_cli_blind2_flag(capsys):
    from torchsr_amd.torchsr import parse_args
    assert parse_args(['train', '--device-data', '--degradation', 'blind2']).degradation == 'blind2'
    with pytest.raises(SystemExit) as exc:
        parse_args(['train', '--degradation', 'blind2'])
    assert exc.value.code == 2 and '--device-data' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(['train', '--device-data', '--degradation', 'sinc'])


# ------------------------------------------------------------------------------------------------------- the ABI
def test_abi_refuses_bad_filter2d_arguments_without_a_gpu():
    """srx_filter2d refuses null pointers and the shapes its kernel is not written for with a status code BEFORE anything is
    launched -- so the checks run here, with fake pointers, on CPU."""
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

    def filt(i=fake, o=fake + 4096, wt=fake, k=fake, n=2, c=3, h=96, w=96, q=0):
        return lib.srx_filter2d(i, o, wt, k, n, c, h, w, q, None)

    for arg in ('i', 'o', 'wt', 'k'):
        assert filt(**{arg: None}) != 0 and 'filter2d' in err() and 'null' in err(), arg
    assert filt(o=fake) != 0 and 'must not be the input' in err()
    for bad in ({'n': 0}, {'n': -1}, {'n': 65536}, {'h': 0}, {'w': -5}):
        assert filt(**bad) != 0 and 'bad shape' in err(), bad
    for c in (0, 1, 2, 4, -3):
        assert filt(c=c) != 0 and '3 channels' in err(), c
    for bad in ({'h': 10}, {'w': 10}, {'h': 1, 'w': 1}):
        assert filt(**bad) != 0 and '11 rows' in err(), bad
