"""``--gt-usm`` without a GPU: the CLI flag, the taps, the loader's and the ABI's refusals, and self-checks of the float64
restatement (usm_ref.py) the GPU tests compare against."""
import math

import numpy as np
import pytest
import torch

import usm_ref as U


# ------------------------------------------------------------------------------------------------------- the CLI
def test_cli_gt_usm_flag(capsys):
    from torchsr_amd.torchsr import parse_args
    assert parse_args(['train']).gt_usm is False
    assert parse_args(['train', '--device-data']).gt_usm is False
    assert parse_args(['train', '--device-data', '--gt-usm']).gt_usm is True
    assert parse_args(['train', '--device-data', '--degradation', 'blind2', '--gt-usm']).gt_usm is True
    with pytest.raises(SystemExit) as exc:
        parse_args(['train', '--gt-usm'])
    err = capsys.readouterr().err
    assert exc.value.code == 2 and '--gt-usm' in err and '--device-data' in err


# ------------------------------------------------------------------------------------------------------- the taps
def test_usm_taps_defaults():
    from torchsr_amd import functional as F
    g = F.usm_taps(51, 8.0)
    assert g.shape == (51,) and g.dtype == np.float32
    assert np.array_equal(g, g[::-1]) and g.argmax() == 25 and (g > 0).all()
    assert abs(float(g.astype(np.float64).sum()) - 1.0) <= 51 * 2.0 ** -24       # 51 roundings of at most half an ulp of < 1
    i = np.arange(51, dtype=np.float64)
    want = np.exp(-(i - 25) ** 2 / (2 * 8.0 ** 2))
    assert np.array_equal(g, (want / want.sum()).astype(np.float32))
    assert np.array_equal(g, U.taps64(51, 8.0).astype(np.float32))
    assert np.array_equal(F.usm_taps(), g)                                       # the defaults are USMSharp's
    assert math.isclose(0.3 * ((51 - 1) / 2 - 1) + 0.8, 8.0, rel_tol=1e-15)      # the sigma cv2.getGaussianKernel(51, 0) derives
    g7 = F.usm_taps(7, 1.7)
    assert g7.shape == (7,) and np.array_equal(g7, U.taps64(7, 1.7).astype(np.float32))


@pytest.mark.parametrize('ksize,sigma', [(50, 8.0), (4, 1.0), (53, 8.0), (1, 1.0), (-3, 1.0), (51.0, 8.0), (True, 1.0), (51, 0.0),
                                         (51, -2.0), (51, float('nan')), (51, float('inf')), (51, None), (51, '8')])
def test_usm_taps_refuses_bad_arguments(ksize, sigma):
    from torchsr_amd import functional as F
    with pytest.raises(ValueError):
        F.usm_taps(ksize, sigma)


def test_usm_sharpen_checks_arguments_before_the_device():
    """Every ValueError is raised from a CPU tensor: nothing has touched a device by then."""
    from torchsr_amd import functional as F
    x = torch.zeros(1, 3, 40, 40)
    for kw in (dict(ksize=50), dict(ksize=53), dict(sigma=0.0), dict(sigma=float('nan')), dict(weight=float('inf')),
               dict(threshold=float('nan')), dict(weight='1'), dict(ksize=21, sigma=-1.0)):
        with pytest.raises(ValueError):
            F.usm_sharpen(x, **kw)
    with pytest.raises(ValueError):
        F.usm_sharpen(torch.zeros(1, 3, 25, 40))     # H = 25: a 51-tap reflect needs 26 rows
    with pytest.raises(ValueError):
        F.usm_sharpen(torch.zeros(1, 3, 40, 25))
    with pytest.raises(ValueError):
        F.usm_sharpen(torch.zeros(3, 40, 40))
    with pytest.raises(ValueError):
        F.usm_sharpen(torch.zeros(0, 3, 40, 40))
    with pytest.raises(RuntimeError, match='no backward'):
        F.usm_sharpen(torch.zeros(1, 3, 40, 40, requires_grad=True))
    with pytest.raises(RuntimeError, match='no CPU fallback'):   # legal arguments: the tensor's device is what is refused
        F.usm_sharpen(x)


# ------------------------------------------------------------------------------------------------------- the loader
def test_device_loader_gt_usm_argument():
    from torchsr_amd.dataset import DeviceLoader
    images = [torch.zeros((40, 40, 3), dtype=torch.uint8)]
    cpu = torch.device('cpu')
    with pytest.raises(ValueError, match='gt_usm'):
        DeviceLoader(images, cpu, 2, 25, 1, False, 3, gt_usm=True)
    with pytest.raises(ValueError, match='gt_usm'):
        DeviceLoader(images, cpu, 2, 24, 4, False, 3, gt_usm=True)
    assert DeviceLoader(images, cpu, 2, 26, 1, False, 3, gt_usm=True).gt_usm is True
    assert DeviceLoader(images, cpu, 2, 24, 4, False, 3).gt_usm is False          # without it a small crop stays legal
    assert DeviceLoader(images, cpu, 2, 32, 4, False, 3, degradation='blind', gt_usm=True).gt_usm is True
    with pytest.raises(ValueError, match='gt_usm'):
        DeviceLoader(images, cpu, 2, 32, 4, False, 3, 1, 0, 1, 'blind')           # a mode in the flag's place is noticed


def test_gt_usm_draws_no_random_numbers():
    """The host side of an epoch -- indices, crop / flip rows, degradation draws -- is the same with and without gt_usm."""
    from torchsr_amd.dataset import DeviceLoader
    images = [torch.zeros((120 + i, 130, 3), dtype=torch.uint8) for i in range(9)]
    for degradation in ('bicubic', 'blind', 'blind2'):
        a = DeviceLoader(images, torch.device('cpu'), 4, 96, 4, False, 3, degradation=degradation)
        b = DeviceLoader(images, torch.device('cpu'), 4, 96, 4, False, 3, degradation=degradation, gt_usm=True)
        for _ in range(2):
            for (ia, ma, da), (ib, mb, db) in zip(a._plan(), b._plan()):
                assert ia == ib and ma == mb and (da is None) == (db is None)
                if da is not None:
                    assert da.keys() == db.keys()
                    for k in da:
                        assert np.array_equal(da[k], db[k]) if isinstance(da[k], np.ndarray) else da[k] == db[k]


# ------------------------------------------------------------------------------------------------------- the ABI
def test_abi_refuses_bad_usm_sharpen_arguments_without_a_gpu():
    """srx_usm_sharpen refuses every argument set its kernels are not written for with a status code BEFORE anything is launched
    -- so the checks run here, with fake pointers, on CPU."""
    import ctypes as C
    from torchsr_amd import _lib
    if torch.cuda.is_available():
        pytest.skip('fake pointers: argument validation is exercised where a missed check cannot reach a device')
    lib = _lib.lib()
    # never dereferenced: the calls below must fail in argument validation.  2 x 3 planes of 96 x 96: 221184 bytes each
    step = 0x100000
    x, out, blur, mask, taps = (0x1000000 + i * step for i in range(5))

    def err():
        buf = C.create_string_buffer(256)
        lib.srx_last_error(buf, 256)
        return buf.value.decode()

    def refused(word, x=x, out=out, blur=blur, mask=mask, taps=taps, ksize=51, planes=6, h=96, w=96, weight=0.5, threshold=10.0):
        rc = lib.srx_usm_sharpen(x, out, blur, mask, taps, ksize, planes, h, w, weight, threshold, None)
        return rc != 0 and word in err()

    for name in ('x', 'out', 'blur', 'mask', 'taps'):
        assert refused('null pointer', **{name: None}), name
    for ksize in (50, 4, 2, 1, 0, -51, 53, 101):
        assert refused('ksize', ksize=ksize), ksize
    assert refused('reflect', h=25) and refused('reflect', w=25) and refused('reflect', h=0) and refused('reflect', w=-4)
    assert refused('reflect', ksize=7, h=3) and refused('reflect', ksize=7, w=3)
    assert refused('planes', planes=0) and refused('planes', planes=-1)
    assert refused('2^31', planes=1 << 31, h=26, w=26) and refused('2^31', planes=1, h=1 << 16, w=1 << 15)
    assert refused('2^31', planes=1 << 11, h=1 << 10, w=1 << 10) and refused('2^31', planes=1 << 62, h=64, w=64)
    assert refused('2^31', planes=3, h=46341, w=46341)                                      # H * W alone passes 2^31
    for bad in (float('nan'), float('inf'), -float('inf')):
        assert refused('finite', weight=bad) and refused('finite', threshold=bad)
    nbytes = 6 * 96 * 96 * 4
    assert refused('overlap', out=x) and refused('overlap', blur=x) and refused('overlap', mask=x)
    assert refused('overlap', blur=out) and refused('overlap', mask=out) and refused('overlap', mask=blur)
    assert refused('overlap', out=x + nbytes - 4) and refused('overlap', out=x - nbytes + 4)      # by one float, either side
    assert refused('overlap', mask=blur + nbytes - 4) and refused('overlap', blur=out - nbytes + 4)
    # the buffers may touch: with a GPU these arguments would launch, so here only the checks' own arithmetic is asked about
    assert x + nbytes <= out and out + nbytes <= blur and blur + nbytes <= mask


# ------------------------------------------------------------------------------------------------------- the restatement
def test_reference_gauss_is_the_reflected_double_sum():
    """``usm_ref.gauss`` against the definition written out with explicit index reflection, on a plane smaller than the kernel."""
    g = U.taps64(7, 1.7)
    x = torch.rand((1, 2, 5, 6), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    got = U.gauss(x, g)

    def refl(i, n):
        i = -i if i < 0 else i
        return 2 * (n - 1) - i if i >= n else i

    for c in range(2):
        for y in range(5):
            for xx in range(6):
                want = sum(g[i] * g[j] * float(x[0, c, refl(y + i - 3, 5), refl(xx + j - 3, 6)]) for i in range(7) for j in range(7))
                assert abs(float(got[0, c, y, xx]) - want) < 1e-14


def test_reference_identities():
    g = U.taps64(51, 8.0)
    flat = np.full((1, 3, 40, 33), 0.37)
    out, blur, mask, _ = U.usm(flat, g, 0.5, 10.0)
    assert float((blur - 0.37).abs().max()) < 1e-14 and float(mask.sum()) == 0 and np.array_equal(out.numpy(), flat)
    x = U.images(2, 40, 61)
    out, _, mask, t = U.usm(x, g, 0.5, 300.0)                  # no residual reaches 300 grey levels
    assert float(t.max()) <= 255 and float(mask.sum()) == 0 and np.array_equal(out.numpy(), x.astype(np.float64))
    out, _, mask, _ = U.usm(x, g, 0.0, 10.0)                   # weight 0: sharp is x
    assert 0.1 < float(mask.mean()) < 0.9 and np.array_equal(out.numpy(), x.astype(np.float64))
    out, _, _, _ = U.usm(x, g, 0.5, 10.0)
    assert float((out - torch.from_numpy(x)).abs().max()) > 1e-2 and float(out.min()) >= 0 and float(out.max()) <= 1


def test_reference_images():
    x = U.images(2, 96, 96)
    assert x.shape == (2, 3, 96, 96) and x.dtype == np.float32 and x.min() >= 0 and x.max() <= 1
    assert np.abs(x.astype(np.float64) * 255 - np.rint(x.astype(np.float64) * 255)).max() < 1e-4
    assert x[:, :, 32:, 48:].std() < 0.5 * x[:, :, :32, :].std()    # the flattened region


def test_tolerances_are_what_the_design_states():
    assert math.isclose((2 * 51 + 2) * 2.0 ** -24, 6.2e-6, rel_tol=0.01) and math.isclose((2 * 51 + 8) * 2.0 ** -24, 6.6e-6, rel_tol=0.01)
    assert 2.5 * 255 * (2 * 51 + 2) * 2.0 ** -24 <= 4e-3      # the mask's undecided band, in grey levels
