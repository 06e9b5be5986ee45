"""``--color-fix`` without a GPU: the fp32 restatement of the wavelet fix (colorfix_ref.wavelet32, whose bits the kernels must
give) against the published form written independently in fp64, its fixed points, the CLI flag, the refusals of
``upscale(color_fix=)`` before the generator runs, those of the functional wrappers before the device is touched and those
of the C entry points before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import colorfix_ref as R

SHAPES = [(8, 12), (5, 7), (36, 68), (120, 200)]  # the first two: planes smaller than the largest radius (16)


def published(sr, u, levels):
    """StableSR's wavelet reconstruction in fp64: an image is split by ``levels`` depthwise 3x3 convolutions with
    [1 2 1]^T [1 2 1] / 16 at the dilations 1, 2, 4, ... on the replicate-padded image, ``high`` collecting what each blur
    removes; the result is the high frequencies of ``sr`` plus the low frequencies of ``u``."""
    k = torch.tensor([[1.0, 2.0, 1.0], [2.0, 4.0, 2.0], [1.0, 2.0, 1.0]], dtype=torch.float64) / 16.0

    def decompose(img):
        c = img.shape[1]
        high, low = torch.zeros_like(img), img
        for i in range(levels):
            r = 2 ** i
            padded = low
            for _ in range(r):  # replicate padding, one pixel at a time: no limit by the size of the plane
                padded = torch.nn.functional.pad(padded, (1, 1, 1, 1), mode='replicate')
            blurred = torch.nn.functional.conv2d(padded, k.expand(c, 1, 3, 3), groups=c, dilation=r)
            high = high + (low - blurred)
            low = blurred
        return high, low

    sr64, u64 = torch.from_numpy(np.asarray(sr, dtype=np.float64)), torch.from_numpy(np.asarray(u, dtype=np.float64))
    return (decompose(sr64)[0] + decompose(u64)[1]).numpy()


def _pair(h, w, seed):
    g = np.random.RandomState(seed)
    return ((g.rand(2, 3, h, w) * 1.2 - 0.1).astype(np.float32) for _ in range(2))


@pytest.mark.parametrize('h,w', SHAPES)
@pytest.mark.parametrize('levels', [1, 3, 5])
def test_wavelet32_against_the_published_form(h, w, levels):
    """Four roundings per level (two per pass) plus the difference and the last sum, each of a value no larger than
    max(|U - sr|, |sr|, |out|) -- the blur is an average --: max error <= (4 levels + 2) 2^-24 max(|U - sr|, |sr|)."""
    sr, u = _pair(h, w, 100 * h + w)
    got = R.wavelet32(sr, u, levels)
    assert got.dtype == np.float32 and got.shape == sr.shape
    want = published(sr, u, levels)
    bound = (4 * levels + 2) * R.U32 * max(np.abs(u.astype(np.float64) - sr).max(), np.abs(sr).max())
    err = np.abs(got.astype(np.float64) - want).max()
    print(f'{(h, w)} levels {levels}: max err {err:.3e}, bound {bound:.3e}')
    assert err <= bound
    assert not np.array_equal(got, sr) and not np.array_equal(got, u)


@pytest.mark.parametrize('h,w', SHAPES)
def test_wavelet32_fixed_points(h, w):
    """``sr == U``: D is 0 and ``sr`` comes back bit for bit.  ``sr = U + c`` with a constant per channel: the blur of a constant
    is the constant and the cast is removed -- ``U`` comes back within (4 levels + 4) 2^-24 max|sr| (D is constant only up
    to the rounding of U + c and of the difference: two more roundings than the bound above)."""
    sr, u = _pair(h, w, 7 * h + w)
    for levels in (1, 5):
        assert np.array_equal(R.wavelet32(u, u, levels), u)
        c = np.array([0.2, -0.13, 0.05], dtype=np.float32).reshape(1, 3, 1, 1)
        cast = u + c
        got = R.wavelet32(cast, u, levels)
        err = np.abs(got.astype(np.float64) - u).max()
        bound = (4 * levels + 4) * R.U32 * np.abs(cast).max()
        print(f'{(h, w)} levels {levels}: cast removed to {err:.3e}, bound {bound:.3e}')
        assert err <= bound


def test_adain_ref_moves_the_moments():
    sr, lr = _pair(36, 68, 3)
    lr = lr[..., :9, :17] * 0.7 + 0.2
    want, (s, b), bound = R.adain_ref(sr, lr)
    (m, v), (ml, vl) = R.moments64(want), R.moments64(lr)
    assert np.allclose(m, ml, rtol=1e-12) and np.allclose(v + 1e-5 * s.astype(np.float64) ** 2, vl + 1e-5, rtol=1e-6)
    got32 = sr * s[..., None, None] + b[..., None, None]
    assert (np.abs(got32.astype(np.float64) - want) <= bound).all()
    one = R.adain_ref(sr[..., :1, :1], lr[..., :1, :1])  # one-pixel planes: both variances 0, s = 1, the input's value
    assert np.array_equal(one[1][0], np.ones((2, 3), dtype=np.float32)) and np.allclose(one[0], lr[..., :1, :1], atol=1e-7)


def test_cli_color_fix_flag():
    from torchsr_amd.torchsr import parse_args
    assert parse_args(['test', 'x.png']).color_fix is None
    assert parse_args(['test', 'x.png', '--color-fix', 'wavelet']).color_fix == 'wavelet'
    assert parse_args(['test', 'x.png', '--color-fix', 'adain']).color_fix == 'adain'
    args = parse_args(['test', 'x.png', '--color-fix', 'adain', '--outscale', '2', '--self-ensemble', '4', '--precision', 'bf16'])
    assert (args.color_fix, args.outscale, args.self_ensemble, args.precision) == ('adain', 2.0, 4, 'bf16')
    for bad in ('blue', 'Wavelet', ''):
        with pytest.raises(SystemExit):
            parse_args(['test', 'x.png', '--color-fix', bad])
    with pytest.raises(SystemExit):
        parse_args(['test', 'x.png', '--color-fix'])


def test_upscale_refuses_bad_color_fix_before_the_generator_runs():
    from torchsr_amd.test import upscale

    class Stub(torch.nn.Module):
        calls = 0

        def forward(self, x):
            Stub.calls += 1
            raise AssertionError('the generator ran')

        def eval(self):
            Stub.calls += 1
            raise AssertionError('the generator was touched')

    stub, x = Stub(), torch.zeros(1, 3, 8, 40)
    for bad in ('blue', 'Wavelet', '', True, 1, ['wavelet'], ('adain',)):
        with pytest.raises(ValueError, match='color_fix'):
            upscale(stub, x, color_fix=bad)
    with pytest.raises(ValueError, match='outscale'):  # the other refusals still come before the generator
        upscale(stub, x, color_fix='wavelet', outscale=-1)
    with pytest.raises(ValueError, match='16:1'):
        upscale(stub, x, color_fix='adain', outscale=0.2)
    with pytest.raises(ValueError, match='self_ensemble'):
        upscale(stub, x, color_fix='adain', self_ensemble=3)
    assert Stub.calls == 0
    for good in ('wavelet', 'adain'):  # a good one goes on to the generator
        with pytest.raises(AssertionError, match='generator'):
            upscale(stub, x, color_fix=good)
    assert Stub.calls == 2


def test_color_fix_wrappers_refuse_before_the_device():
    from torchsr_amd import functional as F
    sr, lr = torch.zeros(2, 3, 8, 12), torch.zeros(2, 3, 2, 3)
    for fix in (F.color_fix_wavelet, F.color_fix_adain):
        with pytest.raises(RuntimeError, match='inference-only'):
            fix(sr.clone().requires_grad_(True), lr)
        with pytest.raises(RuntimeError, match='inference-only'):
            fix(sr, lr.clone().requires_grad_(True))
        with torch.no_grad():
            with pytest.raises(RuntimeError, match='no CPU fallback'):
                fix(sr, lr)
            for bad in (torch.zeros(1, 3, 2, 3), torch.zeros(2, 4, 2, 3), torch.zeros(2, 1, 2, 3)):  # N, C
                with pytest.raises(ValueError, match='N and C'):
                    fix(sr, bad)
            with pytest.raises(ValueError, match='NCHW'):
                fix(sr[0], lr[0])
            with pytest.raises(ValueError, match='positive'):
                fix(sr, torch.zeros(2, 3, 0, 3))
            with pytest.raises(RuntimeError, match='contiguous'):
                fix(sr.transpose(2, 3), lr)
            with pytest.raises(RuntimeError, match='contiguous'):
                fix(sr, lr.transpose(2, 3))
            with pytest.raises(RuntimeError, match='contiguous'):
                fix(sr, lr, out=torch.zeros(2, 3, 12, 8).transpose(2, 3))
    with torch.no_grad():
        for bad in (0, 9, -1, 2.0, True, None, '5'):
            with pytest.raises(ValueError, match='levels'):
                F.color_fix_wavelet(sr, lr, levels=bad)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            F.plane_moments(sr)
        with pytest.raises(ValueError, match='NCHW'):
            F.plane_moments(sr[0])
    with pytest.raises(RuntimeError, match='inference-only'):
        F.plane_moments(sr.clone().requires_grad_(True))


def test_abi_refuses_bad_color_fix_arguments_without_a_gpu():
    """Fake pointers: every call below must fail in argument validation (a missed check would fault here, not on a device)."""
    from torchsr_amd import _lib
    if torch.cuda.is_available():
        pytest.skip('fake pointers: argument validation is exercised where a missed check cannot reach a device')
    lib = _lib.lib()
    a, b, c, d = 0x1000000, 0x2000000, 0x3000000, 0x4000000  # 16 MiB apart; never dereferenced

    def message():
        buf = C.create_string_buffer(512)
        lib.srx_last_error(buf, 512)
        return buf.value.decode()

    def level(what, src=a, sub=b, add=c, dst=d, planes=3, H=8, W=12, radius=4):
        rc = lib.srx_color_fix_wavelet_level(src, sub, add, dst, planes, H, W, radius, None)
        return rc != 0 and what in message() and 'color_fix_wavelet_level' in message()

    for name in ('src', 'dst'):
        assert level('null pointer', **{name: None}), name
    for name in ('planes', 'H', 'W'):
        for v in (0, -4):
            assert level('positive', **{name: v}), (name, v)
    for r in (0, -1, 32769, 1 << 30):
        assert level('radius', radius=r), r
    for name in ('src', 'sub', 'add', 'dst'):
        assert level('aligned', **{name: 0x5000002}), name
    nbytes = 3 * 8 * 12 * 4
    for name in ('src', 'sub', 'add'):
        assert level('overlap', **{name: d}), name                    # in place
        assert level('overlap', **{name: d + nbytes - 4}), name       # starts on dst's last element
        assert level('overlap', **{name: d - nbytes + 4}), name       # its last element on dst's first
    assert level('overlap', planes=1 << 20, H=64, W=64)                # 16 GiB each: the ranges meet
    assert level('2^31', H=1 << 16, W=1 << 15)
    assert level('2^28', planes=1 << 28, H=1, W=1)

    def moments(what, x=a, planes=3, H=8, W=12, part=b, n=None, stats=c):
        n = 3 * lib.srx_plane_moments_blocks(8, 12) * 2 if n is None else n
        rc = lib.srx_plane_moments(x, planes, H, W, part, n, stats, None)
        return rc != 0 and what in message() and 'plane_moments' in message()

    assert lib.srx_plane_moments_blocks(8, 12) == 1 and lib.srx_plane_moments_blocks(4320, 7680) == 512
    assert lib.srx_plane_moments_blocks(0, 4) == 0 and lib.srx_plane_moments_blocks(4, -1) == 0
    assert lib.srx_plane_moments_blocks(1 << 16, 1 << 15) == 0
    for name in ('x', 'part', 'stats'):
        assert moments('null pointer', **{name: None}), name
    for name in ('planes', 'H', 'W'):
        for v in (0, -4):
            assert moments('positive', **{name: v}), (name, v)
    assert moments('aligned', x=0x5000002) and moments('aligned', part=0x5000004) and moments('aligned', stats=0x5000004)
    assert moments('workspace holds', n=5)
    assert moments('overlap', part=a + 8) and moments('overlap', stats=a + nbytes - 8) and moments('overlap', stats=b)
    assert moments('2^31', H=1 << 16, W=1 << 15, n=1 << 40)
    assert moments('2^28', planes=1 << 28, H=1, W=1, n=1 << 40)

    def apply(what, sr=a, dst=b, planes=3, H=8, W=12, st_sr=c, st_lr=d):
        rc = lib.srx_color_fix_adain_apply(sr, dst, planes, H, W, st_sr, st_lr, None)
        return rc != 0 and what in message() and 'color_fix_adain_apply' in message()

    for name in ('sr', 'dst', 'st_sr', 'st_lr'):
        assert apply('null pointer', **{name: None}), name
    for name in ('planes', 'H', 'W'):
        for v in (0, -4):
            assert apply('positive', **{name: v}), (name, v)
    assert apply('aligned', sr=0x5000002) and apply('aligned', dst=0x5000002)
    assert apply('aligned', st_sr=0x5000004) and apply('aligned', st_lr=0x5000004)
    assert apply('overlap', dst=a) and apply('overlap', dst=a + nbytes - 4) and apply('overlap', st_sr=b + 8)
    assert apply('overlap', st_lr=b + nbytes - 8)
    assert apply('2^31', H=1 << 16, W=1 << 15)
    assert apply('2^28', planes=1 << 28, H=1, W=1)
