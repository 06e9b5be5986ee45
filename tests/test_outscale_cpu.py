"""``--outscale`` without a GPU: the resampling tables (``F.resample_tables``) against torch's antialiased bicubic in fp64,
the CLI flag, the refusals of ``upscale(outscale=)`` before the generator runs and those of ``srx_resample_planes`` before
any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

U32 = 2.0 ** -24  # fp32 unit roundoff

AXES = [(1, 1), (5, 3), (7, 2), (16, 16), (96, 48), (76, 57), (44, 66), (37, 11), (53, 97), (64, 4)]


def dense(n_in, n_out):
    """The fp64 table of one axis as a dense [n_out, n_in] matrix."""
    from torchsr_amd import functional as F
    start, weight, k = F.resample_tables(n_in, n_out, dtype='float64')
    m = np.zeros((n_out, n_in))
    for i in range(n_out):
        for t in range(k):
            if weight[i, t] != 0.0:
                m[i, start[i] + t] += weight[i, t]
    return m


def taps(n_in, n_out):
    """``(lo, hi)`` per output, restated from the definition one output at a time."""
    scale = n_in / n_out
    support = 2.0 * scale if scale >= 1.0 else 2.0
    out = []
    for i in range(n_out):
        c = scale * (i + 0.5)
        out.append((max(0, int(c - support + 0.5)), min(n_in, int(c + support + 0.5))))
    return out


@pytest.mark.parametrize('n_in,n_out', AXES)
def test_tables_are_well_formed(n_in, n_out):
    from torchsr_amd import functional as F
    start, weight, k = F.resample_tables(n_in, n_out)
    assert start.dtype == np.int32 and start.shape == (n_out,)
    assert weight.dtype == np.float32 and weight.shape == (n_out, k) and weight.flags['C_CONTIGUOUS']
    spans = taps(n_in, n_out)
    assert k == max(hi - lo for lo, hi in spans) and 1 <= k <= 66
    w64 = F.resample_tables(n_in, n_out, dtype='float64')[1]
    for i, (lo, hi) in enumerate(spans):
        count = hi - lo
        assert start[i] == lo >= 0 and start[i] + count <= n_in and count >= 1
        assert (weight[i, count:] == 0.0).all() and (w64[i, count:] == 0.0).all()  # padded taps: exactly 0
        assert abs(float(weight[i].astype(np.float64).sum()) - 1.0) <= k * U32
        assert abs(w64[i].sum() - 1.0) <= (k + 1) * 2.0 ** -53 * np.abs(w64[i]).sum()
        assert np.array_equal(weight[i], w64[i].astype(np.float32))  # rounded once
    if n_in == n_out:
        assert np.array_equal(dense(n_in, n_out), np.eye(n_in))
        if n_in > 4:  # away from the borders: the four taps of the cubic at -1, 0, 1, 2
            assert weight[n_in // 2].tolist() == [0.0, 1.0, 0.0, 0.0]


@pytest.mark.parametrize('y,x', [(AXES[0], AXES[0])] + list(zip(AXES[1:], AXES[2:] + AXES[1:2])) + [(a, a) for a in AXES[1:3]])
def test_tables_equal_torch_antialiased_bicubic(y, x):
    """``My . x . Mx^T`` against ``F.interpolate(mode='bicubic', antialias=True)`` in fp64: every axis pair of the list once
    as rows and once as columns (reductions, enlargements and mixed cases).  (1, 1) goes with itself only: for a
    [N, C, H, 1] -> [N, C, OH, 1] tensor ATen's CPU kernel returns other values than for the same column inside a wider
    tensor (there it agrees with the tables to 1e-16), so a width of 1 beside a resized height is no reference.)"""
    (h, oh), (w, ow) = y, x
    src = torch.rand(2, 3, h, w, generator=torch.Generator().manual_seed(1000 * h + w), dtype=torch.float64)
    want = torch.nn.functional.interpolate(src, size=(oh, ow), mode='bicubic', antialias=True, align_corners=False)
    got = torch.from_numpy(dense(h, oh)) @ src @ torch.from_numpy(dense(w, ow)).T
    err = (got - want).abs().max().item()
    print(f'{(h, w)} -> {(oh, ow)}: max |tables - torch| = {err:.3e}')
    assert got.shape == want.shape and err <= 1e-12, err


def test_tables_refuse_more_than_16_to_1_and_bad_sizes():
    from torchsr_amd import functional as F
    assert F.resample_tables(64, 4)[2] <= 66
    with pytest.raises(ValueError, match='16:1'):
        F.resample_tables(65, 4)
    for bad in ((0, 4), (4, 0), (-3, 2), (4.0, 2), (4, None), (True, 1)):
        with pytest.raises(ValueError, match='positive int'):
            F.resample_tables(*bad)


def test_resize_refuses_before_the_device():
    from torchsr_amd import functional as F
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match='inference-only'):
        F.resize_bicubic_aa(x.clone().requires_grad_(True), (4, 4))
    with torch.no_grad():
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            F.resize_bicubic_aa(x, (4, 4))
        with pytest.raises(ValueError, match='16:1'):
            F.resize_bicubic_aa(torch.zeros(1, 1, 33, 8), (2, 8))
        for bad in ((0, 4), (4, -1), (4.0, 4), 4, (4, 4, 4)):
            with pytest.raises(ValueError):
                F.resize_bicubic_aa(x, bad)
        with pytest.raises(ValueError, match='NCHW'):
            F.resize_bicubic_aa(x[0], (4, 4))


def test_cli_outscale_flag():
    from torchsr_amd.torchsr import parse_args
    assert parse_args(['test', 'x.png']).outscale is None
    assert parse_args(['test', 'x.png', '--outscale', '2']).outscale == 2.0
    assert parse_args(['test', 'x.png', '--outscale', '1.5']).outscale == 1.5
    assert parse_args(['test', 'x.png', '--outscale', '6']).outscale == 6.0
    args = parse_args(['test', 'x.png', '--outscale', '3', '--self-ensemble', '4', '--precision', 'bf16', '--model', 'esrgan'])
    assert (args.outscale, args.self_ensemble, args.precision, args.model) == (3.0, 4, 'bf16', 'esrgan')
    for bad in ('0', '-1', 'nan', 'abc'):
        with pytest.raises(SystemExit):
            parse_args(['test', 'x.png', '--outscale', bad])


def test_upscale_refuses_bad_outscale_before_the_generator_runs():
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
    for bad in (float('nan'), float('inf'), -float('inf'), 0, 0.0, -2, '2', True, [2]):
        with pytest.raises(ValueError, match='outscale'):
            upscale(stub, x, outscale=bad)
    # 8 x 40 at x4 is 32 x 160: 0.24 gives 2 x 10, exactly 16:1; 0.2 gives 2 x 8 (20:1 along x); 0.05 gives 1 x 2
    for bad in (0.2, 0.05, 1e-9):
        with pytest.raises(ValueError, match='16:1'):
            upscale(stub, x, outscale=bad)
    with pytest.raises(ValueError, match='2\\^31'):
        upscale(stub, x, outscale=1e4)
    with pytest.raises(ValueError, match='self_ensemble'):  # the other refusals still come before the generator
        upscale(stub, x, outscale=2, self_ensemble=3)
    assert Stub.calls == 0
    with pytest.raises(AssertionError, match='generator'):  # a good one (exactly 16:1) goes on to the generator
        upscale(stub, x, outscale=0.24)
    assert Stub.calls == 1


def test_abi_refuses_bad_resample_arguments_without_a_gpu():
    """Fake pointers: every call below must fail in argument validation (a missed check would fault here, not on a device)."""
    from torchsr_amd import _lib
    if torch.cuda.is_available():
        pytest.skip('fake pointers: argument validation is exercised where a missed check cannot reach a device')
    lib = _lib.lib()
    f = lib.srx_resample_planes
    src, dst, ws = 0x1000000, 0x2000000, 0x3000000  # 16 MiB apart; never dereferenced
    sy, wy, sx, wx = 0x4000000, 0x4100000, 0x4200000, 0x4300000

    def refused(what, src=src, dst=dst, planes=3, H=8, W=8, OH=4, OW=4, sy=sy, wy=wy, Ky=8, sx=sx, wx=wx, Kx=8, ws=ws, nws=None):
        nws = 3 * 4 * 8 if nws is None else nws
        rc = f(src, dst, planes, H, W, OH, OW, sy, wy, Ky, sx, wx, Kx, ws, nws, None)
        buf = C.create_string_buffer(512)
        lib.srx_last_error(buf, 512)
        msg = buf.value.decode()
        return rc != 0 and what in msg and 'resample_planes' in msg

    for name in ('src', 'dst', 'ws', 'sy', 'wy', 'sx', 'wx'):
        assert refused('null pointer', **{name: None}), name
    for name in ('planes', 'H', 'W', 'OH', 'OW'):
        assert refused('positive', **{name: 0}), name
        assert refused('positive', **{name: -4}), name
    for name in ('Ky', 'Kx'):
        for k in (0, 67, -1, 1 << 20):
            assert refused('tap counts', **{name: k}), (name, k)
    for name in ('src', 'dst', 'ws', 'sy', 'wy', 'sx', 'wx'):
        assert refused('aligned', **{name: 0x5000002}), name
    assert refused('workspace holds', nws=3 * 4 * 8 - 1)
    assert refused('overlap', dst=src)                                # in place
    assert refused('overlap', dst=src + 3 * 64 * 4 - 4)               # dst starts on src's last element
    assert refused('overlap', src=dst + 3 * 16 * 4 - 4)               # src starts on dst's last element
    assert refused('overlap', ws=src + 4)                             # the workspace inside src
    assert refused('overlap', ws=dst - 3 * 32 * 4 + 4)                # its last element on dst's first
    assert refused('overlap', planes=1 << 20, H=64, W=64, OH=64, OW=32, nws=1 << 40)  # 16 GiB of src: the ranges meet
    big = dict(nws=1 << 62)
    assert refused('2^31', H=1 << 16, W=1 << 15, OH=1 << 12, OW=1 << 11, **big)   # H * W
    assert refused('2^31', H=1 << 12, W=1 << 11, OH=1 << 16, OW=1 << 15, **big)   # OH * OW
    assert refused('2^31', H=1 << 12, W=1 << 16, OH=1 << 15, OW=1 << 12, **big)   # the workspace plane OH * W
    assert refused('2^28', planes=1 << 28, **big)
