"""The compact generator (SRVGGNetCompact) on the GPU: its three kernels through the C ABI, the generator against the fp64
restatement of ``tests/compact_ref.py``, tiled inference, and the command line.

Measured on an MI355X (printed by the tests; DESIGN.md section 3 quotes them): see each test's docstring."""
import functools
import os
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from compact_ref import CompactRef, rounded_forward, seeded_state

pytestmark = pytest.mark.gpu


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


def _rel_l2(a, ref):
    a, ref = a.double().cpu(), ref.double().cpu()
    return ((a - ref).square().sum().sqrt() / ref.square().sum().sqrt().clamp_min(1e-300)).item()


# ------------------------------------------------------------------------------------------------ 1. per-channel PReLU
def _prelu_case(shape, seed):
    g = torch.Generator().manual_seed(seed)
    c = shape[-1]
    x = torch.randn(shape, generator=g)
    x[torch.rand(shape, generator=g) < 0.1] = 0.0          # exact zeros (and -0.0 below): x > 0 is false for both
    x.view(-1)[3] = -0.0
    dy = torch.randn(shape, generator=g)
    slopes = torch.rand(c, generator=g) - 0.3
    slopes[:4] = torch.tensor([0.0, -0.7, 0.25, 1.5])
    return x, dy, slopes


@pytest.fixture(scope='module')
def prelu_refs():
    """torch's own results per case, computed once: forward, dx, dslopes in fp32 (CPU) and dslopes in fp64."""
    out = {}
    for shape, seed in (((2, 5, 7, 64), 1), ((1, 3, 3, 8), 2)):
        x, dy, a = _prelu_case(shape, seed)
        xn, an = x.permute(0, 3, 1, 2).clone().requires_grad_(True), a.clone().requires_grad_(True)
        y = TF.prelu(xn, an)
        y.backward(dy.permute(0, 3, 1, 2))
        d64 = torch.where(x.double() > 0, torch.zeros((), dtype=torch.float64), x.double() * dy.double()).reshape(-1, shape[-1]).sum(0)
        out[shape] = dict(x=x, dy=dy, a=a, y=y.detach().permute(0, 2, 3, 1).contiguous(),
                          dx=xn.grad.permute(0, 2, 3, 1).contiguous(), da32=an.grad.clone(), da64=d64)
    return out


@pytest.mark.parametrize('shape', [(2, 5, 7, 64), (1, 3, 3, 8)])
def test_prelu_channels_kernels(dev, prelu_refs, shape):
    """``srx_prelu_channels_fwd`` / ``_bwd`` against torch: y and dx bit for bit (one multiply each); dslopes at most 4x as far
    from the fp64 sum as torch's fp32 CPU result (floor 1e-6 of the largest gradient); two calls the same bits; accumulate
    adds.  Measured: see the printed ratio."""
    from torchsr_amd import _lib
    L = _lib.lib()
    r = prelu_refs[shape]
    c = shape[-1]
    m = r['x'].numel() // c
    x, dy, a = r['x'].to(dev), r['dy'].to(dev), r['a'].to(dev)
    y = torch.full_like(x, float('nan'))
    _lib.call('srx_prelu_channels_fwd', x.data_ptr(), a.data_ptr(), y.data_ptr(), m, c, c, _stream())
    assert torch.equal(_bits(y.cpu()), _bits(r['y']))
    xi = x.clone()  # in place
    _lib.call('srx_prelu_channels_fwd', xi.data_ptr(), a.data_ptr(), xi.data_ptr(), m, c, c, _stream())
    assert torch.equal(_bits(xi.cpu()), _bits(r['y']))
    nws = L.srx_prelu_channels_ws_floats(m, c)
    assert nws > 0
    ws = torch.empty((nws + 1) // 2, dtype=torch.float64, device=dev)
    outs = []
    for _ in range(2):
        dx = torch.full_like(x, float('nan'))
        da = torch.full((c,), float('nan'), device=dev)
        ws.fill_(float('nan'))
        _lib.call('srx_prelu_channels_bwd', dy.data_ptr(), x.data_ptr(), a.data_ptr(), dx.data_ptr(), da.data_ptr(), 0, m, c, c,
                  ws.data_ptr(), nws, _stream())
        outs.append((dx.cpu(), da.cpu()))
    assert torch.equal(_bits(outs[0][0]), _bits(r['dx']))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
    top = r['da64'].abs().max().item()
    e_gpu = (outs[0][1].double() - r['da64']).abs().max().item() / top
    e_cpu = (r['da32'].double() - r['da64']).abs().max().item() / top
    print(f'prelu_channels dslopes {shape}: GPU {e_gpu:.3e}, torch fp32 CPU {e_cpu:.3e} of the largest gradient; '
          f'ratio {e_gpu / max(e_cpu, 1e-300):.3f}')
    assert e_gpu <= max(4 * e_cpu, 1e-6), (e_gpu, e_cpu)
    # accumulate = 1 adds to what is there
    acc = torch.arange(c, dtype=torch.float32, device=dev) * 0.5 - 3
    before = acc.clone()
    _lib.call('srx_prelu_channels_bwd', dy.data_ptr(), x.data_ptr(), a.data_ptr(), dx.data_ptr(), acc.data_ptr(), 1, m, c, c,
              ws.data_ptr(), nws, _stream())
    assert torch.equal(_bits(acc.cpu()), _bits((before + outs[0][1].to(dev)).cpu()))


def test_prelu_channels_strided_rows(dev):
    """C < Cs: the channels past C pass through (forward: x, backward: dy) and take no part in the slope sums."""
    from torchsr_amd import _lib
    g = torch.Generator().manual_seed(5)
    m, c, cs = 37, 8, 12
    x, dy, a = torch.randn(m, cs, generator=g), torch.randn(m, cs, generator=g), torch.rand(c, generator=g) - 0.5
    xd, dyd, ad = x.to(dev), dy.to(dev), a.to(dev)
    y = torch.empty_like(xd)
    _lib.call('srx_prelu_channels_fwd', xd.data_ptr(), ad.data_ptr(), y.data_ptr(), m, c, cs, _stream())
    want = x.clone()
    want[:, :c] = torch.where(x[:, :c] > 0, x[:, :c], a * x[:, :c])
    assert torch.equal(_bits(y.cpu()), _bits(want))
    nws = _lib.lib().srx_prelu_channels_ws_floats(m, c)
    ws = torch.empty((nws + 1) // 2, dtype=torch.float64, device=dev)
    dx, da = torch.empty_like(xd), torch.empty(c, device=dev)
    _lib.call('srx_prelu_channels_bwd', dyd.data_ptr(), xd.data_ptr(), ad.data_ptr(), dx.data_ptr(), da.data_ptr(), 0, m, c, cs,
              ws.data_ptr(), nws, _stream())
    wdx = dy.clone()
    wdx[:, :c] = torch.where(x[:, :c] > 0, dy[:, :c], a * dy[:, :c])
    assert torch.equal(_bits(dx.cpu()), _bits(wdx))
    wda = torch.where(x[:, :c].double() > 0, torch.zeros((), dtype=torch.float64), (x[:, :c].double() * dy[:, :c].double())).sum(0)
    assert (da.cpu().double() - wda).abs().max().item() <= 1e-6 * wda.abs().max().item()


def test_prelu_channels_refusals_launch_nothing(dev):
    """Every refusal returns non-zero with ``srx_last_error`` set and leaves the outputs as they were."""
    from torchsr_amd import _lib
    L = _lib.lib()
    m, c = 12, 8
    x = torch.randn(m, c, device=dev)
    a = torch.rand(c, device=dev)
    y = torch.full_like(x, 7.0)
    dx, da = torch.full_like(x, 7.0), torch.full((c,), 7.0, device=dev)
    nws = L.srx_prelu_channels_ws_floats(m, c)
    ws = torch.empty((nws + 1) // 2, dtype=torch.float64, device=dev)
    s = _stream()
    fwd = lambda xp, ap, yp, mm, cc, cs: L.srx_prelu_channels_fwd(xp, ap, yp, mm, cc, cs, s)  # noqa: E731
    bwd = lambda dyp, xp, ap, dxp, dap, mm, cc, cs, wp, n: L.srx_prelu_channels_bwd(dyp, xp, ap, dxp, dap, 0, mm, cc, cs, wp, n, s)  # noqa: E731
    P = lambda t: t.data_ptr()  # noqa: E731
    big = torch.zeros(1, 1024, device=dev)
    cases = [
        (fwd(None, P(a), P(y), m, c, c), 'null'), (fwd(P(x), None, P(y), m, c, c), 'null'), (fwd(P(x), P(a), None, m, c, c), 'null'),
        (fwd(P(x), P(a), P(y), m, 6, 8), 'multiples of 4'), (fwd(P(x), P(a), P(y), m, 12, 8), 'exceeds'),
        (fwd(P(big), P(big), P(big), 1, 516, 1024), 'at most'),
        (bwd(None, P(x), P(a), P(dx), P(da), m, c, c, P(ws), nws), 'null'),
        (bwd(P(x), P(x), P(a), P(dx), None, m, c, c, P(ws), nws), 'null'),
        (bwd(P(x), P(x), P(a), P(dx), P(da), m, c, c, None, nws), 'null'),
        (bwd(P(x), P(x), P(a), P(dx), P(da), m, 6, 8, P(ws), nws), 'multiples of 4'),
        (bwd(P(x), P(x), P(a), P(dx), P(da), m, 12, 8, P(ws), nws), 'exceeds'),
        (bwd(P(big), P(big), P(big), P(big), P(big), 1, 516, 1024, P(ws), 1 << 20), 'at most'),
        (bwd(P(x), P(x), P(a), P(dx), P(da), m, c, c, P(ws), nws - 1), 'workspace'),
    ]
    for i, (rc, _) in enumerate(cases):
        assert rc != 0, i
    # the message of the last refusal, and one more to see the message follow the call
    assert 'workspace' in _lib.last_error()
    assert fwd(P(x), P(a), P(y), m, 6, 8) != 0 and 'multiples of 4' in _lib.last_error()
    assert L.srx_prelu_channels_ws_floats(0, 8) == 0
    torch.cuda.synchronize()
    assert float(y.min()) == 7.0 == float(y.max()) and float(dx.min()) == 7.0 == float(dx.max()) and float(da.min()) == 7.0
    assert float(big.abs().max()) == 0.0


# ------------------------------------------------------------------------------------ 1b. per-channel PReLU at its launch limits
PC_FWD_BLOCKS, PC_BWD_BLOCKS, PC_ROWS = 8192, 1024, 64      # compact.hip: the forward's grid cap, the backward's, rows per workgroup
# (M, C, Cs).  180001 x 48: Q = 12 quads per row, 2 160 012 quads on 8192 x 256 lanes -- the grid-stride loop is entered, its
# column step is 8192 * 256 mod 12 = 8 and the last pass is partial; backward: 1024 workgroups of 176 rows, the last ones short or
# empty.  140000 x 64: the Q = 16 twin whose column step is 0; 137 rows per workgroup.
PRELU_LIMITS = [(180001, 48, 48), (140000, 64, 64)]
# backward only: Q = 256 (one row per pass) with C < Cs pass-through channels and C = 512; the training step's own launch
PRELU_BWD_ONLY = [(130, 512, 1024), (65536, 64, 64)]


@functools.lru_cache(maxsize=None)
def _prelu_limit_case(m, c, cs):
    """Operands and torch's results on the CPU, once per shape: y and dx in fp32 (one multiply each: bit for bit), dslopes as the fp64
    sum with the sum of the terms' magnitudes for its bound.  Channels [c, cs) pass through."""
    g = torch.Generator().manual_seed(m + 7 * c + cs)
    x = torch.randn(m, cs, generator=g)
    x[torch.rand(m, cs, generator=g) < 0.1] = 0.0            # exact zeros and -0.0: x > 0 is false for both
    x.view(-1)[3::1001] = -0.0
    dy = torch.randn(m, cs, generator=g)
    a = torch.rand(c, generator=g) * 2 - 0.5
    a[:4] = torch.tensor([0.0, -0.7, 0.25, 1.5])
    old = torch.randn(c, generator=g) * 3
    xc, dyc = x[:, :c], dy[:, :c]
    y, dx = x.clone(), dy.clone()
    y[:, :c] = torch.where(xc > 0, xc, a * xc)
    dx[:, :c] = torch.where(xc > 0, dyc, a * dyc)
    terms = torch.where(xc > 0, torch.zeros((), dtype=torch.float64), xc.double() * dyc.double())
    return dict(x=x, dy=dy, a=a, old=old, y=y, dx=dx, da64=terms.sum(0), mag=terms.abs().sum(0))


@pytest.mark.parametrize('m,c,cs', PRELU_LIMITS)
def test_prelu_channels_fwd_grid_stride_loop(dev, m, c, cs):
    """``srx_prelu_channels_fwd`` with more quads than 8192 x 256 lanes: bit for bit ``torch.where(x > 0, x, a * x)``, out of place
    and in place, nothing written outside y."""
    from guarded import SENTINEL, Guarded
    from torchsr_amd import _lib
    q, lanes = cs // 4, PC_FWD_BLOCKS * 256
    total = m * q
    assert total > lanes and total % lanes != 0 and lanes % q == (8 if q == 12 else 0)
    r = _prelu_limit_case(m, c, cs)
    x, a, want = r['x'].to(dev), r['a'].to(dev), r['y'].to(dev)
    y = Guarded(dev, (m, cs), margin=SENTINEL)
    _lib.call('srx_prelu_channels_fwd', x.data_ptr(), a.data_ptr(), y.ptr(), m, c, cs, _stream())
    assert torch.equal(_bits(y.t), _bits(want)) and y.margins_unchanged()
    xi = Guarded(dev, (m, cs), src=x, margin=SENTINEL)
    _lib.call('srx_prelu_channels_fwd', xi.ptr(), a.data_ptr(), xi.ptr(), m, c, cs, _stream())
    assert torch.equal(_bits(xi.t), _bits(want)) and xi.margins_unchanged()
    assert torch.equal(_bits(x.cpu()), _bits(r['x']))          # the input of the out-of-place call is untouched


@pytest.mark.parametrize('m,c,cs', PRELU_LIMITS + PRELU_BWD_ONLY)
def test_prelu_channels_bwd_at_its_launch_limits(dev, m, c, cs):
    """``srx_prelu_channels_bwd`` on 1024 workgroups of more than 64 rows (the last ones short), at Q = 256 with pass-through
    channels, and at the training step's own size: dx bit for bit; dslopes against the fp64 sum.  The kernel's partial sums are
    fp64 (the products x * dy are exact there) and only the conversion of the total and the accumulating add round to fp32, so

        |dslopes - ref64| <= 2^-24 |ref64| + M 2^-52 sum |x dy|     (+ 2^-24 |old + ref64| when accumulating)

    -- derived from the arithmetic, not measured.  Two calls give the same bits; the workspace has exactly the queried size and
    lies, like every output, between sentinel bands."""
    from guarded import SENTINEL, Guarded
    from torchsr_amd import _lib
    L = _lib.lib()
    nb = min(-(-m // PC_ROWS), PC_BWD_BLOCKS)
    rows_per_block = -(-m // nb)
    if (m, c, cs) in PRELU_LIMITS:
        assert nb == PC_BWD_BLOCKS and rows_per_block > PC_ROWS and nb * rows_per_block > m
    elif cs == 1024:
        assert cs // 4 == 256 and c == 512 and c < cs and nb > 2
    else:
        assert nb == PC_BWD_BLOCKS and rows_per_block == PC_ROWS and nb * rows_per_block == m
    r = _prelu_limit_case(m, c, cs)
    x, dy, a = r['x'].to(dev), r['dy'].to(dev), r['a'].to(dev)
    want_dx = r['dx'].to(dev)
    nws = L.srx_prelu_channels_ws_floats(m, c)
    assert nws == nb * c * 2
    base = 2.0 ** -24 * r['da64'].abs() + m * 2.0 ** -52 * r['mag']
    outs = []
    for accumulate in (0, 0, 1):
        ws = Guarded(dev, (nws,), margin=SENTINEL, margin_floats=256)
        dx = Guarded(dev, (m, cs), margin=SENTINEL)
        da = Guarded(dev, (c,), src=r['old'].to(dev) if accumulate else None, margin=SENTINEL, margin_floats=64)
        _lib.call('srx_prelu_channels_bwd', dy.data_ptr(), x.data_ptr(), a.data_ptr(), dx.ptr(), da.ptr(), accumulate, m, c, cs,
                  ws.ptr(), nws, _stream())
        torch.cuda.synchronize()
        assert ws.margins_unchanged() and dx.margins_unchanged() and da.margins_unchanged()
        assert torch.equal(_bits(dx.t), _bits(want_dx)), accumulate
        got = da.t.cpu().double()
        assert torch.isfinite(got).all()
        ref = r['da64'] + (r['old'].double() if accumulate else 0.0)
        bound = base + (2.0 ** -24 * ref.abs() if accumulate else 0.0)
        err = (got - ref).abs()
        print(f'prelu_channels_bwd {(m, c, cs)} accumulate {accumulate}: {nb} workgroups of {rows_per_block} rows, worst |err| / bound '
              f'{float((err / bound.clamp_min(1e-300)).max()):.3f}')
        assert bool((err <= bound).all()), (accumulate, float((err / bound.clamp_min(1e-300)).max()))
        outs.append(da.t.clone())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))


# ------------------------------------------------------------------------------------------------ 2. the tail kernel
@pytest.mark.parametrize('w', [64, 65, 131])
@pytest.mark.parametrize('s', [2, 3, 4])
def test_shuffle_add_nearest_block_decode(dev, s, w):
    """``srx_shuffle_add_nearest_fwd`` / ``_bwd`` on N = 3 images of h = 4 rows of one, two and three 64-pixel segments (the last
    ragged): the block index is decoded into (segment, row, image) with all three above 1.  Scales 2, 3 and 4 from an fp32, a bf16
    and an fp16 source with channel stride 64 and NaN behind the 3 s^2 channels; backward into the tight stride and into 64.  Bit
    for bit ``pixel_shuffle + interpolate(nearest)`` / ``pixel_unshuffle``; channel 3 and the padding channels zero."""
    from guarded import SENTINEL, Guarded
    from torchsr_amd import _lib, functional as F
    n, h, k = 3, 4, 3 * s * s
    assert -(-w // 64) == {64: 1, 65: 2, 131: 3}[w]
    g = torch.Generator().manual_seed(100 * s + w)
    t = torch.randn(n, h, w, 64, generator=g)
    x = torch.rand(n, 3, h, w, generator=g)
    dy = torch.randn(n, 3, h * s, w * s, generator=g)
    x4 = F.to_nhwc(x.to(dev), 4)
    up = TF.interpolate(x, scale_factor=s, mode='nearest')
    for code, cast in ((0, lambda v: v), (1, lambda v: v.bfloat16()), (2, lambda v: v.half())):
        td = cast(t).to(dev)
        td[..., k:] = float('nan')                      # garbage behind the channels: never read into the result
        y4 = Guarded(dev, (n, h * s, w * s, 4), margin=SENTINEL)
        _lib.call('srx_shuffle_add_nearest_fwd', td.data_ptr(), code, 64, x4.data_ptr(), y4.ptr(), n, h, w, s, _stream())
        want = TF.pixel_shuffle(cast(t[..., :k]).float().permute(0, 3, 1, 2), s) + up
        got = y4.t.cpu()
        assert torch.equal(_bits(got[..., :3].permute(0, 3, 1, 2)), _bits(want)), code
        assert float(got[..., 3].abs().max()) == 0.0 and y4.margins_unchanged(), code
    dy4 = F.to_nhwc(dy.to(dev), 4)
    want_dt = TF.pixel_unshuffle(dy, s).permute(0, 2, 3, 1).contiguous()
    for cs_b in sorted({(k + 3) // 4 * 4, 64}):
        dt = Guarded(dev, (n, h, w, cs_b), margin=SENTINEL)
        _lib.call('srx_shuffle_add_nearest_bwd', dy4.data_ptr(), dt.ptr(), cs_b, n, h, w, s, _stream())
        got = dt.t.cpu()
        assert torch.equal(_bits(got[..., :k]), _bits(want_dt)), cs_b
        assert cs_b == k or float(got[..., k:].abs().max()) == 0.0
        assert dt.margins_unchanged(), cs_b


@pytest.fixture(scope='module')
def tail_refs():
    out = {}
    for s in (2, 4):
        g = torch.Generator().manual_seed(10 + s)
        k = 3 * s * s
        t = torch.randn(2, 5, 7, 64, generator=g)      # channels k .. 63: garbage the kernel must not read into the result
        x = torch.rand(2, 3, 5, 7, generator=g)
        dy = torch.randn(2, 3, 5 * s, 7 * s, generator=g)
        refs = {}
        for name, cast in (('fp32', lambda v: v), ('bf16', lambda v: v.bfloat16().float()), ('fp16', lambda v: v.half().float())):
            tn = cast(t[..., :k]).permute(0, 3, 1, 2).clone().requires_grad_(True)
            y = TF.pixel_shuffle(tn, s) + TF.interpolate(x, scale_factor=s, mode='nearest')
            y.backward(dy)
            refs[name] = (y.detach(), tn.grad.permute(0, 2, 3, 1).contiguous())
        out[s] = dict(t=t, x=x, dy=dy, refs=refs)
    return out


@pytest.mark.parametrize('s', [2, 4])
@pytest.mark.parametrize('kind', ['fp32', 'bf16', 'fp16'])
def test_shuffle_add_nearest_kernels(dev, tail_refs, s, kind):
    """``srx_shuffle_add_nearest_fwd`` is ``pixel_shuffle(t[..., :3 s^2]) + interpolate(x, nearest)`` bit for bit (fp32 source
    with channel stride 48, 16-bit sources with stride 64 and garbage behind the channels), channel
    3 zero; ``_bwd`` is torch autograd's gradient bit for bit with zero padding channels."""
    from torchsr_amd import _lib, functional as F
    r = tail_refs[s]
    k = 3 * s * s
    n, h, w = 2, 5, 7
    if kind == 'fp32':
        cs = 48  # s = 4: no padding at all; s = 2: 36 channels of garbage behind the 12
        td = r['t'][..., :cs].contiguous().to(dev)
        td[..., k:] = float('nan')
    else:
        cs = 64
        td = (r['t'].bfloat16() if kind == 'bf16' else r['t'].half()).to(dev)
        td[..., k:] = float('nan')  # garbage behind the 3 s^2 channels
    x4 = F.to_nhwc(r['x'].to(dev), 4)
    y4 = torch.full((n, h * s, w * s, 4), float('nan'), device=dev)
    _lib.call('srx_shuffle_add_nearest_fwd', td.data_ptr(), {'fp32': 0, 'bf16': 1, 'fp16': 2}[kind], cs, x4.data_ptr(), y4.data_ptr(),
              n, h, w, s, _stream())
    want, want_dt = r['refs'][kind]
    got = y4.cpu()
    assert torch.equal(_bits(got[..., :3].permute(0, 3, 1, 2)), _bits(want))
    assert float(got[..., 3].abs().max()) == 0.0
    # the autograd Function gives the same tensor
    assert torch.equal(F.shuffle_add_nearest(td, x4, s), y4)
    if kind == 'fp32':
        dy4 = F.to_nhwc(r['dy'].to(dev), 4)
        for cs_b in sorted({k, 48, 64}):
            dt = torch.full((n, h, w, cs_b), float('nan'), device=dev)
            _lib.call('srx_shuffle_add_nearest_bwd', dy4.data_ptr(), dt.data_ptr(), cs_b, n, h, w, s, _stream())
            assert torch.equal(_bits(dt.cpu()[..., :k]), _bits(want_dt))
            if cs_b > k:
                assert float(dt[..., k:].abs().max()) == 0.0
        tg = td.clone().requires_grad_(True)
        F.shuffle_add_nearest(tg, x4, s).backward(dy4)
        assert torch.equal(_bits(tg.grad.cpu()[..., :k]), _bits(want_dt))
        assert k == cs or float(tg.grad[..., k:].abs().max()) == 0.0


def test_shuffle_add_nearest_segments_and_refusals(dev):
    """A row longer than one 64-pixel segment with a ragged last one, scale 3, and what the entry points refuse."""
    from torchsr_amd import _lib, functional as F
    L = _lib.lib()
    g = torch.Generator().manual_seed(3)
    for s, w in ((3, 70), (4, 131)):
        k, cs = 3 * s * s, (3 * s * s + 3) // 4 * 4
        t = torch.randn(1, 3, w, cs, generator=g)
        x = torch.rand(1, 3, 3, w, generator=g)
        y4 = F.shuffle_add_nearest(t.to(dev), F.to_nhwc(x.to(dev), 4), s)
        want = TF.pixel_shuffle(t[..., :k].permute(0, 3, 1, 2), s) + TF.interpolate(x, scale_factor=s, mode='nearest')
        assert torch.equal(_bits(y4.cpu()[..., :3].permute(0, 3, 1, 2)), _bits(want))
        dy = torch.randn(1, 3, 3 * s, w * s, generator=g)
        dt = torch.empty(1, 3, w, cs, device=dev)
        dy4 = F.to_nhwc(dy.to(dev), 4)
        _lib.call('srx_shuffle_add_nearest_bwd', dy4.data_ptr(), dt.data_ptr(), cs, 1, 3, w, s, _stream())
        assert torch.equal(_bits(dt.cpu()[..., :k].permute(0, 3, 1, 2)), _bits(TF.pixel_unshuffle(dy, s)))
    t = torch.zeros(1, 2, 2, 48, device=dev)
    x4 = torch.zeros(1, 2, 2, 4, device=dev)
    y4 = torch.full((1, 8, 8, 4), 7.0, device=dev)
    st = _stream()
    for args in ((None, 0, 48, x4.data_ptr(), y4.data_ptr(), 1, 2, 2, 4), (t.data_ptr(), 3, 48, x4.data_ptr(), y4.data_ptr(), 1, 2, 2, 4),
                 (t.data_ptr(), 0, 44, x4.data_ptr(), y4.data_ptr(), 1, 2, 2, 4), (t.data_ptr(), 0, 48, x4.data_ptr(), y4.data_ptr(), 1, 2, 2, 5),
                 (t.data_ptr(), 0, 48, x4.data_ptr(), y4.data_ptr(), 1, 2, 2, 1), (t.data_ptr(), 0, 14, x4.data_ptr(), y4.data_ptr(), 1, 2, 2, 2)):
        assert L.srx_shuffle_add_nearest_fwd(*args, st) != 0
    assert L.srx_shuffle_add_nearest_bwd(y4.data_ptr(), t.data_ptr(), 40, 1, 2, 2, 4, st) != 0
    assert 'channel stride' in _lib.last_error()
    torch.cuda.synchronize()
    assert float(y4.min()) == 7.0 == float(y4.max())


# ------------------------------------------------------------------------------------------------ 3. the _slopes layer
@pytest.mark.parametrize('kind', ['bf16', 'fp16'])
@pytest.mark.parametrize('res', [False, True])
def test_c64_per_channel_slopes(dev, kind, res):
    """``srx_conv3x3_c64_{bf16,f16}_fwd_slopes`` on ``[1, 9, 11, 64]`` against fp64 of the rounded operands, held to the bound
    of the scalar layer's tests (test_ops_gpu.py::test_bf16_native_conv3x3_c64: half a bf16 ulp * 1.001 + 2e-6 of the largest
    value; test_fp16_inference_gpu.py::test_fp16_conv3x3_c64: half an fp16 ulp + 2e-5); with all 64 slopes equal the result
    is the scalar entry point's, bit for bit."""
    from torchsr_amd import _lib
    L = _lib.lib()
    s = _stream()
    n, h, w = 1, 9, 11
    g = torch.Generator().manual_seed(77)
    dt = torch.bfloat16 if kind == 'bf16' else torch.float16
    rnd = lambda v: v.to(dt).double()  # noqa: E731
    x = (torch.rand(n, 64, h, w, generator=g) - 0.5).to(dt)
    wt = torch.randn(64, 64, 3, 3, generator=g) * (2.0 / 576) ** 0.5
    b = torch.randn(64, generator=g) * 0.1
    slopes = torch.rand(64, generator=g) * 2 - 0.5
    slopes[:4] = torch.tensor([0.0, -0.7, 0.25, 1.5])
    skip = (torch.rand(n, 64, h, w, generator=g) - 0.5).to(dt) if res else None
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    sd = None if skip is None else skip.permute(0, 2, 3, 1).contiguous().to(dev)
    pk = torch.empty(L.srx_conv3x3_c64_bf16_packed_bytes(64), dtype=torch.uint8, device=dev)
    sfx = 'f16' if kind == 'fp16' else 'bf16'
    wd, bd = wt.to(dev), b.to(dev)  # (held: the pack reads them on the stream)
    _lib.call(f'srx_conv3x3_c64_{sfx}_pack', wd.data_ptr(), bd.data_ptr(), None, 64, 0, pk.data_ptr(), s)

    def run(sl):
        y = torch.full((n, h, w, 64), float('nan'), dtype=dt, device=dev)
        _lib.call(f'srx_conv3x3_c64_{sfx}_fwd_slopes', n, h, w, 64, 0, xd.data_ptr(), pk.data_ptr(), sl.data_ptr(),
                  None if sd is None else sd.data_ptr(), y.data_ptr(), 64, s)
        return y

    y = run(slopes.to(dev))
    z = TF.conv2d(x.double(), rnd(wt), b.double(), 1, 1)
    z = torch.where(z > 0, z, z * slopes.double().view(1, -1, 1, 1))
    if skip is not None:
        z = z + skip.double()
    got = y.permute(0, 3, 1, 2).float().cpu().double()
    assert torch.isfinite(got).all()
    err = (got - z).abs()
    bound = z.abs() * (2.0 ** -8 * 1.001) + 2e-6 * z.abs().max() if kind == 'bf16' else z.abs() * 2.0 ** -11 + 2e-5 * z.abs().max()
    assert (err <= bound).all(), ((err - bound).max().item(), err.max().item())
    for v in (0.25, -0.5, 1.0):  # the scalar kernel's three activation forms: max(v, v a), the select, none
        ys = torch.full((n, h, w, 64), float('nan'), dtype=dt, device=dev)
        _lib.call(f'srx_conv3x3_c64_{sfx}_fwd', n, h, w, 64, 0, xd.data_ptr(), pk.data_ptr(), v, None if sd is None else sd.data_ptr(),
                  ys.data_ptr(), 64, s)
        assert torch.equal(run(torch.full((64,), v, device=dev)).view(torch.int16), ys.view(torch.int16)), v
    # refusals: no slopes, PixelShuffle
    assert L.srx_conv3x3_c64_bf16_fwd_slopes(n, h, w, 64, 0, xd.data_ptr(), pk.data_ptr(), None, None, y.data_ptr(), 64, s) != 0
    assert L.srx_conv3x3_c64_bf16_fwd_slopes(n, h, w, 256, 2, xd.data_ptr(), pk.data_ptr(), wd.data_ptr(), None, y.data_ptr(), 64, s) != 0


# ------------------------------------------------------------------------------------------------ 4. the generator
NUM_CONV = 3


@pytest.fixture(scope='module')
def gen_refs():
    """The restatement's forward and parameter gradients in fp64 and in fp32 (CPU), once."""
    ref = CompactRef(num_conv=NUM_CONV)
    sd = seeded_state(ref, 4)
    g = torch.Generator().manual_seed(9)
    x = torch.rand(2, 3, 12, 20, generator=g)
    r = torch.randn(2, 3, 48, 80, generator=g)
    out = {'sd': sd, 'x': x, 'r': r}
    for name, dt in (('f64', torch.float64), ('f32', torch.float32)):
        m = CompactRef(num_conv=NUM_CONV).to(dt)
        m.load_state_dict({k: v.to(dt) for k, v in sd.items()})
        y = m(x.to(dt))
        (y * r.to(dt)).sum().backward()
        out[name] = (y.detach(), {k: p.grad.clone() for k, p in m.named_parameters()})
    return out


def _gpu_generator(dev, sd, num_conv=NUM_CONV):
    from torchsr_amd.compact.generator import Generator
    gen = Generator(num_conv=num_conv).to(dev)
    gen.load_state_dict(sd)
    return gen


def test_generator_vs_fp64_restatement(dev, gen_refs):
    """Train-mode forward, every parameter gradient and the eval / no-grad fp32 forward of ``Generator(num_conv=3)`` on
    ``2x3x12x20`` against the fp64 restatement: relative L2 distance at most 4x the fp32 CPU restatement's own distance from
    fp64 (the margin covers MFMA summation order and Winograd).  The measured ratios are printed."""
    from torchsr_amd.test import upscale
    gen = _gpu_generator(dev, gen_refs['sd']).train()
    y64, g64 = gen_refs['f64']
    y32, g32 = gen_refs['f32']
    y = gen(gen_refs['x'].to(dev))
    (y * gen_refs['r'].to(dev)).sum().backward()
    worst = {}

    def hold(name, got, ref64, ref32):
        e, e0 = _rel_l2(got, ref64), _rel_l2(ref32, ref64)
        worst[name] = (e, e0)
        return e <= 4 * e0

    ok = {'train forward': hold('train forward', y.detach(), y64, y32)}
    for k, p in gen.named_parameters():
        assert p.grad is not None, k
        ok[k] = hold(k, p.grad, g64[k], g32[k])
    gen.eval()
    with torch.no_grad():
        ye = upscale(gen, gen_refs['x'].to(dev), precision='fp32')
    ok['eval forward'] = hold('eval forward', ye, y64, y32)
    for k, (e, e0) in worst.items():
        print(f'compact generator {k}: GPU {e:.3e}, fp32 CPU {e0:.3e} from fp64 (relative L2); ratio {e / e0:.3f}')
    bad = [k for k, v in ok.items() if not v]
    assert not bad, {k: worst[k] for k in bad}


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_generator_16bit_chain_vs_rounded_restatement(dev, gen_refs, precision):
    """``upscale(precision='bf16' / 'fp16')``, by the method of test_fp16_inference_gpu.py: every fused layer on its OWN 16-bit
    input against fp64 of the rounded operands -- ``act(conv(x, rnd(w)) + b)`` with per-channel slopes, each stored output
    within half an ulp of the type plus the fp32 sum's floor (the scalar layer's bounds) --, the padded 64 -> 48 tail layer
    with 16 zero channels, the tail kernel bit for bit, and ``upscale`` equal to that chain bit for bit.  End to end against
    the restatement with weights and stored activations rounded to the type: a stored value differs from the restatement's
    only where fp32 summation noise flips a rounding, by one ulp = 2u; five stored layers bound the distance by 10 u of the
    output's range (printed)."""
    from torchsr_amd import functional as F
    from torchsr_amd.test import upscale
    sd, x = gen_refs['sd'], gen_refs['x']
    gen = _gpu_generator(dev, sd).eval()
    dt = torch.bfloat16 if precision == 'bf16' else torch.float16
    u = 2.0 ** -8 if precision == 'bf16' else 2.0 ** -11
    rnd = lambda v: v.to(dt).double()  # noqa: E731
    xd = x.to(dev)
    out = upscale(gen, xd, precision=precision)
    assert out.shape == (2, 3, 48, 80) and torch.isfinite(out).all()
    assert all(m._st.precision == 0 for m in gen.modules() if hasattr(m, '_st'))  # restored
    with torch.no_grad():
        for m in gen.modules():
            if hasattr(m, '_st'):
                m._st.precision = 1 if precision == 'bf16' else F.PRECISION_F16
        try:
            assert gen.native16() == dt
            f = gen.__dict__['_folded']
            x4 = F.to_nhwc(xd, 4)
            nchw = lambda t, c=None: F.to_nchw(t.float(), c).cpu().double()  # noqa: E731
            # the 3-channel 3x3 input conv multiplies the rounded image by rounded weights (as ESRGAN's conv1 does at these
            # precisions); fp32 out, activated in fp32, rounded once
            first = rnd
            y0 = f[0](x4)
            assert y0.dtype == torch.float32
            z = TF.conv2d(first(x), first(sd['body.0.weight']), sd['body.0.bias'].double(), 1, 1)
            z = torch.where(z > 0, z, z * sd['body.1.weight'].double().view(1, -1, 1, 1))
            assert ((nchw(y0) - z).abs().max() / z.abs().max()).item() < 2e-5
            t = F.to_bf16(y0) if precision == 'bf16' else F.to_f16(y0)
            for i, layer in enumerate(f[1:], 1):
                last = i == len(f) - 1
                y = layer(t)
                assert y.dtype == dt and y.shape[3] == 64
                z = TF.conv2d(nchw(t), rnd(sd[f'body.{2 * i}.weight']), sd[f'body.{2 * i}.bias'].double(), 1, 1)
                if not last:
                    z = torch.where(z > 0, z, z * sd[f'body.{2 * i + 1}.weight'].double().view(1, -1, 1, 1))
                got = nchw(y)
                if last:
                    assert float(got[:, 48:].abs().max()) == 0.0  # the 16 zero filters
                    got = got[:, :48]
                err = (got - z).abs()
                bound = z.abs() * (u * 1.001 if precision == 'bf16' else u) + (2e-6 if precision == 'bf16' else 2e-5) * z.abs().max()
                assert (err <= bound).all(), (i, (err - bound).max().item())
                t = y
            y4 = F.shuffle_add_nearest(t, x4, 4)
            want = TF.pixel_shuffle(t[..., :48].float().permute(0, 3, 1, 2), 4) + TF.interpolate(xd, scale_factor=4, mode='nearest')
            assert torch.equal(F.to_nchw(y4, 3), want)
            assert torch.equal(F.to_nchw(y4, 3), out)
        finally:
            for m in gen.modules():
                if hasattr(m, '_st'):
                    m._st.precision = 0
    ref = rounded_forward(sd, x, 4, rnd)
    e = ((out.cpu().double() - ref).abs().max() / ref.abs().max()).item()
    print(f'compact generator {precision} upscale vs the rounded restatement: max error {e:.3e} of the range = {e / u:.2f} u')
    assert e <= 10 * u, e


def test_generator_tail_cut_completes_its_bucket(dev, gen_refs):
    """Data parallel: with the 'g.tail' cut armed (``ddp.BackwardCuts``) the first backward stops in front of body conv
    ``tail_index`` with exactly the gradients of the trainer's tail bucket -- ``body.{tail_index}.weight`` to the end -- complete;
    resuming gives every gradient the bits of the uncut backward."""
    from torchsr_amd import functional as F
    from torchsr_amd.compact.generator import tail_index
    from torchsr_amd.ddp import BackwardCuts
    gen = _gpu_generator(dev, gen_refs['sd']).train()
    x, r = gen_refs['x'].to(dev), gen_refs['r'].to(dev)
    (gen(x) * r).sum().backward()
    want = {k: p.grad.clone() for k, p in gen.named_parameters()}
    gen.zero_grad(set_to_none=True)
    cuts = BackwardCuts(('g.tail',))
    F.cut_hook[0] = cuts
    try:
        (gen(x) * r).sum().backward()
        tail = tail_index(NUM_CONV)
        assert 0 < tail < len(gen.body)
        for k, p in gen.named_parameters():
            assert (p.grad is not None) == (int(k.split('.')[1]) >= tail), k
        assert cuts.pending('g.tail')
        cuts.resume('g.tail')
    finally:
        F.cut_hook[0] = None
    for k, p in gen.named_parameters():
        assert torch.equal(p.grad, want[k]), k


# ------------------------------------------------------------------------------------------------ 5. tiling
def test_compact_tiled_inference_equals_untiled(dev, gen_refs):
    """``num_conv = 3`` (halo 8) on ``1x3x40x150`` with ``max_tile_pixels = 1600``: 2 x 3 tiles of 20 x 64 pixels, each with its
    8-pixel halo, against the untiled call -- the comparison test_cli_gpu.py::test_tiled_inference_equals_untiled makes for
    SRGAN.  The same image through ``self_ensemble=4`` and ``color_fix='adain'``."""
    from torchsr_amd.test import upscale
    gen = _gpu_generator(dev, gen_refs['sd'])
    assert gen.halo == 8
    lr = torch.rand(1, 3, 40, 150, generator=torch.Generator().manual_seed(21)).to(dev)
    whole = upscale(gen, lr, max_tile_pixels=10 ** 9)
    tiled = upscale(gen, lr, max_tile_pixels=1600)
    assert whole.shape == tiled.shape == (1, 3, 160, 600)
    diff = (whole - tiled).abs().max().item()
    print(f'compact tiled vs untiled: max difference {diff:.3e} (range {whole.abs().max().item():.3f})')
    assert diff <= 1e-4 * whole.abs().max().item()
    for p in ('bf16', 'fp16'):  # per-pixel arithmetic of the 16-bit chain does not depend on the tile either
        a, b = upscale(gen, lr, max_tile_pixels=10 ** 9, precision=p), upscale(gen, lr, max_tile_pixels=1600, precision=p)
        assert (a - b).abs().max().item() <= 1e-5 * a.abs().max().item(), p
    ens = upscale(gen, lr, max_tile_pixels=1600, self_ensemble=4)
    fix = upscale(gen, lr, max_tile_pixels=1600, color_fix='adain')
    both = upscale(gen, lr, max_tile_pixels=1600, self_ensemble=4, color_fix='adain', precision='bf16')
    for t in (ens, fix, both):
        assert t.shape == whole.shape and torch.isfinite(t).all()


# ------------------------------------------------------------------------------------------------ 6. command line, captured step
def test_compact_train_then_test_cli(dev, tmp_path, monkeypatch):
    """``train --model compact --num-conv 2`` (one pre-training and one GAN epoch on a tiny synthetic set), ``test``, and
    ``test --weights`` on a Real-ESRGAN-style file holding the same state under ``params_ema``: same pixels."""
    from PIL import Image
    from torchsr_amd.torchsr import main
    monkeypatch.chdir(tmp_path)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'LOCAL_WORLD_SIZE', 'SLURM_NTASKS'):
        monkeypatch.delenv(k, raising=False)
    main(['train', '--model', 'compact', '--num-conv', '2', '--train-dir', 'synthetic:16', '--batch-size', '4', '--epochs', '1',
          '--pretrain-epochs', '1', '--disable-amp', '--seed', '3', '--vgg-weights', 'random'])
    for f in ('compact-psnr-best.pth', 'compact-psnr-latest.pth', 'compact-gan-best.pth', 'compact-gan-latest.pth'):
        assert os.path.exists(f), f
    ckpt = torch.load('compact-gan-best.pth', map_location='cpu')
    assert ckpt['phase'] == 'compact-gan' and list(ckpt['state']) == list(CompactRef(num_conv=2).state_dict())
    Image.fromarray((np.random.RandomState(0).rand(20, 28, 3) * 255).astype('uint8')).save('lr.png')
    main(['test', 'lr.png', '--model', 'compact'])
    first = np.asarray(Image.open('upres-lr.png')).copy()
    assert first.shape == (80, 112, 3)
    os.remove('upres-lr.png')
    torch.save({'params': {k: torch.zeros_like(v) for k, v in ckpt['state'].items()}, 'params_ema': ckpt['state']}, 'published.pth')
    os.remove('compact-gan-best.pth')  # --weights is what is read
    main(['test', 'lr.png', '--model', 'compact', '--weights', 'published.pth'])
    assert np.array_equal(np.asarray(Image.open('upres-lr.png')), first)


def _compact_trainer(dev, sd):
    from oracle.weights import closed_form_state, step_state
    from torchsr_amd.compact.trainer import CompactTrainer
    args = Namespace(disable_amp=False, batch_size=2, epochs=8, gan_checkpoint=None, local_rank=0, pretrain_epochs=1,
                     psnr_checkpoint=None, skip_image_save=True, world_size=1, rank=-1, use_graphs=True, vgg_weights='random',
                     num_conv=NUM_CONV)
    t = CompactTrainer(dev, args, [], [], 2, 2, distributed=False)
    assert t.generator.num_conv == NUM_CONV and t.gen_tail_bucket in t.generator.state_dict()
    t.generator.load_state_dict(sd)
    t.discriminator.load_state_dict(step_state(t.discriminator.state_dict(), 'esrgan.D'))
    t.vgg_loss.features.load_state_dict(closed_form_state(t.vgg_loss.features.state_dict(), prefix='features.'))
    t.generator.train()
    t.discriminator.train()
    return t


def test_compact_captured_step_is_bitwise_reproducible(dev, gen_refs):
    """Two compact trainers from one state (bf16 products, hipGraph replays from the third step): bit-identical losses and
    parameters after four GAN steps -- the new ops capture (no host sync) and reduce in a fixed order."""
    g = torch.Generator().manual_seed(31)
    hr = torch.rand(2, 3, 128, 128, generator=g).to(dev)
    lr = TF.avg_pool2d(hr, 4)
    runs = []
    for _ in range(2):
        t = _compact_trainer(dev, gen_refs['sd'])
        losses = [[v.item() for _k, v in sorted(t.gan_step(lr, hr).items())] for _step in range(4)]
        assert 'gan.all' in t._graphs
        assert all(np.isfinite(v) for step in losses for v in step)
        runs.append((losses, {k: v.clone() for k, v in t.generator.state_dict().items()}))
        del t
    assert runs[0][0] == runs[1][0]
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    moved = [k for k, v in runs[0][1].items() if not torch.equal(v.cpu(), gen_refs['sd'][k])]
    assert len(moved) == len(runs[0][1]), set(runs[0][1]) - set(moved)  # every parameter, slopes included, took a step
