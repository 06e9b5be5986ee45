"""``--discriminator unet`` on the MI355X: the spectral-norm and bilinear kernels, 4x4 stride-2 convs through the existing conv
entry points, the whole ``UNetDiscriminatorSN``, its losses, and the captured GAN step -- against fp64 CPU references
(tests/unet_ref.py, torch.nn.utils.spectral_norm, F.interpolate, F.conv2d).

Tolerances are not taken from the code under test.  Every fp32 comparison is ``max |gpu - ref64| <= bound`` over ALL elements
(nothing is skipped), where ``bound = max(4 * max |ref32 - ref64|, 8 * 2^-23 * max |ref64|)``: four times the error of torch's
own fp32 CPU run of the same reference on the same inputs (another summation order over K up to 8192, other equally valid
roundings in the power iteration, a gradient that divides by sigma twice), with a floor of a few fp32 ulps of the tensor's
largest magnitude.  ``_close`` prints both figures of every comparison before it asserts.  For bf16 products the reference is
the oracle's recipe (oracle/srgan.py, ``_ConvBF16``): the forward rounds each conv's input and (normalised) weight to bf16, the
data gradient dy and the weight, the weight gradient x and dy; conv9 (64 -> 1) keeps fp32 operands in its forward and weight
gradient, conv0 (3 -> 64) in both gradients.  Forward and gradients are compared with that reference by the same rule: four times
its own fp32-against-fp64 error.

Reference errors max |ref32 - ref64| measured on the CPU (seeds as below), one line per comparison; the bound is 4x the figure
or, where that is larger, the floor 8 * 2^-23 * max |ref64| (in brackets):
  spectral norm (8, 36) train:      u 5.5e-08 [5.3e-07]  v 4.2e-08  sigma 7.7e-08  W_sn 3.1e-08  dW 1.4e-07 [1.8e-06]
  spectral norm (64, 576) train:    u 5.0e-08 [3.0e-07]  v 4.0e-08  sigma 1.8e-07  W_sn 2.6e-08  dW 5.1e-07 [2.5e-06]
  spectral norm (512, 4096) train:  u 4.8e-08 [1.4e-07]  v 3.9e-08  sigma 5.6e-08  W_sn 5.6e-09  dW 3.3e-07 [3.2e-06]
  spectral norm, eval:              u, v 0 (unchanged)  sigma 1.0e-09 .. 1.1e-08  W_sn 6.0e-08 .. 3.3e-06  dW 6.5e-07 .. 3.3e-03
                                    (random u and v: sigma ~ 0.02, so W_sn and dW are large; dW floors 8.0e-06 .. 5.5e-03)
  spectral norm, ragged rows:       (100, 44), (520, 68), (1, 576), (3, 8), (256, 4608), (128, 1024) train: u, v 0 .. 1.5e-07
                                    sigma 6.2e-08 .. 3.9e-07  W_sn 7.8e-09 .. 6.3e-08  dW 1.1e-07 .. 5.6e-07; eval: sigma 5.9e-10 .. 2.9e-08
                                    W_sn 1.5e-07 .. 9.2e-05  dW 3.6e-06 .. 4.5e-02 (sigma down to 0.006: W_sn up to 22, dW up to 4.6e+03)
  bilinear x2:                      0 .. 2.4e-07: the floor decides
  conv 4x4 s2 64 -> 128:            y 2.1e-06  dx 1.7e-06  dw 3.6e-05   (the bf16 recipe's reference: 9.8e-07, 9.4e-07, 1.4e-05)
  conv 4x4 s2 256 -> 512:           y 1.7e-06  dx 2.1e-06  dw 7.1e-06   (1.0e-06, 1.0e-06, 3.3e-06)
  conv 3x3 64 -> 1:                 y 1.0e-06  dx 7.7e-08  dw 1.5e-05   (1.1e-06, 6.0e-08, 1.0e-05)
  network 2x3x32x32 train:          logits 5.8e-07 (magnitude 1.0)  dx 7.2e-10 (1.4e-03)  parameter gradients 3e-10 .. 3e-08
                                    (magnitudes 3e-04 .. 5e-02)  u, v 3e-08 .. 9e-08
  network 1x3x24x40 train:          logits 4.7e-07  dx 6.9e-10  parameter gradients 2e-10 .. 3e-08  u, v as above
  network eval / no skips:          logits 5.5e-07 / 5.0e-08  dx 7.7e-10 / 5.1e-11  parameter gradients 3e-10 .. 4e-08 / 2e-10 .. 6e-09
  network, bf16 products:           logits 2.3e-03 (fp32 and fp64 round some operands to different bf16 neighbours)  dx 1.0e-04
                                    parameter gradients 1.7e-05 .. 4.3e-04 (conv9.bias 4.9e-09)  u, v: the fp32 lines (no rounding)
  two fp32 GAN steps (compact / esrgan): the five losses 3e-10 .. 2.2e-07 (bounds 4.2e-08 .. 1.4e-06); u, v after the step 3e-08 .. 9e-08;
                                    parameters after the first step: the Adam criterion in that test's docstring
(a run prints the figures of every comparison: they are recomputed from the references each time).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF
from torch import nn

import unet_ref as R

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23


def _bound(ref32, ref64, extra: float = 0.0) -> float:
    ref64 = torch.as_tensor(ref64, dtype=torch.float64)
    err = (torch.as_tensor(ref32).double() - ref64).abs().max().item()
    return max(4.0 * err, 8.0 * EPS32 * ref64.abs().max().item()) + extra


def _close(what: str, got, ref32, ref64, extra: float = 0.0) -> None:
    got = torch.as_tensor(got).detach().cpu().double().reshape(-1)
    ref64 = torch.as_tensor(ref64).detach().double().reshape(-1)
    ref32 = torch.as_tensor(ref32).detach().double().reshape(-1)
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), what
    bound, err = _bound(ref32, ref64, extra), (got - ref64).abs().max().item()
    print(f'{what}: error {err:.3e}, reference fp32 error {(ref32 - ref64).abs().max().item():.3e}, bound {bound:.3e}, '
          f'largest magnitude {ref64.abs().max().item():.3e}')
    assert err <= bound, (what, err, bound)


# ------------------------------------------------------------------ 1. spectral normalisation
def _sn_module(w, u, v, dtype):
    rows, cols = w.shape
    m = nn.utils.spectral_norm(nn.Linear(cols, rows, bias=False)).to(dtype)
    with torch.no_grad():
        m.weight_orig.copy_(w)
        m.weight_u.copy_(u)
        m.weight_v.copy_(v)
    return m


def _sn_reference(w, u, v, g, train: bool, calls: int = 1):
    """torch's spectral_norm in fp64 and fp32: per call (u, v, sigma, W_sn) and dW of <W_sn, g> for the last call."""
    out = {}
    for dtype in (torch.float64, torch.float32):
        m = _sn_module(w, u, v, dtype).train(train)
        steps = []
        for _ in range(calls):
            m(torch.zeros(1, w.shape[1], dtype=dtype))  # (the forward pre-hook computes m.weight)
            w_sn = m.weight
            uu, vv = m.weight_u.detach().clone(), m.weight_v.detach().clone()
            sigma = torch.dot(uu, torch.mv(m.weight_orig.detach(), vv))
            steps.append((uu, vv, sigma, w_sn.detach().clone()))
        (w_sn * g.to(dtype)).sum().backward()
        out[dtype] = (steps, m.weight_orig.grad.clone())
    return out


# (rows, cols).  The first three fill whole 16-row chunks of pass 1 (sn_wtu_kernel).  Then: 100 rows -- 7 chunks of 15, the last of
# 10; 520 rows -- 32 chunks planned, 17 rows each, so 31 are launched and the workspace keeps a 32nd partial row nobody writes or
# reads; 1 and 3 rows -- fewer than the 4 the uv_keep offset roundup(rows, 4) rounds to; and the network's own 256 x 4608 (conv3's
# 512 x 4096 is above) and 128 x 1024.
SN_CHUNK_SHAPES = [(8, 36), (64, 576), (512, 4096)]
SN_RAGGED_SHAPES = [(100, 44), (520, 68), (1, 576), (3, 8), (256, 4608), (128, 1024)]


@pytest.fixture(scope='module')
def sn_cases():
    cases = {}
    for rows, cols in SN_CHUNK_SHAPES + SN_RAGGED_SHAPES:
        gen = torch.Generator().manual_seed(rows + cols)
        w = torch.randn(rows, cols, generator=gen) * (2.0 / cols) ** 0.5
        u = TF.normalize(torch.randn(rows, generator=gen), dim=0)
        v = TF.normalize(torch.randn(cols, generator=gen), dim=0)
        g = torch.randn(rows, cols, generator=gen)
        cases[(rows, cols)] = (w, u, v, g)
    return cases


def _sn_gpu(dev, w, u, v, g, train: bool, calls: int = 1):
    from torchsr_amd import functional as F
    wd = w.to(dev).requires_grad_(True)
    ud, vd, out = u.to(dev).clone(), v.to(dev).clone(), torch.empty_like(w, device=dev)
    steps = []
    for _ in range(calls):
        w_sn = F.spectral_norm(wd, ud, vd, out, train)
        steps.append((ud.clone(), vd.clone(), w_sn.detach().clone()))
    (dw,) = torch.autograd.grad(w_sn, wd, g.to(dev))
    return steps, dw


def _sn_sigma(dev, w, u, v, train: bool):
    """sigma as ``srx_spectral_norm_fwd`` itself writes it (one call from the given u, v)."""
    from torchsr_amd import _lib
    rows, cols = w.shape
    wd, ud, vd = w.to(dev), u.to(dev).clone(), v.to(dev).clone()
    out, sigma = torch.empty_like(wd), torch.empty(1, device=dev)
    nws = _lib.lib().srx_spectral_norm_ws_floats(rows, cols)
    ws = torch.empty(nws, device=dev)
    _lib.call('srx_spectral_norm_fwd', wd.data_ptr(), ud.data_ptr(), vd.data_ptr(), out.data_ptr(), sigma.data_ptr(), None, rows, cols,
              int(train), ws.data_ptr(), nws, torch.cuda.current_stream().cuda_stream)
    return sigma


@pytest.mark.parametrize('shape', SN_CHUNK_SHAPES + SN_RAGGED_SHAPES)
@pytest.mark.parametrize('train', [True, False])
def test_spectral_norm_forward_and_backward_against_fp64(dev, sn_cases, shape, train):
    w, u, v, g = sn_cases[shape]
    ref = _sn_reference(w, u, v, g, train)
    (steps64, dw64), (steps32, dw32) = ref[torch.float64], ref[torch.float32]
    steps, dw = _sn_gpu(dev, w, u, v, g, train)
    (u64, v64, s64, wsn64), (u32, v32, s32, wsn32) = steps64[0], steps32[0]
    _close(f'sn {shape} train={train} u', steps[0][0], u32, u64)
    _close(f'sn {shape} train={train} v', steps[0][1], v32, v64)
    _close(f'sn {shape} train={train} W_sn', steps[0][2], wsn32, wsn64)
    _close(f'sn {shape} train={train} sigma', _sn_sigma(dev, w, u, v, train), s32, s64)  # the kernel's own output
    _close(f'sn {shape} train={train} dW', dw, dw32, dw64)
    if not train:
        assert torch.equal(steps[0][0].cpu(), u) and torch.equal(steps[0][1].cpu(), v)  # eval: the stored vectors, untouched
    # a second call on the same inputs: the same bits (fixed grids and trees, no atomics)
    steps2, dw2 = _sn_gpu(dev, w, u, v, g, train)
    for a, b in zip(steps[0] + (dw,), steps2[0] + (dw2,)):
        assert torch.equal(a, b)


def test_spectral_norm_sigma_output_and_accumulating_backward(dev, sn_cases):
    """The raw entry points: sigma as written by the kernel, and accumulate = 1 adds dW to what the buffer holds."""
    from torchsr_amd import _lib
    w, u, v, g = sn_cases[(64, 576)]
    ref = _sn_reference(w, u, v, g, True)
    wd, ud, vd, gd = w.to(dev), u.to(dev).clone(), v.to(dev).clone(), g.to(dev)
    out, sigma, keep = torch.empty_like(wd), torch.empty(1, device=dev), torch.empty(64 + 576, device=dev)
    nws = _lib.lib().srx_spectral_norm_ws_floats(64, 576)
    ws = torch.empty(nws, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    _lib.call('srx_spectral_norm_fwd', wd.data_ptr(), ud.data_ptr(), vd.data_ptr(), out.data_ptr(), sigma.data_ptr(), keep.data_ptr(),
              64, 576, 1, ws.data_ptr(), nws, s)
    _close('sn sigma (kernel)', sigma, ref[torch.float32][0][0][2], ref[torch.float64][0][0][2])
    assert torch.equal(keep[:64], ud) and torch.equal(keep[64:], vd)
    base = torch.full_like(wd, 0.5)
    dw0, dw1 = torch.empty_like(wd), base.clone()
    for dw, acc in ((dw0, 0), (dw1, 1)):
        _lib.call('srx_spectral_norm_bwd', gd.data_ptr(), wd.data_ptr(), keep.data_ptr(), keep.data_ptr() + 4 * 64, sigma.data_ptr(),
                  dw.data_ptr(), acc, 64, 576, ws.data_ptr(), nws, s)
    _close('sn dW (kernel)', dw0, ref[torch.float32][1], ref[torch.float64][1])
    assert torch.equal(dw1, dw0 + base)


@pytest.mark.parametrize('shape', SN_CHUNK_SHAPES + SN_RAGGED_SHAPES)
@pytest.mark.parametrize('train', [True, False])
def test_spectral_norm_entry_points_stay_inside_their_buffers(dev, sn_cases, shape, train):
    """``srx_spectral_norm_fwd`` / ``_bwd`` through the C ABI with a workspace of exactly ``srx_spectral_norm_ws_floats`` floats, W_sn,
    uv_keep (``roundup(rows, 4) + cols`` floats) and dW each between two sentinel bands: a write past the chunk partials, past s,
    past v_keep or past the last row fails here.  u, v, sigma, W_sn and dW (through uv_keep) by the module's rule, unchanged."""
    from guarded import SENTINEL, Guarded
    from torchsr_amd import _lib
    rows, cols = shape
    w, u, v, g = sn_cases[shape]
    ref = _sn_reference(w, u, v, g, train)
    (steps64, dw64), (steps32, dw32) = ref[torch.float64], ref[torch.float32]
    (u64, v64, s64, wsn64), (u32, v32, s32, wsn32) = steps64[0], steps32[0]
    chunks = min(-(-rows // 16), 32)
    r4 = (rows + 3) // 4 * 4
    nws = _lib.lib().srx_spectral_norm_ws_floats(rows, cols)
    assert nws == max(chunks * cols + r4, 256), (nws, chunks)
    if shape == (520, 68):      # 17 rows per chunk: 31 chunks are launched, the 32nd partial row stays as it was
        assert -(-rows // -(-rows // chunks)) == chunks - 1
    wd, gd = w.to(dev), g.to(dev)
    s = torch.cuda.current_stream().cuda_stream
    band = dict(margin=SENTINEL, margin_floats=256)
    ud, vd = Guarded(dev, (rows,), src=u.to(dev), **band), Guarded(dev, (cols,), src=v.to(dev), **band)
    out, keep, sigma = Guarded(dev, (rows, cols), **band), Guarded(dev, (r4 + cols,), **band), Guarded(dev, (4,), **band)
    ws = Guarded(dev, (nws,), **band)
    _lib.call('srx_spectral_norm_fwd', wd.data_ptr(), ud.ptr(), vd.ptr(), out.ptr(), sigma.ptr(), keep.ptr(), rows, cols, int(train),
              ws.ptr(), nws, s)
    torch.cuda.synchronize()
    for name, buf in (('u', ud), ('v', vd), ('W_sn', out), ('uv_keep', keep), ('sigma', sigma), ('workspace', ws)):
        assert buf.margins_unchanged(), name
    assert torch.isnan(sigma.t[1:]).all()
    tag = f'sn raw {shape} train={train}'
    _close(f'{tag} u', ud.t, u32, u64)
    _close(f'{tag} v', vd.t, v32, v64)
    _close(f'{tag} sigma', sigma.t[:1], s32, s64)
    _close(f'{tag} W_sn', out.t, wsn32, wsn64)
    assert torch.equal(keep.t[:rows], ud.t) and torch.equal(keep.t[r4:], vd.t)
    if not train:
        assert torch.equal(ud.t.cpu(), u) and torch.equal(vd.t.cpu(), v)
    dws = []
    for _ in range(2):
        ws2, dw = Guarded(dev, (nws,), **band), Guarded(dev, (rows, cols), **band)
        _lib.call('srx_spectral_norm_bwd', gd.data_ptr(), wd.data_ptr(), keep.ptr(), keep.t.data_ptr() + 4 * r4, sigma.ptr(), dw.ptr(), 0,
                  rows, cols, ws2.ptr(), nws, s)
        torch.cuda.synchronize()
        assert ws2.margins_unchanged() and dw.margins_unchanged()
        dws.append(dw.t.clone())
    _close(f'{tag} dW', dws[0], dw32, dw64)
    assert torch.equal(dws[0], dws[1])


def test_three_chained_training_forwards_track_torchs_three(dev, sn_cases):
    w, u, v, g = sn_cases[(64, 576)]
    ref = _sn_reference(w, u, v, g, True, calls=3)
    steps, dw = _sn_gpu(dev, w, u, v, g, True, calls=3)
    for i in range(3):
        (u64, v64, _s, wsn64), (u32, v32, _s32, wsn32) = ref[torch.float64][0][i], ref[torch.float32][0][i]
        _close(f'chained call {i} u', steps[i][0], u32, u64)
        _close(f'chained call {i} v', steps[i][1], v32, v64)
        _close(f'chained call {i} W_sn', steps[i][2], wsn32, wsn64)
    _close('chained dW (vectors of the third call)', dw, ref[torch.float32][1], ref[torch.float64][1])


# ------------------------------------------------------------------ 2. bilinear x2
@pytest.mark.parametrize('h,w,c,cs', [(1, 1, 4, 4), (2, 3, 64, 64), (5, 7, 128, 128), (3, 5, 6, 12)])
def test_bilinear2x_forward_and_backward(dev, h, w, c, cs):
    from torchsr_amd import _lib
    from torchsr_amd import functional as F
    gen = torch.Generator().manual_seed(h * 100 + w * 10 + c)
    x = torch.randn(2, c, h, w, generator=gen)
    dy = torch.randn(2, c, 2 * h, 2 * w, generator=gen)
    refs = {}
    for dtype in (torch.float64, torch.float32):
        xr = x.to(dtype).clone().requires_grad_(True)
        yr = TF.interpolate(xr, scale_factor=2, mode='bilinear', align_corners=False)
        yr.backward(dy.to(dtype))
        refs[dtype] = (yr.detach(), xr.grad)
    nhwc = lambda t: torch.cat([t, torch.full((t.shape[0], cs - c) + tuple(t.shape[2:]), 7.0)], 1).permute(0, 2, 3, 1).contiguous()  # noqa: E731
    if cs == c:
        xd = nhwc(x).to(dev).requires_grad_(True)
        yd = F.upsample_bilinear2x(xd)
        (dxd,) = torch.autograd.grad(yd, xd, nhwc(dy).to(dev))
        (dxd2,) = torch.autograd.grad(F.upsample_bilinear2x(xd), xd, nhwc(dy).to(dev))
    else:  # Cs > C through the entry points: channels past the last whole quad of C are left alone
        xd, dyd = nhwc(x).to(dev), nhwc(dy).to(dev)
        yd, dxd, dxd2 = (torch.full(s, -3.0, device=dev) for s in ((2, 2 * h, 2 * w, cs), (2, h, w, cs), (2, h, w, cs)))
        s = torch.cuda.current_stream().cuda_stream
        _lib.call('srx_upsample_bilinear2x_fwd', xd.data_ptr(), yd.data_ptr(), 2, h, w, c, cs, s)
        for out in (dxd, dxd2):
            _lib.call('srx_upsample_bilinear2x_bwd', dyd.data_ptr(), out.data_ptr(), 2, h, w, c, cs, s)
        q = (c + 3) // 4 * 4
        assert (yd[..., q:] == -3.0).all() and (dxd[..., q:] == -3.0).all()
    assert torch.equal(dxd, dxd2)  # the gather adds in a fixed order
    _close(f'bilinear {h}x{w}x{c}/{cs} y', yd[..., :c].permute(0, 3, 1, 2), refs[torch.float32][0], refs[torch.float64][0])
    _close(f'bilinear {h}x{w}x{c}/{cs} dx', dxd[..., :c].permute(0, 3, 1, 2), refs[torch.float32][1], refs[torch.float64][1])


# ------------------------------------------------------------------ 3. 4x4 stride-2 convs (and conv9) through gconv.hip
def _conv_refs(x, w, b, dy, stride, pad, mask_slope=None, bf16=False):
    """(y, dx, dw) in fp64 and fp32; ``mask_slope``: dx times the LeakyReLU derivative at x (x is that activation's output);
    ``bf16``: the recipe of bf16 products as the oracle states it (oracle/srgan.py, ``_ConvBF16``): the forward rounds x and w,
    the data gradient dy and w, the weight gradient x and dy -- except that a 64 -> <= 4 channel layer keeps fp32 operands in its
    forward and weight gradient and a <= 4 -> 64 channel layer in both gradients."""
    import contextlib
    from oracle import srgan as OS
    out = {}
    for dtype in (torch.float64, torch.float32):
        xr, wr = x.to(dtype).clone().requires_grad_(True), w.to(dtype).clone().requires_grad_(True)
        with (OS.bf16_products() if bf16 else contextlib.nullcontext()):
            y = OS.conv2d(xr, wr, None if b is None else b.to(dtype), stride, pad)
            dx, dw = torch.autograd.grad(y, (xr, wr), dy.to(dtype))
        if mask_slope is not None:
            dx = dx * torch.where(xr.detach() > 0, 1.0, mask_slope).to(dtype)
        out[dtype] = (y.detach(), dx, dw)
    return out


@pytest.mark.parametrize('cin,cout,k,stride,n,h,w', [(64, 128, 4, 2, 2, 16, 24), (256, 512, 4, 2, 2, 8, 8), (64, 1, 3, 1, 2, 8, 16)])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('fold', [False, True])
def test_even_kernel_strided_conv_and_one_channel_conv(dev, cin, cout, k, stride, n, h, w, precision, fold):
    from torchsr_amd import functional as F
    from torchsr_amd.layers import ACT_LRELU, Conv2d, set_conv_precision
    gen = torch.Generator().manual_seed(cin + cout + k)
    x = torch.randn(n, cin, h, w, generator=gen)
    if fold:
        x = TF.leaky_relu(x, 0.2)
    wt = torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5
    bias = None if k == 4 else torch.randn(cout, generator=gen) * 0.1
    ho, wo = (h + 2 - k) // stride + 1, (w + 2 - k) // stride + 1
    dy = torch.randn(n, cout, ho, wo, generator=gen)
    slope = 0.2 if fold else None
    exact = _conv_refs(x, wt, bias, dy, stride, 1, slope)
    conv = Conv2d(cin, cout, k, stride, 1, bias=bias is not None).to(dev)
    with torch.no_grad():
        conv.weight.copy_(wt)
        if bias is not None:
            conv.bias.copy_(bias)
    set_conv_precision(conv, precision)
    xd = F.to_nhwc(x.to(dev)).requires_grad_(True)
    yd = conv(xd, in_act=F.ActFold(ACT_LRELU, 0.2) if fold else None)
    assert yd.shape == (n, ho, wo, F.round4(cout))
    dyd = F.to_nhwc(dy.to(dev))
    dxd, dwd = torch.autograd.grad(yd, (xd, conv.weight), dyd)
    got = (F.to_nchw(yd.detach(), cout), F.to_nchw(dxd, cin), dwd)
    tag = f'conv {cin}->{cout} k{k} s{stride} {precision} fold={fold}'
    if precision == 'fp32':
        for name, g, r32, r64 in zip(('y', 'dx', 'dw'), got, exact[torch.float32], exact[torch.float64]):
            _close(f'{tag} {name}', g, r32, r64)
    else:  # against the reference that rounds what each of the three passes rounds: the same rule as in fp32
        rounded = _conv_refs(x, wt, bias, dy, stride, 1, slope, bf16=True)
        for name, g, r32, r64 in zip(('y', 'dx', 'dw'), got, rounded[torch.float32], rounded[torch.float64]):
            _close(f'{tag} {name}', g, r32, r64)


# ------------------------------------------------------------------ 4. the whole network
def _ref_forward(ref, x, bf16=False):
    """``ref(x)``; with ``bf16``: every conv by the oracle's recipe of bf16 products (``_conv_refs``), forward and backward."""
    if not bf16:
        return ref(x)
    from oracle import srgan as OS
    act = lambda t: TF.leaky_relu(t, 0.2)  # noqa: E731
    up = lambda t: TF.interpolate(t, scale_factor=2, mode='bilinear', align_corners=False)  # noqa: E731

    def conv(m, t):
        for hook in m._forward_pre_hooks.values():  # (spectral_norm computes m.weight there: one power iteration in training)
            hook(m, (t,))
        with OS.bf16_products():
            return OS.conv2d(t, m.weight, m.bias, m.stride[0], m.padding[0])

    sk = ref.skip_connection
    x0 = act(conv(ref.conv0, x))
    x1 = act(conv(ref.conv1, x0))
    x2 = act(conv(ref.conv2, x1))
    x3 = act(conv(ref.conv3, x2))
    x4 = act(conv(ref.conv4, up(x3))) + (x2 if sk else 0)
    x5 = act(conv(ref.conv5, up(x4))) + (x1 if sk else 0)
    x6 = act(conv(ref.conv6, up(x5))) + (x0 if sk else 0)
    return conv(ref.conv9, act(conv(ref.conv8, act(conv(ref.conv7, x6)))))


def _ref_run(sd, x, dout, train, skip, bf16=False):
    out = {}
    for dtype in (torch.float64, torch.float32):
        ref = R.UNetRef(skip_connection=skip).to(dtype)
        ref.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
        ref.train(train)
        xr = x.to(dtype).clone().requires_grad_(True)
        y = _ref_forward(ref, xr, bf16)
        y.backward(dout.to(dtype))
        out[dtype] = {'logits': y.detach(), 'dx': xr.grad, 'grads': {k: p.grad for k, p in ref.named_parameters()},
                      'buffers': {k: b.detach().clone() for k, b in ref.named_buffers()}}
    return out


def _gpu_run(dev, sd, x, dout, train, skip, precision='fp32'):
    from torchsr_amd.layers import set_conv_precision
    from torchsr_amd.realesrgan.discriminator import UNetDiscriminatorSN
    m = UNetDiscriminatorSN(skip_connection=skip)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).train(train)
    set_conv_precision(m, precision)
    xd = x.to(dev).requires_grad_(True)
    y = m(xd)
    y.backward(dout.to(dev))
    return m, {'logits': y.detach(), 'dx': xd.grad, 'grads': {k: p.grad for k, p in m.named_parameters()},
               'buffers': {k: b.detach().clone() for k, b in m.named_buffers()}}


@pytest.fixture(scope='module')
def unet_state():
    return R.seeded_state(R.UNetRef(), 11)


@pytest.mark.parametrize('shape,train,skip', [((2, 3, 32, 32), True, True), ((1, 3, 24, 40), True, True),
                                              ((2, 3, 32, 32), False, True), ((2, 3, 32, 32), True, False)])
def test_network_against_the_fp64_reference(dev, unet_state, shape, train, skip):
    gen = torch.Generator().manual_seed(shape[2] + shape[3])
    x = torch.rand(shape, generator=gen)
    dout = torch.randn(shape[0], 1, shape[2], shape[3], generator=gen) / (shape[2] * shape[3])
    ref = _ref_run(unet_state, x, dout, train, skip)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    _m, got = _gpu_run(dev, unet_state, x, dout, train, skip)
    tag = f'unet {shape} train={train} skip={skip}'
    assert got['logits'].shape == (shape[0], 1, shape[2], shape[3])
    _close(f'{tag} logits', got['logits'], r32['logits'], r64['logits'])
    _close(f'{tag} dx', got['dx'], r32['dx'], r64['dx'])
    assert list(got['grads']) == list(r64['grads'])
    for k in r64['grads']:
        _close(f'{tag} grad {k}', got['grads'][k], r32['grads'][k], r64['grads'][k])
    for k in r64['buffers']:
        _close(f'{tag} {k}', got['buffers'][k], r32['buffers'][k], r64['buffers'][k])
        moved = not torch.equal(got['buffers'][k].cpu(), unet_state[k])
        assert moved == train, (k, 'u and v move in training mode only')


def test_network_with_bf16_products(dev, unet_state):
    shape = (2, 3, 32, 32)
    gen = torch.Generator().manual_seed(64)
    x = torch.rand(shape, generator=gen)
    dout = torch.randn(2, 1, 32, 32, generator=gen) / 1024
    rounded = _ref_run(unet_state, x, dout, True, True, bf16=True)
    exact = _ref_run(unet_state, x, dout, True, True)
    _m, got = _gpu_run(dev, unet_state, x, dout, True, True, 'bf16')
    r64, r32 = rounded[torch.float64], rounded[torch.float32]
    _close('unet bf16 logits', got['logits'], r32['logits'], r64['logits'])
    _close('unet bf16 dx', got['dx'], r32['dx'], r64['dx'])
    for k in r64['grads']:
        _close(f'unet bf16 grad {k}', got['grads'][k], r32['grads'][k], r64['grads'][k])
    for k in r64['buffers']:  # the power iteration is fp32 at every precision
        _close(f'unet bf16 {k}', got['buffers'][k], exact[torch.float32]['buffers'][k], exact[torch.float64]['buffers'][k])


# ------------------------------------------------------------------ 5. the losses
def test_pair_loss_is_one_power_iteration_and_excludes_the_padding_channels(dev, unet_state):
    from torchsr_amd import functional as F
    from torchsr_amd.realesrgan.discriminator import UNetDiscriminatorSN
    gen = torch.Generator().manual_seed(5)
    real, fake = torch.rand(2, 3, 32, 32, generator=gen), torch.rand(2, 3, 32, 32, generator=gen)
    losses, states = {}, {}
    for dtype in (torch.float64, torch.float32):
        ref = R.UNetRef().to(dtype).train()
        ref.load_state_dict({k: v.to(dtype) for k, v in unet_state.items()})
        # two separate forwards of the reference, each from the seeded state (so each is ONE power iteration, as the one 2N forward
        # of pair_loss_nhwc is): a copy of the module per call, the losses and the gradients added
        twin = R.UNetRef().to(dtype).train()
        twin.load_state_dict({k: v.to(dtype) for k, v in unet_state.items()})
        out_r, out_f = ref(real.to(dtype)), twin(fake.to(dtype))
        loss = (TF.binary_cross_entropy_with_logits(out_r, torch.ones_like(out_r))
                + TF.binary_cross_entropy_with_logits(out_f, torch.zeros_like(out_f)))
        loss.backward()
        ref.conv1.weight_orig.grad += twin.conv1.weight_orig.grad
        assert all(torch.equal(a, b) for a, b in zip(ref.buffers(), twin.buffers()))  # u, v do not depend on the input
        grad1 = ref.conv1.weight_orig.grad.clone()
        adv = R.adversarial_loss(ref, fake.to(dtype), torch.tensor(0.25, dtype=dtype), 0.1)
        losses[dtype] = (loss.detach(), grad1, adv.detach())
        states[dtype] = {k: b.detach().clone() for k, b in ref.named_buffers()}
    m = UNetDiscriminatorSN()
    m.load_state_dict(unet_state)
    m = m.to(dev).train()
    loss, aux = m.pair_loss_nhwc(F.to_nhwc(real.to(dev), 4), F.to_nhwc(fake.to(dev), 4))
    loss.backward()
    _close('pair loss', loss, losses[torch.float32][0], losses[torch.float64][0])
    _close('pair loss grad conv1.weight_orig', m.conv1.weight_orig.grad, losses[torch.float32][1], losses[torch.float64][1])
    one = _ref_run(unet_state, torch.cat([real, fake]), torch.zeros(4, 1, 32, 32), True, True)  # u, v after ONE iteration
    for k in one[torch.float64]['buffers']:
        _close(f'pair loss {k} (one iteration)', dict(m.named_buffers())[k], one[torch.float32]['buffers'][k], one[torch.float64]['buffers'][k])
    adv, _aux = m.adversarial_loss_nhwc(F.to_nhwc(fake.to(dev), 4), torch.tensor(0.25, device=dev), 0.1)
    _close('adversarial loss', adv, losses[torch.float32][2], losses[torch.float64][2])
    # the mean runs over N*H*W logits: a loss over the four stored channels would move with what the padding channels hold
    logits4 = torch.full((2, 8, 8, 4), 50.0, device=dev)
    logits4[..., 0] = torch.randn(2, 8, 8, generator=gen).to(dev)
    only = F.bce_with_logits(F.to_nchw(logits4, 1), 1.0)
    want = TF.binary_cross_entropy_with_logits(logits4[..., 0].cpu().double(), torch.ones(2, 8, 8, dtype=torch.float64))
    assert abs(only.item() - want.item()) <= 1e-5 * want.item()
    assert abs(F.bce_with_logits(logits4, 1.0).item() - want.item()) > 0.5 * want.item()  # (what the exclusion prevents)


# ------------------------------------------------------------------ 6, 7. the trainer
def _trainer(dev, model: str, graphs: bool, disc: str = 'unet', seed: int = 3, amp: bool = True):
    from argparse import Namespace
    from oracle.weights import closed_form_state
    from torchsr_amd.models import select_trainer_model
    args = Namespace(disable_amp=not amp, batch_size=2, epochs=8, gan_checkpoint=None, local_rank=0, pretrain_epochs=1,
                     psnr_checkpoint=None, skip_image_save=True, world_size=1, rank=-1, use_graphs=graphs, vgg_weights='random',
                     num_conv=2, model=model)
    if disc is not None:  # (None: a Namespace WITHOUT the attribute, as code that predates the flag builds it)
        args.discriminator = disc
    cls, _crop = select_trainer_model(args)
    if model == 'esrgan':
        import functools
        from torchsr_amd.esrgan.generator import Generator
        cls = type('Small' + cls.__name__, (cls,), {'generator_cls': functools.partial(Generator, num_rrdb_blocks=1)})
    torch.manual_seed(seed)
    t = cls(dev, args, [], [], 2, 2, distributed=False)
    t._args_seen = args
    if disc == 'unet':
        t.discriminator.load_state_dict(R.seeded_state(R.UNetRef(), 11))
    t.vgg_loss.features.load_state_dict(closed_form_state(t.vgg_loss.features.state_dict(), prefix='features.'))
    t.generator.train()
    t.discriminator.train()
    return t


def _batch(dev, seed=31):
    g = torch.Generator().manual_seed(seed)
    hr = torch.rand(2, 3, 32, 32, generator=g).to(dev)
    return TF.avg_pool2d(hr, 4), hr


def _steps(t, lr, hr, n):
    return [[(k, v.item()) for k, v in sorted(t.gan_step(lr, hr).items())] for _ in range(n)]


@pytest.mark.parametrize('model', ['compact', 'esrgan'])
def test_captured_gan_steps_equal_eager_ones_bit_for_bit(dev, model, unet_state):
    lr, hr = _batch(dev)
    runs = []
    for graphs in (False, True):
        t = _trainer(dev, model, graphs)
        gen0 = {k: v.clone() for k, v in t.generator.state_dict().items()}
        losses = _steps(t, lr, hr, 4)  # two eager warm-up steps, the capture, one replay
        assert ('gan.all' in t._graphs) == graphs
        assert all(np.isfinite(v) for step in losses for _k, v in step)
        runs.append((losses, {k: v.clone() for k, v in t.discriminator.state_dict().items()},
                     {k: v.clone() for k, v in t.generator.state_dict().items()}))
        del t
    assert runs[0][0] == runs[1][0]
    for i in (1, 2):
        for k in runs[0][i]:
            assert torch.equal(runs[0][i][k], runs[1][i][k]), k
    assert all(not torch.equal(v.cpu(), unet_state[k]) for k, v in runs[0][1].items()), 'every D tensor, u and v included, moved'
    assert all(not torch.equal(v, gen0[k]) for k, v in runs[0][2].items())
    names = [k for k, _ in runs[0][0][0]]
    assert 'gan/disc-loss' in names and 'gan/adversarial-loss' in names


@pytest.mark.parametrize('model', ['compact', 'esrgan'])
def test_discriminator_vgg_is_bitwise_the_flag_absent(dev, model):
    """Four steps, the last two replayed from the captured graph (128 x 128 crops: the VGG-style discriminator's size), from a
    Namespace with ``discriminator='vgg'`` and from one WITHOUT the attribute: the same trainer class, the same losses, the same
    bits in G and D."""
    from torchsr_amd.compact.trainer import CompactTrainer
    from torchsr_amd.esrgan.trainer import ESRGANTrainer
    from torchsr_amd.realesrgan.trainer import UNetDiscriminatorMixin
    g = torch.Generator().manual_seed(32)
    hr = torch.rand(2, 3, 128, 128, generator=g).to(dev)
    lr = TF.avg_pool2d(hr, 4)
    runs = []
    for disc in ('vgg', None):
        t = _trainer(dev, model, True, disc=disc)
        assert hasattr(t._args_seen, 'discriminator') == (disc is not None)
        assert isinstance(t, CompactTrainer if model == 'compact' else ESRGANTrainer) and not isinstance(t, UNetDiscriminatorMixin)
        losses = _steps(t, lr, hr, 4)
        assert 'gan.all' in t._graphs
        runs.append((losses, {k: v.clone() for k, v in t.discriminator.state_dict().items()},
                     {k: v.clone() for k, v in t.generator.state_dict().items()}))
        del t
    assert runs[0][0] == runs[1][0]
    for i in (1, 2):
        assert list(runs[0][i]) == list(runs[1][i])
        for k in runs[0][i]:
            assert torch.equal(runs[0][i][k], runs[1][i][k]), k


def test_sn_layer_refuses_a_backward_through_a_later_calls_weight(dev, unet_state):
    """``D(a); D(b); backward`` in training mode: the layer's one W_sn buffer holds the second call's weight, so the first call's
    input gradient would be wrong -- the conv's backward raises; one call at a time, and the 2N batch, work."""
    from torchsr_amd.realesrgan.discriminator import UNetDiscriminatorSN
    m = UNetDiscriminatorSN()
    m.load_state_dict(unet_state)
    m = m.to(dev).train()
    gen = torch.Generator().manual_seed(9)
    a, b = (torch.rand(1, 3, 16, 16, generator=gen).to(dev).requires_grad_(True) for _ in range(2))
    ya, yb = m(a), m(b)
    with pytest.raises(RuntimeError, match='ran forward again before this backward'):
        (ya.sum() + yb.sum()).backward()
    m(a).sum().backward()
    m(torch.cat([a, b])).sum().backward()


def test_first_disc_loss_matches_the_reference(dev, unet_state):
    from torchsr_amd import functional as F
    lr, hr = _batch(dev)
    t = _trainer(dev, 'compact', False)
    t._enter_phase('test')  # exact fp32 for the comparison
    with torch.no_grad():
        fake = t.generator(lr).clamp(0, 1)
    t.discriminator.zero_grad()
    loss, _aux = t.discriminator.pair_loss_nhwc(F.to_nhwc(hr, 4), F.to_nhwc(fake, 4))
    refs = {}
    for dtype in (torch.float64, torch.float32):
        ref = R.UNetRef().to(dtype).train()
        ref.load_state_dict({k: v.to(dtype) for k, v in unet_state.items()})
        refs[dtype] = R.pair_loss(ref, hr.cpu().to(dtype), fake.cpu().to(dtype)).detach()
    _close('trainer pair loss', loss, refs[torch.float32], refs[torch.float64])


@pytest.mark.parametrize('model', ['compact', 'esrgan'])
def test_two_fp32_gan_steps_against_the_torch_restatement(dev, model):
    """Losses of two steps, and every parameter after the first, against ``unet_ref.GanStepRef`` in fp64 from the trainer's state.
    Losses: the module's fp32-reference bound.  Parameters: Adam's first step moves every element by lr = 1e-4 in the direction
    of its gradient's sign, so an element agrees to rounding (2e-6: 2 % of a step) unless its gradient is at the noise level, where
    the sign is anybody's: as many elements may differ as four times the count on which torch's own fp32 CPU run of the
    restatement differs from its fp64 run (at least 2, never more than 1 % of the tensor), by no more than 2 lr + 2e-6 = 2.02e-4."""
    import compact_ref
    from oracle import esrgan as OE
    from oracle import srgan as OS
    lr, hr = _batch(dev)
    t = _trainer(dev, model, False, amp=False)
    g_sd = {k: v.detach().cpu().clone() for k, v in t.generator.state_dict().items()}
    d_sd = {k: v.detach().cpu().clone() for k, v in t.discriminator.state_dict().items()}
    vgg_sd = {k: v.detach().cpu().clone() for k, v in t.vgg_loss.features.state_dict().items()}
    runs = {}
    for dtype in (torch.float64, torch.float32):
        if model == 'compact':
            gen = compact_ref.CompactRef(num_conv=2).to(dtype)
            gen.load_state_dict({k: v.to(dtype) for k, v in g_sd.items()})
            gen_state = gen.state_dict
        else:
            gen = R.StateModel({k: v.to(dtype) for k, v in g_sd.items()}, OE.generator_forward)
            gen_state = gen.state
        disc = R.UNetRef().to(dtype)
        disc.load_state_dict({k: v.to(dtype) for k, v in d_sd.items()})
        vgg = {k: v.to(dtype) for k, v in vgg_sd.items()}
        ref = R.GanStepRef(gen, disc, lambda a, b: OS.vgg_loss(vgg, a, b))
        first = ref.step(lr.cpu().to(dtype), hr.cpu().to(dtype))
        after = ({k: v.detach().clone() for k, v in gen_state().items()}, {k: v.detach().clone() for k, v in disc.state_dict().items()})
        runs[dtype] = (first, after, ref.step(lr.cpu().to(dtype), hr.cpu().to(dtype)))
    got1 = {k: v.clone() for k, v in t.gan_step(lr, hr).items()}
    after = ({k: v.detach().cpu().clone() for k, v in t.generator.state_dict().items()},
             {k: v.detach().cpu().clone() for k, v in t.discriminator.state_dict().items()})
    got2 = t.gan_step(lr, hr)
    for i, got in ((0, got1), (2, got2)):
        for k, want in runs[torch.float64][i].items():
            _close(f'{model} step {1 + i // 2} {k}', got[k], runs[torch.float32][i][k], want)
    for which, name in ((0, 'G'), (1, 'D')):
        for k, want in runs[torch.float64][1][which].items():
            if k.endswith(('weight_u', 'weight_v')):  # two power iterations of the step
                _close(f'{model} {name} {k}', after[which][k], runs[torch.float32][1][which][k], want)
                continue
            diff = (after[which][k].double() - want).abs()
            n_bad = int((diff > 2e-6).sum())
            ref_bad = int(((runs[torch.float32][1][which][k].double() - want).abs() > 2e-6).sum())  # the fp32 CPU run against fp64
            print(f'{model} {name} {k}: {n_bad} of {diff.numel()} elements beyond 2e-6 (the fp32 reference run: {ref_bad}), '
                  f'max {diff.max().item():.3e}')
            assert n_bad <= max(2, 4 * ref_bad) and n_bad <= int(1e-2 * diff.numel()) + 2, (name, k, n_bad, ref_bad, diff.max().item())
            assert diff.max().item() <= 2.02e-4, (name, k, diff.max().item())


def test_checkpoint_round_trip_and_the_mismatch_message(dev, unet_state, tmp_path):
    lr, hr = _batch(dev)
    whole = _trainer(dev, 'compact', False)
    _steps(whole, lr, hr, 3)
    first = _trainer(dev, 'compact', False)
    _steps(first, lr, hr, 2)
    state = first._model_state(1, 'compact-gan')
    assert list(state['resume']['discriminator']) == list(R.UNetRef().state_dict())
    path = str(tmp_path / 'ckpt.pth')
    torch.save(state, path)
    second = _trainer(dev, 'compact', False, seed=99)
    ckpt = second._load_checkpoint(path)
    second.generator.load_state_dict(ckpt['state'])
    assert second._restore_resume_state(ckpt)
    _steps(second, lr, hr, 1)
    for a, b in ((whole.discriminator, second.discriminator), (whole.generator, second.generator)):
        for k, v in a.state_dict().items():
            assert torch.equal(v, b.state_dict()[k]), k
    vgg = _trainer(dev, 'compact', False, disc='vgg')
    with pytest.raises(RuntimeError, match='holds a "unet" discriminator, this run trains a "vgg" one'):
        vgg._restore_resume_state(ckpt)
    with pytest.raises(RuntimeError, match='holds a "vgg" discriminator, this run trains a "unet" one'):
        second._restore_resume_state(vgg._model_state(1, 'compact-gan'))
