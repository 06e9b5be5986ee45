"""Every launch form of the kernels with a 3-channel side (thin.hip; cases: plan_forms.py section 4), through the C ABI so that
no layer class can route a call elsewhere, each against fp64 on the CPU of the same arithmetic (the operands as the kernel
rounds them):

* thin_fwd2_kernel<K, R> / thin_fwd2_bf16_kernel<K, R, IN16> as the forward of the 64 -> Cthin layers (fp32, bf16 products, bf16
  input) and as the data gradient of the Cthin -> 64 layers, at every rows-per-wave count R (srx_thin_force_rows) and at the
  planner's own R = 6 under a reservation;
* thin_wgrad_kernel<KH, KW, GROUPS, SGN> (all four) + thin_wgrad_reduce_kernel with wave ranges of one, two and three segments
  that cross row and image ends, ragged last segments, empty trailing ranges and slab counts around the reduction's loop steps;
* first3x3_fwd_kernel<PR, OUT16> with a ragged last tile, with less than one tile, and with waves that walk two tiles.

The name of the kernel a case claims is asserted from the library's launch records.  Every output is a view into a larger
NaN-filled allocation whose bytes before and behind the view must still be NaN afterwards; the padded channels of a
4-channel-stored result must be exactly 0.  Bounds are those of the tests these kernels already have (test_ops_gpu.py): 2e-5
of the tensor's largest value for the forward and the data gradient (fp32 and bf16 products alike -- the reference rounds the
operands as the kernel does, what is left is fp32 summation), 2e-4 for weight and bias gradients, half a bf16 ulp plus 2e-6 of
the largest value for a bf16-stored output.  Each test prints the worst ratio it met (profiles/thin_form_tests_times.txt)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as TF

import plan_forms as PF
from step_layers import prof_launches

pytestmark = pytest.mark.gpu

NAN = float('nan')
GUARD = 256           # elements before and behind every output view (a multiple of the 16-byte stores of either element size)
TOL_FWD, TOL_WGRAD = 2e-5, 2e-4


def _L():
    from torchsr_amd import _lib
    return _lib, _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(autouse=True)
def _overrides_reset(dev):
    """No other test sees a forced row count or a reservation of this module."""
    lib, L = _L()
    try:
        yield
    finally:
        lib.call('srx_thin_force_rows', 0)
        lib.call('srx_set_reserved_cus', 0)
        assert L.srx_plan_cus() == L.srx_device_cus()


def rnd(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def nhwc(x, cs):
    """cpu NCHW -> cpu NHWC with cs stored channels, the padding 0."""
    n, c, h, w = x.shape
    y = torch.zeros(n, h, w, cs, dtype=x.dtype)
    y[..., :c] = x.permute(0, 2, 3, 1)
    return y.contiguous()


def guarded(shape, dev, dtype=torch.float32):
    """(allocation, view): `shape` elements of NaN between two guard regions of NaN."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * GUARD,), NAN, dtype=dtype, device=dev)
    return flat, flat[GUARD:GUARD + n].view(shape)


def guards_intact(flat):
    return bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[-GUARD:]).all())


def ratio(got, want):
    """Largest error over the largest reference value."""
    got, want = got.detach().double().cpu(), want.double()
    assert bool(torch.isfinite(got).all())
    return ((got - want).abs().max() / want.abs().max().clamp_min(1e-30)).item()


def _thin_plan(d, which, n):
    lib, _ = _L()
    out = (C.c_int * 8)()
    lib.call('srx_thin_plan', C.byref(d), which, out)
    return list(out)[:n]


def _pack(d, wt, dev, bwd=False):
    lib, L = _L()
    wf = torch.empty(max(L.srx_conv2d_packed_fwd_floats(C.byref(d)), 4), device=dev)
    wb = torch.empty(max(L.srx_conv2d_packed_bwd_floats(C.byref(d)), 4), device=dev) if bwd else None
    wd = wt.to(dev)
    lib.call('srx_conv2d_pack', C.byref(d), wd.data_ptr(), wf.data_ptr(), None if wb is None else wb.data_ptr(), _stream())
    torch.cuda.synchronize()
    return wf, wb


# -------------------------------------------------------------------------------------------------- operands and fp64 references
def _r16(t):
    return t.bfloat16().double()


@functools.lru_cache(maxsize=None)
def _fwd_case(k, shape, cthin):
    """Operands of a 64 -> cthin layer and the two fp64 references without bias: of the fp32 operands, of the bf16-rounded ones."""
    n, h, w = shape
    seed = 1000 * k + 37 * h + w + cthin
    x = rnd((n, 64, h, w), seed, -0.5, 0.5)
    wt = rnd((cthin, 64, k, k), seed + 1) * (2.0 / (64 * k * k)) ** 0.5 * 1.7
    b = rnd((cthin,), seed + 2) * 0.3
    exact = TF.conv2d(x.double(), wt.double(), None, 1, k // 2)
    rounded = TF.conv2d(_r16(x), _r16(wt), None, 1, k // 2)
    return x, wt, b, exact, rounded


@functools.lru_cache(maxsize=None)
def _dgrad_case(k, shape, cthin):
    n, h, w = shape
    seed = 2000 * k + 41 * h + w + cthin
    dy = rnd((n, 64, h, w), seed, -0.5, 0.5)
    wt = rnd((64, cthin, k, k), seed + 1) * (2.0 / (cthin * k * k)) ** 0.5
    want = torch.nn.grad.conv2d_input((n, cthin, h, w), wt.double(), dy.double(), 1, k // 2)
    return dy, wt, want


@functools.lru_cache(maxsize=None)
def _wgrad_case(k, shape, cthin, sgn):
    """sgn = -1: 64 -> cthin (the thin side is the output gradient); +1: cthin -> 64 (the thin side is the image)."""
    n, h, w = shape
    cin, cout = (64, cthin) if sgn < 0 else (cthin, 64)
    seed = 3000 * k + 43 * h + w + 5 * cthin + sgn
    x, dy = rnd((n, cin, h, w), seed), rnd((n, cout, h, w), seed + 1)
    dw = torch.nn.grad.conv2d_weight(x.double(), (cout, cin, k, k), dy.double(), 1, k // 2)
    return x, dy, dw, dy.double().sum((0, 2, 3))


@functools.lru_cache(maxsize=None)
def _first3_case(shape):
    n, h, w = shape
    seed = 4000 + 47 * h + w
    x = rnd((n, 3, h, w), seed)
    wt = rnd((64, 3, 3, 3), seed + 1) * (2.0 / 27) ** 0.5 * 1.7
    b = rnd((64,), seed + 2) * 0.3
    exact = TF.conv2d(x.double(), wt.double(), None, 1, 1)
    rounded = TF.conv2d(_r16(x), _r16(wt), None, 1, 1)
    return x, wt, b, exact, rounded


# ----------------------------------------------------------------------------------------- forward of the 64 -> cthin layers
def _run_forward(dev, k, shape, cthin, r_want):
    """The three arithmetic forms, with and without bias, under whatever override / reservation is in force; every launch must
    be the kernel with r_want rows per wave.  Returns the worst error ratio."""
    lib, L = _L()
    n, h, w = shape
    x, wt, b, exact, rounded = _fwd_case(k, shape, cthin)
    xg = nhwc(x, 64).to(dev)
    x16 = xg.bfloat16()
    bg = b.to(dev)
    worst = 0.0
    for prec, in16 in ((0, False), (2, False), (2, True)):
        d = lib.Conv2dDesc(*PF.thin_out_desc(n, h, w, k, cthin=cthin, prec=prec))
        if prec == 2 and r_want == 4:      # no such instantiation: refused before any launch, the output untouched
            flat, y = guarded((n, h, w, 4), dev)
            wf, _ = _pack(d, wt, dev)
            out = (C.c_int * 4)()
            assert L.srx_thin_plan(C.byref(d), 0, out) == 2 and 'refused' in lib.last_error()

            def refused():
                with pytest.raises(RuntimeError, match='refused'):
                    if in16:
                        lib.call('srx_conv2d_fwd_bf16in', C.byref(d), x16.data_ptr(), wf.data_ptr(), None, y.data_ptr(), _stream())
                    else:
                        lib.call('srx_conv2d_fwd', C.byref(d), xg.data_ptr(), wf.data_ptr(), None, y.data_ptr(), None, None, 0, _stream())
            assert prof_launches(refused) == [] and bool(torch.isnan(flat).all())
            continue
        plan = _thin_plan(d, 0, 4)
        assert plan == [r_want, -(-h // (4 * r_want)), -(-w // 32), n * -(-h // (4 * r_want)) * -(-w // 32)], plan
        wf, _ = _pack(d, wt, dev)
        name = 'thin_fwd2_kernel<%d, %d>' % (k, r_want) if prec == 0 else 'thin_fwd2_bf16_kernel<%d, %d, %d>' % (k, r_want, in16)
        for bias in (False, True):
            flat, y = guarded((n, h, w, 4), dev)
            bp = bg.data_ptr() if bias else None
            if in16:
                run = lambda: lib.call('srx_conv2d_fwd_bf16in', C.byref(d), x16.data_ptr(), wf.data_ptr(), bp, y.data_ptr(), _stream())  # noqa: E731
            else:
                run = lambda: lib.call('srx_conv2d_fwd', C.byref(d), xg.data_ptr(), wf.data_ptr(), bp, y.data_ptr(), None, None, 0,  # noqa: E731
                                       _stream())
            assert prof_launches(run) == [name]
            assert guards_intact(flat), (name, shape, 'wrote outside its output')
            want = (exact if prec == 0 else rounded) + (b.double().view(1, -1, 1, 1) if bias else 0.0)
            got = y.cpu()
            err = ratio(got[..., :cthin].permute(0, 3, 1, 2), want)
            assert err < TOL_FWD, (name, shape, bias, err)
            if cthin < 4:
                assert float(got[..., cthin:].abs().max()) == 0.0
            worst = max(worst, err)
    return worst


@pytest.mark.parametrize('r,k,shape', PF.THIN_FWD_FORCED, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_output_conv_at_every_forced_row_count(dev, r, k, shape):
    lib, _ = _L()
    lib.call('srx_thin_force_rows', r)
    print('THINFORM forward R=%d K=%d %s worst ratio %.3e of %.0e' % (r, k, shape, _run_forward(dev, k, shape, 3, r), TOL_FWD))


@pytest.mark.parametrize('cthin,r,k,shape', PF.THIN_FWD_CTHIN)
def test_output_conv_with_other_channel_counts(dev, cthin, r, k, shape):
    lib, _ = _L()
    lib.call('srx_thin_force_rows', r)
    print('THINFORM forward cthin=%d R=%d K=%d %s worst ratio %.3e of %.0e' % (cthin, r, k, shape, _run_forward(dev, k, shape, cthin, r), TOL_FWD))


@pytest.mark.parametrize('k', PF.THIN_KS)
def test_output_conv_with_the_models_own_six_rows(dev, k):
    """Enough tiles for the planner itself to take six rows per wave (with 128 compute units reserved)."""
    lib, _ = _L()
    case = PF.THIN_FWD_OWN_R6
    lib.call('srx_set_reserved_cus', case['k'])
    d = lib.Conv2dDesc(*PF.thin_out_desc(*case['shape'], k))
    assert _thin_plan(d, 0, 4) == case['plan']
    print('THINFORM forward own R=6 K=%d %s worst ratio %.3e of %.0e' % (k, case['shape'], _run_forward(dev, k, case['shape'], 3, 6), TOL_FWD))


# ------------------------------------------------------------------------------------ data gradient of the cthin -> 64 layers
def _run_dgrad(dev, k, shape, cthin, r_want):
    lib, L = _L()
    n, h, w = shape
    dy, wt, want = _dgrad_case(k, shape, cthin)
    d = lib.Conv2dDesc(*PF.thin_in_desc(n, h, w, k, cthin=cthin))
    assert _thin_plan(d, 1, 4)[0] == r_want
    _, wb = _pack(d, wt, dev, bwd=True)
    dyg = nhwc(dy, 64).to(dev)
    flat, dx = guarded((n, h, w, 4), dev)
    nws = L.srx_conv2d_bwd_data_ws_floats(C.byref(d))
    ws = torch.empty(max(nws, 4), device=dev)
    names = prof_launches(lambda: lib.call('srx_conv2d_bwd_data', C.byref(d), dyg.data_ptr(), wb.data_ptr(), dx.data_ptr(), 0,
                                           ws.data_ptr(), nws, _stream()))
    assert names == ['thin_fwd2_kernel<%d, %d>' % (k, r_want)], names
    assert guards_intact(flat), (names, shape, 'wrote outside its output')
    got = dx.cpu()
    err = ratio(got[..., :cthin].permute(0, 3, 1, 2), want)
    assert err < TOL_FWD, (k, r_want, shape, cthin, err)
    if cthin < 4:
        assert float(got[..., cthin:].abs().max()) == 0.0
    return err


@pytest.mark.parametrize('r,k,shape', PF.THIN_FWD_FORCED, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_image_data_gradient_at_every_forced_row_count(dev, r, k, shape):
    """The mode-1 pack (thin side = input channels, taps flipped) under the same kernel."""
    lib, _ = _L()
    lib.call('srx_thin_force_rows', r)
    print('THINFORM dgrad R=%d K=%d %s ratio %.3e of %.0e' % (r, k, shape, _run_dgrad(dev, k, shape, 3, r), TOL_FWD))


@pytest.mark.parametrize('cthin,r,k,shape', PF.THIN_FWD_CTHIN)
def test_image_data_gradient_with_other_channel_counts(dev, cthin, r, k, shape):
    lib, _ = _L()
    lib.call('srx_thin_force_rows', r)
    print('THINFORM dgrad cthin=%d R=%d K=%d %s ratio %.3e of %.0e' % (cthin, r, k, shape, _run_dgrad(dev, k, shape, cthin, r), TOL_FWD))


# ---------------------------------------------------------------------------------------------------------- weight gradient
def _run_wgrad(dev, case, sgn, cthin):
    lib, L = _L()
    n, h, w = case['shape']
    k = case['K']
    x, dy, want_dw, want_db = _wgrad_case(k, case['shape'], cthin, sgn)
    cin, cout = (64, cthin) if sgn < 0 else (cthin, 64)
    d = lib.Conv2dDesc(*(PF.thin_out_desc if sgn < 0 else PF.thin_in_desc)(n, h, w, k, cthin=cthin))
    lib.call('srx_set_reserved_cus', case['k'])
    assert _thin_plan(d, 2, 5) == case['plan']
    xg, dyg = nhwc(x, 64 if sgn < 0 else 4).to(dev), nhwc(dy, 4 if sgn < 0 else 64).to(dev)
    nws = L.srx_conv2d_bwd_weight_ws_floats(C.byref(d))
    ws = torch.full((max(nws, 4),), NAN, device=dev)
    name = 'thin_wgrad_kernel<%d, %d, %d, %d>' % (k, k, 3 if k == 9 else 1, sgn)
    worst_w = worst_b = 0.0
    for accumulate in (0, 1):
        fw, dw = guarded((cout, cin, k, k), dev)
        fb, db = guarded((cout,), dev)
        prior_w, prior_b = rnd(dw.shape, 77) * want_dw.abs().max().item() * 0.5, rnd(db.shape, 78) * want_db.abs().max().item() * 0.5
        if accumulate:
            dw.copy_(prior_w)
            db.copy_(prior_b)
        names = prof_launches(lambda: lib.call('srx_conv2d_bwd_weight', C.byref(d), xg.data_ptr(), dyg.data_ptr(), dw.data_ptr(),
                                               accumulate, db.data_ptr(), ws.data_ptr(), nws, _stream()))
        assert [nm for nm in names if nm.startswith('thin_')] == [name], names
        assert guards_intact(fw) and guards_intact(fb), (name, case['id'], 'wrote outside its output')
        ew = ratio(dw, want_dw + (prior_w.double() if accumulate else 0.0))
        eb = ratio(db, want_db + (prior_b.double() if accumulate else 0.0))
        assert ew < TOL_WGRAD and eb < TOL_WGRAD, (name, case['id'], accumulate, ew, eb)
        worst_w, worst_b = max(worst_w, ew), max(worst_b, eb)
    return worst_w, worst_b


@pytest.mark.parametrize('sgn', [-1, 1])
@pytest.mark.parametrize('case', PF.THIN_WGRAD, ids=PF.by_id(PF.THIN_WGRAD))
def test_thin_weight_gradient_forms(dev, case, sgn):
    print('THINFORM wgrad %s sgn=%+d worst ratios dw %.3e db %.3e of %.0e' % ((case['id'], sgn) + _run_wgrad(dev, case, sgn, 3) + (TOL_WGRAD,)))


@pytest.mark.parametrize('sgn', [-1, 1])
@pytest.mark.parametrize('cthin,cid', PF.THIN_WGRAD_CTHIN)
def test_thin_weight_gradient_with_other_channel_counts(dev, cthin, cid, sgn):
    case = PF.THIN_WGRAD[PF.by_id(PF.THIN_WGRAD).index(cid)]
    print('THINFORM wgrad cthin=%d %s sgn=%+d worst ratios dw %.3e db %.3e of %.0e' % ((cthin, cid, sgn) + _run_wgrad(dev, case, sgn, cthin)
                                                                                 + (TOL_WGRAD,)))


# -------------------------------------------------------------------------------- forward of the 3 -> 64 first layers (3 x 3)
@pytest.mark.parametrize('case', PF.THIN_FIRST3, ids=PF.by_id(PF.THIN_FIRST3))
def test_first_layer_forms(dev, case):
    """fp32 operands, bf16-rounded operands (precision = 1) and the bf16-stored output; no activation, ReLU, LeakyReLU; with and
    without bias."""
    lib, L = _L()
    n, h, w = case['shape']
    m = n * h * w
    x, wt, b, exact, rounded = _first3_case(case['shape'])
    xg, bg = nhwc(x, 4).to(dev), b.to(dev)
    lib.call('srx_set_reserved_cus', case['k'])
    worst32 = worst16 = 0.0
    for act, slope in ((0, 0.0), (1, 0.0), (2, 0.2)):
        for prec, out16 in ((0, False), (1, False), (1, True)):
            d = lib.Conv2dDesc(*PF.thin_in_desc(n, h, w, 3, prec=prec, act=act, slope=slope))
            plan = _thin_plan(d, 3, 2)
            assert plan == case['plan'] and (plan[0] > 4 * plan[1]) == case['multi']
            wf, _ = _pack(d, wt, dev)
            nws = L.srx_conv2d_fwd_ws_floats(C.byref(d))
            ws = torch.empty(max(nws, 4), device=dev)
            for bias in (False, True):
                flat, y = guarded((n, h, w, 64), dev, torch.bfloat16 if out16 else torch.float32)
                bp = bg.data_ptr() if bias else None
                if out16:
                    run = lambda: lib.call('srx_conv2d_fwd_first3_to_bf16', C.byref(d), xg.data_ptr(), wf.data_ptr(), bp,  # noqa: E731
                                           y.data_ptr(), _stream())
                else:
                    run = lambda: lib.call('srx_conv2d_fwd', C.byref(d), xg.data_ptr(), wf.data_ptr(), bp, y.data_ptr(), None,  # noqa: E731
                                           ws.data_ptr(), nws, _stream())
                assert prof_launches(run) == ['first3x3_fwd_kernel<%d> MxNxK=%dx64x36' % (prec, m)]
                assert guards_intact(flat), (case['id'], prec, out16, 'wrote outside its output')
                z = (exact if prec == 0 else rounded) + (b.double().view(1, -1, 1, 1) if bias else 0.0)
                z = TF.relu(z) if act == 1 else TF.leaky_relu(z, slope) if act == 2 else z
                got = y.float().cpu().permute(0, 3, 1, 2)
                if out16:   # one rounding of the fp32 sum: half a bf16 ulp (test_bf16_native_conv3x3_c64)
                    assert bool(torch.isfinite(got).all())
                    err = (got.double() - z).abs()
                    bound = z.abs() * (2.0 ** -8 * 1.001) + 2e-6 * z.abs().max()
                    assert bool((err <= bound).all()), (case['id'], act, bias, (err - bound).max().item())
                    worst16 = max(worst16, (err / bound.clamp_min(1e-30)).max().item())
                else:
                    e = ratio(got, z)
                    assert e < TOL_FWD, (case['id'], act, prec, bias, e)
                    worst32 = max(worst32, e)
    print('THINFORM first3 %s worst ratio %.3e of %.0e, bf16 store worst err / bound %.3f' % (case['id'], worst32, TOL_FWD, worst16))
