"""Every case of k4s2_forms.py reaches the launch form it is there for -- asked of srx_conv2d_plan and srx_wgrad_plan alone (host
code: no GPU; without one the library plans for 256 compute units, the MI355X's count) -- and every plan the cost model cuts for
the U-Net critic's conv1..conv3 at the training step's sizes is a form that some case runs on a 4x4 / stride-2 layer.  A planner
change that makes a case vacuous, or moves the step to a form nothing runs, fails here instead of leaving
test_k4s2_forms_gpu.py to pass on another kernel."""
import ctypes as C

import pytest

import k4s2_forms as KF
import wgrad_forms as WF

OK, UNSUPPORTED = 0, 2


def _m():
    from torchsr_amd import _lib
    return _lib


def _reset(L):
    assert L.srx_conv2d_force_plan(0, 0, 0, 0) == 0
    assert L.srx_conv2d_force_s2(0, 0, 0) == 0
    assert L.srx_wgrad_force(-1, 0) == 0
    assert L.srx_wgrad_force_kernels(-1, -1, -1) == 0


@pytest.fixture(autouse=True)
def lib():
    """The library with nothing forced; whatever a test forces is gone afterwards."""
    L = _m().lib()
    _reset(L)
    try:
        yield L
    finally:
        _reset(L)


def _plan(L, d, which):
    """srx_conv2d_plan's answer, or the message of its refusal"""
    out = (C.c_int * 6)(*([-1] * 6))
    rc = L.srx_conv2d_plan(C.byref(d), which, out)
    if rc == UNSUPPORTED:
        return _m().last_error()
    assert rc == OK, (rc, _m().last_error())
    return list(out)


def force(L, case):
    """the overrides of a data-gradient case (the GPU test forces through the same function)"""
    f = case['force']
    if f[0] == 's2':
        assert L.srx_conv2d_force_plan(0, 0, 0, 0) == 0 and L.srx_conv2d_force_s2(*f[1:]) == 0
    else:
        assert L.srx_conv2d_force_s2(1, 0, 0) == 0 and L.srx_conv2d_force_plan(f[1], f[2], 1, f[3]) == 0


def _desc(shape, prec, act=0, slope=0.0):
    return _m().Conv2dDesc(*KF.desc_fields(shape, prec, act, slope))


@pytest.mark.parametrize('case', KF.DGRAD, ids=KF.by_id(KF.DGRAD))
def test_data_gradient_case_plans_its_form(lib, case):
    d = _desc(case['shape'], case['prec'])
    default = _plan(lib, d, 1)
    force(lib, case)
    got = _plan(lib, d, 1)
    assert got == case['plan'], (got, case['plan'])
    assert got[:2] == list(case['tile']) and got[4] == case['ks'] and got[5] == case['form']
    assert lib.srx_conv2d_bwd_data_ws_floats(C.byref(d)) == 0      # strided data gradients take no workspace
    _reset(lib)
    assert _plan(lib, d, 1) == default


def test_data_gradient_cases_reach_every_form():
    """All 8 gconv_s2f_kernel instantiations, each with its gconv_multi_kernel twin on the same layers; the multi-only forms; a ragged
    last row tile for every BM; the odd-extent layer under multi for every 64-column tile."""
    fused = {(c['prec'],) + c['tile'] for c in KF.DGRAD if c['form'] == KF.FUSED}
    assert fused == set(KF.S2F_TILES) and len(fused) == 8
    for prec, bm, bn in KF.S2F_TILES:
        twins = {c['shape'] for c in KF.DGRAD if c['form'] == KF.MULTI and c['ks'] == 1 and (c['prec'],) + c['tile'] == (prec, bm, bn)}
        assert twins >= {c['shape'] for c in KF.DGRAD if c['form'] == KF.FUSED and (c['prec'],) + c['tile'] == (prec, bm, bn)}
        assert (KF.ODD in twins) == (bn == 64)
    only = {(c['prec'],) + c['tile'] + (c['ks'],) for c in KF.DGRAD if c['ks'] == 2 or c['tile'][1] == 32}
    assert only == set(KF.MULTI_ONLY)
    assert all(c['shape'][3] <= 32 for c in KF.DGRAD if c['tile'][1] == 32)
    for shape in KF.SHAPES + [KF.ODD] + KF.NARROW:
        assert all(KF.class_rows(shape) % bm for bm in (64, 128, 144)), shape
        assert shape[5] >= shape[3] and shape[3] % 4 == 0
    assert KF.ODD[1] % 2 == 1 and KF.ODD[2] % 2 == 1
    assert len(set(KF.by_id(KF.DGRAD))) == len(KF.DGRAD) and len(set(KF.by_id(KF.FWD))) == len(KF.FWD)


@pytest.mark.parametrize('case', KF.ODD_FUSED_REFUSED, ids=lambda c: 'p%d.%dx%d' % ((c['prec'],) + c['force'][2:]))
def test_fused_kernel_on_the_odd_extent_layer_is_refused(lib, case):
    d = _desc(case['shape'], case['prec'])
    force(lib, case)
    got = _plan(lib, d, 1)
    assert isinstance(got, str) and case['message'] in got, got
    _reset(lib)
    assert _plan(lib, d, 1)[5] == KF.MULTI     # its own plan: gconv_multi_kernel


@pytest.mark.parametrize('case', KF.FWD, ids=KF.by_id(KF.FWD))
def test_forward_case_plans_its_form(lib, case):
    d = _desc(case['shape'], case['prec'], KF.ACT_LRELU, KF.SLOPE)
    bm, bn = case['tile']
    assert lib.srx_conv2d_force_plan(bm, bn, case['split'], case['ks_arg']) == 0
    got = _plan(lib, d, 0)
    assert got == case['plan'], (got, case['plan'])
    ho, wo = KF.out_size(case['shape'])
    m = case['shape'][0] * ho * wo
    assert m % bm != 0                               # a ragged last row tile
    tiles = -(-m // bm) * (KF.padded_cols(case['shape'][4]) // bn)
    # a forced split sends every tile's partial sums through the workspace: whole tiles of it, none without
    assert lib.srx_conv2d_fwd_ws_floats(C.byref(d)) == (0 if case['split'] == 1 else tiles * case['split'] * bm * bn)


def test_forward_cases_reach_every_tile_whole_and_split():
    got = {(c['prec'],) + c['tile'] + (c['ks_arg'], c['ks'], c['split']) for c in KF.FWD}
    assert got == {t + (s,) for t in KF.SINGLE_TILES for s in KF.FWD_SPLITS}
    assert KF.FWD_BIAS_CASE in KF.SINGLE_TILES
    for c in KF.FWD:
        assert c['shape'] in KF.FWD_SHAPES


def _step_plans(L, layer, batch, prec):
    d = _m().Conv2dDesc(*KF.step_desc_fields(layer, batch, prec))
    w = (C.c_int * 6)()
    assert L.srx_wgrad_plan(C.byref(d), 1, 1, w) == OK, _m().last_error()
    return _plan(L, d, 0), _plan(L, d, 1), list(w)[:4]


@pytest.mark.parametrize('row', KF.STEP_PLANS, ids=lambda r: '%s.n%d.p%d' % r[:3])
def test_step_size_plan_is_a_form_some_case_runs(lib, row):
    """conv1..conv3 at 2N = 32 and N = 16 on 128 x 128 crops: the planner's answers are the recorded ones, and each is a form of
    the tables -- forward (precision, tile, KS, split or whole), data gradient (precision, tile, KS, fused or multi), weight
    gradient (slab kernel, one split or several) on a 4x4 / stride-2 row of wgrad_forms.py."""
    layer, batch, prec, fwd, dgrad, wgrad = row
    if lib.srx_plan_cus() != KF.CUS:
        pytest.skip('the recorded plans are those of a 256-CU part with nothing reserved')
    assert _step_plans(lib, layer, batch, prec) == (fwd, dgrad, wgrad)
    fwd_forms = {KF.fwd_form(c['prec'], c['plan']) for c in KF.FWD}
    dgrad_forms = {KF.dgrad_form(c['prec'], c['plan']) for c in KF.DGRAD}
    k4 = [c for c in WF.CASES if (c['geo']['k'], c['geo']['stride'], c['geo']['pad']) == (KF.K, KF.STRIDE, KF.PAD)]
    wgrad_forms = {(c['expect'][0], c['expect'][1] > 1) for c in k4 if c['precision'] == prec}
    assert KF.fwd_form(prec, fwd) in fwd_forms, ('forward', fwd)
    assert KF.dgrad_form(prec, dgrad) in dgrad_forms, ('data gradient', dgrad)
    assert KF.wgrad_form(wgrad) in wgrad_forms, ('weight gradient', wgrad)


def test_step_size_rows_cover_both_batches_and_precisions():
    assert {r[:3] for r in KF.STEP_PLANS} == {(name, n, p) for name in KF.STEP_LAYERS for n in (32, 16) for p in (0, 1)}
    # the forms the issue was opened for are among them: the fused kernel on conv1, KS = 2 and the 128 x 128 multi tile below it,
    # a split forward, the 256-row tile, the WIDE and BF16 slab kernels in many splits
    assert any(r[4][5] == KF.FUSED for r in KF.STEP_PLANS) and any(r[4][4] == 2 for r in KF.STEP_PLANS)
    assert any(r[4][:2] == [128, 128] and r[4][5] == KF.MULTI for r in KF.STEP_PLANS)
    assert any(r[3][2] == 2 for r in KF.STEP_PLANS) and any(r[3][0] == 256 for r in KF.STEP_PLANS)
    assert {r[5][0] for r in KF.STEP_PLANS} == {WF.WIDE, WF.BF16}


def test_weight_gradient_rows_of_the_even_kernel():
    """wgrad_forms.py's K rows: WIDE, F32 and BF16 on the 64 -> 128 and 128 -> 256 layers, wgrad_dma_kernel<0, 0> on the 96-channel one;
    1, 2, 4 and 5 splits that cut 15-pixel output rows mid-row; an accumulating case; a refused split."""
    k4 = [c for c in WF.CASES if (c['geo']['k'], c['geo']['stride'], c['geo']['pad']) == (KF.K, KF.STRIDE, KF.PAD)]
    by_layer = {}
    for c in k4:
        by_layer.setdefault((c['geo']['cin'], c['geo']['cout']), set()).add(c['expect'][0])
    assert by_layer[(64, 128)] == by_layer[(128, 256)] == {WF.WIDE, WF.F32, WF.BF16}
    assert by_layer[(96, 256)] == {WF.DMA, WF.F32, WF.BF16}
    cuts = {c['expect'][1:3] for c in k4 if c['geo']['h'] == 26}
    assert cuts == {(1, 608), (2, 320), (4, 160), (5, 128)}
    assert all(rps % 15 for ns, rps in cuts if ns > 1)            # no split ends on an output row's end
    assert any(c['accumulate'] for c in k4)
    assert any(g['k'] == KF.K and g['stride'] == KF.STRIDE for g, _p, _n in WF.REFUSED_SPLITS)
