"""Every case of wgrad_forms.py reaches the launch form it is there for -- asked of srx_wgrad_plan and the workspace query alone, which
plan with the function the launches of wgrad.hip plan with (host code: no GPU).  A planner change that makes a case vacuous fails
here, loudly, instead of leaving test_wgrad_forms_gpu.py to pass on another kernel."""
import ctypes as C

import pytest

import wgrad_forms as WF

OK, BADARG, UNSUPPORTED = 0, 1, 2


def cdiv(a, b):
    return -(-a // b)


def roundup(a, b):
    return cdiv(a, b) * b


def _reset(L):
    assert L.srx_wgrad_force(-1, 0) == 0
    assert L.srx_wgrad_force_kernels(-1, -1, -1) == 0


@pytest.fixture
def lib():
    """The library with nothing forced; whatever a test forces is gone afterwards."""
    from torchsr_amd import _lib
    L = _lib.lib()
    _reset(L)
    try:
        yield L
    finally:
        _reset(L)


def desc(case):
    from torchsr_amd import _lib
    return _lib.Conv2dDesc(*WF.desc_fields(case))


def force(L, case):
    nsplit, dma, rows, reduce = case['force']
    assert L.srx_wgrad_force(-1, nsplit) == 0
    assert L.srx_wgrad_force_kernels(dma, rows, reduce) == 0


def plan(L, d, nprob, per_out):
    """srx_wgrad_plan's answer, or None for a refused split (which must carry the message)"""
    from torchsr_amd import _lib
    out = (C.c_int * 6)(*([-1] * 6))
    rc = L.srx_wgrad_plan(C.byref(d), nprob, per_out, out)
    if rc == UNSUPPORTED:
        assert 'row splits refused' in _lib.last_error(), _lib.last_error()
        return None
    assert rc == OK, (rc, _lib.last_error())
    return list(out)


def slab_floats(case):
    """Cnw x (Kw + 1): one slab and its bias row"""
    g = case['geo']
    return roundup(g['cout'], 64) * (roundup(g['k'] * g['k'] * roundup(g['cin'], 4), 64) + 1)


def upsampled_floats(case):
    g = case['geo']
    return case['nprob'] * g['n'] * 2 * g['h'] * 2 * g['w'] * g['cin_s'] if g['up'] == 2 else 0


def check_plan(L, case, got, forced_reduce=None):
    kernel, nsplit, rps, reduce, slabs = case['expect']
    if forced_reduce is not None:
        reduce = forced_reduce
    assert got is not None, case['id']
    if case['model'] and L.srx_plan_cus() != WF.CUS:   # the cost model's own split on another part: the kernels still hold
        assert (got[0], got[3]) == (kernel, reduce), (case['id'], got)
        nsplit, rps, slabs = got[1], got[2], got[5]
    else:
        assert got[:4] + got[5:] == [kernel, nsplit, rps, reduce, slabs], (case['id'], got, case['expect'])
    # workgroups: channel groups (image-row kernel) or 64 x 64 tiles, x problems x splits
    g = case['geo']
    ck = roundup(g['cin'], 4)
    per = ck // 32 if kernel in (WF.ROWS32, WF.ROWS16) else (roundup(g['cout'], 64) // 64) * (roundup(g['k'] ** 2 * ck, 64) // 64)
    assert got[4] == per * case['nprob'] * nsplit, (case['id'], got)
    # the splits are whole chunks (image rows) and none is empty
    ho, wo = WF.out_size(g)
    m = g['n'] * ho * wo
    assert rps % (g['w'] if kernel in (WF.ROWS32, WF.ROWS16) else 32) == 0 and cdiv(m, rps) == nsplit, (case['id'], got)
    assert slabs == nsplit * case['per_out']
    ws = L.srx_conv2d_bwd_weight_multi_ws_floats(C.byref(desc(case)), case['nprob'])
    assert ws == slab_floats(case) * nsplit * case['nprob'] + upsampled_floats(case), (case['id'], ws)


@pytest.mark.parametrize('case', WF.CASES, ids=WF.by_id(WF.CASES))
def test_case_plans_the_form_it_is_listed_under(lib, case):
    """... with its overrides; and with the other reduce kernel forced nothing but the reduce kernel changes"""
    d = desc(case)
    force(lib, case)
    check_plan(lib, case, plan(lib, d, case['nprob'], case['per_out']))
    nsplit, dma, rows, _ = case['force']
    assert lib.srx_wgrad_force_kernels(dma, rows, 0) == 0
    check_plan(lib, case, plan(lib, d, case['nprob'], case['per_out']), forced_reduce=0)
    assert lib.srx_wgrad_force_kernels(dma, rows, 1) == 0     # "on where eligible": not on a K that does not fit
    check_plan(lib, case, plan(lib, d, case['nprob'], case['per_out']))


@pytest.mark.parametrize('case', WF.CASES, ids=WF.by_id(WF.CASES))
def test_case_without_its_overrides(lib, case):
    """Nothing forced: the default kernel of the layer (DMA staging for fp32, the image-row kernel where eligible) at the model's own
    split -- the overrides of the case are what puts it on its form -- and the query, the workspace and a reset agree."""
    d = desc(case)
    got = plan(lib, d, case['nprob'], case['per_out'])
    kernel = case['expect'][0]
    default = {WF.F32: None, WF.BF16: None}.get(kernel, kernel)
    if case['variant'] == 'reg':
        assert got[0] in (WF.DMA, WF.WIDE, WF.LIN)
    elif case['variant'] == 'norows':
        assert got[0] in (WF.ROWS32, WF.ROWS16)
    elif default == WF.LIN:
        assert got[0] == WF.LIN or got[2] // 32 + 3 > 768, got      # (the model's split may be too long for the bit table)
    else:
        assert got[0] == kernel, (case['id'], got)
    assert got[5] == got[1] * case['per_out']
    ws = lib.srx_conv2d_bwd_weight_multi_ws_floats(C.byref(d), case['nprob'])
    assert ws == slab_floats(case) * got[1] * case['nprob'] + upsampled_floats(case)
    force(lib, case)
    forced = plan(lib, d, case['nprob'], case['per_out'])
    _reset(lib)
    assert plan(lib, d, case['nprob'], case['per_out']) == got, (case['id'], forced)


def test_the_table_reaches_every_kernel():
    """All nine kernel names, so that a case edited away is noticed; every variant of every row; the slab counts of the reduction's
    branches; WG_MAXP problems."""
    slab = {WF.SLAB_KERNELS[c['expect'][0]] for c in WF.CASES}
    red = {WF.REDUCE_KERNELS[c['expect'][3]] for c in WF.CASES}
    assert sorted(slab) + sorted(red) == WF.ALL_KERNELS and len(WF.ALL_KERNELS) == 9
    fp32 = {c['expect'][4] for c in WF.CASES if c['precision'] == 0 and c['bias'] and c['accumulate']}
    assert {64, 65, 72} <= fp32
    assert any(c['nprob'] == WF.WG_MAXP for c in WF.CASES)
    assert {c['call'] for c in WF.CASES} == {'plain', 'multi', 'scaled', 'pair'}
    for call in ('scaled', 'pair'):   # on the generic kernels and on the image-row kernel
        ks = {c['expect'][0] for c in WF.CASES if c['call'] == call}
        assert ks & {WF.ROWS32, WF.ROWS16} and ks & {WF.F32, WF.DMA} and WF.BF16 in ks, (call, ks)
    assert len(set(WF.by_id(WF.CASES))) == len(WF.CASES)


@pytest.mark.parametrize('geo,precision,nsplit', WF.REFUSED_SPLITS)
def test_forced_splits_the_rows_cannot_take_are_refused(lib, geo, precision, nsplit):
    from torchsr_amd import _lib
    case = dict(geo=geo, precision=precision)
    d = desc(case)
    before = plan(lib, d, 1, 1)
    assert lib.srx_wgrad_force(-1, nsplit) == 0
    assert plan(lib, d, 1, 1) is None
    assert lib.srx_conv2d_bwd_weight_multi_ws_floats(C.byref(d), 1) == 0 and 'row splits refused' in _lib.last_error()
    # the launch refuses before anything else: null tensors would be the next complaint
    with pytest.raises(RuntimeError, match='row splits refused'):
        x = (C.c_void_p * 1)(16)
        _lib.call('srx_conv2d_bwd_weight_multi', C.byref(d), 1, 1, x, x, x, 0, None, C.c_void_p(16), 1 << 30, None)
    assert lib.srx_wgrad_force(-1, 0) == 0
    assert plan(lib, d, 1, 1) == before


def test_bad_arguments_are_refused(lib):
    from torchsr_amd import _lib
    for bad in WF.BAD_FORCE_KERNELS:
        with pytest.raises(RuntimeError, match='wgrad_force_kernels'):
            _lib.call('srx_wgrad_force_kernels', *bad)
    d = desc(WF.CASES[0])
    before = plan(lib, d, 1, 1)        # (a refused setter changed nothing)
    assert before[0] == WF.DMA
    out = (C.c_int * 6)()
    for nprob, per_out in WF.BAD_PLAN_ARGS:
        assert lib.srx_wgrad_plan(C.byref(d), nprob, per_out, out) == BADARG and 'wgrad_plan' in _lib.last_error()
    assert lib.srx_wgrad_plan(C.byref(d), 1, 1, None) == BADARG
    assert lib.srx_wgrad_plan(None, 1, 1, out) == BADARG
    thin = _lib.Conv2dDesc(2, 8, 8, 3, 4, 64, 64, 3, 3, 1, 1, 0, 0, 0.0, 0, 0)   # the 3-channel path: thin.hip plans it
    assert plan(lib, thin, 1, 1) == [7, 0, 0, 0, 0, 0]


def test_each_override_moves_only_its_own_kernel(lib):
    """dma / rows / reduce one at a time on a layer of each kind; every combination resets with (-1, -1, -1)."""
    from torchsr_amd import _lib
    f32 = _lib.Conv2dDesc(2, 9, 20, 64, 64, 64, 64, 3, 3, 1, 1, 0, 0, 0.0, 0, 0)
    rows = _lib.Conv2dDesc(2, 9, 32, 64, 64, 64, 64, 3, 3, 1, 1, 0, 0, 0.0, 0, 1)
    base = [plan(lib, f32, 1, 1), plan(lib, rows, 1, 1)]
    assert (base[0][0], base[0][3], base[1][0], base[1][3]) == (WF.LIN, 1, WF.ROWS32, 1)
    for dma in (-1, 0, 1):
        for rw in (-1, 0, 1):
            for red in (-1, 0, 1):
                assert lib.srx_wgrad_force_kernels(dma, rw, red) == 0
                a, b = plan(lib, f32, 1, 1), plan(lib, rows, 1, 1)
                assert a[0] == (WF.F32 if dma == 0 else WF.LIN) and b[0] == (WF.BF16 if rw == 0 else WF.ROWS32)
                assert a[3] == b[3] == (0 if red == 0 else 1)
                assert a[1:3] == base[0][1:3]                  # the fp32 split does not depend on the staging
    assert lib.srx_wgrad_force(0, 0) == 0 and lib.srx_wgrad_force_kernels(-1, -1, -1) == 0
    assert plan(lib, f32, 1, 1)[0] == WF.WIDE                  # LIN off: the plain WIDE form
    _reset(lib)
    assert [plan(lib, f32, 1, 1), plan(lib, rows, 1, 1)] == base
