"""Every case of plan_forms.py reaches the launch form it is there for -- asked of the planners alone (host code: no GPU; without
one the library plans for 256 compute units, the MI355X's count).  A planner change that makes a case vacuous fails here, loudly,
instead of leaving test_plan_forms_gpu.py to pass on some other kernel form."""
import ctypes as C

import pytest

import plan_forms as PF


def _lib():
    from torchsr_amd import _lib
    return _lib


@pytest.fixture
def lib():
    """The library on a 256-CU plan; whatever a test reserves is gone afterwards."""
    m = _lib()
    L = m.lib()
    prior_plan = L.srx_plan_cus()
    prior = max(0, L.srx_device_cus() - prior_plan)
    if prior_plan != PF.CUS:
        pytest.skip('the plans of plan_forms.py are those of a 256-CU part with nothing reserved')
    try:
        yield L
    finally:
        assert L.srx_set_reserved_cus(prior) == 0
        assert L.srx_plan_cus() == prior_plan


class reserved:
    """k compute units reserved inside the block; the prior reservation back behind it, and that checked."""

    def __init__(self, L, k):
        self.L, self.k = L, k

    def __enter__(self):
        self.plan_before = self.L.srx_plan_cus()
        self.prior = max(0, self.L.srx_device_cus() - self.plan_before)
        assert self.L.srx_set_reserved_cus(self.k) == 0 and self.L.srx_plan_cus() == PF.CUS - self.k

    def __exit__(self, *exc):
        assert self.L.srx_set_reserved_cus(self.prior) == 0
        assert self.L.srx_plan_cus() == self.plan_before
        return False


def _desc(fields):
    return _lib().Conv2dDesc(*fields)


def _plan(L, d, which):
    out = (C.c_int * 6)()
    assert L.srx_conv2d_plan(C.byref(d), which, out) == 0, _lib().last_error()
    return list(out)


def _c64_plan(L, n, h, w, cout):
    out = (C.c_int * 3)()
    assert L.srx_conv3x3_c64_bf16_plan(n, h, w, cout, out) == 0, _lib().last_error()
    return list(out)


@pytest.mark.parametrize('n,h,w,nb,k', PF.ROW_TILE_48)
def test_row_tile_cases_plan_48_pixels(lib, n, h, w, nb, k):
    d = _desc(PF.row_tile_desc(n, h, w))
    m = n * h * w
    with reserved(lib, k):
        for which in (0, 1):
            plan = _plan(lib, d, which)
            assert plan[0] == PF.ROW_TILE_PIXELS and plan[:4] == [48, 64, 1, m // 48], (which, plan)
        assert lib.srx_conv2d_stat_rows(C.byref(d)) == m // 48
        assert lib.srx_conv2d_bwd_data_bn_rows(C.byref(d)) == m // 48
        assert lib.srx_conv2d_fwd_bn_in_ok(C.byref(d)) == 1
        assert lib.srx_conv2d_bwd_data_bn_in_ok(C.byref(d)) == 1
        assert lib.srx_conv2d_fwd_ws_floats(C.byref(d)) == 0 and lib.srx_conv2d_bwd_data_ws_floats(C.byref(d)) == 0
    if k:  # ... and it is the reservation that makes it so
        assert _plan(lib, d, 0)[0] == 36


@pytest.mark.parametrize('case', PF.C64_MULTI_ITEM, ids=PF.by_id(PF.C64_MULTI_ITEM))
def test_c64_cases_give_a_workgroup_several_items(lib, case):
    n, h, w = case['shape']
    rows, chunks, strips = _c64_plan(lib, n, h, w, case['cout'])
    grid = lib.srx_plan_cus() // (case['cout'] // 64)
    assert n * chunks * strips > grid, (rows, chunks, strips, grid)
    assert n * strips > grid            # (no chunk height the planner may take later brings the items under the grid)
    assert chunks >= case['min_chunks'] and strips >= case['min_strips'], (rows, chunks, strips)
    if case['min_chunks'] > 1:          # consecutive items of a workgroup differ in chunk and in strip, not only in image
        assert grid % chunks != 0 and (grid // chunks) % strips != 0, (chunks, strips, grid)


@pytest.mark.parametrize('n,h,w,cout', PF.THIN9_MULTI_ITEM)
def test_thin9_cases_give_a_workgroup_several_items(lib, n, h, w, cout):
    assert n * -(-w // PF.THIN9_STRIP) > lib.srx_plan_cus()


def _differs(plan0, plan, fields, index):
    return all(plan0[index[f]] != plan[index[f]] for f in fields)


@pytest.mark.parametrize('case', PF.RESERVED_GCONV, ids=PF.by_id(PF.RESERVED_GCONV))
def test_reserved_gconv_cases_move_the_plan(lib, case):
    d = _desc(case['desc'])
    ws_of = lib.srx_conv2d_bwd_data_ws_floats if case['which'] else lib.srx_conv2d_fwd_ws_floats
    plan0, ws0 = _plan(lib, d, case['which']), ws_of(C.byref(d))
    with reserved(lib, case['k']):
        plan, ws = _plan(lib, d, case['which']), ws_of(C.byref(d))
    assert plan0 == case['plan0'] and plan == case['plan'], (plan0, plan)
    assert _differs(plan0, plan, case['fields'], PF.GCONV_FIELDS), (plan0, plan)
    assert ws0 > 0 and ws > 0 and ws != ws0   # every case splits a tail along K: a workspace, and one that moves with the plan
    assert _plan(lib, d, case['which']) == plan0


@pytest.mark.parametrize('case', PF.RESERVED_WINO, ids=PF.by_id(PF.RESERVED_WINO))
def test_reserved_winograd_cases_move_the_plan(lib, case):
    d = _desc(case['desc'])
    out = (C.c_int * 6)()

    def query():
        got = []
        for which in (0, 1):
            assert lib.srx_wino_plan(C.byref(d), which, out) == 0
            got.append((list(out), lib.srx_wino_ws_floats(C.byref(d), which)))
        return got
    assert lib.srx_wino_applicable(C.byref(d)) == 1
    at0 = query()
    with reserved(lib, case['k']):
        atk = query()
        assert lib.srx_wino_applicable(C.byref(d)) == 1
    for (plan0, ws0), (plan, ws) in zip(at0, atk):
        assert plan0 == case['plan0'] and plan == case['plan'] and (ws0, ws) == (case['ws0'], case['ws']), (plan0, ws0, plan, ws)
        assert _differs(plan0, plan, case['fields'], PF.WINO_FIELDS)
    assert query() == at0


@pytest.mark.parametrize('case', PF.RESERVED_C64, ids=PF.by_id(PF.RESERVED_C64))
def test_reserved_c64_cases_move_the_chunks(lib, case):
    n, h, w = case['shape']
    plan0 = _c64_plan(lib, n, h, w, case['cout'])
    with reserved(lib, case['k']):
        plan = _c64_plan(lib, n, h, w, case['cout'])
    assert plan0 == case['plan0'] and plan == case['plan'] and plan0[:2] != plan[:2], (plan0, plan)
    assert _c64_plan(lib, n, h, w, case['cout']) == plan0


@pytest.mark.parametrize('case', PF.RESERVED_WGRAD, ids=PF.by_id(PF.RESERVED_WGRAD))
def test_reserved_weight_gradient_cases_move_the_row_splits(lib, case):
    d = _desc(case['desc'])
    ws0 = lib.srx_conv2d_bwd_weight_multi_ws_floats(C.byref(d), case['nprob'])
    with reserved(lib, case['k']):
        ws = lib.srx_conv2d_bwd_weight_multi_ws_floats(C.byref(d), case['nprob'])
    assert (ws0, ws) == (case['ws0'], case['ws']) and ws != ws0, (ws0, ws)
    assert lib.srx_conv2d_bwd_weight_multi_ws_floats(C.byref(d), case['nprob']) == ws0
