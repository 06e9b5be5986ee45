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


@pytest.mark.parametrize('case', PF.C64_SLOPES, ids=PF.by_id(PF.C64_SLOPES))
def test_c64_slopes_cases_reach_their_tile_form_and_item_count(lib, case):
    """The per-channel-slope cases: the tile form follows the row length, and the multi-item ones give a workgroup several items
    whatever chunk height the planner takes (N x strips > grid)."""
    n, h, w = case['shape']
    rows, chunks, strips = _c64_plan(lib, n, h, w, case['cout'])
    grid = lib.srx_plan_cus() // (case['cout'] // 64)
    form = (4, 1) if w <= 32 else ((2, 2) if w <= 64 else (1, 4))
    assert form == case['form'] and strips == -(-w // (32 * form[1])), (form, strips)
    if case['multi']:
        assert n * chunks * strips > grid and n * strips > grid, (rows, chunks, strips, grid)
    else:
        assert n * chunks * strips <= grid, (rows, chunks, strips, grid)


def test_c64_slopes_cases_cover_every_form():
    for multi in (False, True):
        forms = {c['form'] for c in PF.C64_SLOPES if c['multi'] == multi}
        assert forms >= ({(2, 2), (1, 4)} if not multi else set(PF.C64_SLOPES_FORMS)), (multi, forms)
    assert {c['form'] for c in PF.C64_SLOPES} == set(PF.C64_SLOPES_FORMS)
    two_groups = [c for c in PF.C64_SLOPES if c['cout'] == 128]
    assert {c['multi'] for c in two_groups} == {False, True}
    assert {(c['res'], c['multi']) for c in PF.C64_SLOPES} == {(r, m) for r in (False, True) for m in (False, True)}
    assert any(c['shape'][1] % 2 for c in PF.C64_SLOPES if c['form'] == (2, 2))   # odd rows under two rows per wave


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


# ------------------------------------------------------------------------------------ the kernels with a 3-channel side (thin.hip)
def _thin_plan(L, d, which, n):
    out = (C.c_int * 8)(*([-7] * 8))
    assert L.srx_thin_plan(C.byref(d), which, out) == 0, _lib().last_error()
    assert list(out)[n:] == [-7] * (8 - n)     # the query writes the numbers of its path and nothing behind them
    return list(out)[:n]


class forced_rows:
    """srx_thin_force_rows(rows) inside the block, the model's choice back behind it."""

    def __init__(self, L, rows):
        self.L, self.rows = L, rows

    def __enter__(self):
        assert self.L.srx_thin_force_rows(self.rows) == 0, _lib().last_error()

    def __exit__(self, *exc):
        assert self.L.srx_thin_force_rows(0) == 0
        return False


@pytest.mark.parametrize('r,k,shape', PF.THIN_FWD_FORCED, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_thin_forward_cases_run_the_forced_rows(lib, r, k, shape):
    n, h, w = shape
    want = [r, -(-h // (4 * r)), -(-w // 32), n * -(-h // (4 * r)) * -(-w // 32)]
    fwd, dgrad = _desc(PF.thin_out_desc(n, h, w, k)), _desc(PF.thin_in_desc(n, h, w, k))
    model = _thin_plan(lib, fwd, 0, 4)
    assert model[0] == 3        # (few tiles: the model would not run anything else here)
    with forced_rows(lib, r):
        assert _thin_plan(lib, fwd, 0, 4) == want and _thin_plan(lib, dgrad, 1, 4) == want
        bf16 = _desc(PF.thin_out_desc(n, h, w, k, prec=2))
        if r == 4:                  # no thin_fwd2_bf16_kernel<K, 4>: refused where the layer is planned
            out = (C.c_int * 4)()
            assert lib.srx_thin_plan(C.byref(bf16), 0, out) == 2 and 'refused' in _lib().last_error()
        else:
            assert _thin_plan(lib, bf16, 0, 4) == want
    assert _thin_plan(lib, fwd, 0, 4) == model
    # what each shape is there for
    th, tw = want[1], want[2]
    if shape == PF.thin_fwd_forced_shapes(r)[0]:
        assert (th, tw) == (1, 1) and h % (4 * r) == 4 * r - 1 and w == 31
    elif shape == PF.thin_fwd_forced_shapes(r)[1]:
        assert (th, tw) == (2, 2) and h % (4 * r) == 1 and w % 32 == 1 and n > 1
    elif shape == PF.thin_fwd_forced_shapes(r)[2]:
        assert h < k and (th, tw) == (1, 3) and w % 32 != 0     # every output row has padding rows above and below it
    else:
        assert th == 3 and h % (4 * r) not in (0, 1) and w % 32 == 0 and tw == 2


@pytest.mark.parametrize('cthin,r,k,shape', PF.THIN_FWD_CTHIN)
def test_thin_channel_count_cases_plan(lib, cthin, r, k, shape):
    assert (r, k, shape) in PF.THIN_FWD_FORCED and cthin in (1, 2, 4)
    with forced_rows(lib, r):
        for which, fields in ((0, PF.thin_out_desc(*shape, k, cthin=cthin)), (1, PF.thin_in_desc(*shape, k, cthin=cthin))):
            assert _thin_plan(lib, _desc(fields), which, 4)[0] == r


def test_thin_forward_case_with_the_models_own_six_rows(lib):
    case = PF.THIN_FWD_OWN_R6
    n, h, w = case['shape']
    for k in PF.THIN_KS:
        for prec in (0, 2):
            d = _desc(PF.thin_out_desc(n, h, w, k, prec=prec))
            assert _thin_plan(lib, d, 0, 4) == case['plan0'] and case['plan0'][0] == 3
            with reserved(lib, case['k']):
                plan = _thin_plan(lib, d, 0, 4)
                assert plan == case['plan'] and plan[0] == 6
                assert n * -(-h // 24) * -(-w // 32) >= 4 * lib.srx_plan_cus()
                assert h % 24 == 1 and w % 32 == 1          # (ragged both ways)
            assert _thin_plan(lib, d, 0, 4) == case['plan0']


@pytest.mark.parametrize('case', PF.THIN_WGRAD, ids=PF.by_id(PF.THIN_WGRAD))
def test_thin_weight_gradient_cases_plan(lib, case):
    n, h, w = case['shape']
    with reserved(lib, case['k']):
        plans = [_thin_plan(lib, _desc(f(n, h, w, case['K'])), 2, 5) for f in (PF.thin_out_desc, PF.thin_in_desc)]
        ws = lib.srx_conv2d_bwd_weight_ws_floats(C.byref(_desc(PF.thin_out_desc(n, h, w, case['K']))))
    assert plans[0] == plans[1] == case['plan'], plans
    groups, nseg, spr, nranges, nslabs = case['plan']
    assert groups == (3 if case['K'] == 9 else 1) and nseg == n * h * -(-w // 16)
    assert (nranges - 1) * spr < nseg <= nranges * spr and nslabs == -(-nranges // 4)
    assert 4 * nslabs - nranges == case['empty']
    assert ws >= nslabs * 4 * case['K'] ** 2 * 64         # the workspace query covers the slabs of the launch
    if case['id'].startswith(('k9.4x41x72', 'k9.3x41x40', 'k3.6x41x72')):   # ranges of several segments that cross row and image ends
        wsegs = -(-w // 16)
        assert spr >= 2 and wsegs % spr != 0 and (h * wsegs) % spr != 0 and w % 16 != 0 and case['empty'] > 0
        assert nslabs > 32                                   # (the reduction's 16-way loop runs more than once)
    if case['id'] == 'k9.4x41x72.r128':
        assert spr >= 3 and nseg % spr != 0


def test_thin_weight_gradient_cases_cover_the_reduction_loops():
    """thin_wgrad_reduce_kernel: part p of 4 sums slabs p, p + 4, ...: sixteen at a time while r + 12 < slabs, then four at a time."""
    slabs = sorted({c['plan'][4] for c in PF.THIN_WGRAD})
    assert {1, 2, 3, 4, 5, 15, 16, 17} <= set(slabs)                      # both sides of 4 and of 16
    assert any(s > 32 for s in slabs)                                     # the 16-way loop more than once
    for cthin, cid in PF.THIN_WGRAD_CTHIN:
        assert cid in PF.by_id(PF.THIN_WGRAD) and cthin in (1, 2, 4)
    ks = {(c['K'], c['plan'][2] >= 2) for c in PF.THIN_WGRAD}
    assert ks == {(3, False), (3, True), (9, False), (9, True)}           # both kernel sizes with one and with several segments per range


@pytest.mark.parametrize('case', PF.THIN_FIRST3, ids=PF.by_id(PF.THIN_FIRST3))
def test_first_layer_cases_plan(lib, case):
    n, h, w = case['shape']
    m = n * h * w
    for prec in (0, 1):
        d = _desc(PF.thin_in_desc(n, h, w, 3, prec=prec, act=2, slope=0.2))
        with reserved(lib, case['k']):
            plan = _thin_plan(lib, d, 3, 2)
        assert plan == case['plan'] and plan[0] == -(-m // 32)
        assert (plan[0] > 4 * plan[1]) == case['multi']
    if case['multi']:       # a ragged last tile, and it is the reservation that sends waves to a second tile
        plan0 = _thin_plan(lib, d, 3, 2)
        assert m % 32 != 0 and case['k'] > 0 and plan0[0] <= 4 * plan0[1]
    else:
        assert m < 32


def test_thin_plan_refuses_other_layers_and_bad_arguments(lib):
    out = (C.c_int * 8)()
    gen = _desc(PF._conv(2, 24, 24, 64, 64, 3))
    for which in range(4):
        assert lib.srx_thin_plan(C.byref(gen), which, out) == 2 and 'thin_plan' in _lib().last_error()
    fwd, first = _desc(PF.thin_out_desc(1, 9, 9, 9)), _desc(PF.thin_in_desc(1, 9, 9, 3))
    assert lib.srx_thin_plan(C.byref(fwd), 1, out) == 2 and lib.srx_thin_plan(C.byref(fwd), 3, out) == 2
    assert lib.srx_thin_plan(C.byref(first), 0, out) == 2
    assert lib.srx_thin_plan(C.byref(_desc(PF.thin_in_desc(1, 9, 9, 9))), 3, out) == 2       # 9 x 9: the generic forward
    assert lib.srx_thin_plan(C.byref(fwd), 4, out) == 1 and lib.srx_thin_plan(C.byref(fwd), -1, out) == 1
    assert lib.srx_thin_plan(C.byref(fwd), 0, None) == 1


def test_thin_force_rows_round_trips_and_refuses(lib):
    d = _desc(PF.thin_out_desc(2, 30, 40, 9))
    model = _thin_plan(lib, d, 0, 4)
    assert model == [3, 3, 2, 12]
    try:
        for rows in PF.THIN_ROWS:
            assert lib.srx_thin_force_rows(rows) == 0
            assert _thin_plan(lib, d, 0, 4) == [rows, -(-30 // (4 * rows)), 2, 2 * -(-30 // (4 * rows)) * 2]
            for bad in (-1, 1, 2, 5, 7, 8, 12):      # refused, and the override in force stays
                assert lib.srx_thin_force_rows(bad) == 1 and 'thin_force_rows' in _lib().last_error()
                assert _thin_plan(lib, d, 0, 4)[0] == rows
        assert lib.srx_thin_force_rows(0) == 0 and _thin_plan(lib, d, 0, 4) == model
        # 4 rows with bf16 products: accepted as a setting (fp32 layers run it), refused on the layer that has no such kernel
        assert lib.srx_thin_force_rows(4) == 0
        out = (C.c_int * 4)(*([-7] * 4))
        assert lib.srx_thin_plan(C.byref(_desc(PF.thin_out_desc(2, 30, 40, 9, prec=2))), 0, out) == 2
        assert 'refused' in _lib().last_error() and list(out) == [-7] * 4
        # the weight gradient and the first layer have no rows to force
        wg = _thin_plan(lib, d, 2, 5)
        assert lib.srx_thin_force_rows(0) == 0 and _thin_plan(lib, d, 2, 5) == wg
    finally:
        assert lib.srx_thin_force_rows(0) == 0


@pytest.mark.parametrize('value,rows,said', [('5', 3, True), ('12', 3, True), ('4', 4, False), ('6', 6, False)])
def test_thin_rows_from_the_environment(value, rows, said):
    """SRX_THIN_FWD_ROWS seeds srx_thin_force_rows when the library is loaded, under the override's rule: a value outside
    {0, 3, 4, 6} changes nothing and says so once on stderr."""
    import os
    import subprocess
    import sys
    code = ('import ctypes as C, sys\n'
            'sys.path.insert(0, %r)\n'
            'from torchsr_amd import _lib\n'
            'import plan_forms as PF\n'
            'L = _lib.lib()\n'
            'out = (C.c_int * 4)()\n'
            'd = _lib.Conv2dDesc(*PF.thin_out_desc(2, 30, 40, 9))\n'
            'assert L.srx_thin_plan(C.byref(d), 0, out) == 0, _lib.last_error()\n'
            'print("PLAN", list(out))\n') % os.path.dirname(os.path.abspath(PF.__file__))
    root = os.path.dirname(os.path.dirname(os.path.abspath(PF.__file__)))
    env = dict(os.environ, SRX_THIN_FWD_ROWS=value, PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''))
    env.pop('SRX_RESERVED_CUS', None)
    run = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    tiles_h = -(-30 // (4 * rows))
    assert 'PLAN [%d, %d, 2, %d]' % (rows, tiles_h, 4 * tiles_h) in run.stdout, run.stdout
    lines = [ln for ln in run.stderr.splitlines() if 'SRX_THIN_FWD_ROWS' in ln]
    assert len(lines) == (1 if said else 0), run.stderr
    if said:
        assert lines[0].startswith('libsrx_hip: SRX_THIN_FWD_ROWS=%s ignored' % value)
