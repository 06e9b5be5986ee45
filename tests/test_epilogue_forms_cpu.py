"""Every cell of epilogue_forms.py reaches the launch form it is there for -- asked of srx_conv2d_plan, the workspace queries and
srx_conv2d_stat_rows alone, which plan with the function the launches of gconv.hip plan with (host code: no GPU).  A planner change
that makes a cell vacuous fails here, loudly, instead of leaving test_epilogue_forms_gpu.py to pass on another plan.  Also without a
GPU: the table is complete (every epilogue on every tile form, whole and split; what cannot exist is listed with the library's own
reason), the integer operands keep every fp32 partial sum exact, and the float64 reference equals a second composition of the same
operation through autograd."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as TF

import epilogue_forms as EF
from epilogue_forms import SINGLE_TILES


@pytest.fixture
def lib():
    """The library with nothing forced; whatever a test forces is gone afterwards."""
    from torchsr_amd import _lib
    L = _lib.lib()
    assert L.srx_conv2d_force_plan(0, 0, 0, 0) == 0
    try:
        yield L
    finally:
        assert L.srx_conv2d_force_plan(0, 0, 0, 0) == 0


def desc(e, prec):
    from torchsr_amd import _lib
    return _lib.Conv2dDesc(*EF.desc_fields(e, prec))


def asked(L, e, prec):
    """(plan, workspace floats, statistics rows) of the case's launch under whatever is forced"""
    from torchsr_amd import _lib
    d = desc(e, prec)
    which = 1 if e['kind'] == 'dgrad' else 0
    out = (C.c_int * 6)(*([-1] * 6))
    assert L.srx_conv2d_plan(C.byref(d), which, out) == 0, _lib.last_error()
    ws = (L.srx_conv2d_bwd_data_ws_floats if which else L.srx_conv2d_fwd_ws_floats)(C.byref(d))
    return list(out), ws, L.srx_conv2d_stat_rows(C.byref(d))


_TILE_IDS = [EF.tile_id(t) for t in SINGLE_TILES]


@pytest.mark.parametrize('tile', SINGLE_TILES, ids=_TILE_IDS)
def test_every_cell_plans_the_form_it_is_listed_under(lib, tile):
    """[BM, BN, split, workgroups, KS, 0], tiles x split x BM x BN workspace floats, one statistics row per row tile -- for every
    epilogue of the table on this tile, whole and split 3; the shuffled store plans unsplit under a forced split."""
    prec, bm, bn, ks_arg, ks = tile
    for e in EF.EPILOGUES:
        for split in EF.SPLITS:
            assert lib.srx_conv2d_force_plan(bm, bn, split, ks_arg) == 0
            plan, ws, srows = asked(lib, e, prec)
            wplan, wws, wrows, name = EF.expect(e, tile, split)
            assert plan == wplan, (e['id'], split, plan, wplan)
            assert ws == wws, (e['id'], split, ws, wws)
            if e['kind'] == 'fwd':
                assert srows == wrows, (e['id'], split, srows, wrows)
            if e['id'] == 'D.shuffle':
                assert plan[2] == 1 and ws == 0
            elif split == 3:
                assert plan[2] == 3 and ws > 0     # every tile goes through tail_fixup_kernel
            assert name.split(' MxNxK')[0] in EF.ALL_INSTANTIATIONS


def test_no_layer_is_taken_by_another_kernel(lib):
    """With nothing forced no layer of the table plans the 36-pixel row tile (BM = 36), forward or data gradient, at either
    arithmetic; and none has a <= 4-channel side (thin kernels, first3) or is the 64 -> 64 3x3 layer."""
    for e in EF.EPILOGUES + EF.MIXED:
        for prec in (0, 1):
            plan, _, _ = asked(lib, e, prec)
            assert plan[0] != 36 and plan[0] in (64, 128, 144, 256), (e['id'], plan)
    for name, (n, h, w, cin, cin_s, cout, cout_s, sh, up) in EF.LAYERS.items():
        assert cin > 4 and cout > 4 and (cin, cout) != (64, 64), name
        ho, wo = EF.out_hw(name)
        m = n * ho * wo
        if not name.startswith('M'):   # a ragged last row tile for every BM
            assert m == 792 and all(m % bm for bm in (64, 128, 144, 256))


def test_the_table_is_complete_and_what_cannot_exist_is_refused(lib):
    from torchsr_amd import _lib
    cells = {(e['id'], t, s) for e, t, s in EF.cells()}
    ids = [e['id'] for e in EF.EPILOGUES]
    assert len(set(ids)) == len(ids) == 21
    for i in ids:
        for t in SINGLE_TILES:
            for s in EF.SPLITS:
                listed = any(x.get('epilogue') == i and x.get('split') == s for x in EF.IMPOSSIBLE)
                assert ((i, t, s) in cells) != listed, (i, t, s)
    assert len(cells) == 21 * 15 * 2 - 15
    # every tile side x arithmetic is a row of SINGLE_TILES or listed with the reason the planner gives
    sides = [(144, 128), (144, 64), (128, 128), (128, 64), (64, 64), (128, 32), (64, 32), (256, 128)]
    have = {t[:3] for t in SINGLE_TILES}
    gone = {x['tile']: x['why'] for x in EF.IMPOSSIBLE if 'tile' in x}
    for prec in (0, 1):
        for bm, bn in sides:
            assert ((prec, bm, bn) in have) != ((prec, bm, bn) in gone), (prec, bm, bn)
    e = EF.epilogue('A.lrelu')
    for (prec, bm, bn), why in gone.items():
        for split in EF.SPLITS:
            assert lib.srx_conv2d_force_plan(bm, bn, split, 1) == 0
            for which, ed in ((0, e), (1, EF.epilogue('A.dplain'))):
                out = (C.c_int * 6)()
                assert lib.srx_conv2d_plan(C.byref(desc(ed, prec)), which, out) == 2 and why in _lib.last_error(), _lib.last_error()
    # two wave groups on the 64 x 64 tile in both arithmetics; the 64 x 32 tile always deals its chunks to 2 / 4 groups
    assert [t for t in SINGLE_TILES if t[3] == 2] == [(0, 64, 64, 2, 2), (1, 64, 64, 2, 2)]
    assert (0, 64, 32, 1, 2) in SINGLE_TILES and (1, 64, 32, 1, 4) in SINGLE_TILES
    # the names: every instantiation of the expected set is some cell's launch, and no cell launches another
    names = {EF.expect(e, t, s)[3].split(' MxNxK')[0] for e, t, s in EF.cells()}
    names |= {EF.expect_bf16s(e, t, s)[1].split(' MxNxK')[0] for e in EF.BF16S for t in EF.BF16S_TILES for s in EF.SPLITS}
    assert names == set(EF.ALL_INSTANTIATIONS) and len(EF.ALL_INSTANTIATIONS) == 20
    # every epilogue copy is reached: addend / mask / both on linear rows, the pixel-mapped store, statistics with and without bias
    modes = {(bool(e['addend'] or e['accumulate'] or e['resid']), bool(e['mask'])) for e in EF.EPILOGUES}
    assert modes == {(False, False), (True, False), (False, True), (True, True)}
    assert {(e['stats'], e['bias']) for e in EF.EPILOGUES if e['stats']} == {(True, False), (True, True)}
    assert set(EF.RANDOM_IDS) <= set(ids) and set(EF.RANDOM_FORMS) <= set(SINGLE_TILES)
    assert set(EF.RANDOM_BF16S_IDS) <= {e['id'] for e in EF.BF16S} and set(EF.RANDOM_BF16S_FORMS) <= set(EF.BF16S_TILES)


def test_bf16_storage_cells_plan_their_workspace_and_32_column_tiles_pass_the_planner(lib):
    """srx_conv3x3_bf16s_ws_floats under the forced tile: tiles x split x BM x BN (18 chunks of 64: 6 per split).  A tile that
    exists with bf16 products but not with bf16 storage (128 x 32, 64 x 32) is NOT refused by the planner (forced_tile_refusal asks
    for the bf16-product instantiation): the workspace query answers for it, and run_gconv refuses the launch
    (test_epilogue_forms_gpu.py)."""
    assert EF.BF16S_TILES == [(256, 128, 1, 1), (128, 128, 1, 1), (128, 64, 1, 1), (64, 64, 1, 1), (64, 64, 2, 2)]
    assert EF.BF16S_REFUSED == [(128, 32, 1, 1), (64, 32, 1, 4)]
    d = desc(EF.epilogue('S.fwd16'), 1)
    assert lib.srx_conv3x3_bf16s_applicable(C.byref(d)) == 1
    for tile in EF.BF16S_TILES + EF.BF16S_REFUSED:
        bm, bn, ks_arg, ks = tile
        for split in EF.SPLITS:
            assert lib.srx_conv2d_force_plan(bm, bn, split, ks_arg) == 0
            want = EF.expect_bf16s(None, tile, split)[0]
            for which in (0, 1):
                assert lib.srx_conv3x3_bf16s_ws_floats(C.byref(d), which) == want, (tile, split, which)


@pytest.mark.parametrize('m', EF.MIXED, ids=[m['id'] for m in EF.MIXED])
def test_mixed_rows_plan_whole_and_cut_tiles_on_256_cus(lib, m):
    """The cost model's own plan (nothing forced): whole tiles AND K-split tail tiles in one launch, the ragged row tile among the
    cut ones."""
    if lib.srx_plan_cus() != EF.CUS:
        pytest.skip(EF.MIXED_SKIP % lib.srx_plan_cus())
    prec, bm, bn, ks_arg, ks = m['tile']
    plan, ws, srows = asked(lib, m, prec)
    assert plan == m['plan'], (plan, m['plan'])
    k, cn, cs, ld, cnp = EF.columns(m)
    mrows = EF.rows(m['layer'])
    mtiles = -(-mrows // bm)
    tiles = mtiles * (cnp // bn)
    assert (m['full'], m['tail']) == (tiles // EF.CUS * EF.CUS, tiles % EF.CUS) and m['full'] > 0 and m['tail'] > 0
    assert plan[3] == m['full'] + m['tail'] * plan[2] and ws == m['tail'] * plan[2] * bm * bn
    assert mrows % bm != 0 and (tiles - 1) % mtiles == mtiles - 1   # the last (cut) tile is the ragged row tile
    if m['kind'] == 'fwd':
        assert srows == mtiles


# ------------------------------------------------------------------------------------------------- integer operands stay exact
@functools.lru_cache(maxsize=None)
def _ints(layer):
    return EF.int_operands(layer)


@functools.lru_cache(maxsize=None)
def _conv(layer, kind, absolute=False):
    ops = _ints(layer)
    return EF.conv_ref(layer, kind, EF.abs_ops(ops) if absolute else ops)


_DATA_ROWS = sorted({(e['layer'], e['kind']) for e in EF.EPILOGUES + EF.BF16S + EF.MIXED})


@pytest.mark.parametrize('layer,kind', _DATA_ROWS, ids=['.'.join(r) for r in _DATA_ROWS])
def test_integer_operands_keep_every_partial_sum_exact(layer, kind):
    """conv(|x|, |w|) + |b| (data gradient: + |base| + |addend|) < 2^24 bounds every partial sum in ANY order -- K chunks, K
    splits, wave-group folds --; per column, sum |y| and sum y^2 over ALL M rows < 2^24 bounds every statistics partial; every
    value an epilogue forms is a whole number of sixteenths below 2^24 sixteenths, so each operation of the epilogue is exact in
    fp32 and the float64 reference is the only right answer, signed zeros included.  |y| <= 256 where the output is bf16."""
    import numpy as np
    ops = _ints(layer)
    for k in ('x', 'dy', 'resid', 'addend', 'base', 'maskt'):
        assert set(np.unique(ops[k])) == {-2, -1, 0, 1, 2}, k
    assert set(np.unique(ops['w'])) == {-1, 0, 1} and 0.12 < np.abs(ops['w']).mean() < 0.21   # kept with probability 0.25, a third of those 0
    assert set(np.unique(ops['bias'])) <= set(range(-5, 5)) and len(np.unique(ops['bias'])) > 5
    assert 0.15 < (ops['maskt'] == 0).mean() < 0.25      # about a fifth of the mask is exactly 0 and takes the slope
    a = EF.abs_ops(ops)
    mag = _conv(layer, kind, True)
    mag = mag + (a['bias'].view(1, -1, 1, 1) if kind == 'fwd' else a['base'] + a['addend'])
    assert mag.max().item() < EF.EXACT and mag.max().item() > 64, mag.max().item()
    conv = _conv(layer, kind)
    assert torch.equal(conv, conv.round())
    cases = [e for e in EF.EPILOGUES + EF.BF16S + EF.MIXED if (e['layer'], e['kind']) == (layer, kind)]
    assert cases
    worst = dict(mag=mag.max().item(), s2=0.0, y=0.0)
    for e in cases:
        y, pre = EF.reference(e, ops, conv)
        assert torch.equal(y * 16, (y * 16).round()) and (y.abs().max() * 16).item() < EF.EXACT, e['id']
        worst['y'] = max(worst['y'], y.abs().max().item())
        if kind == 'fwd':
            zero, pos = (pre == 0).double().mean().item(), (pre > 0).double().mean().item()
            assert 0.002 < zero < 0.1 and 0.4 < pos < 0.6, (e['id'], zero, pos)   # both branches and the exact zero are exercised
        if e.get('stats'):
            s1, s2 = pre.abs().sum((0, 2, 3)).max().item(), pre.square().sum((0, 2, 3)).max().item()
            assert s1 < EF.EXACT and s2 < EF.EXACT, (e['id'], s1, s2)
            worst['s2'] = max(worst['s2'], s2)
        if 'out16' in e:
            assert y.abs().max().item() <= 256, e['id']
            assert torch.equal(y.float().bfloat16().double(), y)
    print('EPIFORM', layer, kind, 'max conv(|x|,|w|) + .. %d  max column sum y^2 %.3g  max |y| %g' % (worst['mag'], worst['s2'], worst['y']))


# -------------------------------------------------------------------------------- the reference against a second composition
def test_reference_equals_a_second_composition_through_autograd():
    """reference() composes conv2d_input, scales, addend and torch.where; here the same data gradients come out of autograd: the
    conv's input is the activation a = LeakyReLU(u) on the masked channels with u = the mask tensor (same sign pattern, 0 on the
    slope side), the loss is <out_scale conv(a), dy> + addend_scale <a[:, :64], addend>, and u.grad is the whole epilogue.  The
    shuffled forward is composed from conv2d with its bias, leaky_relu and an index permutation written out by hand."""
    for id_ in ('C.dex64', 'C.dact'):
        e = EF.epilogue(id_)
        ops = {k: torch.as_tensor(v).double() for k, v in _ints('C').items()}
        lo, hi, slope = e['mask']
        u = ops['maskt'].clone().requires_grad_(True)
        a = torch.cat([u[:, :lo], TF.leaky_relu(u[:, lo:hi], slope), u[:, hi:]], 1)
        osc, asc = e['scales']
        loss = (TF.conv2d(a, ops['w'], None, 1, 1) * osc * ops['dy']).sum()
        if e['addend']:
            loss = loss + asc * (a[:, :e['addend'][1]] * ops['addend'][:, :e['addend'][1]]).sum()
        loss.backward()
        want, _ = EF.reference(e, _ints('C'), _conv('C', 'dgrad'))
        assert torch.equal(u.grad, want), id_
    e = EF.epilogue('D.shuffle')
    ops = {k: torch.as_tensor(v).double() for k, v in _ints('D').items()}
    y = TF.leaky_relu(TF.conv2d(ops['x'], ops['w'], ops['bias'], 1, 1), EF.SLOPE)
    n, c, h, w = y.shape
    by_hand = y.view(n, c // 4, 2, 2, h, w).permute(0, 1, 4, 2, 5, 3).reshape(n, c // 4, 2 * h, 2 * w)
    want, _ = EF.reference(e, _ints('D'), _conv('D', 'fwd'))
    assert want.shape == (2, 32, 44, 36) and torch.equal(by_hand, want)
    # the upsampled forward against conv2d of an input repeated by hand
    e = EF.epilogue('E.up')
    ops = {k: torch.as_tensor(v).double() for k, v in _ints('E').items()}
    xr = ops['x'].repeat_interleave(2, 2).repeat_interleave(2, 3)
    want, _ = EF.reference(e, _ints('E'), _conv('E', 'fwd'))
    assert want.shape == (2, 128, 22, 18) and torch.equal(torch.relu(TF.conv2d(xr, ops['w'], ops['bias'], 1, 1)), want)
    # the statistics table: rows of BM pixels, the last one partly filled, every column's totals the plain sums
    pre = _conv('B', 'fwd')
    for bm in (64, 128, 144, 256):
        t = EF.stat_table(pre, bm)
        assert t.shape == (-(-792 // bm), 96, 2)
        assert torch.equal(t[..., 0].sum(0), pre.sum((0, 2, 3))) and torch.equal(t[..., 1].sum(0), pre.square().sum((0, 2, 3)))
        flat = pre.permute(0, 2, 3, 1).reshape(792, 96)
        assert torch.equal(t[-1, :, 0], flat[792 // bm * bm:].sum(0))
