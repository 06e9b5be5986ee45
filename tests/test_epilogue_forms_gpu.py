"""Every epilogue of gconv_kernel (gconv.hip) in every tile form (cells: epilogue_forms.py), through the C ABI so that no layer class
can route a call elsewhere.  Before a launch the forced plan is asserted from srx_conv2d_plan ([BM, BN, split, workgroups, KS, 0]) and
the workspace query (tiles x split x BM x BN floats; bf16 storage has no plan call: srx_conv3x3_bf16s_ws_floats); after it the launch
recorder must show exactly the cell's gconv_kernel<..> instantiation.  tail_fixup_kernel is not a recorded launch: that it ran is
shown by the output -- under a forced split every tile's partial sums go to the workspace and the fix-up alone writes the output
tensor.  Outputs start as NaN (as the accumulated gradient where the epilogue reads it) between sentinel bands, columns past the
layer's own hold a sentinel that must survive, the workspace and the statistics table start as NaN, inputs lie between NaN bands, and
what an epilogue must not read (addend columns past addend_channels, mask columns outside the range) is NaN.

(a) EXACT, every cell.  On the integer operands of epilogue_forms.int_operands every partial sum and every value an epilogue forms is
    exact in fp32 in any order (test_epilogue_forms_cpu.py), so the output and EVERY entry of the statistics table must equal the
    float64 reference bit for bit -- compared as integers after the exact cast, so signed zeros count: the library's activation is
    v > 0 ? v : v * slope, and a negative value under ReLU is -0.  For a bf16 output the reference is .bfloat16() of the exact value.
    The whole and the split-3 result of a cell are bitwise equal to each other; on integers that follows from each being equal to
    the reference, and is asserted all the same.
(b) RANDOM data, one row per epilogue family on three forms each, whole and split 3:  |y - y64| <= c 2^-24 (conv(|x|, |w|) + |b| +
    |addend|) elementwise, c = K + splits + 8 the roundings on the longest chain (K products accumulated, the splits' partial sums,
    bias, slope, scales, addend, mask); bf16 products: x and w rounded to bf16 first; a bf16 output adds half a bf16 ulp of the
    value.  Statistics: c 2^-24 sum |y| and c 2^-24 sum y^2 per row tile and column.  Whole and split results differ by at most the
    sum of their bounds.  Derived, not fitted; the worst error / bound of each row is printed.
(c) MIXED: the cost model's own plan on 256 CUs, whole tiles and K-split tail tiles in one launch -- exact, skipped elsewhere.

Not here: PR = 3 (fp16 products) and the BIG forms stay with test_fp16_inference_gpu.py, gconv_multi_kernel and gconv_s2f_kernel
with test_forced_paths_gpu.py.  Times and the printed ratios: profiles/epilogue_forms_tests_times.txt."""
import ctypes as C
import functools
import math

import pytest
import torch

import epilogue_forms as EF
from epilogue_forms import SINGLE_TILES
from guarded import SENTINEL
from step_layers import prof_launches

pytestmark = pytest.mark.gpu

MARGIN = 4096    # elements of band on either side of a buffer
U = 2.0 ** -24
_SEEN = set()    # gconv_kernel instantiations this module's launches recorded


def _L():
    from torchsr_amd import _lib
    return _lib, _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(autouse=True)
def _forced_plan_reset(dev):
    """No other test sees a forced plan of this module."""
    try:
        yield
    finally:
        _, L = _L()
        assert L.srx_conv2d_force_plan(0, 0, 0, 0) == 0


class Band:
    """A contiguous tensor inside a larger device buffer: MARGIN elements of ``margin`` on either side (outputs: the sentinel; inputs:
    NaN, so that a read outside poisons the result), the interior ``fill`` or a copy of ``src``."""

    def __init__(self, dev, shape, dtype=torch.float32, fill=float('nan'), margin=SENTINEL, src=None, elems=MARGIN):
        n = math.prod(shape)
        self.m = elems
        self.buf = torch.full((2 * elems + n,), margin, dtype=dtype, device=dev)
        self.t = self.buf[elems:elems + n].view(shape)
        if src is not None:
            self.t.copy_(src)
        else:
            self.t.fill_(fill)
        self.margin = torch.tensor(margin, dtype=dtype)
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return self.t.data_ptr()

    def kept(self):
        got = torch.cat([self.buf[:self.m], self.buf[-self.m:]])
        return bool((_bits(got) == _bits(self.margin.to(got.device))).all())


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _nhwc(t, ld=None, pad=float('nan')):
    """NCHW -> NHWC with row stride ld, the columns past the tensor's own filled with ``pad``"""
    t = t.permute(0, 2, 3, 1)
    c = t.shape[-1]
    if ld is None or ld == c:
        return t.contiguous()
    out = torch.full(t.shape[:-1] + (ld,), pad, dtype=t.dtype)
    out[..., :c] = t
    return out


# ------------------------------------------------------------------------------------------------ operands and fp64 references
@functools.lru_cache(maxsize=None)
def _ops(layer, data, bf16):
    """CPU fp32 operands of a data row (NCHW / OIHW): 'int' or 'random' (bf16: rounded first)"""
    if data == 'int':
        return {k: torch.from_numpy(v).float() for k, v in EF.int_operands(layer).items()}
    return EF.random_operands(layer, bf16)


@functools.lru_cache(maxsize=None)
def _dev_ops(layer, data, bf16):
    """Device copies shared by every cell of the row: x and dy between NaN bands, packed weights, bias, and the NHWC addend / base /
    mask tensors the launches cut their own buffers from"""
    lib, L = _L()
    dev = torch.device('cuda:0')
    n, h, w, cin, cin_s, cout, cout_s, sh, up = EF.LAYERS[layer]
    ops = _ops(layer, data, bf16)
    d = lib.Conv2dDesc(n, h, w, cin, cin_s, cout, cout_s, 3, 3, 1, 1, sh, 0, 0.0, up, 0)
    g = dict(bias=ops['bias'].to(dev), w=ops['w'].to(dev))
    g['wf'] = torch.empty(L.srx_conv2d_packed_fwd_floats(C.byref(d)), device=dev)
    g['wb'] = torch.empty(max(L.srx_conv2d_packed_bwd_floats(C.byref(d)), 4), device=dev)
    lib.call('srx_conv2d_pack', C.byref(d), g['w'].data_ptr(), g['wf'].data_ptr(), g['wb'].data_ptr(), _stream())
    if cin_s == cin:
        g['x'] = Band(dev, (n, h, w, cin), margin=float('nan'), src=_nhwc(ops['x']))
    g['dy'] = Band(dev, tuple(_nhwc(ops['dy']).shape), margin=float('nan'), src=_nhwc(ops['dy']))
    for k in ('resid', 'addend', 'base', 'maskt'):
        g[k] = _nhwc(ops[k]).to(dev)
    torch.cuda.synchronize()
    return g


@functools.lru_cache(maxsize=None)
def _conv(layer, kind, data, bf16, absolute=False):
    ops = _ops(layer, data, bf16)
    return EF.conv_ref(layer, kind, EF.abs_ops(ops) if absolute else ops)


@functools.lru_cache(maxsize=None)
def _ref(id_, data, bf16):
    """(output, pre-activation) of the case in float64, NCHW"""
    e = EF.epilogue(id_)
    return EF.reference(e, _ops(e['layer'], data, bf16), _conv(e['layer'], e['kind'], data, bf16))


def _out_shape(e):
    n, h, w, cin, cin_s, cout, cout_s, sh, up = EF.LAYERS[e['layer']]
    ho, wo = EF.out_hw(e['layer'])
    k, cn, cs, ld, cnp = EF.columns(e)
    return (n, 2 * ho, 2 * wo, ld) if sh else (n, ho, wo, ld)


@functools.lru_cache(maxsize=None)
def _want_buffer(id_):
    """The whole output buffer an exact cell must leave, on the device: the reference in the layer's own columns, 0 up to the next
    quad, the sentinel past it"""
    e = EF.epilogue(id_)
    y, _ = _ref(id_, 'int', False)
    k, cn, cs, ld, cnp = EF.columns(e)
    if EF.LAYERS[e['layer']][7]:
        cn = cs = cn // 4
    want = torch.full(_out_shape(e), SENTINEL, dtype=torch.float32)
    want[..., :cs] = 0.0
    want[..., :cn] = y.permute(0, 2, 3, 1).float()
    assert torch.equal(want[..., :cn].double(), y.permute(0, 2, 3, 1))      # (the cast is exact)
    return want.to('cuda:0')


@functools.lru_cache(maxsize=None)
def _want_stats(id_, bm, data='int', bf16=False):
    return EF.stat_table(_ref(id_, data, bf16)[1], bm)


# ----------------------------------------------------------------------------------------------------------------- one launch
def _launch(dev, e, tile, split, data, forced=True, plan_want=None):
    """The cell's call under its forced plan (or the cost model's own: ``plan_want``), with plan, workspace size, launch record and
    bands checked.  Returns (output tensor [N][Ho][Wo][row stride] on the device, statistics table or None, plan)."""
    lib, L = _L()
    prec, bm, bn, ks_arg, ks = tile
    g = _dev_ops(e['layer'], data, bool(prec) and data == 'random')
    n, h, w, cin, cin_s, cout, cout_s, sh, up = EF.LAYERS[e['layer']]
    k, cn, cs, ld, cnp = EF.columns(e)
    d = lib.Conv2dDesc(*EF.desc_fields(e, prec))
    dref = C.byref(d)
    which = 1 if e['kind'] == 'dgrad' else 0
    if forced:
        lib.call('srx_conv2d_force_plan', bm, bn, split, ks_arg)
        wplan, wws, wrows, name = EF.expect(e, tile, split)
    else:
        wplan = plan_want
        assert wplan[3] == e['full'] + e['tail'] * wplan[2] and wplan[2] > 1
        wws = e['tail'] * wplan[2] * bm * bn
        wrows = -(-EF.rows(e['layer']) // bm)
        name = EF.expect(e, tile, 1)[3]
    ints = (C.c_int * 6)()
    lib.call('srx_conv2d_plan', dref, which, ints)
    assert list(ints) == wplan, (e['id'], tile, split, list(ints), wplan)
    nws = (L.srx_conv2d_bwd_data_ws_floats if which else L.srx_conv2d_fwd_ws_floats)(dref)
    assert nws == wws, (e['id'], tile, split, nws, wws)
    ws = Band(dev, (nws,)) if nws else None
    ws_ptr = ws.ptr() if nws else None
    s = _stream()
    # the output: NaN in the columns the launch owns (the accumulated gradient where it reads them), the sentinel past them
    shape = _out_shape(e)
    out = Band(dev, shape)
    lcs = cs // 4 if sh else cs
    out.t[..., lcs:] = SENTINEL
    if e['accumulate']:
        out.t[..., :cn] = g['base']
    part = None
    keep = []     # buffers of this launch
    if which == 0:
        bias = g['bias'].data_ptr() if e['bias'] else None
        if e['stats']:
            assert L.srx_conv2d_stat_rows(dref) == wrows
            part = Band(dev, (wrows, cn, 2))
        if e['resid']:
            resid = Band(dev, shape, margin=float('nan'))
            resid.t[..., :cn] = g['resid']
            keep.append(resid)
            run = lambda: lib.call(e['entry'], dref, g['x'].ptr(), g['wf'].data_ptr(), bias, resid.ptr(), EF.OUT_SCALE, out.ptr(),  # noqa: E731
                                   ws_ptr, nws, s)
        else:
            run = lambda: lib.call(e['entry'], dref, g['x'].ptr(), g['wf'].data_ptr(), bias, out.ptr(),  # noqa: E731
                                   part.ptr() if part else None, ws_ptr, nws, s)
    else:
        add = maskt = None
        if e['addend']:
            ald, ach, wide = e['addend']
            # (columns past addend_channels stay NaN: never read; the band is as long as a tile of rows at the OUTPUT's stride, so
            # that an addend addressed with the wrong stride reads NaN, not another allocation)
            add = Band(dev, shape[:3] + (ald,), margin=float('nan'), elems=256 * ld)
            add.t[..., :ach] = g['addend'][..., :ach]
        if e['mask']:
            lo, hi, slope = e['mask']
            maskt = Band(dev, shape, margin=float('nan'))                # (columns outside the range stay NaN: never read)
            maskt.t[..., lo:hi] = g['maskt'][..., lo:hi]
        keep += [add, maskt]
        dy, wb = g['dy'].ptr(), g['wb'].data_ptr()
        if e['entry'] == 'srx_conv2d_bwd_data':
            run = lambda: lib.call(e['entry'], dref, dy, wb, out.ptr(), int(e['accumulate']), ws_ptr, nws, s)  # noqa: E731
        elif e['entry'] == 'srx_conv2d_bwd_data_add':
            run = lambda: lib.call(e['entry'], dref, dy, wb, add.ptr(), out.ptr(), ws_ptr, nws, s)  # noqa: E731
        elif e['entry'] == 'srx_conv2d_bwd_data_act':
            run = lambda: lib.call(e['entry'], dref, dy, wb, maskt.ptr(), slope, lo, hi, int(e['accumulate']), out.ptr(), ws_ptr,  # noqa: E731
                                   nws, s)
        else:
            ep = lib.DgradEpilogue()
            ep.out_scale, ep.addend_scale = e['scales']
            ep.addend, ep.addend_ld, ep.addend_channels = add.ptr(), ald, ach
            ep.act_out, ep.act_slope, ep.c_lo, ep.c_hi = maskt.ptr(), slope, lo, hi
            run = lambda: lib.call(e['entry'], dref, dy, wb, out.ptr(), C.byref(ep), ws_ptr, nws, s)  # noqa: E731
    names = prof_launches(run)
    lib.call('srx_conv2d_force_plan', 0, 0, 0, 0)
    assert names == [name], (e['id'], tile, split, names, name)
    _SEEN.add(name.split(' MxNxK')[0])
    for what, buf in (('output', out), ('workspace', ws), ('statistics', part)):
        assert buf is None or buf.kept(), (e['id'], tile, split, what, 'bands')
    return out.t, (part.t if part is not None else None), list(ints)


def _assert_bits(got, want, what):
    if not torch.equal(_bits(got), _bits(want)):
        bad = (_bits(got) != _bits(want)).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError('%s: %d of %d elements differ in their bits (%d NaN); first at %s: got %r, want %r; rows %s, columns %s'
                             % (what, len(bad), want.numel(), int(torch.isnan(got).sum()), i, float(got[i]), float(want[i]),
                                sorted(set(bad[:, -2 if bad.shape[1] > 1 else 0].tolist()))[:8], sorted(set(bad[:, -1].tolist()))[:8]))


# ------------------------------------------------------------------------------------------------------------ (a) exact
def _run_exact(dev, e, tile):
    results = []
    for split in EF.SPLITS:
        out, part, plan = _launch(dev, e, tile, split, 'int')
        what = (e['id'], EF.tile_id(tile), 'split %d' % split)
        _assert_bits(out, _want_buffer(e['id']), '%s %s %s output' % what)
        if part is not None:
            want = _want_stats(e['id'], tile[1])
            assert float(want.abs().max()) < EF.EXACT
            _assert_bits(part, want.float().to(dev), '%s %s %s statistics' % what)
        results.append((out, part))
    (o1, p1), (o3, p3) = results
    assert torch.equal(_bits(o1), _bits(o3)) and (p1 is None or torch.equal(_bits(p1), _bits(p3)))


@pytest.mark.parametrize('tile', SINGLE_TILES, ids=[EF.tile_id(t) for t in SINGLE_TILES])
@pytest.mark.parametrize('id_', [e['id'] for e in EF.EPILOGUES])
def test_epilogue_is_exact_on_integers_whole_and_split(dev, id_, tile):
    """Whole (split 1) and split 3 (every tile through tail_fixup_kernel) of one cell: each bit for bit equal to the float64
    reference, hence to each other.  The shuffled store runs unsplit both times, and the plan says so."""
    _run_exact(dev, EF.epilogue(id_), tile)


@pytest.mark.parametrize('m', EF.MIXED, ids=[m['id'] for m in EF.MIXED])
def test_mixed_launch_of_whole_and_cut_tiles_is_exact(dev, m):
    _, L = _L()
    if L.srx_plan_cus() != EF.CUS:
        pytest.skip(EF.MIXED_SKIP % L.srx_plan_cus())
    out, part, plan = _launch(dev, m, m['tile'], None, 'int', forced=False, plan_want=m['plan'])
    _assert_bits(out, _want_buffer(m['id']), m['id'] + ' output')
    if part is not None:
        _assert_bits(part, _want_stats(m['id'], m['tile'][1]).float().to(dev), m['id'] + ' statistics')


# ------------------------------------------------------------------------------------------------------------ bf16 storage
@functools.lru_cache(maxsize=None)
def _bf16s_ops(data):
    """Layer A's operands as the bf16 tensors the bf16-storage entry points take, and the two bf16 weight packs"""
    lib, L = _L()
    dev = torch.device('cuda:0')
    ops = _ops('A', data, True)
    d = lib.Conv2dDesc(*EF.desc_fields(EF.epilogue('S.fwd16'), 1))
    nb = L.srx_conv3x3_bf16s_packed_bytes(C.byref(d))
    assert nb == 128 * 9 * 128 * 2
    g = dict(bias=ops['bias'].to(dev), w=ops['w'].to(dev), wf=torch.empty(nb // 2, dtype=torch.bfloat16, device=dev),
             wb=torch.empty(nb // 2, dtype=torch.bfloat16, device=dev))
    lib.call('srx_conv3x3_bf16s_pack', C.byref(d), g['w'].data_ptr(), g['wf'].data_ptr(), g['wb'].data_ptr(), _stream())
    for k in ('x', 'dy', 'maskt'):
        t = _nhwc(ops[k])
        assert torch.equal(t.bfloat16().float(), t)
        g[k] = Band(dev, tuple(t.shape), dtype=torch.bfloat16, margin=float('nan'), src=t.bfloat16())
    torch.cuda.synchronize()
    return g


def _launch_bf16s(dev, e, tile, split, data, raw=False):
    lib, L = _L()
    bm, bn, ks_arg, ks = tile
    g = _bf16s_ops(data)
    d = lib.Conv2dDesc(*EF.desc_fields(e, 1))
    dref = C.byref(d)
    which = 1 if e['kind'] == 'dgrad' else 0
    lib.call('srx_conv2d_force_plan', bm, bn, split, ks_arg)
    wws, name = EF.expect_bf16s(e, tile, split)
    nws = L.srx_conv3x3_bf16s_ws_floats(dref, which)
    assert nws == wws, (e['id'], tile, split, nws, wws)
    ws = Band(dev, (nws,)) if nws else None
    ws_ptr = ws.ptr() if nws else None
    out = Band(dev, (2, 22, 18, 128), dtype=torch.bfloat16 if e['out16'] else torch.float32)
    s = _stream()
    rc = []
    if which == 0:
        args = ('srx_conv3x3_bf16s_fwd', dref, g['x'].ptr(), g['wf'].data_ptr(), g['bias'].data_ptr(), int(e['relu']), out.ptr(),
                int(e['out16']), ws_ptr, nws, s)
    else:
        args = ('srx_conv3x3_bf16s_bwd_data', dref, g['dy'].ptr(), g['wb'].data_ptr(), g['maskt'].ptr() if e['relu'] else None,
                out.ptr(), int(e['out16']), ws_ptr, nws, s)
    if raw:
        names = prof_launches(lambda: rc.append(getattr(L, args[0])(*args[1:])))
        lib.call('srx_conv2d_force_plan', 0, 0, 0, 0)
        return out, names, rc[0]
    names = prof_launches(lambda: lib.call(*args))
    lib.call('srx_conv2d_force_plan', 0, 0, 0, 0)
    assert names == [name], (e['id'], tile, split, names, name)
    _SEEN.add(name.split(' MxNxK')[0])
    assert out.kept() and (ws is None or ws.kept()), (e['id'], tile, split, 'bands')
    return out.t


def _run_exact_bf16s(dev, e, tile):
    y, _ = _ref(e['id'], 'int', False)
    want = y.permute(0, 2, 3, 1).float().contiguous()
    want = (want.bfloat16() if e['out16'] else want).to(dev)
    assert torch.equal(want.double().cpu(), y.permute(0, 2, 3, 1))
    outs = []
    for split in EF.SPLITS:
        out = _launch_bf16s(dev, e, tile, split, 'int')
        _assert_bits(out, want, '%s %s split %d output' % (e['id'], EF.tile_id(tile), split))
        outs.append(out)
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))


@pytest.mark.parametrize('tile', EF.BF16S_TILES, ids=[EF.tile_id(t) for t in EF.BF16S_TILES])
@pytest.mark.parametrize('id_', [e['id'] for e in EF.BF16S])
def test_bf16_storage_epilogue_is_exact_on_integers_whole_and_split(dev, id_, tile):
    """out16 / mask16: the bf16 store and the bf16 mask load of store_tile and of tail_fixup_kernel, into a bf16 and into an fp32
    output.  |y| <= 256 on these operands, so .bfloat16() of the exact value is exact as well."""
    _run_exact_bf16s(dev, EF.epilogue(id_), tile)


@pytest.mark.parametrize('tile', EF.BF16S_REFUSED, ids=[EF.tile_id(t) for t in EF.BF16S_REFUSED])
def test_bf16_storage_refuses_a_tile_it_has_no_kernel_for(dev, tile):
    """128 x 32 and 64 x 32 exist with bf16 products, not with bf16 storage: forced_tile_refusal lets them through (it asks for the
    bf16-product instantiation), run_gconv refuses them before launching -- SRX_E_UNSUPPORTED, the output untouched, the launch
    recorder empty."""
    lib, _ = _L()
    for id_ in ('S.fwd16', 'S.dmask32'):
        for split in EF.SPLITS:
            out, names, rc = _launch_bf16s(dev, EF.epilogue(id_), tile, split, 'int', raw=True)
            assert rc == 2 and 'no bf16-storage kernel for tile' in lib.last_error(), (rc, lib.last_error())
            assert names == [], names
            torch.cuda.synchronize()
            assert bool(torch.isnan(out.t).all()) and out.kept()


# ------------------------------------------------------------------------------------------------------------ (b) random
def _bound(e, data_bf16, splits):
    """c 2^-24 (conv(|x|, |w|) + |b| + |addend|), NCHW float64, and c"""
    ops = _ops(e['layer'], 'random', data_bf16)
    k = EF.columns(e)[0]
    c = 9 * k + splits + 8
    mag = _conv(e['layer'], e['kind'], 'random', data_bf16, True).clone()
    if e.get('bias'):
        mag += ops['bias'].double().abs().view(1, -1, 1, 1)
    if e.get('addend'):
        ch = e['addend'][1]
        mag[:, :ch] += ops['addend'].double().abs()[:, :ch]
    return c * U * mag, c


def _check_random(e, got, part, bm, data_bf16, splits, what):
    """got: NCHW float64 of the layer's own columns.  Returns the row's bound for the whole-against-split comparison."""
    want, pre = _ref(e['id'], 'random', data_bf16)
    bound, c = _bound(e, data_bf16, splits)
    if e.get('out16'):   # half a bf16 ulp of the value (of the largest value the fp32 result can have)
        bound = bound + torch.exp2(torch.floor(torch.log2((want.abs() + bound).clamp_min(1e-300))) - 8)
    assert bool(torch.isfinite(got).all()), (what, 'not finite')
    err = (got - want).abs()
    ratio = (err / bound).max().item()
    line = 'EPIFORM random %s c %d worst err / bound %.3f' % (what, c, ratio)
    if part is not None:
        t = EF.stat_table(pre, bm)
        a = EF.stat_table(pre.abs(), bm)
        e1, e2 = (part[..., 0].double() - t[..., 0]).abs(), (part[..., 1].double() - t[..., 1]).abs()
        r1, r2 = (e1 / (c * U * a[..., 0])).max().item(), (e2 / (c * U * t[..., 1])).max().item()
        line += '  statistics: sum %.3f  sum of squares %.3f' % (r1, r2)
    print(line)
    outside = int((err > bound).sum())
    assert outside == 0, (what, f'{outside} of {err.numel()} elements outside the derived bound', ratio)
    if part is not None:
        assert r1 <= 1.0 and r2 <= 1.0, (what, 'statistics', r1, r2)
    return bound


@pytest.mark.parametrize('tile', EF.RANDOM_FORMS, ids=[EF.tile_id(t) for t in EF.RANDOM_FORMS])
@pytest.mark.parametrize('id_', EF.RANDOM_IDS)
def test_epilogue_within_the_derived_bound_of_fp64_on_random_data(dev, id_, tile):
    e = EF.epilogue(id_)
    cn = EF.columns(e)[1]
    bf16 = bool(tile[0])
    outs, bounds = [], []
    for split in EF.SPLITS:
        out, part, plan = _launch(dev, e, tile, split, 'random')
        assert plan[2] == split
        got = out[..., :cn].permute(0, 3, 1, 2).double().cpu()
        what = '%s %s split %d' % (id_, EF.tile_id(tile), split)
        bounds.append(_check_random(e, got, None if part is None else part.cpu(), tile[1], bf16, split, what))
        outs.append(got)
    assert bool(((outs[0] - outs[1]).abs() <= bounds[0] + bounds[1]).all())


@pytest.mark.parametrize('tile', EF.RANDOM_BF16S_FORMS, ids=[EF.tile_id(t) for t in EF.RANDOM_BF16S_FORMS])
@pytest.mark.parametrize('id_', EF.RANDOM_BF16S_IDS)
def test_bf16_storage_within_the_derived_bound_of_fp64_on_random_data(dev, id_, tile):
    e = EF.epilogue(id_)
    outs, bounds = [], []
    for split in EF.SPLITS:
        out = _launch_bf16s(dev, e, tile, split, 'random')
        got = out.permute(0, 3, 1, 2).double().cpu()
        bounds.append(_check_random(e, got, None, tile[0], True, split, '%s %s split %d' % (id_, EF.tile_id(tile), split)))
        outs.append(got)
    assert bool(((outs[0] - outs[1]).abs() <= bounds[0] + bounds[1]).all())


def test_zz_every_gconv_kernel_instantiation_ran(dev):
    """Over the whole file the launch records covered every gconv_kernel instantiation kTiles lists under F_GCONV for PR 0, 1 and 2
    (forms this process has not launched yet are launched here)."""
    for t in SINGLE_TILES:
        if EF.kernel_name(t[0], t[1], t[2], t[4]) not in _SEEN:
            _run_exact(dev, EF.epilogue('A.lrelu'), t)
    for t in EF.BF16S_TILES:
        if EF.kernel_name(2, t[0], t[1], t[3]) not in _SEEN:
            _run_exact_bf16s(dev, EF.epilogue('S.fwd16'), t)
    print('EPIFORM instantiations recorded:', len(_SEEN))
    assert sorted(_SEEN) == sorted(EF.ALL_INSTANTIATIONS), sorted(set(EF.ALL_INSTANTIATIONS) ^ _SEEN)
