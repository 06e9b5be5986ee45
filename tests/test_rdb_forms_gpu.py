"""Every calling form of the fused dense block (rdb.hip; cases and the float64 restatement: rdb_forms.py), through the C ABI so that
no module can route a call elsewhere.  Every device tensor the kernel reads or writes lies in a guarded.Guarded buffer: inputs
between NaN bands with NaN in the channels behind them (a read outside a tensor poisons the result), outputs all NaN between
sentinel bands with NaN or the sentinel in their slack channels; after a call every band, every slack channel and every input is
compared bit for bit with what it held.

(a) EXACT, every shape of rdb_forms.SHAPES, both slopes, every form.  On the integer operands every fp32 operation of the kernel is
    exact (the condition is asserted as the reference is computed: rdb_forms.assert_exact; on the CPU alone in
    test_rdb_forms_cpu.py), so c1..c4 and out, g4..g1 and dx must EQUAL a float64 restatement that never sees a device value.  A
    wrong tap, a wrong zero in the halo, a wrong stride, a tile computed twice or not at all, a bf16 rounding that is not to nearest
    even: each is off by at least a quarter at some element.
      forward forms  a: middle of an RRDB (no addend, out = a 192-channel buffer)   b: end of an RRDB (extra = the x channels of a
                     192-channel buffer)   c: last block (out_ld = 64)   d: slack in every stride (200 / 68 / 72)
      backward forms product (64 / 64 / 64, 192 / 192) without and with extra; slack (72 / 68 / 76 / 80, 200 / 196)
(b) the chain of functional._DenseBlock: three blocks of different weights out of ONE srx_rdb_pack / srx_rdb_pack_bwd launch, block
    i on the stream at i * srx_rdb_packed_bytes(), the buffers rotating, the third block adding the first one's x -- equal to the
    float64 chain, forward and (in reverse order) backward.
(c) srx_rdb_fwd_dbg computes the bits srx_rdb_fwd computes and writes its stamps inside [workgroups][8][48].
(d) RANDOM data (the distributions of test_ops_gpu.py's two tests), every shape, form b forward and the product form with extra
    backward, stage by stage on the device's own earlier stages (an fp32 ulp can flip a bf16 rounding of the next stage: not an
    error), every ELEMENT inside  gamma_k (|a| conv |w| [+ |b|, |x|, |extra|, |skip|])  of float64 on the bf16-rounded operands,
    k counted from rdb.hip (rdb_forms.fwd_k / out_k / bwd_k / dx_k).  Behind the LeakyReLU the bound carries the slope where the
    branch is certain (forward: the float64 pre-activation is further below 0 than its own bound; backward: the mask is an input).

Times and the worst ratios of (d): profiles/rdb_forms_tests_times.txt."""
import ctypes as C

import pytest
import torch

import rdb_forms as RF
from guarded import Guarded, SENTINEL
from step_layers import gamma, prof_launches

pytestmark = pytest.mark.gpu
NAN = float('nan')
SHAPES = list(RF.SHAPES)
SHAPE_IDS = [RF.shape_id(s) for s in SHAPES]


def _L():
    from torchsr_amd import _lib
    return _lib, _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _strided(t, ld, tail=NAN):
    """NCHW -> a CPU (N, H, W, ld) tensor: the channels of ``t``, then ``tail``"""
    n, c, h, w = t.shape
    out = torch.full((n, h, w, ld), tail)
    out[..., :c] = _nhwc(t)
    return out


def _kept(name, g, before=None):
    """The bands of a Guarded buffer, and (``before``: the CPU tensor it was filled from) its whole interior, are what they were"""
    assert g.margins_unchanged(), (name, 'bands')
    if before is not None:
        assert _same_bits(g.t.cpu(), before), (name, 'changed')


def _equal(got, want, what, shape):
    """torch.equal(got, float64 restatement), with the first differing element placed relative to tile and image borders"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if torch.equal(got.double(), want):
        return
    bad = (got.double() != want).nonzero()        # (a NaN -- an element never written -- differs too)
    n, c, y, x = bad[0].tolist()
    raise AssertionError('%s: %d of %d elements differ (%d NaN); first at image %d channel %d pixel (%d, %d) = tile (%d, %d) + (%d, %d) of '
                         '%dx%dx%d: got %r, float64 %r' % (what, len(bad), want.numel(), int(torch.isnan(got).sum()), n, c, y, x, y // 8, x // 8,
                                                        y % 8, x % 8, *shape, float(got[n, c, y, x]), float(want[n, c, y, x])))


class Pack:
    """The bf16 streams of ``blocks`` (a list of five-weight lists) out of ONE pack launch: the table of 5 x blocks weight pointers,
    the weights between NaN bands, the streams exactly blocks x srx_rdb_packed_bytes() long between sentinel bands."""

    def __init__(self, dev, blocks, bwd):
        lib, L = _L()
        self.per = L.srx_rdb_packed_bytes()
        assert self.per == 479232
        self.w = [Guarded(dev, tuple(w.shape), w) for ws in blocks for w in ws]
        self.table = torch.tensor([g.t.data_ptr() for g in self.w], dtype=torch.int64).to(dev)
        self.pk = Guarded(dev, (len(blocks) * self.per // 4,), margin=SENTINEL, margin_floats=4096)
        lib.call('srx_rdb_pack_bwd' if bwd else 'srx_rdb_pack', self.table.data_ptr(), len(blocks), self.pk.ptr(), _stream())
        torch.cuda.synchronize()
        self.check()
        # every 4 bytes of the streams were written: none still holds the fill (NaN is no pair of bf16 weights of these tests)
        assert not bool(torch.isnan(self.pk.t).any()), 'pack: bytes never written'

    def ptr(self, i=0):
        return C.c_void_p(self.pk.t.data_ptr() + i * self.per)

    def check(self):
        _kept('packed streams', self.pk)
        for g in self.w:
            _kept('weights', g)


def _biases(dev, bs):
    gs = [Guarded(dev, tuple(b.shape), b, margin_floats=256) for b in bs]
    return gs, (C.c_void_p * 5)(*[g.t.data_ptr() for g in gs])


# --------------------------------------------------------------------------------------------------------------- one forward call
def _run_fwd(dev, shape, ops, pack_ptr, form, scale, slope, post_scale, dbg=None, records=False):
    """srx_rdb_fwd (``dbg``: srx_rdb_fwd_dbg with that stamp buffer) in one of rdb_forms.FWD_FORMS.  Returns (c1..c4 as (N, 128, H, W), out
    as (N, 64, H, W)) on the CPU after every check of what the call must leave alone."""
    lib, L = _L()
    n, h, w = shape
    f = RF.FWD_FORMS[form]
    ld, out_ld, extra_ld = f['ld'], f['out_ld'], f['extra_ld']
    buf0 = _strided(ops['x'], ld)
    buf0[..., 192:] = SENTINEL
    buf = Guarded(dev, tuple(buf0.shape), buf0, margin=SENTINEL)
    out0 = torch.full((n, h, w, out_ld), NAN)
    out0[..., 64:] = SENTINEL if form == 'd' else NAN    # (form a: 'channels 64..191 of out stay NaN')
    out = Guarded(dev, tuple(out0.shape), out0, margin=SENTINEL)
    extra0 = _strided(ops['extra'], extra_ld) if extra_ld else None   # the other channels of the older buffer: NaN
    extra = Guarded(dev, tuple(extra0.shape), extra0) if extra_ld else None
    bg, barr = _biases(dev, ops['bs'])
    s = _stream()

    def run():
        if dbg is not None:
            fn = L.srx_rdb_fwd_dbg      # a developer entry point: bound here, as tools/bench_rdb.py binds it
            fn.restype = C.c_int
            fn.argtypes = [C.c_int] * 3 + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
            rc = fn(n, h, w, buf.ptr(), ld, pack_ptr, barr, scale, slope, out.ptr(), out_ld, s, dbg.ptr())
            assert rc == 0, lib.last_error()
        else:
            lib.call('srx_rdb_fwd', n, h, w, buf.ptr(), ld, pack_ptr, barr, scale, slope, post_scale if extra_ld else 1.0,
                     extra.ptr() if extra_ld else None, extra_ld or 0, out.ptr(), out_ld, s)
    if records:
        names = prof_launches(run)
        assert names == ['rdb_kernel<0> MxNxK=%dx192x(576..1728)' % (n * h * w)], names
    else:
        run()
    torch.cuda.synchronize()
    gb, go = buf.t.cpu(), out.t.cpu()
    tag = (RF.shape_id(shape), 'forward form ' + form)
    assert _same_bits(gb[..., :64], buf0[..., :64]), (tag, 'the x channels of buf changed')
    assert _same_bits(gb[..., 192:], buf0[..., 192:]), (tag, 'slack channels of buf changed')
    assert _same_bits(go[..., 64:], out0[..., 64:]), (tag, 'channels of out behind the result changed')
    _kept(tag + ('buf',), buf)
    _kept(tag + ('out',), out)
    if extra_ld:
        _kept(tag + ('extra',), extra, extra0)
    for g, b in zip(bg, ops['bs']):
        _kept(tag + ('bias',), g, b)
    return _nchw(gb[..., 64:192]), _nchw(go[..., :64])


# -------------------------------------------------------------------------------------------------------------- one backward call
def _run_bwd(dev, shape, dy, acts, skip, extra, pack_ptr, form, scale, slope, skip_scale, records=False):
    """srx_rdb_bwd in one of rdb_forms.BWD_FORMS (``extra`` is passed where the form has an extra_ld; ``skip is dy``: one device
    tensor for both).  Returns ({j: g_j}, dx) on the CPU."""
    lib, _ = _L()
    n, h, w = shape
    f = RF.BWD_FORMS[form]
    ins = dict(dy=_strided(dy, f['dy_ld']), buf=_strided(acts, f['ld']))
    if skip is not dy:       # (the chain: skip IS dy, one tensor, as functional._DenseBlock passes it)
        ins['skip'] = _strided(skip, f['skip_ld'])
    else:
        assert f['skip_ld'] == f['dy_ld']
    if f['extra_ld']:
        ins['extra'] = _strided(extra, f['extra_ld'])
    gin = {k: Guarded(dev, tuple(v.shape), v) for k, v in ins.items()}
    g0 = torch.full((n, h, w, f['gld']), NAN)
    g0[..., 192:] = SENTINEL
    gbuf = Guarded(dev, tuple(g0.shape), g0, margin=SENTINEL)
    dx0 = torch.full((n, h, w, f['dx_ld']), NAN)
    dx0[..., 64:] = SENTINEL
    dx = Guarded(dev, tuple(dx0.shape), dx0, margin=SENTINEL)

    def run():
        lib.call('srx_rdb_bwd', n, h, w, gin['dy'].ptr(), f['dy_ld'], scale, gin['buf'].ptr(), f['ld'], pack_ptr, slope, gbuf.ptr(), f['gld'],
                 gin['skip' if 'skip' in gin else 'dy'].ptr(), f['skip_ld'], skip_scale, gin['extra'].ptr() if f['extra_ld'] else None, f['extra_ld'] or 0, dx.ptr(),
                 f['dx_ld'], _stream())
    if records:
        names = prof_launches(run)
        assert names == ['rdb_kernel<1> MxNxK=%dx192x(576..1728)' % (n * h * w)], names
    else:
        run()
    torch.cuda.synchronize()
    gg, gd = gbuf.t.cpu(), dx.t.cpu()
    tag = (RF.shape_id(shape), 'backward form ' + form)
    assert _same_bits(gg[..., :64], g0[..., :64]), (tag, 'channels 0..63 of gbuf changed')
    assert _same_bits(gg[..., 192:], g0[..., 192:]), (tag, 'slack channels of gbuf changed')
    assert _same_bits(gd[..., 64:], dx0[..., 64:]), (tag, 'slack channels of dx changed')
    _kept(tag + ('gbuf',), gbuf)
    _kept(tag + ('dx',), dx)
    for k, g in gin.items():
        _kept(tag + (k,), g, ins[k])
    return {j: _nchw(gg[..., 64 + 32 * (j - 1):64 + 32 * j]) for j in (4, 3, 2, 1)}, _nchw(gd[..., :64])


# ------------------------------------------------------------------------------------------------------- (a) exact on integers
@pytest.mark.parametrize('variant', list(RF.VARIANTS))
@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_forward_is_exact_on_integers_in_every_form(dev, shape, variant):
    ops, ref, slope = RF.int_operands(shape), RF.exact_forward(shape, variant), RF.VARIANTS[variant]
    pack = Pack(dev, [ops['ws']], bwd=False)
    want_c = torch.cat(ref['c'], 1)
    for form, f in RF.FWD_FORMS.items():
        got_c, got_out = _run_fwd(dev, shape, ops, pack.ptr(), form, RF.SCALE, slope, RF.POST_SCALE, records=form == 'a')
        what = 'forward %s %s form %s ' % (RF.shape_id(shape), variant, form)
        for k in range(4):
            _equal(got_c[:, 32 * k:32 * k + 32], ref['c'][k], what + 'c%d' % (k + 1), shape)
        assert torch.equal(got_c.double(), want_c)
        _equal(got_out, ref['out'] if f['extra_ld'] else ref['y0'], what + 'out', shape)
    pack.check()


@pytest.mark.parametrize('variant', list(RF.VARIANTS))
@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_backward_is_exact_on_integers_in_every_form(dev, shape, variant):
    ops, ref, slope = RF.int_operands(shape), RF.exact_backward(shape, variant), RF.VARIANTS[variant]
    pack = Pack(dev, [ops['ws']], bwd=True)
    for form, f in RF.BWD_FORMS.items():
        got_g, got_dx = _run_bwd(dev, shape, ops['dy'], ops['acts'], ops['skip'], ops['extra'], pack.ptr(), form, RF.SCALE, slope,
                                 RF.SKIP_SCALE, records=form == 'product')
        what = 'backward %s %s form %s ' % (RF.shape_id(shape), variant, form)
        for j in (4, 3, 2, 1):
            _equal(got_g[j], ref['g'][j], what + 'g%d' % j, shape)
        _equal(got_dx, ref['dx'] if f['extra_ld'] else ref['dx0'], what + 'dx', shape)
    pack.check()


# ------------------------------------------------------------------------------------------------- (b) a chain out of one pack
@pytest.mark.parametrize('variant', list(RF.VARIANTS))
def test_forward_chain_of_three_blocks_out_of_one_pack(dev, variant):
    """As functional._DenseBlock.forward: block i reads buffer i and the stream at pack + i * srx_rdb_packed_bytes(), writes the x
    channels of buffer i + 1; the third block writes a dense 64-channel tensor, the first buffer its second addend."""
    lib, _ = _L()
    ch, slope, shape = RF.exact_chain(variant), RF.VARIANTS[variant], RF.CHAIN_SHAPE
    n, h, w = shape
    pack = Pack(dev, [b[0] for b in ch['ops']['blocks']], bwd=False)
    first = _strided(ch['ops']['x'], 192)
    bufs = [Guarded(dev, (n, h, w, 192), first if i == 0 else None, margin=SENTINEL) for i in range(3)]
    out = Guarded(dev, (n, h, w, 64), margin=SENTINEL)
    keep = []
    for i in range(3):
        bg, barr = _biases(dev, ch['ops']['blocks'][i][1])
        keep.append(bg)
        if i == 2:
            lib.call('srx_rdb_fwd', n, h, w, bufs[i].ptr(), 192, pack.ptr(i), barr, RF.SCALE, slope, RF.POST_SCALE, bufs[0].ptr(), 192, out.ptr(), 64, _stream())
        else:
            lib.call('srx_rdb_fwd', n, h, w, bufs[i].ptr(), 192, pack.ptr(i), barr, RF.SCALE, slope, 1.0, None, 0, bufs[i + 1].ptr(), 192, _stream())
    torch.cuda.synchronize()
    for i in range(3):
        got = _nchw(bufs[i].t.cpu())
        what = 'chain %s block %d ' % (variant, i)
        _equal(got[:, :64], ch['bufs'][i][:, :64].double(), what + 'x', shape)
        for k in range(4):
            _equal(got[:, 64 + 32 * k:96 + 32 * k], ch['fwd'][i]['c'][k], what + 'c%d' % (k + 1), shape)
        _kept(what, bufs[i])
    _equal(_nchw(out.t.cpu()), ch['out'], 'chain %s out' % variant, shape)
    _kept('chain out', out)
    pack.check()


@pytest.mark.parametrize('variant', list(RF.VARIANTS))
def test_backward_chain_of_three_blocks_out_of_one_pack(dev, variant):
    """As functional._DenseBlock.backward, last block first: skip IS dy (one tensor), the third block sees rrdb_scale of the output
    gradient, the first adds the RRDB's own output gradient as `extra`; block i reads the stream at pack + i * packed_bytes."""
    ch, slope, shape = RF.exact_chain(variant), RF.VARIANTS[variant], RF.CHAIN_SHAPE
    pack = Pack(dev, [b[0] for b in ch['ops']['blocks']], bwd=True)
    for i in (2, 1, 0):
        a, ref = ch['bwd_args'][i], ch['bwd'][i]
        form = 'product+extra' if a['extra'] is not None else 'product'
        got_g, got_dx = _run_bwd(dev, shape, a['dy'], ch['bufs'][i], a['skip'], a['extra'], pack.ptr(i), form, a['scale'], slope, a['skip_scale'])
        what = 'chain %s backward block %d ' % (variant, i)
        for j in (4, 3, 2, 1):
            _equal(got_g[j], ref['g'][j], what + 'g%d' % j, shape)
        _equal(got_dx, ref['dx'], what + 'dx', shape)
    pack.check()


# -------------------------------------------------------------------------------------------------- (c) the stamped entry point
def test_stamped_entry_point_computes_the_same_bits(dev):
    shape = (3, 24, 24)
    ops, p = RF.random_operands(shape), RF.RANDOM_FWD
    pack = Pack(dev, [ops['ws']], bwd=False)
    c, out = _run_fwd(dev, shape, ops, pack.ptr(), 'a', p['scale'], p['slope'], 1.0)
    stamps = Guarded(dev, (RF.workgroups(shape), 8, 48), margin=SENTINEL, margin_floats=4096)
    c_dbg, out_dbg = _run_fwd(dev, shape, ops, pack.ptr(), 'a', p['scale'], p['slope'], 1.0, dbg=stamps)
    assert bool(torch.isfinite(c).all()) and bool(torch.isfinite(out).all())
    assert _same_bits(c_dbg, c) and _same_bits(out_dbg, out)
    _kept('stamps', stamps)
    # every wave of every workgroup copied its 48 slots; slot 0 (kernel start) and slot 1 (patch staged) are stamps of one clock
    st = stamps.t.cpu().view(torch.int32)
    assert not bool((st == torch.tensor(NAN).view(torch.int32)).all(-1).any()), 'a wave wrote no stamps'
    pack.check()


# ------------------------------------------------------------------------------------- (d) random data, bounded element by element
WORST = {}


def _ratio(got, want, bound, what, tag):
    """worst |got - want| / bound; every element inside its bound (NaN-proof)"""
    err = (got.double() - want).abs()
    assert bool(torch.isfinite(got).all()), (what, 'not finite')
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    WORST[tag] = max(WORST.get(tag, 0.0), ratio)
    outside = int((~(err <= bound)).sum())
    return ratio, outside


@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_forward_within_the_derived_bound_of_fp64(dev, shape):
    ops, p = RF.random_operands(shape), RF.RANDOM_FWD
    pack = Pack(dev, [ops['ws']], bwd=False)
    got_c, got_out = _run_fwd(dev, shape, ops, pack.ptr(), 'b', p['scale'], p['slope'], p['post_scale'])
    given = [got_c[:, 32 * k:32 * k + 32].contiguous() for k in range(4)]
    ref = RF.forward64(ops['x'], ops['ws'], ops['bs'], p['scale'], p['slope'], given=given)
    res = []
    for k in range(1, 5):
        mag = ref['mag'][k - 1]
        g = gamma(RF.fwd_k(k))
        mag = torch.where(ref['pre'][k - 1] < -g * mag, p['slope'] * mag, mag)    # the negative branch for certain: its slope
        res.append(_ratio(given[k - 1], ref['c'][k - 1], g * mag, 'c%d' % k, 'forward c%d' % k))
    want = RF.fwd_out(ref['y0'], p['post_scale'], ops['extra'])
    mag = (ref['mag'][4] * p['scale'] + ops['x'].double().abs()) * p['post_scale'] + ops['extra'].double().abs()
    res.append(_ratio(got_out, want, gamma(RF.out_k(True)) * mag, 'out', 'forward out'))
    print('RDBFORM forward %s random: worst |err| / bound  c1..c4 %s  out %.3f' % (RF.shape_id(shape), ' '.join('%.3f' % r for r, _ in res[:4]), res[4][0]))
    assert all(o == 0 for _, o in res), (RF.shape_id(shape), 'elements outside the derived bound (c1..c4, out):', [o for _, o in res], [r for r, _ in res])
    pack.check()


@pytest.mark.parametrize('shape', SHAPES, ids=SHAPE_IDS)
def test_backward_within_the_derived_bound_of_fp64(dev, shape):
    ops, p = RF.random_operands(shape), RF.RANDOM_BWD
    pack = Pack(dev, [ops['ws']], bwd=True)
    got_g, got_dx = _run_bwd(dev, shape, ops['dy'], ops['acts'], ops['skip'], ops['extra'], pack.ptr(), 'product+extra', p['scale'], p['slope'],
                             p['skip_scale'])
    ref = RF.backward64(ops['dy'], ops['acts'], ops['ws'], p['scale'], p['slope'], ops['skip'], p['skip_scale'], ops['extra'], given=got_g)
    res = []
    for j in (4, 3, 2, 1):
        lo = 64 + 32 * (j - 1)
        branch = torch.where(ops['acts'][:, lo:lo + 32] > 0, 1.0, p['slope']).double()   # the mask is an input: the branch is certain
        res.append(_ratio(got_g[j], ref['g'][j], gamma(RF.bwd_k(j)) * ref['mag'][j] * branch, 'g%d' % j, 'backward g%d' % j))
    res.append(_ratio(got_dx, ref['dx'], gamma(RF.dx_k(True)) * ref['mag'][0], 'dx', 'backward dx'))
    print('RDBFORM backward %s random: worst |err| / bound  g4..g1 %s  dx %.3f' % (RF.shape_id(shape), ' '.join('%.3f' % r for r, _ in res[:4]), res[4][0]))
    assert all(o == 0 for _, o in res), (RF.shape_id(shape), 'elements outside the derived bound (g4..g1, dx):', [o for _, o in res], [r for r, _ in res])
    pack.check()


def test_zz_worst_ratios_of_the_random_cases(dev):
    """The figures profiles/rdb_forms_tests_times.txt quotes (whatever ran in this process)."""
    for tag in sorted(WORST):
        print('RDBFORM worst |err| / bound over the shapes, %s: %.3f' % (tag, WORST[tag]))
    assert all(v <= 1.0 for v in WORST.values()), WORST
