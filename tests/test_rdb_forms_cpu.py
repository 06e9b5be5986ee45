"""What test_rdb_forms_gpu.py rests on, without a GPU (cases and restatement: rdb_forms.py): the integer operands of every shape, both
slopes and the three-block chain keep every fp32 partial sum of the fused dense block exact -- the CONDITION of the equality tests,
asserted here, not measured --; the float64 restatement equals torch's own convolutions and autograd; the random-data bound holds
for an fp32 evaluation and separates right from wrong; and the entry points of rdb.hip refuse what they cannot run (fake pointers:
a refusal comes before any launch)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as TF

import rdb_forms as RF
from step_layers import gamma

SHAPE_IDS = [RF.shape_id(s) for s in RF.SHAPES]


def test_the_table_holds_the_grids_it_is_there_for():
    """workgroups = N x tiles; the XCD renumbering b -> (b & 7) (grid / 8) + (b / 8) is taken when grid % 8 == 0 and is the identity
    only at grid = 8"""
    wg = {s: RF.workgroups(s) for s in RF.SHAPES}
    assert wg[(3, 24, 24)] == 27 and wg[(1, 16, 64)] == 16 and wg[(2, 16, 32)] == 16 and wg[(65, 16, 16)] == 260 > RF.CUS
    assert wg[(1, 1, 1)] == 1 and wg[(1, 8, 8)] == 1 and wg[(1, 9, 8)] == 2 and wg[(1, 8, 9)] == 2 and wg[(1, 5, 40)] == 5
    renumbered = [s for s, g in wg.items() if g % 8 == 0 and g > 8]
    assert (1, 16, 64) in renumbered and (2, 16, 32) in renumbered
    for g in (16,):
        perm = [(b & 7) * (g >> 3) + (b >> 3) for b in range(g)]
        assert sorted(perm) == list(range(g)) and perm != list(range(g))
    assert sum(1 for g in wg.values() if g % 8) >= 6 and any(g % 8 and g > RF.CUS for g in wg.values())
    assert RF.workgroups(RF.CHAIN_SHAPE) == 8
    # a tile with its whole halo inside the image; images no larger than a tile; one narrower than the halo
    assert 24 - 16 >= RF.HALO and RF.TILE >= RF.HALO and min(s[1] for s in RF.SHAPES if s[1] > 1) == RF.HALO
    assert len(RF.SHAPES) == 10 and set(RF.VARIANTS.values()) == {2.0, 0.0}
    assert RF.SCALE == RF.POST_SCALE == RF.SKIP_SCALE == 0.5
    # the forms of functional._DenseBlock and the slack forms, as the issue lists them
    f, b = RF.FWD_FORMS, RF.BWD_FORMS
    assert (f['a']['extra_ld'], f['a']['out_ld']) == (None, 192) and (f['b']['extra_ld'], f['b']['out_ld']) == (192, 192)
    assert (f['c']['extra_ld'], f['c']['out_ld']) == (192, 64) and (f['d']['ld'], f['d']['out_ld'], f['d']['extra_ld']) == (200, 68, 72)
    assert all(b[k][s] == 64 for k in ('product', 'product+extra') for s in ('dy_ld', 'skip_ld', 'dx_ld')) and b['product+extra']['extra_ld'] == 64
    assert [b['slack'][s] for s in ('dy_ld', 'skip_ld', 'dx_ld', 'extra_ld', 'ld', 'gld')] == [72, 68, 76, 80, 200, 196]


# ------------------------------------------------------------------------------------------------ the condition of exactness
@pytest.mark.parametrize('variant', list(RF.VARIANTS))
@pytest.mark.parametrize('shape', list(RF.SHAPES), ids=SHAPE_IDS)
def test_integer_operands_keep_every_partial_sum_exact(shape, variant):
    """(sum of magnitudes) x 4 < 2^24 at every element of every stage, forward and backward, and every value a whole number of
    quarters: rdb_forms.exact_forward / exact_backward assert it (assert_exact) as they compute the reference.  The operands are
    what the issue of these tests prescribes, and the case is not degenerate."""
    ops = RF.int_operands(shape)
    assert all(set(t.unique().tolist()) <= {-1.0, 0.0, 1.0} for t in [ops['x'], ops['dy'], ops['extra']] + ops['ws'])
    assert all(len(w.unique()) == 3 and abs((w != 0).float().mean().item() - RF.DENSITY) < 0.01 for w in ops['ws'])
    assert all(set(b.unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0} for b in ops['bs'])
    fw, bw = RF.exact_forward(shape, variant), RF.exact_backward(shape, variant)
    assert max(fw['worst']) * RF.QUARTERS < RF.EXACT and max(bw['worst'].values()) * RF.QUARTERS < RF.EXACT
    print('RDBFORM %s %s largest sum of magnitudes: forward conv1..5 %s  backward g4..g1, dx %s'
          % (RF.shape_id(shape), variant, [int(v) for v in fw['worst']], [bw['worst'][j] for j in (4, 3, 2, 1, 0)]))
    # stored as fp32 the stage outputs are the float64 values themselves
    for t in fw['c'] + [fw['y0'], fw['out'], bw['dx'], bw['dx0']] + list(bw['g'].values()):
        assert torch.equal(t.float().double(), t)
    if shape[1] * shape[2] >= 64:
        assert (ops['acts'] == 0).float().mean().item() > 0.1                # the c > 0 edge
        c4 = fw['c'][3].float()
        odd = (c4.to(torch.bfloat16).float() != c4).float().mean().item()    # c_4 that the next conv does not read as stored
        assert odd > (0.5 if variant == 'lrelu' else 0.1), odd
        g1 = bw['g'][1].float()
        assert (g1.to(torch.bfloat16).float() != g1).float().mean().item() > 0.05
        if variant == 'relu':
            assert (fw['c'][0] == 0).float().mean().item() > 0.3


@pytest.mark.parametrize('variant', list(RF.VARIANTS))
def test_three_block_chain_stays_exact(variant):
    """The chain of functional._DenseBlock on integers, in sixteenths: the condition for every stage of every block, both ways."""
    ch = RF.exact_chain(variant)
    assert ch['worst'] * RF.SIXTEENTHS * 8 < RF.EXACT, ch['worst']
    print('RDBFORM chain %s density 1/%d largest sum of magnitudes %.1f' % (variant, round(1 / RF.CHAIN_DENSITY[variant]), ch['worst']))
    ws = [b[0] for b in ch['ops']['blocks']]
    assert not any(torch.equal(ws[0][k], ws[1][k]) or torch.equal(ws[1][k], ws[2][k]) for k in range(5))
    assert all((w != 0).sum() >= 64 for blk in ws for w in blk)
    # not degenerate: the last block's output depends on every block (non-zero nearly everywhere, away from its addends)
    assert (ch['out'] != 0).float().mean().item() > 0.9 and ch['out'].abs().max().item() > 8
    assert all(r['dx'].abs().max().item() > 1 for r in ch['bwd'])


# --------------------------------------------------------------------------------- the restatement against torch's own arithmetic
def _plain_block(x, ws, bs, scale, slope):
    """The dense block as torchsr writes it, float64, no rounding anywhere; the pre-activations are kept for their gradients"""
    feats, pres = [x], []
    for k in range(4):
        z = TF.conv2d(torch.cat(feats, 1), ws[k], bs[k], 1, 1)
        z.retain_grad()
        pres.append(z)
        feats.append(torch.where(z > 0, z, z * slope))
    return TF.conv2d(torch.cat(feats, 1), ws[4], bs[4], 1, 1) * scale + x, feats[1:], pres


@pytest.mark.parametrize('slope', [2.0, 0.0])
def test_restatement_equals_conv2d_and_autograd_where_bf16_is_exact(slope):
    """On integers small enough to be bf16 numbers throughout (sparse weights) the roundings of the restatement are the identity, so
    forward64 must equal the plain float64 block and backward64 the gradients autograd takes of it: g_j is the gradient of the
    pre-activation of c_j, dx the input gradient (the `+ x` of the block is skip = dy with skip_scale = 1)."""
    shape = (2, 11, 13)
    n, h, w = shape
    ws, bs = RF.int_weights('restatement', 1.0 / 160 if slope else 1.0 / 40)   # (slope 2 doubles stage by stage)
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-1, 2, (n, 64, h, w), generator=g).float()
    dy = torch.randint(-1, 2, (n, 64, h, w), generator=g).float()
    extra = torch.randint(-1, 2, (n, 64, h, w), generator=g).float()
    r = RF.forward64(x, ws, bs, 0.5, slope)
    xd = x.double().requires_grad_(True)
    y, cs, pres = _plain_block(xd, [t.double() for t in ws], [t.double() for t in bs], 0.5, slope)
    for k in range(4):
        c32 = r['c'][k].float()
        assert torch.equal(c32.to(torch.bfloat16).float(), c32), 'c%d is not a bf16 tensor: choose sparser weights' % (k + 1)
        assert torch.equal(r['c'][k], cs[k].detach()) and torch.equal(r['pre'][k], pres[k].detach())
    assert torch.equal(r['y0'], y.detach()) and r['c'][3].abs().max() > 8
    assert torch.equal(RF.fwd_out(r['y0'], 0.5, extra), y.detach() * 0.5 + extra.double())
    (y * dy.double()).sum().backward()
    acts = torch.cat([x] + [c.float() for c in r['c']], 1)
    b = RF.backward64(dy, acts, ws, 0.5, slope, dy, 1.0, extra)
    for j in (4, 3, 2, 1):
        g32 = b['g'][j].float()
        assert torch.equal(g32.to(torch.bfloat16).float(), g32), 'g%d is not a bf16 tensor' % j
        assert torch.equal(b['g'][j], pres[j - 1].grad), j
    assert torch.equal(b['dx'], xd.grad + extra.double()) and b['dx'].abs().max() > 4


def test_restatement_rounds_sources_to_bf16_and_keeps_outputs_fp32():
    """... and where bf16 is NOT exact: each stage equals conv2d of the bf16-rounded fp32 tensors before it, nothing else."""
    shape = (1, 13, 21)
    ops = RF.int_operands(shape)
    fw = RF.exact_forward(shape, 'lrelu')
    feats = [ops['x']] + [c.float() for c in fw['c']]
    rb = lambda t: t.to(torch.bfloat16).double()  # noqa: E731
    for k in range(4):
        z = TF.conv2d(rb(torch.cat(feats[:k + 1], 1)), rb(ops['ws'][k]), ops['bs'][k].double(), 1, 1)
        assert torch.equal(fw['c'][k], torch.where(z > 0, z, z * 2.0))
    assert not torch.equal(rb(feats[4]), feats[4].double())
    bw = RF.exact_backward(shape, 'lrelu')
    gs = {5: ops['dy'] * RF.SCALE}
    gs.update({j: bw['g'][j].float() for j in (4, 3, 2, 1)})
    for j in (4, 3, 2, 1, 0):
        lo, hi = (64 + 32 * (j - 1), 64 + 32 * j) if j else (0, 64)
        a = sum(torch.nn.grad.conv2d_input((1, RF.conv_cin(k), 13, 21), rb(ops['ws'][k - 1]), rb(gs[k]), padding=1)[:, lo:hi]
                for k in range(max(j, 0) + 1, 6))
        if j:
            assert torch.equal(bw['g'][j], torch.where(ops['acts'][:, lo:hi] > 0, a, a * 2.0)), j
        else:
            assert torch.equal(bw['dx'], a + RF.SKIP_SCALE * ops['skip'].double() + ops['extra'].double())


# ------------------------------------------------------------------------------------------------- the derived bound, on the CPU
def test_rounding_counts_are_those_of_the_issue():
    assert [RF.fwd_k(k) for k in (1, 2, 3, 4)] == [9 * 64 + 2, 9 * 96 + 2, 9 * 128 + 2, 9 * 160 + 2]
    assert RF.out_k(False) == 9 * 192 + 3 and RF.out_k(True) == 9 * 192 + 5
    assert [RF.bwd_k(j) for j in (4, 3, 2, 1)] == [9 * 64 + 1, 9 * 96 + 1, 9 * 128 + 1, 9 * 160 + 1]
    assert RF.dx_k(False) == 9 * 192 + 2 and RF.dx_k(True) == 9 * 192 + 3


def test_derived_bound_holds_for_fp32_and_separates_right_from_wrong():
    """gamma_k (|a| conv |w| + |b|) on the bf16-rounded operands before it judges the kernel: torch's fp32 convolution of the rounded
    operands (some fp32 summation order) lies inside it for every stage, forward and backward; a stage with one tap or one source
    slice dropped lies outside it almost everywhere."""
    shape = (2, 9, 12)
    ops = RF.random_operands(shape)
    p = RF.RANDOM_FWD
    rb = lambda t: t.to(torch.bfloat16).float()  # noqa: E731
    feats = [ops['x']]
    for k in range(1, 5):
        c64, z64, mag = RF.fwd_stage(k, feats, ops['ws'][k - 1], ops['bs'][k - 1], p['slope'])
        for drop in (None, 'tap', 'slice'):
            wk = rb(ops['ws'][k - 1]).clone()
            if drop == 'tap':
                wk[:, :, 1, 1] = 0
            if drop == 'slice':
                wk[:, -32:] = 0
            z = TF.conv2d(rb(torch.cat(feats, 1)), wk, ops['bs'][k - 1], 1, 1)
            c = torch.where(z > 0, z, z * p['slope'])
            bound = gamma(RF.fwd_k(k)) * mag
            out = ((c.double() - c64).abs() > bound).double().mean().item()
            assert out == 0.0 if drop is None else out > 0.9, (k, drop, out)
        feats.append(c64.float())
    b = RF.RANDOM_BWD
    r = RF.backward64(ops['dy'], ops['acts'], ops['ws'], b['scale'], b['slope'], ops['skip'], b['skip_scale'], ops['extra'])
    g5 = rb(ops['dy'] * b['scale'])
    for drop, want in ((False, 0.0), (True, 0.9)):
        w5 = rb(ops['ws'][4]).clone()
        if drop:
            w5[:, :, 1, 1] = 0
        a = torch.nn.grad.conv2d_input((2, 192, 9, 12), w5, g5, padding=1)[:, 160:192]
        g4 = torch.where(ops['acts'][:, 160:192] > 0, a, a * b['slope'])
        bound = gamma(RF.bwd_k(4)) * r['mag'][4] * torch.where(ops['acts'][:, 160:192] > 0, 1.0, b['slope'])
        out = ((g4.double() - r['g'][4]).abs() > bound).double().mean().item()
        assert out == 0.0 if not drop else out > want, (drop, out)


# ---------------------------------------------------------------------------------------------- refusals, with fake pointers
@pytest.fixture(scope='module')
def lib():
    from torchsr_amd import _lib
    return _lib.lib()


def _err():
    from torchsr_amd import _lib
    return _lib.last_error()


FAKE, FAKE2, FAKE3, FAKE4 = 0x10000, 0x20000, 0x30000, 0x40000   # never dereferenced: every call below is refused before a launch


def _refused(rc, words):
    msg = _err()
    assert rc != 0 and msg and words in msg, (rc, msg, words)


def _ids(v):
    if isinstance(v, dict):
        return '-'.join('%s=%s' % (k, x if isinstance(x, (int, type(None))) else 'with-null') for k, x in v.items())
    return v.replace(' ', '_')


def _fwd_args(**kw):
    a = dict(n=1, h=8, w=8, buf=FAKE, ld=192, wpk=FAKE2, biases=(C.c_void_p * 5)(*[FAKE3] * 5), scale=0.2, slope=0.2, post=1.0, extra=None,
             extra_ld=0, out=FAKE4, out_ld=192)
    a.update(kw)
    return (a['n'], a['h'], a['w'], a['buf'], a['ld'], a['wpk'], a['biases'], a['scale'], a['slope'], a['post'], a['extra'], a['extra_ld'],
            a['out'], a['out_ld'], None)


@pytest.mark.parametrize('kw,words', [
    (dict(out=FAKE), 'alias'),
    (dict(ld=188), '>= 192'),
    (dict(ld=194), 'whole quads'),
    (dict(out_ld=60), 'the output >= 64'),
    (dict(out_ld=66), 'whole quads'),
    (dict(extra=FAKE4, extra_ld=192), 'of its own'),
    (dict(extra=FAKE3, extra_ld=60), 'second addend needs >= 64'),
    (dict(extra=FAKE3, extra_ld=66), 'second addend needs >= 64'),
    (dict(biases=(C.c_void_p * 5)(FAKE3, FAKE3, None, FAKE3, FAKE3)), 'null bias 2'),
    (dict(biases=(C.c_void_p * 5)(FAKE3, FAKE3, FAKE3, FAKE3, None)), 'null bias 4'),
    (dict(n=1, h=4096, w=4096), '2^24'),
    (dict(n=65536, h=16, w=16), '2^24'),
    (dict(buf=None), 'null pointer'), (dict(wpk=None), 'null pointer'), (dict(biases=None), 'null pointer'), (dict(out=None), 'null pointer'),
    (dict(n=0), 'rdb_fwd'), (dict(h=0), 'rdb_fwd'), (dict(w=-1), 'rdb_fwd'),
], ids=_ids)
def test_rdb_fwd_refuses(lib, kw, words):
    _refused(lib.srx_rdb_fwd(*_fwd_args(**kw)), words)


def _bwd_args(**kw):
    a = dict(n=1, h=8, w=8, dy=FAKE, dy_ld=64, scale=0.2, buf=FAKE2, ld=192, wpk=FAKE3, slope=0.2, gbuf=FAKE4, gld=192, skip=0x50000, skip_ld=64,
             skip_scale=1.0, extra=None, extra_ld=0, dx=0x60000, dx_ld=64)
    a.update(kw)
    return (a['n'], a['h'], a['w'], a['dy'], a['dy_ld'], a['scale'], a['buf'], a['ld'], a['wpk'], a['slope'], a['gbuf'], a['gld'], a['skip'],
            a['skip_ld'], a['skip_scale'], a['extra'], a['extra_ld'], a['dx'], a['dx_ld'], None)


@pytest.mark.parametrize('kw,words', [
    (dict(dx=FAKE), 'alias'),
    (dict(dx=0x50000), 'alias'),
    (dict(gbuf=FAKE2), 'alias'),
    (dict(extra=0x60000, extra_ld=64), 'of its own'),
    (dict(extra=0x70000, extra_ld=60), 'second addend needs >= 64'),
    (dict(gld=188), '>= 192'), (dict(gld=194), 'whole quads'), (dict(ld=188), '>= 192'),
    (dict(dy_ld=60), '>= 64'), (dict(skip_ld=62), '>= 64'), (dict(dx_ld=63), '>= 64'),
    (dict(dy=None), 'null pointer'), (dict(buf=None), 'null pointer'), (dict(wpk=None), 'null pointer'), (dict(gbuf=None), 'null pointer'),
    (dict(skip=None), 'null pointer'), (dict(dx=None), 'null pointer'),
    (dict(n=1, h=4096, w=4096), '2^24'),
], ids=_ids)
def test_rdb_bwd_refuses(lib, kw, words):
    _refused(lib.srx_rdb_bwd(*_bwd_args(**kw)), words)


@pytest.mark.parametrize('entry', ['srx_rdb_pack', 'srx_rdb_pack_bwd'])
def test_rdb_pack_refuses(lib, entry):
    fn = getattr(lib, entry)
    for args in ((FAKE, 0, FAKE2, None), (FAKE, 4097, FAKE2, None), (FAKE, -1, FAKE2, None), (None, 1, FAKE2, None), (FAKE, 1, None, None)):
        _refused(fn(*args), 'rdb_pack: bad argument')
    assert lib.srx_rdb_packed_bytes() == 479232 and lib.srx_rdb_packed_bytes() % 1024 == 0
