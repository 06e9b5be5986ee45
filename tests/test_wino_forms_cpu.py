"""Every case of wino_forms.py reaches the launch form it is there for -- asked of srx_wino_plan and srx_wino_ws_floats alone, which
plan with the function the launches of wino.hip plan with (host code: no GPU).  A planner change that makes a case vacuous fails here,
loudly, instead of leaving test_wino_forms_gpu.py to pass on another plan.  Also without a GPU: the integer operands of the exact check
keep every fp32 partial sum of the Winograd arithmetic exact (restated in int64), and the derived elementwise bound of the random
check (step_layers.wino_abs / wino_k) holds for an fp32 emulation of that arithmetic and separates right from wrong."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import wino_forms as WF
from step_layers import WINO_AT, WINO_BT, WINO_G, gamma, wino_abs, wino_k

EXACT = 1 << 24   # below it every integer is an fp32 number


def cdiv(a, b):
    return -(-a // b)


@pytest.fixture
def lib():
    """The library with nothing forced; whatever a test forces is gone afterwards."""
    from torchsr_amd import _lib
    L = _lib.lib()
    assert L.srx_wino_force_plan(0, 0, 0) == 0
    try:
        yield L
    finally:
        assert L.srx_wino_force_plan(0, 0, 0) == 0


def desc(geo, entry, relu=False, slope=0.0):
    from torchsr_amd import _lib
    return _lib.Conv2dDesc(*WF.desc_fields(geo, entry, relu, slope))


def plan(L, d, which):
    """srx_wino_plan's answer in the table's order: (bn, zsplit, tsplit, workgroups, tile blocks, chunks per workgroup)"""
    from torchsr_amd import _lib
    out = (C.c_int * 6)(*([-1] * 6))
    assert L.srx_wino_plan(C.byref(d), which, out) == 0, _lib.last_error()
    return (out[0], out[1], out[5], out[2], out[3], out[4])


def asked(L, case, force):
    d = desc(case['geo'], case['entry'], case['relu'], case['slope'])
    wh = WF.which(case['entry'], case['slope'], case['addend'])
    assert L.srx_wino_force_plan(*(force or (0, 0, 0))) == 0
    try:
        return plan(L, d, wh), L.srx_wino_ws_floats(C.byref(d), wh)
    finally:
        assert L.srx_wino_force_plan(0, 0, 0) == 0


def skip_tail_elsewhere(L, case):
    if case['tail'] and L.srx_plan_cus() != WF.CUS:
        pytest.skip(WF.TAIL_SKIP % L.srx_plan_cus())


@pytest.mark.parametrize('case', WF.CASES, ids=WF.by_id(WF.CASES))
def test_case_plans_the_form_it_is_listed_under(lib, case):
    """... and the workspace query is the formula of that form: zsplit outputs for a split, tail x tsplit tile-local blocks for a cut
    last round, nothing otherwise -- for the statistics and inference launches the no-split size, not the plain forward's."""
    skip_tail_elsewhere(lib, case)
    got, ws = asked(lib, case, case['force'])
    if case['force'] is None and lib.srx_plan_cus() != WF.CUS:   # the cost model's own choice on another part: any plan it can run
        assert got[0] in (32, 64) and got[2] == 1
    else:
        assert got == tuple(case['expect']), (case['id'], got, case['expect'])
    bn, zs, ts, wgs, tblocks, chunks = got
    n, h, w, _, _ = case['geo']
    k, cols = WF.gemm_dims(case)
    items = cdiv(n * (h // 2) * (w // 2), WF.WT) * (cols // bn) * zs
    tail = items % WF.CUS if ts > 1 else 0
    assert tblocks == cdiv(n * (h // 2) * (w // 2), WF.WT) and wgs == items + tail * (ts - 1) and chunks == cdiv(k // WF.WKC, zs)
    assert not (zs > 1 and ts > 1) and (ts == 1 or (items > WF.CUS and tail > 0))
    want = zs * n * h * w * cols if zs > 1 else tail * ts * WF.WT * 4 * bn
    assert ws == want, (case['id'], ws, want)
    wh = WF.which(case['entry'], case['slope'], case['addend'])
    if wh in (WF.WHICH_STATS, WF.WHICH_ACT):
        assert zs == 1 and (ts == 1 or wh == WF.WHICH_STATS)
    # the kernels the table lists are those of the plan
    names = [WF.MAIN[bn]] + ([WF.FIXUP] if zs > 1 else []) + ([WF.TAIL_FIXUP[bn]] if ts > 1 else [])
    assert case['kernels'] == names or lib.srx_plan_cus() != WF.CUS


def test_inference_and_statistics_launches_do_not_ask_for_a_split_workspace(lib):
    """A layer whose plain forward the model splits (Z5: 4 splits, 46080 floats): the same layer as a statistics (which = 2) or
    LeakyReLU / addend launch (which = 3) plans whole tiles and needs no workspace -- the query equals what the launch needs."""
    geo = WF.case('Z5')['geo']
    d = desc(geo, 'fwd')
    out = {wh: (plan(lib, d, wh), lib.srx_wino_ws_floats(C.byref(d), wh)) for wh in range(4)}
    if lib.srx_plan_cus() == WF.CUS:
        assert out[0] == ((32, 4, 1, 16, 2, 1), 4 * 3 * 6 * 10 * 64), out[0]
    for wh in (WF.WHICH_STATS, WF.WHICH_ACT):
        assert out[wh][0][1] == 1 and out[wh][0][2] == 1 and out[wh][1] == 0, (wh, out[wh])
    # a PixelShuffle layer plans as which = 3 only
    sh = desc(WF.case('S2')['geo'], 'shuffle')
    ints = (C.c_int * 6)()
    assert plan(lib, sh, WF.WHICH_ACT)[:3] in ((32, 1, 1), (64, 1, 1))
    for wh in (0, 1, 2, 4, -1):
        assert lib.srx_wino_plan(C.byref(sh), wh, ints) != 0
    assert lib.srx_wino_plan(C.byref(d), 4, ints) != 0 and lib.srx_wino_plan(C.byref(d), -1, ints) != 0
    assert lib.srx_wino_ws_floats(C.byref(d), 4) == 0


@pytest.mark.parametrize('geo,entry,force,why', WF.FALLBACKS, ids=[f'{e}.{"x".join(map(str, g))}.{"-".join(map(str, f))}' for g, e, f, _ in WF.FALLBACKS])
def test_forced_plan_the_launch_cannot_take_reports_the_planners_own(lib, geo, entry, force, why):
    """No silent other form: what srx_wino_plan reports under a forced plan the launch cannot run is the plan with nothing forced --
    and it is not the forced one, so a case table that asserts its plan would notice."""
    case = dict(geo=geo, entry=entry, relu=False, slope=WF.SLOPE if entry in ('act', 'shuffle') else 0.0, addend=False)
    own = asked(lib, case, None)
    got = asked(lib, case, force)
    assert got == own, (why, got, own)
    if lib.srx_plan_cus() == WF.CUS:
        assert got[0][:3] != tuple(force), (why, got)
    if entry == 'dgrad' and force == (32, 1, 4) and lib.srx_plan_cus() == WF.CUS:
        assert got[0] == (64, 3, 1, 198, 33, 3)


def test_bad_forced_plans_are_refused(lib):
    from torchsr_amd import _lib
    d = desc(WF.case('Z5')['geo'], 'fwd')
    before = plan(lib, d, 0)
    for bad in WF.BAD_FORCE:
        with pytest.raises(RuntimeError, match='wino_force_plan'):
            _lib.call('srx_wino_force_plan', *bad)
        assert plan(lib, d, 0) == before, bad        # (a refused setter changed nothing)


def test_the_table_reaches_every_kernel_and_entry():
    assert sorted({k for c in WF.CASES for k in c['kernels']}) == sorted(WF.ALL_KERNELS) and len(WF.ALL_KERNELS) == 5
    assert {c['entry'] for c in WF.CASES} == {'fwd', 'dgrad', 'stats', 'act', 'shuffle'}
    assert len(set(WF.by_id(WF.CASES))) == len(WF.CASES)
    assert set(WF.RANDOM_IDS) <= set(WF.by_id(WF.CASES))
    # statistics in each tail fix-up and in each main epilogue; a mask in each fix-up kernel
    stats = {k for c in WF.CASES if c['entry'] == 'stats' for k in c['kernels']}
    assert set(WF.ALL_KERNELS) - {WF.FIXUP} <= stats
    masked = {k for c in WF.CASES if c['mask'] for k in c['kernels']}
    assert {WF.FIXUP, WF.TAIL_FIXUP[32]} <= masked
    for c in WF.CASES:   # cases that share operands are one layer
        assert all(o['geo'] == c['geo'] and o['wkeep'] == c['wkeep'] for o in WF.CASES if o['data'] == c['data']), c['id']


# ------------------------------------------------------------------------------------------- integer operands stay exact
def winograd_int64(x, w):
    """The three transforms restated in int64 for integer operands x (N, Cin, H, W) and w (Cout, Cin, 3, 3) of multiples of 4:
    (Y, max over tiles, xi and co of sum_ci |U| |V|).  2 G is an integer matrix and U = (2G) g (2G)^T / 4 must divide.  The channel
    contraction is a float64 matrix product of integers below 2^53: exact, and BLAS."""
    bt, at = np.array(WINO_BT, dtype=np.int64), np.array(WINO_AT, dtype=np.int64)
    g2 = np.array([[2 * v for v in r] for r in WINO_G]).astype(np.int64)
    assert (g2 == 2 * np.array(WINO_G)).all()
    n, cin, h, wd = x.shape
    th, tw = h // 2, wd // 2
    u4 = np.einsum('ip,ocpq,jq->ijco', g2, w.astype(np.int64), g2)
    assert (u4 % 4 == 0).all(), 'G g G^T is not an integer'
    u = (u4 // 4).reshape(16, cin, -1)
    xp = np.pad(x.astype(np.int64), ((0, 0), (0, 0), (1, 1), (1, 1)))
    patches = np.lib.stride_tricks.sliding_window_view(xp, (4, 4), axis=(2, 3))[:, :, ::2, ::2]    # (N, Cin, TH, TW, 4, 4)
    v = np.einsum('ip,ncyxpq,jq->ijnyxc', bt, patches, bt).reshape(16, n * th * tw, cin)
    m = np.matmul(v.astype(np.float64), u.astype(np.float64))
    mabs = np.matmul(np.abs(v).astype(np.float64), np.abs(u).astype(np.float64))
    assert mabs.max() < 2.0 ** 53
    m = m.astype(np.int64).reshape(4, 4, n, th, tw, -1)
    y = np.einsum('ui,vj,ijnyxo->noyuxv', at, at, m).reshape(n, -1, h, wd)
    return y, int(mabs.max())


def effective(case, d):
    """The forward problem the launch computes: (input, weights) -- a data gradient convolves dy with the transposed, flipped filter"""
    if case['entry'] == 'dgrad':
        return d['x'], np.ascontiguousarray(d['w'].transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])
    return d['x'], d['w']


@pytest.mark.parametrize('case', WF.CASES, ids=WF.by_id(WF.CASES))
def test_integer_operands_keep_every_partial_sum_exact(case):
    """sum_ci |U_xi| |V_xi| < 2^24 for every tile, xi and co -- so every fp32 partial sum of the channel contraction is an integer
    below 2^24 in ANY order, splits and parts included --, the nine-term sums of the output transform likewise, and sum |y|,
    sum y^2 < 2^24 over each statistics block of 128 pixels.  The restated Winograd arithmetic equals the direct convolution."""
    d = WF.int_inputs(case)
    assert set(np.unique(d['x'])) <= {-1, 0, 1} and set(np.unique(d['w'])) <= {-4, 0, 4}
    assert len(np.unique(d['w'])) == 3 and len(np.unique(d['bias'])) > 3
    a, w = effective(case, d)
    y, worst = winograd_int64(a, w)
    assert worst < EXACT, (case['id'], worst)
    assert 9 * worst < EXACT, (case['id'], 'output transform', worst)     # |A^T| M |A|: at most nine entries of M per output
    ref = TF.conv2d(torch.from_numpy(a.astype(np.float64)), torch.from_numpy(w.astype(np.float64)), None, 1, 1).numpy()
    assert (y == ref).all(), case['id']
    assert np.abs(y).max() > 8            # (not a degenerate layer)
    if case['entry'] == 'stats':
        n, h, wd, cin, cout = case['geo']
        if case['bias']:
            y = y + d['bias'].astype(np.int64).reshape(1, -1, 1, 1)
        tiles = y.reshape(n, cout, h // 2, 2, wd // 2, 2).transpose(0, 2, 4, 1, 3, 5).reshape(-1, cout, 4)
        rows = cdiv(tiles.shape[0], WF.WT)
        tiles = np.concatenate([tiles, np.zeros((rows * WF.WT - tiles.shape[0], cout, 4), dtype=np.int64)])
        blocks = tiles.reshape(rows, WF.WT, cout, 4)
        s1, s2 = np.abs(blocks).sum((1, 3)).max(), (blocks * blocks).sum((1, 3)).max()
        assert s1 < EXACT and s2 < EXACT, (case['id'], s1, s2)
    # the epilogue: quarters of (|y| + |bias|) and the addend stay far below 2^24 as well
    assert 4 * (np.abs(y).max() + 5 + 3) < EXACT


# ------------------------------------------------------------------------------------------------- the derived bound, on the CPU
def winograd_fp32(x, w, bias, reverse):
    """wino.hip's arithmetic in numpy float32, operation by operation: the pack routine's two passes of G (two additions, then the
    exact halving), B^T d B in two passes of one addition, a sequential fp32 accumulation over the input channels (ascending, or
    descending: another summation order), A^T M A in two passes of two additions, + bias."""
    f = np.float32
    x, w = x.astype(f), w.astype(f)
    n, cin, h, wd = x.shape
    cout = w.shape[0]
    th, tw = h // 2, wd // 2

    def g_pass(t):   # rows 0..2 of the leading axis -> 4
        return np.stack([t[0], f(.5) * ((t[0] + t[1]) + t[2]), f(.5) * ((t[0] - t[1]) + t[2]), t[2]])
    gw = np.moveaxis(w, (2, 3), (0, 1))                               # (3, 3, Cout, Cin)
    u = g_pass(gw)                                                    # (4, 3, ..)
    u = np.moveaxis(g_pass(np.moveaxis(u, 1, 0)), 0, 1)               # (4, 4, Cout, Cin)

    def b_pass(t):
        return np.stack([t[0] - t[2], t[1] + t[2], t[2] - t[1], t[1] - t[3]])
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    p = np.lib.stride_tricks.sliding_window_view(xp, (4, 4), axis=(2, 3))[:, :, ::2, ::2]
    p = np.moveaxis(p, (4, 5), (0, 1))                                # (4, 4, N, Cin, TH, TW)
    v = b_pass(np.moveaxis(b_pass(np.moveaxis(p, 1, 0)), 1, 0))      # within the rows first, as stage_patch does, then across them
    m = np.zeros((4, 4, n, cout, th, tw), dtype=f)
    for ci in (range(cin - 1, -1, -1) if reverse else range(cin)):
        m = m + (u[:, :, None, :, ci, None, None] * v[:, :, :, None, ci]).astype(f)
    assert m.dtype == f

    def a_pass(t):
        return np.stack([(t[0] + t[1]) + t[2], (t[1] - t[2]) - t[3]])
    y = a_pass(np.moveaxis(a_pass(m), 1, 0))                          # (2 v, 2 u, N, Cout, TH, TW)
    y = np.transpose(y, (2, 3, 4, 1, 5, 0)).reshape(n, cout, h, wd)
    if bias is not None:
        y = y + bias.astype(f).reshape(1, -1, 1, 1)
    assert y.dtype == f
    return y


def test_derived_bound_holds_for_an_fp32_emulation_and_separates_right_from_wrong():
    """step_layers.wino_abs / wino_k before they judge a kernel: the fp32 emulation of the Winograd arithmetic, in two summation
    orders, lies inside gamma_k (|A^T| [sum (|G||g||G^T|) (.) (|B^T||d||B|)] |A| + |bias|) around float64; the two orders differ (the
    check is not of one lucky order); a result with one tap or one input channel dropped lies outside it.  The magnitude term is
    what the transforms cost and no more: elementwise at least the direct form's |x| conv |w| (the triangle inequality through the
    Winograd identity), on average below 9 x it -- while k is Cin + 12 against the direct form's 9 Cin + 1."""
    n, h, wd, cin, cout = 2, 6, 10, 64, 32
    g = torch.Generator().manual_seed(3)
    x = torch.randn((n, cin, h, wd), generator=g)
    w = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn((cout,), generator=g) * 0.1
    y64 = TF.conv2d(x.double(), w.double(), b.double(), 1, 1)
    bound = gamma(wino_k(cin, 1, True)) * (wino_abs(x, w) + b.double().abs().view(1, -1, 1, 1))
    assert bound.shape == y64.shape and bound.dtype == torch.float64 and bool((bound > 0).all())
    ys = [torch.from_numpy(winograd_fp32(x.numpy(), w.numpy(), b.numpy(), rev)) for rev in (False, True)]
    assert not torch.equal(ys[0], ys[1])
    for y in ys:
        err = (y.double() - y64).abs()
        assert bool((err <= bound).all()), (err / bound).max().item()
        assert ((y.double() - y64).norm() / y64.norm()).item() < 1e-6
    over = wino_abs(x, w) / TF.conv2d(x.double().abs(), w.double().abs(), None, 1, 1)
    assert over.min().item() >= 1.0 - 1e-12 and over.mean().item() < 9.0, (over.min().item(), over.mean().item())
    assert wino_k(cin, 1, True) == cin + 12 and wino_k(cin, 8, False, extra=2) == cin + 20
    w_cut = w.clone()
    w_cut[:, :, 1, 2] = 0.0
    x_cut = x.clone()
    x_cut[:, cin // 2] = 0.0
    for bad in (winograd_fp32(x.numpy(), w_cut.numpy(), b.numpy(), False), winograd_fp32(x_cut.numpy(), w.numpy(), b.numpy(), False)):
        off = (torch.from_numpy(bad).double() - y64).abs() > bound
        assert off.double().mean().item() > 0.5
    # the data gradient is the forward problem of dy and the transposed, flipped filter
    dy = torch.randn((n, cout, h, wd), generator=g)
    w_t = w.transpose(0, 1).flip(2, 3).contiguous()
    dx64 = torch.nn.grad.conv2d_input((n, cin, h, wd), w.double(), dy.double(), 1, 1)
    assert torch.allclose(dx64, TF.conv2d(dy.double(), w_t.double(), None, 1, 1), rtol=1e-12, atol=1e-12)
    dx = torch.from_numpy(winograd_fp32(dy.numpy(), w_t.numpy(), None, False))
    assert bool(((dx.double() - dx64).abs() <= gamma(wino_k(cout)) * wino_abs(dy, w_t)).all())
    # conv_refs hands the same bound to test_step_layers_gpu.check, at the most splits a plan can have
    from step_layers import WINO_MAX_PARTS, conv_refs
    by = conv_refs('y', x, w, x.shape, w.shape, 1, 1, 0, b, wino=True)
    bdx = conv_refs('dx', dy, w, x.shape, w.shape, 1, 1, 0, None, wino=True)
    assert len(by) == 4 and torch.equal(by[0], y64) and torch.allclose(by[3], bound * (gamma(wino_k(cin, WINO_MAX_PARTS, True)) / gamma(wino_k(cin, 1, True))), rtol=1e-12, atol=0)
    assert len(bdx) == 4 and torch.equal(bdx[0], dx64) and torch.allclose(bdx[3], gamma(wino_k(cout, WINO_MAX_PARTS)) * wino_abs(dy, w_t), rtol=1e-12, atol=0)
    # wino_abs in passes of a few images is one pass (to the rounding of the float64 matrix products, whose blocking may differ)
    assert torch.allclose(wino_abs(x, w, tiles_per_pass=1), wino_abs(x, w), rtol=1e-12, atol=0)
