"""Every launch form of the weight gradient (wgrad.hip; cases: wgrad_forms.py), through the C ABI so that no layer class can route a
call elsewhere, each against fp64 on the CPU:

* the seven slab kernels -- wgrad_kernel<0> (register-staged fp32, srx_wgrad_force_kernels(0, ., .)), wgrad_dma_kernel<0, 0> / <1, 0> /
  <1, 1>, wgrad_kernel<1>, wgrad_rows_bf16_kernel<32> / <16> -- under forced row splits (srx_wgrad_force) that start mid-row, cut
  images, leave a short last split, on strided, shuffled, upsampled inputs and maps smaller than a chunk;
* both reduce kernels on every case (srx_wgrad_force_kernels(., ., 0): wgrad_reduce_kernel), bit for bit against each other where
  both can run -- "same sums in the same order" is the source's claim -- with 64, 65 and 72 slabs per output, the PixelShuffle
  channel order, paired outputs, per-output scales and accumulation.

The kernels a case launches are asserted from the library's records (srx_prof_start_aux) against what srx_wgrad_plan reported.
Bound, elementwise, the convention of test_esrgan_layers_gpu.run_dense_wgrad_case: with M_tot the pixels summed into one output over
its per_out segments and e one more rounding for a scale other than 1 and one for accumulation,

    |dW - dW64| <= gamma(M_tot + e) (|scale| (|x| conv |dy|) + |old|),      |db - db64| <= gamma(M_tot + e) (|scale| sum |dy| + |old|)

u = 2^-24; bf16 products: the reference convolves the bf16-ROUNDED operands (a bf16 x bf16 product is exact in fp32), the bias
gradient sums the unrounded fp32 dy.  A worst-case bound of any summation order: nothing here is a measured tolerance.  Workspaces
have exactly the queried size, start as NaN and lie between sentinel bands; every output lies between sentinel bands and starts
as NaN unless it accumulates.  Each case prints the worst error / bound it met (profiles/wgrad_form_tests_times.txt)."""
import ctypes as C
import functools
import zlib

import pytest
import torch
import torch.nn.functional as TF

import wgrad_forms as WF
from step_layers import conv_refs, gamma, prof_launches

pytestmark = pytest.mark.gpu

NAN = float('nan')
GUARD = 256          # floats before and behind the workspace and every output
SENTINEL = 12345.0
U = 2.0 ** -24
_SEEN = set()        # kernel names this module's launches recorded
_RAN = set()         # case ids that ran
_RESULTS = {}        # (row, variant) -> the outputs on the CPU, for the printed fp32 comparison


def _L():
    from torchsr_amd import _lib
    return _lib, _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _reset():
    lib, L = _L()
    assert L.srx_wgrad_force(-1, 0) == 0
    assert L.srx_wgrad_force_kernels(-1, -1, -1) == 0


@pytest.fixture(autouse=True)
def _overrides_reset(dev):
    """No other test sees a forced split or kernel of this module."""
    try:
        yield
    finally:
        _reset()


def guarded(n, dev, fill):
    """(allocation, view of n floats holding `fill`) between two bands of SENTINEL"""
    flat = torch.full((n + 2 * GUARD,), SENTINEL, device=dev)
    flat[GUARD:GUARD + n] = fill
    return flat, flat[GUARD:GUARD + n]


def guards_intact(flat):
    return bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[-GUARD:] == SENTINEL).all())


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ operands and fp64 references
@functools.lru_cache(maxsize=None)
def _operands(row):
    """The tensors of a table row, shared by its variants: per problem the input buffer (N, Cin_s, H, W: every stored channel random,
    the layer reads the first Cin) and the output gradient in the conv's own layout (N, Cout, Ho, Wo); per output the old values."""
    case = next(c for c in WF.CASES if c['row'] == row)
    g = case['geo']
    gen = torch.Generator().manual_seed(zlib.crc32(row.encode()))
    ho, wo = WF.out_size(g)
    bufs = [torch.rand((g['n'], g['cin_s'], g['h'], g['w']), generator=gen) * 2 - 1 for _ in range(case['nprob'])]
    dys = [torch.rand((g['n'], g['cout'], ho, wo), generator=gen) * 2 - 1 for _ in range(case['nprob'])]
    nout = case['nprob'] // case['per_out']
    olds = []
    for _ in range(nout):
        if case['call'] == 'pair':
            half = g['cout'] // 2
            shapes = [(half, case['cin_lo'], g['k'], g['k']), (half, g['cin'], g['k'], g['k'])]
            olds.append([(torch.randn(s, generator=gen) * 0.5, torch.randn(s[0], generator=gen) * 0.5) for s in shapes])
        else:
            s = (g['cout'], g['cin'], g['k'], g['k'])
            olds.append([(torch.randn(s, generator=gen) * 0.5, torch.randn(s[0], generator=gen) * 0.5)])
    return bufs, dys, olds


@functools.lru_cache(maxsize=None)
def _reference(row, rounded):
    """Per output and conv of it (one; two for a pair): (dW64, |x| conv |dy|, db64, sum |dy|) summed over the output's segments,
    before scale and accumulation.  Computed once per row and product precision."""
    case = next(c for c in WF.CASES if c['row'] == row)
    g = case['geo']
    bufs, dys, olds = _operands(row)
    m = dys[0][:, 0].numel()
    out = []
    for o in range(len(olds)):
        convs = []
        if case['call'] == 'pair':
            half = g['cout'] // 2
            parts = [(case['cin_lo'], slice(0, half)), (g['cin'], slice(half, g['cout']))]
        else:
            parts = [(g['cin'], slice(0, g['cout']))]
        for cin, cols in parts:
            acc = None
            for i in range(o * case['per_out'], (o + 1) * case['per_out']):
                x, dy = bufs[i][:, :cin].contiguous(), dys[i][:, cols].contiguous()
                w_shape = (dy.shape[1], cin, g['k'], g['k'])
                dw64, _, bound = conv_refs('dW', x, dy, x.shape, w_shape, g['stride'], g['pad'], g['up'], None, rounded, U)
                terms = [dw64, bound / gamma(m, U), dy.double().sum((0, 2, 3)), dy.double().abs().sum((0, 2, 3))]
                acc = terms if acc is None else [a + t for a, t in zip(acc, terms)]
            convs.append(tuple(acc))
        out.append(convs)
    return out, m


def _nhwc(t, cs, off=0):
    """cpu NCHW -> cpu NHWC of cs stored channels, the tensor's channels at [off, off + C), the others random"""
    n, c, h, w = t.shape
    y = torch.rand((n, h, w, cs), generator=torch.Generator().manual_seed(c + h)) - 0.5
    y[..., off:off + c] = t.permute(0, 2, 3, 1)
    return y.contiguous()


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t if isinstance(t, int) else t.data_ptr() for t in ts])


# ----------------------------------------------------------------------------------------------------------------- one launch
def _launch(dev, case, reduce):
    """The case's call with its overrides and the reduce kernel `reduce` (-1: the default) forced: plan, workspace and launch records
    checked; returns the outputs as [(dW, db) per conv per output] on the CPU and the names of the two kernels."""
    lib, L = _L()
    g = case['geo']
    d = lib.Conv2dDesc(*WF.desc_fields(case))
    nsplit, dma, rows, _ = case['force']
    lib.call('srx_wgrad_force', -1, nsplit)
    lib.call('srx_wgrad_force_kernels', dma, rows, reduce)
    nprob, per_out = case['nprob'], case['per_out']
    plan = (C.c_int * 6)()
    lib.call('srx_wgrad_plan', C.byref(d), nprob, per_out, plan)
    plan = list(plan)
    kernel, ens, erps, ered, eslabs = case['expect']
    if reduce == 0:
        ered = 0
    if case['model'] and L.srx_plan_cus() != WF.CUS:
        assert (plan[0], plan[3]) == (kernel, ered), (case['id'], plan)
    else:
        assert plan[:4] + plan[5:] == [kernel, ens, erps, ered, eslabs], (case['id'], plan, case['expect'])
    ho, wo = WF.out_size(g)
    m = g['n'] * ho * wo
    ck = (g['cin'] + 3) // 4 * 4
    kk = g['k'] * g['k'] * ck
    cnw, kw = -(-g['cout'] // 64) * 64, -(-kk // 64) * 64
    nws = L.srx_conv2d_bwd_weight_multi_ws_floats(C.byref(d), nprob)
    up_floats = nprob * g['n'] * 2 * g['h'] * 2 * g['w'] * g['cin_s'] if g['up'] == 2 else 0
    assert nws == cnw * (kw + 1) * plan[1] * nprob + up_floats, (case['id'], nws, plan)
    ws_flat, ws = guarded(nws, dev, NAN)

    bufs, dys, olds = _operands(case['row'])
    gx = [_nhwc(b, g['cin_s']).to(dev) for b in bufs]
    if g['shuffle']:
        gdy = [_nhwc(TF.pixel_shuffle(t, 2), g['cout_s'], case['dy_off']).to(dev) for t in dys]
    else:
        gdy = [_nhwc(t, g['cout_s'], case['dy_off']).to(dev) for t in dys]
    outs = []   # per output, per conv: (dW allocation, dW view, db allocation, db view)
    for convs in olds:
        row = []
        for w0, b0 in convs:
            wf, wv = guarded(w0.numel(), dev, w0.reshape(-1).to(dev) if case['accumulate'] else NAN)
            bf, bv = guarded(b0.numel(), dev, b0.to(dev) if case['accumulate'] else NAN)
            row.append((wf, wv, bf, bv))
        outs.append(row)
    bias = case['bias']
    xs, dyp = _ptrs(gx), _ptrs([t.data_ptr() + 4 * case['dy_off'] for t in gdy])
    dws = _ptrs([r[0][1] for r in outs])
    dbs = _ptrs([r[0][3] for r in outs]) if bias else None
    acc, s = case['accumulate'], _stream()
    if case['call'] == 'plain':
        def run():
            lib.call('srx_conv2d_bwd_weight', C.byref(d), xs[0], dyp[0], dws[0], acc, dbs[0] if bias else None, ws.data_ptr(), nws, s)
    elif case['call'] == 'multi':
        def run():
            lib.call('srx_conv2d_bwd_weight_multi', C.byref(d), nprob, per_out, xs, dyp, dws, acc, dbs, ws.data_ptr(), nws, s)
    elif case['call'] == 'scaled':
        scales = (C.c_float * len(outs))(*case['scales'])

        def run():
            lib.call('srx_conv2d_bwd_weight_multi_scaled', C.byref(d), nprob, per_out, xs, dyp, dws, acc, dbs, scales, ws.data_ptr(), nws, s)
    else:
        dws_hi = _ptrs([r[1][1] for r in outs])
        dbs_hi = _ptrs([r[1][3] for r in outs]) if bias else None

        def run():
            lib.call('srx_conv2d_bwd_weight_multi_pair', C.byref(d), nprob, xs, dyp, dws, dws_hi, case['cin_lo'], acc, dbs, dbs_hi,
                     ws.data_ptr(), nws, s)
    names = prof_launches(run, aux=True)
    torch.cuda.synchronize()
    # exactly the slab kernel and the reduce kernel the plan reported
    want = [f"{WF.SLAB_KERNELS[plan[0]]} MxNxK={m}x{g['cout']}x{kk} x{nprob}", WF.REDUCE_KERNELS[plan[3]]]
    assert names == want, (case['id'], names, want)
    _SEEN.update(n.split(' MxNxK=')[0] for n in names)
    assert guards_intact(ws_flat), (case['id'], 'workspace bands')
    got = []
    for row in outs:
        conv = []
        for wf, wv, bf, bv in row:
            assert guards_intact(wf) and guards_intact(bf), (case['id'], 'output bands')
            conv.append((wv.cpu(), bv.cpu()))
        got.append(conv)
    return got, names


def _check(case, got):
    """Every output within the bound; the worst error / bound of dW and db"""
    ref, m = _reference(case['row'], case['precision'] != 0)
    _, _, olds = _operands(case['row'])
    worst = [0.0, 0.0]
    for o, convs in enumerate(ref):
        sc = _f32(case['scales'][o]) if case['scales'] else 1.0
        e = (1 if sc != 1.0 else 0) + (1 if case['accumulate'] else 0)
        gm = gamma(case['per_out'] * m + e, U)
        for j, (dw64, absw, db64, absb) in enumerate(convs):
            w0, b0 = olds[o][j]
            oldw = w0.double() if case['accumulate'] else torch.zeros_like(dw64)
            oldb = b0.double() if case['accumulate'] else torch.zeros_like(db64)
            gw, gb = got[o][j]
            for k, (have, want, bound) in enumerate(((gw.reshape(dw64.shape), sc * dw64 + oldw, gm * (abs(sc) * absw + oldw.abs())),
                                                     (gb, sc * db64 + oldb, gm * (abs(sc) * absb + oldb.abs())))):
                if k == 1 and not case['bias']:
                    continue
                assert bool(torch.isfinite(have).all()), (case['id'], o, j, 'dW' if k == 0 else 'db', 'not finite')
                err = (have.double() - want).abs()
                ratio = (err / bound.clamp_min(1e-300)).max().item()
                worst[k] = max(worst[k], ratio)
                assert bool((err <= bound).all()), (case['id'], o, j, 'dW' if k == 0 else 'db', ratio, err.max().item())
    return worst


def _run_case(dev, case):
    g = case['geo']
    kk = g['k'] * g['k'] * ((g['cin'] + 3) // 4 * 4)
    got, names = _launch(dev, case, -1)
    worst = _check(case, got)
    print('WGRADFORM %s %s + %s worst err/bound dW %.2e db %.2e' % (case['id'], names[0].split(' MxNxK=')[0], names[1], worst[0], worst[1]))
    if 4 * kk <= 48 * 1024:   # the other reduce kernel on the same slabs: bit for bit
        other, onames = _launch(dev, case, 0)
        assert onames[1] == 'wgrad_reduce_kernel' and names[1] == 'wgrad_reduce_rows_kernel'
        oworst = _check(case, other)
        same = all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for ra, rb in zip(got, other) for a, b in zip(ra, rb))
        print('WGRADFORM %s %s + %s worst err/bound dW %.2e db %.2e, reduce kernels bit-identical: %s'
              % (case['id'], onames[0].split(' MxNxK=')[0], onames[1], oworst[0], oworst[1], same))
        assert same, (case['id'], 'wgrad_reduce_kernel and wgrad_reduce_rows_kernel differ')
    else:
        assert names[1] == 'wgrad_reduce_kernel'
    _RAN.add(case['id'])
    _RESULTS[(case['row'], case['variant'])] = got
    twin = _RESULTS.get((case['row'], {'reg': 'dma', 'dma': 'reg'}.get(case['variant'])))
    if twin is not None:   # printed, not asserted: the two fp32 kernels need not sum in one order
        same = all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for ra, rb in zip(got, twin) for a, b in zip(ra, rb))
        print('WGRADFORM %s wgrad_kernel<0> and wgrad_dma_kernel bit-identical: %s' % (case['row'], same))


@pytest.mark.parametrize('case', WF.CASES, ids=WF.by_id(WF.CASES))
def test_wgrad_form_against_fp64(dev, case):
    _run_case(dev, case)


def test_refused_row_split_launches_nothing(dev):
    """15 image rows into 10 splits: the image-row kernel's call refuses, the gradient and the workspace stay as they were."""
    lib, L = _L()
    geo, prec, nsplit = WF.REFUSED_SPLITS[0]
    d = lib.Conv2dDesc(*WF.desc_fields(dict(geo=geo, precision=prec)))
    lib.call('srx_wgrad_force', -1, nsplit)
    assert L.srx_conv2d_bwd_weight_multi_ws_floats(C.byref(d), 1) == 0 and 'row splits refused' in lib.last_error()
    x = torch.zeros(geo['n'], geo['h'], geo['w'], geo['cin_s'], device=dev)
    dy = torch.zeros(geo['n'], geo['h'], geo['w'], geo['cout_s'], device=dev)
    dw = torch.full((geo['cout'], geo['cin'], 3, 3), 3.0, device=dev)
    ws = torch.full((1 << 18,), 5.0, device=dev)
    with pytest.raises(RuntimeError, match='row splits refused'):
        lib.call('srx_conv2d_bwd_weight', C.byref(d), x.data_ptr(), dy.data_ptr(), dw.data_ptr(), 0, None, ws.data_ptr(), ws.numel(), _stream())
    torch.cuda.synchronize()
    assert bool((dw == 3.0).all()) and bool((ws == 5.0).all())
    for bad in WF.BAD_FORCE_KERNELS:
        with pytest.raises(RuntimeError, match='wgrad_force_kernels'):
            lib.call('srx_wgrad_force_kernels', *bad)


def test_zz_every_kernel_of_wgrad_ran(dev):
    """The union of the kernel names this module's launches recorded is all nine (cases this process has not run yet run here)."""
    for case in WF.CASES:
        if case['id'] not in _RAN:
            _run_case(dev, case)
            _reset()
    print('WGRADFORM kernels recorded:', sorted(_SEEN))
    assert sorted(_SEEN) == sorted(WF.ALL_KERNELS), sorted(set(WF.ALL_KERNELS) ^ _SEEN)
