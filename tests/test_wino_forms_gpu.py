"""Every launch form of the Winograd convolution (wino.hip; cases: wino_forms.py), through the C ABI so that no layer class can route
a call elsewhere.  Before a launch the forced plan is asserted from srx_wino_plan; after it the launch records (srx_prof_start_aux)
must name exactly the case's kernels.  Outputs, workspace and statistics tables start as NaN between sentinel bands, the inputs lie
between NaN bands; the workspace is exactly srx_wino_ws_floats(d, which) long, NULL where that is 0.  Two kinds of check:

(a) EXACT, every case.  Integer operands (wino_forms.int_inputs: x in {-1, 0, 1}, g in {-4, 0, 4}, integer bias and addend, slope
    0.25) keep every fp32 partial sum of the Winograd arithmetic an integer below 2^24 in any order (test_wino_forms_cpu.py), so the
    output must EQUAL torch's float64 convolution of the same integers, epilogue and PixelShuffle included, and the statistics table
    must equal the int64 sums over each block's valid tiles.  No tolerance: a dropped, doubled or mis-assigned chunk, tile, part or
    channel is off by at least 0.25.

(b) RANDOM data, one case per kernel path (wino_forms.RANDOM_IDS), against float64:
    * elementwise  |y - y64| <= gamma_k (|A^T| [sum_ci (|G||g||G^T|) (.) (|B^T||d||B|)] |A| + |bias| [+ |addend|]),  u = 2^-24,
      k = step_layers.wino_k: the rounding chain counted from the code (filter transform 4, input transform 2, product 1, Cin
      accumulations, parts - 1 additions of the splits or parts, output transform 4, bias 1), + 1 for LeakyReLU's multiplication,
      + 1 for the addend's addition.  Behind an activation the bound is scaled by the branch's slope where the float64
      pre-activation is further from 0 than its own bound (ReLU's negative side: exactly 0), and is the unscaled one where either
      branch is right.  A masked element of a data gradient is exactly 0.  Nothing in this bound is fitted.
    * the project's figures: max |err| <= 2e-5 max |ref|, and relL2(kernel, fp64) <= 3.0 relL2(torch CPU fp32, fp64) + 1e-7
      (F_WINO of test_step_layers_gpu.py).
    * statistics against float64 sums of the kernel's OWN output: gamma_128 sum |y| and gamma_129 sum y^2 per block and channel.
(c) linearity of a split: Z1 and T4 run the forced plan and the whole-tile plan (bn, 1, 1) of the same random layer (Z1.whole,
    T4.whole); each meets (b).

Times: profiles/wino_forms_tests_times.txt."""
import ctypes as C
import functools
import zlib

import pytest
import torch
import torch.nn.functional as TF

import wino_forms as WF
from guarded import Guarded, SENTINEL
from step_layers import gamma, prof_launches, wino_abs, wino_k

pytestmark = pytest.mark.gpu

F_WINO = 3.0
_SEEN = set()   # kernel names this module's launches recorded
_RAN = set()    # (kind, case id) that ran


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
        assert L.srx_wino_force_plan(0, 0, 0) == 0


def _skip_tail_elsewhere(case):
    _, L = _L()
    if case['tail'] and L.srx_plan_cus() != WF.CUS:
        pytest.skip(WF.TAIL_SKIP % L.srx_plan_cus())


# ------------------------------------------------------------------------------------------------ operands and fp64 references
@functools.lru_cache(maxsize=None)
def _operands(data, kind):
    """The CPU fp32 tensors of a data row (shared by its variants): x (the output gradient for a data gradient), w, bias, addend,
    below (the pre-activation of the layer below a data gradient; its ReLU is the mask).  kind 'int': wino_forms.int_inputs;
    'random': normal inputs, Kaiming weights."""
    case = WF.case(next(c['id'] for c in WF.CASES if c['data'] == data))
    n, h, w, cin, cout = case['geo']
    if kind == 'int':
        d = WF.int_inputs(case)
        return {k: torch.from_numpy(v).float() for k, v in d.items()}
    g = torch.Generator().manual_seed(zlib.crc32(data.encode()))
    return dict(x=torch.randn((n, cout if case['entry'] == 'dgrad' else cin, h, w), generator=g),
                w=torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5,
                bias=torch.randn((cout,), generator=g) * 0.1, addend=torch.randn((n, cout, h, w), generator=g),
                below=torch.randn((n, cin, h, w), generator=g))


def _effective(case, ops):
    """The forward problem the launch computes: a data gradient convolves dy with the transposed, flipped filter"""
    if case['entry'] == 'dgrad':
        return ops['x'], ops['w'].transpose(0, 1).flip(2, 3).contiguous()
    return ops['x'], ops['w']


@functools.lru_cache(maxsize=None)
def _conv_refs(data, kind):
    """Once per data row: the float64 convolution without bias, torch's fp32 one and (random data) the Winograd magnitude term."""
    case = WF.case(next(c['id'] for c in WF.CASES if c['data'] == data))
    a, w = _effective(case, _operands(data, kind))
    y64 = TF.conv2d(a.double(), w.double(), None, 1, 1)
    if kind == 'int':
        return y64, None, None
    return y64, TF.conv2d(a, w, None, 1, 1), wino_abs(a, w)


def _epilogue(case, ops, pre, dtype):
    """bias, activation, mask, addend and PixelShuffle on a pre-bias convolution, in ``dtype``: (pre-activation, output)"""
    if case['bias']:
        pre = pre + ops['bias'].to(dtype).view(1, -1, 1, 1)
    y = torch.relu(pre) if case['relu'] else torch.where(pre > 0, pre, pre * case['slope']) if case['slope'] else pre
    if case['mask']:
        y = y * (torch.relu(ops['below']) > 0).to(dtype)
    if case['addend']:
        y = y + ops['addend'].to(dtype)
    if case['entry'] == 'shuffle':
        y = TF.pixel_shuffle(y, 2)
    return pre, y


def _blocks(y, rows):
    """(N, C, H, W) -> [tile block][32 tiles][C][4 pixels], tiles in (image, tile row, tile column) order, padding tiles 0"""
    n, c, h, w = y.shape
    tiles = y.reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(-1, c, 4)
    pad = rows * WF.WT - tiles.shape[0]
    if pad:
        tiles = torch.cat([tiles, torch.zeros((pad, c, 4), dtype=tiles.dtype)])
    return tiles.reshape(rows, WF.WT, c, 4)


# ----------------------------------------------------------------------------------------------------------------- one launch
def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _launch(dev, case, kind):
    """The case's call under its forced plan: plan, workspace size, launch records and bands checked.  Returns (output NCHW on the
    CPU, statistics table [rows][C][2] on the CPU or None, the plan in the table's order)."""
    lib, L = _L()
    ops = _operands(case['data'], kind)
    n, h, w, cin, cout = case['geo']
    entry = case['entry']
    k, cols = WF.gemm_dims(case)
    d = lib.Conv2dDesc(*WF.desc_fields(case['geo'], entry, case['relu'], case['slope']))
    dref = C.byref(d)
    s = _stream()
    # operands: inputs between NaN bands (a read outside one poisons the result), the packed weights exactly as long as queried
    nf = L.srx_wino_packed_floats(dref)
    assert nf == 16 * cin * cout
    wg = Guarded(dev, tuple(ops['w'].shape), ops['w'])
    upk = Guarded(dev, (nf,), margin=SENTINEL, margin_floats=4096)
    lib.call('srx_wino_pack', dref, wg.ptr(), upk.ptr(), 1 if entry == 'dgrad' else 0, s)
    torch.cuda.synchronize()
    assert upk.margins_unchanged() and bool(torch.isfinite(upk.t).all()), (case['id'], 'pack')
    xg = Guarded(dev, (n, h, w, k), _nhwc(ops['x']))
    bias = Guarded(dev, (cout,), ops['bias'], margin_floats=256) if case['bias'] else None
    mask = Guarded(dev, (n, h, w, cin), _nhwc(torch.relu(ops['below']))) if case['mask'] else None
    add = Guarded(dev, (n, h, w, cout), _nhwc(ops['addend'])) if case['addend'] else None
    out_shape = (n, 2 * h, 2 * w, cout // 4) if entry == 'shuffle' else (n, h, w, cols)
    y = Guarded(dev, out_shape, margin=SENTINEL)
    rows = L.srx_wino_stat_rows(dref) if entry == 'stats' else 0
    part = Guarded(dev, (rows, cout, 2), margin=SENTINEL, margin_floats=4096) if entry == 'stats' else None
    # the plan, forced
    which = WF.which(entry, case['slope'], case['addend'])
    lib.call('srx_wino_force_plan', *(case['force'] or (0, 0, 0)))
    ints = (C.c_int * 6)()
    lib.call('srx_wino_plan', dref, which, ints)
    plan = (ints[0], ints[1], ints[5], ints[2], ints[3], ints[4])
    if case['force'] is not None or L.srx_plan_cus() == WF.CUS:
        assert plan == tuple(case['expect']), (case['id'], plan, case['expect'])
    nws = L.srx_wino_ws_floats(dref, which)
    bn, zs, ts = plan[:3]
    assert (nws > 0) == (zs > 1 or ts > 1), (case['id'], nws, plan)
    ws = Guarded(dev, (nws,), margin=SENTINEL, margin_floats=4096) if nws else None
    ws_ptr = ws.ptr() if nws else None

    def run():
        if entry == 'fwd':
            lib.call('srx_wino_fwd', dref, xg.ptr(), upk.ptr(), bias.ptr() if bias else None, y.ptr(), ws_ptr, nws, s)
        elif entry == 'dgrad':
            lib.call('srx_wino_bwd_data', dref, xg.ptr(), upk.ptr(), mask.ptr() if mask else None, y.ptr(), ws_ptr, nws, s)
        elif entry == 'stats':
            lib.call('srx_wino_fwd_stats', dref, xg.ptr(), upk.ptr(), bias.ptr() if bias else None, y.ptr(), part.ptr(), ws_ptr, nws, s)
        else:
            lib.call('srx_wino_fwd_act', dref, xg.ptr(), upk.ptr(), bias.ptr() if bias else None, add.ptr() if add else None, y.ptr(),
                     ws_ptr, nws, s)
    names = prof_launches(run, aux=True)
    torch.cuda.synchronize()
    lib.call('srx_wino_force_plan', 0, 0, 0)
    # exactly the kernels of the plan, in order
    kernels = [WF.MAIN[bn]] + ([WF.FIXUP] if zs > 1 else []) + ([WF.TAIL_FIXUP[bn]] if ts > 1 else [])
    want = [f'{kernels[0]} MxNxK={n * h * w}x{cols}x{9 * k}'] + kernels[1:]
    assert names == want, (case['id'], names, want)
    if case['force'] is not None or L.srx_plan_cus() == WF.CUS:
        assert kernels == case['kernels'], (case['id'], kernels)
    _SEEN.update(kernels)
    for name, buf in (('output', y), ('workspace', ws), ('statistics', part), ('packed weights', upk), ('input', xg)):
        assert buf is None or buf.margins_unchanged(), (case['id'], name, 'bands')
    got = y.t.cpu().permute(0, 3, 1, 2).contiguous()
    return got, (part.t.cpu() if part is not None else None), plan


# ------------------------------------------------------------------------------------------------------------ (a) exact
def _run_exact(dev, case):
    got, part, _ = _launch(dev, case, 'int')
    ops = _operands(case['data'], 'int')
    y64, _, _ = _conv_refs(case['data'], 'int')
    pre, want = _epilogue(case, ops, y64, torch.float64)
    assert got.shape == want.shape
    wrong = int((got.double() != want).sum())     # (a NaN -- an element never written -- is unequal too)
    assert wrong == 0, (case['id'], f'{wrong} of {want.numel()} elements differ', int(torch.isnan(got).sum()), 'NaN')
    if part is not None:
        blocks = _blocks(pre.to(torch.int64), part.shape[0])
        s1, s2 = blocks.sum((1, 3)), (blocks * blocks).sum((1, 3))
        bad = int((part[..., 0].double() != s1.double()).sum()), int((part[..., 1].double() != s2.double()).sum())
        assert bad == (0, 0), (case['id'], 'statistics entries that differ (sum, sum of squares):', bad, 'of', s1.numel())
    _RAN.add(('int', case['id']))


@pytest.mark.parametrize('case', WF.CASES, ids=WF.by_id(WF.CASES))
def test_wino_form_is_exact_on_integers(dev, case):
    _skip_tail_elsewhere(case)
    _run_exact(dev, case)


# ------------------------------------------------------------------------------------------------------------ (b), (c) random
def _run_random(dev, case):
    got, part, plan = _launch(dev, case, 'random')
    ops = _operands(case['data'], 'random')
    y64, y32, mag = _conv_refs(case['data'], 'random')
    k, _ = WF.gemm_dims(case)
    bn, zs, ts = plan[:3]
    lrelu, addend = bool(case['slope']), case['addend']
    kk = wino_k(k, max(zs, ts), case['bias'], extra=(1 if lrelu else 0) + (1 if addend else 0))
    if case['bias']:
        mag = mag + ops['bias'].double().abs().view(1, -1, 1, 1)
    pre64, want = _epilogue(case, ops, y64, torch.float64)
    _, theirs = _epilogue(case, ops, y32, torch.float32)
    # behind an activation: the negative branch's slope where the pre-activation is further below 0 than its own bound
    if case['relu'] or lrelu:
        neg = 0.0 if case['relu'] else case['slope']
        mag = torch.where(pre64 < -gamma(kk) * mag, neg * mag, mag)
    if addend:
        mag = mag + ops['addend'].double().abs()
    bound = gamma(kk) * mag
    if case['mask']:
        bound = bound * (torch.relu(ops['below']) > 0).double()
    if case['entry'] == 'shuffle':
        bound = TF.pixel_shuffle(bound, 2)
    assert bool(torch.isfinite(got).all()), (case['id'], 'not finite')
    err = (got.double() - want).abs()
    ratio = (err / bound.clamp_min(1e-300))[bound > 0].max().item()
    mine = ((got.double() - want).norm() / want.norm()).item()
    torchs = ((theirs.double() - want).norm() / want.norm()).item()
    print('WINOFORM %s plan %s k %d worst err/bound %.3f  max err / max ref %.2e  relL2 kernel %.3e torch-fp32 %.3e ratio %.2f'
          % (case['id'], plan[:3], kk, ratio, err.max().item() / want.abs().max().item(), mine, torchs, mine / max(torchs, 1e-300)))
    outside = int((err > bound).sum())
    assert outside == 0, (case['id'], f'{outside} of {err.numel()} elements outside the derived bound', ratio)
    assert err.max().item() <= 2e-5 * want.abs().max().item(), (case['id'], err.max().item(), want.abs().max().item())
    if part is not None:   # against the kernel's own output (the pre-activation IS the output of a statistics launch)
        blocks = _blocks(got.double(), part.shape[0])
        a1, a2 = blocks.abs().sum((1, 3)), blocks.square().sum((1, 3))
        e1, e2 = (part[..., 0].double() - blocks.sum((1, 3))).abs(), (part[..., 1].double() - a2).abs()
        print('WINOFORM %s statistics worst err/bound: sum %.3f  sum of squares %.3f'
              % (case['id'], (e1 / (gamma(128) * a1)).max().item(), (e2 / (gamma(129) * a2)).max().item()))
        assert bool((e1 <= gamma(128) * a1).all()) and bool((e2 <= gamma(129) * a2).all()), (case['id'], 'statistics')
    assert mine <= F_WINO * torchs + 1e-7, (case['id'], 'relL2 over F_WINO x torch fp32', mine, torchs, mine / max(torchs, 1e-300))
    _RAN.add(('random', case['id']))


@pytest.mark.parametrize('case', [WF.case(i) for i in WF.RANDOM_IDS], ids=WF.RANDOM_IDS)
def test_wino_form_within_the_derived_bound_of_fp64(dev, case):
    _skip_tail_elsewhere(case)
    _run_random(dev, case)


def test_zz_every_wino_kernel_ran(dev):
    """Over the whole file the launch records covered all five kernels (cases this process has not run yet run here)."""
    _, L = _L()
    for case in WF.CASES:
        if case['tail'] and L.srx_plan_cus() != WF.CUS:
            continue
        if ('int', case['id']) not in _RAN:
            _run_exact(dev, case)
    print('WINOFORM kernels recorded:', sorted(_SEEN))
    if L.srx_plan_cus() != WF.CUS:
        pytest.skip(WF.TAIL_SKIP % L.srx_plan_cus())
    assert sorted(_SEEN) == sorted(WF.ALL_KERNELS), sorted(set(WF.ALL_KERNELS) ^ _SEEN)
