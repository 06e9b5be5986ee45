"""The three passes of nn.Linear (csrc/linear.hip) in every launch form of linear_forms.py, through the C ABI under
srx_linear_force, against fp64.

Bound, per element and with no fitted factor: |got - ref64| <= gamma(t) (|a| @ |b| (+ |bias| / |prefill|)) + one fp32 denormal,
gamma of step_layers.py at the fp32 unit roundoff 2^-24, t = the terms of the element's sum plus the additions behind it:
  forward        K products summed (in any order: gamma does not care how the MFMAs, the four waves and the splits cut the sum)
                 + `splits` additions of the partials (the first onto 0) + the bias + the LeakyReLU multiplication: K + splits + 2
  data gradient  J + splits + 1
  weight gradient B + 1, one more with accumulate (the addition onto what was there)
ReLU / LeakyReLU: an element whose fp64 pre-activation lies within its bound of 0 may come out on either side of the kink; exactly
those are left out of the activated comparison (under 1 % of a tensor: asserted, on the fp64 reference alone) and every element
is compared before the activation by a second call with act = 0.

Surroundings: every input is a view inside a NaN-filled device buffer with 64 rows of its own row length on either side -- further
than any form reaches past a tensor (b0 + 63 in the forward and data gradient, bb0 + 31 in the weight gradient, j0 + 15 in the
weight), so a load that the fast forms' range check wrongly admits lands in memory this test owns and poisons the result.  The
outputs and the workspace (passed at exactly srx_linear_ws_floats) are NaN-filled views between sentinel margins that must come
back bit-unchanged: a partial that the final pass reads and no split wrote, or an element no one stored, stays NaN.

The fast and the plain form cut and order every sum alike (linear.hip says so): wherever a shape runs both, the results are
held bit-equal."""
import ctypes as C

import pytest
import torch

import linear_forms as LF
from guarded import SENTINEL, Guarded, within
from step_layers import U32, gamma

pytestmark = pytest.mark.gpu

TINY = 2.0 ** -149
SLOPE32 = float(torch.tensor(LF.SLOPE, dtype=torch.float32))  # the slope the kernel multiplies by
CASES = {c[0]: c for c in LF.CASES}


@pytest.fixture
def lib():
    from torchsr_amd import _lib
    assert _lib.lib().srx_linear_force(0, 0) == 0
    try:
        yield _lib
    finally:
        assert _lib.lib().srx_linear_force(0, 0) == 0
        out = (C.c_int * 6)()
        assert _lib.lib().srx_linear_plan(16, 1024, 64, 0, out) == 0 and list(out) == [4, 256, 1, 1, 2, 2]


def workspace(dev, nws, k, j):
    """exactly srx_linear_ws_floats NaNs between sentinel margins of 64 of the longer rows"""
    return Guarded(dev, (nws,), margin=SENTINEL, margin_floats=64 * max(k, j))


_cache = {}


def inputs(b, k, j):
    """seeded inputs, weights scaled by K^-0.5 -- made once per shape, never written to"""
    key = ('in', b, k, j)
    if key not in _cache:
        _cache.clear()  # (one shape at a time: the product shapes' tensors are 75 MB each, 150 MB in fp64)
        g = torch.Generator().manual_seed(1000003 * b + 1009 * k + j)
        _cache[key] = dict(x=torch.randn(b, k, generator=g), w=torch.randn(j, k, generator=g) * k ** -0.5,
                           dy=torch.randn(b, j, generator=g), bias=torch.randn(j, generator=g) * 0.1,
                           dw0=torch.randn(j, k, generator=g))
    return _cache[key]


def reference(b, k, j):
    """the inputs, the fp64 results and the magnitude sums of the bounds"""
    r = inputs(b, k, j)
    if 'y' not in r:
        xd, wd, dyd = r['x'].double(), r['w'].double(), r['dy'].double()
        r['y'] = xd @ wd.t()
        r['y_mag'] = xd.abs() @ wd.abs().t()
        r['dx'] = dyd @ wd
        r['dx_mag'] = dyd.abs() @ wd.abs()
        r['dw'] = dyd.t() @ xd
        r['dw_mag'] = dyd.abs().t() @ xd.abs()
    return r


def plan(lib, b, k, j, which):
    out = (C.c_int * 6)()
    rc = lib.lib().srx_linear_plan(b, k, j, which, out)
    return list(out) if rc == 0 else None


def run(lib, dev, r, b, k, j, form, splits, acts, bias):
    """Every pass the forcing allows, in guarded buffers.  Returns ({name: result on the CPU}, the three plans)."""
    L = lib.lib()
    assert L.srx_linear_force(form, splits) == 0
    plans = [plan(lib, b, k, j, which) for which in (0, 1, 2)]
    nws = L.srx_linear_ws_floats(b, k, j)
    x, w, dy = Guarded(dev, (b, k), r['x']), Guarded(dev, (j, k), r['w']), Guarded(dev, (b, j), r['dy'])
    bs = Guarded(dev, (j,), r['bias'])
    res = {}
    guards = []
    if plans[0] is not None:
        assert nws >= plans[0][0] * b * j
        for act in acts:
            ws = workspace(dev, nws, k, j)
            y = Guarded(dev, (b, j), margin=SENTINEL)
            lib.call('srx_linear_fwd', x.ptr(), w.ptr(), bs.ptr() if bias else None, y.ptr(), b, k, j, act, SLOPE32, ws.ptr(), nws, None)
            res['y', act] = y.t.cpu()
            guards += [('y', y), ('ws(fwd)', ws)]
    if plans[1] is not None:
        assert nws >= plans[1][0] * b * k
        ws = workspace(dev, nws, k, j)
        dx = Guarded(dev, (b, k), margin=SENTINEL)
        lib.call('srx_linear_bwd_data', dy.ptr(), w.ptr(), dx.ptr(), b, k, j, ws.ptr(), nws, None)
        res['dx'] = dx.t.cpu()
        guards += [('dx', dx), ('ws(dgrad)', ws)]
    if plans[2] is not None:
        for acc in (0, 1):
            dw = Guarded(dev, (j, k), r['dw0'] if acc else None, margin=SENTINEL)
            lib.call('srx_linear_bwd_weight', x.ptr(), dy.ptr(), dw.ptr(), acc, b, k, j, None)
            res['dw', acc] = dw.t.cpu()
            guards.append(('dw', dw))
    torch.cuda.synchronize()
    for name, gd in guards:
        assert gd.margins_unchanged(), '%s: a store outside the tensor' % name
    for name, gd in (('x', x), ('w', w), ('dy', dy), ('bias', bs)):
        assert bool(torch.isnan(gd.buf[:gd.m]).all()) and bool(torch.isnan(gd.buf[-gd.m:]).all()), '%s: an input margin was written' % name
    assert L.srx_linear_force(0, 0) == 0
    return res, plans


def act64(v, act):
    if act == 1:
        return v.clamp_min(0.0)
    if act == 2:
        return torch.where(v > 0, v, v * SLOPE32)
    return v


@pytest.mark.parametrize('cid', LF.IDS)
def test_linear_form_against_fp64(dev, lib, cid):
    _, b, k, j, form, splits, act, bias, _ = CASES[cid]
    r = reference(b, k, j)
    res, plans = run(lib, dev, r, b, k, j, form, splits, sorted({0, act}), bias)
    assert plans == [None if p is None else list(p) for p in LF.PLANS[cid]], 'the case no longer runs the form it is there for'
    if plans[0] is not None:
        bd = r['bias'].double() if bias else torch.zeros(j, dtype=torch.float64)
        pre = r['y'] + bd
        bound = gamma(k + plans[0][0] + 2, U32) * (r['y_mag'] + bd.abs()) + TINY
        within(res['y', 0], pre, bound, 'y before the activation')
        if act:
            near = pre.abs() <= bound  # the kink may flip these: compared before the activation (above) alone
            assert near.double().mean().item() < 0.01, 'more than 1 % of the outputs within their bound of the kink'
            keep = ~near
            within(res['y', act][keep], act64(pre, act)[keep], bound[keep], 'y behind activation %d' % act)
    if plans[1] is not None:
        within(res['dx'], r['dx'], gamma(j + plans[1][0] + 1, U32) * r['dx_mag'] + TINY, 'dx')
    if plans[2] is not None:
        within(res['dw', 0], r['dw'], gamma(b + 1, U32) * r['dw_mag'] + TINY, 'dw')
        d0 = r['dw0'].double()
        within(res['dw', 1], r['dw'] + d0, gamma(b + 2, U32) * (r['dw_mag'] + d0.abs()) + TINY, 'dw, accumulated')
    # the same shape in the plain form, bit for bit
    if form != 1:
        plain, pplans = run(lib, dev, r, b, k, j, 1, splits, sorted({0, act}), bias)
        assert all(p is not None and p[4] == 1 and p[5] == 1 for p in pplans)
        both = sorted(set(plain) & set(res), key=str)
        assert both, 'nothing to compare'
        for name in both:
            assert torch.equal(plain[name], res[name]), 'the two forms differ in %s' % (name,)


@pytest.mark.parametrize('b,k,j', LF.PRODUCT, ids=lambda v: str(v))
def test_defaults_unchanged(dev, lib, b, k, j):
    """nothing forced = the form the plan reports, bit for bit"""
    r = inputs(b, k, j)
    free, plans = run(lib, dev, r, b, k, j, 0, 0, [0], 1)
    assert all(p is not None for p in plans) and len(free) == 4
    assert plans[0][4] == 2 and plans[0][5] == 2, 'the product shapes run the fast forward'
    forced = {}
    for which, names in ((0, [('y', 0)]), (1, ['dx']), (2, [('dw', 0), ('dw', 1)])):
        form = plans[which][4]
        assert form == plans[which][5]
        if form not in forced:
            forced[form] = run(lib, dev, r, b, k, j, form, 0, [0], 1)
        assert forced[form][1][which] == plans[which]
        for name in names:
            assert torch.equal(forced[form][0][name], free[name]), (which, name)
