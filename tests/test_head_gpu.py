"""The discriminator head + adversarial loss node (csrc/head.hip, functional.gan_head) against stock torch autograd on CPU in
fp64: srgan/discriminator.py:65-69 + srgan/trainer.py:446-448,456-457; esrgan/discriminator.py:73-76 + esrgan/trainer.py:451-453,
468-469.  Tolerance 2e-5 of each tensor's scale (fp32 sums of <= 18432 terms against fp64).

Below that: head.hip alone, through the C ABI on a given hidden layer, stage by stage against fp64 with derived elementwise bounds
(see the comment block there)."""
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu


def rel(a, b, floor=1e-9):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return ((a - b).abs().max() / b.abs().max().clamp_min(floor)).item()


def loss_from_saved(mode, v, n, weight, shift, addend):
    """the reference's expressions behind what the head saves for its backward -- v = sigmoid(z) (SRGAN modes) or z (ESRGAN modes):
    (loss, its terms by name)"""
    if mode == 0:
        a = TF.binary_cross_entropy(v[:n], torch.ones_like(v[:n]))
        c = TF.binary_cross_entropy(v[n:], torch.zeros_like(v[n:]))
        return a + c, dict(a=a, c=c)
    if mode == 1:
        adv = TF.binary_cross_entropy(v, torch.ones_like(v))
        return addend + weight * adv, dict(adv=adv)
    if mode == 2:
        real, fake = v[:n], v[n:]
        a = TF.binary_cross_entropy_with_logits(real - fake.mean(), torch.ones_like(real))
        c = TF.binary_cross_entropy_with_logits(fake - real.mean(), torch.zeros_like(fake))
        return (a + c) / 2, dict(a=a, c=c, mr=real.mean(), mf=fake.mean())
    adv = TF.binary_cross_entropy_with_logits(v - shift, torch.ones_like(v))
    return addend + weight * adv, dict(adv=adv)


def reference(mode, x, w1, b1, w2, b2, n, weight, shift, addend):
    """the reference's expressions, fp64"""
    h = TF.leaky_relu(TF.linear(x, w1, b1), 0.2)
    z = TF.linear(h, w2, b2)
    return loss_from_saved(mode, torch.sigmoid(z) if mode < 2 else z, n, weight, shift, addend)[0]


@pytest.mark.parametrize('mode,b,k,j,n', [(0, 32, 18432, 1024, 16), (1, 16, 18432, 1024, 0), (0, 4, 512, 1024, 2),
                                          (2, 32, 8192, 100, 16), (3, 16, 8192, 100, 0), (2, 6, 256, 100, 3), (0, 24, 300 * 4, 40, 9)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize('direct', [False, True], ids=['returned', 'into_grad'])
def test_gan_head(dev, mode, b, k, j, n, direct):
    from torchsr_amd import functional as F
    from torchsr_amd.layers import Linear
    g = torch.Generator().manual_seed(7 + mode)
    x = torch.randn(b, k, generator=g)
    lin1, lin2 = Linear(k, j), Linear(j, 1)
    with torch.no_grad():
        lin1.weight.copy_(torch.randn(j, k, generator=g) * (2.0 / k) ** 0.5)
        lin1.bias.copy_(torch.randn(j, generator=g) * 0.1)
        lin2.weight.copy_(torch.randn(1, j, generator=g) * (4.0 / j) ** 0.5)
        lin2.bias.copy_(torch.randn(1, generator=g) * 0.1)
    weight = 0.001 if mode == 1 else 0.005
    shift = torch.tensor(0.3) if mode == 3 else None
    addend = torch.tensor(1.25) if mode in (1, 3) else None
    # fp64 reference
    xr = x.double().requires_grad_(True)
    ps = [p.detach().double().requires_grad_(True) for p in (lin1.weight, lin1.bias, lin2.weight, lin2.bias)]
    ar = None if addend is None else addend.double().requires_grad_(True)
    ref = reference(mode, xr, *ps, n, weight, None if shift is None else shift.double(), ar)
    up = 0.7
    (ref * up).backward()
    # the node
    lin1, lin2 = lin1.to(dev), lin2.to(dev)
    xg = x.to(dev).requires_grad_(True)
    ag = None if addend is None else addend.to(dev).requires_grad_(True)
    params = [lin1.weight, lin1.bias, lin2.weight, lin2.bias]
    old = F.direct_grads[0]
    F.direct_grads[0] = direct
    try:
        if direct:  # the trainers' form: gradients ACCUMULATE into existing .grad buffers
            for p in params:
                p.grad = torch.full_like(p, 0.5)
        loss, aux = F.gan_head(xg, lin1, lin2, mode, n_first=n, slope=0.2, adv_weight=weight,
                               shift=None if shift is None else shift.to(dev), addend=ag)
        loss.backward(torch.tensor(up, device=dev))
    finally:
        F.direct_grads[0] = old
    assert rel(loss, ref) < 2e-5
    assert rel(xg.grad, xr.grad) < 2e-5
    # scale of a logit gradient: the relativistic discriminator loss does not depend on the last bias at all (the mean of
    # the other half is subtracted from every logit), so that gradient is an exact 0 that fp32 meets to rounding of its terms
    zscale = up / b
    for p, r in zip(params, ps):
        got = p.grad - 0.5 if direct else p.grad
        assert rel(got, r.grad, floor=zscale) < (2e-4 if direct else 2e-5), (tuple(p.shape))
    if ag is not None:
        assert rel(ag.grad, ar.grad) < 1e-6
        assert rel(aux[1], (ref - addend.double()) / weight) < 2e-4  # the adversarial term itself


def test_gan_head_without_weight_gradients(dev):
    """the discriminator pass of the generator update (srgan/trainer.py:456 under layers.no_weight_grad): input gradient only"""
    from torchsr_amd import functional as F
    from torchsr_amd.layers import Linear, no_weight_grad
    torch.manual_seed(3)
    lin1, lin2 = Linear(256, 64).to(dev), Linear(64, 1).to(dev)
    x = torch.randn(8, 256, device=dev, requires_grad=True)
    c = torch.tensor(2.0, device=dev, requires_grad=True)
    with no_weight_grad():
        loss, aux = F.gan_head(x, lin1, lin2, F.HEAD_SRGAN_G, adv_weight=0.001, addend=c)
    loss.backward()
    assert x.grad is not None and c.grad is not None and float(c.grad) == 1.0
    assert all(p.grad is None for p in list(lin1.parameters()) + list(lin2.parameters()))
    xr = x.detach().cpu().double().requires_grad_(True)
    ref = reference(1, xr, *[p.detach().cpu().double() for p in (lin1.weight, lin1.bias, lin2.weight, lin2.bias)], 0, 0.001, None,
                    torch.tensor(2.0, dtype=torch.float64))
    ref.backward()
    assert rel(x.grad, xr.grad) < 2e-5 and rel(loss, ref) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------------
# csrc/head.hip alone, through the C ABI on a given `hidden`: the head's own arithmetic, apart from the linear layer before it.
#
# The kernels hand over everything the next stage starts from -- the forward saves zp (probabilities / logits) and out[], the
# backward reads them back -- so every stage is held to the fp64 value of the reference's expression ON THE DEVICE'S OWN
# INPUT of that stage; the stages compose to the whole, and no bound has to carry the conditioning of log(1 - p) near p = 1.
# u = 2^-24 (one fp32 rounding), gamma(t) of step_layers.py, TINY one fp32 denormal.  ULP = 2 u: HIP's expf, logf and log1pf are
# within 1 ulp (HIP programming guide, "HIP math API", maximum ulp error of the single-precision functions), and one ulp of a
# result is at most 2 u of it; fp32 division and the casts from the fp64 row sums are correctly rounded (u).  U1 = u + 2^-45:
# a rounding to fp32 behind an fp64 sum of <= 256 terms.
#
#   logits   z = sum_j h w2 + b2: J products and J - 1 additions in eight lanes, the butterfly's three, the bias -- any order:
#            ez = gamma(J + 4) (|h| . |w2| + |b2|).  ESRGAN modes save z itself.
#   sigmoid  SRGAN modes save p = 1 / (1 + expf(-z)): sigmoid moves at most |dz| / 4, expf's 2 u reach p as 2 u (1 - p), the
#            addition and the division one u each, one more for the products of these: ep = ez / 4 + 5 u p.
#   terms    BCE(p, t in {0, 1}) = -max(logf(p), -100) or -max(log1pf(-p), -100), everything else exact: ULP |term|.
#            BCEWithLogits(a, t) = max(a, 0) - t a (exact in fp32) + log1pf(expf(-|a|)) with a = z - m: the rounded mean u |m| and
#            the subtraction u |a| move the term by as much (it is 1-Lipschitz); expf's 2 u reach the log as 2 u e / (1 + e) <= u,
#            log1pf adds ULP ln 2, the last addition u (|a| + ln 2): u (2 |a| + |m| + 4).
#   means    fp64 sums cast to fp32: the mean of the terms' errors + U1 |mean|; a + c, addend + weight adv: gamma(1), gamma(2).
#   dz       SRGAN: ((gl / cnt) (p - t) / max((1 - p) p, 1e-12)) p (1 - p) -- products and quotients only, 11 roundings and the
#            fp32 value of 1e-12: gamma(12) |dz|.  ESRGAN: coef (sigmoid(a) - t) with coef two roundings and the product one:
#            coef (u (|m| + |a|) / 4 + 5 u sigmoid + u |sigmoid - t|) + gamma(3) |d|; the discriminator's dz adds the other half's
#            sum over its own count: that half's errors and gamma(4) of its |sum| (U1, 1 / n, the product) over the count, and u |dz|.
#   dpre     dz w2 (slope): (edz + gamma(3) (|dz| + edz)) |w2| (slope).    dw2 = dz . h: (edz + gamma(B + 1) (|dz| + edz)) . |h|.
#   db1      sum_b dpre: sum_b (edpre + gamma(B) (|dpre| + edpre)).        db2 = fp32(sum64 dz): sum edz + U1 sum |dz|.
# ---------------------------------------------------------------------------------------------------------------------------
import ctypes as C  # noqa: E402

from guarded import SENTINEL, Guarded, within  # noqa: E402
from step_layers import U32, gamma  # noqa: E402

U = U32
ULP = 2.0 * U
U1 = U + 2.0 ** -45
TINY = 2.0 ** -149
SLOPE, UP = 0.2, 0.7


def f32(v):
    """the fp32 value a float argument becomes on its way into the kernel"""
    return float(torch.tensor(v, dtype=torch.float32))


def head_inputs(mode, b, j, seed=0):
    g = torch.Generator().manual_seed(100 * b + j + 7 * mode + seed)
    hidden = TF.leaky_relu(torch.randn(b, j, generator=g), SLOPE)
    hidden[::3, ::5] = 0.0  # (an output of exactly 0: LeakyReLU's backward from the output takes the slope there)
    return dict(hidden=hidden, w2=torch.randn(j, generator=g) * (4.0 / j) ** 0.5, b2=torch.randn(1, generator=g) * 0.1,
                shift=torch.tensor([0.3]), addend=torch.tensor([1.25]), weight=f32(0.001 if mode == 1 else 0.005))


def head_run(lib, dev, mode, b, j, n, t, loss=True, dw2=True, db2=True, db1=True, bias=True, prefill=None):
    """One forward and one backward launch in guarded buffers: {name: result on the CPU}.  `prefill`: accumulate = 1 onto it."""
    nan = float('nan')
    h = lib.GanHead(mode, b, j, n, SLOPE, t['weight'])
    hidden, w2 = Guarded(dev, (b, j), t['hidden']), Guarded(dev, (j,), t['w2'])
    one = {k: Guarded(dev, (1,), t[k], margin_floats=64) for k in ('b2', 'shift', 'addend')}
    zp = Guarded(dev, (b,), margin=SENTINEL)
    out = Guarded(dev, (8,), margin=SENTINEL, margin_floats=64)
    ls = Guarded(dev, (1,), margin=SENTINEL, margin_floats=64)
    gen = mode in (1, 3)
    lib.call('srx_gan_head_fwd', C.byref(h), hidden.ptr(), w2.ptr(), one['b2'].ptr() if bias else None,
             one['shift'].ptr() if mode == 3 else None, one['addend'].ptr() if gen else None, zp.ptr(), out.ptr(),
             ls.ptr() if loss else None, None)
    res = dict(zp=zp.t.cpu(), out=out.t.cpu(), loss=ls.t.cpu())
    # the backward reads what the forward saved, from NaN surroundings of its own
    zin, oin = Guarded(dev, (b,), zp.t), Guarded(dev, (8,), out.t, margin_floats=64)
    gs = Guarded(dev, (1,), torch.tensor([UP]), margin_floats=64)
    outs = dict(dpre=Guarded(dev, (b, j), margin=SENTINEL))
    for name, on, shape in (('dw2', dw2, (j,)), ('db2', db2, (1,)), ('db1', db1, (j,))):
        if on:
            outs[name] = Guarded(dev, shape, None if prefill is None else prefill[name], margin=SENTINEL, margin_floats=64 * j)
    ptr = lambda name: outs[name].ptr() if name in outs else None  # noqa: E731
    lib.call('srx_gan_head_bwd', C.byref(h), hidden.ptr(), w2.ptr(), zin.ptr(), oin.ptr(), one['shift'].ptr() if mode == 3 else None,
             gs.ptr(), ptr('dpre'), ptr('dw2'), ptr('db2'), ptr('db1'), 0 if prefill is None else 1, None)
    torch.cuda.synchronize()
    for name, gd in outs.items():
        res[name] = gd.t.cpu()
    for name, gd in list(outs.items()) + [('zp', zp), ('out', out), ('loss', ls), ('hidden', hidden), ('w2', w2), ('zp (backward)', zin),
                                          ('out (backward)', oin), ('g', gs)] + list(one.items()):
        assert gd.margins_unchanged(), '%s: a store outside the tensor' % name
    if not loss:
        assert bool(torch.isnan(res['loss']).all()), 'a NULL loss was written somewhere else'
    assert bool(torch.isnan(res['out'][6:]).all()) and (mode == 2 or bool(torch.isnan(res['out'][4:6]).all()))
    return res


def same(a, b, names=None):
    for name in names or sorted(set(a) | set(b)):
        assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), name  # (bitwise: NaN tails of out[] included)


def scalar(v):
    return torch.as_tensor(v, dtype=torch.float64).reshape(1)


def head_check(res, mode, b, j, n, t, bias=True, grads=('dw2', 'db2', 'db1')):
    """every stage of `res` against the fp64 value of the reference's expression on the stage's own input (bounds: above)"""
    hd, wd = t['hidden'].double(), t['w2'].double()
    bd = t['b2'].double() if bias else torch.zeros(1, dtype=torch.float64)
    weight, shift, addend = t['weight'], t['shift'].double(), t['addend'].double()
    # logits / probabilities
    z64 = hd @ wd + bd
    ez = gamma(j + 4, U) * (hd.abs() @ wd.abs() + bd.abs()) + TINY
    if mode < 2:
        p64 = torch.sigmoid(z64)
        within(res['zp'], p64, ez / 4 + 5 * U * p64 + TINY, 'p')
    else:
        within(res['zp'], z64, ez, 'z')
    # loss terms, from the saved tensor
    v = res['zp'].double()
    out = res['out'].double()
    half = [(slice(0, n), n), (slice(n, b), b - n)] if mode in (0, 2) else [(slice(0, b), b)]
    if mode < 2:
        tgt = torch.ones(b, dtype=torch.float64)
        if mode == 0:
            tgt[n:] = 0.0
        terms = TF.binary_cross_entropy(v, tgt, reduction='none')
        eterm = ULP * terms
        m_other = None
    else:
        if mode == 2:
            mr64, mf64 = v[:n].mean(), v[n:].mean()
            within(out[4:5], scalar(mr64), U * mr64.abs() + 2.0 ** -45 * v[:n].abs().mean() + TINY, 'out[4], mean(real)')
            within(out[5:6], scalar(mf64), U * mf64.abs() + 2.0 ** -45 * v[n:].abs().mean() + TINY, 'out[5], mean(fake)')
            m_other = torch.cat([out[5].expand(n), out[4].expand(b - n)])  # the means the device went on with
            tgt = torch.cat([torch.ones(n, dtype=torch.float64), torch.zeros(b - n, dtype=torch.float64)])
        else:
            m_other = shift.expand(b)
            tgt = torch.ones(b, dtype=torch.float64)
        a = v - m_other
        terms = TF.binary_cross_entropy_with_logits(a, tgt, reduction='none')
        eterm = U * (2 * a.abs() + m_other.abs() + 4)
    ref_terms = loss_from_saved(mode, v, n, weight, shift, addend)[1]
    means = []
    for (sl, cnt), name in zip(half, ('a', 'c') if len(half) == 2 else ('adv',)):
        m = terms[sl].mean()
        if mode != 2:  # (mode 2: `terms` starts from the device's rounded means, the reference from its own: within eterm)
            assert abs(float(m - ref_terms[name])) <= 2.0 ** -45 * float(m.abs()), 'the test restates the reference wrongly'
        else:
            assert abs(float(m - ref_terms[name])) <= float(U * m_other[sl].abs().max()) + 2.0 ** -45 * float(m.abs())
        means.append((m, eterm[sl].mean() + U1 * m.abs() + TINY))
    if len(half) == 2:
        within(out[1:2], scalar(means[0][0]), scalar(means[0][1]), 'out[1], the term of the first rows')
        within(out[2:3], scalar(means[1][0]), scalar(means[1][1]), 'out[2], the term of the other rows')
        tot = out[1] + out[2] if mode == 0 else 0.5 * out[1] + 0.5 * out[2]
        within(out[0:1], scalar(tot), scalar(gamma(1, U) * tot.abs() + TINY), 'out[0]')
    else:
        within(out[1:2], scalar(means[0][0]), scalar(means[0][1]), 'out[1], the adversarial term')
        tot = addend + weight * out[1]
        within(out[0:1], tot, gamma(2, U) * (addend.abs() + (weight * out[1]).abs()) + TINY, 'out[0]')
        assert float(res['out'][2]) == 0.0
    assert float(res['out'][3]) == 0.0
    if not torch.isnan(res['loss']).all():
        assert torch.equal(res['loss'], res['out'][0:1])
    # logit gradients, from the saved tensor and the saved means
    g = f32(UP)
    vv = v.clone().requires_grad_(True)
    (loss_from_saved(mode, vv, n, weight, shift, addend)[0] * g).backward()
    if mode < 2:
        dz = vv.grad * v * (1 - v)
        edz = gamma(12, U) * dz.abs() + TINY
    else:
        dz = vv.grad
        sg = torch.sigmoid(a)
        coef = torch.cat([torch.full((cnt,), (0.5 if mode == 2 else weight) * g / cnt, dtype=torch.float64) for _, cnt in half])
        d = coef * (sg - tgt)
        ed = coef * (U * (m_other.abs() + a.abs()) / 4 + 5 * U * sg + U * (sg - tgt).abs()) + gamma(3, U) * d.abs()
        if mode == 2:
            (r, nr), (f, nf) = half
            other = torch.cat([((ed[f].sum() + gamma(4, U) * d[f].sum().abs()) / nr).expand(nr),
                               ((ed[r].sum() + gamma(4, U) * d[r].sum().abs()) / nf).expand(nf)])
            edz = ed + other + U * dz.abs() + TINY
        else:
            edz = ed + TINY
    # what the backward makes of them
    lre = torch.where(t['hidden'] > 0, 1.0, f32(SLOPE)).double()
    dpre = dz[:, None] * wd[None, :] * lre
    edpre = (edz + gamma(3, U) * (dz.abs() + edz))[:, None] * wd.abs()[None, :] * lre + TINY
    within(res['dpre'], dpre, edpre, 'dpre')
    if 'dw2' in grads:
        within(res['dw2'], dz @ hd, (edz + gamma(b + 1, U) * (dz.abs() + edz)) @ hd.abs() + TINY, 'dw2')
    if 'db1' in grads:
        within(res['db1'], dpre.sum(0), (edpre + gamma(b, U) * (dpre.abs() + edpre)).sum(0) + TINY, 'db1')
    if 'db2' in grads:
        within(res['db2'], scalar(dz.sum()), scalar(edz.sum() * (1 + U) + U1 * dz.abs().sum() + TINY), 'db2')


@pytest.fixture
def lib():
    from torchsr_amd import _lib
    _lib.lib()
    return _lib


# (B, J, n_first): rows 2 (one of each call), 9, 33 (a second pass of 32 rows in the forward, a fifth trip of 8 in the backward), 40
# and 256 (HEAD_MAX_B); n_first 1, B - 1 and uneven in between; J 1, 7 (no multiple of 8: the eight lanes of a row end unevenly),
# 100 (ESRGAN's), 257 (a second workgroup of the backward with one unit), 1024 (SRGAN's), 2049
HEAD_SHAPES = [(2, 1, 1), (9, 7, 8), (33, 100, 13), (40, 257, 1), (9, 1024, 4), (256, 1024, 100), (33, 2049, 32), (256, 2049, 255), (40, 7, 39)]


@pytest.mark.parametrize('b,j,n', HEAD_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize('mode', [0, 1, 2, 3])
def test_head_alone(dev, lib, mode, b, j, n):
    """rows, units and modes: every output of both launches within its derived bound, nothing stored or read outside, and the
    second call bit-equal to the first (head.hip: fixed-order reductions)"""
    n = n if mode in (0, 2) else 0
    t = head_inputs(mode, b, j)
    res = head_run(lib, dev, mode, b, j, n, t)
    head_check(res, mode, b, j, n, t)
    same(res, head_run(lib, dev, mode, b, j, n, t))


@pytest.mark.parametrize('mode', [0, 1, 2, 3])
def test_head_pointer_forms(dev, lib, mode):
    b, j, n = 33, 257, (13 if mode in (0, 2) else 0)
    t = head_inputs(mode, b, j, seed=1)
    full = head_run(lib, dev, mode, b, j, n, t)
    head_check(full, mode, b, j, n, t)
    rest = ['zp', 'out', 'dpre', 'dw2', 'db2', 'db1']
    # loss = NULL, and each gradient NULL in turn: the others as before, bit for bit
    same(full, head_run(lib, dev, mode, b, j, n, t, loss=False), rest)
    for off in ('dw2', 'db2', 'db1'):
        got = head_run(lib, dev, mode, b, j, n, t, **{off: False})
        assert off not in got
        same(full, got, [name for name in rest + ['loss'] if name != off])
    # accumulate = 1: what accumulate = 0 stores, added to what was there -- one fp32 addition
    g = torch.Generator().manual_seed(5)
    prefill = dict(dw2=torch.randn(j, generator=g), db2=torch.randn(1, generator=g), db1=torch.randn(j, generator=g))
    acc = head_run(lib, dev, mode, b, j, n, t, prefill=prefill)
    same(full, acc, ['zp', 'out', 'loss', 'dpre'])
    for name in ('dw2', 'db2', 'db1'):
        want = full[name].double() + prefill[name].double()
        within(acc[name], want, U * want.abs() + TINY, name + ', accumulated')
    # b2 = NULL: a bias of 0
    nob = head_run(lib, dev, mode, b, j, n, t, bias=False)
    head_check(nob, mode, b, j, n, t, bias=False)
    zero = dict(t, b2=torch.zeros(1))
    same(nob, head_run(lib, dev, mode, b, j, n, zero))


def test_head_refusals(dev, lib):
    """more than 256 rows, and a discriminator update without rows of both calls: refused before anything is launched"""
    room = torch.zeros(257 * 16, device=dev)  # (never touched; real memory all the same, should a check ever be missed)
    one = C.c_void_p(room.data_ptr())
    L = lib.lib()
    for mode, b, n in [(0, 257, 100), (1, 257, 0), (2, 257, 100), (3, 257, 0), (0, 8, 0), (0, 8, 8), (2, 8, 0), (2, 8, 8), (0, 1, 1)]:
        h = lib.GanHead(mode, b, 16, n, SLOPE, 0.005)
        assert L.srx_gan_head_fwd(C.byref(h), one, one, one, one, one, one, one, one, None) == 1, (mode, b, n)
        assert 'gan_head_fwd' in lib.last_error()
        assert L.srx_gan_head_bwd(C.byref(h), one, one, one, one, one, one, one, one, one, one, 0, None) == 1, (mode, b, n)
        assert 'gan_head_bwd' in lib.last_error()


# rows of one call: (logit, ...) -- 40 and above give p == 1.0f (expf(-40) is below half an ulp of 1), -110 and below p == 0.0f
# (expf(110) overflows fp32: 1 / inf)
SATURATED = {
    'all wrong': ([-120.0, -110.0], [40.0, 55.0]),      # every term -max(log 0, -100) = 100
    'all right': ([40.0, 55.0], [-120.0, -110.0]),      # every term -log 1 = 0
    'mixed': ([40.0, -120.0, 0.3, -1.1, 2.5], [-120.0, 40.0, 0.7, -0.2, -3.0, 1.4, 31.0]),
}


@pytest.mark.parametrize('name', list(SATURATED))
@pytest.mark.parametrize('mode', [0, 1])
def test_head_saturated_probabilities(dev, lib, mode, name):
    """Logits that saturate the fp32 sigmoid, against torch's fp32 CPU autograd on the same `hidden`: p is exactly 1.0f or 0.0f,
    the loss terms of such rows exactly 0 or 100 (the -100 clamp of the logs), their dpre rows exactly 0 (torch's chain
    (p - t) / max((1 - p) p, 1e-12) . p (1 - p) ends in a factor 0).  fp64 is deliberately NOT the reference of these rows: in
    fp64 sigmoid(40) < 1 and sigmoid(-120) > 0, nothing saturates and the terms are 40 and 120, not 0 and 100.  The ordinary rows
    in between still meet head_check's bounds (which start every stage from the device's own saved p, so they hold here too)."""
    real, fake = SATURATED[name]
    logits = torch.tensor(real + fake)
    b, n, j = len(logits), (len(real) if mode == 0 else 0), 12
    t = head_inputs(mode, b, j, seed=2)
    t['hidden'] = t['hidden'] * 0.05
    t['hidden'][:, 0] = logits            # unit 0 carries the logit: w2[0] = 1, the other units add a few hundredths
    t['w2'][0] = 1.0
    t['b2'] = torch.zeros(1)
    res = head_run(lib, dev, mode, b, j, n, t)
    head_check(res, mode, b, j, n, t)
    same(res, head_run(lib, dev, mode, b, j, n, t))
    sat1, sat0 = logits >= 30.0, logits <= -110.0
    assert bool((res['zp'][sat1] == 1.0).all()) and bool((res['zp'][sat0] == 0.0).all())
    # torch, fp32, CPU
    h32 = t['hidden'].clone().requires_grad_(True)
    w32 = t['w2'].clone().requires_grad_(True)
    p32 = torch.sigmoid(TF.linear(h32, w32[None, :], t['b2']))[:, 0]
    assert bool((p32[sat1] == 1.0).all()) and bool((p32[sat0] == 0.0).all())
    l32, terms32 = loss_from_saved(mode, p32, n, t['weight'], None, t['addend'][0])
    (l32 * UP).backward()
    sat = sat1 | sat0
    assert bool((h32.grad[sat] == 0).all()), "torch's own fp32 chain does not end in 0 on the saturated rows"
    assert bool((res['dpre'][sat] == 0).all())
    tgt = torch.ones(b)
    if mode == 0:
        tgt[n:] = 0.0
    wrong = (sat1 & (tgt == 0)) | (sat0 & (tgt == 1))
    if name != 'mixed':  # every row saturated: each term exactly 100 (the wrong side) or 0, and the means those of such terms
        assert bool(sat.all())
        exact = torch.where(wrong, 100.0, 0.0).double()
        if mode == 0:
            a, c = float(exact[:n].mean()), float(exact[n:].mean())
            assert (a, c) == ((100.0, 100.0) if name == 'all wrong' else (0.0, 0.0))
            assert [float(x) for x in res['out'][:3]] == [a + c, a, c] and (terms32['a'].item(), terms32['c'].item()) == (a, c)
        else:  # (every row against 1: one call's rows are wrong where the other's are right)
            assert float(exact.mean()) == 50.0 and float(res['out'][1]) == 50.0 and terms32['adv'].item() == 50.0
    else:
        assert 0 < int(sat.sum()) < b and 0 < int(wrong.sum()) < int(sat.sum())
