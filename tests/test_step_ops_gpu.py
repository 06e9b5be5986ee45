"""The BatchNorm, loss, pool, activation-backward, layout and Adam kernels (norm.hip, loss.hip, eltwise.hip, optim.hip) at the sizes
the batch-16 SRGAN and ESRGAN steps run them, and at the edges of their launch geometry (step_layers.STEP_OPS).

Two kinds of check:

1. EXACT, on integer-valued data.  Inputs are small integers and slopes powers of two (step_layers.SLOPE = 0.25), so every
   product and every partial sum of every kernel is an fp32 number whatever the order of summation (the precondition, sum of
   |terms| < 2^24 per output counted in quarters, is verified in int64 by test_cpu.py::test_step_ops_integer_cases_stay_exact).
   The kernels' sums must then EQUAL the int64 truth: a dropped, doubled or mis-grouped row is off by at least a quarter.
2. RANDOM data against the formula of include/srx.h evaluated in float64 from the same fp32 operands, with bounds derived from
   the kernels' structure (u = 2^-24):
   * elementwise outputs: |out - ref64| <= c u B, B the sum of the absolute values of the expression's terms, c the number of
     roundings of the expression as the kernel evaluates it, plus one -- each c stands next to its expression below;
   * reductions: |out - ref64| <= gamma_k sum|terms|, gamma_k = k u / (1 - k u), k the longest fp32 chain the kernel's structure
     allows before it continues in fp64 (rows per block from srx_bn_rows_per_block, elements per thread + the wave and LDS
     folds for the losses), plus the roundings of one term.
   relL2(kernel, fp64) is printed beside relL2(torch CPU fp32, fp64); elementwise outputs are held to F_DIRECT x torch's
   (test_step_layers_gpu.py's figure), reductions only report the ratio (parity section).

The BatchNorm entry points are called on the ABI with the argument lists functional._BNAct passes (the statistics have to be
read back, and fed, directly); losses, pools, activations and Adam go through functional.* / optim.FlatAdam.
test_step_ops_are_covered holds the table to the steps: every non-convolution call of one eager step of each trainer must be a
row of STEP_OPS.
"""
import numpy as np
import pytest
import torch

from step_layers import OP_ARGS, OPS_TESTED_ELSEWHERE, SLOPE, STEP_OPS, int_inputs, op_key, record_op_calls

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
F_DIRECT = 1.5      # test_step_layers_gpu.py's budget for direct forms
# Outputs measured (MI355X) above the budget, relL2 > F_DIRECT x torch's + 1e-7.  One: the input gradient of a BatchNorm over 256
# rows per group whose channels have mean 4 / standard deviation 1.  Cause: srx_bn_partial_stats sums x and x^2 in fp32 per 32-row
# block and the variance is E[x^2] - E[x]^2 (include/srx.h): a 17-fold cancellation, and with eight blocks per group little
# averaging of the blocks' rounding errors -- invstd sits 4.8 x as far from fp64 as torch's (which accumulates in double on the
# CPU), and dy is linear in invstd: 3.21 x on 512 x 512 in two groups (3.07 x on 256 x 512 in one, inside the budget only through
# its 1e-7 floor).  From 576 rows per group on the ratio is <= 2.3 and inside the budget.  In the steps these statistics come from
# the conv epilogues' tables (test_step_layers_gpu.py bounds those).  The case is a strict xfail that raises FormOverBudget only
# after every other check has passed; the output may not move more than 10 % above its measured ratio.
OVER_F = {'bn.512x512.g2.lrelu dy': 3.21}
PIN_MARGIN = 1.1
EPS, MOM = 1e-5, 0.1
F32 = np.float32


class FormOverBudget(AssertionError):
    """An output's distance from fp64 is above F_DIRECT x torch fp32's (and within its pin): a finding OVER_F records."""


def gamma(k):
    return k * U / (1.0 - k * U)


def rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm((a - ref).ravel()) / max(np.linalg.norm(ref.ravel()), 1e-300))


def ulps(got, ref64):
    """distance of fp32 ``got`` from the float64 value ``ref64`` in units of ref's fp32 spacing"""
    ref64 = np.asarray(ref64, np.float64)
    return np.abs(np.asarray(got, np.float64) - ref64) / np.spacing(np.abs(ref64).astype(F32)).astype(np.float64)


def gpu(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(dev)


def host(t):
    return t.detach().cpu().numpy()


def p_(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def rng_of(case, salt=0):
    import zlib
    return np.random.default_rng(zlib.crc32(case['id'].encode()) + 1 + salt)


def budget(what, mine, theirs, report):
    print(f'  {what:44s} kernel {mine:.3e}  torch-fp32 {theirs:.3e}  ratio {mine / max(theirs, 1e-300):5.2f}')
    report.append((what, mine, theirs, mine > F_DIRECT * theirs + 1e-7))
    if what in OVER_F:
        assert mine <= PIN_MARGIN * OVER_F[what] * theirs + 1e-7, (what, mine, theirs, OVER_F[what])
    else:
        assert mine <= F_DIRECT * theirs + 1e-7, (what, mine, theirs)


def note_ratio(what, got, ref32, ref64):
    """reductions: the ratio to torch's fp32 distance is reported, not asserted (torch's CPU sums are pairwise)"""
    mine, theirs = rel_l2(got, ref64), rel_l2(ref32, ref64)
    print(f'  {what:44s} kernel {mine:.3e}  torch-fp32 {theirs:.3e}  ratio {mine / max(theirs, 1e-300):5.2f}  (reduction: reported)')


def within(what, got, ref64, bound):
    err = np.abs(np.asarray(got, np.float64) - ref64)
    worst = float((err - bound).max())
    print(f'  {what:44s} max |err| / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}')
    assert worst <= 0.0, (what, worst, float(err.max()))


def exact(what, got, truth):
    got, truth = np.asarray(got, np.float64), np.asarray(truth, np.float64)
    assert got.shape == truth.shape, (what, got.shape, truth.shape)
    bad = int((got != truth).sum())
    assert bad == 0, (what, f'{bad} of {got.size} differ', float(np.abs(got - truth).max()))


# ------------------------------------------------------------------------------------------------------------- BatchNorm
def bn_forward(case, dev, y, gamma_, beta, res, prelu, rm, rv, nbt, slope):
    """functional._BNAct.forward's calls; returns (partial table or None, mean, invstd, out)"""
    from torchsr_amd import _lib
    m, c, groups, act = case['M'], case['C'], case['groups'], case['act']
    s = stream()
    mean = torch.full((groups * c,), float('nan'), device=dev)
    invstd = torch.full((groups * c,), float('nan'), device=dev)
    out = torch.full_like(y, float('nan'))
    if case['training']:
        rows = _lib.lib().srx_bn_stat_rows(m)
        part = torch.full((rows, c, 2), float('nan'), device=dev)
        _lib.call('srx_bn_partial_stats', p_(y), p_(part), m, c, s)
        _lib.call('srx_bn_train_fwd', p_(y), p_(part), rows, m, c, groups, EPS, MOM, p_(gamma_), p_(beta), p_(res), p_(out), act,
                  slope, p_(prelu), p_(mean), p_(invstd), p_(rm), p_(rv), p_(nbt), s)
    else:
        part = None
        _lib.call('srx_bn_eval_stats', p_(rm), p_(rv), c, EPS, p_(mean), p_(invstd), s)
        _lib.call('srx_bn_act_fwd', p_(y), p_(mean), p_(invstd), p_(gamma_), p_(beta), p_(res), p_(out), m, c, act, slope,
                  p_(prelu), s)
    return part, mean, invstd, out


def bn_backward(case, dev, dout, y, mean, invstd, gamma_, beta, prelu, dgamma, dbeta, dprelu, slope):
    """functional._BNAct.backward's call with the parameters' .grad as accumulation targets; returns (sums, dy)"""
    from torchsr_amd import _lib
    m, c, groups, act = case['M'], case['C'], case['groups'], case['act']
    sums = torch.full((groups * (2 * c + 4),), float('nan'), device=dev)
    dy = torch.full_like(y, float('nan'))
    nws = _lib.lib().srx_bn_bwd_ws_floats(m, c)
    ws = torch.full((nws,), float('nan'), device=dev)
    _lib.call('srx_bn_act_bwd', p_(dout), p_(y), p_(mean), p_(invstd), p_(gamma_), p_(beta), p_(sums), p_(dy), m, c, groups, act,
              slope, p_(prelu), 1 if case['training'] else 0, p_(dgamma), p_(dbeta), p_(dprelu), p_(ws), nws, stream())
    return sums.view(groups, 2 * c + 4), dy


def expected_rows_per_block(m):
    return 512 if m >= 131072 else 128 if m >= 32768 else 32  # norm.hip: three row-block regimes


def running_ref(mu64, var64, per, rm0, rv0):
    """the running statistics after one update per group, in float64 with the fp32 rounding after each (include/srx.h)"""
    mom = float(F32(MOM))
    rm, rv = rm0.astype(np.float64), rv0.astype(np.float64)
    for g in range(mu64.shape[0]):
        unb = var64[g] * per / (per - 1.0) if per > 1 else var64[g]
        rm = ((1.0 - mom) * rm + mom * mu64[g]).astype(F32).astype(np.float64)
        rv = ((1.0 - mom) * rv + mom * unb).astype(F32).astype(np.float64)
    return rm, rv


def check_bn_exact(case, dev):
    from torchsr_amd import _lib
    m, c, groups, act = case['M'], case['C'], case['groups'], case['act']
    per = m // groups
    d = int_inputs(case)
    yi, di = d['y'].astype(np.int64), d['dout'].astype(np.int64)
    rng = rng_of(case)
    y, dout = gpu(d['y'], dev), gpu(d['dout'], dev)
    ones, zeros = torch.ones(c, device=dev), torch.zeros(c, device=dev)
    prelu = torch.full((1,), SLOPE, device=dev) if act == 3 else None
    rpb = _lib.lib().srx_bn_rows_per_block(m)
    assert rpb == expected_rows_per_block(m), (m, rpb)
    assert _lib.lib().srx_bn_stat_rows(m) == -(-m // rpb)
    rm0, rv0 = rng.standard_normal(c).astype(F32), (0.5 + rng.random(c)).astype(F32)
    rm, rv, nbt = gpu(rm0, dev), gpu(rv0, dev), torch.tensor(7, dtype=torch.int64, device=dev)
    part, mean, invstd, _ = bn_forward(case, dev, y, ones, zeros, None, prelu, rm, rv, nbt, SLOPE)
    if case['training']:
        edges = np.arange(0, m, rpb)
        got = host(part)
        exact('partial sums', got[:, :, 0], np.add.reduceat(yi, edges, axis=0))
        exact('partial sums of squares', got[:, :, 1], np.add.reduceat(yi * yi, edges, axis=0))
        s1 = yi.reshape(groups, per, c).sum(1).astype(np.float64)
        s2 = (yi * yi).reshape(groups, per, c).sum(1).astype(np.float64)
        mu = s1 / per
        var = np.maximum(s2 / per - mu * mu, 0.0)
        exact('mean', host(mean).reshape(groups, c), mu.astype(F32))
        # invstd and the running statistics: the fp64 formula of include/srx.h, rounded to fp32 where the kernel rounds (after
        # each group's update) -- 1 ulp
        assert ulps(host(invstd).reshape(groups, c), 1.0 / np.sqrt(var + float(F32(EPS)))).max() <= 1.0
        rm_ref, rv_ref = running_ref(mu, var, per, rm0, rv0)
        print(f'  running statistics: {ulps(host(rm), rm_ref).max():.2f} / {ulps(host(rv), rv_ref).max():.2f} ulp')
        assert ulps(host(rm), rm_ref).max() <= 1.0 and ulps(host(rv), rv_ref).max() <= 1.0
        assert int(nbt.item()) == 7 + groups
        if groups == 1:  # the one-group entry point on the same table: the same statistics, bit for bit
            m2, i2 = torch.full_like(mean, float('nan')), torch.full_like(invstd, float('nan'))
            _lib.call('srx_bn_finalize', p_(part), part.shape[0], m, c, EPS, MOM, p_(m2), p_(i2), None, None, None, stream())
            assert torch.equal(m2, mean) and torch.equal(i2, invstd)
    else:
        exact('eval mean', host(mean), rm0)
        # 1.0f / sqrtf(rv + eps): three roundings, plus one
        assert np.abs(host(invstd) - 1.0 / np.sqrt(rv0.astype(np.float64) + float(F32(EPS)))).max() <= 4 * U * (1.0 / np.sqrt(rv0.min()))
        assert int(nbt.item()) == 7
    # backward on fed statistics: mean 0, invstd 1, gamma 1, beta 0 -> xhat = z = y, an integer
    mean0, inv1 = torch.zeros(groups * c, device=dev), torch.ones(groups * c, device=dev)
    g0 = {k: rng.integers(-8, 9, n).astype(F32) for k, n in (('dgamma', c), ('dbeta', c), ('dprelu', 1))}
    acc = {k: gpu(v, dev) for k, v in g0.items()}
    sums, _ = bn_backward(case, dev, dout, y, mean0, inv1, ones, zeros, prelu, acc['dgamma'], acc['dbeta'],
                          acc['dprelu'] if act == 3 else None, SLOPE)
    dz4 = 4 * di if act == 0 else np.where(yi > 0, 4 * di, di)  # quarters (SLOPE = 1/4)
    sd = dz4.reshape(groups, per, c).sum(1) / 4.0
    sx = (dz4 * yi).reshape(groups, per, c).sum(1) / 4.0
    got = host(sums)
    exact('sum dz', got[:, :c], sd)
    exact('sum dz xhat', got[:, c:2 * c], sx)
    exact('dbeta_acc', host(acc['dbeta']), g0['dbeta'] + sd.sum(0))
    exact('dgamma_acc', host(acc['dgamma']), g0['dgamma'] + sx.sum(0))
    if act == 3:
        sp = np.where(yi > 0, 0, di * yi).reshape(groups, per * c).sum(1).astype(np.float64)
        exact('prelu partial', got[:, 2 * c], sp)
        exact('dprelu_acc', host(acc['dprelu']), g0['dprelu'] + sp.sum())


def act_np(z, act, slope):
    return z if act == 0 else np.where(z > 0, z, z * slope)


def torch_bn(y, gamma_, beta, res, dout, case, slope, dtype):
    """act(BatchNorm(y)) [+ res] and its gradients by torch autograd on the CPU in ``dtype``, group by group"""
    import torch.nn.functional as TF
    groups, act, c = case['groups'] if case['training'] else 1, case['act'], case['C']
    t = lambda a: torch.from_numpy(a).to(dtype)  # noqa: E731
    yt, gt, bt = t(y).requires_grad_(True), t(gamma_).requires_grad_(True), t(beta).requires_grad_(True)
    st = torch.tensor([slope], dtype=dtype, requires_grad=True)
    outs = []
    for yg in yt.chunk(groups):
        if case['training']:
            z = TF.batch_norm(yg, None, None, gt, bt, True, 0.0, EPS)
        else:
            z = TF.batch_norm(yg, t(case['_rm']), t(case['_rv']), gt, bt, False, 0.0, EPS)
        outs.append(z if act == 0 else TF.prelu(z, st))
    out = torch.cat(outs)
    if res is not None:
        out = out + t(res)
    out.backward(t(dout))
    return [a.detach().numpy() for a in (out, yt.grad, gt.grad, bt.grad)] + [st.grad.numpy() if act == 3 else None]


def check_bn_random(case, dev, report):
    from torchsr_amd import _lib
    m, c, groups, act, training = case['M'], case['C'], case['groups'], case['act'], case['training']
    per = m // groups
    rng = rng_of(case, 1)
    # channel means 0, 1 and 4 against standard deviations 1 and 4, every combination: E[x^2] - E[x]^2 cancels up to 17-fold
    ch_mean = np.array([0.0, 1.0, 4.0])[np.arange(c) % 3]
    ch_std = np.array([1.0, 4.0])[np.arange(c) % 2]
    y = (rng.standard_normal((m, c)) * ch_std + ch_mean).astype(F32)
    dout = rng.standard_normal((m, c)).astype(F32)
    res = rng.standard_normal((m, c)).astype(F32) if case['residual'] else None
    gam, bet = (1.0 + 0.2 * rng.standard_normal(c)).astype(F32), (0.1 * rng.standard_normal(c)).astype(F32)
    slope = SLOPE if act == 3 else 0.2
    slope64 = float(F32(slope))
    rm0, rv0 = (ch_mean + 0.1 * rng.standard_normal(c)).astype(F32), (ch_std ** 2 * (0.8 + 0.4 * rng.random(c))).astype(F32)
    case = dict(case, _rm=rm0, _rv=rv0)
    yg, dg, rg = gpu(y, dev), gpu(dout, dev), None if res is None else gpu(res, dev)
    gg, bg = gpu(gam, dev), gpu(bet, dev)
    prelu = torch.full((1,), slope, device=dev) if act == 3 else None
    rm, rv, nbt = gpu(rm0, dev), gpu(rv0, dev), torch.zeros((), dtype=torch.int64, device=dev)
    part, mean, invstd, out = bn_forward(case, dev, yg, gg, bg, rg, prelu, rm, rv, nbt, slope)
    acc = {k: torch.zeros(n, device=dev) for k, n in (('dgamma', c), ('dbeta', c), ('dprelu', 1))}
    sums, dy = bn_backward(case, dev, dg, yg, mean, invstd, gg, bg, prelu, acc['dgamma'], acc['dbeta'],
                           acc['dprelu'] if act == 3 else None, slope)
    tag = case['id']
    y64, d64 = y.astype(np.float64), dout.astype(np.float64)
    G = groups if training else 1
    mu_k, is_k = host(mean).reshape(G, c).astype(np.float64), host(invstd).reshape(G, c).astype(np.float64)
    if training:
        k = _lib.lib().srx_bn_rows_per_block(m)  # the longest fp32 chain: one block's rows, in any order
        edges = np.arange(0, m, k)
        a1, a2 = np.add.reduceat(np.abs(y64), edges, axis=0), np.add.reduceat(y64 * y64, edges, axis=0)
        got = host(part)
        within(f'{tag} partial sum', got[:, :, 0], np.add.reduceat(y64, edges, axis=0), gamma(k) * a1)
        within(f'{tag} partial sum sq', got[:, :, 1], a2, gamma(k + 1) * a2)  # (+ the rounding of the square)
        # finalize runs in fp64: the statistics inherit the tables' bounds; one rounding to fp32 at the end
        y3 = y64.reshape(G, per, c)
        mu, ex2 = y3.mean(1), (y3 * y3).mean(1)
        var = np.maximum(ex2 - mu * mu, 0.0)
        dmu = gamma(k) * np.abs(y3).mean(1)
        dvar = gamma(k + 1) * ex2 + 2 * np.abs(mu) * dmu + dmu * dmu
        within(f'{tag} mean', mu_k, mu, dmu + U * np.abs(mu))
        inv = 1.0 / np.sqrt(var + float(F32(EPS)))
        lo = 1.0 / np.sqrt(var + dvar + float(F32(EPS)))
        hi = 1.0 / np.sqrt(np.maximum(var - dvar, 0.0) + float(F32(EPS)))
        within(f'{tag} invstd', is_k, inv, np.maximum(hi - inv, inv - lo) + U * hi)
        t32 = torch.from_numpy(y).reshape(G, per, c)
        note_ratio(f'{tag} mean', mu_k, t32.mean(1).numpy(), mu)
        note_ratio(f'{tag} invstd', is_k, (t32.var(1, unbiased=False) + EPS).rsqrt().numpy(), inv)
    rep = lambda a: np.repeat(a, m // G, axis=0)  # noqa: E731  ([G][C] -> [M][C])
    mu_r, is_r = rep(mu_k), rep(is_k)
    g64, b64 = gam.astype(np.float64), bet.astype(np.float64)
    # out = act((y - mean) * (invstd * gamma) + beta) [+ res]: roundings y - mean, invstd * gamma, the product, + beta = 4, * slope
    # with an activation, + res with a residual, plus one: c = 5 .. 7; B = (|y| + |mean|) |invstd gamma| + |beta| [+ |res|]
    c_out = 4 + (1 if act else 0) + (0 if res is None else 1) + 1
    z64 = (y64 - mu_r) * (is_r * g64) + b64
    ref = act_np(z64, act, slope64) + (0.0 if res is None else res.astype(np.float64))
    B = (np.abs(y64) + np.abs(mu_r)) * np.abs(is_r * g64) + np.abs(b64) + (0.0 if res is None else np.abs(res))
    within(f'{tag} out (c = {c_out})', host(out), ref, c_out * U * B)
    # backward sums: terms dz = dout * act'(z) and dz * xhat, xhat = (y - mean) * invstd (2 roundings), z (2 more), dz (1), the
    # product (1): at most 6 per term on top of the chain of k rows; the fp64 finalize rounds once.  An element whose z is
    # within its own rounding error of 0 may take either slope: its whole |dout| (1 - slope) is allowed for.
    xh = (y64 - mu_r) * is_r
    zb = xh * g64 + b64
    amb = (np.abs(zb) <= 4 * U * (np.abs(xh * g64) + np.abs(b64))) if act else np.zeros_like(zb, bool)
    da = 1.0 if act == 0 else np.where(zb > 0, 1.0, slope64)
    dz = d64 * da
    k = _lib.lib().srx_bn_rows_per_block(m)
    flip = np.where(amb, np.abs(d64) * (1 - slope64), 0.0)
    Gs = G
    grp = lambda a: a.reshape(Gs, -1, c).sum(1)  # noqa: E731  (per group and channel)
    got = host(sums).astype(np.float64)
    if not training:
        got = got[:1]
    within(f'{tag} sum dz', got[:, :c], grp(dz), gamma(k + 7) * grp(np.abs(dz)) + grp(flip))
    within(f'{tag} sum dz xhat', got[:, c:2 * c], grp(dz * xh), gamma(k + 7) * grp(np.abs(dz * xh)) + grp(flip * np.abs(xh)))
    within(f'{tag} dbeta', host(acc['dbeta']), grp(dz).sum(0), gamma(k + 7 + Gs) * grp(np.abs(dz)).sum(0) + grp(flip).sum(0))
    within(f'{tag} dgamma', host(acc['dgamma']), grp(dz * xh).sum(0),
           gamma(k + 7 + Gs) * grp(np.abs(dz * xh)).sum(0) + grp(flip * np.abs(xh)).sum(0))
    if act == 3:  # one fp32 chain per block: rows x C / 256 per thread, 6 butterfly levels, 3 adds; d * z: 4 + 1 roundings
        kp = -(-k * c // 256) + 9
        tp = np.where(zb > 0, 0.0, d64 * zb)
        within(f'{tag} dprelu', host(acc['dprelu']), tp.sum(), gamma(kp + 6 + Gs) * np.abs(tp).sum() + (flip * np.abs(zb)).sum() + 1e-300)
    # dy = gamma invstd (dz - sum_dz / M - xhat sum_dzxhat / M) from the kernel's own sums.  Roundings, training: xhat 2, sd * invM 1,
    # the difference 1, xhat * sx 1, * invM 1, the difference 1, gamma * invstd 1, the product 1 = 9, dz = dout * slope 1 more with
    # an activation, plus one: c = 10 / 11.  Eval: both sums are 0 and drop out exactly, xhat only decides the slope: gamma *
    # invstd, the product, dz with an activation, plus one: c = 3 / 4.  (invM = 1.0f / (float) M is taken as the kernel computes
    # it); B = |gamma invstd| (|dz| + |sd invM| + |xhat sx invM|)
    c_dy = (9 if training else 2) + (1 if act else 0) + 1
    if training:
        inv_m = float(F32(1.0) / F32(per))
        sd, sx = rep(got[:, :c]), rep(got[:, c:2 * c])
    else:
        inv_m, sd, sx = 0.0, 0.0, 0.0
    gi = g64 * is_r

    def dy_of(dz_):
        return gi * (dz_ - sd * inv_m - xh * sx * inv_m), np.abs(gi) * (np.abs(dz_) + np.abs(sd * inv_m) + np.abs(xh * sx * inv_m))

    ref, B = dy_of(dz)
    err = np.abs(host(dy).astype(np.float64) - ref)
    if amb.any():  # either slope is right where z is within rounding of 0
        alt, B2 = dy_of(d64 * np.where(zb > 0, slope64, 1.0))
        err = np.where(amb, np.minimum(err, np.abs(host(dy) - alt)), err)
        B = np.maximum(B, B2)
    print(f'  {tag} dy (c = {c_dy}): max |err| / bound {float((err / np.maximum(c_dy * U * B, 1e-300)).max()):.3f}, ambiguous z: {int(amb.sum())}')
    assert (err <= c_dy * U * B).all(), (tag, 'dy', float(err.max()))
    if groups == 1:
        check_bn_wrappers(case, dev, (dg, yg, mean, invstd, gg, bg, prelu), slope, sums, dy, acc)
    # against torch on the CPU, fp32 and fp64 (true BatchNorm, its own statistics)
    t64 = torch_bn(y64, g64, b64, None if res is None else res.astype(np.float64), d64, case, slope64, torch.float64)
    t32 = torch_bn(y, gam, bet, res, dout, case, slope, torch.float32)
    budget(f'{tag} out', rel_l2(host(out), t64[0]), rel_l2(t32[0], t64[0]), report)
    budget(f'{tag} dy', rel_l2(host(dy), t64[1]), rel_l2(t32[1], t64[1]), report)
    note_ratio(f'{tag} dgamma', host(acc['dgamma']), t32[2], t64[2])
    note_ratio(f'{tag} dbeta', host(acc['dbeta']), t32[3], t64[3])
    if act == 3:
        note_ratio(f'{tag} dprelu', host(acc['dprelu']), t32[4], t64[4])


def check_bn_wrappers(case, dev, tensors, slope, sums, dy, acc):
    """The two-call form (srx_bn_act_bwd_reduce, srx_bn_act_bwd_apply) and srx_bn_act_bwd_finish WITH its apply pass, fed the table
    the reduce left in its workspace (the PReLU partial in one column): the same kernels behind other argument lists, so sums,
    accumulated gradients and dy must equal srx_bn_act_bwd's bit for bit."""
    from torchsr_amd import _lib
    m, c, act, training = case['M'], case['C'], case['act'], case['training']
    dout, y, mean, invstd, gam, bet, prelu = tensors
    nan = float('nan')
    nws = _lib.lib().srx_bn_bwd_ws_floats(m, c)
    ws = torch.full((nws,), nan, device=dev)
    a2 = {k: torch.zeros_like(v) for k, v in acc.items()}
    s2, dy2 = torch.full((2 * c + 4,), nan, device=dev), torch.full_like(dy, nan)
    _lib.call('srx_bn_act_bwd_reduce', p_(dout), p_(y), p_(mean), p_(invstd), p_(gam), p_(bet), p_(s2), m, c, act, slope, p_(prelu),
              p_(a2['dgamma']), p_(a2['dbeta']), p_(a2['dprelu']) if act == 3 else None, p_(ws), nws, stream())
    _lib.call('srx_bn_act_bwd_apply', p_(dout), p_(y), p_(mean), p_(invstd), p_(gam), p_(bet), p_(s2), p_(dy2), m, c, act, slope,
              p_(prelu), 1 if training else 0, stream())
    want = sums.reshape(-1)[:2 * c + 1]
    assert torch.equal(s2[:2 * c + 1], want) and torch.equal(dy2, dy)
    assert all(torch.equal(a2[k], acc[k]) for k in a2)
    if not training:
        return
    a3 = {k: torch.zeros_like(v) for k, v in acc.items()}
    s3, dy3 = torch.full((2 * c + 4,), nan, device=dev), torch.full_like(dy, nan)
    _lib.call('srx_bn_act_bwd_finish', p_(dout), p_(y), p_(mean), p_(invstd), p_(gam), p_(bet), p_(ws), _lib.lib().srx_bn_stat_rows(m), 1,
              p_(s3), p_(dy3), m, c, act, slope, p_(prelu), p_(a3['dgamma']), p_(a3['dbeta']), p_(a3['dprelu']) if act == 3 else None,
              stream())
    assert torch.equal(s3[:2 * c + 1], want) and torch.equal(dy3, dy)
    assert all(torch.equal(a3[k], acc[k]) for k in a3)


def run_bn(case, dev, report):
    check_bn_exact(case, dev)
    check_bn_random(case, dev, report)


def run_bn_finish(case, dev, report):
    """srx_bn_act_bwd_finish on a hand-built table (what srx_conv2d_bwd_data_bn leaves): sums and parameter gradients only
    (dy = NULL, as the residual tower calls it); the PReLU partial in one or two columns"""
    from torchsr_amd import _lib
    rows, c, cols = case['rows'], case['C'], case['prelu_cols']
    t = int_inputs(case)['table'].astype(np.int64)
    rng = rng_of(case)
    g0 = {k: rng.integers(-8, 9, n).astype(F32) for k, n in (('dgamma', c), ('dbeta', c), ('dprelu', 1))}
    acc = {k: gpu(v, dev) for k, v in g0.items()}
    sums = torch.full((2 * c + 4,), float('nan'), device=dev)
    prelu = torch.full((1,), SLOPE, device=dev)
    table = gpu(t, dev)
    _lib.call('srx_bn_act_bwd_finish', None, None, None, None, None, None, p_(table), rows, cols, p_(sums), None, case['M'], c, case['act'],
              0.0, p_(prelu), p_(acc['dgamma']), p_(acc['dbeta']), p_(acc['dprelu']), stream())
    col = t.sum(0)
    pre = col[2 * c] + (col[2 * c + 1] if cols == 2 else 0)
    got = host(sums)
    exact('finish sums', got[:2 * c], col[:2 * c])
    exact('finish prelu', got[2 * c], pre)
    exact('finish dbeta', host(acc['dbeta']), g0['dbeta'] + col[:c])
    exact('finish dgamma', host(acc['dgamma']), g0['dgamma'] + col[c:2 * c])
    exact('finish dprelu', host(acc['dprelu']), g0['dprelu'] + pre)


# ----------------------------------------------------------------------------------------------- colsum, activations, axpby
def run_colsum(case, dev, report):
    from torchsr_amd import _lib
    m, c, cs, accumulate = case['M'], case['C'], case['Cs'], case['accumulate']
    xi = int_inputs(case)['x'].astype(np.int64)
    rng = rng_of(case)
    nws = max(1, _lib.lib().srx_colsum_ws_floats(m, c))

    def call(x, out0):
        out = gpu(out0, dev)
        ws = torch.full((nws,), float('nan'), device=dev)
        xg = gpu(x, dev)
        _lib.call('srx_colsum', p_(xg), p_(out), m, c, cs, accumulate, p_(ws), nws, stream())
        return host(out)

    out0 = rng.integers(-8, 9, c).astype(F32)
    exact('colsum', call(xi, out0), xi[:, :c].sum(0) + (out0 if accumulate else 0))
    # random data: the fp32 chain is one partial block's rows (the scalar fallback sums in fp64: one rounding)
    x = rng.standard_normal((m, cs)).astype(F32)
    rpb = max(16, -(-m // 256)) if cs % 4 == 0 else 1  # eltwise.hip colsum_rows_per_block: at most 256 partial rows, 16 rows at least
    got = call(x, out0)
    x64 = x.astype(np.float64)[:, :c]
    ref = x64.sum(0) + (out0 if accumulate else 0)
    within(f"{case['id']} random", got, ref, gamma(rpb + 2) * (np.abs(x64).sum(0) + np.abs(out0)))
    note_ratio(f"{case['id']}", got, torch.from_numpy(x)[:, :c].sum(0).numpy() + (out0 if accumulate else 0), ref)


def run_prelu_bwd(case, dev, report):
    from torchsr_amd import functional as F
    n = case['n']
    d = int_inputs(case)
    xi, gi = d['x'].astype(np.int64), d['dy'].astype(np.int64)
    x = gpu(d['x'], dev).requires_grad_(True)
    w = torch.nn.Parameter(torch.full((1,), SLOPE, device=dev))
    w.grad = torch.full((1,), 5.0, device=dev)  # a .grad buffer with something in it: the kernel accumulates
    was = F.direct_grads[0]
    F.direct_grads[0] = True
    try:
        y = F.prelu(x, w)
        y.backward(gpu(d['dy'], dev))
    finally:
        F.direct_grads[0] = was
    exact('prelu y', host(y), np.where(xi > 0, 4 * xi, xi) / 4.0)
    exact('prelu dx', host(x.grad), np.where(xi > 0, 4 * gi, gi) / 4.0)
    exact('prelu dslope (accumulated)', host(w.grad), [5.0 + np.where(xi > 0, 0, gi * xi).sum()])
    x2 = gpu(d['x'], dev).requires_grad_(True)  # without a sink: the gradient is returned (accumulate = 0)
    w2 = torch.full((1,), SLOPE, device=dev, requires_grad=True)
    F.prelu(x2, w2).backward(gpu(d['dy'], dev))
    exact('prelu dslope', host(w2.grad), [np.where(xi > 0, 0, gi * xi).sum()])
    assert n == xi.size


def run_act_bwd(case, dev, report):
    """dx = y > 0 ? dy : (ReLU ? 0 : dy * slope): one product per element, so ANY fp32 data must match numpy's fp32 bit for bit"""
    from torchsr_amd import _lib
    rng = rng_of(case)
    act, slope = case['act'], 0.2
    if case['op'] == 'act_bwd':
        n = case['n']
        y = np.maximum(rng.standard_normal(n), 0).astype(F32) if act == 1 else rng.standard_normal(n).astype(F32)
        dy = rng.standard_normal(n).astype(F32)
        dx, dyg, yg = torch.full((n + 4,), float('nan'), device=dev), gpu(dy, dev), gpu(y, dev)
        _lib.call('srx_act_bwd_from_out', p_(dyg), p_(yg), p_(dx), n, act, slope, stream())
        got = host(dx)
        assert np.isnan(got[n:]).all()  # nothing written past n
        got = got[:n]
    else:
        m, c, ld = case['M'], case['C'], case['ld']
        y = rng.standard_normal((m, ld)).astype(F32)
        dy = rng.standard_normal((m, ld)).astype(F32)
        dx, dyg, yg = torch.full((m, ld), float('nan'), device=dev), gpu(dy, dev), gpu(y, dev)
        _lib.call('srx_act_bwd_from_out_strided', p_(dyg), ld, p_(yg), ld, p_(dx), ld, m, c, act, slope, stream())
        got = host(dx)
        assert np.isnan(got[:, c:]).all()  # the other channels of the wide buffer are not touched
        got, y, dy = got[:, :c], y[:, :c], dy[:, :c]
    ref = np.where(y > 0, dy, F32(0) if act == 1 else dy * F32(slope))
    assert np.array_equal(got, ref), case['id']


def run_axpby(case, dev, report):
    """y = a x + b z: roundings a x, b z, the sum = 3, plus one: c = 4 (an fma drops one); B = |a x| + |b z|"""
    from torchsr_amd import functional as F
    rng = rng_of(case)
    n, a, b = case['n'], 0.2, 1.0
    x, z = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    got = host(F.axpby(gpu(x, dev), gpu(z, dev), a, b))
    a64, b64 = float(F32(a)), float(F32(b))
    ref = a64 * x.astype(np.float64) + b64 * z
    within(f"{case['id']}", got, ref, 4 * U * (np.abs(a64 * x) + np.abs(b64 * z)))
    t32 = (torch.from_numpy(x) * a + torch.from_numpy(z) * b).numpy()
    budget(f"{case['id']} y", rel_l2(got, ref), rel_l2(t32, ref), report)


def run_channels(case, dev, report):
    """srx_axpby_channels / srx_copy_channels on channel slices of wide rows, integer data and a = 0.25: exact"""
    from torchsr_amd import _lib
    m, c, wide = case['M'], case['C'], case['wide']
    rng = rng_of(case)
    x, z = (rng.integers(-8, 9, (m, wide)).astype(F32) for _ in range(2))
    y0 = rng.integers(-8, 9, (m, wide)).astype(F32)
    xg, zg, yg = gpu(x, dev), gpu(z, dev), gpu(y0, dev)
    xo, zo, yo = 64, 0, wide - c
    _lib.call('srx_axpby_channels', p_(xg), wide, xo, p_(zg), wide, zo, p_(yg), wide, yo, c, m, SLOPE, 1.0, stream())
    want = y0.copy()
    want[:, yo:yo + c] = x[:, xo:xo + c] * F32(SLOPE) + z[:, zo:zo + c]
    assert np.array_equal(host(yg), want)  # (the other channels of the wide rows untouched)
    for accumulate in (0, 1):
        dst = gpu(y0, dev)
        dense = gpu(x[:, :c].copy(), dev)
        _lib.call('srx_copy_channels', p_(dense), c, 0, p_(dst), wide, yo, c, m, accumulate, stream())
        want = y0.copy()
        want[:, yo:yo + c] = x[:, :c] + (y0[:, yo:yo + c] if accumulate else 0)
        assert np.array_equal(host(dst), want)


# ------------------------------------------------------------------------------------------------------------------ losses
def loss_chain(n):
    """the longest fp32 chain of loss_partial_kernel: min(1024, ceil(n / 1024)) blocks of 256 threads stride over n, then 6
    butterfly levels in the wave and 3 adds across the four waves; everything after that is fp64"""
    nb = min(1024, -(-n // 1024))
    return -(-n // (nb * 256)) + 6 + 3


def run_pair_loss(case, dev, report):
    """mse / l1 (with and without an explicit divisor) / mean"""
    from torchsr_amd import functional as F
    op, n, count = case['op'], case['n'], case.get('count', 0)
    div = count or n

    def run(a, b, gscale):
        ag = gpu(a, dev).requires_grad_(True)
        bg = gpu(b, dev).requires_grad_(True)
        loss = F.mse_loss(ag, bg) if op == 'mse' else F.l1_loss(ag, bg, count) if op == 'l1' else F.mean(ag)
        (loss * gscale).backward()
        return host(loss), host(ag.grad), None if op == 'mean' else host(bg.grad)

    def terms(a64, b64):
        dlt = a64 - b64
        return (dlt * dlt, 2 * dlt) if op == 'mse' else (np.abs(dlt), np.sign(dlt)) if op == 'l1' else (a64, np.ones_like(a64))

    d = int_inputs(dict(case, op='mse'))  # (the three families share one generator; the id seeds it)
    ai, bi = d['a'].astype(np.int64), d['b'].astype(np.int64) * (0 if op == 'mean' else 1)
    pow2 = n & (n - 1) == 0 and not count
    loss, da, db = run(ai, bi, 0.5 if pow2 else 1.0)
    t, dt = terms(ai.astype(np.float64), bi.astype(np.float64))
    assert float(loss) == float(F32(t.sum() / div)), (case['id'], float(loss), t.sum() / div)  # float32(sum / n), the sums exact
    if pow2:  # gscale / n a power of two: the backward is exact too
        exact('da', da, 0.5 / n * dt)
    if db is not None:
        assert np.array_equal(db, -da)
    # random data
    rng = rng_of(case)
    a, b = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32) * (0 if op == 'mean' else 1)
    loss, da, db = run(a, b, 1.0)
    t, dt = terms(a.astype(np.float64), b.astype(np.float64))
    # a term costs 2 roundings (mse: a - b, the square), the fp64 tail one more (the cast of sum * (1 / n))
    k = loss_chain(n) + 2 + 1
    within(f"{case['id']} loss", loss, t.sum() / div, gamma(k) * np.abs(t).sum() / div)
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    t32 = ((ta - tb) ** 2).sum() if op == 'mse' else (ta - tb).abs().sum() if op == 'l1' else ta.sum()
    note_ratio(f"{case['id']} loss", loss, float(t32) / F32(div), t.sum() / div)
    # da = (gscale * (1.0f / (float) n)) * d: roundings 1 / n, gscale / n, a - b, the product = 4, plus one: c = 5
    ref = dt / div
    within(f"{case['id']} da", da, ref, 5 * U * np.abs(ref))
    if db is not None:
        assert np.array_equal(db, -da)

    def torch_grad(dtype):  # autograd of torch's own loss on the CPU
        import torch.nn.functional as TF
        xa, xb = ta.to(dtype).requires_grad_(True), tb.to(dtype)
        if op == 'mse':
            val = TF.mse_loss(xa, xb)
        elif op == 'l1':
            val = (xa - xb).abs().sum() / count if count else TF.l1_loss(xa, xb)
        else:
            val = xa.mean()
        val.backward()
        return xa.grad.numpy()

    g64 = torch_grad(torch.float64)
    budget(f"{case['id']} da", rel_l2(da, g64), rel_l2(torch_grad(torch.float32), g64), report)


# logf / log1pf / expf of the device library: the ROCm install carries no accuracy table for them (no HIP math document under its
# share/ tree), so the figure is measured, two ways, by test_device_log_and_exp_... below, in ulps of the float64 value's fp32
# spacing (MI355X):
#   * densely and independently of loss.hip -- torch's device log / log1p / exp (ATen's elementwise kernels over the same device
#     math library) on 3.6e5 arguments in (0, 1] and 3.2e5 in [0, 90]: log 1.875, log1p 0.562, exp 0.836;
#   * through loss.hip itself, one element per call (srx_bce_fwd / srx_bce_logits_fwd on n = 1: the loss IS that element's term),
#     2 500 probabilities and 2 000 logits: logf 2.107, log1pf 0.519, log1pf(expf(.)) 1.290.
# The bounds allow twice the worst figure found, 2 x 2.107 = 4.2, stated with headroom as 5 ulps per call; both sweeps run with every
# suite and must stay within the half of that -- a fast intrinsic in loss.hip (hundreds of ulps near p = 1) would not.  A property
# of the math library, not of the kernels under test.
MATH_ULPS = 5.0


def run_bce(case, dev, report):
    from torchsr_amd import functional as F
    op, n = case['op'], case['n']
    rng = rng_of(case)
    k = loss_chain(n)
    for target in (1.0, 0.0):
        if op == 'bce':
            p = (1.0 / (1.0 + np.exp(-rng.standard_normal(n) * 6))).astype(F32)
            p[::7], p[3::11] = 0.0, 1.0  # saturated probabilities: the -100 clamp
            p = np.clip(p, 0.0, 1.0)
            pg = gpu(p, dev).requires_grad_(True)
            loss = F.bce_loss(pg, target)
            p64 = p.astype(np.float64)
            with np.errstate(divide='ignore'):
                lg = np.maximum(np.log(p64), -100.0) if target == 1.0 else np.maximum(np.log1p(-p64), -100.0)
            t = -lg
            # per element: the library's log (MATH_ULPS), for target 0 the rounding of 1 - (-p) is inside log1pf's argument (exact:
            # negation), the product with the target and the negation are exact: (MATH_ULPS + 1) u |term|
            per_elem = (2 * MATH_ULPS + 1) * U * np.abs(t)  # (1 ulp is at most 2 u of the value)
            dref = (p64 - target) / np.maximum((1 - p64) * p64, float(F32(1e-12))) / n
            dc = 6  # p - t, 1 - p, the product, the quotient, 1 / n, the scaling = 6 roundings ... plus one below
        else:
            x = (rng.standard_normal(n) * 10).astype(F32)
            x[::5] = np.clip(x[::5] * 3, -30, 30)  # |logit| up to 30
            shift = F32(0.375)
            xg = gpu(x, dev).requires_grad_(True)
            loss = F.bce_with_logits(xg, target, torch.tensor(shift, device=dev))
            a = (x - shift).astype(np.float64)  # (the kernel's a = x - shift, one rounding, taken as computed)
            sp = np.log1p(np.exp(-np.abs(a)))
            t = (1 - target) * a + np.maximum(-a, 0) + sp
            # (1 - t) a + max(-a, 0) + log1p(exp(-|a|)): two additions, expf and log1pf (MATH_ULPS each, on a term <= log 2)
            per_elem = 3 * U * (np.abs((1 - target) * a) + np.maximum(-a, 0) + sp) + 2 * (2 * MATH_ULPS) * U * sp
            dref = (1.0 / (1.0 + np.exp(-a)) - target) / n
            dc = 5  # expf (counted in MATH_ULPS below), 1 + e, the quotient, - target, 1 / n, the scaling
        loss.backward()
        what = f"{case['id']} target {target:.0f}"

        def torch_grad(dtype):  # autograd of torch's own loss on the CPU
            import torch.nn.functional as TF
            if op == 'bce':
                v = torch.from_numpy(p).to(dtype).requires_grad_(True)
                TF.binary_cross_entropy(v, torch.full_like(v, target)).backward()
            else:
                v = torch.from_numpy(x).to(dtype).requires_grad_(True)
                z = v - torch.tensor(shift).to(dtype)
                TF.binary_cross_entropy_with_logits(z, torch.full_like(z, target)).backward()
            return v.grad.numpy()
        within(f'{what} loss', host(loss), t.sum() / n, (gamma(k + 1) * np.abs(t).sum() + per_elem.sum() * (1 + gamma(k))) / n + 1e-300)
        got = host((pg if op == 'bce' else xg).grad).astype(np.float64)
        if op == 'bce':
            within(f'{what} dp', got, dref, (dc + 1) * U * np.abs(dref))
        else:  # sigmoid(a) - t cancels for t = 1: the bound is on the terms |sigmoid| + |t|
            sg = 1.0 / (1.0 + np.exp(-a))
            within(f'{what} dx', got, dref, (dc + 1 + 2 * MATH_ULPS) * U * (sg + target) / n)
        g64 = torch_grad(torch.float64)
        budget(f"{what} {'dp' if op == 'bce' else 'dx'}", rel_l2(got, g64), rel_l2(torch_grad(torch.float32), g64), report)


def test_device_log_and_exp_are_within_the_ulps_the_bce_bounds_assume(dev):
    """The two sweeps behind MATH_ULPS (see there): the device library through torch, densely, and loss.hip's own calls one
    element at a time, against float64.  Every figure must stay within MATH_ULPS / 2: the BCE bounds allow twice that."""
    from torchsr_amd import _lib
    worst = {}
    p = np.unique(np.concatenate([np.linspace(0, 1, 1 << 18)[1:], 10.0 ** -np.linspace(0, 37, 1 << 16),
                                  1 - 10.0 ** -np.linspace(0.5, 7.5, 1 << 16)]).astype(F32))
    p = p[(p > 0) & (p < 1)]
    pg, p64 = torch.from_numpy(p).to(dev), p.astype(np.float64)
    worst['lib log'] = float(ulps(host(torch.log(pg)), np.log(p64)).max())
    worst['lib log1p'] = float(max(ulps(host(torch.log1p(-pg)), np.log1p(-p64)).max(), ulps(host(torch.log1p(pg)), np.log1p(p64)).max()))
    a = np.unique(np.concatenate([np.linspace(0, 40, 1 << 18), np.random.default_rng(1).random(1 << 16) * 90]).astype(F32))
    e64 = np.exp(-a.astype(np.float64))
    worst['lib exp'] = float(ulps(host(torch.exp(-torch.from_numpy(a).to(dev))), e64)[e64 > 1.2e-38].max())  # (normal results)
    ws, out = torch.zeros(2048, device=dev), torch.zeros((), device=dev)
    grid = np.unique(np.concatenate([np.linspace(1e-6, 1 - 1e-6, 1500), 10.0 ** -np.linspace(0.01, 30, 500),
                                     1 - 10.0 ** -np.linspace(0.5, 7, 500)]).astype(F32))
    for v in grid[(grid > 0) & (grid < 1)]:  # -logf(p) and -log1pf(-p): the whole term of one element
        pt = torch.full((1,), float(v), device=dev)
        for tgt, f, name in ((1.0, lambda z: -np.log(z), 'logf'), (0.0, lambda z: -np.log1p(-z), 'log1pf')):
            _lib.call('srx_bce_fwd', p_(pt), tgt, p_(out), 1, p_(ws), stream())
            worst[name] = max(worst.get(name, 0.0), float(ulps(out.item(), min(f(np.float64(v)), 100.0))))
    for v in np.linspace(0.0, 30.0, 2000).astype(F32):  # a >= 0, target 1: the term is log1pf(expf(-a)) alone
        xt = torch.full((1,), float(v), device=dev)
        _lib.call('srx_bce_logits_fwd', p_(xt), None, 1.0, p_(out), 1, p_(ws), stream())
        worst['log1pf(expf)'] = max(worst.get('log1pf(expf)', 0.0), float(ulps(out.item(), np.log1p(np.exp(-np.float64(v))))))
    print('  worst ulp error:', {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= MATH_ULPS / 2, worst


# ------------------------------------------------------------------------------------------------------------- pools, layout
def run_pool(case, dev, report):
    import torch.nn.functional as TF
    from torchsr_amd import _lib, functional as F
    n, h, w, c = case['N'], case['H'], case['W'], case['C']
    rng = rng_of(case)
    x = np.maximum(rng.integers(-3, 4, (n, h, w, c)), 0).astype(F32)  # ReLU outputs: 4/7 zeros, many windows tie (at 0 and above)
    xg = gpu(x, dev).requires_grad_(True)
    y = F.maxpool2x2(xg)
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    yt = TF.max_pool2d(xt, 2, 2)
    assert np.array_equal(host(y), yt.detach().permute(0, 2, 3, 1).numpy())
    if not case.get('bwd'):
        return
    gy = rng.standard_normal((n, h // 2, w // 2, c)).astype(F32)
    y.backward(gpu(gy, dev))
    yt.backward(torch.from_numpy(gy).permute(0, 3, 1, 2))
    ref = xt.grad.permute(0, 2, 3, 1).numpy()
    assert np.array_equal(host(xg.grad), ref)
    win = (ref != 0).reshape(n, h // 2, 2, w // 2, 2, c)
    assert all(win[:, :, i, :, j].any() for i in (0, 1) for j in (0, 1))  # the maxima sit at each of the four positions
    dx, gyg = torch.full_like(xg, float('nan')), gpu(gy, dev)
    _lib.call('srx_maxpool2x2_relu_bwd', p_(gyg), p_(xg), p_(dx), n, h, w, c, stream())
    assert np.array_equal(host(dx), ref * (x > 0))


def run_layout(case, dev, report):
    from torchsr_amd import functional as F
    n, c, h, w, cs = case['N'], case['Cin'], case['H'], case['W'], case['Cs']
    x = rng_of(case).standard_normal((n, c, h, w)).astype(F32)
    y = F.to_nhwc(gpu(x, dev), cs)
    want = np.zeros((n, h, w, cs), F32)
    want[..., :c] = x.transpose(0, 2, 3, 1)
    assert np.array_equal(host(y), want)
    assert np.array_equal(host(F.to_nchw(y, c)), x)


# -------------------------------------------------------------------------------------------------------------------- Adam
_ADAM_LENGTHS = {}


def adam_lengths(dev):
    """the flat-buffer lengths of the four models, read from the built models"""
    if not _ADAM_LENGTHS:
        from torchsr_amd.esrgan import discriminator as ed, generator as eg
        from torchsr_amd.optim import FlatParams
        from torchsr_amd.srgan import discriminator as sd, generator as sg
        for kind, g, d in (('srgan', sg, sd), ('esrgan', eg, ed)):
            _ADAM_LENGTHS[f'{kind}.G'] = FlatParams(g.Generator().to(dev)).numel
            _ADAM_LENGTHS[f'{kind}.D'] = FlatParams(d.Discriminator().to(dev)).numel
    return _ADAM_LENGTHS


def run_adam(case, dev, report):
    """Five steps of optim.FlatAdam (srx_adam_step) with grad_scale 0.5 and the learning rate halved ON THE DEVICE between steps 2
    and 3; after every step p, m, v against ONE float64 Adam step from the kernel's own previous fp32 state.
      g' = g * scale                                  1 rounding
      m' = b1 m + (1 - b1) g'                         + 3: c = 5, B = |b1 m| + |(1 - b1) g'|
      v' = b2 v + (1 - b2) g' g'                      + 4: c = 6, B = v'
      p' = p - step_size (m' / (sqrt(v') / sqrt(bc2) + eps))
           m' 4 roundings, the denominator 8 (v' 5, sqrt, quotient, + eps), the quotient, the product, the difference 3, the two
           scalars step_size = lr / bc1 and sqrt(bc2) 2: 17, plus one: c = 18, B = |p| + step_size (|m'| + B_m) / denom
    (1 - b1, 1 - b2, bc1, bc2 are taken as the kernel computes them: fp32 differences, bias corrections from a float64 pow.)"""
    from torchsr_amd import optim
    n = case.get('n') or adam_lengths(dev)[case['model']]
    rng = rng_of(case)
    pad = 8 + (-n) % 4  # (FlatParams rounds a buffer up to whole quads)
    holder = torch.nn.Module()
    holder.w = torch.nn.Parameter(torch.zeros(n + pad, device=dev))
    flat = optim.FlatParams(holder)
    flat.numel = n  # the padding past n belongs to nobody: it must come back untouched
    opt = optim.FlatAdam(flat, lr=1e-4)
    opt.grad_scale = 0.5
    p0 = (rng.standard_normal(n + pad) * 0.05).astype(F32)
    flat.data.copy_(gpu(p0, dev))
    sentinel = (np.arange(pad) + 1.5).astype(F32)
    for buf in (flat.data, opt.exp_avg, opt.exp_avg_sq):
        buf[n:] = gpu(sentinel, dev)
    b1, b2, eps = (float(F32(v)) for v in (0.9, 0.999, 1e-8))
    omb1, omb2 = float(F32(1) - F32(0.9)), float(F32(1) - F32(0.999))
    lr = 1e-4
    p, m, v = p0[:n].astype(np.float64), np.zeros(n), np.zeros(n)
    for step in range(1, 6):
        if step == 3:
            opt.lr_dev.mul_(0.5)  # StepLR's rewrite of the device scalar
            lr *= 0.5
        g = (rng.standard_normal(n + pad) * 10.0 ** rng.integers(-6, 0, n + pad)).astype(F32)
        flat.grad.copy_(gpu(g, dev))
        opt.step()
        gs = g[:n].astype(np.float64) * 0.5
        bc1 = float(F32(1.0 - b1 ** step))
        bc2s = float(np.sqrt(F32(1.0 - b2 ** step)))
        ss = float(F32(float(F32(lr)) / bc1))
        bm = np.abs(b1 * m) + np.abs(omb1 * gs)
        m_ref = b1 * m + omb1 * gs
        v_ref = b2 * v + omb2 * gs * gs
        den = np.sqrt(v_ref) / bc2s + eps
        p_ref = p - ss * (m_ref / den)
        got = [host(t).astype(np.float64) for t in (flat.data, opt.exp_avg, opt.exp_avg_sq)]
        for t in got:
            assert np.array_equal(t[n:], sentinel), (case['id'], step, 'padding past n was written')
        pk, mk, vk = (t[:n] for t in got)
        what = f"{case['id']} step {step}"
        within(f'{what} m', mk, m_ref, 5 * U * bm)
        within(f'{what} v', vk, v_ref, 6 * U * v_ref + 1e-300)
        within(f'{what} p', pk, p_ref, 18 * U * (np.abs(p) + ss * (np.abs(m_ref) + bm) / den))
        if step == 5:  # torch's fp32 Adam step from the same state (the CPU's own arithmetic)
            tp, tm, tv = (torch.from_numpy(a.astype(F32)) for a in (p, m, v))
            tg = torch.from_numpy(g[:n]) * 0.5
            tm = tm * 0.9 + tg * (1 - 0.9)
            tv = tv * 0.999 + tg * tg * (1 - 0.999)
            tp = tp - (lr / (1 - 0.9 ** step)) * (tm / (tv.sqrt() / (1 - 0.999 ** step) ** 0.5 + 1e-8))
            # (p moves by ~lr per step: the distance is taken on the UPDATE p' - p, not on p, where it would vanish)
            budget(f"{case['id']} update", rel_l2(pk - p, p_ref - p), rel_l2(tp.numpy().astype(np.float64) - p, p_ref - p), report)
            budget(f"{case['id']} m", rel_l2(mk, m_ref), rel_l2(tm.numpy(), m_ref), report)
            budget(f"{case['id']} v", rel_l2(vk, v_ref), rel_l2(tv.numpy(), v_ref), report)
        p, m, v = pk, mk, vk
    assert int(opt.step_count.item()) == 5


RUNNERS = {'bn': run_bn, 'bn_finish': run_bn_finish, 'colsum': run_colsum, 'prelu_bwd': run_prelu_bwd, 'act_bwd': run_act_bwd,
           'act_bwd_strided': run_act_bwd, 'axpby': run_axpby, 'mse': run_pair_loss, 'l1': run_pair_loss, 'mean': run_pair_loss,
           'bce': run_bce, 'bce_logits': run_bce, 'channels': run_channels, 'pool': run_pool, 'layout': run_layout, 'adam': run_adam}


def case_covers(case, dev):
    if case['op'] == 'adam' and 'model' in case:
        return [('srx_adam_step', adam_lengths(dev)[case['model']], 0, 1, 0)]
    return case['covers']


def _param(case):
    over = {k: v for k, v in OVER_F.items() if k.split(' ')[0] == case['id']}
    if not over:
        return pytest.param(case, id=case['id'])
    why = ', '.join(f'{k} {v:.2f} x' for k, v in over.items())
    return pytest.param(case, id=case['id'], marks=pytest.mark.xfail(strict=True, raises=FormOverBudget,
                                                                       reason=f'measured above F (torch fp32 distance): {why}'))


@pytest.mark.parametrize('case', [_param(c) for c in STEP_OPS])
def test_step_op(dev, monkeypatch, case):
    report = []
    calls = record_op_calls(monkeypatch, lambda: RUNNERS[case['op']](case, dev, report))
    made = {op_key(n, a) for n, a in calls if n in OP_ARGS}
    missing = [k for k in case_covers(case, dev) if k not in made]  # the case makes the calls the guard credits it with
    assert not missing, (case['id'], missing, sorted(made))
    over = [(what, mine / max(theirs, 1e-300)) for what, mine, theirs, out in report if out]
    if over:
        raise FormOverBudget(over)


def _step_calls(dev, monkeypatch):
    import os
    from conftest import GOLDEN
    from oracle.weights import seeded_input
    import test_esrgan_gpu
    import test_step_gpu
    gold = np.load(os.path.join(GOLDEN, 'srgan_steps.npz'))
    s_lr, s_hr = (int(v) for v in gold['b16_seeds'])
    lr, hr = seeded_input((16, 3, 24, 24), s_lr).to(dev), seeded_input((16, 3, 96, 96), s_hr).to(dev)
    t = test_step_gpu.make_trainer(dev, use_graphs=False, batch=16)
    t.overlap_branches = False
    calls = record_op_calls(monkeypatch, lambda: t.gan_step(lr, hr))
    del t
    gold = np.load(os.path.join(GOLDEN, 'esrgan.npz'))
    s_lr, s_hr = (int(v) for v in gold['b4_seeds'])
    lr = seeded_input((4, 3, 32, 32), s_lr).repeat(4, 1, 1, 1).to(dev)
    hr = seeded_input((4, 3, 128, 128), s_hr).repeat(4, 1, 1, 1).to(dev)
    t = test_esrgan_gpu.make_trainer(dev, batch=16)
    t.overlap_branches = False
    return calls + record_op_calls(monkeypatch, lambda: t.gan_step(lr, hr))


def test_step_ops_are_covered(dev, monkeypatch):
    """One eager batch-16 GAN step of each trainer with ``_lib.call`` (and its aliases) wrapped: every non-convolution call --
    (entry point, M or n, C, groups, act) -- is credited to a row of STEP_OPS (test_step_op checks that the row really makes that
    call), or is one of the entry points outside the four files, which have op-level tests of their own (OPS_TESTED_ELSEWHERE).
    A new size or entry point in a step fails here until it has a case."""
    calls = _step_calls(dev, monkeypatch)
    assert calls
    table = {k for case in STEP_OPS for k in case_covers(case, dev)}
    unknown = sorted({n for n, _ in calls if n not in OP_ARGS and n not in OPS_TESTED_ELSEWHERE})
    assert not unknown, unknown
    missing = sorted({op_key(n, a) for n, a in calls if n in OP_ARGS} - table)
    assert not missing, missing
