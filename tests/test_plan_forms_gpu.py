"""The launch forms of plan_forms.py on the GPU, each against an fp64 evaluation of the same operation on the CPU:

1. the 48-pixel row tile (rowtile.hip, RT48) in its five modes -- plain, BNR, BNL, BNB, BNR + BNB -- at one and at two patch-load
   batches per thread, with nothing reserved (11 520 pixels) and at the reference batch with 8 compute units reserved;
2. the persistent inference kernels (c64.hip, thin9.hip; bf16 and fp16) with more work items than workgroups, so that every
   workgroup goes through its item loop more than once;
3. the plans a reservation produces (srx_set_reserved_cus, as ddp.GradBuckets sets it inside a step): K-split tails, tiles,
   Winograd column widths, chunk geometry and weight-gradient row splits at values no other test runs -- the reported plan,
   the kernel that ran (its srx_prof record) and the numbers, as test_forced_paths_gpu.py checks its forced plans.

test_plan_forms_cpu.py proves through the planners alone that every case reaches its form.  Outputs, side outputs and
workspaces start as NaN; channels that belong to nobody hold a sentinel.  Every size a launch needs is asked for under the
reservation the launch runs under."""
import contextlib
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as TF

import plan_forms as PF
from test_forced_paths_gpu import SENTINEL, _launched, _plan, _tile_args, rel_err

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
U16 = 2.0 ** -11   # fp16 unit roundoff (test_fp16_inference_gpu.py)
NAN = float('nan')


def gamma(k):
    """Bound on the relative error of an fp32 sum of k terms in any order (test_step_ops_gpu.py)."""
    return k * U / (1.0 - k * U)


def _L():
    from torchsr_amd import _lib
    return _lib, _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _reserved_now(L):
    return max(0, L.srx_device_cus() - L.srx_plan_cus())


@pytest.fixture(scope='module', autouse=True)
def _reservation_restored():
    """Whatever the cases reserve, the module leaves the plans as it found them."""
    yield
    if torch.cuda.is_available():
        _, L = _L()
        assert L.srx_plan_cus() == L.srx_device_cus()


@pytest.fixture
def reserve(dev):
    """reserve(k): a block inside which k compute units are reserved; the prior reservation is read first and put back in a
    finally, and that it is back is checked."""
    lib, L = _L()

    @contextlib.contextmanager
    def block(k):
        prior, plan_before = _reserved_now(L), L.srx_plan_cus()
        lib.call('srx_set_reserved_cus', k)
        try:
            assert L.srx_plan_cus() == L.srx_device_cus() - k
            yield
        finally:
            lib.call('srx_set_reserved_cus', prior)
            assert L.srx_plan_cus() == plan_before
    prior, plan_before = _reserved_now(L), L.srx_plan_cus()
    try:
        yield block
    finally:
        lib.call('srx_set_reserved_cus', prior)
        assert L.srx_plan_cus() == plan_before


def _p(t):
    return None if t is None else t.data_ptr()


def _nhwc64(t):
    return t.detach().cpu().double()


def _run(fn):
    """fn under the per-launch records: (what fn returns, the names of the conv kernels it launched), device idle afterwards."""
    holder = []
    names = _launched(lambda: holder.append(fn()))
    torch.cuda.synchronize()
    return holder[0], names


# =============================================================================================================== 1. row tile
C64CH = 64
TABLE_W = 2 * C64CH + 4
SLOPE = 0.25


def _clear_of_zero(y, mean, invstd, gam, beta):
    """Moves the few elements of y whose normalised value z = gamma (y - mean) invstd + beta lies within 1e-3 of 0 to |z| >= 3e-3:
    the backward of PReLU is discontinuous there, and a z that rounds to the other side in fp32 (|error| < 1e-6) would be a
    legitimate difference from fp64 of (1 - slope) x the gradient.  With |z| >= 1e-3 the sign is the same in both."""
    z = (y.double() - mean.double()) * invstd.double() * gam.double() + beta.double()
    near = z.abs() < 1e-3
    shift = (4e-3 / (gam.double() * invstd.double())).expand_as(z)
    y = torch.where(near, (y.double() + shift).float(), y)
    z = (y.double() - mean.double()) * invstd.double() * gam.double() + beta.double()
    assert float(z.abs().min()) > 1e-3
    return y


class RowTile:
    """One 3x3 / 64 -> 64 layer at (N, H, W): operands on the CPU (fp32) and the GPU, packed weights, and the fp64 convolutions
    every test of the shape shares -- computed once, never changed."""

    def __init__(self, n, h, w, dev):
        lib, L = _L()
        c = C64CH
        self.n, self.h, self.w, self.m, self.dev = n, h, w, n * h * w, dev
        g = torch.Generator().manual_seed(4800 + 100 * n + w)
        r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        self.wt, self.bias = r(c, c, 3, 3) * 0.05, r(c) * 0.3
        self.x, self.dy, self.res = r(n, h, w, c), r(n, h, w, c), r(n, h, w, c)
        # two BatchNorm layers' constants: 'a' above the conv (BNL forward / BNB backward), 'b' below it (BNR)
        self.bn = {}
        for tag in 'ab':
            mean, invstd = r(c) * 0.1, torch.rand(c, generator=g) + 0.5
            gam, beta = 1.0 + 0.2 * r(c), r(c) * 0.3
            y = _clear_of_zero(r(n, h, w, c), mean, invstd, gam, beta)
            self.bn[tag] = dict(y=y, mean=mean, invstd=invstd, gamma=gam, beta=beta)
        self.gpu = {k: v.to(dev) for k, v in dict(wt=self.wt, bias=self.bias, x=self.x, dy=self.dy, res=self.res).items()}
        for tag in 'ab':
            self.gpu[tag] = {k: v.to(dev) for k, v in self.bn[tag].items()}
        self.prelu = torch.tensor([SLOPE], device=dev)
        d = self.desc()
        self.wf = torch.empty(L.srx_conv2d_packed_fwd_floats(C.byref(d)), device=dev)
        self.wb = torch.empty(L.srx_conv2d_packed_bwd_floats(C.byref(d)), device=dev)
        lib.call('srx_conv2d_pack', C.byref(d), _p(self.gpu['wt']), _p(self.wf), _p(self.wb), _stream())
        torch.cuda.synchronize()

    def desc(self, act=0, slope=0.0):
        lib, _ = _L()
        return lib.Conv2dDesc(*PF.row_tile_desc(self.n, self.h, self.w, act, slope))

    def conv64(self, x64):
        """fp64 conv of an NHWC tensor (no bias)."""
        y = TF.conv2d(x64.permute(0, 3, 1, 2), self.wt.double(), None, padding=1)
        return y.permute(0, 2, 3, 1).contiguous()

    def dgrad64(self, dy64):
        c = C64CH
        dx = torch.nn.grad.conv2d_input((self.n, c, self.h, self.w), self.wt.double(), dy64.permute(0, 3, 1, 2).contiguous(), padding=1)
        return dx.permute(0, 2, 3, 1).contiguous()

    @functools.cached_property
    def conv_x(self):
        return self.conv64(self.x.double())

    @functools.cached_property
    def dgrad_dy(self):
        return self.dgrad64(self.dy.double())

    def z64(self, tag, y64=None):
        """(xhat, z) of BatchNorm layer `tag` in fp64."""
        b = self.bn[tag]
        xh = ((b['y'].double() if y64 is None else y64) - b['mean'].double()) * b['invstd'].double()
        return xh, xh * b['gamma'].double() + b['beta'].double()

    def fresh(self):
        return torch.full((self.n, self.h, self.w, C64CH), NAN, device=self.dev)

    def name(self, nb, mode=''):
        return f'rt36_conv3x3_c64_kernel<{nb}{mode}> MxNxK={self.m}x64x576'


@functools.lru_cache(maxsize=None)
def _row_tile(n, h, w):
    return RowTile(n, h, w, torch.device('cuda:0'))


def _check_plan_48(lay, d):
    _, L = _L()
    rows = lay.m // PF.ROW_TILE_PIXELS
    for which in (0, 1):
        assert _plan(d, which)[:4] == [48, 64, 1, rows], _plan(d, which)
    assert L.srx_conv2d_stat_rows(C.byref(d)) == rows and L.srx_conv2d_bwd_data_bn_rows(C.byref(d)) == rows
    assert L.srx_conv2d_fwd_ws_floats(C.byref(d)) == 0 and L.srx_conv2d_bwd_data_ws_floats(C.byref(d)) == 0
    return rows


def _blocks(t64, rows):
    """[M or N, H, W][C] fp64 -> per-block sums [rows][C] over blocks of 48 consecutive pixels."""
    return t64.reshape(rows, PF.ROW_TILE_PIXELS, -1).sum(1)


def _within(what, got, ref64, bound):
    err = (got.detach().cpu().double() - ref64).abs()
    print(f'  {what:40s} max |err| / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}')
    assert bool((err <= bound).all()), (what, float((err - bound).max()), float(err.max()))


def _check_stat_table(lay, part, y, rows):
    """The BatchNorm partial table [rows][64][2] of a conv output y (as the kernel stored it, fp32): per block of 48 pixels the
    sums of y and y^2.  The kernel adds a block's 48 values in fp32 in some order: |error| <= gamma(48) sum|y|, and
    gamma(49) sum y^2 with the rounding of each square (test_step_ops_gpu.py's bound for partial sums, k = 48 rows per block)."""
    assert tuple(part.shape) == (rows, C64CH, 2) and not torch.isnan(part).any()
    y64 = _nhwc64(y)
    k = PF.ROW_TILE_PIXELS
    _within('partial sum', part[:, :, 0], _blocks(y64, rows), gamma(k) * _blocks(y64.abs(), rows))
    _within('partial sum of squares', part[:, :, 1], _blocks(y64 * y64, rows), gamma(k + 1) * _blocks(y64 * y64, rows))


def _bn_bwd64(lay, tag, dout64, prelu):
    """fp64 backward of BatchNorm (+ PReLU) layer `tag` for the output gradient dout64: dz, xhat, z and the per-channel sums."""
    xh, z = lay.z64(tag)
    dz = dout64 * torch.where(z > 0, 1.0, SLOPE) if prelu else dout64
    return dz, xh, z


def _check_bnr_table(lay, table, dx, rows, prelu):
    """Table of the BNR epilogue against fp64 per-block sums formed from the kernel's own dx (fp32, exact in fp64): columns
    [0, C) sum dz, [C, 2C) sum dz xhat, 2C + 2C+1 the PReLU slope partial sum(dx z over z <= 0).  fp32 chains of at most 48
    terms; a term carries up to 4 roundings of its own (xhat: 2, z: 2 / the product: 1)."""
    c = C64CH
    assert torch.isfinite(table[:, :2 * c + 2]).all()
    dz, xh, z = _bn_bwd64(lay, 'b', _nhwc64(dx), prelu)
    k = PF.ROW_TILE_PIXELS + 4
    _within('table sum dz', table[:, :c], _blocks(dz, rows), gamma(k) * _blocks(dz.abs(), rows))
    _within('table sum dz xhat', table[:, c:2 * c], _blocks(dz * xh, rows), gamma(k) * _blocks((dz * xh).abs(), rows))
    if prelu:
        t = torch.where(z > 0, 0.0, _nhwc64(dx) * z)
        want, mag = _blocks(t, rows).sum(1), _blocks(t.abs(), rows).sum(1)
        # (a lane adds up to 32 terms, its wave's 64 lanes are folded, the two waves' columns are added here: no chain of more
        # than 32 + 63 + 1 fp32 additions, and the 4 roundings of a term)
        _within('table prelu partial', table[:, 2 * c] + table[:, 2 * c + 1], want, gamma(100) * mag)


@pytest.mark.parametrize('n,h,w,nb,k', PF.ROW_TILE_48)
def test_row_tile_48_forward(dev, reserve, n, h, w, nb, k):
    """srx_conv2d_fwd with bias + LeakyReLU, with the BatchNorm partial table, and srx_conv2d_fwd_residual: RT48, plain mode."""
    lib, _ = _L()
    lay, s = _row_tile(n, h, w), _stream()
    G = lay.gpu
    with reserve(k):
        d_act, d_lin = lay.desc(lib.ACT_LRELU, 0.2), lay.desc()
        rows = _check_plan_48(lay, d_lin)
        y_act, y_lin, y_res = lay.fresh(), lay.fresh(), lay.fresh()
        part = torch.full((rows, C64CH, 2), NAN, device=dev)
        _, n1 = _run(lambda: lib.call('srx_conv2d_fwd', C.byref(d_act), _p(G['x']), _p(lay.wf), _p(G['bias']), _p(y_act), None, None, 0, s))
        _, n2 = _run(lambda: lib.call('srx_conv2d_fwd', C.byref(d_lin), _p(G['x']), _p(lay.wf), _p(G['bias']), _p(y_lin), _p(part), None, 0, s))
        _, n3 = _run(lambda: lib.call('srx_conv2d_fwd_residual', C.byref(d_act), _p(G['x']), _p(lay.wf), _p(G['bias']), _p(G['res']), 1.0,
                                      _p(y_res), None, 0, s))
    assert n1 == n2 == n3 == [lay.name(nb)], (n1, n2, n3)
    pre = lay.conv_x + lay.bias.double()
    act = torch.where(pre > 0, pre, pre * 0.2)
    for what, got, want in (('bias + lrelu', y_act, act), ('bias', y_lin, pre), ('residual', y_res, act + lay.res.double())):
        assert not torch.isnan(got).any(), what
        err = rel_err(got, want)
        print(f'  {what}: rel err {err:.3g}')
        assert err < 1e-5, (what, err)
    _check_stat_table(lay, part, y_lin, rows)


@pytest.mark.parametrize('prelu', [True, False])
@pytest.mark.parametrize('n,h,w,nb,k', PF.ROW_TILE_48)
def test_row_tile_48_forward_with_batchnorm_on_its_input(dev, reserve, n, h, w, nb, k, prelu):
    """srx_conv2d_fwd_bn_in (BNL): normalise + PReLU, or normalise + skip addend, while the patch is staged.  Bit for bit the
    separate launches (srx_bn_act_fwd, srx_conv2d_fwd: both plan 48 pixels here) and fp64 to 1e-5 -- the bounds of
    test_ops_gpu.py::test_forward_conv_with_batchnorm_on_its_input."""
    lib, L = _L()
    lay, s = _row_tile(n, h, w), _stream()
    G, A = lay.gpu, lay.gpu['a']
    act = lib.ACT_PRELU if prelu else lib.ACT_NONE
    sp = _p(lay.prelu) if prelu else None
    res = None if prelu else G['res']
    with reserve(k):
        d = lay.desc()
        rows = _check_plan_48(lay, d)
        assert L.srx_conv2d_fwd_bn_in_ok(C.byref(d)) == 1
        a0, y0, part0 = lay.fresh(), lay.fresh(), torch.full((rows, C64CH, 2), NAN, device=dev)
        lib.call('srx_bn_act_fwd', _p(A['y']), _p(A['mean']), _p(A['invstd']), _p(A['gamma']), _p(A['beta']), _p(res), _p(a0), lay.m,
                 C64CH, act, 0.0, sp, s)
        _, n0 = _run(lambda: lib.call('srx_conv2d_fwd', C.byref(d), _p(a0), _p(lay.wf), _p(G['bias']), _p(y0), _p(part0), None, 0, s))
        a1, y1, part1 = lay.fresh(), lay.fresh(), torch.full((rows, C64CH, 2), NAN, device=dev)
        _, n1 = _run(lambda: lib.call('srx_conv2d_fwd_bn_in', C.byref(d), _p(A['y']), _p(A['mean']), _p(A['invstd']), _p(A['gamma']),
                                      _p(A['beta']), sp, _p(res), _p(a1), _p(lay.wf), _p(G['bias']), _p(y1), _p(part1), s))
    assert n0 == [lay.name(nb)] and n1 == [lay.name(nb, ', BNL')], (n0, n1)
    assert not torch.isnan(a1).any() and not torch.isnan(y1).any()
    assert torch.equal(a0, a1) and torch.equal(y0, y1) and torch.equal(part0, part1)
    _, z = lay.z64('a')
    ref_a = torch.where(z > 0, z, z * SLOPE) if prelu else z + lay.res.double()
    ref_y = lay.conv64(ref_a) + lay.bias.double()
    ea, ey = rel_err(a1, ref_a), rel_err(y1, ref_y)
    print(f'  act_out rel err {ea:.3g}, y rel err {ey:.3g}')
    assert ea < 1e-5 and ey < 1e-5, (ea, ey)
    _check_stat_table(lay, part1, y1, rows)


@pytest.mark.parametrize('n,h,w,nb,k', PF.ROW_TILE_48)
def test_row_tile_48_data_gradient(dev, reserve, n, h, w, nb, k):
    """srx_conv2d_bwd_data and srx_conv2d_bwd_data_add: RT48, plain mode, the addend in the epilogue."""
    lib, _ = _L()
    lay, s = _row_tile(n, h, w), _stream()
    G = lay.gpu
    with reserve(k):
        d = lay.desc()
        _check_plan_48(lay, d)
        dx0, dx1 = lay.fresh(), lay.fresh()
        _, n0 = _run(lambda: lib.call('srx_conv2d_bwd_data', C.byref(d), _p(G['dy']), _p(lay.wb), _p(dx0), 0, None, 0, s))
        _, n1 = _run(lambda: lib.call('srx_conv2d_bwd_data_add', C.byref(d), _p(G['dy']), _p(lay.wb), _p(G['res']), _p(dx1), None, 0, s))
    assert n0 == n1 == [lay.name(nb)], (n0, n1)
    for what, got, want in (('dx', dx0, lay.dgrad_dy), ('dx + addend', dx1, lay.dgrad_dy + lay.res.double())):
        assert not torch.isnan(got).any(), what
        err = rel_err(got, want)
        print(f'  {what}: rel err {err:.3g}')
        assert err < 1e-5, (what, err)


def _finish(lay, dx, table, rows, prelu):
    """srx_bn_act_bwd_finish on a BNR table: (sums, dy, dgamma, dbeta, dprelu), all NaN / zero before."""
    lib, _ = _L()
    B = lay.gpu['b']
    c, dev = C64CH, lay.dev
    sums, out = torch.full((TABLE_W,), NAN, device=dev), lay.fresh()
    gg, gb, gp = torch.zeros(c, device=dev), torch.zeros(c, device=dev), torch.zeros(1, device=dev)
    lib.call('srx_bn_act_bwd_finish', _p(dx), _p(B['y']), _p(B['mean']), _p(B['invstd']), _p(B['gamma']), _p(B['beta']), _p(table), rows, 2,
             _p(sums), _p(out), lay.m, c, lib.ACT_PRELU if prelu else lib.ACT_NONE, 0.0, _p(lay.prelu) if prelu else None,
             _p(gg), _p(gb), _p(gp) if prelu else None, _stream())
    torch.cuda.synchronize()
    return sums, out, gg, gb, gp


def _check_finish(lay, dx, got, prelu):
    """The finished BatchNorm backward below the conv against fp64 of the srx.h formulas, from the kernel's own dx."""
    sums, out, gg, gb, gp = got
    c, m = C64CH, lay.m
    b = lay.bn['b']
    dz, xh, z = _bn_bwd64(lay, 'b', _nhwc64(dx), prelu)
    s1, s2 = dz.reshape(m, c).sum(0), (dz * xh).reshape(m, c).sum(0)
    dy = b['gamma'].double() * b['invstd'].double() * (dz - s1 / m - xh * s2 / m)
    errs = dict(sum_dz=rel_err(sums[:c], s1), sum_dz_xhat=rel_err(sums[c:2 * c], s2), dy=rel_err(out, dy), dgamma=rel_err(gg, s2),
                dbeta=rel_err(gb, s1))
    print('  finish: ' + ', '.join(f'{k} {v:.3g}' for k, v in errs.items()))
    assert not torch.isnan(out).any() and all(v < 1e-5 for v in errs.values()), errs
    if prelu:
        want = float(torch.where(z > 0, 0.0, _nhwc64(dx) * z).sum())
        assert abs(gp.item() - want) <= 1e-5 * max(abs(want), 1.0), (gp.item(), want)
        assert abs(sums[2 * c].item() - want) <= 1e-5 * max(abs(want), 1.0), (sums[2 * c].item(), want)


@pytest.mark.parametrize('prelu', [True, False])
@pytest.mark.parametrize('n,h,w,nb,k', PF.ROW_TILE_48)
def test_row_tile_48_data_gradient_with_bn_backward_reduce_epilogue(dev, reserve, n, h, w, nb, k, prelu):
    """srx_conv2d_bwd_data_bn (BNR) + srx_bn_act_bwd_finish, without and with an addend: dx bit for bit the plain data gradient's
    (same kernel body, both at 48 pixels) and within 1e-5 of fp64; the table per 48-pixel block and the finished sums, dy and
    parameter gradients against fp64 (test_ops_gpu.py::test_data_gradient_with_bn_backward_reduce_epilogue's bounds)."""
    lib, _ = _L()
    lay, s = _row_tile(n, h, w), _stream()
    G, B = lay.gpu, lay.gpu['b']
    sp = _p(lay.prelu) if prelu else None
    for add, want in ((None, lay.dgrad_dy), (G['res'], lay.dgrad_dy + lay.res.double())):
        with reserve(k):
            d = lay.desc()
            rows = _check_plan_48(lay, d)
            dx0, dx1 = lay.fresh(), lay.fresh()
            if add is None:
                lib.call('srx_conv2d_bwd_data', C.byref(d), _p(G['dy']), _p(lay.wb), _p(dx0), 0, None, 0, s)
            else:
                lib.call('srx_conv2d_bwd_data_add', C.byref(d), _p(G['dy']), _p(lay.wb), _p(add), _p(dx0), None, 0, s)
            table = torch.full((rows, TABLE_W), NAN, device=dev)
            _, names = _run(lambda: lib.call('srx_conv2d_bwd_data_bn', C.byref(d), _p(G['dy']), _p(lay.wb), _p(add), _p(dx1), _p(B['y']),
                                             _p(B['mean']), _p(B['invstd']), _p(B['gamma']), _p(B['beta']), sp, _p(table), s))
            got = _finish(lay, dx1, table, rows, prelu)
        assert names == [lay.name(nb, ', BNR')], names
        assert not torch.isnan(dx1).any() and torch.equal(dx0, dx1)
        err = rel_err(dx1, want)
        print(f'  addend {add is not None}: dx rel err {err:.3g}')
        assert err < 1e-5, err
        _check_bnr_table(lay, table, dx1, rows, prelu)
        _check_finish(lay, dx1, got, prelu)


@pytest.mark.parametrize('prelu', [True, False])
@pytest.mark.parametrize('below', [True, False])
@pytest.mark.parametrize('n,h,w,nb,k', PF.ROW_TILE_48)
def test_row_tile_48_data_gradient_with_batchnorm_backward_on_its_input(dev, reserve, n, h, w, nb, k, below, prelu):
    """srx_conv2d_bwd_data_bn_in (BNB, and BNR + BNB with a BatchNorm below): the apply pass of the BatchNorm (+ PReLU) backward
    above the conv while the patch is staged, dy written on the side, against fp64 of the srx.h formulas at the bounds of
    test_ops_gpu.py::test_data_gradient_with_batchnorm_backward_on_its_input (dy 2e-6, dx and the sums 1e-5)."""
    lib, L = _L()
    lay, s = _row_tile(n, h, w), _stream()
    G, A, B = lay.gpu, lay.gpu['a'], lay.gpu['b']
    c, m = C64CH, lay.m
    sp = _p(lay.prelu) if prelu else None
    # the layer above in fp64; its finalised sums are an operand (fp32, as srx_bn_act_bwd_finish(dy = NULL) leaves them)
    a = lay.bn['a']
    dz, xh, _ = _bn_bwd64(lay, 'a', lay.dy.double(), prelu)
    sums = torch.zeros(TABLE_W)
    sums[:c], sums[c:2 * c] = dz.reshape(m, c).sum(0).float(), (dz * xh).reshape(m, c).sum(0).float()
    s1, s2 = sums[:c].double(), sums[c:2 * c].double()
    ref_dy = a['gamma'].double() * a['invstd'].double() * (dz - s1 / m - xh * s2 / m)
    ref_dx = lay.dgrad64(ref_dy) + lay.res.double()
    sums_g = sums.to(dev)
    bp = (lambda t: _p(t)) if below else (lambda t: None)
    with reserve(k):
        d = lay.desc()
        rows = _check_plan_48(lay, d)
        assert L.srx_conv2d_bwd_data_bn_in_ok(C.byref(d)) == 1
        dy1, dx1 = lay.fresh(), lay.fresh()
        table = torch.full((rows, TABLE_W), NAN, device=dev)
        _, names = _run(lambda: lib.call(
            'srx_conv2d_bwd_data_bn_in', C.byref(d), _p(G['dy']), _p(A['y']), _p(A['mean']), _p(A['invstd']), _p(A['gamma']), _p(A['beta']),
            sp, _p(sums_g), _p(dy1), _p(lay.wb), _p(G['res']), _p(dx1), bp(B['y']), bp(B['mean']), bp(B['invstd']), bp(B['gamma']),
            bp(B['beta']), None, bp(table), s))
        got = _finish(lay, dx1, table, rows, False) if below else None
    assert names == [lay.name(nb, ', BNR, BNB' if below else ', BNB')], names
    assert not torch.isnan(dy1).any() and not torch.isnan(dx1).any()   # every pixel written, by the workgroup that owns it
    e_dy, e_dx = rel_err(dy1, ref_dy), rel_err(dx1, ref_dx)
    print(f'  dy rel err {e_dy:.3g}, dx rel err {e_dx:.3g}')
    assert e_dy < 2e-6 and e_dx < 1e-5, (e_dy, e_dx)
    if below:
        _check_bnr_table(lay, table, dx1, rows, False)
        _check_finish(lay, dx1, got, False)
    else:
        assert torch.isnan(table).all()   # no BatchNorm below: the table is not touched


# ==================================================================================================== 2. persistent kernels
def _c64_items(n, h, w, cout):
    """(items, workgroups along x) of the launch srx_conv3x3_c64_*_fwd makes now."""
    _, L = _L()
    out = (C.c_int * 3)()
    assert L.srx_conv3x3_c64_bf16_plan(n, h, w, cout, out) == 0
    return list(out), n * out[1] * out[2], max(1, L.srx_plan_cus() // (cout // 64))


def _c64_slopes(cout, g):
    """One slope per output channel, random in (-0.5, 1.5) with 0, -0.7, 0.25 and 1.5 among them; no two alike, so that a swapped
    channel (half, group) shows."""
    a = torch.rand(cout, generator=g) * 2 - 0.5
    a[:4] = torch.tensor([0.0, -0.7, 0.25, 1.5])
    assert a.unique().numel() == cout and float(a.min()) >= -0.7 and float(a.max()) <= 1.5
    return a


def _c64_check(dev, f16, n, h, w, cout, shuffle, res):
    """srx_conv3x3_c64_{bf16,f16}_fwd against fp64 of the same (rounded) operands, at the bounds of test_ops_gpu.py::
    test_bf16_native_conv3x3_c64 / test_fp16_inference_gpu.py::test_fp16_conv3x3_c64: one rounding of the fp32 sum -- half a bf16
    ulp (2^-8 relative) or half an fp16 ulp (2^-11) -- plus the fp32 sum's floor."""
    lib, L = _L()
    s = _stream()
    dt = torch.float16 if f16 else torch.bfloat16
    tag = 'f16' if f16 else 'bf16'
    g = torch.Generator().manual_seed(1000 * h + w + cout + n + (7 if f16 else 0))
    x = (torch.rand(n, 64, h, w, generator=g) - 0.5).to(dt)
    wt = torch.randn(cout, 64, 3, 3, generator=g) * (2.0 / 576) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    slope = 0.25
    oh, ow, oc = (2 * h, 2 * w, 64) if shuffle else (h, w, cout)
    skip = (torch.rand(n, oc, oh, ow, generator=g) - 0.5).to(dt) if res else None
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    wd, bd = wt.to(dev), b.to(dev)
    pk = torch.empty(getattr(L, f'srx_conv3x3_c64_{tag}_packed_bytes')(cout), dtype=torch.uint8, device=dev)
    lib.call(f'srx_conv3x3_c64_{tag}_pack', _p(wd), _p(bd), None, cout, shuffle, _p(pk), s)
    y = torch.full((n, oh, ow, oc), NAN, dtype=dt, device=dev)
    sd = None if skip is None else skip.permute(0, 2, 3, 1).contiguous().to(dev)
    _, names = _run(lambda: lib.call(f'srx_conv3x3_c64_{tag}_fwd', n, h, w, cout, shuffle, _p(xd), _p(pk), slope, _p(sd), _p(y), oc, s))
    rw, cw = (4, 1) if w <= 32 else ((2, 2) if w <= 64 else (1, 4))
    assert names == [f'c64_{tag}_kernel<{rw}, {cw}> MxNxK={n * h * w}x{cout}x576'], names
    z = TF.conv2d(x.double(), wt.to(dt).double(), b.double(), 1, 1)
    if shuffle:
        z = TF.pixel_shuffle(z, 2)
    z = torch.where(z > 0, z, z * slope)
    if skip is not None:
        z = z + skip.double()
    got = y.permute(0, 3, 1, 2).float().cpu().double()
    assert torch.isfinite(got).all()
    err = (got - z).abs()
    bound = z.abs() * U16 + 2e-5 * z.abs().max() if f16 else z.abs() * (2.0 ** -8 * 1.001) + 2e-6 * z.abs().max()
    print(f'  c64 {tag} {(n, h, w, cout)}: max err / bound {float((err / bound).max()):.3f}')
    assert (err <= bound).all(), ((err - bound).max().item(), err.max().item())
    same = (z.float().to(dt).double() == got).double().mean().item()   # ... and it IS the rounding of the right value
    assert same > 0.995, same


@pytest.mark.parametrize('f16', [False, True], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('case', PF.C64_MULTI_ITEM, ids=PF.by_id(PF.C64_MULTI_ITEM))
def test_c64_workgroups_walk_several_items(dev, case, f16):
    """More (image, strip, chunk) items than workgroups: every workgroup restarts its LDS row ring and prologue for a second item
    with the weights still in registers, the epilogue of one item's last rows overlapping the next item's first loads."""
    n, h, w = case['shape']
    plan, items, grid = _c64_items(n, h, w, case['cout'])
    assert items > grid and plan[1] >= case['min_chunks'] and plan[2] >= case['min_strips'], (plan, items, grid)
    _c64_check(dev, f16, n, h, w, case['cout'], case['shuffle'], case['res'])


_SLOPES_SEEN = set()   # the c64_*_slopes_kernel instantiations this module's launches recorded


def _c64_slopes_check(dev, f16, n, h, w, cout, res, form):
    """srx_conv3x3_c64_{bf16,f16}_fwd_slopes (c64_{bf16,f16}_slopes_kernel<RW, CW>: PC = true, one PReLU slope per output channel)
    against fp64 of the same (rounded) operands at _c64_check's bounds -- half a bf16 ulp x 1.001 + 2e-6 of the range, or half an
    fp16 ulp + 2e-5 of it, and more than 99.5 % of the values the rounding of the right one.  With all slopes equal to 0.25, -0.5
    and 1.0 -- the scalar kernel's three activation forms -- the result is the scalar entry point's, bit for bit."""
    lib, L = _L()
    s = _stream()
    dt = torch.float16 if f16 else torch.bfloat16
    tag = 'f16' if f16 else 'bf16'
    g = torch.Generator().manual_seed(2000 * h + w + cout + n + (7 if f16 else 0))
    x = (torch.rand(n, 64, h, w, generator=g) - 0.5).to(dt)
    wt = torch.randn(cout, 64, 3, 3, generator=g) * (2.0 / 576) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    a = _c64_slopes(cout, g)
    skip = (torch.rand(n, cout, h, w, generator=g) - 0.5).to(dt) if res else None
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    wd, bd = wt.to(dev), b.to(dev)
    pk = torch.empty(getattr(L, f'srx_conv3x3_c64_{tag}_packed_bytes')(cout), dtype=torch.uint8, device=dev)
    lib.call(f'srx_conv3x3_c64_{tag}_pack', _p(wd), _p(bd), None, cout, 0, _p(pk), s)
    sd = None if skip is None else skip.permute(0, 2, 3, 1).contiguous().to(dev)

    def run(sl):
        y = torch.full((n, h, w, cout), NAN, dtype=dt, device=dev)
        lib.call(f'srx_conv3x3_c64_{tag}_fwd_slopes', n, h, w, cout, 0, _p(xd), _p(pk), _p(sl), _p(sd), _p(y), cout, s)
        return y

    ad = a.to(dev)
    y, names = _run(lambda: run(ad))
    rw, cw = form
    assert names == [f'c64_{tag}_slopes_kernel<{rw}, {cw}> MxNxK={n * h * w}x{cout}x576'], names
    _SLOPES_SEEN.add(names[0].split(' MxNxK=')[0])
    z = TF.conv2d(x.double(), wt.to(dt).double(), b.double(), 1, 1)
    z = torch.where(z > 0, z, z * a.double().view(1, -1, 1, 1))
    if skip is not None:
        z = z + skip.double()
    got = y.permute(0, 3, 1, 2).float().cpu().double()
    assert torch.isfinite(got).all()
    err = (got - z).abs()
    bound = z.abs() * U16 + 2e-5 * z.abs().max() if f16 else z.abs() * (2.0 ** -8 * 1.001) + 2e-6 * z.abs().max()
    same = (z.float().to(dt).double() == got).double().mean().item()   # ... and it IS the rounding of the right value
    print(f'  c64 slopes {tag} {(n, h, w, cout)} <{rw}, {cw}>: max err / bound {float((err / bound).max()):.3f}, same {same:.5f}')
    assert (err <= bound).all(), ((err - bound).max().item(), err.max().item())
    assert same > 0.995, same
    for v in (0.25, -0.5, 1.0):
        ys = torch.full((n, h, w, cout), NAN, dtype=dt, device=dev)
        lib.call(f'srx_conv3x3_c64_{tag}_fwd', n, h, w, cout, 0, _p(xd), _p(pk), v, _p(sd), _p(ys), cout, s)
        yv = run(torch.full((cout,), v, device=dev))
        torch.cuda.synchronize()
        assert not torch.isnan(ys).any() and torch.equal(yv.view(torch.int16), ys.view(torch.int16)), v


@pytest.mark.parametrize('f16', [False, True], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('case', PF.C64_SLOPES, ids=PF.by_id(PF.C64_SLOPES))
def test_c64_per_channel_slopes_in_every_tile_form(dev, case, f16):
    """The PC = true instantiations <4, 1>, <2, 2> and <1, 4> in both types: frames wider than 64 pixels, odd rows, ragged strips,
    two channel groups (the slopes 64..127 must reach group 1), and workgroups that walk several items with the slopes kept in
    registers across them."""
    n, h, w = case['shape']
    plan, items, grid = _c64_items(n, h, w, case['cout'])
    assert (items > grid) == case['multi'], (plan, items, grid)
    _c64_slopes_check(dev, f16, n, h, w, case['cout'], case['res'], case['form'])


def test_zz_every_slopes_kernel_instantiation_ran(dev):
    """All six c64_{bf16,f16}_slopes_kernel<RW, CW> names were recorded (cases this process has not run yet run here)."""
    want = {f'c64_{tag}_slopes_kernel<{rw}, {cw}>' for tag in ('bf16', 'f16') for rw, cw in PF.C64_SLOPES_FORMS}
    for f16 in (False, True):
        for form in PF.C64_SLOPES_FORMS:
            if f'c64_{"f16" if f16 else "bf16"}_slopes_kernel<{form[0]}, {form[1]}>' not in _SLOPES_SEEN:
                case = next(c for c in sorted(PF.C64_SLOPES, key=lambda c: c['multi']) if c['form'] == form)
                _c64_slopes_check(dev, f16, *case['shape'], case['cout'], case['res'], form)
    print('  c64 slopes kernels recorded:', sorted(_SLOPES_SEEN))
    assert _SLOPES_SEEN == want and len(want) == 6


def _thin9_check(dev, f16, n, h, w, cout):
    """srx_conv9x9_c64_thin_{bf16,f16}_fwd against fp64 of the rounded operands: 2e-5 of the tensor's maximum, channels >= Cout
    exactly 0 (test_ops_gpu.py::test_bf16_output_conv_with_taps_as_gemm_columns, test_fp16_inference_gpu.py::
    test_fp16_output_conv_thin9)."""
    lib, L = _L()
    s = _stream()
    dt = torch.float16 if f16 else torch.bfloat16
    tag = 'f16' if f16 else 'bf16'
    g = torch.Generator().manual_seed(7 * h + w + n + (1 if f16 else 0))
    x = (torch.rand(n, 64, h, w, generator=g) - 0.5).to(dt)
    wt = torch.randn(cout, 64, 9, 9, generator=g) * (1.0 / 5184) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    wd, bd = wt.to(dev), b.to(dev)
    pk = torch.empty(getattr(L, f'srx_conv9x9_c64_thin_{tag}_packed_bytes')(), dtype=torch.uint8, device=dev)
    lib.call(f'srx_conv9x9_c64_thin_{tag}_pack', _p(wd), _p(bd), cout, _p(pk), s)
    y = torch.full((n, h, w, 4), NAN, device=dev)
    _, names = _run(lambda: lib.call(f'srx_conv9x9_c64_thin_{tag}_fwd', n, h, w, _p(xd), _p(pk), _p(y), s))
    assert names == [f't9_{tag}_kernel MxNxK={n * h * w}x3x5184'], names
    z = TF.conv2d(x.double(), wt.to(dt).double(), b.double(), 1, 4)
    got = y.permute(0, 3, 1, 2).cpu().double()
    assert torch.isfinite(got).all()
    err = ((got[:, :cout] - z).abs().max() / z.abs().max()).item()
    print(f'  thin9 {tag} {(n, h, w, cout)}: rel err {err:.3g}')
    assert err < 2e-5, err
    assert float(got[:, cout:].abs().max()) == 0.0


@pytest.mark.parametrize('f16', [False, True], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('n,h,w,cout', PF.THIN9_MULTI_ITEM + PF.THIN9_OTHER)
def test_thin9_workgroups_walk_several_items(dev, n, h, w, cout, f16):
    """More column strips than workgroups (plan_forms.THIN9_MULTI_ITEM): the output-row ring and the input window start over for
    every further item of a workgroup.  (THIN9_OTHER: 130 strips, one item per workgroup -- see plan_forms.py.)"""
    _, L = _L()
    if (n, h, w, cout) in PF.THIN9_MULTI_ITEM:
        assert n * -(-w // PF.THIN9_STRIP) > L.srx_plan_cus()
    _thin9_check(dev, f16, n, h, w, cout)


# =============================================================================================== 3. plans under a reservation
def _gconv_name(plan, prec):
    bm, bn, _, _, ks, _ = plan
    head, _, wm, wn, xr = _tile_args(bm, bn)
    if bm == 256:
        wn = 64
    return f'gconv_kernel<{head}, {bn}, {wm}, {wn}, {ks}, {xr}, {prec}>'


@pytest.mark.parametrize('case', PF.RESERVED_GCONV, ids=PF.by_id(PF.RESERVED_GCONV))
def test_reserved_plans_of_single_launch_convs(dev, reserve, case):
    """Forward / data gradient on gconv_kernel with the tail split, tile and workgroup count a reservation produces: the plan, the
    launch and the numbers against fp64 (of bf16-rounded operands at precision 1) at test_forced_paths_gpu.py's 1e-5.  The split
    tail's partial sums go through the workspace, which starts as NaN like the output."""
    lib, L = _L()
    s = _stream()
    d = lib.Conv2dDesc(*case['desc'])
    n, h, w, cin, cin_s, cout, cout_s, k, prec, which = d.N, d.H, d.W, d.Cin, d.Cin_s, d.Cout, d.Cout_s, d.KH, d.precision, case['which']
    g = torch.Generator().manual_seed(n * 1000 + h * 37 + cin + 3 * cout + case['k'])
    wt = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.3
    x = torch.randn(n, h, w, cin_s, generator=g) * 1.5       # (channels past Cin: someone else's, never read into the result)
    dy = torch.randn(n, h, w, cout_s, generator=g)
    r = (lambda t: t.bfloat16().double()) if prec else (lambda t: t.double())
    if which == 0:
        ref = TF.conv2d(r(x[..., :cin].permute(0, 3, 1, 2)), r(wt), bias.double(), padding=k // 2)
    else:
        ref = torch.nn.grad.conv2d_input((n, cin, h, w), r(wt), r(dy[..., :cout].permute(0, 3, 1, 2)), padding=k // 2)
    ref = ref.permute(0, 2, 3, 1)
    xg, dyg, wg, bg = x.to(dev), dy.to(dev), wt.to(dev), bias.to(dev)
    with reserve(case['k']):
        wf = torch.empty(max(L.srx_conv2d_packed_fwd_floats(C.byref(d)), 4), device=dev)
        wb = torch.empty(max(L.srx_conv2d_packed_bwd_floats(C.byref(d)), 4), device=dev)
        lib.call('srx_conv2d_pack', C.byref(d), _p(wg), _p(wf), _p(wb), s)
        need = (L.srx_conv2d_bwd_data_ws_floats if which else L.srx_conv2d_fwd_ws_floats)(C.byref(d))
        plan = _plan(d, which)
        ws = torch.full((max(need, 4),), NAN, device=dev)
        if which == 0:
            out, live = torch.full((n, h, w, cout_s), NAN, device=dev), cout
            _, names = _run(lambda: lib.call('srx_conv2d_fwd', C.byref(d), _p(xg), _p(wf), _p(bg), _p(out), None, _p(ws), need, s))
        else:
            out, live = torch.full((n, h, w, cin_s), NAN, device=dev), cin
            out[..., (cin + 3) // 4 * 4:] = SENTINEL   # channels past Cin's last quad belong to someone else
            _, names = _run(lambda: lib.call('srx_conv2d_bwd_data', C.byref(d), _p(dyg), _p(wb), _p(out), 0, _p(ws), need, s))
    assert plan == case['plan'], (plan, case['plan'])
    bm, bn = plan[:2]
    assert need > 0 and need % (bm * bn) == 0, need   # whole tiles of partial sums: the tail of the last round, cut `split` ways
    assert len(names) == 1 and names[0].startswith(_gconv_name(plan, prec) + ' MxNxK='), (names, _gconv_name(plan, prec))
    assert not torch.isnan(out).any()
    quad = (live + 3) // 4 * 4
    if quad > live:
        assert float(out[..., live:quad].abs().max()) == 0.0   # the rest of the last channel quad is written as 0
    assert bool((out[..., quad:] == SENTINEL).all())
    err = rel_err(out[..., :live], ref)
    print(f'  {case["id"]}: plan {plan} ws {need} rel err {err:.3g}')
    assert err < 1e-5, err


@pytest.mark.parametrize('case', PF.RESERVED_WINO, ids=PF.by_id(PF.RESERVED_WINO))
def test_reserved_plans_of_winograd(dev, reserve, case):
    """Winograd forward (bias + ReLU) and masked data gradient under the plan a reservation produces -- 32-column workgroups, no
    channel split, no workspace, where the free chip runs 64 columns split three ways -- against fp64 at test_wino_gpu.py's 2e-5."""
    lib, L = _L()
    s = _stream()
    n, h, w, cin, _, cout = case['desc'][:6]
    d = lib.Conv2dDesc(*(case['desc'][:12] + (lib.ACT_RELU,) + case['desc'][13:]))
    dref = C.byref(d)
    g = torch.Generator().manual_seed(11 + case['k'])
    x = torch.randn(n, cin, h, w, generator=g).relu()
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    bias = torch.randn(cout, generator=g) * 0.1
    dy = torch.randn(n, cout, h, w, generator=g)
    yr = TF.relu(TF.conv2d(x.double(), wt.double(), bias.double(), padding=1))
    dxr = torch.nn.grad.conv2d_input((n, cin, h, w), wt.double(), dy.double(), padding=1) * (x.double() > 0)
    xg, dyg = x.permute(0, 2, 3, 1).contiguous().to(dev), dy.permute(0, 2, 3, 1).contiguous().to(dev)
    wg, bg = wt.to(dev), bias.to(dev)
    plan = (C.c_int * 6)()
    with reserve(case['k']):
        nf = L.srx_wino_packed_floats(dref)
        uf, ub = torch.empty(nf, device=dev), torch.empty(nf, device=dev)
        lib.call('srx_wino_pack', dref, _p(wg), _p(uf), 0, s)
        lib.call('srx_wino_pack', dref, _p(wg), _p(ub), 1, s)
        got = []
        for which in (0, 1):
            lib.call('srx_wino_plan', dref, which, plan)
            nws = L.srx_wino_ws_floats(dref, which)
            assert list(plan) == case['plan'] and nws == case['ws'], (which, list(plan), nws)
            ws = torch.full((max(nws, 4),), NAN, device=dev)
            out = torch.full((n, h, w, cout if which == 0 else cin), NAN, device=dev)
            if which == 0:
                _, names = _run(lambda: lib.call('srx_wino_fwd', dref, _p(xg), _p(uf), _p(bg), _p(out), _p(ws), nws, s))
            else:
                _, names = _run(lambda: lib.call('srx_wino_bwd_data', dref, _p(dyg), _p(ub), _p(xg), _p(out), _p(ws), nws, s))
            assert names == [f'wino_kernel<{case["plan"][0]}> MxNxK={n * h * w}x{cout if which == 0 else cin}x{9 * (cin if which == 0 else cout)}'], names
            got.append(out)
    for what, out, want in (('y', got[0], yr), ('dx', got[1], dxr)):
        assert not torch.isnan(out).any(), what
        err = rel_err(out.permute(0, 3, 1, 2), want)
        print(f'  {case["id"]} {what}: rel err {err:.3g}')
        assert err < 2e-5, (what, err)


@pytest.mark.parametrize('f16', [False, True], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('case', PF.RESERVED_C64, ids=PF.by_id(PF.RESERVED_C64))
def test_reserved_chunk_geometry_of_c64(dev, reserve, case, f16):
    """The 16-bit inference conv with the chunk geometry a reservation produces (75 chunks of 4 rows on 192 workgroups where
    the free chip cuts 100 of 3 on 256), at the bounds of the persistent cases above."""
    n, h, w = case['shape']
    with reserve(case['k']):
        plan, _, grid = _c64_items(n, h, w, case['cout'])
        assert plan == case['plan'] and grid == (PF.CUS - case['k']) // (case['cout'] // 64), (plan, grid)
        _c64_check(dev, f16, n, h, w, case['cout'], 0, True)


@pytest.mark.parametrize('case', PF.RESERVED_WGRAD, ids=PF.by_id(PF.RESERVED_WGRAD))
def test_reserved_row_splits_of_weight_gradients(dev, reserve, case):
    """srx_conv2d_bwd_weight_multi (two problems, a gradient each, bias gradients riding along) with the row splits a reservation
    produces -- the workspace size says which -- against fp64 at test_forced_paths_gpu.py's 2e-4, into NaN-free gradients only if
    every split's slab is written and reduced (the workspace starts as NaN)."""
    lib, L = _L()
    s = _stream()
    d = lib.Conv2dDesc(*case['desc'])
    n, h, w, cin, cout, k, nprob = d.N, d.H, d.W, d.Cin, d.Cout, d.KH, case['nprob']
    g = torch.Generator().manual_seed(n + h * 7 + w * 13 + cout + case['k'])
    xs = [torch.randn(n, h, w, cin, generator=g) for _ in range(nprob)]
    dys = [torch.randn(n, h, w, cout, generator=g) for _ in range(nprob)]
    want_w = [torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2).double(), (cout, cin, k, k), dy.permute(0, 3, 1, 2).double(), padding=k // 2)
              for x, dy in zip(xs, dys)]
    want_b = [dy.double().sum((0, 1, 2)) for dy in dys]
    gx, gdy = [t.to(dev) for t in xs], [t.to(dev) for t in dys]
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    dws = [torch.full((cout, cin, k, k), NAN, device=dev) for _ in range(nprob)]
    dbs = [torch.full((cout,), NAN, device=dev) for _ in range(nprob)]
    with reserve(case['k']):
        nws = L.srx_conv2d_bwd_weight_multi_ws_floats(C.byref(d), nprob)
        assert nws == case['ws'], (nws, case['ws'])
        ws = torch.full((nws,), NAN, device=dev)
        _, names = _run(lambda: lib.call('srx_conv2d_bwd_weight_multi', C.byref(d), nprob, 1, arr(gx), arr(gdy), arr(dws), 0, arr(dbs),
                                         _p(ws), nws, s))
    m = n * h * w
    assert names == [f'wgrad_dma_kernel<1, 1> MxNxK={m}x{cout}x{k * k * cin} x{nprob}'], names
    per_split = (cout + 63) // 64 * 64 * (k * k * cin + 1) * nprob   # one slab + one bias row per problem and row split
    assert nws % per_split == 0 and nws // per_split != case['ws0'] // per_split
    print(f'  {case["id"]}: {nws // per_split} row splits ({case["ws0"] // per_split} with nothing reserved)')
    for i in range(nprob):
        assert not torch.isnan(dws[i]).any() and not torch.isnan(dbs[i]).any(), i
        ew, eb = rel_err(dws[i], want_w[i]), rel_err(dbs[i], want_b[i])
        print(f'  {case["id"]} problem {i}: {names[0]}  dW rel err {ew:.3g}, db rel err {eb:.3g}')
        assert ew < 2e-4 and eb < 2e-4, (i, ew, eb)
