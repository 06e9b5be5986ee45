"""The 4x4 / stride 2 / pad 1 layers of the U-Net critic (conv1..conv3) under every launch form of gconv.hip a plan can give them
(cases: k4s2_forms.py; that each case reaches its form: test_k4s2_forms_cpu.py), checked as test_forced_paths_gpu.py checks its 3x3
layers: the plan the library reports, the kernel that really ran (its srx_prof record), and the numbers against fp64 of
bf16-rounded (precision 1) or plain fp32 operands at that file's bound, rel_err < 1e-5.

* data gradient: every gconv_s2f_kernel instantiation and its gconv_multi_kernel twin on the same tile, bit for bit against each
  other, under the plain epilogue and the three activation masks; the multi-only forms (64 x 64 with KS = 2, 128 x 32 on
  Cin <= 32); the odd-extent layer under multi, the fused kernel refused on it with dx untouched;
* forward: every gconv_kernel tile whole and cut in two along K (NaN-filled workspace, tail_fixup_kernel), with the layer's own
  LeakyReLU(0.2) epilogue and no bias, one tile also with a bias.

Outputs start as NaN, channels past Cin hold a sentinel.  The weight gradient's 4x4 rows run in test_wgrad_forms_gpu.py (rows K1..K3
of wgrad_forms.py).  Each test prints the worst error it met (profiles/k4s2_slopes_tests_times.txt)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as TF

import k4s2_forms as KF
import test_forced_paths_gpu as FP
from test_forced_paths_gpu import SENTINEL, _launched, _plan, _tile_args, multi_name, rel_err, s2f_name

pytestmark = pytest.mark.gpu

NAN = float('nan')
_SEEN = set()      # kernel names (template head, without the GEMM shape) this module's launches recorded


@pytest.fixture(autouse=True)
def _no_forced_plans(dev):
    """Every override is off again after each test, whether it passed or not."""
    try:
        yield
    finally:
        from torchsr_amd import _lib
        L = _lib.lib()
        assert L.srx_conv2d_force_plan(0, 0, 0, 0) == 0
        assert L.srx_conv2d_force_s2(0, 0, 0) == 0
        assert L.srx_wgrad_force(-1, 0) == 0
        assert L.srx_wgrad_force_kernels(-1, -1, -1) == 0


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _layer(shape, prec):
    """test_forced_paths_gpu.Layer with a 4 x 4 kernel: packed weights, dy, the mask input and the fp64 data gradient, once per
    (shape, precision) and never changed"""
    lay = FP._layer(*shape, prec, KF.K)
    assert (lay.d.KH, lay.d.KW, lay.d.stride, lay.d.pad) == (KF.K, KF.K, KF.STRIDE, KF.PAD)
    return lay


def _force(case):
    from torchsr_amd import _lib
    f = case['force']
    if f[0] == 's2':
        _lib.call('srx_conv2d_force_plan', 0, 0, 0, 0)
        _lib.call('srx_conv2d_force_s2', *f[1:])
    else:
        _lib.call('srx_conv2d_force_s2', 1, 0, 0)
        _lib.call('srx_conv2d_force_plan', f[1], f[2], 1, f[3])


def _dgrad_name(case):
    bm, bn = case['tile']
    return s2f_name(case['prec'], bm, bn) if case['form'] == KF.FUSED else multi_name(case['prec'], bm, bn, case['ks'])


def _run_dgrad_case(case):
    """The case's layer under its override: FP._check_layer asserts the plan, the one recorded launch, NaN-free dx, the sentinel
    behind Cin and rel_err < 1e-5 for the plain epilogue and the three masks; returns the four dx."""
    lay = _layer(case['shape'], case['prec'])
    _force(case)
    name = _dgrad_name(case)
    outs = FP._check_layer(lay, name, case['plan'])
    _SEEN.add(name)
    worst = max(rel_err(dx[..., :lay.cin], lay.want(mask)) for dx, mask in zip(outs, [None] + lay.masks()))
    print(f'K4S2 {case["id"]}: {name} plan {case["plan"]} worst rel err {worst:.3g}')
    return outs


def _cases(form, prec, bm, bn, ks=1):
    return [c for c in KF.DGRAD if (c['form'], c['prec'], c['tile'], c['ks']) == (form, prec, (bm, bn), ks)]


# ------------------------------------------------------------------------------------------------------------- data gradient
@pytest.mark.parametrize('prec,bm,bn', KF.S2F_TILES, ids=lambda v: str(v))
def test_k4s2_dgrad_fused_and_multi_forms_of_one_tile(dev, prec, bm, bn):
    """gconv_s2f_kernel on every instantiation and gconv_multi_kernel on the same tile, on every layer whose columns the tile
    divides: both against fp64, and bit for bit against each other (same products, same k order).  The odd-extent layer runs the
    multi form alone."""
    assert KF.S2F_TILES == FP.S2F_TILES
    fused = {c['shape']: c for c in _cases(KF.FUSED, prec, bm, bn)}
    multi = {c['shape']: c for c in _cases(KF.MULTI, prec, bm, bn)}
    assert fused and set(fused) <= set(multi)
    for i, shape in enumerate(multi):
        got_multi = _run_dgrad_case(multi[shape])
        if shape not in fused:
            assert shape == KF.ODD
            continue
        got_fused = _run_dgrad_case(fused[shape])
        if i == 0:
            FP._check_refusals(_layer(shape, prec))
        for a, b in zip(got_fused, got_multi):
            assert torch.equal(a, b), (shape, rel_err(a, b))


@pytest.mark.parametrize('prec,bm,bn,ks', KF.MULTI_ONLY, ids=lambda v: str(v))
def test_k4s2_dgrad_multi_only_forms(dev, prec, bm, bn, ks):
    """The gconv_multi_kernel forms without a fused twin: the two-wave-group 64 x 64 tile (KS = 2: the step's own plan for conv2 and
    conv3 in fp32) on every layer, the odd-extent one included, and the 32-column tile of layers with Cin <= 32."""
    cases = _cases(KF.MULTI, prec, bm, bn, ks)
    assert cases
    for i, case in enumerate(cases):
        _run_dgrad_case(case)
        if i == 0:
            FP._check_refusals(_layer(case['shape'], prec))


@pytest.mark.parametrize('case', KF.ODD_FUSED_REFUSED, ids=lambda c: 'p%d.%dx%d' % ((c['prec'],) + c['force'][2:]))
def test_k4s2_fused_kernel_on_the_odd_extent_layer_is_refused(dev, case):
    """H = 13, W = 17: the classes lie on different grids.  The forced fused kernel is an error before anything is launched -- the
    plan query says so and dx keeps every bit, plain epilogue and mask."""
    from torchsr_amd import _lib
    L = _lib.lib()
    lay = _layer(case['shape'], case['prec'])
    _force(case)
    out = (C.c_int * 6)()
    assert L.srx_conv2d_plan(C.byref(lay.d), 1, out) == 2 and case['message'] in _lib.last_error(), _lib.last_error()
    dx = lay.fresh_dx()
    dx[..., :lay.cin] = 3.0
    before = dx.clone()
    for mask in (None, (0, lay.cin)):
        with pytest.raises(RuntimeError, match=case['message']):
            lay.run(mask, dx=dx)
    torch.cuda.synchronize()
    assert torch.equal(dx, before)


# ------------------------------------------------------------------------------------------------------------------- forward
class FwdLayer:
    """A 4x4 / stride 2 / pad 1 layer's forward with the critic's LeakyReLU(0.2) epilogue: x (channels past Cin: a sentinel, they
    are someone else's), packed weights, a bias for the one case that runs with it, and the fp64 results without and with the bias
    of bf16-rounded (precision 1) or plain fp32 operands -- computed once, never changed."""

    def __init__(self, shape, prec, dev):
        from torchsr_amd import _lib
        L = _lib.lib()
        n, h, w, cin, cout, cin_s = shape
        self.shape, self.prec, self.dev = shape, prec, dev
        self.d = _lib.Conv2dDesc(*KF.desc_fields(shape, prec, KF.ACT_LRELU, KF.SLOPE))
        self.ho, self.wo = KF.out_size(shape)
        g = torch.Generator().manual_seed(4000 + n * 1000 + h * 37 + cin + 3 * cout)
        wt = torch.randn(cout, cin, KF.K, KF.K, generator=g) * 0.05
        x = torch.randn(n, h, w, cin_s, generator=g)
        x[..., cin:] = SENTINEL
        bias = torch.randn(cout, generator=g)
        self.x, self.bias = x.to(dev), bias.to(dev)
        self.wf = torch.empty(L.srx_conv2d_packed_fwd_floats(C.byref(self.d)), device=dev)
        wb = torch.empty(max(L.srx_conv2d_packed_bwd_floats(C.byref(self.d)), 4), device=dev)
        wg = wt.to(dev)
        _lib.call('srx_conv2d_pack', C.byref(self.d), wg.data_ptr(), self.wf.data_ptr(), wb.data_ptr(), _stream())
        r = (lambda t: t.bfloat16().double()) if prec else (lambda t: t.double())
        z = TF.conv2d(r(x[..., :cin].permute(0, 3, 1, 2)), r(wt), None, stride=KF.STRIDE, padding=KF.PAD).permute(0, 2, 3, 1)
        act = lambda v: torch.where(v > 0, v, v * KF.SLOPE).contiguous()  # noqa: E731
        self.want = {False: act(z), True: act(z + bias.double())}   # NHWC, fp64
        torch.cuda.synchronize()

    def run(self, with_bias):
        """Into a NaN-filled output, the split-K workspace (exactly the queried size) NaN-filled too."""
        from torchsr_amd import _lib
        L = _lib.lib()
        need = L.srx_conv2d_fwd_ws_floats(C.byref(self.d))
        ws = torch.full((max(need, 4),), NAN, device=self.dev)
        y = torch.full((self.shape[0], self.ho, self.wo, self.shape[4]), NAN, device=self.dev)
        _lib.call('srx_conv2d_fwd', C.byref(self.d), self.x.data_ptr(), self.wf.data_ptr(), self.bias.data_ptr() if with_bias else None,
                  y.data_ptr(), None, ws.data_ptr(), need, _stream())
        return y, need


@functools.lru_cache(maxsize=None)
def _fwd_layer(shape, prec):
    return FwdLayer(shape, prec, torch.device('cuda:0'))


@pytest.mark.parametrize('prec,bm,bn,ks_arg,ks', KF.SINGLE_TILES, ids=lambda v: str(v))
def test_k4s2_forward_under_forced_tiles(dev, prec, bm, bn, ks_arg, ks):
    """Every gconv_kernel tile a plan can ask for, forced on the 64 -> 128 and 128 -> 256 layers' forward, whole (split 1) and with
    every tile cut in two along K (split 2).  The fix-up pass of a split plan (tail_fixup_kernel) is not a recorded launch; that
    it ran is shown by the output: under a forced split every tile's partial sums go to the workspace and tail_fixup_kernel alone
    writes the output tensor, which starts as NaN (the workspace too)."""
    from torchsr_amd import _lib
    assert KF.SINGLE_TILES == FP.SINGLE_TILES
    head, _, wm, wn, xr = _tile_args(bm, bn)
    if bm == 256:
        wn = 64   # (the 256-row tile: 64 x 64 per wave)
    kernel = f'gconv_kernel<{head}, {bn}, {wm}, {wn}, {ks}, {xr}, {prec}>'
    cases = [c for c in KF.FWD if (c['prec'],) + c['tile'] + (c['ks_arg'], c['ks']) == (prec, bm, bn, ks_arg, ks)]
    assert {(c['split'], c['shape']) for c in cases} == {(s, sh) for s in KF.FWD_SPLITS for sh in KF.FWD_SHAPES}
    for case in cases:
        shape, split = case['shape'], case['split']
        lay = _fwd_layer(shape, prec)
        m, cin, cout = shape[0] * lay.ho * lay.wo, shape[3], shape[4]
        name = f'{kernel} MxNxK={m}x{cout}x{KF.K * KF.K * cin}'
        _lib.call('srx_conv2d_force_plan', bm, bn, split, ks_arg)
        assert _plan(lay.d, 0) == case['plan'], (_plan(lay.d, 0), case['plan'])
        biases = (False, True) if (prec, bm, bn, ks_arg, ks) == KF.FWD_BIAS_CASE and shape == KF.FWD_SHAPES[0] else (False,)
        for with_bias in biases:
            holder = []
            names = _launched(lambda: holder.append(lay.run(with_bias)))
            y, need = holder[0]
            assert names == [name], (names, name, split)
            assert need == (0 if split == 1 else case['plan'][3] * bm * bn), (need, case['plan'])
            torch.cuda.synchronize()
            assert not torch.isnan(y).any(), (shape, split, with_bias)
            err = rel_err(y, lay.want[with_bias])
            print(f'K4S2 {case["id"]} bias {with_bias}: {kernel} rel err {err:.3g}')
            assert err < 1e-5, (shape, split, with_bias, err)
        _SEEN.add(kernel)


# ---------------------------------------------------------------------------------------------------------------- the record
def test_zz_every_strided_dgrad_form_ran_on_a_4x4_layer(dev):
    """The union of the data-gradient kernel names this module's launches recorded: all 8 gconv_s2f_kernel instantiations, their
    multi twins and the multi-only forms (cases this process has not run yet run here)."""
    want = {_dgrad_name(c) for c in KF.DGRAD}
    for case in KF.DGRAD:
        if _dgrad_name(case) not in _SEEN:
            _run_dgrad_case(case)
    fused = sorted(n for n in _SEEN if n.startswith('gconv_s2f_kernel'))
    print('K4S2 data-gradient kernels recorded:', sorted(n for n in _SEEN if not n.startswith('gconv_kernel')))
    assert len(fused) == 8 and want <= _SEEN, sorted(want - _SEEN)
