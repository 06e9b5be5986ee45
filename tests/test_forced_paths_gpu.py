"""Every kernel form the strided data gradient and the fp32 weight gradient can launch, forced in-process
(srx_conv2d_force_plan / srx_conv2d_force_s2 / srx_wgrad_force) and checked three ways: the plan the library reports,
the kernel that really ran (its srx_prof record), and the numbers against an fp64 reference.  Forms the cost model
picks only at some shapes -- or never -- are otherwise covered by nothing but the whole-step goldens.
"""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_forced_plans():
    """Every override is off again after each test, whether it passed or not."""
    yield
    from torchsr_amd import _lib
    L = _lib.lib()
    assert L.srx_conv2d_force_plan(0, 0, 0, 0) == 0
    assert L.srx_conv2d_force_s2(0, 0, 0) == 0
    assert L.srx_wgrad_force(-1, 0) == 0
    assert L.srx_wgrad_force_kernels(-1, -1, -1) == 0


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-6)).item()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _plan(d, which):
    from torchsr_amd import _lib
    out = (C.c_int * 6)()
    _lib.call('srx_conv2d_plan', C.byref(d), which, out)
    return list(out)


def _launched(fn):
    """Run fn with the per-launch records on; the names of the conv kernels it launched."""
    from torchsr_amd import _lib
    L = _lib.lib()
    _lib.call('srx_prof_start', 64)
    try:
        fn()
    finally:
        n = L.srx_prof_stop()
    names = []
    buf, ms, fl = C.create_string_buffer(128), C.c_float(), C.c_double()
    for i in range(n):
        _lib.call('srx_prof_get', i, buf, 128, C.byref(ms), C.byref(fl))
        names.append(buf.value.decode())
    return names


def _tile_args(bm, bn):
    """gconv template head of a tile: BM BN WM WN, the 144-row tile being 128 rows + XR = 16."""
    return (128 if bm == 144 else bm), bn, (64 if bn == 128 else 32), 32, (16 if bm == 144 else 0)


def s2f_name(prec, bm, bn):
    b, n, wm, wn, xr = _tile_args(bm, bn)
    return f'gconv_s2f_kernel<{b}, {n}, {wm}, {wn}, {xr}, {prec}>'


def multi_name(prec, bm, bn, ks):
    b, n, wm, wn, xr = _tile_args(bm, bn)
    return f'gconv_multi_kernel<{b}, {n}, {wm}, {wn}, {xr}, {prec}, {ks}>'


# ------------------------------------------------------------------ a. strided data gradients
SENTINEL = 7.0


class Layer:
    """A k x k (3x3; 4x4: test_k4s2_forms_gpu.py) / stride 2 / pad 1 layer with packed weights, dy, the activation output x (mask
    input, in dx's layout) and the fp64 data gradient of bf16-rounded (precision 1) or plain fp32 operands."""

    def __init__(self, n, h, w, cin, cout, cin_s, prec, dev, k=3):
        from torchsr_amd import _lib
        L = _lib.lib()
        self.n, self.h, self.w, self.cin, self.cout, self.cin_s, self.prec = n, h, w, cin, cout, cin_s, prec
        self.d = _lib.Conv2dDesc(n, h, w, cin, cin_s, cout, cout, k, k, 2, 1, 0, 0, 0.0, 0, prec)
        ho, wo = (h + 2 - k) // 2 + 1, (w + 2 - k) // 2 + 1
        g = torch.Generator().manual_seed(n * 1000 + h * 37 + cin + 3 * cout)
        wt = torch.randn(cout, cin, k, k, generator=g) * 0.05
        dy = torch.randn(n, ho, wo, cout, generator=g)
        self.x = torch.randn(n, h, w, cin_s, generator=g).to(dev)
        self.dy = dy.to(dev)
        self.wb = torch.empty(max(L.srx_conv2d_packed_bwd_floats(C.byref(self.d)), 4), device=dev)
        wf = torch.empty(L.srx_conv2d_packed_fwd_floats(C.byref(self.d)), device=dev)
        wg = wt.to(dev)
        _lib.call('srx_conv2d_pack', C.byref(self.d), wg.data_ptr(), wf.data_ptr(), self.wb.data_ptr(), _stream())
        r = (lambda t: t.bfloat16().double()) if prec else (lambda t: t.double())
        ref = torch.nn.grad.conv2d_input((n, cin, h, w), r(wt), r(dy.permute(0, 3, 1, 2)), stride=2, padding=1)
        self.ref = ref.permute(0, 2, 3, 1).contiguous()   # NHWC, fp64
        self.xc = self.x.cpu().double()
        torch.cuda.synchronize()

    def masks(self):
        """(c_lo, c_hi) of the activation mask: the full range, a partial one that starts past 0, one whose end lies past Cin
        and is not a quad (the epilogue clips it to Cin)."""
        c = self.cin
        part = (16, c - 16) if c > 32 else (8, c - 4)
        return [(0, c), part, (8 if c <= 32 else 12, c + 2)]

    def want(self, mask):
        want = self.ref.clone()
        if mask is not None:
            lo, hi = mask[0], min(mask[1], self.cin)
            want[..., lo:hi] *= torch.where(self.xc[..., lo:hi] > 0, 1.0, 0.2)
        return want

    def fresh_dx(self):
        dx = torch.full((self.n, self.h, self.w, self.cin_s), float('nan'), device=self.x.device)
        dx[..., self.cin:] = SENTINEL   # channels past Cin belong to someone else
        return dx

    def run(self, mask=None, dx=None, **epi):
        from torchsr_amd import _lib
        e = _lib.DgradEpilogue()
        if mask is not None:
            e.act_out, e.act_slope, e.c_lo, e.c_hi = self.x.data_ptr(), 0.2, mask[0], mask[1]
        for k, v in epi.items():
            setattr(e, k, v)
        dx = self.fresh_dx() if dx is None else dx
        _lib.call('srx_conv2d_bwd_data_ex', C.byref(self.d), self.dy.data_ptr(), self.wb.data_ptr(), dx.data_ptr(), C.byref(e),
                  None, 0, _stream())
        return dx


@functools.lru_cache(maxsize=None)
def _layer(n, h, w, cin, cout, cin_s, prec, k=3):
    return Layer(n, h, w, cin, cout, cin_s, prec, torch.device('cuda:0'), k)


# Ragged last row tile for every BM (M = 585, 198, 126, 30), padded output columns (Cin 96 -> 128 columns, 192 -> 192),
# channels past Cin (Cin_s > Cin, pre-filled with a sentinel), Cout 64 / 96 / 128 / 256 (K per class up to 4 x 256).
SHAPES = [(3, 26, 30, 64, 64, 64), (2, 22, 18, 128, 128, 136), (2, 14, 18, 96, 256, 100), (1, 10, 12, 192, 96, 196)]
NARROW = [(3, 26, 30, 32, 64, 36), (2, 22, 18, 20, 96, 24)]   # Cin <= 32: one 32-column tile


def _shapes(bn, narrow=False):
    return [s for s in (NARROW if narrow else SHAPES) if ((s[3] + 63) // 64 * 64 if s[3] > 32 else 32) % bn == 0]


def _check_layer(lay, name, plan_want):
    """Plain epilogue (dx NaN-filled: every pixel of every stride-parity class written) and the three masks; returns the dx
    tensors so that two forms of one tile can be compared bit for bit."""
    assert _plan(lay.d, 1) == plan_want, (_plan(lay.d, 1), plan_want)
    outs = []
    for mask in [None] + lay.masks():
        holder = []
        names = _launched(lambda: holder.append(lay.run(mask)))
        assert len(names) == 1 and names[0] == name, (names, name)
        dx = holder[0]
        torch.cuda.synchronize()
        assert not torch.isnan(dx).any(), mask
        assert bool((dx[..., lay.cin:] == SENTINEL).all()), mask
        assert rel_err(dx[..., :lay.cin], lay.want(mask)) < 1e-5, (mask, rel_err(dx[..., :lay.cin], lay.want(mask)))
        outs.append(dx)
    return outs


def _check_refusals(lay):
    """Strided layers take the plain and the masked epilogue only: an addend, accumulate (with or without a mask) and a lone
    out_scale are refused before anything runs -- dx keeps every bit."""
    from torchsr_amd import _lib
    dx = lay.fresh_dx()
    dx[..., :lay.cin] = 3.0
    before = dx.clone()
    add = torch.ones_like(dx)
    for mask, epi, msg in ((None, dict(addend=add.data_ptr()), 'stride-1 layers'),
                           (None, dict(accumulate=1), 'accumulate'),
                           ((0, lay.cin), dict(accumulate=1), 'accumulate'),
                           (None, dict(out_scale=0.5), 'without an addend')):
        with pytest.raises(RuntimeError, match=msg):
            lay.run(mask, dx=dx, **epi)
    torch.cuda.synchronize()
    assert torch.equal(dx, before)


def _plan_row(lay, bm, bn, ks, multi):
    cnp = (lay.cin + 63) // 64 * 64 if lay.cin > 32 else 32
    m = lay.n * ((lay.h + 1) // 2) * ((lay.w + 1) // 2)
    wgs = -(-m // bm) * (cnp // bn) * (1 if multi == 2 else 4)
    return [bm, bn, 1, wgs, ks, multi]


S2F_TILES = [(0, 144, 128), (0, 144, 64), (0, 128, 128), (0, 128, 64), (0, 64, 64), (1, 128, 128), (1, 128, 64), (1, 64, 64)]


@pytest.mark.parametrize('prec,bm,bn', S2F_TILES, ids=lambda v: str(v))
def test_strided_dgrad_fused_and_multi_forms_of_one_tile(dev, prec, bm, bn):
    """gconv_s2f_kernel on every instantiation and gconv_multi_kernel on the same tile: both against fp64, and bit for bit
    against each other (same products, same k order: the fused kernel only walks the classes inside one workgroup)."""
    from torchsr_amd import _lib
    L = _lib.lib()
    for i, shape in enumerate(_shapes(bn)):
        lay = _layer(*shape, prec)
        _lib.call('srx_conv2d_force_plan', 0, 0, 0, 0)
        _lib.call('srx_conv2d_force_s2', 2, bm, bn)
        fused = _check_layer(lay, s2f_name(prec, bm, bn), _plan_row(lay, bm, bn, 1, 2))
        if i == 0:
            _check_refusals(lay)
        _lib.call('srx_conv2d_force_s2', 1, 0, 0)
        _lib.call('srx_conv2d_force_plan', bm, bn, 1, 1)
        multi = _check_layer(lay, multi_name(prec, bm, bn, 1), _plan_row(lay, bm, bn, 1, 1))
        for a, b in zip(fused, multi):
            assert torch.equal(a, b), (shape, rel_err(a, b))
    assert L.srx_conv2d_force_s2(0, 0, 0) == 0


@pytest.mark.parametrize('prec,bm,bn,ks', [(0, 64, 64, 2), (1, 64, 64, 2), (0, 128, 32, 1), (1, 128, 32, 1)], ids=lambda v: str(v))
def test_strided_dgrad_multi_only_forms(dev, prec, bm, bn, ks):
    """The gconv_multi_kernel forms without a fused twin: the two-wave-group 64 x 64 tile (KS = 2) and the 32-column tile of
    layers with Cin <= 32."""
    from torchsr_amd import _lib
    _lib.call('srx_conv2d_force_s2', 1, 0, 0)
    _lib.call('srx_conv2d_force_plan', bm, bn, 1, ks)
    for i, shape in enumerate(_shapes(bn, narrow=bn == 32)):
        lay = _layer(*shape, prec)
        _check_layer(lay, multi_name(prec, bm, bn, ks), _plan_row(lay, bm, bn, ks, 1))
        if i == 0:
            _check_refusals(lay)


@pytest.mark.parametrize('n,h,w,prec,default', [(16, 96, 96, 0, (144, 64, 2)), (16, 96, 96, 1, (128, 64, 1)),
                                                (16, 128, 128, 0, (128, 64, 2)), (16, 128, 128, 1, (128, 64, 2))])
def test_strided_dgrad_discriminator_layer_default_and_forced(dev, n, h, w, prec, default):
    """The discriminators' 64 -> 64 stride-2 layer at the training batch: the cost model's own plan (pinned), and the other form
    of the same tile forced -- both against fp64 and bit for bit against each other."""
    from torchsr_amd import _lib
    bm, bn, multi = default
    lay = Layer(n, h, w, 64, 64, 64, prec, dev)
    name = s2f_name(prec, bm, bn) if multi == 2 else multi_name(prec, bm, bn, 1)
    got = []
    for mask in (None, (0, 64)):
        assert _plan(lay.d, 1) == _plan_row(lay, bm, bn, 1, multi)
        holder = []
        assert _launched(lambda: holder.append(lay.run(mask))) == [name]
        torch.cuda.synchronize()
        assert rel_err(holder[0][..., :64], lay.want(mask)) < 1e-5
        got.append(holder[0])
    if multi == 2:
        _lib.call('srx_conv2d_force_s2', 1, 0, 0)
        _lib.call('srx_conv2d_force_plan', bm, bn, 1, 1)
        other = multi_name(prec, bm, bn, 1)
    else:
        _lib.call('srx_conv2d_force_s2', 2, bm, bn)
        other = s2f_name(prec, bm, bn)
    for mask, want in zip((None, (0, 64)), got):
        holder = []
        assert _launched(lambda: holder.append(lay.run(mask))) == [other]
        torch.cuda.synchronize()
        assert torch.equal(holder[0], want)


def test_forced_strided_forms_a_layer_cannot_run_are_refused(dev):
    """A forced form with no kernel for the layer is an error before anything is launched -- never a silent other kernel:
    the fused kernel on an odd extent (H = 13: classes on different grids), on Cin = 32 (one 32-column tile), on Cout = 48
    (not whole chunks per tap); tiles with no instantiation at the layer's arithmetic; a tile wider than the padded columns."""
    from torchsr_amd import _lib
    L = _lib.lib()
    cases = [((2, 13, 18, 64, 64, 64), 0, ('s2', 2, 128, 64), 'stride-parity classes'),
             ((2, 14, 18, 32, 64, 32), 0, ('s2', 2, 64, 64), 'stride-parity classes'),
             ((2, 14, 18, 64, 48, 64), 0, ('s2', 2, 64, 64), 'stride-parity classes'),
             ((3, 26, 30, 64, 64, 64), 1, ('s2', 2, 144, 64), 'no instantiation'),
             ((2, 14, 18, 96, 256, 100), 1, ('s2', 2, 144, 128), 'no instantiation'),
             ((1, 10, 12, 192, 96, 196), 0, ('s2', 2, 128, 128), 'do not divide'),
             ((3, 26, 30, 64, 64, 64), 0, ('plan', 64, 32, 1, 1), 'no instantiation'),   # (gconv_multi_kernel has no 64 x 32 form)
             ((3, 26, 30, 64, 64, 64), 1, ('plan', 144, 64, 1, 1), 'no 144-row tile'),
             ((2, 22, 18, 128, 128, 136), 0, ('plan', 256, 128, 1, 1), 'no 256-row tile'),
             ((1, 10, 12, 192, 96, 196), 0, ('plan', 128, 128, 1, 1), 'do not divide'),
             ((3, 26, 30, 64, 64, 64), 0, ('plan', 128, 64, 1, 2), 'two wave groups')]
    for shape, prec, force, msg in cases:
        if force[0] == 's2':
            _lib.call('srx_conv2d_force_plan', 0, 0, 0, 0)
            _lib.call('srx_conv2d_force_s2', *force[1:])
        else:
            _lib.call('srx_conv2d_force_s2', 1, 0, 0)
            _lib.call('srx_conv2d_force_plan', *force[1:])
        lay = _layer(*shape, prec) if shape in [s[:6] for s in SHAPES] else Layer(*shape, prec, dev)
        out = (C.c_int * 6)()
        assert L.srx_conv2d_plan(C.byref(lay.d), 1, out) == 2 and msg in _lib.last_error(), (shape, force, _lib.last_error())
        dx = lay.fresh_dx()
        dx[..., :lay.cin] = 3.0
        before = dx.clone()
        for mask in (None, (0, lay.cin)):
            with pytest.raises(RuntimeError, match=msg):
                lay.run(mask, dx=dx)
        torch.cuda.synchronize()
        assert torch.equal(dx, before), (shape, force)
    _lib.call('srx_conv2d_force_plan', 0, 0, 0, 0)
    _lib.call('srx_conv2d_force_s2', 0, 0, 0)
    for bad in ((3, 0, 0), (2, 96, 64), (2, 144, 32), (0, 64, 64)):
        with pytest.raises(RuntimeError, match='force_s2'):
            _lib.call('srx_conv2d_force_s2', *bad)
    for bad in ((144, 64, 0, 1), (100, 64, 1, 1), (64, 64, 1, 3), (64, 0, 1, 1), (64, 64, 17, 1)):
        with pytest.raises(RuntimeError, match='force_plan'):
            _lib.call('srx_conv2d_force_plan', *bad)


# ------------------------------------------------------------------ b. single-launch convs (gconv_kernel) under forced tiles
class DenseLayer:
    """3x3 / stride 1 / pad 1, 128 -> 128 channels, N = 2, 22 x 18: M = 792 leaves a ragged last row tile for every BM
    (792 = 5 x 144 + 72 = 6 x 128 + 24 = 12 x 64 + 24 = 3 x 256 + 24), every BN divides the 128 padded columns, K = 1152 is 36
    chunks (a forced split of 3: 12 each).  Neither the 36-pixel row-tile shape nor a thin layer.  Forward (with bias) and data
    gradient against the fp64 convolution of bf16-rounded (precision 1) or plain fp32 operands."""
    N, H, W, CH = 2, 22, 18, 128

    def __init__(self, prec, dev):
        from torchsr_amd import _lib
        L = _lib.lib()
        n, h, w, c = self.N, self.H, self.W, self.CH
        self.d = _lib.Conv2dDesc(n, h, w, c, c, c, c, 3, 3, 1, 1, 0, 0, 0.0, 0, prec)
        g = torch.Generator().manual_seed(792 + prec)
        wt = torch.randn(c, c, 3, 3, generator=g) * 0.05
        x = torch.randn(n, h, w, c, generator=g)
        dy = torch.randn(n, h, w, c, generator=g)
        bias = torch.randn(c, generator=g)
        self.x, self.dy, self.bias = x.to(dev), dy.to(dev), bias.to(dev)
        self.wf = torch.empty(L.srx_conv2d_packed_fwd_floats(C.byref(self.d)), device=dev)
        self.wb = torch.empty(L.srx_conv2d_packed_bwd_floats(C.byref(self.d)), device=dev)
        wg = wt.to(dev)
        _lib.call('srx_conv2d_pack', C.byref(self.d), wg.data_ptr(), self.wf.data_ptr(), self.wb.data_ptr(), _stream())
        r = (lambda t: t.bfloat16().double()) if prec else (lambda t: t.double())
        y = torch.nn.functional.conv2d(r(x.permute(0, 3, 1, 2)), r(wt), bias.double(), padding=1)
        dx = torch.nn.grad.conv2d_input((n, c, h, w), r(wt), r(dy.permute(0, 3, 1, 2)), padding=1)
        self.want = [y.permute(0, 2, 3, 1).contiguous(), dx.permute(0, 2, 3, 1).contiguous()]   # NHWC, fp64
        torch.cuda.synchronize()

    def run(self, which):
        """Forward (which = 0) or data gradient (1) into a NaN-filled output, the split-K workspace NaN-filled too."""
        from torchsr_amd import _lib
        L = _lib.lib()
        need = (L.srx_conv2d_bwd_data_ws_floats if which else L.srx_conv2d_fwd_ws_floats)(C.byref(self.d))
        ws = torch.full((max(need, 4),), float('nan'), device=self.x.device)
        out = torch.full((self.N, self.H, self.W, self.CH), float('nan'), device=self.x.device)
        if which:
            _lib.call('srx_conv2d_bwd_data', C.byref(self.d), self.dy.data_ptr(), self.wb.data_ptr(), out.data_ptr(), 0,
                      ws.data_ptr(), need, _stream())
        else:
            _lib.call('srx_conv2d_fwd', C.byref(self.d), self.x.data_ptr(), self.wf.data_ptr(), self.bias.data_ptr(), out.data_ptr(),
                      None, ws.data_ptr(), need, _stream())
        return out, need


@functools.lru_cache(maxsize=None)
def _dense_layer(prec):
    return DenseLayer(prec, torch.device('cuda:0'))


# (precision, BM, BN, KS asked for, KS of the kernel): the 64 x 32 tile deals its k-chunks to 2 (fp32) / 4 (bf16) wave groups
SINGLE_TILES = [(0, 144, 128, 1, 1), (0, 144, 64, 1, 1), (0, 128, 128, 1, 1), (0, 128, 64, 1, 1), (0, 64, 64, 1, 1),
                (0, 64, 64, 2, 2), (0, 64, 32, 1, 2), (0, 128, 32, 1, 1),
                (1, 256, 128, 1, 1), (1, 128, 128, 1, 1), (1, 128, 64, 1, 1), (1, 64, 64, 1, 1), (1, 64, 64, 2, 2),
                (1, 128, 32, 1, 1), (1, 64, 32, 1, 4)]


@pytest.mark.parametrize('prec,bm,bn,ks_arg,ks', SINGLE_TILES, ids=lambda v: str(v))
def test_forced_tiles_on_single_launch_convs(dev, prec, bm, bn, ks_arg, ks):
    """Every gconv_kernel tile a plan can ask for at fp32 / bf16 products, forced on a stride-1 layer's forward and data
    gradient, whole (split 1) and with every tile cut three ways along K (split 3): the reported plan, the launch that ran and
    the numbers.  The fix-up pass of a split plan (tail_fixup_kernel) is not a recorded launch, so the recorder shows the
    gconv_kernel launch alone; that the fix-up ran after it is shown by the output: under a forced split every tile's partial
    sums go to the workspace and tail_fixup_kernel alone writes the output tensor, which starts as NaN (the workspace too)."""
    from torchsr_amd import _lib
    lay = _dense_layer(prec)
    m, c = lay.N * lay.H * lay.W, lay.CH
    head, _, wm, wn, xr = _tile_args(bm, bn)
    if bm == 256:
        wn = 64   # (the 256-row tile: 64 x 64 per wave)
    name = f'gconv_kernel<{head}, {bn}, {wm}, {wn}, {ks}, {xr}, {prec}> MxNxK={m}x{c}x{9 * c}'
    for split in (1, 3):
        _lib.call('srx_conv2d_force_plan', bm, bn, split, ks_arg)
        for which in (0, 1):
            assert _plan(lay.d, which) == [bm, bn, split, -(-m // bm) * (c // bn) * split, ks, 0], (_plan(lay.d, which), split, which)
            holder = []
            names = _launched(lambda: holder.append(lay.run(which)))
            out, need = holder[0]
            assert names == [name], (names, name, split, which)
            assert need == (0 if split == 1 else -(-m // bm) * (c // bn) * split * bm * bn), (need, split, which)
            torch.cuda.synchronize()
            assert not torch.isnan(out).any(), (split, which)
            err = rel_err(out, lay.want[which])
            print(f'prec {prec} tile {bm}x{bn} ks {ks} split {split} which {which}: rel err {err:.3g}')
            assert err < 1e-5, (split, which, err)


# ------------------------------------------------------------------ c. the LIN weight gradient
def _wgrad(dev, n, h, w, cin, cout, k, nsplit=0, nprob=1, accumulate=0, lin_names=True):
    """fp32 stride-1 same-size layer(s): the LIN and the plain WIDE form of wgrad_dma_kernel (forced), bit for bit against each
    other and against fp64 (bias gradient riding along)."""
    from torchsr_amd import _lib
    L = _lib.lib()
    pad = k // 2
    d = _lib.Conv2dDesc(n, h, w, cin, cin, cout, cout, k, k, 1, pad, 0, 0, 0.0, 0, 0)
    g = torch.Generator().manual_seed(n + h * 7 + w * 13 + k + nprob)
    xs = [torch.randn(n, h, w, cin, generator=g) for _ in range(nprob)]
    dys = [torch.randn(n, h, w, cout, generator=g) for _ in range(nprob)]
    base_w, base_b = torch.randn(cout, cin, k, k, generator=g), torch.randn(cout, generator=g)
    want_w = base_w.double() * accumulate
    want_b = base_b.double() * accumulate
    for x, dy in zip(xs, dys):
        want_w = want_w + torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2).double(), (cout, cin, k, k),
                                                      dy.permute(0, 3, 1, 2).double(), padding=pad)
        want_b = want_b + dy.double().sum((0, 1, 2))
    gx, gdy = [t.to(dev) for t in xs], [t.to(dev) for t in dys]
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    m = n * h * w
    results = {}
    for lin in (1, 0):
        _lib.call('srx_wgrad_force', lin, nsplit)
        nws = L.srx_conv2d_bwd_weight_multi_ws_floats(C.byref(d), nprob)
        assert nws > 0, _lib.last_error()
        ws = torch.empty(nws, device=dev)
        dw, db = base_w.to(dev), base_b.to(dev)
        names = _launched(lambda: _lib.call('srx_conv2d_bwd_weight_multi', C.byref(d), nprob, nprob, arr(gx), arr(gdy),
                                            arr([dw]), accumulate, arr([db]), ws.data_ptr(), nws, _stream()))
        form = '1, 1' if lin and lin_names else '1, 0'
        assert names == [f'wgrad_dma_kernel<{form}> MxNxK={m}x{cout}x{k * k * cin} x{nprob}'], names
        torch.cuda.synchronize()
        assert rel_err(dw, want_w) < 2e-4 and rel_err(db, want_b) < 2e-4, (lin, rel_err(dw, want_w), rel_err(db, want_b))
        results[lin] = (dw, db)
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    return results


@pytest.mark.parametrize('n,h,w,cin,cout,k,nsplit,nprob,accumulate', [
    (2, 9, 20, 64, 64, 3, 0, 1, 0),      # W = 20: rows wrap inside a 32-row chunk; M = 360 not a multiple of 32
    (3, 7, 13, 64, 128, 1, 0, 1, 1),     # 1 x 1, M = 273, accumulate into existing gradients
    (2, 12, 20, 64, 64, 3, 4, 1, 0),     # 4 forced splits of 128 rows: images cut mid-row (20-pixel rows)
    (2, 9, 20, 64, 64, 3, 0, 3, 1),      # grouped: three problems summed into one gradient
    (1, 6, 10, 128, 64, 3, 0, 1, 0),     # one split shorter than a chunk of look-ahead
])
def test_lin_weight_gradient_equals_plain_form(dev, n, h, w, cin, cout, k, nsplit, nprob, accumulate):
    _wgrad(dev, n, h, w, cin, cout, k, nsplit, nprob, accumulate)


def test_lin_weight_gradient_at_the_bit_table_limit(dev):
    """rows_per_split / 32 + 3 == WG_MASKW (768): 765 chunks per split, the largest split the LIN form takes -- and the layer
    whose split is one chunk longer runs the plain form even with LIN asked for."""
    _wgrad(dev, 2, 120, 204, 64, 64, 3, nsplit=2)                    # 2 x 24480 rows: 765 chunks per split
    _wgrad(dev, 2, 70, 350, 64, 64, 3, nsplit=2, lin_names=False)    # 2 x 24500 rows: 766 chunks per split


def test_forced_row_splits_the_rows_cannot_take_are_refused(dev):
    from torchsr_amd import _lib
    L = _lib.lib()
    d = _lib.Conv2dDesc(2, 12, 20, 64, 64, 64, 64, 3, 3, 1, 1, 0, 0, 0.0, 0, 0)   # 480 rows: at most 4 splits of >= 128
    _lib.call('srx_wgrad_force', -1, 5)
    assert L.srx_conv2d_bwd_weight_multi_ws_floats(C.byref(d), 1) == 0 and 'row splits refused' in _lib.last_error()
    x = torch.zeros(2, 12, 20, 64, device=dev)
    dw = torch.full((64, 64, 3, 3), 3.0, device=dev)
    ws = torch.empty(1 << 20, device=dev)
    with pytest.raises(RuntimeError, match='row splits refused'):
        _lib.call('srx_conv2d_bwd_weight', C.byref(d), x.data_ptr(), x.data_ptr(), dw.data_ptr(), 0, None, ws.data_ptr(),
                  ws.numel(), _stream())
    torch.cuda.synchronize()
    assert bool((dw == 3.0).all())
    for bad in ((2, 0), (-1, 65), (0, -1)):
        with pytest.raises(RuntimeError, match='wgrad_force'):
            _lib.call('srx_wgrad_force', *bad)
