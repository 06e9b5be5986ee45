"""Every epilogue of the generic convolution (gconv_kernel, gconv.hip) in every tile form: the case table, the integer operands and the
float64 reference.  gconv_kernel finishes an output through one of three hand-written copies of one piece of arithmetic -- store_tile
of gconv_body (linear or pixel-mapped rows x plain / addend / mask / addend + mask; under bf16 storage bf16 or fp32 out x plain /
mask), the extra 16 x 16 block of the 144-row tiles (XR = 16), and tail_fixup_kernel<BM, BN> behind every K-split tile (BM = 144: a
third, partly filled 64-row pass) -- plus the fold of the KS = 2 / 4 wave groups and the statistics reduce.

Data only.  test_epilogue_forms_cpu.py holds every cell to its form through the host-only planner (a planner change that makes a cell
vacuous fails there, without a GPU) and checks the exactness conditions of the integer operands; test_epilogue_forms_gpu.py runs the
launches: bit for bit on integers, inside a derived bound of float64 on random data.

A cell is (epilogue case, tile form, split).  The tile forms are the (precision, BM, BN, KS asked, KS run) rows of SINGLE_TILES in
test_forced_paths_gpu.py (imported, not copied), each forced with srx_conv2d_force_plan whole (split 1) and cut three ways along K
(split 3: every tile through tail_fixup_kernel).  The bf16-storage cases (srx_conv3x3_bf16s_*) run on the tiles kTiles lists for
gconv_kernel at PR = 2.  MIXED rows run with nothing forced: their expectation is written for a 256-CU plan (whole tiles and K-split
tail tiles in one launch) and they are skipped, never passed, where srx_plan_cus() != CUS.

Not here: PR = 3 (fp16 products, the input conv of fp16 inference) and the BIG forms (above 2^24 pixels) stay with
test_fp16_inference_gpu.py; gconv_multi_kernel and gconv_s2f_kernel stay with test_forced_paths_gpu.py.

Layers: 3x3 / stride 1 / pad 1 at N = 2, 22 x 18, so M = 792 = 5 x 144 + 72 = 6 x 128 + 24 = 12 x 64 + 24 = 3 x 256 + 24: every tile
has a ragged last row tile; K = 9 x 128 is 36 chunks, 12 per split (bf16 storage: 18 chunks of 64, 6 per split).  None is taken by
the 36-pixel row tile, the thin kernels or first3 (no 64 -> 64 layer, no <= 4-channel side)."""
import zlib

from test_forced_paths_gpu import SINGLE_TILES, _tile_args

CUS = 256
MIXED_SKIP = 'a launch of whole and K-split tiles is the cost model\'s choice on a %d-CU plan (srx_plan_cus() = %%d)' % CUS
SLOPE = 0.25      # LeakyReLU of the forward cases; a power of two: an integer times it is a whole number of quarters
MASK_SLOPE = 0.5  # slope of the folded activation backward of srx_conv2d_bwd_data_ex
OUT_SCALE, ADD_SCALE = 0.25, 0.5
SPLITS = (1, 3)
EXACT = 1 << 24   # below it every integer is an fp32 number

# geometry of a layer: N, H, W of the INPUT tensor, Cin, Cin_s, Cout, Cout_s, shuffle, up
LAYERS = {
    'A': (2, 22, 18, 128, 128, 128, 128, 0, 0),    # dense strides
    'B': (2, 22, 18, 128, 128, 96, 104, 0, 0),     # 128 padded columns: a 64-column tile half masked, a 128-column tile a quarter
    'B94': (2, 22, 18, 128, 128, 94, 104, 0, 0),   # ... columns 94 and 95 are written as zero, 96..103 belong to someone else
    'C': (2, 22, 18, 96, 192, 128, 128, 0, 0),     # data gradients: 128 channels contracted into 96 columns of the dense block's wide buffer
    'D': (2, 22, 18, 128, 128, 128, 32, 2, 0),     # PixelShuffle store: the output is [2][44][36][32]
    'E': (2, 11, 9, 128, 128, 128, 128, 0, 2),     # nearest-upsample gather: M is 792 again
    # the cost model's own plans on 256 CUs, whole tiles and K-split tail tiles in one launch
    'M1': (3, 76, 82, 64, 64, 128, 128, 0, 0),     # forward: 128 x 64, 294 tiles = 256 whole + 38 cut 4 ways, the last row tile 8 rows
    'M2': (3, 76, 74, 32, 32, 64, 64, 0, 0),       # data gradient into 32 columns: 64 x 32 (KS 2), 264 tiles = 256 whole + 8 cut 4 ways
}


def out_hw(layer):
    """(Ho, Wo) of the conv's own output grid (M = N Ho Wo rows), before a PixelShuffle store"""
    n, h, w, cin, cin_s, cout, cout_s, sh, up = LAYERS[layer]
    return (2 * h, 2 * w) if up == 2 else (h, w)


def rows(layer):
    ho, wo = out_hw(layer)
    return LAYERS[layer][0] * ho * wo


# ------------------------------------------------------------------------------------------------------------------ epilogue cases
# kind: 'fwd' | 'dgrad'.  entry: the C function.  Forward: bias, act (0 none, 1 ReLU, 2 LeakyReLU SLOPE), stats (BatchNorm partial table),
# resid (srx_conv2d_fwd_residual with OUT_SCALE).  Data gradient: accumulate; addend = (row stride, channels, wide) -- wide: read out of a
# Cin_s-wide buffer --; scales = (out_scale, addend_scale); mask = (c_lo, c_hi, slope).
EPILOGUES = []


def _epi(id_, kind, entry, **kw):
    e = dict(id=id_, layer=id_.split('.')[0], kind=kind, entry=entry, bias=False, act=0, stats=False, resid=False, accumulate=False,
             addend=None, scales=(1.0, 1.0), mask=None)
    assert set(kw) <= set(e), kw
    e.update(kw)
    EPILOGUES.append(e)


for _l in ('A', 'B', 'B94'):
    _epi(f'{_l}.lrelu', 'fwd', 'srx_conv2d_fwd', bias=True, act=2)
_epi('A.nobias', 'fwd', 'srx_conv2d_fwd')
for _l in ('A', 'B'):
    _epi(f'{_l}.resid', 'fwd', 'srx_conv2d_fwd_residual', bias=True, act=2, resid=True)
    _epi(f'{_l}.stats', 'fwd', 'srx_conv2d_fwd', stats=True)
    _epi(f'{_l}.stats_bias', 'fwd', 'srx_conv2d_fwd', stats=True, bias=True)
_epi('D.shuffle', 'fwd', 'srx_conv2d_fwd', bias=True, act=2)
_epi('E.up', 'fwd', 'srx_conv2d_fwd', bias=True, act=1)
for _l in ('A', 'C'):
    _epi(f'{_l}.dplain', 'dgrad', 'srx_conv2d_bwd_data')
    _epi(f'{_l}.dacc', 'dgrad', 'srx_conv2d_bwd_data', accumulate=True)
_epi('C.dadd', 'dgrad', 'srx_conv2d_bwd_data_add', addend=(192, 96, False))
_epi('C.dact', 'dgrad', 'srx_conv2d_bwd_data_act', mask=(0, 96, SLOPE))
_epi('C.dact_acc', 'dgrad', 'srx_conv2d_bwd_data_act', mask=(64, 96, SLOPE), accumulate=True)
# addend_channels 64 < Cin: columns 64..95 take no addend
_epi('C.dex64', 'dgrad', 'srx_conv2d_bwd_data_ex', addend=(64, 64, False), scales=(OUT_SCALE, ADD_SCALE), mask=(64, 96, MASK_SLOPE))
_epi('C.dex192', 'dgrad', 'srx_conv2d_bwd_data_ex', addend=(192, 64, True), scales=(OUT_SCALE, ADD_SCALE), mask=(64, 96, MASK_SLOPE))

# bf16 storage (layer A, precision = 1): out16 = the output tensor is bf16; relu: forward ReLU / data gradient relu_out mask
BF16S = []
for _o in (16, 32):
    BF16S.append(dict(id=f'S.fwd{_o}', layer='A', kind='fwd', out16=_o == 16, relu=True, bias=True))
    BF16S.append(dict(id=f'S.d{_o}', layer='A', kind='dgrad', out16=_o == 16, relu=False, bias=False))
    BF16S.append(dict(id=f'S.dmask{_o}', layer='A', kind='dgrad', out16=_o == 16, relu=True, bias=False))
# the tiles kTiles lists for gconv_kernel at PR = 2 -- the bf16-product rows of SINGLE_TILES less the 32-column tiles, which exist with
# bf16 products but not with bf16 storage: forced, they are refused by run_gconv before anything is launched
BF16S_TILES = [t[1:] for t in SINGLE_TILES if t[0] == 1 and t[2] != 32]
BF16S_REFUSED = [t[1:] for t in SINGLE_TILES if t[0] == 1 and t[2] == 32]

# the cost model's own plan (force = None) on CUS compute units: (epilogue id, which, plan, whole tiles, cut tiles)
MIXED = [
    dict(id='M1.lrelu', layer='M1', kind='fwd', entry='srx_conv2d_fwd', bias=True, act=2, stats=False, tile=(0, 128, 64, 1, 1),
         plan=[128, 64, 4, 408, 1, 0], full=256, tail=38),
    dict(id='M1.stats_bias', layer='M1', kind='fwd', entry='srx_conv2d_fwd', bias=True, act=0, stats=True, tile=(0, 128, 64, 1, 1),
         plan=[128, 64, 4, 408, 1, 0], full=256, tail=38),
    dict(id='M2.dact_acc', layer='M2', kind='dgrad', entry='srx_conv2d_bwd_data_act', mask=(0, 32, SLOPE), accumulate=True,
         tile=(0, 64, 32, 1, 2), plan=[64, 32, 4, 288, 2, 0], full=256, tail=8),
]
for _m in MIXED:
    for _k, _v in dict(bias=False, act=0, stats=False, resid=False, accumulate=False, addend=None, scales=(1.0, 1.0), mask=None).items():
        _m.setdefault(_k, _v)

# cells that cannot exist, with the reason the library gives (the planner refuses the first two; the third runs unsplit)
IMPOSSIBLE = [
    dict(tile=(1, 144, 128), why='no 144-row tile with bf16 products'),
    dict(tile=(1, 144, 64), why='no 144-row tile with bf16 products'),
    dict(tile=(0, 256, 128), why='no 256-row tile with fp32 products'),
    dict(epilogue='D.shuffle', split=3, why='a pixel-mapped output is not linear in the tile: the shuffled store runs unsplit'),
]

# random data: one row per epilogue family on three forms each (bf16 storage: the two it has)
RANDOM_FORMS = [(0, 144, 128, 1, 1), (0, 64, 64, 2, 2), (1, 256, 128, 1, 1)]
RANDOM_IDS = ['A.lrelu', 'A.stats_bias', 'C.dex64']
RANDOM_BF16S_IDS = ['S.fwd16']
RANDOM_BF16S_FORMS = [(64, 64, 2, 2), (256, 128, 1, 1)]


def kernel_name(prec, bm, bn, ks):
    """The instantiation a tile form launches, as the launch recorder spells it (prec: the kernel's PR, 2 under bf16 storage)"""
    head, _, wm, wn, xr = _tile_args(bm, bn)
    if bm == 256:
        wn = 64   # (the 256-row tile: 64 x 64 per wave)
    return f'gconv_kernel<{head}, {bn}, {wm}, {wn}, {ks}, {xr}, {prec}>'


# every gconv_kernel instantiation kTiles lists under F_GCONV for PR 0, 1 and 2 (held here as names, not parsed out of gconv.hip)
ALL_INSTANTIATIONS = [
    'gconv_kernel<128, 128, 64, 32, 1, 16, 0>', 'gconv_kernel<128, 64, 32, 32, 1, 16, 0>', 'gconv_kernel<128, 128, 64, 32, 1, 0, 0>',
    'gconv_kernel<128, 64, 32, 32, 1, 0, 0>', 'gconv_kernel<64, 64, 32, 32, 1, 0, 0>', 'gconv_kernel<64, 64, 32, 32, 2, 0, 0>',
    'gconv_kernel<128, 32, 32, 32, 1, 0, 0>', 'gconv_kernel<64, 32, 32, 32, 2, 0, 0>',
    'gconv_kernel<128, 128, 64, 32, 1, 0, 1>', 'gconv_kernel<128, 64, 32, 32, 1, 0, 1>', 'gconv_kernel<64, 64, 32, 32, 1, 0, 1>',
    'gconv_kernel<64, 64, 32, 32, 2, 0, 1>', 'gconv_kernel<128, 32, 32, 32, 1, 0, 1>', 'gconv_kernel<64, 32, 32, 32, 4, 0, 1>',
    'gconv_kernel<256, 128, 64, 64, 1, 0, 1>',
    'gconv_kernel<128, 128, 64, 32, 1, 0, 2>', 'gconv_kernel<128, 64, 32, 32, 1, 0, 2>', 'gconv_kernel<64, 64, 32, 32, 1, 0, 2>',
    'gconv_kernel<64, 64, 32, 32, 2, 0, 2>', 'gconv_kernel<256, 128, 64, 64, 1, 0, 2>',
]


def epilogue(id_):
    return next(e for e in EPILOGUES + BF16S + MIXED if e['id'] == id_)


def tile_id(t):
    return 'x'.join(map(str, t))


def cells():
    """Every (epilogue, tile form, split) cell of the forced table"""
    return [(e, t, s) for e in EPILOGUES for t in SINGLE_TILES for s in SPLITS if not (e['id'] == 'D.shuffle' and s != 1)]


def columns(e):
    """(contracted channels, output columns Cn, columns the launch may store Cs, row stride of the output, padded columns)"""
    n, h, w, cin, cin_s, cout, cout_s, sh, up = LAYERS[e['layer']]
    k, cn, ld = (cout, cin, cin_s) if e['kind'] == 'dgrad' else (cin, cout, cout_s)
    return k, cn, -(-cn // 4) * 4, ld, (32 if cn <= 32 else -(-cn // 64) * 64)


def desc_fields(e, prec):
    """Conv2dDesc fields: N, H, W, Cin, Cin_s, Cout, Cout_s, KH, KW, stride, pad, shuffle, act, slope, up, precision"""
    n, h, w, cin, cin_s, cout, cout_s, sh, up = LAYERS[e['layer']]
    act = e.get('act', 0)
    return (n, h, w, cin, cin_s, cout, cout_s, 3, 3, 1, 1, sh, act, SLOPE if act == 2 else 0.0, up, prec)


def expect(e, tile, split):
    """What a forced cell must plan: (srx_conv2d_plan's answer, workspace floats, statistics rows, the recorded launch)"""
    prec, bm, bn, ks_arg, ks = tile
    k, cn, cs, ld, cnp = columns(e)
    m = rows(e['layer'])
    if LAYERS[e['layer']][7]:
        split = 1          # the shuffled store runs unsplit, whatever is asked
    tiles = -(-m // bm) * (cnp // bn)
    kchunks = 9 * (-(-k // 4) * 4) // 32
    assert kchunks % split == 0
    return ([bm, bn, split, tiles * split, ks, 0], 0 if split == 1 else tiles * split * bm * bn, -(-m // bm),
            f'{kernel_name(prec, bm, bn, ks)} MxNxK={m}x{cn}x{9 * (-(-k // 4) * 4)}')


def expect_bf16s(e, tile, split):
    """(workspace floats, the recorded launch) of a bf16-storage cell; K counts bf16 values"""
    bm, bn, ks_arg, ks = tile
    tiles = -(-792 // bm) * (128 // bn)
    return (0 if split == 1 else tiles * split * bm * bn), f'{kernel_name(2, bm, bn, ks)} MxNxK=792x128x1152'


# ------------------------------------------------------------------------------------------------------------------------ operands
def int_operands(layer):
    """The integer operands of a layer's exact checks (numpy int8, NCHW / OIHW; the tests cast them), seeded by the layer's name and
    shared by every case on it: ``x``, ``dy`` (on the conv's output grid), ``resid`` (laid out like the forward output), ``addend``,
    ``base`` (what an accumulating data gradient finds in dx) and ``maskt`` (the activation output whose sign is the mask; about a
    fifth of it exactly 0, which takes the slope) in {-2..2}; ``bias`` in {-4..4}; ``w`` in {-1, 0, 1}, a quarter of it non-zero.
    With slopes and scales 0.25 and 0.5 every value of every epilogue is a whole number of sixteenths."""
    import numpy as np
    n, h, w, cin, cin_s, cout, cout_s, sh, up = LAYERS[layer]
    ho, wo = out_hw(layer)
    rng = np.random.default_rng(zlib.crc32(layer.encode()))
    i8 = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape, dtype=np.int8)  # noqa: E731
    d = dict(x=i8(-2, 2, (n, cin, h, w)), dy=i8(-2, 2, (n, cout, ho, wo)), bias=i8(-4, 4, (cout,)))
    keep = rng.random((cout, cin, 3, 3), dtype=np.float32) < 0.25
    d['w'] = (i8(-1, 1, (cout, cin, 3, 3)) * keep).astype(np.int8)
    d['resid'] = i8(-2, 2, (n, cout // 4, 2 * ho, 2 * wo) if sh else (n, cout, ho, wo))
    for name in ('addend', 'base', 'maskt'):
        d[name] = i8(-2, 2, (n, cin, h, w))
    return d


def random_operands(layer, bf16):
    """N(0, 1) operands of the same shapes (torch fp32, seeded by the layer); bf16: x, dy, w and maskt rounded to bf16 first"""
    import torch
    shapes = {k: v.shape for k, v in int_operands(layer).items()}
    g = torch.Generator().manual_seed(zlib.crc32(layer.encode()) + (1 if bf16 else 0))
    d = {k: torch.randn(tuple(s), generator=g) for k, s in shapes.items()}
    if bf16:
        for k in ('x', 'dy', 'w', 'maskt'):
            d[k] = d[k].bfloat16().float()
    return d


# ----------------------------------------------------------------------------------------------------------------- fp64 reference
def conv_ref(layer, kind, ops):
    """Once per data row and kind: the float64 convolution without bias (NCHW, the conv's own output grid) -- conv2d of the
    (nearest-upsampled) input, or conv2d_input of dy.  ``ops``: tensors or arrays of the operands."""
    import torch
    import torch.nn.functional as TF
    n, h, w, cin, cin_s, cout, cout_s, sh, up = LAYERS[layer]
    t = lambda v: torch.as_tensor(v).double()  # noqa: E731
    if kind == 'dgrad':
        return torch.nn.grad.conv2d_input((n, cin, h, w), t(ops['w']), t(ops['dy']), stride=1, padding=1)
    x = t(ops['x'])
    if up == 2:
        x = TF.interpolate(x, scale_factor=2, mode='nearest')
    return TF.conv2d(x, t(ops['w']), None, 1, 1)


def abs_ops(ops):
    import torch
    return {k: torch.as_tensor(v).double().abs() for k, v in ops.items()}


def reference(e, ops, conv):
    """The case's epilogue on ``conv`` (conv_ref's result), in plain float64 torch: (output, pre-activation) as NCHW tensors of the
    layer's real channels (PixelShuffle applied to the output).  An activation is v > 0 ? v : v * slope as the library defines it
    (ReLU: slope 0, so a negative value becomes -0), the mask is applied where the activation output is NOT > 0."""
    import torch
    import torch.nn.functional as TF
    t = lambda v: torch.as_tensor(v).double()  # noqa: E731
    n, h, w, cin, cin_s, cout, cout_s, sh, up = LAYERS[e['layer']]
    pre = conv + 0.0     # (an exact zero of the convolution is +0, as a sum that starts at +0 leaves it)
    if e['kind'] == 'fwd':
        if e['bias']:
            pre = pre + t(ops['bias']).view(1, -1, 1, 1)
        act = e.get('act', 1 if e.get('relu') else 0)
        y = pre if act == 0 else torch.where(pre > 0, pre, pre * (0.0 if act == 1 else SLOPE))
        if e.get('resid'):
            y = y * OUT_SCALE + t(ops['resid'])
        if sh:
            y = TF.pixel_shuffle(y, 2)
        return y, pre
    osc, asc = e.get('scales', (1.0, 1.0))
    y = pre * osc if e.get('addend') else pre
    if e.get('accumulate'):
        y = y + t(ops['base'])
    if e.get('addend'):
        ch = e['addend'][1]
        add = torch.zeros_like(y)
        add[:, :ch] = t(ops['addend'])[:, :ch] * asc
        y = y + add
    mask = e.get('mask') or ((0, cin, 0.0) if e.get('relu') else None)
    if mask:
        lo, hi, slope = mask
        y = y.clone()
        y[:, lo:hi] = torch.where(t(ops['maskt'])[:, lo:hi] > 0, y[:, lo:hi], y[:, lo:hi] * slope)
    return y, pre


def stat_table(pre, bm):
    """[row tiles][C][2]: float64 (sum, sum of squares) of the pre-activation over each row tile's valid rows, one row per BM rows of
    the M = N Ho Wo pixels"""
    import torch
    c = pre.shape[1]
    p = pre.permute(0, 2, 3, 1).reshape(-1, c)
    m = p.shape[0]
    nt = -(-m // bm)
    p = torch.cat([p, torch.zeros((nt * bm - m, c), dtype=p.dtype)]).view(nt, bm, c)
    return torch.stack([p.sum(1), p.square().sum(1)], dim=2)
