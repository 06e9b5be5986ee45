"""Every launch form of gconv.hip on a 4x4 / stride 2 / pad 1 layer (the U-Net critic's conv1..conv3): with K = 4 and pad 1 all four
stride-parity classes of the data gradient have 2 x 2 taps and both borders read one row outside the image -- geometry no 3x3
layer has.  The forced forms (srx_conv2d_force_plan / srx_conv2d_force_s2) of the data gradient and of the forward, and the plans
the cost model cuts for conv1..conv3 at the training step's sizes, each tied to a case that runs its form.  The weight gradient's
4x4 rows live in wgrad_forms.py (rows K1..K3).

Data only.  test_k4s2_forms_cpu.py holds every case to the form it is here for through the host-only planner (srx_conv2d_plan,
srx_wgrad_plan: a planner change that makes a case vacuous fails there, without a GPU); test_k4s2_forms_gpu.py runs the launches
against fp64.  All plans are those of a 256-CU part -- what srx_plan_cus() reports on the MI355X and, by default, without a GPU."""

CUS = 256
K, STRIDE, PAD = 4, 2, 1
ACT_LRELU, SLOPE = 2, 0.2      # the layer's own epilogue (SNConv2d): LeakyReLU(0.2), no bias

# (N, H, W, Cin, Cout, Cin_s).  Output grids of 585, 198, 126 and 30 rows: a ragged last row tile for every BM; channels past Cin
# (Cin_s > Cin) on three of them; 96 and 192 input channels pad to 128 and 192 output columns of the data gradient.
SHAPES = [(3, 26, 30, 64, 128, 64), (2, 22, 18, 128, 256, 136), (2, 14, 18, 96, 256, 100), (1, 10, 12, 192, 96, 196)]
# odd extents: the stride-parity classes lie on different grids (7 x 9, 7 x 8, 6 x 9, 6 x 8): gconv_multi_kernel only
ODD = (2, 13, 17, 64, 128, 64)
NARROW = [(3, 26, 30, 32, 64, 36), (2, 22, 18, 20, 96, 24)]   # Cin <= 32: one 32-column tile
FWD_SHAPES = SHAPES[:2]

# gconv_s2f_kernel's instantiations (precision, BM, BN): test_forced_paths_gpu.S2F_TILES
S2F_TILES = [(0, 144, 128), (0, 144, 64), (0, 128, 128), (0, 128, 64), (0, 64, 64), (1, 128, 128), (1, 128, 64), (1, 64, 64)]
# gconv_multi_kernel forms without a fused twin: (precision, BM, BN, KS)
MULTI_ONLY = [(0, 64, 64, 2), (1, 64, 64, 2), (0, 128, 32, 1), (1, 128, 32, 1)]
# gconv_kernel's tiles (precision, BM, BN, KS asked for, KS of the kernel): test_forced_paths_gpu.SINGLE_TILES
SINGLE_TILES = [(0, 144, 128, 1, 1), (0, 144, 64, 1, 1), (0, 128, 128, 1, 1), (0, 128, 64, 1, 1), (0, 64, 64, 1, 1),
                (0, 64, 64, 2, 2), (0, 64, 32, 1, 2), (0, 128, 32, 1, 1),
                (1, 256, 128, 1, 1), (1, 128, 128, 1, 1), (1, 128, 64, 1, 1), (1, 64, 64, 1, 1), (1, 64, 64, 2, 2),
                (1, 128, 32, 1, 1), (1, 64, 32, 1, 4)]
FWD_SPLITS = (1, 2)            # whole, and every tile cut in two along K (workspace + tail_fixup_kernel)
FWD_BIAS_CASE = (0, 128, 64, 1, 1)   # the one tile that also runs with a bias (both splits, first shape)

FUSED, MULTI = 2, 1            # srx_conv2d_plan's out[5] on a strided data gradient


def desc_fields(shape, prec, act=0, slope=0.0):
    """Conv2dDesc fields: N, H, W, Cin, Cin_s, Cout, Cout_s, KH, KW, stride, pad, shuffle, act, slope, up, precision"""
    n, h, w, cin, cout, cin_s = shape
    return (n, h, w, cin, cin_s, cout, cout, K, K, STRIDE, PAD, 0, act, slope, 0, prec)


def out_size(shape):
    return (shape[1] + 2 * PAD - K) // STRIDE + 1, (shape[2] + 2 * PAD - K) // STRIDE + 1


def padded_cols(c):
    """columns of a packed operand: whole 64-column tiles, 32 for the narrow tile"""
    return (c + 63) // 64 * 64 if c > 32 else 32


def class_rows(shape):
    """GEMM rows of the data gradient's largest stride-parity class"""
    return shape[0] * ((shape[1] + 1) // 2) * ((shape[2] + 1) // 2)


def dgrad_plan(shape, bm, bn, ks, form):
    """srx_conv2d_plan(d, 1): the fused kernel walks the four classes inside one workgroup, gconv_multi_kernel launches one
    workgroup per class and tile"""
    wgs = -(-class_rows(shape) // bm) * (padded_cols(shape[3]) // bn) * (1 if form == FUSED else 4)
    return [bm, bn, 1, wgs, ks, form]


def fwd_plan(shape, bm, bn, split, ks):
    ho, wo = out_size(shape)
    return [bm, bn, split, -(-shape[0] * ho * wo // bm) * (padded_cols(shape[4]) // bn) * split, ks, 0]


def fused_shapes(bn):
    """the layers whose padded columns the tile's divide"""
    return [s for s in SHAPES if padded_cols(s[3]) % bn == 0]


def _sid(shape):
    return '%dx%dx%d.%dto%d' % shape[:5]


# ------------------------------------------------------------------------------------------------------------- data gradient
# A case: the layer, the products' precision, the override (('s2', mode, BM, BN) for srx_conv2d_force_s2 with the plan override
# off, ('plan', BM, BN, KS) for srx_conv2d_force_plan with the fused kernel off), the plan srx_conv2d_plan must report.
DGRAD = []
for _prec, _bm, _bn in S2F_TILES:
    for _s in fused_shapes(_bn):
        DGRAD.append(dict(id='fused.p%d.%dx%d.%s' % (_prec, _bm, _bn, _sid(_s)), shape=_s, prec=_prec, tile=(_bm, _bn), ks=1, form=FUSED,
                          force=('s2', 2, _bm, _bn), plan=dgrad_plan(_s, _bm, _bn, 1, FUSED)))
        DGRAD.append(dict(id='multi.p%d.%dx%d.%s' % (_prec, _bm, _bn, _sid(_s)), shape=_s, prec=_prec, tile=(_bm, _bn), ks=1, form=MULTI,
                          force=('plan', _bm, _bn, 1), plan=dgrad_plan(_s, _bm, _bn, 1, MULTI)))
    if padded_cols(ODD[3]) % _bn == 0:   # the odd-extent layer: the multi twin alone (the fused kernel is refused, below)
        DGRAD.append(dict(id='multi.p%d.%dx%d.%s' % (_prec, _bm, _bn, _sid(ODD)), shape=ODD, prec=_prec, tile=(_bm, _bn), ks=1, form=MULTI,
                          force=('plan', _bm, _bn, 1), plan=dgrad_plan(ODD, _bm, _bn, 1, MULTI)))
for _prec, _bm, _bn, _ks in MULTI_ONLY:
    for _s in (NARROW if _bn == 32 else SHAPES + [ODD]):
        DGRAD.append(dict(id='multi.p%d.%dx%d.ks%d.%s' % (_prec, _bm, _bn, _ks, _sid(_s)), shape=_s, prec=_prec, tile=(_bm, _bn), ks=_ks,
                          form=MULTI, force=('plan', _bm, _bn, _ks), plan=dgrad_plan(_s, _bm, _bn, _ks, MULTI)))
# the fused kernel forced on the odd-extent layer: refused with this message, nothing launched, dx untouched
ODD_FUSED_REFUSED = [dict(shape=ODD, prec=p, force=('s2', 2, bm, bn), message='stride-parity classes')
                     for p, bm, bn in ((0, 128, 64), (1, 64, 64))]

# ------------------------------------------------------------------------------------------------------------------- forward
FWD = []
for _prec, _bm, _bn, _ka, _ks in SINGLE_TILES:
    for _split in FWD_SPLITS:
        for _s in FWD_SHAPES:
            FWD.append(dict(id='fwd.p%d.%dx%d.ks%d.split%d.%s' % (_prec, _bm, _bn, _ks, _split, _sid(_s)), shape=_s, prec=_prec,
                            tile=(_bm, _bn), ks_arg=_ka, ks=_ks, split=_split, plan=fwd_plan(_s, _bm, _bn, _split, _ks)))

# ------------------------------------------------------------------------------------------ the training step's own plans
# conv1..conv3 of the U-Net critic on 128 x 128 crops: (input extent, Cin, Cout); batches 2N = 32 (the discriminator's pair) and
# N = 16 (the generator's adversarial pass).  What the planners answer there, recorded: srx_conv2d_plan(d, 0), srx_conv2d_plan(d, 1)
# and srx_wgrad_plan(d, 1, 1)[:4].  test_k4s2_forms_cpu.py holds the planner to these rows and each row's FORM to a case above
# (forward: precision, tile, KS, split or not; data gradient: precision, tile, KS, fused or multi; weight gradient: slab kernel,
# one split or several -- wgrad_forms.py rows K1..K3), so a plan that moves to a form nothing runs on a 4x4 layer fails there.
STEP_LAYERS = {'conv1': (128, 64, 128), 'conv2': (64, 128, 256), 'conv3': (32, 256, 512)}
STEP_PLANS = [
    # (layer, batch, precision, forward plan, data-gradient plan, weight gradient: kernel, splits, pixels per split, reduce)
    ('conv1', 32, 0, [128, 128, 1, 1024, 1, 0], [128, 64, 1, 1024, 1, 2], [2, 24, 5472, 1]),
    ('conv1', 32, 1, [256, 128, 1, 512, 1, 0], [128, 64, 1, 1024, 1, 2], [4, 32, 4096, 1]),
    ('conv2', 32, 0, [128, 128, 1, 512, 1, 0], [64, 64, 1, 4096, 2, 1], [2, 6, 5472, 1]),
    ('conv2', 32, 1, [256, 128, 1, 256, 1, 0], [128, 128, 1, 1024, 1, 1], [4, 8, 4096, 1]),
    ('conv3', 32, 0, [128, 128, 1, 256, 1, 0], [64, 64, 1, 2048, 2, 1], [2, 3, 2752, 1]),
    ('conv3', 32, 1, [128, 128, 1, 256, 1, 0], [128, 128, 1, 512, 1, 1], [4, 2, 4096, 1]),
    ('conv1', 16, 0, [128, 128, 1, 512, 1, 0], [128, 64, 1, 512, 1, 2], [2, 24, 2752, 1]),
    ('conv1', 16, 1, [256, 128, 1, 256, 1, 0], [128, 64, 1, 512, 1, 2], [4, 32, 2048, 1]),
    ('conv2', 16, 0, [128, 128, 1, 256, 1, 0], [64, 64, 1, 2048, 2, 1], [2, 6, 2752, 1]),
    ('conv2', 16, 1, [128, 128, 1, 256, 1, 0], [128, 128, 1, 512, 1, 1], [4, 8, 2048, 1]),
    ('conv3', 16, 0, [128, 128, 2, 256, 1, 0], [64, 64, 1, 1024, 2, 1], [2, 1, 4096, 1]),
    ('conv3', 16, 1, [128, 64, 1, 256, 1, 0], [128, 128, 1, 256, 1, 1], [4, 2, 2048, 1]),
]


def step_desc_fields(layer, batch, prec):
    extent, cin, cout = STEP_LAYERS[layer]
    return desc_fields((batch, extent, extent, cin, cout, cin), prec, ACT_LRELU, SLOPE)


def fwd_form(prec, plan):
    return (prec, plan[0], plan[1], plan[4], plan[2] > 1)


def dgrad_form(prec, plan):
    return (prec, plan[0], plan[1], plan[4], plan[5])


def wgrad_form(plan):
    return (plan[0], plan[1] > 1)


def by_id(cases):
    return [c['id'] for c in cases]
