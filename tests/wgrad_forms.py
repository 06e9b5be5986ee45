"""Every launch form of the weight gradient (wgrad.hip): the seven slab kernels -- wgrad_kernel<0>, wgrad_dma_kernel<0, 0> / <1, 0> /
<1, 1>, wgrad_kernel<1>, wgrad_rows_bf16_kernel<32> / <16> -- and the two reduce kernels, forced through srx_wgrad_force (row splits)
and srx_wgrad_force_kernels (which kernel) and held to the form by srx_wgrad_plan.  Rows K1..K3: the 4 x 4 / stride 2 / pad 1 layers of
the U-Net critic (test_k4s2_forms_cpu.py ties the training step's own plans for them to these rows).

Data only.  test_wgrad_forms_cpu.py holds every case to the form it is here for through the host-only planner (a planner change that
makes a case vacuous fails there, without a GPU); test_wgrad_forms_gpu.py runs the launches against fp64.

A case: ``geo`` -- the layer (N, H, W: the conv's input, before the x2 upsampling ``up = 2`` fuses into the gather), ``call`` -- the
entry point ('plain' srx_conv2d_bwd_weight, 'multi', 'scaled', 'pair': srx_conv2d_bwd_weight_multi*), ``nprob`` problems of which
``per_out`` are summed into one output, ``force`` -- (nsplit of srx_wgrad_force, then dma, rows, reduce of srx_wgrad_force_kernels),
``expect`` -- what srx_wgrad_plan must answer: (slab kernel, row splits, output pixels per split, reduce kernel, slabs per output).
``model``: the split is the cost model's own (nothing forced, more than one split possible), as a 256-CU part plans it -- what
srx_plan_cus() reports on the MI355X and, by default, without a GPU."""

CUS = 256
WG_MAXP = 72

# srx_wgrad_plan's out[0] and out[3], and the launch records the kernels leave (srx_prof_start_aux)
F32, DMA, WIDE, LIN, BF16, ROWS32, ROWS16 = range(7)
SLAB_KERNELS = {F32: 'wgrad_kernel<0>', DMA: 'wgrad_dma_kernel<0, 0>', WIDE: 'wgrad_dma_kernel<1, 0>', LIN: 'wgrad_dma_kernel<1, 1>',
                BF16: 'wgrad_kernel<1>', ROWS32: 'wgrad_rows_bf16_kernel<32>', ROWS16: 'wgrad_rows_bf16_kernel<16>'}
REDUCE_KERNELS = {0: 'wgrad_reduce_kernel', 1: 'wgrad_reduce_rows_kernel'}
ALL_KERNELS = sorted(SLAB_KERNELS.values()) + sorted(REDUCE_KERNELS.values())


def _geo(n, h, w, cin, cout, k=3, stride=1, pad=None, shuffle=0, up=0, cin_s=None, cout_s=None):
    cin_s = cin_s or (cin + 3) // 4 * 4
    cout_s = cout_s or ((cout // 4 if shuffle else cout) + 3) // 4 * 4
    return dict(n=n, h=h, w=w, cin=cin, cin_s=cin_s, cout=cout, cout_s=cout_s, k=k, stride=stride, pad=k // 2 if pad is None else pad,
                shuffle=shuffle, up=up)


def desc_fields(case):
    """Conv2dDesc fields of a case: N, H, W, Cin, Cin_s, Cout, Cout_s, KH, KW, stride, pad, shuffle, act, slope, up, precision"""
    g = case['geo']
    return (g['n'], g['h'], g['w'], g['cin'], g['cin_s'], g['cout'], g['cout_s'], g['k'], g['k'], g['stride'], g['pad'], g['shuffle'],
            0, 0.0, g['up'], case['precision'])


def out_size(geo):
    """(Ho, Wo) of the conv"""
    uf = 2 if geo['up'] == 2 else 1
    return ((uf * geo['h'] + 2 * geo['pad'] - geo['k']) // geo['stride'] + 1, (uf * geo['w'] + 2 * geo['pad'] - geo['k']) // geo['stride'] + 1)


CASES = []


def _add(id_, geo, kernels, split, nsplit=0, reduce=1, model=False, call='multi', nprob=1, per_out=1, accumulate=0, bias=True,
         scales=None, cin_lo=0, dy_off=0, split_norows=None):
    """One row of the tables below in each of its variants.  kernels: {variant: slab kernel} with the variants 'dma' (fp32, defaults),
    'reg' (fp32, DMA staging off), 'bf16' (bf16 products on a layer the image-row kernel does not take), 'rows' (bf16, defaults) and
    'norows' (bf16, image-row kernel off: wgrad_kernel<1> on the same data, at the model's own split ``split_norows`` -- a split
    counted in image rows means nothing to it).  split: (row splits, output pixels per split)."""
    for variant, kernel in kernels.items():
        ns, sp, md = (0, split_norows, True) if variant == 'norows' else (nsplit, split, model)
        CASES.append(dict(
            id=f'{id_}.{variant}', row=id_, variant=variant, geo=geo, precision=0 if variant in ('dma', 'reg') else 1, call=call,
            nprob=nprob, per_out=per_out, accumulate=accumulate, bias=bias, scales=scales, cin_lo=cin_lo, dy_off=dy_off, model=md,
            force=(ns, 0 if variant == 'reg' else -1, 0 if variant == 'norows' else -1, -1),
            expect=(kernel, sp[0], sp[1], reduce, sp[0] * per_out)))


_GEN = {'dma': DMA, 'reg': F32, 'bf16': BF16}          # a layer whose channels do not come in whole tiles of 64
_GEN_WIDE = {'dma': WIDE, 'reg': F32, 'bf16': BF16}    # ... whose channels do, off the LIN form by stride or PixelShuffle

# ------------------------------------------------------------------------------------------------------------ the generic kernels
# G1: Ck = 24 (not a multiple of 64: dma<0, 0>), 286 pixels in 2 splits of 160: the second starts in the middle of an image row
# (160 = 12 x 13 + 4); 40 columns pad the 64-wide tile
_add('G1.2x11x13.24to40', _geo(2, 11, 13, 24, 40), _GEN, (2, 160), nsplit=2)
# G2: stride 2, 9 x 8 maps, 288 pixels in 2 splits: the WIDE form, LIN ineligible by the stride
_add('G2.4x17x15.s2', _geo(4, 17, 15, 64, 64, stride=2), _GEN_WIDE, (2, 160), nsplit=2)
# G3: PixelShuffle: dy is the shuffled tensor (dD0 / dD1), the bias gradient in the conv's own channel order, both accumulated
_add('G3.2x12x11.shuffle', _geo(2, 12, 11, 64, 256, shuffle=2), _GEN_WIDE, (2, 160), nsplit=2, accumulate=1)
# G4: the fused x2 upsample: the plan is the upsampled layer's (2 x 12 x 22 = 528 pixels in 4 splits of 160, the last one 48)
_add('G4.2x6x11.up2', _geo(2, 6, 11, 64, 32, up=2), _GEN, (4, 160), nsplit=4)
# G5: 1 x 1, one k-tile, 35 pixels: the split is shorter than the four-chunk prefetch
_add('G5.1x5x7.1x1', _geo(1, 5, 7, 64, 8, k=1), _GEN, (1, 64), call='plain')
# G6: output maps smaller than a 32-row chunk: 2 x 2 maps (eight images per chunk, stride 3) and 1 x 1 maps (32 images per chunk)
_add('G6a.40x4x4.s3', _geo(40, 4, 4, 8, 12, stride=3), _GEN, (2, 96), model=True)
_add('G6b.130x3x3.p0', _geo(130, 3, 3, 8, 8, pad=0), _GEN, (2, 96), nsplit=2)
# G7: (a) K = 12800 floats do not fit the row-wise reduction's LDS: wgrad_reduce_kernel with nothing forced; (b) Cin x T = 2304: the
# reduction's tail behind the eight register-held old values, accumulating
_add('G7a.1x6x6.512.5x5', _geo(1, 6, 6, 512, 8, k=5), _GEN, (1, 64), reduce=0, call='plain')
_add('G7b.1x6x6.256', _geo(1, 6, 6, 256, 8), _GEN, (1, 64), call='plain', accumulate=1)
# G8: 64 -> 64 3 x 3 fp32 with bias, accumulating: slabs per output at and above the 64 lanes of the reduction's bias shuffle
_LIN = {'dma': LIN, 'reg': F32}
_add('G8.72slabs.2x48x48', _geo(2, 48, 48, 64, 64), _LIN, (36, 128), nsplit=36, nprob=2, per_out=2, accumulate=1)
_add('G8.64slabs.2x32x32', _geo(2, 32, 32, 64, 64), _LIN, (16, 128), nsplit=16, nprob=4, per_out=4, accumulate=1)
_add('G8.65slabs.2x26x32', _geo(2, 26, 32, 64, 64), _LIN, (13, 128), nsplit=13, nprob=5, per_out=5, accumulate=1)
_add('G8.72probs.1x4x4', _geo(1, 4, 4, 8, 8, k=1), {'dma': DMA, 'reg': F32}, (1, 32), nprob=WG_MAXP, per_out=WG_MAXP, accumulate=1)
# G9: per-output scales on dW and db, four outputs: a dense block's conv reading 64 of the 192-strided buffer's channels
for _acc in (0, 1):
    _add(f'G9.scaled.acc{_acc}', _geo(2, 12, 12, 64, 32, cin_s=192, cout_s=192), _GEN, (3, 96), model=True, call='scaled', nprob=4,
         scales=(1.0, 0.2, 0.04, 3.0), accumulate=_acc)
# G10: paired outputs on the generic kernels (fp32; W = 16 with bf16 products would be the image-row kernel's)
_add('G10.pair.2x9x16', _geo(2, 9, 16, 96, 64, cin_s=192, cout_s=192), {'dma': DMA, 'reg': F32}, (3, 96), model=True, call='pair',
     cin_lo=64, dy_off=64)

# --------------------------------------------------------------------------------------------------------- the image-row kernel
# bf16 products, 3 x 3 / stride 1 / pad 1, 64 output columns; splits count image rows.  Each also runs wgrad_kernel<1> on the same data.
_R16, _R32 = {'rows': ROWS16, 'norows': BF16}, {'rows': ROWS32, 'norows': BF16}
# R1: 15 image rows of 16 pixels.  4 splits: rows 4 / 4 / 4 / 3, every image cut; 15: one row per split, both neighbours outside it
for _ns in (1, 4, 15):
    _add(f'R1.3x5x16.s{_ns}', _geo(3, 5, 16, 32, 64), _R16, (_ns, -(-15 // _ns) * 16), nsplit=_ns, split_norows=(2, 128))
# R2: paired outputs (64 and 96 input channels: three channel groups), two problems, 14 rows in splits of 5 / 5 / 4: 18 workgroups
_add('R2.pair.2x7x32', _geo(2, 7, 32, 96, 64, cin_s=192, cout_s=192), _R32, (3, 160), nsplit=3, call='pair', nprob=2, cin_lo=64,
     dy_off=64, accumulate=1, split_norows=(4, 128))
# R3: images of one and two rows: every row is a top or a bottom border
for _ns in (1, 4):
    _add(f'R3.4x1x16.s{_ns}', _geo(4, 1, 16, 32, 64), _R16, (_ns, 64 // _ns), nsplit=_ns, split_norows=(1, 64))
for _ns in (1, 6):
    _add(f'R3.3x2x32.s{_ns}', _geo(3, 2, 32, 32, 64), _R32, (_ns, 192 // _ns), nsplit=_ns, split_norows=(2, 96))
# R4: per-output scales on the image-row kernel, R1's geometry; the model cuts 8 splits of two rows (the last: one)
_add('R4.scaled.3x5x16', _geo(3, 5, 16, 32, 64), _R16, (8, 32), model=True, call='scaled', nprob=2, scales=(0.04, 1.0), split_norows=(2, 128))

# ------------------------------------------------------------------------------------------- 4 x 4 / stride 2 / pad 1 (even kernel)
# The U-Net critic's conv1..conv3: every output pixel gathers a 4 x 4 patch that starts one row and column outside the image at
# the top / left border and ends one outside at the bottom / right.  WIDE (64 | Cin), F32 (DMA staging off) and BF16 each.
_K4 = dict(k=4, stride=2, pad=1)
# K1: 64 -> 128 on 3 x 26 x 30: 585 output pixels in rows of 15 -- one split, and 2 x 320, 4 x 160, 5 x 128 pixels, every cut
# in the middle of an output row (320 = 21 x 15 + 5, 160 = 10 x 15 + 10, 128 = 8 x 15 + 8); two 64-column tiles
for _ns, _rps in ((1, 608), (2, 320), (4, 160), (5, 128)):
    _add(f'K1.3x26x30.k4s2.s{_ns}', _geo(3, 26, 30, 64, 128, **_K4), _GEN_WIDE, (_ns, _rps), nsplit=_ns)
# K2: 128 -> 256 of a 136-strided buffer, 198 pixels in 2 splits (the second: 70), accumulating into existing gradients
_add('K2.2x22x18.k4s2.acc', _geo(2, 22, 18, 128, 256, cin_s=136, **_K4), _GEN_WIDE, (2, 128), nsplit=2, accumulate=1)
# K3: 96 input channels (not whole 64-channel k-tiles per tap: wgrad_dma_kernel<0, 0>), 126 pixels: one split shorter than its chunks
_add('K3.2x14x18.k4s2.96', _geo(2, 14, 18, 96, 256, cin_s=100, **_K4), _GEN, (1, 128), nsplit=1)

# ------------------------------------------------------------------------------------------------------------------- refusals
# (geometry, precision, forced splits): splits the rows cannot take -- 15 image rows into 10 (8 + 7 are 2 splits), 15 into 16; the
# generic kernels' own rule: 286 pixels into 4 splits of fewer than 128, and the 4 x 4 stride-2 layer's 198 into 4
REFUSED_SPLITS = [(_geo(3, 5, 16, 32, 64), 1, 10), (_geo(3, 5, 16, 32, 64), 1, 16), (_geo(2, 11, 13, 24, 40), 0, 4),
                  (_geo(2, 22, 18, 128, 256, cin_s=136, **_K4), 0, 4)]
BAD_FORCE_KERNELS = [(2, -1, -1), (-1, -2, -1), (-1, -1, 2), (0, 0, 5)]
# srx_wgrad_plan(d, nprob, per_out, .): (nprob, per_out)
BAD_PLAN_ARGS = [(0, 1), (WG_MAXP + 1, 1), (4, 3), (2, 0)]


def by_id(cases):
    return [c['id'] for c in cases]
