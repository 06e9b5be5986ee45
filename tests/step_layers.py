"""The conv problems of the batch-16 SRGAN GAN step (BASELINE configs[1], the bench.py headline), shared by the tests that
exercise them at the step's own sizes (test_ops_gpu.py, test_step_layers_gpu.py), and below them the non-convolution problems
of the SRGAN and ESRGAN steps (STEP_OPS: test_step_ops_gpu.py, test_cpu.py)."""
from torchsr_amd._lib import ACT_LRELU, ACT_RELU

FULL_SIZE_LAYERS = [
    # every distinct conv shape of the batch-16 SRGAN GAN step (BASELINE configs[1]): N, H, W, Cin, Cout, k, s, p, shuffle
    (16, 24, 24, 64, 64, 3, 1, 1, 0), (16, 24, 24, 3, 64, 9, 1, 4, 0), (16, 24, 24, 64, 256, 3, 1, 1, 2),
    (16, 48, 48, 64, 256, 3, 1, 1, 2), (16, 96, 96, 64, 3, 9, 1, 4, 0), (16, 96, 96, 3, 64, 3, 1, 1, 0),
    (16, 96, 96, 64, 64, 3, 2, 1, 0), (16, 48, 48, 64, 128, 3, 1, 1, 0), (16, 48, 48, 128, 128, 3, 2, 1, 0),
    (16, 24, 24, 128, 256, 3, 1, 1, 0), (16, 24, 24, 256, 256, 3, 2, 1, 0), (16, 12, 12, 256, 512, 3, 1, 1, 0),
    (16, 12, 12, 512, 512, 3, 2, 1, 0), (32, 96, 96, 64, 64, 3, 1, 1, 0), (32, 48, 48, 128, 128, 3, 1, 1, 0),
    (32, 24, 24, 256, 256, 3, 1, 1, 0), (32, 12, 12, 512, 512, 3, 1, 1, 0), (32, 6, 6, 512, 512, 3, 1, 1, 0),
]


def _case(id_, shape, kernels, **kw):
    return dict(id=id_, shape=shape, kernels=kernels, **kw)


# Each entry: one layer as the step calls it.  shape = (N, H, W, Cin, Cout, k, stride, pad); flags as layers.Conv2d takes them
# (act / slope / shuffle / bias), stats: the BatchNorm partial sums from the conv epilogue, in_act: the input is the output of
# a ReLU / LeakyReLU whose backward this layer's data gradient applies, dx / dw: which gradients the step takes there.
# kernels: launch-name prefixes the case must produce (the form it is there to test).
_D = [  # discriminator: 3 -> 64 (+LeakyReLU), then conv + BatchNorm + LeakyReLU blocks; pair pass N = 32, adversarial N = 16
    ('d2', 96, 64, 64, 2), ('d5', 96 // 2, 64, 128, 1), ('d8', 48, 128, 128, 2), ('d11', 24, 128, 256, 1),
    ('d14', 24, 256, 256, 2), ('d17', 12, 256, 512, 1), ('d20', 12, 512, 512, 2)]
_VGG = [  # VGG19 features[:36], every distinct shape: source + target forward at N = 32, the source's data gradient at N = 16
    ('v2', 96, 64, 64), ('v5', 48, 64, 128), ('v7', 48, 128, 128), ('v10', 24, 128, 256), ('v12', 24, 256, 256),
    ('v19', 12, 256, 512), ('v21', 12, 512, 512), ('v28', 6, 512, 512)]

STEP_CONVS = [
    # generator
    _case('g.conv1', (16, 24, 24, 3, 64, 9, 1, 4), ('gconv_kernel', 'thin_wgrad_kernel<9, 9, 3, 1>'), bias=True, dx=False),
    dict(id='g.tower', tower=(16, 24, 24, 64, 3), kernels=('rt36_conv3x3_c64_kernel<1, BNL>', 'rt36_conv3x3_c64_kernel<1, BNR, BNB>',
                                                           'wgrad_dma_kernel<1, 1>')),
    _case('g.conv2', (16, 24, 24, 64, 64, 3, 1, 1), ('rt36_conv3x3_c64_kernel<1>',), stats=True),
    _case('g.up1', (16, 24, 24, 64, 256, 3, 1, 1), ('wino_kernel', 'gconv_kernel', 'wgrad_dma_kernel'), bias=True, shuffle=2),
    _case('g.up2', (16, 48, 48, 64, 256, 3, 1, 1), ('wino_kernel', 'gconv_kernel', 'wgrad_dma_kernel'), bias=True, shuffle=2),
    _case('g.conv3', (16, 96, 96, 64, 3, 9, 1, 4), ('thin_fwd2_kernel<9, 3>', 'thin_wgrad_kernel<9, 9, 3, -1>'), bias=True),
    # discriminator, first layer (LeakyReLU in the epilogue; its backward folded into d2's data gradient)
    _case('d0.pair', (32, 96, 96, 3, 64, 3, 1, 1), ('first3x3_fwd_kernel', 'thin_wgrad_kernel<3, 3, 1, 1>'), bias=True,
          act=ACT_LRELU, slope=0.2, dx=False),
    _case('d0.adv', (16, 96, 96, 3, 64, 3, 1, 1), ('first3x3_fwd_kernel',), bias=True, act=ACT_LRELU, slope=0.2, dw=False),
]
for _id, _hw, _ci, _co, _s in _D:
    _fold = 'lrelu' if _id == 'd2' else None
    for _tag, _n, _dw in (('pair', 32, True), ('adv', 16, False)):
        STEP_CONVS.append(_case(f'{_id}.{_tag}', (_n, _hw, _hw, _ci, _co, 3, _s, 1),
                                ('wino_kernel',) if _s == 1 else ('gconv_kernel',), stats=True, in_act=_fold, dw=_dw))
STEP_CONVS.append(_case('v0.n32', (32, 96, 96, 3, 64, 3, 1, 1), ('first3x3_fwd_kernel',), bias=True, act=ACT_RELU, dx=False, dw=False))
STEP_CONVS.append(_case('v0.n16', (16, 96, 96, 3, 64, 3, 1, 1), ('first3x3_fwd_kernel', 'thin_fwd2_kernel<3, 3>'), bias=True, act=ACT_RELU, dw=False))
for _id, _hw, _ci, _co in _VGG:
    STEP_CONVS.append(_case(f'{_id}.n32', (32, _hw, _hw, _ci, _co, 3, 1, 1), ('wino_kernel',), bias=True, act=ACT_RELU,
                            in_act='relu', dx=False, dw=False))
    STEP_CONVS.append(_case(f'{_id}.n16', (16, _hw, _hw, _ci, _co, 3, 1, 1), ('gconv_kernel',) if _hw == 6 else ('wino_kernel',), bias=True, act=ACT_RELU,
                            in_act='relu', dw=False))
# the perceptual loss's last VGG19 layers through the frozen stack: forward at source + target, data gradient of the source
STEP_CONVS.append(dict(id='v28.stack', stack=(16, 6, 6, 512, 512), kernels=('wino_kernel<32> MxNxK=576x512x4608',)))


# ---------------------------------------------------------------------------------------------------------------------------
# The conv problems of the batch-16 ESRGAN GAN step (BASELINE configs[3]: 23 RRDBs, 128 x 128 crops; bf16 products in the
# quoted configuration, exact fp32 with --disable-amp), read off the model code and one eager step per precision under
# prof_launches.  Row format of STEP_CONVS plus: up (nearest x2 upsampling in the conv's gather; shape holds the INPUT size),
# fold_out (the step hands this layer's activation backward to its consumer: ActFold, act_bwd_folded), precisions (in which
# precision the step makes the call); kernels: launch-name prefixes per precision, filled in from _EK below the table.  exact: outputs the bf16 step computes in
# exact fp32 (the layers with a 3-channel side: oracle.srgan._ConvBF16, thin_in / thin_out).
def _ecase(id_, shape, precisions=('fp32', 'bf16'), **kw):
    return dict(id=id_, shape=shape, precisions=precisions, **kw)


_ED = [  # discriminator conv + BatchNorm layers: id, input H = W, Cin, Cout, stride
    ('d2', 128, 64, 64, 2), ('d5', 64, 64, 128, 1), ('d8', 64, 128, 128, 2), ('d11', 32, 128, 256, 1), ('d14', 32, 256, 256, 2),
    ('d17', 16, 256, 512, 1), ('d20', 16, 512, 512, 2), ('d23', 8, 512, 512, 1), ('d26', 8, 512, 512, 2)]
_EVGG = [  # VGG19 features[:36] at 128 x 128, every distinct shape behind the first layer: id, H = W, Cin, Cout
    ('v2', 128, 64, 64), ('v5', 64, 64, 128), ('v7', 64, 128, 128), ('v10', 32, 128, 256), ('v12', 32, 256, 256),
    ('v19', 16, 256, 512), ('v21', 16, 512, 512), ('v28', 8, 512, 512)]

_LR = dict(act=ACT_LRELU, slope=0.2)
ESRGAN_STEP_CONVS = [
    # generator (esrgan/generator.py): 3 -> 64 on the 32 x 32 crops, the trunk's tail, two nearest-x2 gather convs, 64 -> 3
    _ecase('g.conv1', (16, 32, 32, 3, 64, 3, 1, 1), bias=True, dx=False, exact=('dx', 'dW')),
    _ecase('g.conv2', (16, 32, 32, 64, 64, 3, 1, 1), bias=True),
    _ecase('g.up1', (16, 32, 32, 64, 64, 3, 1, 1), bias=True, up=2, **_LR),
    _ecase('g.up2', (16, 64, 64, 64, 64, 3, 1, 1), bias=True, up=2, fold_out=True, **_LR),
    _ecase('g.conv3', (16, 128, 128, 64, 64, 3, 1, 1), bias=True, in_act='lrelu', **_LR),
    _ecase('g.conv4', (16, 128, 128, 64, 3, 3, 1, 1), bias=True, exact=('y', 'dW')),
]
# the dense blocks (functional._RRDBTrunk, 16 x 32 x 32 pixels, 64 + 4 x 32 channels in 192-strided buffers).  Exact fp32: one
# launch per conv forward and per data gradient (dense: conv k + 1 with the trunk's descriptors and epilogues); bf16: the fused
# block kernels (CONV_LAUNCHES_TESTED_ELSEWHERE).  Both: the weight gradients as the trunk queues them -- conv1 + conv2 and
# conv3 + conv4 as pairs, conv5 with the block's scale -- reading 64 / 96, 128 / 160 and 192 channels, bias gradients riding along.
for _k in range(5):
    ESRGAN_STEP_CONVS.append(dict(id=f'g.rdb.conv{_k + 1}', dense=_k, nhw=(16, 32, 32), precisions=('fp32',)))
for _lo in (0, 2):
    ESRGAN_STEP_CONVS.append(dict(id=f'g.rdb.w{_lo + 1}{_lo + 2}', pair=_lo, nhw=(16, 32, 32), precisions=('fp32', 'bf16')))
ESRGAN_STEP_CONVS.append(dict(id='g.rdb.w5', scaled=True, nhw=(16, 32, 32), precisions=('fp32', 'bf16')))
# discriminator (esrgan/discriminator.py, 128 x 128 crops): the pair pass on real + fake (N = 32, weight gradients), the
# adversarial pass on the fakes (N = 16, data gradients only).  The first layer's LeakyReLU backward rides in d2's data gradient.
ESRGAN_STEP_CONVS += [
    _ecase('d0.pair', (32, 128, 128, 3, 64, 3, 1, 1), bias=True, fold_out=True, dx=False,
           exact=('dx', 'dW'), **_LR),
    _ecase('d0.adv', (16, 128, 128, 3, 64, 3, 1, 1), bias=True, fold_out=True, dw=False,
           exact=('dx', 'dW'), **_LR),
]
for _id, _hw, _ci, _co, _s in _ED:
    for _tag, _n, _dw in (('pair', 32, True), ('adv', 16, False)):
        ESRGAN_STEP_CONVS.append(_ecase(f'{_id}.{_tag}', (_n, _hw, _hw, _ci, _co, 3, _s, 1), stats=True, in_act='lrelu' if _id == 'd2' else None, dw=_dw))
# VGG19 features[:36] (srgan/loss.py): source + target forward at N = 32, the source's data gradient at N = 16.  Exact fp32:
# layer by layer as in STEP_CONVS; bf16: the frozen stack keeps its inner activations as bf16 (functional.
# _stack_conv_fwd) -- bf16s = (H = W, Cin, Cout), out16: the forms of the forward output at this shape (0: fp32, in front of a
# pool and at the end; 1: bf16), dx16: the data gradient's (fp32 only for the layer behind the 3 -> 64 one), masked: the layer's
# input is a conv's ReLU output whose backward the data gradient applies (behind a pool the pool's backward has it)
ESRGAN_STEP_CONVS += [
    _ecase('v0.n32', (32, 128, 128, 3, 64, 3, 1, 1), precisions=('fp32',), bias=True, act=ACT_RELU, dx=False, dw=False),
    _ecase('v0.n16', (16, 128, 128, 3, 64, 3, 1, 1), precisions=('fp32',), bias=True, act=ACT_RELU, dw=False),
    dict(id='v0.stack', first3=128, precisions=('bf16',)),
]
for _id, _hw, _ci, _co in _EVGG:
    ESRGAN_STEP_CONVS.append(_ecase(f'{_id}.n32', (32, _hw, _hw, _ci, _co, 3, 1, 1), precisions=('fp32',), bias=True, act=ACT_RELU,
                                    in_act='relu', dx=False, dw=False))
    ESRGAN_STEP_CONVS.append(_ecase(f'{_id}.n16', (16, _hw, _hw, _ci, _co, 3, 1, 1), precisions=('fp32',), bias=True, act=ACT_RELU,
                                    in_act='relu', dw=False))
    # (v2, v7: in front of a pool; v12, v21, v28: three or four layers of the shape, the last one in front of a pool / the end)
    ESRGAN_STEP_CONVS.append(dict(id=f'{_id}.stack', bf16s=(_hw, _ci, _co), out16={'v2': (0,), 'v7': (0,), 'v5': (1,), 'v10': (1,), 'v19': (1,)}.get(_id, (1, 0)),
                                  dx16=0 if _id == 'v2' else 1, masked=_id not in ('v5', 'v10', 'v19'), precisions=('bf16',)))

# per row and precision: the launches (kernel, template arguments) the row must produce, read off a run on an MI355X
_EK = {'g.conv1': {'fp32': ('first3x3_fwd_kernel<0>', 'thin_wgrad_kernel<3, 3, 1, 1>'),
             'bf16': ('first3x3_fwd_kernel<1>', 'thin_wgrad_kernel<3, 3, 1, 1>')},
 'g.conv2': {'fp32': ('wgrad_dma_kernel<1, 1>', 'wgrad_reduce_rows_kernel', 'wino_kernel<32>'),
             'bf16': ('gconv_kernel<64, 64, 32, 32, 2, 0, 1>', 'wgrad_reduce_rows_kernel', 'wgrad_rows_bf16_kernel<32>')},
 'g.up1': {'fp32': ('gconv_kernel<128, 64, 32, 32, 1, 0, 0>', 'wgrad_dma_kernel<1, 1>', 'wgrad_reduce_rows_kernel'),
           'bf16': ('gconv_kernel<128, 64, 32, 32, 1, 0, 1>', 'wgrad_kernel<1>', 'wgrad_reduce_rows_kernel')},
 'g.up2': {'fp32': ('gconv_kernel<128, 64, 32, 32, 1, 0, 0>', 'wgrad_dma_kernel<1, 1>', 'wgrad_reduce_rows_kernel'),
           'bf16': ('gconv_kernel<128, 64, 32, 32, 1, 0, 1>', 'wgrad_kernel<1>', 'wgrad_reduce_rows_kernel')},
 'g.conv3': {'fp32': ('gconv_kernel<128, 64, 32, 32, 1, 0, 0>', 'wgrad_dma_kernel<1, 1>', 'wgrad_reduce_rows_kernel'),
             'bf16': ('gconv_kernel<128, 64, 32, 32, 1, 0, 1>', 'wgrad_kernel<1>', 'wgrad_reduce_rows_kernel')},
 'g.conv4': {'fp32': ('gconv_kernel<128, 64, 32, 32, 1, 0, 0>', 'thin_fwd2_kernel<3, 3>', 'thin_wgrad_kernel<3, 3, 1, -1>'),
             'bf16': ('gconv_kernel<128, 64, 32, 32, 1, 0, 1>', 'thin_fwd2_kernel<3, 3>', 'thin_wgrad_kernel<3, 3, 1, -1>')},
 'g.rdb.conv1': {'fp32': ('gconv_kernel<64, 32, 32, 32, 2, 0, 0>', 'gconv_kernel<64, 64, 32, 32, 2, 0, 0>')},
 'g.rdb.conv2': {'fp32': ('gconv_kernel<128, 64, 32, 32, 1, 0, 0>', 'gconv_kernel<64, 32, 32, 32, 2, 0, 0>')},
 'g.rdb.conv3': {'fp32': ('gconv_kernel<128, 64, 32, 32, 1, 0, 0>', 'gconv_kernel<64, 32, 32, 32, 2, 0, 0>')},
 'g.rdb.conv4': {'fp32': ('gconv_kernel<128, 64, 32, 32, 1, 0, 0>', 'gconv_kernel<64, 32, 32, 32, 2, 0, 0>')},
 'g.rdb.conv5': {'fp32': ('gconv_kernel<128, 64, 32, 32, 1, 0, 0>',)},
 'g.rdb.w12': {'fp32': ('wgrad_dma_kernel<0, 0>', 'wgrad_reduce_rows_kernel'),
               'bf16': ('wgrad_reduce_rows_kernel', 'wgrad_rows_bf16_kernel<32>')},
 'g.rdb.w34': {'fp32': ('wgrad_dma_kernel<0, 0>', 'wgrad_reduce_rows_kernel'),
               'bf16': ('wgrad_reduce_rows_kernel', 'wgrad_rows_bf16_kernel<32>')},
 'g.rdb.w5': {'fp32': ('wgrad_dma_kernel<1, 1>', 'wgrad_reduce_rows_kernel'),
              'bf16': ('wgrad_reduce_rows_kernel', 'wgrad_rows_bf16_kernel<32>')},
 'd0.pair': {'fp32': ('first3x3_fwd_kernel<0>', 'thin_wgrad_kernel<3, 3, 1, 1>'),
             'bf16': ('first3x3_fwd_kernel<1>', 'thin_wgrad_kernel<3, 3, 1, 1>')},
 'd0.adv': {'fp32': ('first3x3_fwd_kernel<0>', 'thin_fwd2_kernel<3, 3>'),
            'bf16': ('first3x3_fwd_kernel<1>', 'thin_fwd2_kernel<3, 3>')},
 'd2.pair': {'fp32': ('gconv_kernel<128, 64, 32, 32, 1, 0, 0>', 'gconv_s2f_kernel<128, 64, 32, 32, 0, 0>',
                      'wgrad_dma_kernel<1, 0>', 'wgrad_reduce_rows_kernel'),
             'bf16': ('gconv_kernel<128, 64, 32, 32, 1, 0, 1>', 'gconv_s2f_kernel<128, 64, 32, 32, 0, 1>', 'wgrad_kernel<1>',
                      'wgrad_reduce_rows_kernel')},
 'd2.adv': {'fp32': ('gconv_kernel<128, 64, 32, 32, 1, 0, 0>', 'gconv_s2f_kernel<128, 64, 32, 32, 0, 0>'),
            'bf16': ('gconv_kernel<128, 64, 32, 32, 1, 0, 1>', 'gconv_s2f_kernel<128, 64, 32, 32, 0, 1>')},
 'd5.pair': {'fp32': ('wgrad_dma_kernel<1, 1>', 'wgrad_reduce_rows_kernel', 'wino_kernel<64>'),
             'bf16': ('gconv_kernel<128, 64, 32, 32, 1, 0, 1>', 'gconv_kernel<256, 128, 64, 64, 1, 0, 1>', 'wgrad_kernel<1>',
                      'wgrad_reduce_rows_kernel')},
 'd5.adv': {'fp32': ('wino_kernel<64>',),
            'bf16': ('gconv_kernel<128, 64, 32, 32, 1, 0, 1>', 'gconv_kernel<256, 128, 64, 64, 1, 0, 1>')},
 'd8.pair': {'fp32': ('gconv_kernel<128, 128, 64, 32, 1, 0, 0>', 'gconv_multi_kernel<128, 128, 64, 32, 0, 0, 1>',
                      'wgrad_dma_kernel<1, 0>', 'wgrad_reduce_rows_kernel'),
             'bf16': ('gconv_kernel<128, 128, 64, 32, 1, 0, 1>', 'gconv_multi_kernel<128, 128, 64, 32, 0, 1, 1>',
                      'wgrad_kernel<1>', 'wgrad_reduce_rows_kernel')},
 'd8.adv': {'fp32': ('gconv_kernel<128, 64, 32, 32, 1, 0, 0>', 'gconv_multi_kernel<128, 128, 64, 32, 0, 0, 1>'),
            'bf16': ('gconv_kernel<128, 64, 32, 32, 1, 0, 1>', 'gconv_multi_kernel<128, 128, 64, 32, 0, 1, 1>')},
 'd11.pair': {'fp32': ('wgrad_dma_kernel<1, 1>', 'wgrad_reduce_rows_kernel', 'wino_kernel<64>'),
              'bf16': ('gconv_kernel<128, 128, 64, 32, 1, 0, 1>', 'gconv_kernel<256, 128, 64, 64, 1, 0, 1>', 'wgrad_kernel<1>',
                       'wgrad_reduce_rows_kernel')},
 'd11.adv': {'fp32': ('wino_kernel<64>',),
             'bf16': ('gconv_kernel<128, 128, 64, 32, 1, 0, 1>', 'gconv_kernel<128, 64, 32, 32, 1, 0, 1>')},
 'd14.pair': {'fp32': ('gconv_kernel<128, 64, 32, 32, 1, 0, 0>', 'gconv_multi_kernel<128, 128, 64, 32, 0, 0, 1>',
                       'wgrad_dma_kernel<1, 0>', 'wgrad_reduce_rows_kernel'),
              'bf16': ('gconv_kernel<128, 64, 32, 32, 1, 0, 1>', 'gconv_multi_kernel<128, 128, 64, 32, 0, 1, 1>',
                       'wgrad_kernel<1>', 'wgrad_reduce_rows_kernel')},
 'd14.adv': {'fp32': ('gconv_kernel<128, 128, 64, 32, 1, 0, 0>', 'gconv_multi_kernel<128, 64, 32, 32, 0, 0, 1>'),
             'bf16': ('gconv_kernel<64, 64, 32, 32, 2, 0, 1>', 'gconv_multi_kernel<128, 64, 32, 32, 0, 1, 1>')},
 'd17.pair': {'fp32': ('wgrad_dma_kernel<1, 1>', 'wgrad_reduce_rows_kernel', 'wino_kernel<64>'),
              'bf16': ('gconv_kernel<128, 128, 64, 32, 1, 0, 1>', 'gconv_kernel<128, 64, 32, 32, 1, 0, 1>', 'wgrad_kernel<1>',
                       'wgrad_reduce_rows_kernel')},
 'd17.adv': {'fp32': ('wino_kernel<32>', 'wino_kernel<64>'), 'bf16': ('gconv_kernel<128, 64, 32, 32, 1, 0, 1>',)},
 'd20.pair': {'fp32': ('gconv_kernel<128, 128, 64, 32, 1, 0, 0>', 'gconv_multi_kernel<64, 64, 32, 32, 0, 0, 2>',
                       'wgrad_dma_kernel<1, 0>', 'wgrad_reduce_rows_kernel'),
              'bf16': ('gconv_kernel<128, 64, 32, 32, 1, 0, 1>', 'gconv_multi_kernel<128, 64, 32, 32, 0, 1, 1>',
                       'wgrad_kernel<1>', 'wgrad_reduce_rows_kernel')},
 'd20.adv': {'fp32': ('gconv_kernel<128, 128, 64, 32, 1, 0, 0>', 'gconv_multi_kernel<64, 64, 32, 32, 0, 0, 2>'),
             'bf16': ('gconv_kernel<128, 64, 32, 32, 1, 0, 1>', 'gconv_multi_kernel<64, 64, 32, 32, 0, 1, 2>')},
 'd23.pair': {'fp32': ('wgrad_dma_kernel<1, 1>', 'wgrad_reduce_rows_kernel', 'wino_kernel<32>'),
              'bf16': ('gconv_kernel<128, 64, 32, 32, 1, 0, 1>', 'wgrad_kernel<1>', 'wgrad_reduce_rows_kernel')},
 'd23.adv': {'fp32': ('wino_kernel<32>', 'wino_kernel<64>'), 'bf16': ('gconv_kernel<128, 64, 32, 32, 1, 0, 1>',)},
 'd26.pair': {'fp32': ('gconv_kernel<128, 64, 32, 32, 1, 0, 0>', 'gconv_multi_kernel<64, 64, 32, 32, 0, 0, 2>',
                       'wgrad_dma_kernel<1, 0>', 'wgrad_reduce_rows_kernel'),
              'bf16': ('gconv_kernel<128, 64, 32, 32, 1, 0, 1>', 'gconv_multi_kernel<64, 64, 32, 32, 0, 1, 2>',
                       'wgrad_kernel<1>', 'wgrad_reduce_rows_kernel')},
 'd26.adv': {'fp32': ('gconv_kernel<128, 64, 32, 32, 1, 0, 0>', 'gconv_multi_kernel<64, 64, 32, 32, 0, 0, 2>'),
             'bf16': ('gconv_kernel<64, 64, 32, 32, 2, 0, 1>', 'gconv_multi_kernel<64, 64, 32, 32, 0, 1, 2>')},
 'v0.n32': {'fp32': ('first3x3_fwd_kernel<0>',)},
 'v0.n16': {'fp32': ('first3x3_fwd_kernel<0>', 'thin_fwd2_kernel<3, 3>')},
 'v0.stack': {'bf16': ('first3x3_fwd_kernel<1>', 'thin_fwd2_kernel<3, 3>')},
 'v2.n32': {'fp32': ('wino_kernel<64>',)},
 'v2.n16': {'fp32': ('wino_kernel<64>',)},
 'v2.stack': {'bf16': ('gconv_kernel<128, 64, 32, 32, 1, 0, 2>',)},
 'v5.n32': {'fp32': ('wino_kernel<64>',)},
 'v5.n16': {'fp32': ('wino_kernel<64>',)},
 'v5.stack': {'bf16': ('gconv_kernel<128, 64, 32, 32, 1, 0, 2>', 'gconv_kernel<256, 128, 64, 64, 1, 0, 2>')},
 'v7.n32': {'fp32': ('wino_kernel<64>',)},
 'v7.n16': {'fp32': ('wino_kernel<64>',)},
 'v7.stack': {'bf16': ('gconv_kernel<256, 128, 64, 64, 1, 0, 2>',)},
 'v10.n32': {'fp32': ('wino_kernel<64>',)},
 'v10.n16': {'fp32': ('wino_kernel<64>',)},
 'v10.stack': {'bf16': ('gconv_kernel<128, 64, 32, 32, 1, 0, 2>', 'gconv_kernel<256, 128, 64, 64, 1, 0, 2>')},
 'v12.n32': {'fp32': ('wino_kernel<64>',)},
 'v12.n16': {'fp32': ('wino_kernel<64>',)},
 'v12.stack': {'bf16': ('gconv_kernel<128, 128, 64, 32, 1, 0, 2>', 'gconv_kernel<256, 128, 64, 64, 1, 0, 2>')},
 'v19.n32': {'fp32': ('wino_kernel<64>',)},
 'v19.n16': {'fp32': ('wino_kernel<32>', 'wino_kernel<64>')},
 'v19.stack': {'bf16': ('gconv_kernel<128, 128, 64, 32, 1, 0, 2>', 'gconv_kernel<64, 64, 32, 32, 2, 0, 2>')},
 'v21.n32': {'fp32': ('wino_kernel<64>',)},
 'v21.n16': {'fp32': ('wino_kernel<64>',)},
 'v21.stack': {'bf16': ('gconv_kernel<128, 128, 64, 32, 1, 0, 2>', 'gconv_kernel<128, 64, 32, 32, 1, 0, 2>')},
 'v28.n32': {'fp32': ('wino_kernel<32>',)},
 'v28.n16': {'fp32': ('wino_kernel<64>',)},
 'v28.stack': {'bf16': ('gconv_kernel<128, 64, 32, 32, 1, 0, 2>', 'gconv_kernel<64, 64, 32, 32, 2, 0, 2>')}}
for _c in ESRGAN_STEP_CONVS:
    _c['kernels'] = {_p: _EK[_c['id']][_p] for _p in _c['precisions']}

# Conv-family launches of the ESRGAN step that have no row: the fused dense block (bf16) and the pack launches, and the tests that
# hold them at 16 x 32 x 32, and (the dense block) the tests of its every calling form: exact on integers, bounded element by element
CONV_LAUNCHES_TESTED_ELSEWHERE = {
    'rdb_kernel<0>': 'test_ops_gpu.py::test_fused_dense_block_forward[16-32-32], test_rdb_forms_gpu.py::test_forward_is_exact_on_integers_in_every_form, '
                     '::test_forward_chain_of_three_blocks_out_of_one_pack, ::test_forward_within_the_derived_bound_of_fp64',
    'rdb_kernel<1>': 'test_ops_gpu.py::test_fused_dense_block_backward[16-32-32], test_rdb_forms_gpu.py::test_backward_is_exact_on_integers_in_every_form, '
                     '::test_backward_chain_of_three_blocks_out_of_one_pack, ::test_backward_within_the_derived_bound_of_fp64',
    'rdb_pack_kernel': 'test_ops_gpu.py::test_fused_dense_block_forward[16-32-32], test_rdb_forms_gpu.py::test_forward_chain_of_three_blocks_out_of_one_pack, '
                       '::test_backward_chain_of_three_blocks_out_of_one_pack (three blocks out of one launch)',
    'pack_table_kernel': 'test_pack_table_gpu.py::test_one_table_for_every_layer',
}


def esrgan_case_shapes(case):
    """The (N, H, W, Cin, Cout, k, stride, pad, up) problems of one ESRGAN_STEP_CONVS row (H, W: the conv's input size)."""
    if 'shape' in case:
        return {tuple(case['shape']) + (case.get('up', 0),)}
    if 'bf16s' in case:
        hw, cin, cout = case['bf16s']
        return {(n, hw, hw, cin, cout, 3, 1, 1, 0) for n in (32, 16)}
    if 'first3' in case:
        return {(n, case['first3'], case['first3'], 3, 64, 3, 1, 1, 0) for n in (32, 16)}
    n, h, w = case['nhw']
    ks = (case['dense'],) if 'dense' in case else (case['pair'], case['pair'] + 1) if 'pair' in case else (4,)
    return {(n, h, w, 64 + 32 * k, 64 if k == 4 else 32, 3, 1, 1, 0) for k in ks}


def prof_launches(fn, buf_len=160, aux=False):
    """Run ``fn`` with the library's per-launch records on (srx_prof_*); the names of the conv kernels it launched, with the
    template arguments and, where the name carries it, ' MxNxK=..'.  ``aux``: the weight gradients' slab reductions too."""
    import ctypes as C
    import torch
    from torchsr_amd import _lib
    torch.cuda.synchronize()
    _lib.call('srx_prof_start_aux' if aux else 'srx_prof_start', 8192)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        n = _lib.lib().srx_prof_stop()
    buf, ms, fl = C.create_string_buffer(buf_len), C.c_float(), C.c_double()
    names = []
    for i in range(n):
        _lib.call('srx_prof_get', i, buf, buf_len, C.byref(ms), C.byref(fl))
        names.append(buf.value.decode())
    return names



# ---------------------------------------------------------------------------------------------------------------------------
# The float64 reference of one conv product and its elementwise bound (test_step_layers_gpu.py, test_esrgan_layers_gpu.py; the
# bound's own check without a GPU: test_cpu.py).
U32 = 2.0 ** -24   # unit roundoff of a round-to-nearest fp32 accumulation


def gamma(k, u=U32):
    """gamma_k = k u / (1 - k u): the worst relative error of a k-term sum in any order, every addition rounded with unit u."""
    return k * u / (1.0 - k * u)


def bf16_round(t):
    import torch
    return t.to(torch.bfloat16).to(t.dtype)


def conv_refs(what, a, b, x_shape, w_shape, stride, pad, up=0, bias=None, rounded=False, u=U32, wino=False):
    """One product of the layer ``x_shape`` (N, Cin, H, W: the conv's input BEFORE the nearest x2 upsampling ``up = 2`` fuses
    into its gather) * ``w_shape`` (Cout, Cin, k, k): ``what`` = 'y' (a = x, b = W, + the fp32 bias), 'dx' (a = dy, b = W) or 'dW'
    (a = x, b = dy), three ways: (float64 value, torch fp32 value, the elementwise bound gamma_K (|a| conv |b|), K the reduction
    length).  ``rounded``: bf16 products -- BOTH factors are rounded to bf16 first (test_conv2d_bf16_products,
    oracle.srgan.bf16_products(exact_sums=True)); a bf16 x bf16 product is exact in fp32, so the float64 value differs from the
    kernel's by the K-term fp32 accumulation alone and the same bound holds, on the rounded operands.  ``wino`` ('y' and 'dx' of a
    3 x 3 / stride 1 / pad 1 fp32 layer): a fourth value, the elementwise bound of the Winograd form (wino_bound below)."""
    import torch
    import torch.nn.functional as TF
    if wino:
        assert what in ('y', 'dx') and tuple(w_shape[2:]) == (3, 3) and (stride, pad, up) == (1, 1, 0) and not rounded
        w_eff = b if what == 'y' else b.transpose(0, 1).flip(2, 3)
        return conv_refs(what, a, b, x_shape, w_shape, stride, pad, up, bias, rounded, u) + (wino_bound(a, w_eff, bias, u=u),)
    if rounded:
        a, b = bf16_round(a), bf16_round(b)
    cout, cin, k, _ = w_shape
    ups = (lambda t: TF.interpolate(t, scale_factor=2, mode='nearest')) if up == 2 else (lambda t: t)
    n, _, h, w = x_shape
    in_shape = (n, cin, 2 * h, 2 * w) if up == 2 else tuple(x_shape)
    if what == 'y':
        def f(x, wt, bb):
            return TF.conv2d(ups(x), wt, bb, stride, pad)
        kk = cin * k * k + (1 if bias is not None else 0)
        bd = None if bias is None else bias.double()
        return f(a.double(), b.double(), bd), f(a, b, bias), gamma(kk, u) * f(a.double().abs(), b.double().abs(), None if bd is None else bd.abs())
    if what == 'dx':
        def f(dy, wt):  # the adjoint of the gather: the gradient of the upsampled tensor summed over each 2 x 2 block
            d = torch.nn.grad.conv2d_input(in_shape, wt, dy, stride, pad)
            return 4.0 * TF.avg_pool2d(d, 2) if up == 2 else d
        kk = cout * k * k * (4 if up == 2 else 1) + 1
        return f(a.double(), b.double()), f(a, b), gamma(kk, u) * f(a.double().abs(), b.double().abs())
    if what == 'dW':
        def f(x, dy):
            return torch.nn.grad.conv2d_weight(ups(x), tuple(w_shape), dy, stride, pad)
        m = b[:, 0].numel()
        return f(a.double(), b.double()), f(a, b), gamma(m, u) * f(a.double().abs(), b.double().abs())
    raise KeyError(what)


# Winograd F(2x2, 3x3) (wino.hip): Y = A^T [ sum_ci (G g G^T) (.) (B^T d B) ] A.  The bound of one output element is NOT that of
# the direct form: the transforms cancel, so an error is relative to the sum of the ABSOLUTE transformed terms,
#     |y - y64| <= gamma_k ( |A^T| [ sum_ci (|G| |g| |G^T|) (.) (|B^T| |d| |B|) ] |A| + |bias| ),
# k = wino_k(...): the longest chain of roundings between an operand and the output, counted from the code.
WINO_BT = ((1, 0, -1, 0), (0, 1, 1, 0), (0, -1, 1, 0), (0, 1, 0, -1))
WINO_G = ((1, 0, 0), (.5, .5, .5), (.5, -.5, .5), (0, 0, 1))
WINO_AT = ((1, 1, 1, 0), (0, 1, -1, -1))
WINO_MAX_PARTS = 16   # srx_wino_force_plan's and the planner's limit: 16 splits of every tile (8 parts of a tile of the last round)


def wino_k(cin, parts=1, bias=False, extra=0):
    """Roundings between an operand and one output element of wino.hip, each next to where the code makes it."""
    return (4                       # filter transform, srx_wino_pack_one: G g is two additions per entry (the halving is exact), (G g) G^T two more
            + 2                     # input transform, stage_patch: B^T d is one addition per entry, (B^T d) B one more
            + 1                     # the product U V (counted apart from its accumulation: right for a fused MFMA step too)
            + cin                   # the MFMA chain over the input channels, the first step's addition to C = 0 included
            + (parts - 1)           # wino_fixup_kernel / wino_tail_fixup_kernel: the splits or parts, added in order onto the first
            + 4                     # output transform, the epilogue: A^T M is two additions per entry, (A^T M) A two more
            + (1 if bias else 0)    # + bias
            + extra)                # the caller's: LeakyReLU's multiplication, the addend's addition


def wino_bound(a, w_eff, bias=None, parts=WINO_MAX_PARTS, extra=0, u=U32):
    """gamma_k (wino_abs + |bias|) of the forward problem a * w_eff; ``parts``: the splits or parts of the launch's plan -- the
    planner's limit where the caller does not know the plan (a layer class chose it)."""
    mag = wino_abs(a, w_eff)
    if bias is not None:
        mag = mag + bias.double().abs().view(1, -1, 1, 1)
    return gamma(wino_k(w_eff.shape[1], parts, bias is not None, extra), u) * mag


def wino_abs(a, w_eff, tiles_per_pass=8192):
    """|A^T| [ sum_ci (|G| |g| |G^T|) (.) (|B^T| |d| |B|) ] |A| of the forward problem ``a`` (N, Cin, H, W; H, W even) * ``w_eff``
    (Cout, Cin, 3, 3) in float64, shaped like the output (N, Cout, H, W).  A data gradient is the forward problem of dy and
    ``w.transpose(0, 1).flip(2, 3)``.  Images are taken a few at a time: the transformed patches of a step-sized layer are GBs."""
    import torch
    import torch.nn.functional as TF
    bt, g, at = (torch.tensor(m, dtype=torch.float64).abs() for m in (WINO_BT, WINO_G, WINO_AT))
    n, cin, h, w = a.shape
    cout = w_eff.shape[0]
    th, tw = h // 2, w // 2
    uabs = torch.einsum('ip,ocpq,jq->ijco', g, w_eff.double().abs(), g).reshape(16, cin, cout)
    out = torch.empty((n, cout, h, w), dtype=torch.float64)
    step = max(1, tiles_per_pass // (th * tw))
    for n0 in range(0, n, step):
        ap = TF.pad(a[n0:n0 + step].double().abs(), (1, 1, 1, 1))
        m = ap.shape[0]
        patches = ap.unfold(2, 4, 2).unfold(3, 4, 2)                                  # (m, Cin, TH, TW, 4, 4)
        vabs = torch.einsum('ip,ncyxpq,jq->ijnyxc', bt, patches, bt).reshape(16, m * th * tw, cin)
        mabs = torch.bmm(vabs, uabs).reshape(4, 4, m, th, tw, cout)
        out[n0:n0 + step] = torch.einsum('ui,vj,ijnyxo->noyuxv', at, at, mabs).reshape(m, cout, h, w)
    return out

# ---------------------------------------------------------------------------------------------------------------------------
# The non-convolution launches of the steps: BatchNorm, losses, pools, activations' backward, layout, Adam (norm.hip, loss.hip,
# eltwise.hip, optim.hip).  OP_ARGS names the INTEGER arguments of each entry point in the order of the C signature
# (include/srx.h); op_key folds them into (entry point, rows M or elements n, C, groups, act): what a STEP_OPS row is matched by.
OP_ARGS = {
    'srx_nchw_to_nhwc': ('N', 'Cin', 'H', 'W', 'C'), 'srx_nhwc_to_nchw': ('N', 'Cin', 'H', 'W', 'C'),
    'srx_colsum': ('M', 'C', 'Cs', 'accumulate'), 'srx_act_bwd_from_out': ('n', 'act'),
    'srx_act_bwd_from_out_strided': ('ldy', 'ly', 'ldx', 'M', 'C', 'act'), 'srx_prelu_fwd': ('n',),
    'srx_prelu_bwd': ('accumulate', 'n'), 'srx_lrelu_fwd': ('n',), 'srx_axpby': ('n',),
    'srx_axpby_channels': ('x_cs', 'x_off', 'z_cs', 'z_off', 'y_cs', 'y_off', 'C', 'M'),
    'srx_copy_channels': ('src_cs', 'src_off', 'dst_cs', 'dst_off', 'C', 'M', 'accumulate'),
    'srx_upsample_nearest2x_fwd': ('N', 'H', 'W', 'C'), 'srx_upsample_nearest2x_bwd': ('N', 'H', 'W', 'C'),
    'srx_mean_fwd': ('n',), 'srx_mean_bwd': ('n',), 'srx_sigmoid_fwd': ('n',), 'srx_sigmoid_bwd': ('n',),
    'srx_bn_partial_stats': ('M', 'C'), 'srx_bn_finalize': ('rows', 'M', 'C'), 'srx_bn_eval_stats': ('C',),
    'srx_bn_act_fwd': ('M', 'C', 'act'), 'srx_bn_act_bwd_reduce': ('M', 'C', 'act'),
    'srx_bn_act_bwd_apply': ('M', 'C', 'act', 'training'), 'srx_bn_train_fwd': ('rows', 'M', 'C', 'groups', 'act'),
    'srx_bn_act_bwd': ('M', 'C', 'groups', 'act', 'training'), 'srx_bn_act_bwd_finish': ('rows', 'prelu_cols', 'M', 'C', 'act'),
    'srx_maxpool2x2_fwd': ('N', 'H', 'W', 'C'), 'srx_maxpool2x2_bwd': ('N', 'H', 'W', 'C'),
    'srx_maxpool2x2_relu_bwd': ('N', 'H', 'W', 'C'), 'srx_maxpool2x2_fwd_to_bf16': ('N', 'H', 'W', 'C'),
    'srx_maxpool2x2_relu_bwd_bf16': ('N', 'H', 'W', 'C'), 'srx_act_bwd_from_out_to_bf16': ('n', 'act'),
    'srx_mse_fwd': ('n',), 'srx_l1_fwd': ('n',), 'srx_mse_bwd': ('n',), 'srx_l1_bwd': ('n',), 'srx_l1_fwd_count': ('n', 'count'),
    'srx_l1_bwd_count': ('n', 'count'), 'srx_bce_fwd': ('n',), 'srx_bce_bwd': ('n',), 'srx_bce_logits_fwd': ('n',),
    'srx_bce_logits_bwd': ('n',), 'srx_adam_step': ('n',),
}
# srx_* launches that are neither convolutions nor in the four files above, and the op-level tests that hold them
OPS_TESTED_ELSEWHERE = {
    'srx_linear_fwd': 'test_linear_forms_gpu.py (every launch form, fp64), test_ops_gpu.py::test_linear',
    'srx_linear_bwd_data': 'test_linear_forms_gpu.py, test_ops_gpu.py::test_linear',
    'srx_linear_bwd_weight': 'test_linear_forms_gpu.py, test_ops_gpu.py::test_linear',
    'srx_gan_head_fwd': 'test_head_gpu.py', 'srx_gan_head_bwd': 'test_head_gpu.py',
    'srx_ring_push': 'test_step_gpu.py (one thread, no shape)', 'srx_crop_flip_u8': 'test_ops_gpu.py', 'srx_bicubic_down': 'test_ops_gpu.py',
}
_CONV_PREFIXES = ('srx_conv', 'srx_wino', 'srx_pack_table', 'srx_rdb', 'srx_prof', 'srx_f32_to', 'srx_bf16_to', 'srx_f16_to',
                  'srx_wgrad', 'srx_set_', 'srx_plan_', 'srx_occupy', 'srx_device', 'srx_version', 'srx_last', 'srx_build')


def op_key(name, ints):
    """(entry point, M or n, C, groups, act) of one recorded call; pools, layout and upsampling kernels: M = N * H * W pixels of
    the tensor whose size the arguments give."""
    a = dict(zip(OP_ARGS[name], ints))
    size = a['M'] if 'M' in a else a['n'] if 'n' in a else a['N'] * a['H'] * a['W'] if 'N' in a else 0
    return (name, int(size), int(a.get('C', 0)), int(a.get('groups', 1)), int(a.get('act', 0)))


def record_op_calls(monkeypatch, fn):
    """Run ``fn`` with ``torchsr_amd._lib.call`` -- and every module-level alias of it in the package (functional.py, optim.py
    import the name) -- wrapped: the (entry point, integer arguments) of every srx_* call that is not a convolution, in call
    order.  The integer arguments are those the ctypes signature declares as int / int64 (sizes and flags, never pointers)."""
    import ctypes as C
    import sys
    import torch
    from torchsr_amd import _lib
    import torchsr_amd.esrgan.trainer  # noqa: F401  (every module that binds `call` must be loaded BEFORE the patch: one imported
    import torchsr_amd.srgan.trainer  # noqa: F401   while it is in place would keep the spy as its alias for good)
    import torchsr_amd.functional  # noqa: F401
    import torchsr_amd.optim  # noqa: F401
    real = _lib.call
    calls = []

    def spy(name, *args):
        if not name.startswith(_CONV_PREFIXES):
            types = _lib._SIGS[name][1]
            calls.append((name, tuple(int(v) for v, t in zip(args, types) if t in (C.c_int, C.c_int64))))
        return real(name, *args)

    for mod_name, mod in list(sys.modules.items()):
        if mod is None or not (mod_name == 'torchsr_amd' or mod_name.startswith('torchsr_amd.')):
            continue
        for attr, val in list(vars(mod).items()):
            if val is real:
                monkeypatch.setattr(mod, attr, spy)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        monkeypatch.undo()
    return calls


# STEP_OPS: the non-convolution problems of the batch-16 SRGAN step and the batch-16 ESRGAN step (rows the recorder above finds
# there: test_step_ops_are_covered) plus the edges of the kernels' launch geometry.  op: the family (one runner in
# test_step_ops_gpu.py); the other fields are that family's sizes.  covers: op_key()s of the calls the case makes.
ACT_NONE_, ACT_PRELU_ = 0, 3
SLOPE = 0.25  # a power of two: integer data times the slope stays exact (counted in quarters)


def _bn(m, c, groups=1, act=ACT_LRELU, training=True, residual=False, finish_rows=0):
    tag = {0: 'none', 2: 'lrelu', 3: 'prelu'}[act]
    id_ = f'bn.{m}x{c}.g{groups}.{tag}' + ('' if training else '.eval') + ('.res' if residual else '')
    if training:
        covers = [('srx_bn_partial_stats', m, c, 1, 0), ('srx_bn_train_fwd', m, c, groups, act), ('srx_bn_act_bwd', m, c, groups, act)]
        if groups == 1:  # (the residual tower finalises its conv epilogue's table with the one-group call)
            covers.append(('srx_bn_finalize', m, c, 1, 0))
    else:
        covers = [('srx_bn_eval_stats', 0, c, 1, 0), ('srx_bn_act_fwd', m, c, 1, act), ('srx_bn_act_bwd', m, c, 1, act)]
    if groups == 1:  # the two-call form of the backward and, in training, its finish form WITH the apply pass
        covers += [('srx_bn_act_bwd_reduce', m, c, 1, act), ('srx_bn_act_bwd_apply', m, c, 1, act)]
        if training:
            covers.append(('srx_bn_act_bwd_finish', m, c, 1, act))
    return dict(id=id_, op='bn', M=m, C=c, groups=groups, act=act, training=training, residual=residual, covers=covers)


STEP_OPS = [
    # generator: the residual tower's BatchNorm + PReLU, its BatchNorm + skip, conv2's BatchNorm + skip (16 x 24 x 24 rows)
    _bn(9216, 64, act=ACT_PRELU_), _bn(9216, 64, act=ACT_NONE_, residual=True), _bn(9216, 64, act=ACT_NONE_),
    _bn(9216, 64, act=ACT_PRELU_, training=False), _bn(9216, 64, act=ACT_NONE_, training=False, residual=True),
    # SRGAN discriminator on real + fake as one batch of 32 (two groups): 128-row blocks and, above 4 Mi elements, the
    # grid-stride regime of the streaming kernels
    _bn(73728, 64, 2), _bn(73728, 128, 2), _bn(18432, 128, 2), _bn(18432, 256, 2), _bn(4608, 256, 2), _bn(4608, 512, 2),
    _bn(1152, 512, 2),
    # ... and on the 16 generated images alone (the generator's adversarial term)
    _bn(36864, 64), _bn(36864, 128), _bn(9216, 128), _bn(9216, 256), _bn(2304, 256), _bn(2304, 512), _bn(576, 512),
    # ESRGAN discriminator, 32 images of 128 x 128: the first M on the 512-row plan
    _bn(131072, 64, 2),
    _bn(131072, 128, 2),
    # ... its other layers, pair pass (two groups) and adversarial pass
    _bn(65536, 64), _bn(65536, 128), _bn(32768, 128, 2), _bn(32768, 256, 2), _bn(16384, 128), _bn(16384, 256), _bn(8192, 256, 2),
    _bn(8192, 512, 2), _bn(4096, 256), _bn(4096, 512), _bn(2048, 512, 2), _bn(1024, 512), _bn(512, 512, 2), _bn(256, 512),
    # the row-block thresholds from both sides (one group: the last block is partial)
    _bn(32767, 16), _bn(32768, 16), _bn(131071, 16), _bn(131072, 16),
    # C = 256: 4 row lanes, 16 rows per trip; the last block holds 16 + 1 rows
    _bn(36 * 32 + 17, 256, act=ACT_NONE_),
    # cq = 10 does not divide 256 (6 idle threads), the narrowest and the widest channel count
    _bn(4608, 40, act=ACT_PRELU_), _bn(4608, 8), _bn(1152, 1024, act=ACT_NONE_, residual=True),
]
STEP_OPS += [
    # srx_bn_act_bwd_finish on a hand-built table: the PReLU partial in one and in two columns; 257 rows: one past a lane trip
    dict(id='bn_finish.257x64.cols1', op='bn_finish', rows=257, C=64, M=9216, prelu_cols=1, act=3, covers=[('srx_bn_act_bwd_finish', 9216, 64, 1, 3)]),
    dict(id='bn_finish.256x64.cols2', op='bn_finish', rows=256, C=64, M=9216, prelu_cols=2, act=3, covers=[('srx_bn_act_bwd_finish', 9216, 64, 1, 3)]),
    dict(id='bn_finish.256x64.cols2.none', op='bn_finish', rows=256, C=64, M=9216, prelu_cols=2, act=0, covers=[('srx_bn_act_bwd_finish', 9216, 64, 1, 0)]),
]


def _colsum(m, c, cs, acc):
    return dict(id=f'colsum.{m}x{c}.cs{cs}.acc{acc}', op='colsum', M=m, C=c, Cs=cs, accumulate=acc, covers=[('srx_colsum', m, c, 1, 0)])


STEP_OPS += [_colsum(147456, 64, 64, 1), _colsum(9216, 3, 4, 0), _colsum(4099, 100, 104, 1), _colsum(32, 1, 1, 0), _colsum(32, 1, 1, 1),
             _colsum(32, 1024, 1024, 1)]


def _n(op, n, entries, **kw):
    return dict(id=f'{op}.{n}' + ''.join(f'.{k}{v}' for k, v in kw.items()), op=op, n=n, covers=[(e, n, 0, 1, kw.get('act', 0)) for e in entries], **kw)


LOSS_SIZES = (16 * 96 * 96 * 4, 16 * 6 * 6 * 512, 16 * 8 * 8 * 512, 1024 * 1024 - 1, 1024 * 1024, 1024 * 1024 + 1, 1, 16, 32)
for _nn in LOSS_SIZES:
    STEP_OPS.append(_n('mse', _nn, ('srx_mse_fwd', 'srx_mse_bwd')))
    STEP_OPS.append(_n('l1', _nn, ('srx_l1_fwd', 'srx_l1_bwd')))
    STEP_OPS.append(_n('mean', _nn, ('srx_mean_fwd', 'srx_mean_bwd')))
    STEP_OPS.append(_n('bce', _nn, ('srx_bce_fwd', 'srx_bce_bwd')))
    STEP_OPS.append(_n('bce_logits', _nn, ('srx_bce_logits_fwd', 'srx_bce_logits_bwd')))
STEP_OPS.append(dict(id='l1_count.589824', op='l1', n=16 * 96 * 96 * 4, count=16 * 96 * 96 * 3,
                     covers=[('srx_l1_fwd_count', 16 * 96 * 96 * 4, 0, 1, 0), ('srx_l1_bwd_count', 16 * 96 * 96 * 4, 0, 1, 0)]))
STEP_OPS.append(dict(id='l1_count.1048576', op='l1', n=16 * 128 * 128 * 4, count=16 * 128 * 128 * 3,
                     covers=[('srx_l1_fwd_count', 1024 * 1024, 0, 1, 0), ('srx_l1_bwd_count', 1024 * 1024, 0, 1, 0)]))
STEP_OPS.append(dict(id='l1_count.1048577', op='l1', n=1024 * 1024 + 1, count=786433,
                     covers=[('srx_l1_fwd_count', 1024 * 1024 + 1, 0, 1, 0), ('srx_l1_bwd_count', 1024 * 1024 + 1, 0, 1, 0)]))
# activations' backward at the generator's sizes (16 x 96 x 96 x 64 is past the 4096-block cap), n & 3 tails included
for _nn in (16 * 24 * 24 * 64, 16 * 48 * 48 * 64, 16 * 96 * 96 * 64, 4096 * 1024 + 1027):
    STEP_OPS.append(_n('prelu_bwd', _nn, ('srx_prelu_fwd', 'srx_prelu_bwd')))
    STEP_OPS.append(_n('act_bwd', _nn, ('srx_act_bwd_from_out',), act=2))
for _nn, _a in ((16 * 96 * 96 * 64, 1), (16 * 6 * 6 * 512, 1), (16 * 8 * 8 * 512, 1), (16 * 64 * 64 * 64, 2), (16 * 128 * 128 * 64, 2)):
    STEP_OPS.append(_n('act_bwd', _nn, ('srx_act_bwd_from_out',), act=_a))
STEP_OPS.append(dict(id='act_bwd_strided.32768x32', op='act_bwd_strided', M=16 * 32 * 32 * 2, C=32, ld=192, act=2,
                     covers=[('srx_act_bwd_from_out_strided', 16 * 32 * 32 * 2, 32, 1, 2)]))
STEP_OPS.append(dict(id='act_bwd_strided.147456x64', op='act_bwd_strided', M=147456, C=64, ld=68, act=1,
                     covers=[('srx_act_bwd_from_out_strided', 147456, 64, 1, 1)]))
for _nn in (1, 16 * 24 * 24 * 64, 16 * 32 * 32 * 64, 16 * 96 * 96 * 64, 4096 * 1024 + 1026):
    STEP_OPS.append(_n('axpby', _nn, ('srx_axpby',)))
# VGG19's pools in the perceptual loss: source + target forward (N = 32), the source's backward (N = 16)
for _hw, _c in ((96, 64), (48, 128), (24, 256), (12, 512), (128, 64), (64, 128), (32, 256), (16, 512)):
    STEP_OPS.append(dict(id=f'pool.32x{_hw}x{_c}', op='pool', N=32, H=_hw, W=_hw, C=_c, covers=[('srx_maxpool2x2_fwd', 32 * _hw * _hw, _c, 1, 0)]))
    STEP_OPS.append(dict(id=f'pool.16x{_hw}x{_c}', op='pool', N=16, H=_hw, W=_hw, C=_c, bwd=True,
                         covers=[('srx_maxpool2x2_fwd', 16 * _hw * _hw, _c, 1, 0), ('srx_maxpool2x2_bwd', 16 * _hw * _hw, _c, 1, 0),
                                 ('srx_maxpool2x2_relu_bwd', 16 * _hw * _hw, _c, 1, 0)]))
# layout at the module boundary: images in (3 -> 4 channels), images out, the discriminator's flatten
for _nn, _c, _hw, _cs in ((16, 3, 24, 4), (16, 3, 96, 4), (32, 3, 96, 4), (32, 512, 6, 512), (16, 512, 6, 512), (16, 3, 32, 4), (16, 3, 128, 4),
                           (32, 512, 4, 512), (16, 512, 4, 512)):
    STEP_OPS.append(dict(id=f'layout.{_nn}x{_c}x{_hw}', op='layout', N=_nn, Cin=_c, H=_hw, W=_hw, Cs=_cs,
                         covers=[('srx_nchw_to_nhwc', _nn * _hw * _hw, _cs, 1, 0), ('srx_nhwc_to_nchw', _nn * _hw * _hw, _cs, 1, 0)]))
# ESRGAN's trunk between dense-block buffers: 64-channel slices of 192-channel rows
STEP_OPS.append(dict(id='channels.16384x64', op='channels', M=16 * 32 * 32, C=64, wide=192,
                     covers=[('srx_axpby_channels', 16384, 64, 1, 0), ('srx_copy_channels', 16384, 64, 1, 0)]))
STEP_OPS.append(dict(id='channels.147457x32', op='channels', M=147457, C=32, wide=192,
                     covers=[('srx_axpby_channels', 147457, 32, 1, 0), ('srx_copy_channels', 147457, 32, 1, 0)]))
# Adam on the flat buffers of the four models (lengths read from the built models) and on lengths with an n & 3 tail past the
# 4096-block cap (4096 x 1024 floats)
STEP_OPS += [dict(id=f'adam.{_k}.{_m}', op='adam', model=f'{_k}.{_m}', covers=[]) for _k in ('srgan', 'esrgan') for _m in 'GD']
STEP_OPS += [dict(id=f'adam.tail{_r}', op='adam', n=4096 * 1024 + 1024 + _r, covers=[('srx_adam_step', 4096 * 1024 + 1024 + _r, 0, 1, 0)])
             for _r in (1, 2, 3)]


def _rng(case):
    import zlib
    import numpy as np
    return np.random.default_rng(zlib.crc32(case['id'].encode()))


def _sparse(rng, shape, hi, keep, pin=1):
    """integers in [-hi, hi], a fraction ``keep`` of them kept, the rest zero -- except the last four elements and every 1024th,
    which are ``pin``: every block of every launch geometry and every n & 3 tail holds non-zeros"""
    import numpy as np
    v = rng.integers(-hi, hi + 1, shape, dtype=np.int8)
    if keep >= 1.0:
        return v
    v = np.where(rng.random(shape, dtype=np.float32) < keep, v, 0).astype(np.int8)
    flat = v.reshape(-1)
    flat[-4:] = pin
    flat[::1024] = pin
    return v


def int_inputs(case):
    """The integer-valued inputs of a case's exact check (int8 arrays; the tests cast them to fp32), or None when the family has
    no exact check.  Every product of two of them, times SLOPE, is a whole number of quarters."""
    rng, op = _rng(case), case['op']
    if op == 'bn':
        shape = (case['M'], case['C'])
        d = dict(y=_sparse(rng, shape, 3, 1.0), dout=_sparse(rng, shape, 2, 1.0))
        if case['act'] == ACT_PRELU_:  # the slope gradient is ONE sum over the whole tensor: sparser gradients
            d['dout'] = _sparse(rng, shape, 2, 0.25)
        return d
    if op == 'bn_finish':
        return dict(table=_sparse(rng, (case['rows'], 2 * case['C'] + 4), 100, 1.0).astype('int32'))
    if op == 'colsum':
        x = _sparse(rng, (case['M'], case['Cs']), 3, 1.0)
        x[-1][x[-1] == 0] = 1  # the last row counts in every column
        return dict(x=x)
    if op in ('mse', 'l1', 'mean'):
        n = case['n']
        return dict(a=_sparse(rng, n, 2, 0.5), b=_sparse(rng, n, 1, 0.5, pin=-1))
    if op == 'prelu_bwd':
        n = case['n']
        return dict(x=_sparse(rng, n, 2, 0.75, pin=-1), dy=_sparse(rng, n, 1, 0.5))
    return None


def int_abs_sums(case, d):
    """{output: largest sum of ABSOLUTE values of the terms of any one output element}, in the smallest unit present (quarters
    where SLOPE multiplies), computed in int64: below 2^24 every partial sum in every order is an fp32 number."""
    import numpy as np
    op = case['op']
    i64 = lambda a: a.astype(np.int64)  # noqa: E731
    if op == 'bn':
        y, dout = i64(d['y']), i64(d['dout'])
        per = case['M'] // case['groups']
        out = {'sum y': np.abs(y).sum(0).max(), 'sum y^2': (y * y).sum(0).max()}
        if case['act'] == ACT_NONE_:
            dz4 = 4 * dout
        else:
            dz4 = np.where(y > 0, 4 * dout, dout)  # quarters
        out['sum dz'] = np.abs(dz4).sum(0).max()          # (the parameter gradients total over the groups)
        out['sum dz xhat'] = np.abs(dz4 * y).sum(0).max()
        if case['act'] == ACT_PRELU_:
            out['d prelu'] = np.abs(np.where(y > 0, 0, dout * y)).sum()
        assert per * case['groups'] == case['M']
        # + the non-zero .grad the sums are accumulated into (|grad| <= 8 units, see the runner)
        return {k: int(v) + 4 * 8 for k, v in out.items()}
    if op == 'bn_finish':
        t = np.abs(i64(d['table']))
        c = case['C']
        cols = t[:, :2 * c].sum(0).max()
        pre = t[:, 2 * c:2 * c + case['prelu_cols']].sum()
        return {'columns': int(cols) + 8, 'prelu': int(pre) + 8}
    if op == 'colsum':
        return {'colsum': int(np.abs(i64(d['x'])).sum(0).max()) + 8}
    if op in ('mse', 'l1', 'mean'):
        a, b = i64(d['a']), i64(d['b'])
        return {'mse': int(((a - b) ** 2).sum()), 'l1': int(np.abs(a - b).sum()), 'mean': int(np.abs(a).sum())}
    if op == 'prelu_bwd':
        x, dy = i64(d['x']), i64(d['dy'])
        return {'dslope': int(np.abs(np.where(x > 0, 0, dy * x)).sum()) + 8}
    raise KeyError(op)
