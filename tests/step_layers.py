"""The conv problems of the batch-16 SRGAN GAN step (BASELINE configs[1], the bench.py headline), shared by the tests that
exercise them at the step's own sizes (test_ops_gpu.py, test_step_layers_gpu.py)."""
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


def prof_launches(fn, buf_len=160):
    """Run ``fn`` with the library's per-launch records on (srx_prof_*); the names of the conv kernels it launched, with the
    template arguments and, where the name carries it, ' MxNxK=..'."""
    import ctypes as C
    import torch
    from torchsr_amd import _lib
    torch.cuda.synchronize()
    _lib.call('srx_prof_start', 8192)
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
