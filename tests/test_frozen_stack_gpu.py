"""The one frozen-stack walk behind both perceptual-loss nodes (functional ``_stack_forward`` / ``_stack_backward``): every
calling form launches one kernel per layer and direction, of its own kind; and the general plain stack -- LeakyReLU convs, a
pool whose input is no ReLU output -- against torch autograd in fp64."""
from collections import Counter

import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-9)).item()


def _recorded(fn):
    """The names of the C-ABI calls ``fn`` makes through ``functional.call``, in order."""
    from torchsr_amd import functional as F
    real_call, names = F.call, []
    F.call = lambda name, *a: (names.append(name), real_call(name, *a))[1]
    try:
        fn()
    finally:
        F.call = real_call
    return names


# ------------------------------------------------------------------ 1. one launch per layer and direction
CONV_FWD = {'fp32': {'srx_wino_fwd', 'srx_conv2d_fwd'}, 'bf16': {'srx_conv2d_fwd_first3_to_bf16', 'srx_conv3x3_bf16s_fwd'}}
CONV_BWD = {'fp32': {'srx_wino_bwd_data', 'srx_conv2d_bwd_data', 'srx_conv2d_bwd_data_act'},
            'bf16': {'srx_conv3x3_bf16s_bwd_data', 'srx_conv2d_bwd_data'}}
# (pool forward, pool backward, the top of the backward) of a form
PLAIN = {'fp32': ('srx_maxpool2x2_fwd', 'srx_maxpool2x2_relu_bwd', 'srx_act_bwd_from_out'),
         'bf16': ('srx_maxpool2x2_fwd_to_bf16', 'srx_maxpool2x2_relu_bwd_bf16', 'srx_act_bwd_from_out_to_bf16')}
TAP = ('srx_maxpool2x2_relu_fwd_tap', 'srx_maxpool2x2_relu_bwd_tap', 'srx_tap_l1_bwd_top')


@pytest.mark.parametrize('pair', [True, False], ids=['pair', 'target_features'])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('which', ['VGGLoss', 'PerceptualLoss'])
def test_one_launch_per_layer_and_direction(dev, which, precision, pair):
    """Forward + backward of a loss at (2, 3, 16, 16) -- the smallest size at which four pools and the bf16-storage path both
    hold -- after a warm-up call (which packs): the counts of the launches by name, expected from the layer list alone."""
    from torchsr_amd import functional as F
    from torchsr_amd.layers import set_conv_precision
    from torchsr_amd.realesrgan.loss import PerceptualLoss
    from torchsr_amd.srgan.loss import VGGLoss
    tap = which == 'PerceptualLoss'
    module = (PerceptualLoss if tap else VGGLoss)(weights='random').to(dev)
    set_conv_precision(module, precision)
    g = torch.Generator().manual_seed(11)
    src4 = F.to_nhwc(torch.rand(2, 3, 16, 16, generator=g).to(dev), 4)
    tgt = torch.rand(2, 3, 16, 16, generator=g).to(dev)
    tgt4 = F.to_nhwc(tgt, 4)
    tfeats = None if pair else module.target_features(tgt)
    layers = module._stack()[0] if tap else module._stack()
    n_conv, n_pool = sum(k == 'conv' for k, _ in layers), sum(k == 'pool' for k, _ in layers)
    assert (n_conv, n_pool) == (16, 4)
    taps = module._stack()[1] if tap else ()
    assert F._bf16_stack_ok(layers, (4 if pair else 2, 16, 16, 4), taps) == (precision == 'bf16')

    def run():
        s = src4.clone().requires_grad_(True)
        (module.forward_nhwc(s, tgt4) if pair else module.forward_nhwc(s, None, target_features=tfeats)).backward()
        assert bool(torch.isfinite(s.grad).all()) and float(s.grad.abs().max()) > 0
    run()
    names = _recorded(run)
    count = Counter(n for n in names if 'pack' not in n)   # (the pack entry points: none after the warm-up, and not counted)
    pool_fwd, pool_bwd, top = TAP if tap else PLAIN[precision]
    want = Counter({pool_fwd: n_pool, pool_bwd: n_pool, top: 1})
    if tap:
        want.update({'srx_normalize_pair_nhwc4': 1, 'srx_normalize_nhwc4_bwd': 1})
        want.update({'srx_tap_l1_finalize': n_pool, 'srx_tap_l1_fwd': 1} if pair else {'srx_tap_l1_fwd': n_pool + 1})
    else:
        want.update({'srx_l1_fwd': 1, 'srx_l1_bwd': 1})   # F.l1_loss behind the node
        assert not any('tap' in n or 'normalize' in n for n in names)
    if precision == 'bf16':
        want.update({'srx_conv2d_fwd_first3_to_bf16': 1, 'srx_conv3x3_bf16s_fwd': n_conv - 1,
                     'srx_conv3x3_bf16s_bwd_data': n_conv - 1, 'srx_conv2d_bwd_data': 1})
        assert count == want, (count, want)
        return
    for allowed in (CONV_FWD[precision], CONV_BWD[precision]):   # one per conv, drawn from the path's set
        assert sum(count.pop(n, 0) for n in allowed) == n_conv, (allowed, names)
    assert count == want, (count, want)


# ------------------------------------------------------------------ 2. the general plain stack
LRELU_SEED = 2
SLOPE = 0.2
TIE = 1e-4


def _lrelu_case(seed):
    """Seeded weights (kaiming-normal for LeakyReLU(0.2), small biases), a source and a target batch of (2, 3, 8, 12) and the
    coefficients of the scalar ``(fs * coef).sum()``."""
    g = torch.Generator().manual_seed(seed)
    w = [torch.randn(16, 3, 3, 3, generator=g) * (2.0 / (1 + SLOPE ** 2) / 27) ** 0.5,
         torch.randn(32, 16, 3, 3, generator=g) * (2.0 / (1 + SLOPE ** 2) / 144) ** 0.5]
    b = [torch.randn(16, generator=g) * 0.1, torch.randn(32, generator=g) * 0.1]
    src, tgt = torch.rand(2, 3, 8, 12, generator=g), torch.rand(2, 3, 8, 12, generator=g)
    coef = torch.randn(2, 32, 4, 6, generator=g)
    return w, b, src, tgt, coef


def _lrelu_reference(w, b, x, coef, dt):
    """``(features, input gradient of (features * coef).sum(), margin)`` by torch autograd on the CPU in ``dt``; ``margin``: the
    smallest distance of a decision from a tie -- a pre-activation from 0, a pool window's maximum from its runner-up."""
    x = x.to(dt).clone().requires_grad_(True)
    pre1 = TF.conv2d(x, w[0].to(dt), b[0].to(dt), padding=1)
    a1 = TF.leaky_relu(pre1, SLOPE)
    p = TF.max_pool2d(a1, 2)
    pre2 = TF.conv2d(p, w[1].to(dt), b[1].to(dt), padding=1)
    f = TF.leaky_relu(pre2, SLOPE)
    (f * coef.to(dt)).sum().backward()
    n, c, h, wd = a1.shape
    top = a1.detach().view(n, c, h // 2, 2, wd // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 4).sort(dim=1, descending=True).values
    margin = min(pre1.abs().min().item(), pre2.abs().min().item(), (top[:, 0] - top[:, 1]).min().item())
    return f.detach(), x.grad.clone(), margin


def _nhwc(t, c_store):
    out = torch.zeros(t.shape[0], t.shape[2], t.shape[3], c_store, dtype=t.dtype)
    out[..., :t.shape[1]] = t.permute(0, 2, 3, 1)
    return out


@pytest.mark.parametrize('with_target', [False, True], ids=['source-alone', 'source+target'])
def test_general_plain_stack_against_fp64(dev, with_target):
    """``[conv 3 -> 16 + LeakyReLU(0.2), pool, conv 16 -> 32 + LeakyReLU(0.2)]`` through ``frozen_conv_stack`` on a (2, 8, 12, 4)
    NHWC input: the branches only the plain fp32 node has -- the layer's own activation on top, a pool whose input is no ReLU
    output (``srx_maxpool2x2_bwd`` + ``srx_act_bwd_from_out``), layer 0 through ``_layer_dgrad`` -- against torch autograd in fp64.

    Bound (``test_loss_against_the_reference``' rule): no further from fp64, in ``rel``, than 3x the fp32 CPU torch evaluation's
    own distance, floor 1e-5.  ``LRELU_SEED`` was chosen on the CPU so that no pre-activation and no pool-window margin of the fp64
    run, source or target, lies within 1e-4 of a tie (asserted below; the smallest margins are 2.8e-4 and 2.5e-4; seeds 0..11 were
    looked at), so no decision can flip.  The fp32 CPU evaluation's distance from fp64 for that seed: features 2.9e-7 (source) / 3.7e-7 (target), gradient 2.3e-7."""
    from torchsr_amd import functional as F
    from torchsr_amd._lib import ACT_LRELU
    from torchsr_amd.layers import Conv2d
    w, b, src, tgt, coef = _lrelu_case(LRELU_SEED)
    convs = [Conv2d(3, 16, 3, 1, 1, act=ACT_LRELU, slope=SLOPE), Conv2d(16, 32, 3, 1, 1, act=ACT_LRELU, slope=SLOPE)]
    for m, wt, bs in zip(convs, w, b):
        with torch.no_grad():
            m.weight.copy_(wt)
            m.bias.copy_(bs)
        m.to(dev).requires_grad_(False)
    layers = [('conv', convs[0]), ('pool', None), ('conv', convs[1])]
    refs = {}
    for name, x in (('source', src), ('target', tgt)):
        f64, g64, margin = _lrelu_reference(w, b, x, coef, torch.float64)
        f32, g32, _ = _lrelu_reference(w, b, x, coef, torch.float32)
        print(f'{name}: smallest margin {margin:.3e}; fp32 CPU vs fp64: features {rel(f32, f64):.2e}, gradient {rel(g32, g64):.2e}')
        assert margin > TIE, (name, margin)
        refs[name] = (f64, g64, max(1e-5, 3 * rel(f32, f64)), max(1e-5, 3 * rel(g32, g64)))
    s4 = _nhwc(src, 4).to(dev).requires_grad_(True)
    t4 = _nhwc(tgt, 4).to(dev) if with_target else None
    got = {}

    def run():
        fs, ft = F.frozen_conv_stack(s4, t4, layers)
        assert (ft is None) == (t4 is None) and (ft is None or not ft.requires_grad)
        (fs * _nhwc(coef, 32).to(dev)).sum().backward()
        got['fs'], got['ft'] = fs.detach(), ft
    names = _recorded(run)
    assert names.count('srx_maxpool2x2_bwd') == 1 and names.count('srx_act_bwd_from_out') == 2   # one on top, one behind the pool
    assert names.index('srx_act_bwd_from_out') < names.index('srx_maxpool2x2_bwd') < len(names) - 1 - names[::-1].index('srx_act_bwd_from_out')
    assert 'srx_maxpool2x2_relu_bwd' not in names and names.count('srx_maxpool2x2_fwd') == 1
    f64, g64, allow_f, allow_g = refs['source']
    grad = s4.grad[..., :3].permute(0, 3, 1, 2)
    print(f'features: distance {rel(got["fs"].permute(0, 3, 1, 2), f64):.2e}, allowed {allow_f:.2e}; '
          f'gradient: distance {rel(grad, g64):.2e}, allowed {allow_g:.2e}')
    assert rel(got['fs'].permute(0, 3, 1, 2), f64) <= allow_f
    assert rel(grad, g64) <= allow_g
    if with_target:
        print(f'target features: distance {rel(got["ft"].permute(0, 3, 1, 2), refs["target"][0]):.2e}, allowed {refs["target"][2]:.2e}')
        assert rel(got['ft'].permute(0, 3, 1, 2), refs['target'][0]) <= refs['target'][2]
