"""Reference for ``train --perceptual realesrgan``: BasicSR's ``PerceptualLoss`` with the options of Real-ESRGAN's
``train_realesrgan_x4plus.yml``, restated from its public definition in plain torch (``F.conv2d`` / ``relu`` / ``max_pool2d``),
in whatever dtype the inputs carry.

    vgg19.features[:35], use_input_norm (ImageNet mean / std), layer_weights conv1_2 0.1, conv2_2 0.1, conv3_4 1, conv4_4 1,
    conv5_4 1 -- all taken BEFORE the ReLU --, L1 criterion, perceptual_weight 1, no style term.

``bf16=True`` is the product's autocast arithmetic: every conv multiplies bf16-rounded operands (``oracle.srgan._ConvBF16``).
The activations the bf16-storage path keeps as bf16 -- the outputs of the non-tap convs and of the pools -- feed convs only, so
rounding them where they are stored is the rounding their consumer applies: ``stored`` is written out all the same.
"""
import torch
import torch.nn.functional as F

from oracle import srgan as O

VGG19_CFG = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 256, 'M', 512, 512, 512, 512, 'M', 512, 512, 512, 512, 'M']
LAYER_WEIGHTS = {'conv1_2': 0.1, 'conv2_2': 0.1, 'conv3_4': 1.0, 'conv4_4': 1.0, 'conv5_4': 1.0}
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
CONV_INDICES = [0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28, 30, 32, 34]


def layout():
    """[(features index, kind, name)] of ``vgg19.features[:35]``: kind 'conv' | 'relu' | 'pool'; name ``convB_K`` / ``reluB_K`` / ``poolB``."""
    out, idx, block, k = [], 0, 1, 0
    for v in VGG19_CFG:
        if v == 'M':
            out.append((idx, 'pool', f'pool{block}'))
            idx, block, k = idx + 1, block + 1, 0
        else:
            k += 1
            out += [(idx, 'conv', f'conv{block}_{k}'), (idx + 1, 'relu', f'relu{block}_{k}')]
            idx += 2
    return out[:35]


def normalize(x):
    mean = torch.tensor(MEAN, dtype=x.dtype).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=x.dtype).view(1, 3, 1, 1)
    return (x - mean) / std


def _conv(x, w, b, bf16):
    if bf16:
        with O.bf16_products():
            return O.conv2d(x, w, b, 1, 1)
    return F.conv2d(x, w, b, 1, 1)


def features(sd, x, bf16=False, pool_first=False, prefix=''):
    """{name: pre-ReLU feature} of the five taps; ``x`` NCHW in [0, 1], ``sd``: ``{prefix}{index}.weight / .bias`` in x's dtype.
    ``pool_first``: behind a tap the pool runs before the ReLU (what the product does) instead of after it."""
    stored = O._r if bf16 else (lambda t: t)
    out, feats, lay = normalize(x), {}, layout()
    i = 0
    while i < len(lay):
        idx, kind, name = lay[i]
        if kind == 'conv':
            out = _conv(out, sd[f'{prefix}{idx}.weight'], sd[f'{prefix}{idx}.bias'], bf16)
            if name in LAYER_WEIGHTS:
                feats[name] = out
                if pool_first and i + 2 < len(lay) and lay[i + 2][1] == 'pool':
                    out = stored(F.relu(F.max_pool2d(out, 2, 2)))
                    i += 3
                    continue
        elif kind == 'relu':
            out = F.relu(out)
            if i + 1 < len(lay) and lay[i + 1][1] != 'pool':
                out = stored(out)       # a non-tap conv's bf16 output
        else:
            out = stored(F.max_pool2d(out, 2, 2))
        i += 1
    return feats


def perceptual_loss(sd, source, target, bf16=False, pool_first=False, prefix=''):
    fs = features(sd, source, bf16, pool_first, prefix)
    ft = features(sd, target.detach(), bf16, pool_first, prefix)
    return sum(LAYER_WEIGHTS[k] * F.l1_loss(fs[k], ft[k]) for k in LAYER_WEIGHTS)


def hooked_loss(sd, source, target):
    """The same loss by an independent route: an ``nn.Sequential`` of torch modules, features collected by forward hooks."""
    mods = []
    for idx, kind, _name in layout():
        if kind == 'conv':
            w = sd[f'{idx}.weight']
            m = torch.nn.Conv2d(w.shape[1], w.shape[0], 3, 1, 1).to(w.dtype)
            with torch.no_grad():
                m.weight.copy_(w)
                m.bias.copy_(sd[f'{idx}.bias'])
            mods.append(m)
        else:
            mods.append(torch.nn.ReLU() if kind == 'relu' else torch.nn.MaxPool2d(2, 2))
    net = torch.nn.Sequential(*mods)
    taps = {idx: name for idx, kind, name in layout() if kind == 'conv' and name in LAYER_WEIGHTS}
    got = {}
    hooks = [net[idx].register_forward_hook(lambda _m, _i, o, name=name: got.__setitem__(name, o)) for idx, name in taps.items()]
    try:
        net(normalize(source))
        fs = dict(got)
        net(normalize(target))
        ft = dict(got)
    finally:
        for h in hooks:
            h.remove()
    return sum(LAYER_WEIGHTS[k] * (fs[k] - ft[k]).abs().mean() for k in LAYER_WEIGHTS)


def random_state(seed=1234, dtype=torch.float32):
    """``PerceptualLoss(weights='random', seed=seed)``'s features: kaiming-normal (fan_out) weights, zero biases, fp32 draws."""
    g = torch.Generator().manual_seed(seed)
    sd, cin = {}, 3
    convs = [v for v in VGG19_CFG if v != 'M']
    for idx, cout in zip(CONV_INDICES, convs):
        sd[f'{idx}.weight'] = (torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (cout * 9)) ** 0.5).to(dtype)
        sd[f'{idx}.bias'] = torch.zeros(cout, dtype=dtype)
        cin = cout
    return sd
