"""Trace every C-ABI call of the training steps and of inference (developer tool, needs the GPU): the check that a change to the
host code -- the autograd Functions and launchers of torchsr_amd/functional.py -- changed no launch.

    python tools/call_trace.py OUT.txt      # once per tree, both against the same library (SRX_LIB); then `cmp` the two files

``_lib.call`` and every module-level alias of it in the package are wrapped (as tests/step_layers.py::record_op_calls does, but for
every entry point, the conv ones included).  One line per call: the name, then per argument -- by the declared ctypes signature --
the value of an int / int64 / size_t / float, the fields of a conv descriptor, and for any other pointer only whether it is null.
Each case runs eagerly (no hipGraph), from one seed, at the smallest sizes the step tests use (batch 2, their trainer settings,
their golden inputs): three SRGAN steps, three ESRGAN steps in fp32 and three under autocast (bf16-storage VGG stack, fused dense
blocks) -- the first packs lazily per layer, the later ones after the pack tables took over --, the VGG loss forward and backward
alone, and Generator inference in fp32, bf16 and fp16: a first call, a second (every pack current) and a third after an in-place
update of one weight that changes no value (that layer's repack and nothing else); then every calling form of the two
perceptual-loss nodes (``frozen_stack_cases``), each followed by a ``=`` line with digests of its results.  The digest of the
library's sources is the first line.  Sizing calls made on the library handle directly (``*_ws_floats``) are not traced; the sizes they return are
(``nws`` arguments).  A swapped pair of non-null pointers is invisible here: the numerical tests cover that.
"""
import ctypes as C
import hashlib
import os
import sys
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from oracle.weights import closed_form_state, step_state  # noqa: E402
from torchsr_amd import _lib  # noqa: E402
import torchsr_amd.esrgan.trainer  # noqa: E402,F401  (every module that binds `call` is loaded before the wrap)
import torchsr_amd.srgan.trainer  # noqa: E402,F401
import torchsr_amd.functional  # noqa: E402,F401
import torchsr_amd.optim  # noqa: E402,F401
import torchsr_amd.test  # noqa: E402,F401

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
VALUES = (C.c_int, C.c_int64, C.c_size_t, C.c_float)
DESC = C.POINTER(_lib.Conv2dDesc)


def show(v, t) -> str:
    if t in VALUES:
        return repr(float(v)) if t is C.c_float else str(int(v))
    if t is DESC and v is not None:
        d = v._obj if hasattr(v, '_obj') else v.contents  # ctypes.byref(d), or ctypes.pointer(d)
        return '{' + ','.join(format(getattr(d, f), '.9g' if ft is C.c_float else 'd') for f, ft in d._fields_) + '}'
    null = v is None or v == 0 or (isinstance(v, C.c_void_p) and not v.value)
    return 'null' if null else 'ptr'


def traced(out, tag, fn) -> None:
    """Run ``fn`` with the wrap in place; its calls go to ``out`` under the heading ``tag``."""
    real = _lib.call

    def spy(name, *args):
        out.append(name + ' ' + ' '.join(show(v, t) for v, t in zip(args, _lib._SIGS[name][1])))
        return real(name, *args)

    bound = [(mod, attr) for name, mod in list(sys.modules.items())
             if mod is not None and (name == 'torchsr_amd' or name.startswith('torchsr_amd.'))
             for attr, val in list(vars(mod).items()) if val is real]
    out.append('# ' + tag)
    for mod, attr in bound:
        setattr(mod, attr, spy)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        for mod, attr in bound:
            setattr(mod, attr, real)


def trainer(cls, dev, tag, disable_amp):
    """The settings of ``make_trainer`` in tests/test_step_gpu.py and tests/test_esrgan_gpu.py, batch 2, no hipGraph."""
    args = Namespace(disable_amp=disable_amp, batch_size=2, epochs=8, gan_checkpoint=None, local_rank=0, pretrain_epochs=1,
                     psnr_checkpoint=None, skip_image_save=True, world_size=1, rank=-1, use_graphs=False, vgg_weights='random')
    t = cls(dev, args, [], [], 2, 2, distributed=False)
    t.generator.load_state_dict(step_state(t.generator.state_dict(), tag + '.G'))
    t.discriminator.load_state_dict(step_state(t.discriminator.state_dict(), tag + '.D'))
    t.vgg_loss.features.load_state_dict(closed_form_state(t.vgg_loss.features.state_dict(), prefix='features.'))
    t.generator.train()
    t.discriminator.train()
    return t


def sha(t) -> str:
    return hashlib.sha256(t.detach().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def frozen_stack_cases(out, dev, vgg, src, tgt) -> None:
    """Every path through the frozen-stack walk behind ``VGGLoss`` and ``PerceptualLoss`` (functional.frozen_conv_stack /
    frozen_tap_stack): fp32 and bf16 storage, [source; target] and source alone, stack prefixes, the general LeakyReLU stack; each
    once more on the direct kernels (``_dev.NO_WINO``) and, where bf16, on fp32 storage (``_dev.NO_BF16S``).  Behind each case a
    ``=`` line with the sha256 of the result's and the input gradient's bytes: two trees must agree on those too."""
    from torchsr_amd import _dev
    from torchsr_amd import functional as F
    from torchsr_amd._lib import ACT_LRELU
    from torchsr_amd.layers import Conv2d, set_conv_precision
    from torchsr_amd.realesrgan.loss import PerceptualLoss
    percep = PerceptualLoss(weights='random').to(dev)
    src4, tgt4 = F.to_nhwc(src, 4), F.to_nhwc(tgt, 4)
    g = torch.Generator().manual_seed(5)
    convs = [Conv2d(3, 16, 3, 1, 1, act=ACT_LRELU, slope=0.2), Conv2d(16, 32, 3, 1, 1, act=ACT_LRELU, slope=0.2)]
    for m in convs:
        with torch.no_grad():
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * 0.2)
            m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
        m.to(dev).requires_grad_(False)
    lrelu = [('conv', convs[0]), ('pool', None), ('conv', convs[1])]
    small = torch.rand(2, 8, 12, 4, generator=g).to(dev)
    small[..., 3] = 0
    small_t = small.flip(0).contiguous()

    def case(tag, fn, x=None):
        """``fn(x)`` -> a loss (differentiated when ``x`` is given) or a list of tensors"""
        res = []

        def run():
            leaf = None if x is None else x.clone().requires_grad_(True)
            y = fn(leaf)
            if leaf is not None:
                y.backward()
                res.extend([y, leaf.grad])
            else:
                res.extend(y)
        traced(out, tag, run)
        out.append('= ' + ' '.join(sha(t) for t in res))

    def features_sum(layers, x, t):
        fs, _ = F.frozen_conv_stack(x, t, layers)
        return fs.sum()

    def cases(precision, switch):
        tag = precision + ('' if switch is None else ', ' + switch)
        stack = vgg._stack()
        with torch.no_grad():
            tf_vgg = vgg.target_features(tgt)
        case('VGG loss, source + target, ' + tag, lambda x: vgg.forward_nhwc(x, tgt4), src4)
        case('VGG loss, source + target_features, ' + tag, lambda x: vgg.forward_nhwc(x, None, target_features=tf_vgg), src4)
        if precision == 'bf16':
            for k in (2, 4, 5):
                case('frozen_conv_stack, layers[:%d], %s' % (k, tag), lambda x: features_sum(stack[:k], x, None), src4)
        case('perceptual loss, target_features() alone, ' + tag, lambda _: percep.target_features(tgt))
        tf_p = percep.target_features(tgt)
        case('perceptual loss, source + target, ' + tag, lambda x: percep.forward_nhwc(x, tgt4), src4)
        case('perceptual loss, source + target_features, ' + tag, lambda x: percep.forward_nhwc(x, None, target_features=tf_p), src4)
        if precision == 'fp32':
            case('LeakyReLU stack, source alone, ' + tag, lambda x: features_sum(lrelu, x, None), small)
            case('LeakyReLU stack, source + target, ' + tag, lambda x: features_sum(lrelu, x, small_t), small)

    for precision in ('fp32', 'bf16'):
        set_conv_precision(vgg, precision)
        set_conv_precision(percep, precision)
        for switch in (None, 'NO_WINO') + (('NO_BF16S',) if precision == 'bf16' else ()):
            was = None if switch is None else getattr(_dev, switch)
            if switch is not None:
                setattr(_dev, switch, True)
            try:
                cases(precision, switch)
            finally:
                if switch is not None:
                    setattr(_dev, switch, was)
    set_conv_precision(vgg, 'fp32')


def main():
    from torchsr_amd.esrgan.trainer import ESRGANTrainer
    from torchsr_amd.srgan.generator import Generator
    from torchsr_amd.srgan.loss import VGGLoss
    from torchsr_amd.srgan.trainer import SRGANTrainer
    from torchsr_amd.test import upscale
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    out = []

    def step(cls, tag, gold, disable_amp, what):
        g = np.load(os.path.join(GOLDEN, gold))
        lr, hr = torch.from_numpy(g['low_res']).to(dev), torch.from_numpy(g['high_res']).to(dev)
        t = trainer(cls, dev, tag, disable_amp)
        for i in (1, 2, 3):
            traced(out, '%s, step %d' % (what, i), lambda: t.gan_step(lr, hr))

    out.append('# library sources ' + _lib.source_digest())
    step(SRGANTrainer, 'srgan', 'srgan_steps.npz', True, 'SRGAN, fp32')
    step(ESRGANTrainer, 'esrgan', 'esrgan.npz', True, 'ESRGAN, fp32')
    step(ESRGANTrainer, 'esrgan', 'esrgan.npz', False, 'ESRGAN, autocast')

    vgg = VGGLoss(weights='random').to(dev)
    src, tgt = torch.rand(2, 3, 32, 48, device=dev).requires_grad_(True), torch.rand(2, 3, 32, 48, device=dev)
    traced(out, 'VGG loss forward and backward, fp32', lambda: vgg(src, tgt).backward())

    gen = Generator().to(dev)
    low = torch.rand(2, 3, 24, 24, device=dev)
    for precision in ('fp32', 'bf16', 'fp16'):
        traced(out, 'Generator inference, %s, first call' % precision, lambda: upscale(gen, low, precision=precision))
        traced(out, 'Generator inference, %s, second call' % precision, lambda: upscale(gen, low, precision=precision))
        with torch.no_grad():
            gen.conv1[0].weight.mul_(1.0)
        traced(out, 'Generator inference, %s, after an in-place update of conv1' % precision,
               lambda: upscale(gen, low, precision=precision))

    frozen_stack_cases(out, dev, vgg, src.detach(), tgt)

    with open(sys.argv[1], 'w') as f:
        f.write('\n'.join(out) + '\n')
    print('%d calls in %d cases written to %s' % (sum(ln[0] not in '#=' for ln in out), sum(ln.startswith('#') for ln in out) - 1,
                                                  sys.argv[1]))


if __name__ == '__main__':
    main()
