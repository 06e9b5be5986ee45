"""The U-Net discriminator (``train --discriminator unet``) next to the VGG-style one, at batch 16 and 128 x 128 crops, bf16
products (the ESRGAN GAN phase's arithmetic), every figure from a replayed hipGraph in ONE process:

* forward + backward of each discriminator on the 2N batch with its own loss (what the D phase of a step runs),
* the ESRGAN GAN step with each discriminator (``gan_step``, the trainers' captured graph),
* the eight spectral-norm forwards alone (training mode: the power iteration and the W / sigma pass of every layer), and
  with their backwards (the closed-form dW accumulated into the flat gradient buffer).

The discriminators run as they do inside a trainer's D phase: parameters and gradients in ``FlatParams`` buffers, weight
gradients accumulated straight into them (``functional.direct_grads``) and issued together by the ``WeightGradQueue``.

Every configuration is warmed up; a figure is the time per replay of a batch of replays between two device events, taken in
ROUNDS rounds that walk through all configurations in turn, so that a drift of the machine lands on every one of them; the
table gives the median, minimum and maximum of the rounds.  Weights are the modules' seeded default initialisation (the
arithmetic does not depend on them); the crops are uniform noise.

``--ab FILE`` appends the regression check of the headline step to the same report: FILE holds the output of
``tools/ab.sh <parent library> <this library> 3`` run in the same session (lines ``<library file name> <ms per step>``, the two
libraries alternating); the first name met is the parent.

    python tools/bench_unet_disc.py [--rounds 5] [--calls 20] [--ab FILE] [--out profiles/unet_disc_times.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402

BATCH, CROP = 16, 128


def timed(fn, calls):
    """Milliseconds per call of ``calls`` calls of ``fn`` on the device (one pair of events around the batch)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def captured(fn, warm=3):
    """``fn`` as a replayed hipGraph: ``warm`` eager calls on a side stream, the capture, one replay."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(warm):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    return g.replay


def disc_fwd_bwd(disc, real4, fake4):
    """The D phase's work on the discriminator, as ``_phase_disc_loss`` issues it: one memset of the flat gradient, the 2N forward,
    its loss, the backward with the weight gradients accumulated into the flat buffer and issued together at its end."""
    from torchsr_amd import functional as F
    from torchsr_amd.optim import FlatParams
    flat = FlatParams(disc)
    one = torch.ones((), dtype=torch.float32, device=real4.device)

    def run():
        flat.zero_grad()
        loss, _ = disc.pair_loss_nhwc(real4, fake4)
        with F.deferred_weight_grads():
            loss.backward(one)
    return run


def sn_forwards(disc):
    layers = [m for m in disc.modules() if hasattr(m, 'normalised_weight')]
    assert len(layers) == 8

    def run():
        with torch.no_grad():
            for m in layers:
                m.normalised_weight()
    return run, sum(m.weight_orig.numel() for m in layers) * 4


def sn_forwards_backwards(disc):
    """The eight normalisations with their backwards: G = dL/dW_sn is a fixed tensor per layer, dW goes to ``weight_orig.grad``."""
    layers = [m for m in disc.modules() if hasattr(m, 'normalised_weight')]
    grads = [torch.randn_like(m.weight_orig) for m in layers]

    def run():
        for m, g in zip(layers, grads):
            m.normalised_weight().backward(g)
    return run


def ab_section(path):
    """Section 2 of the report from the output of tools/ab.sh (parent first)."""
    rows = {}
    with open(path) as f:
        for line in f:
            parts = line.split()
            if len(parts) == 2:
                rows.setdefault(parts[0], []).append(float(parts[1]))
    if len(rows) != 2 or len({len(v) for v in rows.values()}) != 1:
        raise SystemExit(f'bench_unet_disc: {path} must hold alternating lines of two libraries, got {dict(rows)}')
    (pa, a), (pb, b) = rows.items()
    med = statistics.median
    lines = ['', '2. Headline step (bench.py: SRGAN GAN step, batch 16, 96 x 96, fp32; --discriminator vgg is the default and selects the',
             f'   same trainer classes as before): the parent commit\'s library ({pa}) against this one ({pb}) in the same session,',
             f'   {len(a)} alternating rounds of tools/ab.sh, milliseconds per step', '',
             f'     {"round":<8s} {"parent":>8s} {"this":>8s}']
    lines += [f'     {i + 1:<8d} {x:8.3f} {y:8.3f}' for i, (x, y) in enumerate(zip(a, b))]
    lines += [f'     {"median":<8s} {med(a):8.3f} {med(b):8.3f}', '',
              f'   the parent\'s own spread over its rounds: {min(a):.3f} .. {max(a):.3f} ms; this library\'s median {med(b):.3f} ms lies '
              f'{"inside" if min(a) <= med(b) <= max(a) else ("below" if med(b) < min(a) else "ABOVE")} it']
    return lines


def gan_stepper(dev, discriminator, seed):
    from torchsr_amd.models import select_trainer_model
    args = bench._targs(BATCH, True, model='esrgan', discriminator=discriminator)
    cls, _ = select_trainer_model(args)
    torch.manual_seed(0)
    t = cls(dev, args, [], [], BATCH, BATCH)
    t.generator.train()
    t.discriminator.train()
    lr, hr = bench._crops(dev, BATCH, CROP, seed)
    for _ in range(8):  # two eager passes, the capture, five replays
        t.gan_step(lr, hr)
    torch.cuda.synchronize()
    assert 'gan.all' in t._graphs
    return lambda: t.gan_step(lr, hr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20, help='replays per round and configuration')
    ap.add_argument('--ab', type=str, default=None, help='output of tools/ab.sh <parent library> <this library>: appended as section 2')
    ap.add_argument('--out', type=str, default=os.path.join('profiles', 'unet_disc_times.txt'))
    args = ap.parse_args()
    if args.rounds < 3 or args.rounds * args.calls < 100:
        raise SystemExit('bench_unet_disc: at least 3 rounds and 100 timed replays per figure')
    if not torch.cuda.is_available():
        raise SystemExit('bench_unet_disc: needs the MI355X (no CPU timing says anything about it)')
    dev = torch.device('cuda:0')
    from torchsr_amd import functional as F
    from torchsr_amd.esrgan.discriminator import Discriminator
    from torchsr_amd.layers import set_conv_precision
    from torchsr_amd.realesrgan.discriminator import UNetDiscriminatorSN
    torch.manual_seed(0)
    _lr, hr = bench._crops(dev, BATCH, CROP, 78)
    real4 = F.to_nhwc(hr, 4)
    fake4 = F.to_nhwc(torch.rand(BATCH, 3, CROP, CROP, generator=torch.Generator().manual_seed(1)).to(dev), 4)
    vgg, unet = Discriminator(image_size=CROP).to(dev).train(), UNetDiscriminatorSN().to(dev).train()
    for m in (vgg, unet):
        set_conv_precision(m, 'bf16')
    F.direct_grads[0] = True  # as in a trainer: parameter gradients accumulate straight into the flat .grad views
    sn_run, sn_bytes = sn_forwards(unet)
    configs = [('D fwd+bwd, vgg (2N = 32)', captured(disc_fwd_bwd(vgg, real4, fake4))),
               ('D fwd+bwd, unet (2N = 32)', captured(disc_fwd_bwd(unet, real4, fake4))),
               ('8 spectral-norm forwards', captured(sn_run)),
               ('8 spectral-norm fwd + bwd', captured(sn_forwards_backwards(unet))),
               ('ESRGAN GAN step, vgg', gan_stepper(dev, 'vgg', 78)),
               ('ESRGAN GAN step, unet', gan_stepper(dev, 'unet', 78))]
    for _, fn in configs:
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in configs}
    for _ in range(args.rounds):
        for name, fn in configs:
            times[name].append(timed(fn, args.calls))
    lines = ['U-Net discriminator (train --discriminator unet): measured times (MI355X, one session)', '', '1. python tools/bench_unet_disc.py', '',
             f'{args.rounds} rounds through all configurations after warm-up; {args.calls} replays per round and configuration; time per '
             f'replay on the device (events around a batch); batch {BATCH}, {CROP} x {CROP} crops, bf16 products; every figure is a '
             f'replayed hipGraph', '',
             f'{"":<30s} {"median":>9s} {"min":>9s} {"max":>9s}  {"spread":>7s}   (milliseconds)']
    for name, _ in configs:
        ts = times[name]
        lines.append(f'{name:<30s} {statistics.median(ts):9.3f} {min(ts):9.3f} {max(ts):9.3f}  {max(ts) - min(ts):7.3f}')
    sn = statistics.median(times['8 spectral-norm forwards'])
    lines += ['', f'spectral norm: {sn_bytes / 1e6:.1f} MB of weights, three reads and one write per training forward = '
                  f'{4 * sn_bytes / 1e6:.1f} MB in {sn * 1e3:.1f} us = {4 * sn_bytes / (sn * 1e-3) / 1e12:.2f} TB/s end to end over 32 launches '
                  f'(the weights fit the 256 MB Infinity Cache: not an HBM rate); a GAN step runs these twice',
              f'GAN step, unet - vgg: {statistics.median(times["ESRGAN GAN step, unet"]) - statistics.median(times["ESRGAN GAN step, vgg"]):+.3f} ms']
    if args.ab:
        lines += ab_section(args.ab)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
