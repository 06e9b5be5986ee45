"""Training at x2 next to x4: the ESRGAN GAN step (23 blocks, batch 16, 128 x 128 targets, bf16 products, captured as a hipGraph)
with ``--scale 2`` -- a 64 x 64 input behind pixel_unshuffle(2) -- and with the default x4 -- a 32 x 32 input -- and the x2 input
layer's weight gradient (``srx_unshuffle2_conv_bwd_weight``, csrc/unshuffle.hip) alone at the step's size.

Both steps run a 32 x 32 trunk; the expectation stated next to the numbers is that they differ by the input layer only (the
loader is outside the step: both are fed device tensors).

One process; every configuration is warmed up (the trainers until their step is a replayed graph); a figure is the time per call
of a batch of calls between two device events, taken in ROUNDS rounds that walk through all configurations in turn, so that a
drift of the machine lands on every one of them; the table gives the median, minimum and maximum of the rounds.  Weights are the
seeded defaults (the arithmetic does not depend on them), VGG19 is seeded random, the batch is uniform noise.

    python tools/bench_x2_train.py [--rounds 5] [--steps 20] [--out profiles/x2_train_times.txt]
"""
import argparse
import os
import statistics
import sys
import warnings
from argparse import Namespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as TF  # noqa: E402

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


def trainer(dev, scale):
    from torchsr_amd.esrgan.trainer import ESRGANTrainer
    args = Namespace(disable_amp=False, batch_size=BATCH, epochs=8, gan_checkpoint=None, local_rank=0, pretrain_epochs=1,
                     psnr_checkpoint=None, skip_image_save=True, world_size=1, rank=-1, use_graphs=True, vgg_weights='random',
                     model='esrgan', scale=scale)
    torch.manual_seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        t = ESRGANTrainer(dev, args, [], [], BATCH, BATCH, distributed=False)
    t.generator.train()
    t.discriminator.train()
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20, help='steps per round and configuration')
    ap.add_argument('--out', type=str, default=os.path.join('profiles', 'x2_train_times.txt'))
    args = ap.parse_args()
    if args.rounds < 3 or args.rounds * args.steps < 100:
        raise SystemExit('bench_x2_train: at least 3 rounds and 100 timed steps per figure')
    if not torch.cuda.is_available():
        raise SystemExit('bench_x2_train: needs the MI355X (no CPU timing says anything about it)')
    dev = torch.device('cuda:0')
    from torchsr_amd import _lib
    hr = torch.rand(BATCH, 3, CROP, CROP, generator=torch.Generator().manual_seed(0)).to(dev)
    configs = []
    for scale in (2, 4):
        t, lr = trainer(dev, scale), TF.avg_pool2d(hr, scale)
        for _ in range(4):  # two eager steps, the capture, a replay
            losses = t.gan_step(lr, hr)
        if 'gan.all' not in t._graphs or not all(torch.isfinite(v).all() for v in losses.values()):
            raise SystemExit(f'bench_x2_train: the x{scale} step was not captured, or its losses are not finite')
        configs.append((f'ESRGAN GAN step x{scale} ({CROP // scale} x {CROP // scale} input)', lambda t=t, lr=lr: t.gan_step(lr, hr)))
    # the kernel alone, at the step's size: image [16, 64, 64, 4], dy [16, 32, 32, 64]
    n, h, w = BATCH, CROP // 2, CROP // 2
    x4 = torch.rand(n, h, w, 4, device=dev)
    dy = torch.randn(n, h // 2, w // 2, 64, device=dev)
    dw = torch.zeros(64, 12, 3, 3, device=dev)
    nws = _lib.lib().srx_unshuffle2_conv_wgrad_ws_floats(n, h, w)
    ws = torch.empty(nws, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    configs.append(('unshuffle2 weight gradient (kernel + reduce)',
                    lambda: _lib.call('srx_unshuffle2_conv_bwd_weight', n, h, w, x4.data_ptr(), dy.data_ptr(), dw.data_ptr(), 0,
                                      ws.data_ptr(), nws, s)))
    for _, fn in configs:
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in configs}
    for _ in range(args.rounds):
        for name, fn in configs:
            times[name].append(timed(fn, args.steps))
    lines = [f'{args.rounds} rounds through all configurations after warm-up; {args.steps} calls per round and configuration; time per '
             f'call on the device (events around a batch)', '',
             f'batch {BATCH}, {CROP} x {CROP} targets, bf16 products, 23 blocks, one hipGraph per step: milliseconds',
             f'{"":<48s} {"median":>9s} {"min":>9s} {"max":>9s}  {"spread":>7s}']
    for name, _ in configs:
        ts = times[name]
        lines.append(f'{name:<48s} {statistics.median(ts):9.3f} {min(ts):9.3f} {max(ts):9.3f}  {max(ts) - min(ts):7.3f}')
    med = {name: statistics.median(ts) for name, ts in times.items()}
    (n2, _), (n4, _), (nk, _) = configs
    lines += ['', f'x2 step - x4 step = {med[n2] - med[n4]:+.3f} ms ({med[n2] / med[n4]:.3f} x); expected: the input layer only -- the x2 '
              f'layer\'s forward, pack and weight gradient ({med[nk]:.3f} ms of it) in place of the 3 -> 64 conv\'s; the trunk, the '
              'tail, the critic and the losses see the same shapes']
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
