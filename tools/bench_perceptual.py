"""The multi-layer perceptual loss (``train --perceptual realesrgan``) next to the single-layer one, every figure from a replayed
hipGraph in ONE process:

* the loss node, forward + backward to the source image, at batch 16 with 128 x 128 crops (the ESRGAN step's size) and with
  96 x 96 crops, fp32 and bf16 products, ``single`` (``VGGLoss``) against ``realesrgan`` (``PerceptualLoss``);
* the fused tap kernels against their unfused compositions at the largest tap (conv1_2 of a batch of 16 + 16 crops of
  128 x 128: 2 x 16 x 128 x 128 x 64 floats): the pool that sums ``|fs - ft|`` on the way against the pool plus an L1 pass over
  the two halves, and the pool backward that adds the tap's L1 gradient against pool backward, ``srx_l1_bwd`` and an add.

Every configuration is warmed up; a figure is the time per replay of a batch of replays between two device events, taken in
ROUNDS rounds that walk through all configurations in turn, so that a drift of the machine lands on every one of them; the table
gives the median, minimum and maximum of the rounds.  Features are the seeded random ones (the arithmetic does not depend on
them); the crops are uniform noise.

    python tools/bench_perceptual.py [--rounds 5] [--calls 20] [--out profiles/perceptual_times.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from bench_unet_disc import captured, timed  # noqa: E402

BATCH = 16


def node_fwd_bwd(module, src4, tgt4):
    one = torch.ones((), dtype=torch.float32, device=src4.device)

    def run():
        torch.autograd.grad(module.forward_nhwc(src4, tgt4), src4, one)
    return run


def tap_kernel_pairs(dev):
    """[(name, fused, unfused)] at conv1_2's size; every closure issues launches on the current stream only."""
    from torchsr_amd import _lib
    call, L = _lib.call, _lib.lib()
    n, h, w, c = BATCH, 128, 128, 64
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2 * n, h, w, c), generator=g).to(dev)
    dy = torch.randn((n, h // 2, w // 2, c), generator=g).to(dev)
    y = torch.empty((2 * n, h // 2, w // 2, c), device=dev)
    xs, xt = x[:n], x[n:]
    dx, tmp, tmp2 = torch.empty_like(xs), torch.empty_like(xs), torch.empty_like(xs)
    loss, ws, gscale = torch.zeros((), device=dev), torch.empty(2048, device=dev), torch.ones(1, device=dev)
    nb, numel = L.srx_tap_blocks(n, h, w, c), xs.numel()
    s = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731

    def fwd_fused():
        call('srx_maxpool2x2_relu_fwd_tap', x.data_ptr(), y.data_ptr(), 0, n, 2 * n, h, w, c, ws.data_ptr(), s())
        call('srx_tap_l1_finalize', ws.data_ptr(), nb, 0.1 / numel, loss.data_ptr(), 0, s())

    def fwd_unfused():
        call('srx_maxpool2x2_relu_fwd_tap', x.data_ptr(), y.data_ptr(), 0, n, 2 * n, h, w, c, None, s())
        call('srx_tap_l1_fwd', xs.data_ptr(), xt.data_ptr(), numel, 0.1, loss.data_ptr(), 0, ws.data_ptr(), s())

    def bwd_fused():
        call('srx_maxpool2x2_relu_bwd_tap', dy.data_ptr(), 0, xs.data_ptr(), xt.data_ptr(), dx.data_ptr(), 0, 0.1 / numel,
             gscale.data_ptr(), n, h, w, c, s())

    def bwd_unfused():
        call('srx_maxpool2x2_relu_bwd', dy.data_ptr(), xs.data_ptr(), tmp.data_ptr(), n, h, w, c, s())
        call('srx_l1_bwd', xs.data_ptr(), xt.data_ptr(), gscale.data_ptr(), tmp2.data_ptr(), None, numel, s())
        call('srx_axpby', tmp.data_ptr(), tmp2.data_ptr(), dx.data_ptr(), numel, 1.0, 0.1, s())

    gb = x.numel() * 4 / 1e9
    return [('tap pool fwd + L1 (conv1_2)', fwd_fused, fwd_unfused, f'{gb:.2f} GB read once / twice'),
            ('tap pool bwd + L1 grad (conv1_2)', bwd_fused, bwd_unfused, '')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20, help='replays per round and configuration')
    ap.add_argument('--out', type=str, default=os.path.join('profiles', 'perceptual_times.txt'))
    args = ap.parse_args()
    if args.rounds < 3 or args.rounds * args.calls < 100:
        raise SystemExit('bench_perceptual: at least 3 rounds and 100 timed replays per figure')
    if not torch.cuda.is_available():
        raise SystemExit('bench_perceptual: needs the MI355X (no CPU timing says anything about it)')
    dev = torch.device('cuda:0')
    from torchsr_amd import functional as F
    from torchsr_amd.layers import set_conv_precision
    from torchsr_amd.realesrgan.loss import PerceptualLoss
    from torchsr_amd.srgan.loss import VGGLoss
    # A captured graph holds addresses, not tensors: every closure -- with its module, packed weights and images -- is kept until the
    # last replay (the next capture empties the allocator's cache, and a graph replayed after that would read freed memory).
    configs, keep = [], []

    def graph_of(fn):
        keep.append(fn)
        return captured(fn)
    for crop in (128, 96):
        _lr, hr = bench._crops(dev, BATCH, crop, 78)
        tgt4 = F.to_nhwc(hr, 4)
        src4 = F.to_nhwc(torch.rand(BATCH, 3, crop, crop, generator=torch.Generator().manual_seed(1)).to(dev), 4).requires_grad_(True)
        for precision in ('fp32', 'bf16'):
            for name, cls in (('single', VGGLoss), ('realesrgan', PerceptualLoss)):
                module = cls(weights='random').to(dev)
                set_conv_precision(module, precision)
                configs.append((f'node fwd+bwd {crop}x{crop} {precision} {name}', graph_of(node_fwd_bwd(module, src4, tgt4))))
    pairs = tap_kernel_pairs(dev)
    for name, fused, unfused, _ in pairs:
        configs += [(f'{name}, fused', graph_of(fused)), (f'{name}, unfused', graph_of(unfused))]
    for _, fn in configs:
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in configs}
    for _ in range(args.rounds):
        for name, fn in configs:
            times[name].append(timed(fn, args.calls))
    med = {name: statistics.median(ts) for name, ts in times.items()}
    lines = ['Multi-layer perceptual loss (train --perceptual realesrgan): measured times (MI355X, one session)', '',
             'python tools/bench_perceptual.py', '',
             f'{args.rounds} rounds through all configurations after warm-up; {args.calls} replays per round and configuration; time per '
             f'replay on the device (events around a batch); batch {BATCH}; every figure is a replayed hipGraph', '',
             f'{"":<46s} {"median":>9s} {"min":>9s} {"max":>9s}  {"spread":>7s}   (milliseconds)']
    for name, _ in configs:
        ts = times[name]
        lines.append(f'{name:<46s} {med[name]:9.3f} {min(ts):9.3f} {max(ts):9.3f}  {max(ts) - min(ts):7.3f}')
    lines.append('')
    for crop in (128, 96):
        for precision in ('fp32', 'bf16'):
            a, b = med[f'node fwd+bwd {crop}x{crop} {precision} single'], med[f'node fwd+bwd {crop}x{crop} {precision} realesrgan']
            lines.append(f'node, {crop}x{crop} {precision}: realesrgan - single = {b - a:+.3f} ms ({b / a:.3f}x)')
    for name, _f, _u, note in pairs:
        a, b = med[f'{name}, fused'], med[f'{name}, unfused']
        verdict = 'the fused kernel is faster and is what the node runs' if a < b else \
            'the fused kernel is NOT faster than its unfused composition here'
        lines.append(f'{name}: fused {a:.3f} ms, unfused {b:.3f} ms: {verdict}{" (" + note + ")" if note else ""}')
    lines += ['', 'The ESRGAN GAN step with each loss is not measured here.']
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
