"""RRDBNet at x2 (``esrgan.Generator(23, scale_factor=2)``, RealESRGAN_x2plus's net) on the 1080p frame:

(a) its input layer -- pixel_unshuffle(2) + 3x3 conv over 12 channels as ONE launch on the image, unshuffle2_conv_fwd_kernel
    (csrc/unshuffle.hip) -- against the generic gather-GEMM's launch of the same layer written as a 6x6 / stride 2 / pad 2 conv
    over the NHWC-4 image (``v[o][c][2 ky + dy][2 kx + dx] = w[o][4 c + 2 dy + dx][ky][kx]``; even sizes only, which is why it
    is the A/B partner and not a second dispatch), fp32 and bf16 products; the two results are compared first;
(b) the whole 1080p -> 4K frame with 23 blocks at both precisions, next to the x4 frame (1080p -> 8K) of the same net.

One process; every configuration is warmed up; a figure is the time per call of a batch of calls between two device events,
taken in ROUNDS rounds that walk through all configurations in turn, so that a drift of the machine lands on every one of
them; the tables give the median, minimum and maximum of the rounds.  The weights are seeded random values (the arithmetic
does not depend on them); the frame is uniform noise.

    python tools/bench_rrdbnet_x2.py [--rounds 5] [--calls 40] [--frames 2] [--out profiles/rrdbnet_x2_times.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def timed(fn, calls):
    """Milliseconds per call of ``calls`` calls of ``fn`` on the device (one pair of events around the batch)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def alternate(configs, rounds, calls):
    """``configs``: [(name, fn)].  Two warm-up calls each, then ``rounds`` rounds in order; returns {name: [ms per call]}."""
    for _, fn in configs:
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in configs}
    for _ in range(rounds):
        for name, fn in configs:
            times[name].append(timed(fn, calls))
    return times


def table(times, order, extra=lambda name, med: ''):
    lines = [f'{"":<34s} {"median":>9s} {"min":>9s} {"max":>9s}  {"spread":>7s}']
    for name in order:
        ts = times[name]
        med = statistics.median(ts)
        lines.append(f'{name:<34s} {med:9.3f} {min(ts):9.3f} {max(ts):9.3f}  {max(ts) - min(ts):7.3f}  {extra(name, med)}')
    return lines


def as_6x6_stride2(w):
    """OIHW [64, 12, 3, 3] over the unshuffled image -> OIHW [64, 3, 6, 6] over the image."""
    v = torch.empty(w.shape[0], 3, 6, 6, dtype=w.dtype)
    for c in range(3):
        for dy in range(2):
            for dx in range(2):
                v[:, c, dy::2, dx::2] = w[:, 4 * c + 2 * dy + dx]
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=40, help='launches of the input layer per round and configuration')
    ap.add_argument('--frames', type=int, default=2, help='whole frames per round and configuration')
    ap.add_argument('--blocks', type=int, default=23)
    ap.add_argument('--out', type=str, default=os.path.join('profiles', 'rrdbnet_x2_times.txt'))
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    args = ap.parse_args()
    if args.rounds < 3:
        raise SystemExit('bench_rrdbnet_x2: at least 3 rounds')
    if args.height % 2 or args.width % 2:
        raise SystemExit('bench_rrdbnet_x2: the generic 6x6 / stride 2 partner has no reflected edge: even sizes')
    if not torch.cuda.is_available():
        raise SystemExit('bench_rrdbnet_x2: needs the MI355X (no CPU timing says anything about it)')
    dev = torch.device('cuda:0')
    from torchsr_amd import functional as F
    from torchsr_amd.esrgan.generator import Generator
    from torchsr_amd.layers import Conv2d
    from torchsr_amd.test import upscale
    h, w = args.height, args.width
    g = torch.Generator().manual_seed(0)
    lr = torch.rand(1, 3, h, w, generator=g).to(dev)
    gens = {s: Generator(args.blocks, scale_factor=s) for s in (2, 4)}
    with torch.no_grad():
        for s, gen in gens.items():  # biases away from the initialisation's zeros
            for k, p in gen.named_parameters():
                if k.endswith('.bias'):
                    p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 0.2)
            gen.to(dev).eval()
    lines = [f'{args.rounds} rounds through all configurations of a table after two warm-up calls each; time per call on the device '
             f'(events around a batch)', '']

    # (a) the input layer alone
    conv1 = gens[2].conv1
    generic = Conv2d(3, 64, kernel_size=6, stride=2, padding=2).to(dev).eval()
    with torch.no_grad():
        generic.weight.copy_(as_6x6_stride2(conv1.weight.detach().cpu()))
        generic.bias.copy_(conv1.bias)
        x4 = F.to_nhwc(lr, 4)
        configs = []
        for prec in (0, 1):
            def new(p=prec):
                conv1._st.precision = p
                return conv1(x4)

            def old(p=prec):
                generic._st.precision = p
                return generic(x4)
            a, b = new(), old()
            assert a.shape == b.shape == (1, h // 2, w // 2, 64)
            dist = ((a - b).abs().max() / b.abs().max()).item()
            lines.append(f'input layer, {"bf16" if prec else "fp32"} products: max |unshuffle2 kernel - generic 6x6/s2| = {dist:.3e} of '
                         f'the largest value')
            tag = 'bf16' if prec else 'fp32'
            configs += [(f'unshuffle2_conv_fwd_kernel {tag}', new), (f'generic 6x6 / stride 2 {tag}', old)]
            del a, b
        t = alternate(configs, args.rounds, args.calls)
        conv1._st.precision = generic._st.precision = 0
    out_mb = (h // 2) * (w // 2) * 256 / 1e6
    lines += ['', f'(a) input layer of the x2 net on a {w} x {h} frame ({out_mb:.0f} MB of output), {args.calls} launches per round: '
              f'milliseconds per launch']
    lines += table(t, [n for n, _ in configs], lambda n, med: f'{out_mb / med:7.1f} GB/s written')
    for tag in ('fp32', 'bf16'):
        a, b = statistics.median(t[f'unshuffle2_conv_fwd_kernel {tag}']), statistics.median(t[f'generic 6x6 / stride 2 {tag}'])
        lines.append(f'{tag}: the generic launch takes {b / a:.2f} x the unshuffle2 kernel\'s time ({b:.3f} vs {a:.3f} ms)')
    print('\n'.join(lines), flush=True)

    # (b) the whole frame; x2 tiles of the image hold 4 x the default's pixels -- the trunk runs on a quarter of them
    from torchsr_amd.test import MAX_TILE_PIXELS
    frames = []
    for prec in ('fp32', 'bf16'):
        frames.append((f'x2 {w}x{h} -> {2 * w}x{2 * h} {prec}',
                       lambda p=prec: upscale(gens[2], lr, scale=2, precision=p, max_tile_pixels=4 * MAX_TILE_PIXELS)))
        frames.append((f'x4 {w}x{h} -> {4 * w}x{4 * h} {prec}', lambda p=prec: upscale(gens[4], lr, scale=4, precision=p)))
    with torch.no_grad():
        ref = upscale(gens[2], lr, scale=2, precision='fp32', max_tile_pixels=4 * MAX_TILE_PIXELS)
        low = upscale(gens[2], lr, scale=2, precision='bf16', max_tile_pixels=4 * MAX_TILE_PIXELS)
        assert ref.shape == (1, 3, 2 * h, 2 * w)
        dist = ((low - ref).abs().max() / ref.abs().max()).item()
        del ref, low
        tf = alternate(frames, args.rounds, args.frames)
    tail = ['', f'x2 frame: max |bf16 - fp32| = {dist:.3e} of the largest value', '',
            f'(b) whole frame, {args.blocks} blocks, {args.frames} frames per round (x2: tiles of {4 * MAX_TILE_PIXELS} image pixels, halo '
            f'{gens[2].halo}; x4: tiles of {MAX_TILE_PIXELS}, halo {gens[4].halo}): milliseconds per frame']
    tail += table(tf, [n for n, _ in frames], lambda n, med: f'{1e3 / med:6.2f} frames/s')
    for prec in ('fp32', 'bf16'):
        a = statistics.median(tf[f'x2 {w}x{h} -> {2 * w}x{2 * h} {prec}'])
        b = statistics.median(tf[f'x4 {w}x{h} -> {4 * w}x{4 * h} {prec}'])
        tail.append(f'{prec}: the x4 frame takes {b / a:.2f} x the x2 frame\'s time ({b:.1f} vs {a:.1f} ms)')
    print('\n'.join(tail), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines + tail) + '\n')


if __name__ == '__main__':
    main()
