"""The compact generator (SRVGGNetCompact) on the 1080p frame (BASELINE config 5): ``upscale(compact, 1080p, precision)`` -> x4
for every precision and for ``num_conv`` 16 (realesr-animevideov3) and 32 (realesr-general-x4v3), next to the SRGAN bf16
frame in the same process.

One process; every configuration is warmed up; a figure is the time per frame of a batch of frames between two device
events, taken in ROUNDS rounds that walk through all configurations in turn, so that a drift of the machine lands on every
one of them (rounds x frames >= 100 frames per figure); the table gives the median, minimum and maximum of the rounds.  The
weights are seeded random values at He scale (the arithmetic does not depend on them); the frame is uniform noise.  FLOP/s
are the convs' multiply-adds over the frame time: an end-to-end rate, not a kernel's.

    python tools/bench_compact.py [--rounds 5] [--frames 20] [--out profiles/compact_times.txt]
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


def compact_flops(num_conv, h, w, scale=4, feat=64):
    """Multiply-adds x 2 of one frame: 3 -> feat, num_conv x feat -> feat, feat -> 3 scale^2, all 3x3 at low resolution."""
    return 2.0 * 9 * h * w * (3 * feat + num_conv * feat * feat + feat * 3 * scale * scale)


def seeded(gen, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in gen.named_parameters():
            if p.dim() == 4:
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / (1.1 * p.shape[1] * 9)) ** 0.5)
            elif k.endswith('.bias'):
                p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 0.2)
            else:
                p.copy_(torch.rand(p.shape, generator=g) * 0.5)
    return gen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--frames', type=int, default=20, help='frames per round and configuration')
    ap.add_argument('--out', type=str, default=os.path.join('profiles', 'compact_times.txt'))
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    args = ap.parse_args()
    if args.rounds < 3 or args.rounds * args.frames < 100:
        raise SystemExit('bench_compact: at least 3 rounds and 100 timed frames per figure')
    if not torch.cuda.is_available():
        raise SystemExit('bench_compact: needs the MI355X (no CPU timing says anything about it)')
    dev = torch.device('cuda:0')
    from torchsr_amd.compact.generator import Generator as Compact
    from torchsr_amd.srgan.generator import Generator as SRGAN
    from torchsr_amd.test import upscale
    h, w = args.height, args.width
    lr = torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(0)).to(dev)
    gens = {n: seeded(Compact(num_conv=n), n).to(dev).eval() for n in (16, 32)}
    srgan = SRGAN().to(dev).eval()
    configs = [('srgan bf16', lambda: upscale(srgan, lr, precision='bf16'))]
    for n in (16, 32):
        for prec in ('fp32', 'bf16', 'fp16'):
            configs.append((f'compact-{n} {prec}', lambda g=gens[n], p=prec: upscale(g, lr, precision=p)))
    with torch.no_grad():
        for n in (16, 32):  # the 16-bit results against the fp32 one, at the size that is timed
            ref = upscale(gens[n], lr, precision='fp32')
            for prec in ('bf16', 'fp16'):
                out = upscale(gens[n], lr, precision=prec)
                dist = ((out - ref).abs().max() / ref.abs().max()).item()
                print(f'compact-{n} {prec}: max |x - fp32| = {dist:.3e} of the range', flush=True)
            del ref, out
    t = alternate(configs, args.rounds, args.frames)
    lines = [f'{args.rounds} rounds through all configurations after two warm-up frames each; {args.frames} frames per round and '
             f'configuration; time per frame on the device (events around a batch)', '',
             f'{w} x {h} frame -> {4 * w} x {4 * h}: milliseconds per frame',
             f'{"":<28s} {"median":>9s} {"min":>9s} {"max":>9s}  {"spread":>7s}  {"frames/s":>8s}  {"conv TFLOP/s (end to end)":>26s}']
    base = statistics.median(t['srgan bf16'])
    for name, _ in configs:
        ts = t[name]
        med = statistics.median(ts)
        rate = ''
        if name.startswith('compact-'):
            rate = f'{compact_flops(int(name.split()[0].split("-")[1]), h, w) / (med * 1e-3) / 1e12:26.1f}'
        lines.append(f'{name:<28s} {med:9.3f} {min(ts):9.3f} {max(ts):9.3f}  {max(ts) - min(ts):7.3f}  {1e3 / med:8.1f}  {rate}')
    lines.append('')
    for n in (16, 32):
        for prec in ('bf16', 'fp16'):
            med = statistics.median(t[f'compact-{n} {prec}'])
            lines.append(f'compact-{n} {prec}: {base / med:.2f} x the SRGAN bf16 frame rate ({med:.3f} vs {base:.3f} ms)')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
