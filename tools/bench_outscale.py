"""``--outscale`` on the 1080p frame (BASELINE config 5): the resampler ``F.resize_bicubic_aa`` (``srx_resample_planes``) on the
8K result -> 4K (``--outscale 2``) and -> 5760 x 3240 (``--outscale 3``) against ATen's
``F.interpolate(mode='bicubic', antialias=True)`` on the same GPU tensor -- the library call a user would otherwise write --
and the frame ``upscale(srgan, 1080p, precision, outscale=2)`` against the plain frame.

One process; every shape is warmed up; a figure is the time per call of a batch of calls between two device events, taken
in ROUNDS rounds that alternate the two sides of a comparison, so that a drift of the machine lands on both (rounds x batch
>= 100 calls per figure); the table gives the median, minimum and maximum of the rounds.  Bytes per second are over the
least traffic: one read of the input and one write of the output.

    python tools/bench_outscale.py [--rounds 5] [--batch 25] [--frames 20] [--out profiles/outscale_times.txt]
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


def spread(ts):
    return max(ts) - min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batch', type=int, default=25, help='resampler calls per round and side')
    ap.add_argument('--frames', type=int, default=20, help='frames per round and configuration')
    ap.add_argument('--out', type=str, default=os.path.join('profiles', 'outscale_times.txt'))
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    args = ap.parse_args()
    if args.rounds < 3 or args.rounds * args.batch < 100 or args.rounds * args.frames < 100:
        raise SystemExit('bench_outscale: at least 3 rounds and 100 timed calls per figure')
    if not torch.cuda.is_available():
        raise SystemExit('bench_outscale: needs the MI355X (no CPU timing says anything about it)')
    dev = torch.device('cuda:0')
    from torchsr_amd import functional as F
    from torchsr_amd.srgan.generator import Generator
    from torchsr_amd.test import upscale
    torch.manual_seed(0)
    h, w = args.height, args.width
    lines = [f'{args.rounds} alternating rounds after two warm-up calls each; time per call on the device (events around a batch)', '']
    verdicts = []

    # ---- the resampler against ATen on the x4 result of the frame
    with torch.no_grad():
        big = torch.rand(1, 3, 4 * h, 4 * w, device=dev) - 0.25
        lines += [f'resize of [1, 3, {4 * h}, {4 * w}] fp32, {args.batch} calls per round and side: microseconds per call',
                  f'{"":<52s} {"median":>9s} {"min":>9s} {"max":>9s}']
        for s in (2, 3):
            size = (int(h * s + 0.5), int(w * s + 0.5))
            out = torch.empty(1, 3, *size, device=dev)
            ours = lambda: F.resize_bicubic_aa(big, size, out=out)  # noqa: E731
            aten = lambda: torch.nn.functional.interpolate(big, size=size, mode='bicubic', antialias=True,  # noqa: E731
                                                           align_corners=False)
            diff = (ours() - aten()).abs().max().item()
            t = alternate([('ours', ours), ('aten', aten)], args.rounds, args.batch)
            ko, ka = [1e3 * v for v in t['ours']], [1e3 * v for v in t['aten']]
            need = 4 * 3 * (16 * h * w + size[0] * size[1])
            mo, ma = statistics.median(ko), statistics.median(ka)
            lines += [f'{"-> " + str(size[1]) + " x " + str(size[0]) + " (--outscale " + str(s) + ")":<52s}',
                      f'{"  srx_resample_planes (2 launches)":<52s} {mo:9.1f} {min(ko):9.1f} {max(ko):9.1f}  '
                      f'{need / 1e6:.0f} MB it must move: {need / (mo * 1e-6) / 1e12:.2f} TB/s',
                      f'{"  ATen interpolate(bicubic, antialias=True)":<52s} {ma:9.1f} {min(ka):9.1f} {max(ka):9.1f}  '
                      f'{ma / mo:5.2f} x the kernel',
                      f'  spread (max - min): kernel {spread(ko):.1f} us, ATen {spread(ka):.1f} us; ATen - kernel (medians) '
                      f'{ma - mo:.1f} us; max |kernel - ATen| = {diff:.3e}']
            ok = mo <= ma + max(spread(ko), spread(ka))
            verdicts.append(f'--outscale {s}: the kernel is {"NOT SLOWER" if ok else "SLOWER"} than ATen\'s call beyond the '
                            f'round-to-round spread')
            del out
        del big

    # ---- the frame
    gen = Generator().to(dev).eval()
    lr = torch.rand(1, 3, h, w, device=dev)
    configs = []
    for prec in ('fp32', 'bf16'):
        configs.append((f'{prec} plain', lambda p=prec: upscale(gen, lr, precision=p)))
        configs.append((f'{prec} outscale=2', lambda p=prec: upscale(gen, lr, precision=p, outscale=2)))
    t = alternate(configs, args.rounds, args.frames)
    lines += ['', f'SRGAN generator, {w} x {h} frame, {args.frames} frames per round and configuration: milliseconds per frame',
              f'{"":<52s} {"median":>9s} {"min":>9s} {"max":>9s}']
    for prec in ('fp32', 'bf16'):
        a, b = t[f'{prec} plain'], t[f'{prec} outscale=2']
        lines += [f'{prec + " -> " + str(4 * w) + " x " + str(4 * h):<52s} {statistics.median(a):9.3f} {min(a):9.3f} {max(a):9.3f}',
                  f'{prec + " outscale=2 -> " + str(2 * w) + " x " + str(2 * h):<52s} {statistics.median(b):9.3f} {min(b):9.3f} '
                  f'{max(b):9.3f}  + {statistics.median(b) - statistics.median(a):.3f} ms (spread: plain {spread(a):.3f}, '
                  f'outscale {spread(b):.3f})']
    lines += [''] + verdicts
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
