"""``--color-fix`` on the 1080p frame (BASELINE config 5, SRGAN bf16): every kernel of ``csrc/colorfix.hip`` on the 8K result,
the two operators ``F.color_fix_wavelet`` / ``F.color_fix_adain``, and the frame ``upscale(srgan, 1080p, 'bf16', color_fix=m)``
against the plain frame.  The yardstick is ``copy_`` of one 8K fp32 frame, timed in the same process and the same rounds: a
pass is compared with the copy of the bytes it must move.

One process; every shape is warmed up; a figure is the time per call of a batch of calls between two device events, taken
in ROUNDS rounds that run the configurations of a table one after another, so that a drift of the machine lands on all of
them (rounds x batch >= 100 calls per figure); the tables give the median, minimum and maximum of the rounds.  Bytes are the
least traffic: one read of every operand and one write of the result.

    python tools/bench_color_fix.py [--rounds 5] [--batch 20] [--frames 20] [--out profiles/color_fix_times.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batch', type=int, default=20, help='kernel / operator calls per round and configuration')
    ap.add_argument('--frames', type=int, default=20, help='frames per round and configuration')
    ap.add_argument('--out', type=str, default=os.path.join('profiles', 'color_fix_times.txt'))
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    args = ap.parse_args()
    if args.rounds < 3 or args.rounds * args.batch < 100 or args.rounds * args.frames < 100:
        raise SystemExit('bench_color_fix: at least 3 rounds and 100 timed calls per figure')
    if not torch.cuda.is_available():
        raise SystemExit('bench_color_fix: needs the MI355X (no CPU timing says anything about it)')
    dev = torch.device('cuda:0')
    from torchsr_amd import _lib
    from torchsr_amd import functional as F
    from torchsr_amd.srgan.generator import Generator
    from torchsr_amd.test import upscale
    torch.manual_seed(0)
    h, w = args.height, args.width
    H, W = 4 * h, 4 * w
    frame = 3 * H * W * 4  # bytes of one fp32 frame of the result
    small = 3 * h * w * 4
    lines = [f'{args.rounds} rounds after two warm-up calls each; time per call on the device (events around a batch)', '']

    with torch.no_grad():
        sr = torch.rand(1, 3, H, W, device=dev)
        lr = torch.rand(1, 3, h, w, device=dev)
        u = F.resize_bicubic_aa(lr, (H, W))
        a, b = torch.empty_like(sr), torch.empty_like(sr)
        s = torch.cuda.current_stream().cuda_stream
        m_sr, m_lr = F.plane_moments(sr), F.plane_moments(lr)
        blocks = _lib.lib().srx_plane_moments_blocks(H, W)
        part = torch.empty(3 * blocks * 2, dtype=torch.float64, device=dev)
        stats = torch.empty(3, 2, dtype=torch.float64, device=dev)

        def level(src, sub, add, dst, r):
            ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
            _lib.call('srx_color_fix_wavelet_level', ptr(src), ptr(sub), ptr(add), ptr(dst), 3, H, W, r, s)

        # name, function, bytes it must move
        configs = [('copy_ of one frame (the yardstick)', lambda: b.copy_(a), 2 * frame)]
        a.copy_(u).sub_(sr)
        for r in (1, 2, 4, 8, 16):
            configs.append((f'level, radius {r}', lambda r=r: level(a, None, None, b, r), 2 * frame))
        configs += [
            ('level, radius 3 (the scalar form)', lambda: level(a, None, None, b, 3), 2 * frame),
            ('level, radius 1, U - sr folded in', lambda: level(u, sr, None, b, 1), 3 * frame),
            ('  unfolded: torch.sub(U, sr) + level, radius 1', lambda: (torch.sub(u, sr, out=a), level(a, None, None, b, 1)), 5 * frame),
            ('level, radius 16, sr + D folded in', lambda: level(a, None, sr, b, 16), 3 * frame),
            ('  unfolded: level, radius 16 + torch.add(sr, D)', lambda: (level(a, None, None, b, 16), torch.add(sr, b, out=b)), 5 * frame),
            ('resize_bicubic_aa of the input to the result\'s size', lambda: F.resize_bicubic_aa(lr, (H, W), out=b), small + frame),
            ('plane moments of the result (2 launches)',
             lambda: _lib.call('srx_plane_moments', sr.data_ptr(), 3, H, W, part.data_ptr(), part.numel(), stats.data_ptr(), s), frame),
            ('plane moments of the input (2 launches)', lambda: F.plane_moments(lr), small),
            ('AdaIN map', lambda: _lib.call('srx_color_fix_adain_apply', sr.data_ptr(), b.data_ptr(), 3, H, W, m_sr.data_ptr(),
                                            m_lr.data_ptr(), s), 2 * frame),
            ('F.color_fix_wavelet (resize + 5 levels)', lambda: F.color_fix_wavelet(sr, lr, out=b), small + frame + 2 * 3 * frame + 3 * 2 * frame),
            ('F.color_fix_adain (moments x 2 + map)', lambda: F.color_fix_adain(sr, lr, out=b), 3 * frame + small),
        ]
        t = alternate([(n, f) for n, f, _ in configs], args.rounds, args.batch)
        copy_ms = statistics.median(t[configs[0][0]])
        lines += [f'[1, 3, {H}, {W}] fp32 against the [1, 3, {h}, {w}] input, {args.batch} calls per round: microseconds per call; '
                  f'MB it must move; GB/s; time over the copy of the same bytes',
                  f'{"":<56s} {"median":>9s} {"min":>9s} {"max":>9s} {"MB":>8s} {"GB/s":>8s} {"x copy":>7s}']
        for name, _, nbytes in configs:
            us = [1e3 * v for v in t[name]]
            med = statistics.median(us)
            lines.append(f'{name:<56s} {med:9.1f} {min(us):9.1f} {max(us):9.1f} {nbytes / 1e6:8.0f} {nbytes / (med * 1e-6) / 1e9:8.0f} '
                         f'{med * 1e-3 / (copy_ms * nbytes / (2 * frame)):7.2f}')
        del a, b, u, part

        # ---- the frame
        gen = Generator().to(dev).eval()
        configs = [('bf16 plain', lambda: upscale(gen, lr, precision='bf16')),
                   ('bf16 color_fix=wavelet', lambda: upscale(gen, lr, precision='bf16', color_fix='wavelet')),
                   ('bf16 color_fix=adain', lambda: upscale(gen, lr, precision='bf16', color_fix='adain'))]
        t = alternate(configs, args.rounds, args.frames)
    lines += ['', f'SRGAN generator, {w} x {h} frame -> {W} x {H}, {args.frames} frames per round and configuration: milliseconds per frame',
              f'{"":<56s} {"median":>9s} {"min":>9s} {"max":>9s}']
    plain = statistics.median(t['bf16 plain'])
    for name, _ in configs:
        v = t[name]
        more = '' if name == 'bf16 plain' else f'  + {statistics.median(v) - plain:.3f} ms'
        lines.append(f'{name:<56s} {statistics.median(v):9.3f} {min(v):9.3f} {max(v):9.3f}{more}  (spread {max(v) - min(v):.3f})')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
