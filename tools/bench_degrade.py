"""``--degradation blind`` against ``bicubic`` on the device data path: the time per batch of the two ``DeviceLoader`` modes at
batch 16 and crops of 96 (SRGAN) and 128 (ESRGAN), and each of the three new kernels (``srx_blur_aniso``,
``srx_add_gaussian_noise``, ``srx_jpeg_sim``) alone on a batch of the loader's shapes.

One process; every shape is warmed up; a loader figure is the time between two device events around a run of batches (the
host side of a batch -- the parameter draw, the small uploads, the launches -- lies between them too, so this is what a
training loop waits for), taken in ROUNDS rounds that alternate the two modes so that a drift of the machine lands on both
(rounds x batches = 200 batches per figure); a kernel figure is the time per call of 200 calls between two events.  The
table gives the median, minimum and maximum of the rounds.

    python tools/bench_degrade.py [--rounds 4] [--batches 50] [--calls 200] [--out profiles/degrade_times.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

STEP_MS = {96: ('SRGAN', 6.56), 128: ('ESRGAN', 9.7)}  # the batch-16 training steps the loaders feed


def batches_of(loader):
    """Batches without end: one epoch after the other."""
    while True:
        for batch in loader:
            yield batch


def timed_batches(stream, n):
    """Milliseconds per batch of ``n`` batches drawn from ``stream``."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        next(stream)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def timed_calls(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def row(name, ts, unit=1e3):
    ts = [unit * t for t in ts]
    return f'{name:<58s} {statistics.median(ts):9.1f} {min(ts):9.1f} {max(ts):9.1f}'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--batches', type=int, default=50, help='batches per round and mode')
    ap.add_argument('--calls', type=int, default=200, help='calls per round of a kernel alone')
    ap.add_argument('--out', type=str, default=os.path.join('profiles', 'degrade_times.txt'))
    args = ap.parse_args()
    if args.rounds < 3 or args.rounds * args.batches < 200 or args.calls < 200:
        raise SystemExit('bench_degrade: at least 3 rounds, 200 batches per loader figure and 200 calls per kernel figure')
    if not torch.cuda.is_available():
        raise SystemExit('bench_degrade: needs the MI355X (no CPU timing says anything about it)')
    dev = torch.device('cuda:0')
    from torchsr_amd import _lib
    from torchsr_amd.dataset import initialize_device_datasets
    call = _lib.call
    batch = 16
    lines = [f'batch {batch}; {args.rounds} alternating rounds of {args.batches} batches per loader mode, {args.rounds} rounds of '
             f'{args.calls} calls per kernel, after a warm-up; microseconds (events on the device)', '']
    verdicts = []
    for crop in (96, 128):
        model, step_ms = STEP_MS[crop]
        lines += [f'crop {crop} -> {crop // 4} ({model}, {step_ms} ms per step)', f'{"":<58s} {"median":>9s} {"min":>9s} {"max":>9s}']
        streams = {}
        for mode in ('bicubic', 'blind'):
            loader = initialize_device_datasets('synthetic:256', dev, batch_size=batch, crop_size=crop, seed=3, degradation=mode)[0]
            streams[mode] = batches_of(loader)
            for _ in range(20):
                next(streams[mode])
        torch.cuda.synchronize()
        times = {mode: [] for mode in streams}
        for _ in range(args.rounds):
            for mode in streams:
                times[mode].append(timed_batches(streams[mode], args.batches))
        for mode in streams:
            lines.append(row(f'DeviceLoader batch, --degradation {mode}', times[mode]))
        extra = statistics.median(times['blind']) - statistics.median(times['bicubic'])
        share = extra / step_ms
        lines.append(f'  blind - bicubic (medians): {1e3 * extra:.1f} us = {share:.1%} of the {model} step')

        # each kernel alone, on a batch drawn as the loader draws it, and the blur at its largest kernel
        lc = crop // 4
        deg = loader._draw_degradation(batch)
        dv = {k: torch.from_numpy(deg[k]).to(dev) for k in ('parm', 'ksize', 'sigma_n', 'gray', 'quality')}
        k21 = torch.full((batch,), 21, dtype=torch.int32, device=dev)
        hr, hr2 = torch.rand(batch, 3, crop, crop, device=dev), torch.empty(batch, 3, crop, crop, device=dev)
        lr = (torch.rand(batch, 3, lc, lc, device=dev) * 255).round() / 255
        lr2 = torch.empty_like(lr)
        s = torch.cuda.current_stream().cuda_stream
        kernels = [
            (f'srx_blur_aniso, drawn sizes {sorted(deg["ksize"].tolist())}',
             lambda: call('srx_blur_aniso', hr.data_ptr(), hr2.data_ptr(), dv['parm'].data_ptr(), dv['ksize'].data_ptr(), batch, 3, crop, crop, s)),
            ('srx_blur_aniso, every sample 21 x 21',
             lambda: call('srx_blur_aniso', hr.data_ptr(), hr2.data_ptr(), dv['parm'].data_ptr(), k21.data_ptr(), batch, 3, crop, crop, s)),
            ('srx_bicubic_down (the existing kernel)',
             lambda: call('srx_bicubic_down', hr.data_ptr(), lr2.data_ptr(), batch, 3, crop, crop, 4, 0, s)),
            ('srx_add_gaussian_noise',
             lambda: call('srx_add_gaussian_noise', lr.data_ptr(), lr2.data_ptr(), dv['sigma_n'].data_ptr(), dv['gray'].data_ptr(), 1, 2, batch, lc, lc, 1, s)),
            ('srx_jpeg_sim',
             lambda: call('srx_jpeg_sim', lr.data_ptr(), lr2.data_ptr(), dv['quality'].data_ptr(), batch, lc, lc, 1, s)),
        ]
        ktimes = {}
        for name, fn in kernels:
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            ktimes[name] = [timed_calls(fn, args.calls) for _ in range(args.rounds)]
            lines.append(row('  ' + name, ktimes[name]))
        new = {n: statistics.median(t) for n, t in ktimes.items() if 'drawn' in n or 'noise' in n or 'jpeg' in n}
        worst = max(new, key=new.get)
        verdicts.append(f'crop {crop}: the blind batch costs {1e3 * extra:.0f} us more than the bicubic one, {share:.1%} of the {model} step '
                        f'({"OVER" if share > 0.05 else "under"} 5 %); the three new kernels alone take {1e3 * sum(new.values()):.0f} us, '
                        f'most of it {worst.split(",")[0]} ({1e3 * new[worst]:.0f} us)')
        lines.append('')
    lines += verdicts
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
