"""``--jpeg-420-prob`` on the device data path: ``srx_jpeg_sim2`` (a chroma launch and a luma launch) with no, half and all of
its samples flagged 4:2:0 against ``srx_jpeg_sim`` (one launch) on the same tensors, [16, 3, 24, 24] and [16, 3, 32, 32] (the
low-resolution batches of crops 96 and 128, where ``blind`` runs its JPEG); and the time per train batch of a ``blind`` and of a
``blind2`` ``DeviceLoader`` with ``jpeg420_prob`` 1 against the same loader with 0.

The protocol of tools/bench_degrade.py: one process; every shape is warmed up; a kernel figure is the time per call of CALLS calls
between two device events, a loader figure the time per batch of a run of batches between two events (the host side of a batch
lies between them too, so this is what a training loop waits for); both are taken in ROUNDS rounds that alternate the
candidates so that a drift of the machine lands on all of them.  The table gives the median, minimum and maximum of the rounds.

    python tools/bench_jpeg420.py [--rounds 4] [--batches 50] [--calls 200] [--out profiles/jpeg420_times.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench_degrade import STEP_MS, batches_of, timed_batches, timed_calls  # noqa: E402


def row(name, ts, unit=1e3):
    """bench_degrade's row with room for this table's names."""
    ts = [unit * t for t in ts]
    return f'{name:<66s} {statistics.median(ts):9.1f} {min(ts):9.1f} {max(ts):9.1f}'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--batches', type=int, default=50, help='batches per round and loader')
    ap.add_argument('--calls', type=int, default=200, help='calls per round of a kernel alone')
    ap.add_argument('--out', type=str, default=os.path.join('profiles', 'jpeg420_times.txt'))
    args = ap.parse_args()
    if args.rounds < 3 or args.rounds * args.batches < 200 or args.calls < 200:
        raise SystemExit('bench_jpeg420: at least 3 rounds, 200 batches per loader figure and 200 calls per kernel figure')
    if not torch.cuda.is_available():
        raise SystemExit('bench_jpeg420: needs the MI355X (no CPU timing says anything about it)')
    dev = torch.device('cuda:0')
    from torchsr_amd import _lib
    from torchsr_amd.dataset import initialize_device_datasets
    call = _lib.call
    batch, crop = 16, 96
    model, step_ms = STEP_MS[crop]
    lines = [f'batch {batch}; {args.rounds} alternating rounds of {args.calls} calls per kernel, {args.rounds} alternating rounds of '
             f'{args.batches} batches per loader, after a warm-up; microseconds (events on the device)', '',
             f'{"":<66s} {"median":>9s} {"min":>9s} {"max":>9s}']
    verdicts = []
    s = torch.cuda.current_stream().cuda_stream
    quality = torch.tensor([30 + (i * 13) % 66 for i in range(batch)], dtype=torch.int32, device=dev)   # 30 .. 95, as the loader draws
    flag_sets = {'no flag set': [0] * batch, 'half the flags set': [i & 1 for i in range(batch)], 'every flag set': [1] * batch}
    flags = {k: torch.tensor(v, dtype=torch.int32, device=dev) for k, v in flag_sets.items()}
    for side in (24, 32):
        x = (torch.rand(batch, 3, side, side, device=dev) * 255).round() / 255
        out = torch.empty_like(x)
        nbytes = call('srx_jpeg_sim2_workspace', batch, side, side)
        ws = torch.empty(nbytes // 4, device=dev)
        old = f'srx_jpeg_sim [16, 3, {side}, {side}]'
        kernels = {old: lambda: call('srx_jpeg_sim', x.data_ptr(), out.data_ptr(), quality.data_ptr(), batch, side, side, 1, s)}
        for k, f in flags.items():
            kernels[f'srx_jpeg_sim2 [16, 3, {side}, {side}], {k} (2 launches)'] = (
                lambda f=f: call('srx_jpeg_sim2', x.data_ptr(), out.data_ptr(), quality.data_ptr(), f.data_ptr(), batch, side, side, 1,
                                 ws.data_ptr(), nbytes, None, s))
        for fn in kernels.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        ktimes = {name: [] for name in kernels}
        for _ in range(args.rounds):
            for name, fn in kernels.items():
                ktimes[name].append(timed_calls(fn, args.calls))
        for name in kernels:
            lines.append(row(name, ktimes[name]))
        med = {name: statistics.median(t) for name, t in ktimes.items()}
        new = [med[n] for n in kernels if n != old]
        lines.append('  srx_jpeg_sim2 / srx_jpeg_sim (medians): ' + ', '.join(f'{t / med[old]:.2f}' for t in new))
        verdicts.append(f'{side} x {side}: srx_jpeg_sim2 takes {1e3 * new[0]:.1f} / {1e3 * new[1]:.1f} / {1e3 * new[2]:.1f} us with no / half / '
                        f'all of its flags set against {1e3 * med[old]:.1f} us for srx_jpeg_sim')
        lines.append('')

    # train batches with and without the flag
    for mode in ('blind', 'blind2'):
        streams = {}
        for prob in (0.0, 1.0):
            loader = initialize_device_datasets('synthetic:256', dev, batch_size=batch, crop_size=crop, seed=3, degradation=mode,
                                                jpeg420_prob=prob)[0]
            streams[prob] = batches_of(loader)
            for _ in range(20):
                next(streams[prob])
        torch.cuda.synchronize()
        times = {prob: [] for prob in streams}
        for _ in range(args.rounds):
            for prob in streams:
                times[prob].append(timed_batches(streams[prob], args.batches))
        for prob in streams:
            lines.append(row(f'DeviceLoader batch, {mode}, crop {crop}, --jpeg-420-prob {prob:g}', times[prob]))
        extra = statistics.median(times[1.0]) - statistics.median(times[0.0])
        spread = max(times[0.0]) - min(times[0.0])
        lines.append(f'  --jpeg-420-prob 1 on {mode} (medians): {1e3 * extra:+.1f} us = {extra / step_ms:+.1%} of the {model} step; the '
                     f'rounds without the flag span {1e3 * spread:.1f} us')
        verdicts.append(f'--jpeg-420-prob 1 changes a {mode} batch by {1e3 * extra:+.0f} us ({extra / step_ms:+.1%} of the {model} step), '
                        f'{"beyond" if abs(extra) > spread else "within"} the {1e3 * spread:.0f} us the rounds without it span')
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
