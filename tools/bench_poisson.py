"""``--poisson-noise-prob`` on the device data path: ``srx_add_poisson_noise`` (a clear and two launches: the level masks, then
one table-driven draw per value) against ``srx_add_gaussian_noise`` (one launch) on the same tensors, [16, 3, 24, 24] (crop 96
at x1/4, where ``blind`` adds its noise) and [16, 3, 144, 144] (the largest first size ``blind2`` draws at crop 96), with every
sample drawing Poisson; and the time per train batch of a ``blind2`` ``DeviceLoader`` with ``poisson_prob`` 0.5 against the same
loader with 0.

The protocol of tools/bench_usm.py: one process; every shape is warmed up; a kernel figure is the time per call of CALLS calls
between two device events, a loader figure the time per batch of a run of batches between two events (the host side of a batch
lies between them too, so this is what a training loop waits for); both are taken in ROUNDS rounds that alternate the
candidates so that a drift of the machine lands on all of them.  The table gives the median, minimum and maximum of the rounds.

    python tools/bench_poisson.py [--rounds 4] [--batches 50] [--calls 200] [--out profiles/poisson_times.txt]
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
    ap.add_argument('--out', type=str, default=os.path.join('profiles', 'poisson_times.txt'))
    args = ap.parse_args()
    if args.rounds < 3 or args.rounds * args.batches < 200 or args.calls < 200:
        raise SystemExit('bench_poisson: at least 3 rounds, 200 batches per loader figure and 200 calls per kernel figure')
    if not torch.cuda.is_available():
        raise SystemExit('bench_poisson: needs the MI355X (no CPU timing says anything about it)')
    dev = torch.device('cuda:0')
    from torchsr_amd import _lib
    from torchsr_amd import functional as F
    from torchsr_amd.dataset import initialize_device_datasets
    call = _lib.call
    batch, crop = 16, 96
    model, step_ms = STEP_MS[crop]
    lines = [f'batch {batch}; {args.rounds} alternating rounds of {args.calls} calls per kernel, {args.rounds} alternating rounds of '
             f'{args.batches} batches per loader, after a warm-up; microseconds (events on the device)', '',
             f'{"":<66s} {"median":>9s} {"min":>9s} {"max":>9s}']
    verdicts = []
    s = torch.cuda.current_stream().cuda_stream
    tables = F.poisson_tables(dev)
    gray = torch.tensor([i % 5 < 2 for i in range(batch)], dtype=torch.int32, device=dev)   # 40 % grey, as the loader draws
    ones = torch.full((batch,), 1.0, device=dev)
    sigma = torch.full((batch,), 10.0 / 255.0, device=dev)
    levels = torch.empty((batch, 8), dtype=torch.int32, device=dev)
    for side in (24, 144):
        x = (torch.rand(batch, 3, side, side, device=dev) * 255).round() / 255
        out = torch.empty_like(x)
        names = (f'srx_add_poisson_noise [16, 3, {side}, {side}] (clear + 2 launches)', f'srx_add_gaussian_noise [16, 3, {side}, {side}]')
        kernels = {
            names[0]: lambda: call('srx_add_poisson_noise', x.data_ptr(), out.data_ptr(), ones.data_ptr(), gray.data_ptr(),
                                   tables.data_ptr(), levels.data_ptr(), 1, 2, batch, side, side, 0, s),
            names[1]: lambda: call('srx_add_gaussian_noise', x.data_ptr(), out.data_ptr(), sigma.data_ptr(), gray.data_ptr(), 1, 2,
                                   batch, side, side, 1, s),
        }
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
        poi, gau = statistics.median(ktimes[names[0]]), statistics.median(ktimes[names[1]])
        lines.append(f'  Poisson / Gaussian (medians): {poi / gau:.2f}')
        verdicts.append(f'{side} x {side}: srx_add_poisson_noise takes {1e3 * poi:.1f} us against {1e3 * gau:.1f} us for srx_add_gaussian_noise, '
                        f'{poi / gau:.2f} times')

    # a blind2 train batch with and without the flag
    streams = {}
    for prob in (0.0, 0.5):
        loader = initialize_device_datasets('synthetic:256', dev, batch_size=batch, crop_size=crop, seed=3, degradation='blind2',
                                            poisson_prob=prob)[0]
        streams[prob] = batches_of(loader)
        for _ in range(20):
            next(streams[prob])
    torch.cuda.synchronize()
    times = {prob: [] for prob in streams}
    for _ in range(args.rounds):
        for prob in streams:
            times[prob].append(timed_batches(streams[prob], args.batches))
    lines.append('')
    for prob in streams:
        lines.append(row(f'DeviceLoader batch, blind2, crop {crop}, --poisson-noise-prob {prob:g}', times[prob]))
    extra = statistics.median(times[0.5]) - statistics.median(times[0.0])
    spread = max(times[0.0]) - min(times[0.0])
    lines.append(f'  --poisson-noise-prob 0.5 on blind2 (medians): {1e3 * extra:+.1f} us = {extra / step_ms:+.1%} of the {model} step; the '
                 f'rounds without the flag span {1e3 * spread:.1f} us')
    verdicts.append(f'--poisson-noise-prob 0.5 changes a blind2 batch by {1e3 * extra:+.0f} us ({extra / step_ms:+.1%} of the {model} step), '
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
