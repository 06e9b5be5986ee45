"""``--pair-pool`` on the device data path: the time per train batch of a ``blind2`` ``DeviceLoader`` (batch 16, crop 128 -> 32, the
ESRGAN shapes) with a pool of 192 pairs against the same loader without one, and ``srx_pool_exchange`` alone on the tensors of
such a batch, in both modes.

The protocol of tools/bench_poisson.py: one process; everything is warmed up (the pooled loader until its pool is full, so that
its rounds time exchanges, not the fill); a loader figure is the time per batch of a run of batches between two device events
(the host side of a batch lies between them too, so this is what a training loop waits for), a kernel figure the time per call of
CALLS calls between two events; both are taken in ROUNDS rounds that alternate the candidates so that a drift of the machine
lands on all of them.  The table gives the median, minimum and maximum of the rounds.

    python tools/bench_pair_pool.py [--rounds 4] [--batches 50] [--calls 200] [--out profiles/pair_pool_times.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench_degrade import STEP_MS, batches_of, timed_batches, timed_calls  # noqa: E402
from bench_poisson import row  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--batches', type=int, default=50, help='batches per round and loader')
    ap.add_argument('--calls', type=int, default=200, help='calls per round of the kernel alone')
    ap.add_argument('--out', type=str, default=os.path.join('profiles', 'pair_pool_times.txt'))
    args = ap.parse_args()
    if args.rounds < 3 or args.rounds * args.batches < 200 or args.calls < 200:
        raise SystemExit('bench_pair_pool: at least 3 rounds, 200 batches per loader figure and 200 calls per kernel figure')
    if not torch.cuda.is_available():
        raise SystemExit('bench_pair_pool: needs the MI355X (no CPU timing says anything about it)')
    dev = torch.device('cuda:0')
    from torchsr_amd import _lib
    from torchsr_amd.dataset import initialize_device_datasets
    call = _lib.call
    batch, crop, cap = 16, 128, 192
    lc = crop // 4
    model, step_ms = STEP_MS[crop]
    lines = [f'batch {batch}, crop {crop} -> {lc}, pool of {cap} pairs ({cap * 12 * (crop * crop + lc * lc) / 1e6:.1f} MB); {args.rounds} '
             f'alternating rounds of {args.calls} calls per kernel, {args.rounds} alternating rounds of {args.batches} batches per '
             f'loader, after a warm-up; microseconds (events on the device)', '',
             f'{"":<66s} {"median":>9s} {"min":>9s} {"max":>9s}']
    verdicts = []

    # the kernel alone: a fixed set of distinct slots, the pool and the batch of the loader's shapes
    s = torch.cuda.current_stream().cuda_stream
    pool_lr, pool_hr = torch.rand(cap, 3, lc, lc, device=dev), torch.rand(cap, 3, crop, crop, device=dev)
    lr, hr = torch.rand(batch, 3, lc, lc, device=dev), torch.rand(batch, 3, crop, crop, device=dev)
    slots = torch.tensor([(37 * i + 5) % cap for i in range(batch)], dtype=torch.int32).to(dev)
    assert len(set(slots.tolist())) == batch
    moved = batch * 3 * (crop * crop + lc * lc) * 4
    kernels = {
        f'srx_pool_exchange, exchange, [16, 3, {lc}, {lc}] + [16, 3, {crop}, {crop}]':
            lambda: call('srx_pool_exchange', pool_lr.data_ptr(), lr.data_ptr(), 3 * lc * lc, pool_hr.data_ptr(), hr.data_ptr(),
                         3 * crop * crop, slots.data_ptr(), batch, cap, 1, s),
        f'srx_pool_exchange, store, [16, 3, {lc}, {lc}] + [16, 3, {crop}, {crop}]':
            lambda: call('srx_pool_exchange', pool_lr.data_ptr(), lr.data_ptr(), 3 * lc * lc, pool_hr.data_ptr(), hr.data_ptr(),
                         3 * crop * crop, slots.data_ptr(), batch, cap, 0, s),
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
    exch, store = (statistics.median(ktimes[name]) for name in kernels)
    lines.append(f'  an exchange reads and writes {moved / 1e6:.2f} MB each way: {2 * moved / (exch * 1e-3) / 1e12:.2f} TB/s at the median')
    verdicts.append(f'srx_pool_exchange takes {1e3 * exch:.1f} us per exchange and {1e3 * store:.1f} us per store at batch {batch}, crop {crop}')

    # a blind2 train batch with and without the pool
    streams = {}
    for pool in (0, cap):
        loader = initialize_device_datasets('synthetic:256', dev, batch_size=batch, crop_size=crop, seed=3, degradation='blind2',
                                            pair_pool=pool)[0]
        streams[pool] = batches_of(loader)
        for _ in range(max(20, pool // batch + 8)):
            next(streams[pool])
        assert loader.pool_filled == pool
    torch.cuda.synchronize()
    times = {pool: [] for pool in streams}
    for _ in range(args.rounds):
        for pool in streams:
            times[pool].append(timed_batches(streams[pool], args.batches))
    lines.append('')
    for pool in streams:
        lines.append(row(f'DeviceLoader batch, blind2, crop {crop}, --pair-pool {pool}', times[pool]))
    extra = statistics.median(times[cap]) - statistics.median(times[0])
    spread = max(times[0]) - min(times[0])
    lines.append(f'  --pair-pool {cap} on blind2 (medians): {1e3 * extra:+.1f} us = {extra / step_ms:+.1%} of the {model} step; the rounds '
                 f'without the pool span {1e3 * spread:.1f} us')
    verdicts.append(f'--pair-pool {cap} changes a blind2 batch by {1e3 * extra:+.0f} us ({extra / step_ms:+.1%} of the {model} step), '
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
