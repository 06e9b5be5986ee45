"""``--degradation blind2`` against ``blind`` and ``bicubic`` on the device data path: the time per batch of the three
``DeviceLoader`` modes at batch 16 and crops of 96 (SRGAN) and 128 (ESRGAN), and ``srx_filter2d`` against ``srx_blur_aniso`` with
every sample at 21 x 21 on the same tensors.

The protocol of tools/bench_degrade.py: one process; every shape is warmed up; a loader figure is the time between two device
events around a run of batches (the host side of a batch -- the parameter draw with its kernel tables, the small uploads, the
launches -- lies between them too, so this is what a training loop waits for), taken in ROUNDS rounds that alternate the modes
so that a drift of the machine lands on all of them; a kernel figure is the time per call of CALLS calls between two events,
the two kernels alternating likewise.  The table gives the median, minimum and maximum of the rounds.

    python tools/bench_degrade2.py [--rounds 4] [--batches 50] [--calls 200] [--out profiles/degrade2_times.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench_degrade import STEP_MS, batches_of, row, timed_batches, timed_calls  # noqa: E402

MODES = ('bicubic', 'blind', 'blind2')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--batches', type=int, default=50, help='batches per round and mode')
    ap.add_argument('--calls', type=int, default=200, help='calls per round of a kernel alone')
    ap.add_argument('--out', type=str, default=os.path.join('profiles', 'degrade2_times.txt'))
    args = ap.parse_args()
    if args.rounds < 3 or args.rounds * args.batches < 200 or args.calls < 200:
        raise SystemExit('bench_degrade2: at least 3 rounds, 200 batches per loader figure and 200 calls per kernel figure')
    if not torch.cuda.is_available():
        raise SystemExit('bench_degrade2: needs the MI355X (no CPU timing says anything about it)')
    dev = torch.device('cuda:0')
    import numpy as np
    from torchsr_amd import _lib
    from torchsr_amd.dataset import initialize_device_datasets
    from torchsr_amd.degradation import kernel_slot, kernel_weights
    call = _lib.call
    batch = 16
    lines = [f'batch {batch}; {args.rounds} alternating rounds of {args.batches} batches per loader mode, {args.rounds} alternating '
             f'rounds of {args.calls} calls per kernel, after a warm-up; microseconds (events on the device)', '']
    verdicts = []
    for crop in (96, 128):
        model, step_ms = STEP_MS[crop]
        lines += [f'crop {crop} -> {crop // 4} ({model}, {step_ms} ms per step)', f'{"":<58s} {"median":>9s} {"min":>9s} {"max":>9s}']
        streams = {}
        for mode in MODES:
            loader = initialize_device_datasets('synthetic:256', dev, batch_size=batch, crop_size=crop, seed=3, degradation=mode)[0]
            streams[mode] = batches_of(loader)
            for _ in range(20):
                next(streams[mode])
        torch.cuda.synchronize()
        times = {mode: [] for mode in MODES}
        for _ in range(args.rounds):
            for mode in MODES:
                times[mode].append(timed_batches(streams[mode], args.batches))
        for mode in MODES:
            lines.append(row(f'DeviceLoader batch, --degradation {mode}', times[mode]))
        med = {mode: statistics.median(times[mode]) for mode in MODES}
        for base in ('blind', 'bicubic'):
            extra = med['blind2'] - med[base]
            lines.append(f'  blind2 - {base} (medians): {1e3 * extra:.1f} us = {extra / step_ms:.1%} of the {model} step')
        verdicts.append(f'crop {crop}: a blind2 batch takes {1e3 * med["blind2"]:.0f} us, {1e3 * (med["blind2"] - med["bicubic"]):.0f} us more '
                        f'than a bicubic one: {(med["blind2"] - med["bicubic"]) / step_ms:.1%} of the {model} step')

        # the two blurs with every sample at 21 x 21, on the same tensors: a Gaussian table against the Gaussian computed in place
        parm = torch.tensor([[2.9, 1.1, 2.4, 0.0]] * batch, dtype=torch.float32, device=dev)
        slot = kernel_slot(kernel_weights('gauss', 21, 2.9, 1.1, 2.4))
        tables = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(slot, (batch, 21, 21)))).to(dev)
        k21 = torch.full((batch,), 21, dtype=torch.int32, device=dev)
        hr, hr2 = torch.rand(batch, 3, crop, crop, device=dev), torch.empty(batch, 3, crop, crop, device=dev)
        s = torch.cuda.current_stream().cuda_stream
        kernels = {
            'srx_blur_aniso, every sample 21 x 21':
                lambda: call('srx_blur_aniso', hr.data_ptr(), hr2.data_ptr(), parm.data_ptr(), k21.data_ptr(), batch, 3, crop, crop, s),
            'srx_filter2d, every sample 21 x 21':
                lambda: call('srx_filter2d', hr.data_ptr(), hr2.data_ptr(), tables.data_ptr(), k21.data_ptr(), batch, 3, crop, crop, 0, s),
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
            lines.append(row('  ' + name, ktimes[name]))
        blur, filt = ktimes['srx_blur_aniso, every sample 21 x 21'], ktimes['srx_filter2d, every sample 21 x 21']
        over, spread = statistics.median(filt) - statistics.median(blur), max(blur) - min(blur)
        verdicts.append(f'crop {crop}: srx_filter2d - srx_blur_aniso at 21 x 21 (medians) = {1e3 * over:+.1f} us; srx_blur_aniso\'s own min-max '
                        f'spread is {1e3 * spread:.1f} us: {"SLOWER by more than the spread" if over > spread else "not slower beyond the spread"}')
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
