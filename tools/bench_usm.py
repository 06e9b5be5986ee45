"""``--gt-usm`` on the device data path: ``functional.usm_sharpen`` (two launches, each a separable 51-tap pass pair) against
``srx_filter2d`` with every sample at 21 x 21 -- the yardstick: a direct 2-D sum of 441 fmas per pixel against about 180 per
launch here -- on the same tensors, [16, 3, 96, 96] (SRGAN's crop) and [16, 3, 128, 128] (ESRGAN's); and the time per train
batch of the ``DeviceLoader`` with and without ``gt_usm``, for ``bicubic`` and for ``blind2``.

The protocol of tools/bench_degrade2.py: one process; every shape is warmed up; a kernel figure is the time per call of CALLS
calls between two device events, a loader figure the time per batch of a run of batches between two events (the host side of a
batch lies between them too, so this is what a training loop waits for); both are taken in ROUNDS rounds that alternate the
candidates so that a drift of the machine lands on all of them.  The table gives the median, minimum and maximum of the rounds.

    python tools/bench_usm.py [--rounds 4] [--batches 50] [--calls 200] [--out profiles/usm_times.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench_degrade import STEP_MS, batches_of, row, timed_batches, timed_calls  # noqa: E402

LOADERS = (('bicubic', False), ('bicubic', True), ('blind2', False), ('blind2', True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--batches', type=int, default=50, help='batches per round and loader')
    ap.add_argument('--calls', type=int, default=200, help='calls per round of a kernel alone')
    ap.add_argument('--out', type=str, default=os.path.join('profiles', 'usm_times.txt'))
    args = ap.parse_args()
    if args.rounds < 3 or args.rounds * args.batches < 200 or args.calls < 200:
        raise SystemExit('bench_usm: at least 3 rounds, 200 batches per loader figure and 200 calls per kernel figure')
    if not torch.cuda.is_available():
        raise SystemExit('bench_usm: needs the MI355X (no CPU timing says anything about it)')
    dev = torch.device('cuda:0')
    import numpy as np
    from torchsr_amd import _lib
    from torchsr_amd import functional as F
    from torchsr_amd.dataset import initialize_device_datasets
    from torchsr_amd.degradation import kernel_slot, kernel_weights
    call = _lib.call
    batch = 16
    lines = [f'batch {batch}; {args.rounds} alternating rounds of {args.calls} calls per kernel, {args.rounds} alternating rounds of '
             f'{args.batches} batches per loader, after a warm-up; microseconds (events on the device)', '']
    verdicts = []
    for crop in (96, 128):
        model, step_ms = STEP_MS[crop]
        lines += [f'crop {crop} ({model}, {step_ms} ms per step)', f'{"":<58s} {"median":>9s} {"min":>9s} {"max":>9s}']
        # the operation and its yardstick on the same tensors
        slot = kernel_slot(kernel_weights('gauss', 21, 2.9, 1.1, 2.4))
        tables = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(slot, (batch, 21, 21)))).to(dev)
        k21 = torch.full((batch,), 21, dtype=torch.int32, device=dev)
        hr, hr2 = torch.rand(batch, 3, crop, crop, device=dev), torch.empty(batch, 3, crop, crop, device=dev)
        s = torch.cuda.current_stream().cuda_stream
        usm_name, filt_name = f'usm_sharpen [16, 3, {crop}, {crop}], 51 taps (2 launches)', 'srx_filter2d, every sample 21 x 21'
        with torch.no_grad():
            kernels = {
                usm_name: lambda: F.usm_sharpen(hr),
                filt_name: lambda: call('srx_filter2d', hr.data_ptr(), hr2.data_ptr(), tables.data_ptr(), k21.data_ptr(), batch, 3, crop,
                                        crop, 0, s),
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
        usm, filt = statistics.median(ktimes[usm_name]), statistics.median(ktimes[filt_name])
        spread = max(ktimes[filt_name]) - min(ktimes[filt_name])
        lines.append(f'  usm_sharpen / 2 (medians): {1e3 * usm / 2:.1f} us per launch against {1e3 * filt:.1f} us')
        verdicts.append(f'crop {crop}: one usm launch (half of usm_sharpen) - srx_filter2d at 21 x 21 (medians) = {1e3 * (usm / 2 - filt):+.1f} us; '
                        f'srx_filter2d\'s own min-max spread is {1e3 * spread:.1f} us: '
                        f'{"SLOWER by more than the spread" if usm / 2 - filt > spread else "not slower beyond the spread"}')

        # a train batch with and without gt_usm
        streams = {}
        for key in LOADERS:
            loader = initialize_device_datasets('synthetic:256', dev, batch_size=batch, crop_size=crop, seed=3, degradation=key[0],
                                                gt_usm=key[1])[0]
            streams[key] = batches_of(loader)
            for _ in range(20):
                next(streams[key])
        torch.cuda.synchronize()
        times = {key: [] for key in LOADERS}
        for _ in range(args.rounds):
            for key in LOADERS:
                times[key].append(timed_batches(streams[key], args.batches))
        for key in LOADERS:
            lines.append(row(f'DeviceLoader batch, --degradation {key[0]}{" --gt-usm" if key[1] else ""}', times[key]))
        for mode in ('bicubic', 'blind2'):
            extra = statistics.median(times[(mode, True)]) - statistics.median(times[(mode, False)])
            lines.append(f'  --gt-usm on {mode} (medians): {1e3 * extra:+.1f} us = {extra / step_ms:+.1%} of the {model} step')
            verdicts.append(f'crop {crop}: --gt-usm changes a {mode} batch by {1e3 * extra:+.0f} us: {extra / step_ms:+.1%} of the {model} step')
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
