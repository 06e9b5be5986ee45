"""What the gradient guard (--clip-grad-norm / --skip-nonfinite-steps) costs per step (developer tool, needs the MI355X):
the SRGAN batch-16 fp32 GAN step and the ESRGAN batch-16 bf16 GAN step as replayed hipGraphs, guard off and on, timed in
alternating rounds in ONE process, plus srx_grad_guard alone on the SRGAN discriminator's flat gradient.

    python tools/grad_guard_ab.py [rounds] [steps per round]

The guard is idle here (clip norm 1e30 on finite gradients): it launches and reads exactly what an active one does."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from torchsr_amd._lib import call  # noqa: E402
from torchsr_amd.esrgan.trainer import ESRGANTrainer  # noqa: E402
from torchsr_amd.srgan.trainer import SRGANTrainer  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
dev = torch.device('cuda:0')
GUARD = {'clip_grad_norm': 1e30, 'skip_nonfinite_steps': True}


def build(cls, amp, crop, seed, **extra):
    torch.manual_seed(0)
    t = cls(dev, bench._targs(16, amp, **extra), [], [], 16, 16)
    t.generator.train()
    t.discriminator.train()
    lr, hr = bench._crops(dev, 16, crop, seed)
    for _ in range(8):  # two eager passes, the capture, five replays
        t.gan_step(lr, hr)
    torch.cuda.synchronize()
    assert 'gan.all' in t._graphs
    return lambda: t.gan_step(lr, hr), t


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


for name, cls, amp, crop, seed in (('SRGAN GAN step, batch 16, 96x96, fp32', SRGANTrainer, False, 96, 77),
                                   ('ESRGAN GAN step, batch 16, 128x128, bf16 products', ESRGANTrainer, True, 128, 78)):
    off, _ = build(cls, amp, crop, seed)
    on, t_on = build(cls, amp, crop, seed, **GUARD)
    ms = {'off': [], 'on': []}
    for _ in range(rounds):
        ms['off'].append(timed(off, steps))
        ms['on'].append(timed(on, steps))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    print(f'{name}: guard off {med["off"]:.3f} ms/step, on {med["on"]:.3f} ms/step '
          f'({(med["on"] / med["off"] - 1) * 100:+.2f} %); rounds off {[round(x, 3) for x in ms["off"]]} '
          f'on {[round(x, 3) for x in ms["on"]]}')
    stats = {k: getattr(t_on, k).guard_stats() for k in ('disc_optimizer', 'gen_optimizer')}
    print(f'  guard state after the run: {stats}')
    if cls is SRGANTrainer:
        opt = t_on.disc_optimizer
        n, reps = opt.flat.numel, 200
        st = torch.cuda.current_stream().cuda_stream
        args = (opt.flat.grad.data_ptr(), n, 1.0, 1e30, 1, opt.guard_ws.data_ptr(), opt.guard_ws.numel() * 8,
                opt.guard_state.data_ptr(), st)
        for _ in range(10):
            call('srx_grad_guard', *args)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call('srx_grad_guard', *args)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / reps * 1e3
        print(f'  srx_grad_guard alone, SRGAN discriminator gradient ({n} floats, {n * 4 / 1e6:.1f} MB): {us:.1f} us per call '
              f'(sum-of-squares + finalise launch, {reps} calls back to back between two events; {n * 4 / us / 1e6:.2f} TB/s -- '
              'the buffer fits the 256 MB Infinity Cache, so this is not an HBM rate)')
    del off, on, t_on
    torch.cuda.empty_cache()
