"""What --ema-decay costs per step (developer tool, needs the MI355X): the ESRGAN and compact batch-16 bf16 GAN steps as replayed
hipGraphs, the average off and on, timed in alternating rounds in ONE process, plus srx_ema_update alone on both generators'
flat buffers.  Writes profiles/ema_times.txt (and prints it).

    python tools/bench_ema.py [rounds] [steps per round] [--parent-lib PATH]

--parent-lib: a libsrx_hip.so built from the commit before the average existed.  A third trainer per model then captures its
step through that library -- same process, same rounds -- to show that the step with the average off is the step as it was."""
import contextlib
import ctypes as C
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from torchsr_amd import _lib  # noqa: E402
from torchsr_amd.compact.trainer import CompactTrainer  # noqa: E402
from torchsr_amd.esrgan.trainer import ESRGANTrainer  # noqa: E402

argv = sys.argv[1:]
parent_path = None
if '--parent-lib' in argv:
    at = argv.index('--parent-lib')
    parent_path = argv[at + 1]
    del argv[at:at + 2]
rounds = int(argv[0]) if len(argv) > 0 else 5
steps = int(argv[1]) if len(argv) > 1 else 40
dev = torch.device('cuda:0')
DECAY = 0.999
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def load_parent(path):
    """The other library with this tree's signatures (an entry point it lacks simply cannot be called)."""
    _lib.lib()  # this tree's first: torch has initialised HIP by then
    handle = C.CDLL(path)
    for name, (res, args) in _lib._SIGS.items():
        fn = getattr(handle, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return handle


@contextlib.contextmanager
def through(handle):
    """Every library call inside goes to ``handle`` (None: this tree's library)."""
    if handle is None:
        yield
        return
    own = _lib.lib()
    _lib._lib = handle
    try:
        yield
    finally:
        _lib._lib = own


def build(cls, crop, seed, handle=None, **extra):
    with through(handle):
        torch.manual_seed(0)
        t = cls(dev, bench._targs(16, True, **extra), [], [], 16, 16)
        t.generator.train()
        t.discriminator.train()
        lr, hr = bench._crops(dev, 16, crop, seed)
        for _ in range(8):  # two eager passes, the capture, five replays
            t.gan_step(lr, hr)
        torch.cuda.synchronize()
    assert 'gan.all' in t._graphs

    def step():
        with through(handle):
            t.gan_step(lr, hr)
    return step, t


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def kernel_alone(t, reps=200):
    ema = t.gen_ema
    for _ in range(10):
        ema.update()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ema.update()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


parent = load_parent(parent_path) if parent_path else None
say(f'--ema-decay {DECAY}: {rounds} alternating rounds of {steps} replayed steps per configuration, one process; medians')
for name, cls, seed in (('ESRGAN GAN step, batch 16, 128x128, bf16 products', ESRGANTrainer, 78),
                        ('compact GAN step, batch 16, 128x128, bf16 products', CompactTrainer, 79)):
    legs = {'off': build(cls, 128, seed), 'on': build(cls, 128, seed, ema_decay=DECAY)}
    if parent is not None:
        legs['parent'] = build(cls, 128, seed, handle=parent)
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, (fn, _t) in legs.items():
            ms[k].append(timed(fn, steps))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    say(f'{name}: average off {med["off"]:.3f} ms/step, on {med["on"]:.3f} ms/step ({(med["on"] - med["off"]) * 1e3:+.1f} us, '
        f'{(med["on"] / med["off"] - 1) * 100:+.2f} %)')
    say('  rounds ' + '; '.join(f'{k} {[round(x, 3) for x in v]}' for k, v in ms.items()))
    if parent is not None:
        say(f'  the parent commit\'s library, same process: {med["parent"]:.3f} ms/step (off is {(med["off"] / med["parent"] - 1) * 100:+.2f} % of it)')
    t_on = legs['on'][1]
    n = t_on.gen_flat.numel
    us = kernel_alone(t_on)
    say(f'  srx_ema_update alone, {n} floats ({3 * n * 4 / 1e6:.1f} MB over its three streams): {us:.1f} us per call, 200 calls back '
        f'to back between two events ({3 * n * 4 / us / 1e6:.2f} TB/s; both buffers fit the 256 MB Infinity Cache when nothing '
        'else runs, so this is not an HBM rate -- inside the step the buffers come from HBM)')
    del legs, t_on
    torch.cuda.empty_cache()
os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
with open(os.path.join(ROOT, 'profiles', 'ema_times.txt'), 'w') as f:
    f.write('\n'.join(lines) + '\n')
