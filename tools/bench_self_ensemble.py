"""Self-ensemble inference on the 1080p -> 8K frame (BASELINE config 5): frame times with ``self_ensemble`` 0 / 4 / 8 at fp32 and
bf16, the plain frame transposed (1920 x 1080 input) next to the upright one, and the cost of the ensemble's geometry --
the ``srx_dihedral_planes`` launches of one 8-variant frame against the torch restatement (flip / transpose / contiguous /
mul / add) on the same tensors.

One process; every configuration is warmed up, then timed with device events in ROUNDS rounds that alternate the
configurations, so that a drift of the machine lands on all of them; the table gives median, minimum and maximum.

    python tools/bench_self_ensemble.py [--rounds 5] [--out profiles/self_ensemble_times.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def T(x, k):
    if k & 1:
        x = x.transpose(-1, -2)
    if k & 2:
        x = x.flip(-1)
    if k & 4:
        x = x.flip(-2)
    return x


def T_inv(x, k):
    if k & 4:
        x = x.flip(-2)
    if k & 2:
        x = x.flip(-1)
    if k & 1:
        x = x.transpose(-1, -2)
    return x


def timed(fn):
    """Milliseconds of ``fn`` on the device (events around it; the result is dropped before the next call)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(configs, rounds):
    """``configs``: [(name, fn)].  One warm-up call each, then ``rounds`` rounds in order; returns {name: [ms]}."""
    for _, fn in configs:
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in configs}
    for _ in range(rounds):
        for name, fn in configs:
            times[name].append(timed(fn))
    return times


def row(name, ts, extra=''):
    return f'{name:<44s} {statistics.median(ts):10.3f} {min(ts):10.3f} {max(ts):10.3f}  {extra}'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', type=str, default=os.path.join('profiles', 'self_ensemble_times.txt'))
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_self_ensemble: needs the MI355X (no CPU timing says anything about it)')
    dev = torch.device('cuda:0')
    from torchsr_amd import functional as F
    from torchsr_amd.srgan.generator import Generator
    from torchsr_amd.test import upscale
    torch.manual_seed(0)
    gen = Generator().to(dev).eval()
    h, w = args.height, args.width
    lr = torch.rand(1, 3, h, w, device=dev)
    lr_t = lr.transpose(-1, -2).contiguous()
    lines = [f'SRGAN generator, {w} x {h} -> {4 * w} x {4 * h}, {args.rounds} alternating rounds after a warm-up call each; '
             f'milliseconds on the device (events)', '',
             f'{"frame":<44s} {"median":>10s} {"min":>10s} {"max":>10s}']

    # ---- frame times
    configs = []
    for prec in ('fp32', 'bf16'):
        for n in (0, 4, 8):
            configs.append((f'{prec} self_ensemble={n}', lambda p=prec, n=n: upscale(gen, lr, precision=p, self_ensemble=n)))
        configs.append((f'{prec} self_ensemble=0, transposed frame', lambda p=prec: upscale(gen, lr_t, precision=p)))
    times = alternate(configs, args.rounds)
    for name, _ in configs:
        prec = name.split()[0]
        base = statistics.median(times[f'{prec} self_ensemble=0'])
        lines.append(row(name, times[name], f'{statistics.median(times[name]) / base:5.2f} x the plain frame'))

    # ---- geometry of one 8-variant frame: 7 launches on the input, 8 on the results, against torch on the same tensors
    with torch.no_grad():
        ys = {0: torch.rand(1, 3, 4 * h, 4 * w, device=dev), 1: torch.rand(1, 3, 4 * w, 4 * h, device=dev)}
        acc = torch.empty(1, 3, 4 * h, 4 * w, device=dev)

        def kernel_geometry():
            for k in range(8):
                if k:
                    F.dihedral(lr, k)
                F.dihedral(ys[k & 1], F.dihedral_inverse(k), out=acc, alpha=0.125, beta=0.0 if k == 0 else 1.0)

        def torch_geometry():
            a = None
            for k in range(8):
                if k:
                    T(lr, k).contiguous()
                y = T_inv(ys[k & 1], k) * 0.125
                a = y if a is None else a + y
            return a

        kernel_geometry()
        same = torch.equal(acc, torch_geometry())
        gt = alternate([('kernel', kernel_geometry), ('torch', torch_geometry)], max(args.rounds, 10))
    hr_bytes, lr_bytes = 4 * 3 * 16 * h * w, 4 * 3 * h * w
    need = 8 * hr_bytes + 7 * hr_bytes + 8 * hr_bytes + 7 * 2 * lr_bytes  # results read, sum read (not the first), sum written, inputs
    km, tm = statistics.median(gt['kernel']), statistics.median(gt['torch'])
    lines += ['', f'geometry of one 8-variant frame (7 input + 8 result maps), {max(args.rounds, 10)} alternating rounds; the two '
              f'sums are {"bitwise equal" if same else "NOT EQUAL"}',
              f'{"":<44s} {"median":>10s} {"min":>10s} {"max":>10s}',
              row('srx_dihedral_planes, 15 launches', gt['kernel'],
                  f'{need / 1e9:.2f} GB it must move: {need / (km * 1e-3) / 1e12:.2f} TB/s'),
              row('torch flip / transpose / contiguous / mul / add', gt['torch'], f'{tm / km:5.2f} x the kernel'),
              f'spread (max - min): kernel {max(gt["kernel"]) - min(gt["kernel"]):.3f} ms, torch '
              f'{max(gt["torch"]) - min(gt["torch"]):.3f} ms; difference of the medians {tm - km:.3f} ms']
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
