"""Dump the conv planners' answers for a grid of layers (developer tool, host code only: no GPU needed): the check that a
change to the planners, the forced-plan refusals or the tile table changed no plan.

    SRX_LIB=/path/to/libsrx_hip.so python tools/plan_dump.py OUT.txt      # once per library; then `cmp` the two files

One line per (override, layer): the six numbers of srx_conv2d_plan for the forward and for the data gradient, then
srx_conv2d_fwd_ws_floats / srx_conv2d_bwd_data_ws_floats -- or, where a call is refused, its status and message.  The layers:
the conv shapes of the SRGAN and ESRGAN training steps (tests/step_layers.py; what tools/shapes.py and tools/esrgan_shapes.py
profile), of 1080p -> 8K inference (tools/infer_shapes.py) with its whole-frame and fp16 calls, and a cross product of batch,
extent, channels, stride, kernel size and precision.  The overrides: none, every value srx_conv2d_force_plan accepts, every
value srx_conv2d_force_s2 accepts, and a few values each refuses.
"""
import ctypes as C
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.step_layers import FULL_SIZE_LAYERS, STEP_CONVS  # noqa: E402
from torchsr_amd import _lib  # noqa: E402


def desc(n, h, w, cin, cout, k, stride, pad, shuffle=0, up=0, prec=0, cin_s=None):
    cin_s = cin_s or (cin + 3) // 4 * 4
    cout_s = (cout // 4 if shuffle else cout) + 3 & ~3
    return _lib.Conv2dDesc(n, h, w, cin, cin_s, cout, cout_s, k, k, stride, pad, shuffle, 0, 0.0, up, prec)


def layers():
    out = []
    for prec in (0, 1):
        for s in FULL_SIZE_LAYERS:
            out.append(desc(*s[:8], shuffle=s[8], prec=prec))
        for c in STEP_CONVS:
            if 'shape' in c:
                out.append(desc(*c['shape'], shuffle=c.get('shuffle', 0), prec=prec))
        # ESRGAN step, batch 16, 32 -> 128 pixel crops: dense blocks (one 192-channel buffer), trunk, x2 upsampling convs, discriminator
        for i in range(4):
            out.append(desc(16, 32, 32, 64 + 32 * i, 32, 3, 1, 1, prec=prec, cin_s=192))
        out.append(desc(16, 32, 32, 192, 64, 3, 1, 1, prec=prec))
        out += [desc(16, 32, 32, 3, 64, 3, 1, 1, prec=prec), desc(16, 32, 32, 64, 64, 3, 1, 1, prec=prec),
                desc(16, 32, 32, 64, 64, 3, 1, 1, up=2, prec=prec), desc(16, 64, 64, 64, 64, 3, 1, 1, up=2, prec=prec),
                desc(16, 128, 128, 64, 64, 3, 1, 1, prec=prec), desc(16, 128, 128, 64, 3, 3, 1, 1, prec=prec)]
        for n in (16, 32):
            hw, cin = 128, 64
            out.append(desc(n, 128, 128, 3, 64, 3, 1, 1, prec=prec))
            for cout in (64, 128, 128, 256, 256, 512, 512, 512, 512):
                stride = 2 if cout == cin else 1
                out.append(desc(n, hw, hw, cin, cout, 3, stride, 1, prec=prec))
                hw, cin = hw // stride, cout
        # 1080p -> 8K inference: SRGAN generator, then whole-frame calls above 2^24 pixels
        out += [desc(1, 1080, 1920, 3, 64, 9, 1, 4, prec=prec), desc(1, 1080, 1920, 64, 64, 3, 1, 1, prec=prec),
                desc(1, 1080, 1920, 64, 256, 3, 1, 1, shuffle=2, prec=prec), desc(1, 2160, 3840, 64, 256, 3, 1, 1, shuffle=2, prec=prec),
                desc(1, 4320, 7680, 64, 3, 9, 1, 4, prec=prec)]
        for cout in (32, 64, 128, 96):
            out.append(desc(1, 4320, 7680, 64, cout, 3, 1, 1, prec=prec))
    out += [desc(1, 1080, 1920, 3, 64, 9, 1, 4, prec=3), desc(1, 4320, 7680, 3, 64, 3, 1, 1, prec=3), desc(1, 4320, 7680, 3, 32, 3, 1, 1, prec=3),
            desc(1, 1080, 1920, 64, 3, 9, 1, 4, prec=2), desc(16, 24, 24, 3, 128, 3, 1, 1, prec=3)]
    chans = (3, 32, 48, 64, 96, 128, 256, 512)
    for n, e, cin, cout, stride, k, prec in itertools.product((1, 3, 16), (6, 13, 24, 96, 128), chans, chans, (1, 2), (1, 3, 5), (0, 1)):
        out.append(desc(n, e, e, cin, cout, k, stride, k // 2, prec=prec))
    return out


def main():
    L = _lib.lib()
    descs = layers()
    names = [' '.join(str(getattr(d, f)) for f, _ in d._fields_ if f not in ('act', 'slope')) for d in descs]
    refs = [C.byref(d) for d in descs]
    plan = (C.c_int * 6)()

    def one(ref, which):
        for i in range(6):
            plan[i] = -1
        rc = L.srx_conv2d_plan(ref, which, plan)
        return ','.join(map(str, plan)) if rc == 0 else 'status %d: %s' % (rc, _lib.last_error())

    count = [0]

    def dump(f, tag):
        # (the layer is spelled out in the first dump and named by its index in the others)
        for i, (name, ref) in enumerate(zip(names, refs)):
            f.write('%s | %s | fwd %s | dgrad %s | ws %d %d\n' % (tag, name if tag == 'model' else '#%d' % i, one(ref, 0), one(ref, 1),
                                                               L.srx_conv2d_fwd_ws_floats(ref), L.srx_conv2d_bwd_data_ws_floats(ref)))
        count[0] += len(refs)

    def force(f, fn, args):
        rc = getattr(L, fn)(*args)
        f.write('%s%s -> %s\n' % (fn, args, 'accepted' if rc == 0 else 'status %d: %s' % (rc, _lib.last_error())))
        count[0] += 1
        return rc == 0

    with open(sys.argv[1], 'w') as f:
        dump(f, 'model')
        # every argument set near the accepted ones: the accepted dump, the refused print their message
        for args in itertools.product((0, 32, 64, 100, 128, 144, 256), (0, 32, 64, 96, 128, 256), range(0, 18), (0, 1, 2, 3)):
            if force(f, 'srx_conv2d_force_plan', args) and any(args):
                dump(f, 'plan %d,%d,%d,%d' % args)
        force(f, 'srx_conv2d_force_plan', (0, 0, 0, 0))
        for args in itertools.product((0, 1, 2, 3), (0, 32, 64, 96, 128, 144, 256), (0, 32, 64, 128, 256)):
            if force(f, 'srx_conv2d_force_s2', args) and any(args):
                dump(f, 's2 %d,%d,%d' % args)
        for s2, fp in itertools.product(((1, 0, 0), (2, 0, 0), (2, 128, 64)), ((64, 64, 1, 2), (144, 128, 1, 1), (64, 32, 2, 1), (256, 128, 1, 1))):
            force(f, 'srx_conv2d_force_s2', s2)
            force(f, 'srx_conv2d_force_plan', fp)
            dump(f, 's2 %d,%d,%d plan %d,%d,%d,%d' % (s2 + fp))
        force(f, 'srx_conv2d_force_plan', (0, 0, 0, 0))
        force(f, 'srx_conv2d_force_s2', (0, 0, 0))
    print('%d layers, %d lines written to %s' % (len(descs), count[0], sys.argv[1]))


if __name__ == '__main__':
    main()
