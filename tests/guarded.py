"""Device tensors with owned surroundings, and the elementwise comparison, for the tests that watch what a kernel reads and writes
next to its tensors (test_linear_forms_gpu.py, test_head_gpu.py); and the plain NaN-guarded output of the degradation kernels'
tests (test_degrade_gpu.py, test_degrade2_gpu.py, test_usm_gpu.py)."""
import ctypes as C
import math

import torch

SENTINEL = 12345.6789
GUARD = 64  # floats of NaN on either side of a _guarded output: a store outside the tensor shows


def _guarded(shape, dev):
    """``(buf, out)``: an output of ``shape``, all NaN, between GUARD NaN floats on either side."""
    n = math.prod(shape)
    buf = torch.full((GUARD + n + GUARD,), float('nan'), device=dev)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _band_kept(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """A contiguous view of `shape` inside a larger device buffer: 64 rows of its own row length (or `margin_floats`) on either
    side, 16-byte aligned.  Inputs: NaN margins.  Outputs: sentinel margins, a NaN (or given) interior."""

    def __init__(self, dev, shape, src=None, margin=float('nan'), margin_floats=None):
        n = 1
        for s in shape:
            n *= s
        self.m = 64 * shape[-1] if margin_floats is None else margin_floats
        self.margin = margin
        self.buf = torch.full((2 * self.m + n,), margin, dtype=torch.float32, device=dev)
        self.t = self.buf[self.m:self.m + n].view(shape)
        self.t.fill_(float('nan'))
        if src is not None:
            self.t.copy_(src)
        assert self.t.data_ptr() % 16 == 0 and self.t.is_contiguous()

    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def margins_unchanged(self):
        want = torch.tensor(self.margin, dtype=torch.float32).view(torch.int32).item()
        got = torch.cat([self.buf[:self.m], self.buf[-self.m:]]).view(torch.int32)
        return bool((got == want).all())


def within(got, ref, bound, what):
    """elementwise, NaN-proof: every element of `got` within its own bound"""
    err = (got.double() - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    ok = err <= bound
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError('%s: %d of %d elements outside their bound; first at %s: got %r, fp64 %r, bound %.3e; worst err / bound %.3f'
                             % (what, len(bad), ok.numel(), i, float(got[i]), float(ref[i]), float(bound[i]),
                                float((err / bound).nan_to_num(float('inf')).max())))
