"""Restatements for the second-order degradation in numpy / torch float64: ``srx_filter2d``, the separable resize of
``functional.resize_tables`` and torch's own ``interpolate`` as its reference.  Imported by test_degrade2_cpu.py and
test_degrade2_gpu.py; nothing here touches a GPU."""
import numpy as np
import torch

import degrade_ref as R

SLOT = 21
# the size pairs the resize tables were checked on: reductions, enlargements, the identity, the smallest and most lopsided
RESIZE_PAIRS = [(96, 16), (96, 144), (96, 72), (144, 16), (16, 32), (24, 24), (40, 24), (128, 192), (11, 7), (7, 11), (5, 80),
                (80, 5), (16, 24), (136, 32)]
MODES = ('area', 'bilinear', 'bicubic')


def reflect_index(i: np.ndarray, n: int) -> np.ndarray:
    """-k -> k, n - 1 + k -> n - 1 - k (torch's mode='reflect'), for |offset| <= n - 1."""
    i = np.abs(i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def window(slot: np.ndarray, ks: int) -> np.ndarray:
    """The centred ks x ks window of a 21 x 21 slot."""
    o = SLOT // 2 - ks // 2
    return slot[o:o + ks, o:o + ks]


def quantize8(v):
    return np.rint(np.clip(v, 0.0, 1.0) * 255.0) / 255.0


def filter2d(x, weights, ksize, quantize=0) -> np.ndarray:
    """``srx_filter2d`` in float64, by its definition: out[n][c][y][x] = sum_ij w_n[i][j] in[n][c][y + i - r][x + j - r] over the
    centred window of sample n's slot, indices reflected; the size clamped as the kernel clamps it; weights as given."""
    x = np.asarray(x, dtype=np.float64)
    weights = np.asarray(weights, dtype=np.float64)
    n_s, _, h, w = x.shape
    out = np.empty_like(x)
    for n in range(n_s):
        ks = R.legal_ksize(int(ksize[n]))
        if ks == 0:
            out[n] = x[n]
            continue
        r, wn = ks // 2, window(weights[n], ks)
        acc = np.zeros_like(x[n])
        for i in range(ks):
            rows = reflect_index(np.arange(h) + i - r, h)
            for j in range(ks):
                cols = reflect_index(np.arange(w) + j - r, w)
                acc += wn[i, j] * x[n][:, rows][:, :, cols]
        out[n] = acc
    return quantize8(out) if quantize else out


def filter2d_conv(x, weights, ksize) -> torch.Tensor:
    """The same through torch: reflect padding + conv2d (a correlation), one kernel per sample, float64."""
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64)
    out = torch.empty_like(x)
    for n in range(x.shape[0]):
        ks = R.legal_ksize(int(ksize[n]))
        if ks == 0:
            out[n] = x[n]
            continue
        wn = torch.as_tensor(np.ascontiguousarray(window(np.asarray(weights[n], dtype=np.float64), ks)))
        p = torch.nn.functional.pad(x[n][None], (ks // 2,) * 4, mode='reflect')
        out[n] = torch.nn.functional.conv2d(p, wn[None, None].expand(x.shape[1], 1, ks, ks), groups=x.shape[1])[0]
    return out


def filter2d_tolerance(weights, ksize, xmax: float) -> float:
    """The fp32 bound of one filter2d case: ks^2 products and sums, (ks^2 + 2) 2^-24 sum |w| max |x|, at the worst sample."""
    tol = 0.0
    for n in range(len(ksize)):
        ks = R.legal_ksize(int(ksize[n]))
        if ks:
            tol = max(tol, (ks * ks + 2) * 2.0 ** -24 * float(np.abs(window(np.asarray(weights[n], dtype=np.float64), ks)).sum()) * xmax)
    return tol


def apply_tables(x: np.ndarray, start, weight, axis: int) -> np.ndarray:
    """One axis of ``srx_resample_planes`` in the dtype of ``weight``'s product with ``x``: out[i] = sum_t weight[i][t] x[min(start[i]
    + t, n_in - 1)] along ``axis``."""
    x = np.moveaxis(np.asarray(x), axis, -1)
    n_in = x.shape[-1]
    idx = np.minimum(np.asarray(start, dtype=np.int64)[:, None] + np.arange(weight.shape[1])[None, :], n_in - 1)
    out = (x[..., idx] * weight).sum(axis=-1)
    return np.moveaxis(out, -1, axis)


def interpolate64(x, size, mode) -> np.ndarray:
    """torch's resize without antialiasing on the float64 CPU copy of ``x`` (NCHW), the reference of ``functional.resize``."""
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64)
    kw = {} if mode == 'area' else {'align_corners': False}
    return torch.nn.functional.interpolate(x, size=size, mode=mode, **kw).numpy()


def resize_tolerance(tables_y, tables_x, xmax: float) -> float:
    """(Ky + 2) 2^-24 sum |w_y| + (Kx + 2) 2^-24 sum |w_x|, each sum at the worst row of its table, times max |x|."""
    tol = 0.0
    for _, weight, k in (tables_y, tables_x):
        tol += (k + 2) * 2.0 ** -24 * float(np.abs(np.asarray(weight, dtype=np.float64)).sum(axis=1).max())
    return tol * xmax
