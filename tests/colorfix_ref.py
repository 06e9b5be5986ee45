"""The colour fixes of ``csrc/colorfix.hip`` restated with numpy: ``wavelet32`` follows the fp32 steps of the kernels one
rounding at a time (the kernels must give its bits), ``adain_ref`` gives the fp64 value of the AdaIN map with the fp32
coefficients and the bound a correct fp32 evaluation stays within."""
import numpy as np

U32 = 2.0 ** -24  # fp32 unit roundoff
F32 = np.float32


def _pass(d, r, axis):
    """``0.25f * (d[cl(i - r)] + d[cl(i + r)]) + 0.5f * d[i]`` along ``axis`` in fp32: the products are exact, the sum of the
    neighbours rounds once and the last addition once (an fma of the exact products rounds the same)."""
    n = d.shape[axis]
    i = np.arange(n)
    lo, hi = np.take(d, np.clip(i - r, 0, n - 1), axis=axis), np.take(d, np.clip(i + r, 0, n - 1), axis=axis)
    out = F32(0.25) * (lo + hi) + F32(0.5) * d
    assert out.dtype == np.float32
    return out


def wavelet32(sr, u, levels=5):
    """``sr + B(u - sr)`` on fp32 arrays ``[..., H, W]``: one rounding for the difference, per level a pass along W then one along
    H at the radius 2^i with replicate padding, one rounding for the last sum."""
    sr, u = np.ascontiguousarray(sr, dtype=np.float32), np.ascontiguousarray(u, dtype=np.float32)
    assert sr.shape == u.shape
    d = u - sr
    for i in range(levels):
        d = _pass(_pass(d, 1 << i, -1), 1 << i, -2)
    return sr + d


def moments64(x):
    """Mean and unbiased variance (0 for one element) of every plane of ``[..., H, W]`` in fp64."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-2] * x.shape[-1]
    return x.mean(axis=(-2, -1)), (x.var(axis=(-2, -1), ddof=1) if n > 1 else np.zeros(x.shape[:-2]))


def adain_ref(sr, lr):
    """``(want, (s, b), bound)``: ``sr * s + b`` per plane in fp64 with ``s = sqrt(var_lr + 1e-5) / sqrt(var_sr + 1e-5)`` and
    ``b = mean_lr - mean_sr * s``; the two rounded to fp32; and ``4 * 2^-24 * (|sr| * s + |b|)`` per element -- a rounding each
    of s, of b and of the fma, with a margin of about 2."""
    (ms, vs), (ml, vl) = moments64(sr), moments64(lr)
    s = np.sqrt(vl + 1e-5) / np.sqrt(vs + 1e-5)
    b = ml - ms * s
    sr64 = np.asarray(sr, dtype=np.float64)
    want = sr64 * s[..., None, None] + b[..., None, None]
    bound = 4 * U32 * (np.abs(sr64) * s[..., None, None] + np.abs(b)[..., None, None])
    return want, (s.astype(np.float32), b.astype(np.float32)), bound
