"""Host side of the second-order degradation ('Second-order degradation'): the blur kernels ``srx_filter2d`` takes as
tables -- Gaussian, generalised Gaussian, plateau and sinc, the families of Real-ESRGAN -- built in float64 with numpy.
Nothing here touches a GPU."""
import functools
import math

import numpy as np

KERNEL_SLOT = 21  # srx_filter2d's slot: a sample's ks x ks kernel sits centred in KERNEL_SLOT x KERNEL_SLOT floats
KERNEL_KINDS = ('gauss', 'generalized', 'plateau', 'sinc')

_J1_THETA = (np.arange(128, dtype=np.float64) + 0.5) * (math.pi / 128)
_J1_SIN = np.sin(_J1_THETA)


def bessel_j1(x):
    """The Bessel function J1 in float64 without scipy: Bessel's integral ``1/pi int_0^pi cos(t - x sin t) dt`` by the midpoint
    rule on 128 points, ``mean_k cos(t_k - x sin t_k)``, ``t_k = (k + 1/2) pi / 128``.  The integrand is periodic and entire, so
    the rule converges geometrically: on [0, 45] (the kernels need ``pi * 10 sqrt 2 = 44.4``) it agrees with
    ``scipy.special.j1`` to 7.1e-16."""
    x = np.asarray(x, dtype=np.float64)
    return np.cos(_J1_THETA - x[..., None] * _J1_SIN).mean(axis=-1)


@functools.lru_cache(maxsize=None)
def _grid(ksize: int):
    """Per kernel size, built once and never written to: ``dx = j - r`` and ``dy = i - r`` (float64 [ks][ks]), the distinct radii
    ``|v|`` and, per tap, which of them it has."""
    r = ksize // 2
    i, j = np.meshgrid(np.arange(ksize), np.arange(ksize), indexing='ij')
    radii, where = np.unique((j - r) ** 2 + (i - r) ** 2, return_inverse=True)
    return (j - r).astype(np.float64), (i - r).astype(np.float64), np.sqrt(radii.astype(np.float64)), where.reshape(ksize, ksize)


def kernel_weights(kind: str, ksize: int, sigma_x: float = 1.0, sigma_y: float = 1.0, theta: float = 0.0, beta: float = 1.0,
                   omega_c: float = math.pi) -> np.ndarray:
    """One blur kernel, float64 ``[ksize][ksize]``, normalised to sum 1.  With ``r = ksize // 2``, ``v = (j - r, i - r)``,
    ``S = R(theta) diag(sigma_x^2, sigma_y^2) R(theta)'`` (``srx_blur_aniso``'s) and ``q = v' S^-1 v``:

    ``'gauss'``: ``exp(-q / 2)``; ``'generalized'``: ``exp(-q^beta / 2)``; ``'plateau'``: ``1 / (1 + q^beta)``;
    ``'sinc'``: the ideal circular low-pass of cutoff ``omega_c``, ``omega_c J1(omega_c rho) / (2 pi rho)`` with ``rho = |v|`` and
    ``omega_c^2 / (4 pi)`` at the centre (basicsr's ``circular_lowpass_kernel``); it has negative lobes."""
    if kind not in KERNEL_KINDS:
        raise ValueError(f'kernel_weights: kind must be one of {KERNEL_KINDS}, got {kind!r}')
    if isinstance(ksize, bool) or not isinstance(ksize, (int, np.integer)) or ksize < 1 or ksize % 2 == 0 or ksize > KERNEL_SLOT:
        raise ValueError(f'kernel_weights: ksize must be odd in 1..{KERNEL_SLOT}, got {ksize!r}')
    dx, dy, rho, where = _grid(int(ksize))
    if kind == 'sinc':  # radially symmetric: J1 once per distinct radius
        safe = np.where(rho > 0, rho, 1.0)
        vals = np.where(rho > 0, omega_c * bessel_j1(omega_c * safe) / (2.0 * math.pi * safe), omega_c * omega_c / (4.0 * math.pi))
        w = vals[where]
    else:
        # S^-1 = R diag(1 / sigma_x^2, 1 / sigma_y^2) R' written out: q = a dx^2 + 2 b dx dy + c dy^2
        cs, sn, ix, iy = math.cos(theta), math.sin(theta), 1.0 / (sigma_x * sigma_x), 1.0 / (sigma_y * sigma_y)
        q = (cs * cs * ix + sn * sn * iy) * (dx * dx) + (2.0 * cs * sn * (ix - iy)) * (dx * dy) + (sn * sn * ix + cs * cs * iy) * (dy * dy)
        if kind == 'gauss':
            w = np.exp(-0.5 * q)
        elif kind == 'generalized':
            w = np.exp(-0.5 * np.power(q, beta))
        else:
            w = 1.0 / (1.0 + np.power(q, beta))
    return w / w.sum()


def kernel_slot(w, out=None) -> np.ndarray:
    """``w`` ([ks][ks], ks odd) rounded to float32 and centred in a zero ``[21][21]`` slot, as ``srx_filter2d`` reads it; ``w =
    None`` (no kernel: ksize 0) leaves the slot zero."""
    slot = np.zeros((KERNEL_SLOT, KERNEL_SLOT), dtype=np.float32) if out is None else out
    if w is not None:
        ks = w.shape[0]
        o = KERNEL_SLOT // 2 - ks // 2
        slot[o:o + ks, o:o + ks] = w
    return slot
