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


# ------------------------------------------------------------------------------------------------ Poisson noise
POISSON_VALS = (1, 2, 4, 8, 16, 32, 64, 128, 256)  # what the number of distinct 8-bit levels of a sample rounds up to
POISSON_K = 512      # entries of a full threshold row: k = 0 .. 511
POISSON_WINDOW = 256  # entries of a packed row; the part of a full row that is neither 0 nor 2^31 is under 200 entries wide


@functools.lru_cache(maxsize=None)
def _poisson_thresholds(vals: int) -> np.ndarray:
    lg = np.array([math.lgamma(k + 1.0) for k in range(POISSON_K)], dtype=np.float64)
    k = np.arange(POISSON_K, dtype=np.float64)
    t = np.empty((256, POISSON_K), dtype=np.uint32)
    for level in range(256):
        lam = level * vals / 255                                  # float64 from the two integers
        if level == 0:
            pmf = np.zeros(POISSON_K, dtype=np.float64)
            pmf[0] = 1.0
        else:
            pmf = np.exp(k * math.log(lam) - lam - lg)
        cdf = np.cumsum(pmf)                                      # ascending k
        tail = np.cumsum(pmf[::-1])[::-1] - pmf                   # sum over j > k, the small terms first
        row = np.minimum(np.floor(cdf * 2.0 ** 31), 2.0 ** 31)
        row[tail < 2.0 ** -32] = 2.0 ** 31
        t[level] = row.astype(np.uint32)
    t.setflags(write=False)
    return t


def poisson_thresholds(vals: int) -> np.ndarray:
    """The sampler's table for one of ``POISSON_VALS``: uint32 ``T[256][512]``, ``T[level][k] = min(floor(CDF(k) 2^31), 2^31)`` of
    the Poisson distribution with ``lambda = level * vals / 255``.  A draw is the smallest ``k`` with ``(r >> 1) < T[level][k]``,
    ``r`` a uniform 32-bit word.  lambda is formed in float64 from the integers, the pmf is ``exp(k ln(lambda) - lambda -
    lgamma(k + 1))`` and is summed in ascending ``k``; level 0 is the point mass at 0.  A float64 sum of the whole pmf ends one
    ulp below 1 as often as on it, so a row would stall at ``2^31 - 1`` and a draw could run off its end: from the first ``k``
    whose upper tail ``sum_{j > k} pmf(j)`` (summed from the far end) is below ``2^-32`` the entry IS ``2^31`` -- one count above
    the exact floor, where ``r >> 1`` cannot tell the two apart by more than its own resolution.  Read-only; built once."""
    if isinstance(vals, bool) or not isinstance(vals, (int, np.integer)) or int(vals) not in POISSON_VALS:
        raise ValueError(f'poisson_thresholds: vals must be one of {POISSON_VALS}, got {vals!r}')
    return _poisson_thresholds(int(vals))


@functools.lru_cache(maxsize=None)
def poisson_table_words() -> np.ndarray:
    """The nine tables as ``srx_add_poisson_noise`` reads them, one int32 array: ``first[9][256]``, then the uint32 windows
    ``win[9][256][256]`` (their bit patterns), ``v = log2(vals)``.  ``first[v][level]`` is the first ``k`` whose threshold is not
    0 and ``win[v][level][j] = T[level][first + j]`` (``2^31`` past the row's end); every window ends on ``2^31``, so the
    smallest ``k`` with ``(r >> 1) < T[level][k]`` is ``first`` plus the number of window entries that are ``<= r >> 1``."""
    first = np.zeros((len(POISSON_VALS), 256), dtype=np.int32)
    win = np.full((len(POISSON_VALS), 256, POISSON_WINDOW), 1 << 31, dtype=np.uint32)
    for v, vals in enumerate(POISSON_VALS):
        t = poisson_thresholds(vals)
        for level in range(256):
            k0 = int(np.argmax(t[level] > 0))
            part = t[level, k0:k0 + POISSON_WINDOW]
            first[v, level] = k0
            win[v, level, :len(part)] = part
    if not (win[:, :, -1] == 1 << 31).all():
        raise AssertionError('poisson_table_words: a row does not reach 2^31 inside its window')
    words = np.concatenate([first.reshape(-1), win.reshape(-1).view(np.int32)])
    words.setflags(write=False)
    return words
