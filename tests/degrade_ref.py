"""Restatements of the blind-degradation kernels (csrc/degrade.hip) in numpy / torch float64, and of Philox4x32-10 in
integer numpy.  Imported by test_degrade_cpu.py and test_degrade_gpu.py; nothing here touches a GPU."""
import io
import math

import numpy as np
import torch

# ---------------------------------------------------------------------------------------------------------------- blur
BLUR_MAX_K = 21


def legal_ksize(k: int) -> int:
    """What the kernel makes of a kernel size: <= 0 copies, even sizes go to the next odd one, more than 21 is 21."""
    if k <= 0:
        return 0
    return min(k | 1, BLUR_MAX_K)


def blur_weights(sigma_x: float, sigma_y: float, theta: float, ksize: int) -> torch.Tensor:
    """w[i][j] = exp(-v' S^-1 v / 2) / sum, v = (j - r, i - r), S = R(theta) diag(sx^2, sy^2) R(theta)', float64."""
    r = ksize // 2
    c, s = math.cos(theta), math.sin(theta)
    rot = np.array([[c, -s], [s, c]])
    inv = np.linalg.inv(rot @ np.diag([sigma_x ** 2, sigma_y ** 2]) @ rot.T)
    i, j = np.meshgrid(np.arange(ksize), np.arange(ksize), indexing='ij')
    v = np.stack([j - r, i - r], -1).astype(np.float64)
    w = np.exp(-0.5 * np.einsum('ija,ab,ijb->ij', v, inv, v))
    return torch.from_numpy(w / w.sum())


def blur(x: torch.Tensor, parm, ksize) -> torch.Tensor:
    """``srx_blur_aniso`` in float64: reflect padding + conv2d (a correlation), one kernel per sample."""
    x = x.detach().cpu().double()
    out = torch.empty_like(x)
    for n in range(x.shape[0]):
        k = legal_ksize(int(ksize[n]))
        if k == 0:
            out[n] = x[n]
            continue
        w = blur_weights(float(parm[n][0]), float(parm[n][1]), float(parm[n][2]), k)
        p = torch.nn.functional.pad(x[n][None], (k // 2,) * 4, mode='reflect')
        out[n] = torch.nn.functional.conv2d(p, w[None, None].expand(x.shape[1], 1, k, k), groups=x.shape[1])[0]
    return out


# ---------------------------------------------------------------------------------------------------------------- Philox
def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., 'Parallel random numbers: as easy as 1, 2, 3', SC11).  ``counter``: four uint32 arrays
    (or ints), ``key``: two; returns four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & 0xFFFFFFFF for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    m0, m1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                       # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & mask, p1 >> np.uint64(32), p1 & mask
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def gaussian_z(n_samples: int, h: int, w: int, seed_lo: int, seed_hi: int, gray) -> np.ndarray:
    """The normal deviates of ``srx_add_gaussian_noise``, float64 [N][3][H][W]: counter (p, n, 0, 0), key (seed_lo, seed_hi)."""
    p = np.arange(h * w, dtype=np.uint64)[None, :]
    n = np.arange(n_samples, dtype=np.uint64)[:, None]
    r = philox4x32_10((p, n, 0, 0), (seed_lo, seed_hi))
    u = [((v >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24 for v in r]
    rad0, rad2 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    z = np.stack([rad0 * np.cos(2 * np.pi * u[1]), rad0 * np.sin(2 * np.pi * u[1]), rad2 * np.cos(2 * np.pi * u[3])], 1)
    g = np.asarray(gray).astype(bool)
    z[g] = z[g][:, :1]
    return z.reshape(n_samples, 3, h, w)


def add_gaussian_noise(x, sigma, gray, seed_lo, seed_hi, quantize):
    """Float64 ``srx_add_gaussian_noise``.  Returns (out, pre): ``pre`` is the value in grey levels before the rounding
    (None without ``quantize``)."""
    x = np.asarray(x, dtype=np.float64)
    n, _, h, w = x.shape
    v = x + np.asarray(sigma, dtype=np.float64)[:, None, None, None] * gaussian_z(n, h, w, seed_lo, seed_hi, gray)
    if not quantize:
        return v, None
    pre = np.clip(v, 0.0, 1.0) * 255.0
    return np.rint(pre) / 255.0, pre


# ---------------------------------------------------------------------------------------------------------------- JPEG
# ITU-T T.81 Annex K, tables K.1 and K.2, row-major [vertical frequency][horizontal frequency]
JPEG_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]).reshape(8, 8)
JPEG_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                        47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32).reshape(8, 8)


def jpeg_tables(quality: int):
    """libjpeg's jpeg_quality_scaling + jpeg_add_quant_table (baseline): the luminance and chrominance step tables."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (JPEG_LUMA, JPEG_CHROMA))


def dct_matrix() -> np.ndarray:
    k, n = np.meshgrid(np.arange(8), np.arange(8), indexing='ij')
    d = 0.5 * np.cos((2 * n + 1) * k * np.pi / 16)
    d[0] /= np.sqrt(2.0)
    return d


def _blocks(p):
    """[..., H, W] -> [..., H/8, W/8, 8, 8]"""
    h, w = p.shape[-2:]
    return p.reshape(p.shape[:-2] + (h // 8, 8, w // 8, 8)).swapaxes(-3, -2)


def _unblocks(b):
    hb, wb = b.shape[-4], b.shape[-3]
    return b.swapaxes(-3, -2).reshape(b.shape[:-4] + (hb * 8, wb * 8))


def jpeg_sim(x, quality, quantize, dtype=np.float64):
    """``srx_jpeg_sim`` with every float operation in ``dtype``.  Returns (out [N][3][H][W], t [N][3][H/8][W/8][8][8]): ``t`` is
    coefficient / step before the rounding (zeros for a passed-through sample)."""
    x = np.asarray(x)
    out = np.empty(x.shape, dtype=dtype)
    n_s, _, h, w = x.shape
    t_all = np.zeros((n_s, 3, h // 8, w // 8, 8, 8), dtype=dtype)
    d = dct_matrix().astype(dtype)
    f = lambda v: dtype(v)  # noqa: E731
    for n in range(n_s):
        q = int(quality[n])
        if q < 1 or q > 100:
            out[n] = x[n]
            continue
        s = np.clip(np.rint(x[n].astype(dtype) * f(255.0)), 0, 255).astype(np.int64)
        r, g, b = s[0], s[1], s[2]
        ycc = np.stack([(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
                        (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
                        (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16])
        blk = _blocks((ycc - 128).astype(dtype))
        coef = np.matmul(np.matmul(d, blk), d.T)
        ql, qc = jpeg_tables(q)
        step = np.stack([ql, qc, qc]).astype(dtype)[:, None, None]
        t = coef / step
        t_all[n] = t
        dec = _unblocks(np.matmul(np.matmul(d.T, np.rint(t) * step), d))
        yy, cb, cr = dec[0] + f(128.0), dec[1], dec[2]
        rgb = np.stack([yy + f(1.402) * cr, yy - f(0.344136286) * cb - f(0.714136286) * cr, yy + f(1.772) * cb])
        o = np.clip(rgb / f(255.0), 0, 1)
        out[n] = np.rint(o * f(255.0)) / f(255.0) if quantize else o
    return out, t_all


def tie_prone_blocks(t: np.ndarray, delta: float) -> np.ndarray:
    """bool [N][H/8][W/8]: some of the block's 192 values coefficient / step lies within ``delta`` of a half-integer."""
    frac = np.abs(t - np.floor(t) - 0.5)
    return (frac < delta).any(axis=(1, 4, 5))


def jpeg_images(n: int, h: int, w: int, seed: int) -> np.ndarray:
    """The 8-bit valued float32 images of the JPEG tests, [n][3][h][w]: 0.5 + 0.3 sin(x / 5 + c + t) + 0.1 cos(y / 3 + t) +
    N(0, 0.03), t the image's number."""
    rng = np.random.RandomState(seed)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    img = np.stack([np.stack([0.5 + 0.3 * np.sin(x / 5 + c + t) + 0.1 * np.cos(y / 3 + t) for c in range(3)]) for t in range(n)])
    img = img + rng.normal(0, 0.03, img.shape)
    return (np.rint(np.clip(img, 0, 1) * 255) / 255).astype(np.float32)


def pil_jpeg(img8: np.ndarray, quality: int):
    """The real codec: ``img8`` uint8 [3][H][W] saved with ``quality`` and 4:4:4, decoded.  Returns (uint8 [3][H][W], tables)."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img8.transpose(1, 2, 0))).save(buf, 'JPEG', quality=quality, subsampling=0)
    buf.seek(0)
    im = Image.open(buf)
    tables = {k: np.asarray(list(v)).reshape(8, 8) for k, v in im.quantization.items()}
    return np.asarray(im.convert('RGB')).transpose(2, 0, 1), tables


def pil_ratio(result, img, quality: int) -> float:
    """mse(PIL, source) / mse(result, PIL) in grey levels for one image [3][H][W] in [0, 1]: how much nearer ``result`` lies to
    what libjpeg decodes than the compression's own damage."""
    src = np.rint(np.asarray(img, dtype=np.float64) * 255)
    pil, _ = pil_jpeg(src.astype(np.uint8), quality)
    pil = pil.astype(np.float64)
    res = np.asarray(result, dtype=np.float64) * 255
    return float(((pil - src) ** 2).mean() / ((res - pil) ** 2).mean())
