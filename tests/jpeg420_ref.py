"""``srx_jpeg_sim2`` restated in numpy ('Chroma subsampling'): the JPEG model of degrade_ref.py with 4:2:0 chroma
subsampling per sample -- libjpeg's h2v2_downsample on the integer Cb and Cr, the H/2 x W/2 planes edge-replicated to whole
blocks, the chrominance table, and libjpeg's h2v2_fancy_upsample in floating point -- split into its encode half (the quotients
coefficient / step before the rounding) and its decode half (from rounded quotients to RGB), each with every float operation in
one dtype; and the real codec at 4:2:0 through PIL."""
import io

import numpy as np

from degrade_ref import _blocks, _unblocks, dct_matrix, jpeg_images, jpeg_sim, jpeg_tables  # noqa: F401


def chroma_blocks(extent: int) -> int:
    """8 x 8 blocks along one axis of the padded chroma plane of an image ``extent`` pixels long: one per 16 pixels, rounded up."""
    return (extent + 15) // 16


def coded(q) -> bool:
    return 1 <= int(q) <= 100


def ycc_levels(x, dtype=np.float64):
    """[3][H][W] in [0, 1] -> libjpeg's integer Y, Cb, Cr, int64 [3][H][W]"""
    s = np.clip(np.rint(np.asarray(x).astype(dtype) * dtype(255.0)), 0, 255).astype(np.int64)
    r, g, b = s[0], s[1], s[2]
    return np.stack([(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
                     (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
                     (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16])


def downsample(c):
    """libjpeg's h2v2_downsample on integer planes [..., H, W] -> [..., H/2, W/2]: (a + b + c + d + bias) >> 2, bias 1, 2, 1, 2, ...
    along the output columns of every row."""
    bias = 1 + (np.arange(c.shape[-1] // 2) & 1)
    return (c[..., 0::2, 0::2] + c[..., 0::2, 1::2] + c[..., 1::2, 0::2] + c[..., 1::2, 1::2] + bias) >> 2


def pad_edge(p):
    """[..., h, w] edge-replicated to multiples of 8: what the padding of a partial 16 x 16 MCU amounts to."""
    h, w = p.shape[-2:]
    return np.pad(p, [(0, 0)] * (p.ndim - 2) + [(0, -h % 8), (0, -w % 8)], mode='edge')


def upsample(p, dtype=np.float64):
    """libjpeg's h2v2_fancy_upsample without its integer rounding, [..., h, w] -> [..., 2 h, 2 w]: 3 (3 c + v) + (3 h + d) over
    16, c the sample over the pixel, v / h its vertical / horizontal neighbour on the pixel's side, d the diagonal one; a
    neighbour outside the plane is the edge sample."""
    p = np.asarray(p, dtype=dtype)
    h, w = p.shape[-2:]

    def near_far(n):
        i = np.arange(2 * n)
        return i >> 1, np.clip((i >> 1) + np.where(i & 1, 1, -1), 0, n - 1)

    (cy, ny), (cx, nx) = near_far(h), near_far(w)
    f = dtype
    c, v = p[..., cy, :][..., cx], p[..., ny, :][..., cx]
    hn, d = p[..., cy, :][..., nx], p[..., ny, :][..., nx]
    return (f(3.0) * (f(3.0) * c + v) + (f(3.0) * hn + d)) / f(16.0)


def _steps(q, dtype):
    ql, qc = jpeg_tables(int(q))
    return ql.astype(dtype), qc.astype(dtype)


def encode(x, quality, chroma420, dtype=np.float64):
    """The encode half: ``quot`` [N][3][H W] of ``dtype`` in ``srx_jpeg_sim2``'s ``quot_out`` layout -- coefficient / step before the
    rounding, block after block in raster order, 64 values each; a 4:4:4 sample's planes from [n][0], [n][1], [n][2]; a 4:2:0
    sample's Y blocks from [n][0] and its ceil(H / 16) x ceil(W / 16) Cb and Cr blocks from [n][1] and [n][2]; zero elsewhere."""
    x = np.asarray(x)
    n_s, _, h, w = x.shape
    quot = np.zeros((n_s, 3, h * w), dtype=dtype)
    d = dct_matrix().astype(dtype)
    for n in range(n_s):
        if not coded(quality[n]):
            continue
        ql, qc = _steps(quality[n], dtype)
        ycc = ycc_levels(x[n], dtype)

        def t(planes, step):
            return (np.matmul(np.matmul(d, _blocks((planes - 128).astype(dtype))), d.T) / step).reshape(planes.shape[0], -1)

        if chroma420[n]:
            quot[n, 0] = t(ycc[:1], ql)[0]
            tc = t(pad_edge(downsample(ycc[1:])), qc)
            quot[n, 1:, :tc.shape[1]] = tc
        else:
            quot[n, 0], quot[n, 1:] = t(ycc[:1], ql)[0], t(ycc[1:], qc)
    return quot


def decode_ycc(quot_n, h, w, q, flag, dtype=np.float64):
    """One coded sample's decoded Y, Cb - 128, Cr - 128, [3][H][W] of ``dtype``, from its ROUNDED quotients [3][H W]."""
    d = dct_matrix().astype(dtype)
    ql, qc = _steps(q, dtype)

    def dec(tq, hb, wb, step):
        blk = np.asarray(tq, dtype=dtype).reshape(-1, hb, wb, 8, 8) * step
        return _unblocks(np.matmul(np.matmul(d.T, blk), d))

    yy = dec(quot_n[0], h // 8, w // 8, ql) + dtype(128.0)
    if flag:
        hb, wb = chroma_blocks(h), chroma_blocks(w)
        cbcr = upsample(dec(quot_n[1:, :hb * wb * 64], hb, wb, qc)[:, :h // 2, :w // 2], dtype)
    else:
        cbcr = dec(quot_n[1:], h // 8, w // 8, qc)
    return np.concatenate([yy, cbcr])


def decode(quot, x, quality, chroma420, quantize, dtype=np.float64):
    """The decode half: from ROUNDED quotients in ``encode``'s layout to RGB [N][3][H][W] of ``dtype``; ``x`` gives the shape and
    the samples whose quality is no JPEG quality, which are copied."""
    x = np.asarray(x)
    n_s, _, h, w = x.shape
    out = np.empty(x.shape, dtype=dtype)
    f = dtype
    for n in range(n_s):
        if not coded(quality[n]):
            out[n] = x[n]
            continue
        yy, cb, cr = decode_ycc(quot[n], h, w, quality[n], chroma420[n], dtype)
        rgb = np.stack([yy + f(1.402) * cr, yy - f(0.344136286) * cb - f(0.714136286) * cr, yy + f(1.772) * cb])
        o = np.clip(rgb / f(255.0), 0, 1)
        out[n] = np.rint(o * f(255.0)) / f(255.0) if quantize else o
    return out


def jpeg420_sim(x, quality, chroma420, quantize, dtype=np.float64):
    """``srx_jpeg_sim2`` with every float operation in ``dtype``.  Returns (out [N][3][H][W], quot [N][3][H W])."""
    quot = encode(x, quality, chroma420, dtype)
    return decode(np.rint(quot), x, quality, chroma420, quantize, dtype), quot


def pil_jpeg420(img8: np.ndarray, quality: int):
    """The real codec: ``img8`` uint8 [3][H][W] saved with ``quality`` and 4:2:0, decoded.  Returns (uint8 [3][H][W], tables)."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img8.transpose(1, 2, 0))).save(buf, 'JPEG', quality=quality, subsampling=2)
    buf.seek(0)
    im = Image.open(buf)
    tables = {k: np.asarray(list(v)).reshape(8, 8) for k, v in im.quantization.items()}
    return np.asarray(im.convert('RGB')).transpose(2, 0, 1), tables


def pil_ratio420(result, img, quality: int, pil=None) -> float:
    """degrade_ref.pil_ratio against the 4:2:0 file: mse(PIL, source) / mse(result, PIL) in grey levels for one image
    [3][H][W] in [0, 1].  ``pil``: the decoded file, when the caller already has it."""
    src = np.rint(np.asarray(img, dtype=np.float64) * 255)
    if pil is None:
        pil, _ = pil_jpeg420(src.astype(np.uint8), quality)
    pil = pil.astype(np.float64)
    res = np.asarray(result, dtype=np.float64) * 255
    return float(((pil - src) ** 2).mean() / ((res - pil) ** 2).mean())
