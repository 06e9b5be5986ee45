"""Restatement of ``srx_add_poisson_noise`` (csrc/degrade.hip) in numpy: the levels in float32 (the kernel's own operations, one
rounding each), the draws in integers from the full threshold rows of ``degradation.poisson_thresholds`` (not the packed windows
the device reads), the result in float64; and the exact thresholds with ``decimal``.  Imported by test_poisson_cpu.py and
test_poisson_gpu.py; nothing here touches a GPU."""
import decimal

import numpy as np

from degrade_ref import philox4x32_10

F32 = np.float32


def luma(x: np.ndarray) -> np.ndarray:
    """float32 [N][H][W]: fadd(fadd(fmul(.299f, r), fmul(.587f, g)), fmul(.114f, b)), every operation rounded to float32."""
    x = np.asarray(x, dtype=F32)
    return (F32(.299) * x[:, 0] + F32(.587) * x[:, 1]) + F32(.114) * x[:, 2]


def _fma32(a, b, c):
    """``(fl32(a * b + c), ambiguous)`` for float32 arrays through float64: the product is exact there, the sum is rounded to
    53 bits and then to 24, which is the single rounding of an fma unless the float64 value sits exactly on a float32 midpoint --
    those elements are flagged."""
    d = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)
    return d.astype(F32), (d.view(np.uint64) & np.uint64((1 << 29) - 1)) == np.uint64(1 << 28)


def wrong_lumas(x: np.ndarray):
    """What ``luma`` must NOT be, float32 [N][H][W] each, and the elements whose emulation is ambiguous: the two contractions a
    compiler that fuses freely makes of it -- ``fl(fma(.587, g, fl(.299 r)) + fl(.114 b))`` and ``fma(b, .114, fma(.299, r,
    fl(.587 g)))`` -- and the sum in the other order, ``fl(.299 r) + (fl(.587 g) + fl(.114 b))``."""
    x = np.asarray(x, dtype=F32)
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    cr, cg, cb = F32(.299), F32(.587), F32(.114)
    a1, m1 = _fma32(cg, g, cr * r)
    b1, m2 = _fma32(cr, r, cg * g)
    b2, m3 = _fma32(b, cb, b1)
    return (a1 + cb * b, b2, cr * r + (cg * g + cb * b)), m1 | m2 | m3


def level(v: np.ndarray) -> np.ndarray:
    """int64: rintf(fminf(fmaxf(v, 0), 1) * 255) in float32; a NaN counts as 0 (fmaxf returns the other operand)."""
    v = np.asarray(v, dtype=F32)
    v = np.where(np.isnan(v), F32(0), v)
    return np.rint(np.minimum(np.maximum(v, F32(0)), F32(1)) * F32(255)).astype(np.int64)


def sample_levels(x: np.ndarray, gray) -> np.ndarray:
    """int64 [N][3][H][W]: the level of every value; a grey sample's three channels all hold the level of its luma."""
    x = np.asarray(x, dtype=F32)
    q = level(x)
    g = np.asarray(gray).astype(bool)
    if g.any():
        q[g] = level(luma(x[g]))[:, None]
    return q


def level_masks(x: np.ndarray, scale, gray) -> np.ndarray:
    """int32 [N][8]: bit q of sample n's 256-bit mask is set when some value of it has level q; empty where scale is 0."""
    q = sample_levels(x, gray)
    out = np.zeros((q.shape[0], 8), dtype=np.uint32)
    for n in range(q.shape[0]):
        if float(np.asarray(scale)[n]) == 0.0:
            continue
        for lv in np.unique(q[n]):
            out[n, lv >> 5] |= np.uint32(1 << (lv & 31))
    return out.view(np.int32)


def vals_of(masks: np.ndarray) -> np.ndarray:
    """int64 [N]: the number of set bits of each mask rounded up to a power of two (an empty mask: 1)."""
    count = np.array([sum(bin(int(w)).count('1') for w in row.view(np.uint32)) for row in np.asarray(masks, dtype=np.int32)])
    return np.array([1 if c <= 1 else 1 << int(c - 1).bit_length() for c in count], dtype=np.int64)


def words(n_samples: int, h: int, w: int, seed: int) -> np.ndarray:
    """uint32 [N][3][H][W]: Philox4x32-10, counter (p, n, 1, 0), key (seed low, seed high); word c for channel c."""
    p = np.arange(h * w, dtype=np.uint64)[None, :]
    n = np.arange(n_samples, dtype=np.uint64)[:, None]
    r = philox4x32_10((p, n, 1, 0), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(r[:3], 1).reshape(n_samples, 3, h, w)


def draws(x: np.ndarray, scale, gray, seed: int):
    """``(k, q, vals)``: the integer draw of every value (int64 [N][3][H][W]; 0 where scale is 0), its level, and int64 [N].
    The smallest k with (r >> 1) < T[level][k], from the full rows of ``poisson_thresholds``."""
    from torchsr_amd.degradation import poisson_thresholds
    x = np.asarray(x, dtype=F32)
    n_s, _, h, w = x.shape
    q = sample_levels(x, gray)
    vals = vals_of(level_masks(x, scale, gray))
    r = words(n_s, h, w, seed)
    g = np.asarray(gray).astype(bool)
    r[g] = r[g][:, :1]                                   # word 0 feeds all three channels
    u = (r >> np.uint32(1)).astype(np.int64)
    k = np.zeros(q.shape, dtype=np.int64)
    for n in range(n_s):
        if float(np.asarray(scale)[n]) == 0.0:
            continue
        t = poisson_thresholds(int(vals[n])).astype(np.int64)
        for lv in np.unique(q[n]):
            at = q[n] == lv
            k[n][at] = np.searchsorted(t[lv], u[n][at], side='right')   # the number of thresholds <= u
    return k, q, vals


def result64(x: np.ndarray, scale, k, q, vals) -> np.ndarray:
    """float64 ``x + scale (k / vals - q / 255)``."""
    sc = np.asarray(scale, dtype=np.float64)[:, None, None, None]
    vv = np.asarray(vals, dtype=np.float64)[:, None, None, None]
    return np.asarray(x, dtype=np.float64) + sc * (k / vv - q / 255.0)


def result_bound(x: np.ndarray, scale, k, q, vals) -> np.ndarray:
    """Elementwise bound of |device - result64| with u = 2^-24, half an ulp relative.  The kernel computes t = fl(q * c) with
    c = fl(1 / 255): c is off by at most u / 255 and the product is rounded once, so |t - q / 255| <= 2 u q / 255 (q / 255 <= 1).
    d = fl(k / vals - t), k / vals exact: one more rounding, u |d|.  out = fl(scale d + x), one fma: u |out|.  Together
    u (|scale| (2 q / 255 + |d|) + |out|); the factor 1 + 2^-20 covers the products of two such terms."""
    u = 2.0 ** -24
    sc = np.abs(np.asarray(scale, dtype=np.float64))[:, None, None, None]
    d = np.abs(k / np.asarray(vals, dtype=np.float64)[:, None, None, None] - q / 255.0)
    return u * (sc * (2.0 * q / 255.0 + d) + np.abs(result64(x, scale, k, q, vals))) * (1.0 + 2.0 ** -20)


def recover_k(out, x, scale, q, vals) -> np.ndarray:
    """int64: ``rint((out - x) / scale * vals + q * vals / 255)`` in float64, samples with scale 0 give 0."""
    sc = np.asarray(scale, dtype=np.float64)[:, None, None, None]
    vv = np.asarray(vals, dtype=np.float64)[:, None, None, None]
    safe = np.where(sc == 0, 1.0, sc)
    k = np.rint((np.asarray(out, dtype=np.float64) - np.asarray(x, dtype=np.float64)) / safe * vv + q * vv / 255.0)
    return np.where(sc == 0, 0, k).astype(np.int64)


def exact_thresholds(level_: int, vals: int, n_k: int, bits: int = 31):
    """``floor(CDF(k) 2^bits)`` for k = 0 .. n_k - 1 of Poisson(level * vals / 255) as Python ints, with 80-digit decimals on the
    rational lambda: pmf(k) = exp(-lambda) lambda^k / k!."""
    with decimal.localcontext() as ctx:
        ctx.prec = 80
        lam = decimal.Decimal(level_ * vals) / decimal.Decimal(255)
        term = (-lam).exp()
        cdf, out = decimal.Decimal(0), []
        for k in range(n_k):
            if k:
                term = term * lam / k
            cdf += term
            out.append(int((cdf * (1 << bits)).to_integral_value(rounding=decimal.ROUND_FLOOR)))
        return out


# ------------------------------------------------------------------------------------------------------------ test images
# 64 (r, g, b) grey levels, found by a search over all 256^3: the level of the float32 luma, rounded after every operation,
# differs from the level under BOTH contracted forms of ``wrong_lumas`` (and for 24 of them from the re-ordered sum's too)
GREY_TRIPLES = (
    (1, 39, 222), (3, 11, 89), (15, 51, 27), (15, 75, 35), (16, 196, 76), (18, 40, 67), (23, 7, 101), (25, 29, 193),
    (27, 21, 150), (30, 18, 26), (30, 104, 13), (30, 106, 222), (30, 114, 58), (30, 120, 185), (30, 134, 148), (30, 148, 111),
    (32, 218, 219), (34, 22, 30), (35, 25, 240), (38, 12, 71), (39, 195, 91), (41, 21, 201), (44, 90, 101), (46, 34, 42),
    (51, 221, 66), (51, 241, 156), (53, 105, 237), (53, 133, 163), (58, 170, 12), (63, 23, 133), (67, 21, 10), (70, 58, 66),
    (76, 22, 183), (81, 175, 154), (95, 21, 112), (99, 97, 140), (104, 98, 227), (104, 160, 206), (110, 30, 0), (114, 22, 250),
    (117, 135, 248), (120, 80, 190), (123, 21, 214), (125, 75, 150), (127, 125, 168), (129, 183, 22), (132, 196, 70),
    (134, 170, 146), (136, 90, 79), (141, 23, 60), (146, 92, 253), (151, 143, 65), (155, 105, 180), (157, 189, 251),
    (161, 63, 170), (162, 192, 47), (165, 205, 95), (170, 220, 145), (179, 61, 98), (180, 230, 155), (184, 70, 21), (186, 98, 240),
    (189, 147, 50), (194, 58, 232))


def grey_triples_image() -> np.ndarray:
    """float32 [1][3][8][8]: pixel i holds ``GREY_TRIPLES[i] / 255``."""
    return (np.array(GREY_TRIPLES, dtype=np.float64).T.reshape(1, 3, 8, 8) / 255).astype(F32)


def level_images():
    """The inputs of the levels and draws tests: ``{name: (x float32 [N][3][H][W], scale float32 [N], gray int32 [N], seed)}``.
    Scales are powers of two and small integers' ratios of them, far above where recover_k could be ambiguous."""
    rng = np.random.RandomState(11)
    cases = {}
    # one sample, constant: one level, vals 1
    cases['constant-8x8'] = (np.full((1, 3, 8, 8), 77 / 255, dtype=F32), np.array([0.5], dtype=F32), np.array([0], dtype=np.int32), 5)
    # odd sizes, three samples: random levels; a grey sample; a sample that is copied
    x = (rng.randint(0, 256, (3, 3, 17, 29)) / 255).astype(F32)
    cases['odd-17x29'] = (x, np.array([1.0, 0.75, 0.0], dtype=F32), np.array([0, 1, 0], dtype=np.int32), (7 << 32) | 9)
    # exactly 128 and exactly 129 distinct levels: vals 128 and 256
    a = np.resize(np.arange(128) * 2, 3 * 24 * 24).reshape(3, 24, 24)
    b = np.resize(np.concatenate([np.arange(128) * 2, [255]]), 3 * 24 * 24).reshape(3, 24, 24)
    cases['128-and-129-levels'] = ((np.stack([a, b]) / 255).astype(F32), np.array([2.0, 3.0], dtype=F32),
                                   np.array([0, 0], dtype=np.int32), 1 << 63)
    # values just outside [0, 1] and at k + 0.5 grey levels (rint goes to the even level; float32 decides which side a tie is on)
    edge = np.concatenate([[-1e-3, -1e-8, 0.0, 1.0, 1.0 + 1e-7, 1.5, -5.0], (np.arange(40) + 0.5) / 255, (np.arange(200, 255) + 0.5) / 255])
    e = np.resize(edge, 2 * 3 * 8 * 8).reshape(2, 3, 8, 8).astype(F32)
    e[1] = e[1, :, ::-1].copy()
    cases['edges-8x8'] = (e, np.array([0.25, 1.5], dtype=F32), np.array([0, 1], dtype=np.int32), 123456789)
    # a grey sample on which a contracted or re-ordered luma gets another level at EVERY pixel (test_poisson_cpu.py asserts it)
    cases['grey-triples-8x8'] = (grey_triples_image(), np.array([1.0], dtype=F32), np.array([1], dtype=np.int32), 424242)
    return cases


def cycle_image() -> np.ndarray:
    """float32 [1][3][128][128]: the levels 0..255 in turn, 192 values on each."""
    return (np.resize(np.arange(256), 3 * 128 * 128).reshape(1, 3, 128, 128) / 255).astype(F32)


CYCLE_SEED = 20240607


def cycle_draws():
    x = cycle_image()
    k, q, vals = draws(x, [1.0], [0], CYCLE_SEED)
    assert vals.tolist() == [256] and (np.bincount(q.reshape(-1), minlength=256) == 192).all()
    return k, q, vals


def moment_scores(k, q, vals=256):
    """Pooled over every draw, in standard errors: the mean of k - lambda (variance lambda each), and the mean of
    (k - lambda)^2 / lambda over lambda > 0 less 1 (variance 2 + 1 / lambda each: the fourth central moment of a Poisson variable
    is 3 lambda^2 + lambda)."""
    lam = q.astype(np.float64) * 256 / 255
    d = k.astype(np.float64) - lam
    z_mean = d.sum() / np.sqrt(lam.sum())
    pos = lam > 0
    z_var = (d[pos] ** 2 / lam[pos] - 1.0).sum() / np.sqrt((2.0 + 1.0 / lam[pos]).sum())
    return float(z_mean), float(z_var), lam
