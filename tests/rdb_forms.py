"""Every calling form of the fused dense block (rdb.hip): rdb_kernel<0> / <1> through srx_rdb_fwd, srx_rdb_bwd and srx_rdb_fwd_dbg,
on the weight streams of srx_rdb_pack / srx_rdb_pack_bwd (rdb_pack_kernel).

Data only, and the float64 restatement of the block both test files share -- no GPU code.  test_rdb_forms_cpu.py holds every case to
the condition that makes its integer operands exact in fp32 (without a GPU); test_rdb_forms_gpu.py runs the launches: equal to the
restatement on integers, inside a derived elementwise bound of it on random data.

The block (8 x 8 pixel tiles, a 5-pixel halo recomputed in LDS on regions 16, 14, 12 and 10 pixels wide):

  forward   c_k = LeakyReLU(conv_k(bf16(cat(x, c_1..c_{k-1}))) + b_k), k = 1..4, kept in fp32 and rounded to bf16 where read again;
            out = (conv_5(bf16(cat(x, c_1..c_4))) + b_5) * scale + x   [then  * post_scale + extra  where `extra` is given]
  backward  g_5 = bf16(scale * dy);  g_j = (c_j > 0 ? a_j : a_j * slope),  a_j = sum_{k > j} conv_k^T(bf16(g_k))[c_j], j = 4..1, kept in
            fp32;  dx = sum_k conv_k^T(bf16(g_k))[x] + skip_scale * skip  [+ extra]

Weights are rounded to bf16 by the pack.  Every sum below is a float64 convolution of bf16 numbers: exact for the integer operands,
and for random data further from the true sum than any fp32 accumulation is allowed to be by a factor of 2^-29.

The integer operands (int_operands): x, dy, extra in {-1, 0, 1}, skip in [-3, 3], saved activations in [-2, 2] (a fifth exact zeros:
the c > 0 edge), weights in {-1, 0, 1} with a fraction DENSITY non-zero, biases in [-2, 2]; slope 2 (or 0: a ReLU), scale = post_scale
= skip_scale = 1/2.  Every value is then a whole number of quarters, and wherever the per-element sum of magnitudes |a| conv |w| + |b|
times 4 stays below 2^24 (assert_exact, asserted for every case) every fp32 partial sum of every stage is exact IN ANY ORDER: the
device result must EQUAL the restatement.  c_4 reaches tens of thousands, so most of it is not a bf16 number: the kernel's
round-to-nearest-even, ties included, is compared with torch's wherever a stage output is read again."""
import functools
import zlib

TILE, HALO = 8, 5
CUS = 256

# (N, H, W) -> what the shape is in the table for
SHAPES = {
    (1, 1, 1): 'everything but one pixel lies outside the image',
    (1, 8, 8): 'one whole tile: the entire halo is zero padding',
    (1, 9, 8): 'a second tile that holds one row',
    (1, 8, 9): 'a second tile that holds one column',
    (1, 13, 21): 'ragged in both axes',
    (1, 5, 40): 'narrower than the halo, five tiles in a row',
    (3, 24, 24): '27 workgroups (not a multiple of 8); tile (1, 1) has its whole halo inside the image; three images',
    (1, 16, 64): '16 workgroups: the XCD renumbering with two tiles per XCD, tiles_x = 8',
    (2, 16, 32): '16 workgroups: the renumbering across an image boundary',
    (65, 16, 16): '260 workgroups, more than the 256 CUs; a large image index',
}
CHAIN_SHAPE = (2, 16, 16)        # three blocks out of one pack, as functional._DenseBlock runs an RRDB
VARIANTS = {'lrelu': 2.0, 'relu': 0.0}   # slope on integers: LeakyReLU that stays on integers; ReLU (half the values exact zeros)
SCALE = POST_SCALE = SKIP_SCALE = 0.5
DENSITY = 1.0 / 8                # non-zero weights of a single block
# ... of the three-block chain: a block's output is the next one's input, so the magnitudes multiply block by block (with slope 2
# about a hundredfold per block at 1/8) and the scales halve the unit twice more: sixteenths.  Densities at which the third block's
# largest sum of magnitudes, in sixteenths, is still a factor of 8 below 2^24 (test_rdb_forms_cpu.py asserts the condition itself)
CHAIN_DENSITY = {'lrelu': 1.0 / 192, 'relu': 1.0 / 64}
EXACT = 1 << 24                  # below it every integer is an fp32 number
QUARTERS, SIXTEENTHS = 4, 16

# the operand scales of the random-data cases: those of test_ops_gpu.py::test_fused_dense_block_forward / _backward
RANDOM_FWD = dict(scale=0.2, slope=0.2, post_scale=0.7)
RANDOM_BWD = dict(scale=0.2 * 0.7, slope=0.2, skip_scale=0.9)

# forward calling forms: strides (block buffer, out, extra or None), post_scale, and what the channels past the tensors hold
FWD_FORMS = {
    'a': dict(ld=192, out_ld=192, extra_ld=None, why='middle of an RRDB: no addend, out = the next block buffer'),
    'b': dict(ld=192, out_ld=192, extra_ld=192, why="end of an RRDB: extra = an older block buffer's x channels"),
    'c': dict(ld=192, out_ld=64, extra_ld=192, why='last block of the trunk: a dense 64-channel result'),
    'd': dict(ld=200, out_ld=68, extra_ld=72, why='slack in every stride'),
}
BWD_FORMS = {
    'product': dict(dy_ld=64, skip_ld=64, dx_ld=64, extra_ld=None, ld=192, gld=192),
    'product+extra': dict(dy_ld=64, skip_ld=64, dx_ld=64, extra_ld=64, ld=192, gld=192),
    'slack': dict(dy_ld=72, skip_ld=68, dx_ld=76, extra_ld=80, ld=200, gld=196),
}


def shape_id(shape):
    return 'x'.join(map(str, shape))


def workgroups(shape):
    n, h, w = shape
    return n * (-(-h // TILE)) * (-(-w // TILE))


def conv_cin(k):
    """input channels of conv k (1..5)"""
    return 64 + 32 * (k - 1)


def conv_cout(k):
    return 64 if k == 5 else 32


# ------------------------------------------------------------------------------------------------------------------- operands
def _rng(tag):
    import numpy as np
    return np.random.default_rng(zlib.crc32(tag.encode()))


def int_weights(tag, density=DENSITY):
    """Five OIHW weights in {-1, 0, 1} (each entry non-zero with probability ``density``) and five integer biases in [-2, 2]."""
    import numpy as np
    import torch
    rng = _rng('rdb weights ' + tag)
    ws, bs = [], []
    for k in range(1, 6):
        shp = (conv_cout(k), conv_cin(k), 3, 3)
        sign = 2 * rng.integers(0, 2, shp, dtype=np.int8) - 1
        ws.append(torch.from_numpy((sign * (rng.random(shp) < density)).astype(np.float32)))
        bs.append(torch.from_numpy(rng.integers(-2, 3, (conv_cout(k),)).astype(np.float32)))
    return ws, bs


def int_operands(shape, density=DENSITY):
    """The integer operands of a shape's exact checks, NCHW fp32 tensors: ws, bs (int_weights), x, dy, extra in {-1, 0, 1}, skip in
    [-3, 3], acts (192 channels: x, c1..c4 as a forward pass would have left them; integers in [-2, 2], a fifth of them 0)."""
    import numpy as np
    import torch
    n, h, w = shape
    ws, bs = int_weights(shape_id(shape), density)
    rng = _rng('rdb data ' + shape_id(shape))
    t = lambda lo, hi, c: torch.from_numpy(rng.integers(lo, hi + 1, (n, c, h, w)).astype(np.float32))  # noqa: E731
    return dict(ws=ws, bs=bs, x=t(-1, 1, 64), dy=t(-1, 1, 64), extra=t(-1, 1, 64), skip=t(-3, 3, 64), acts=t(-2, 2, 192))


def random_operands(shape):
    """The distributions of test_ops_gpu.py's two dense-block tests: normal data, Kaiming weights, biases of 0.1."""
    import torch
    n, h, w = shape
    g = torch.Generator().manual_seed(zlib.crc32(('rdb random ' + shape_id(shape)).encode()))
    ws = [torch.randn(conv_cout(k), conv_cin(k), 3, 3, generator=g) * (2.0 / (9 * conv_cin(k))) ** 0.5 for k in range(1, 6)]
    bs = [torch.randn(conv_cout(k), generator=g) * 0.1 for k in range(1, 6)]
    t = lambda c: torch.randn(n, c, h, w, generator=g)  # noqa: E731
    return dict(ws=ws, bs=bs, x=t(64), dy=t(64), extra=t(64), skip=t(64), acts=t(192))


# ------------------------------------------------------------------------------------------------------- the float64 restatement
def r16(t):
    """fp32 -> bf16 (round to nearest even) -> float64: what the kernel's (__bf16) conversions and the pack leave of an operand"""
    import torch
    assert t.dtype == torch.float32
    return t.to(torch.bfloat16).double()


def _conv(a, w, bias=None):
    import torch.nn.functional as TF
    return TF.conv2d(a, w, bias, 1, 1)


def fwd_stage(k, feats, w, b, slope):
    """Stage k = 1..4 of the forward on the fp32 sources ``feats`` = [x, c_1, .., c_{k-1}]: (c_k, its pre-activation, the
    magnitude term |a| conv |w| + |b|), all float64."""
    import torch
    a, wr = r16(torch.cat(feats, 1)), r16(w)
    z = _conv(a, wr, b.double())
    mag = _conv(a.abs(), wr.abs(), b.double().abs())
    return torch.where(z > 0, z, z * slope), z, mag


def fwd_last(feats, w, b, scale, x):
    """The last stage without the second addend: ((conv_5 + b_5) * scale + x, the magnitude term of the conv and its bias)."""
    import torch
    a, wr = r16(torch.cat(feats, 1)), r16(w)
    return _conv(a, wr, b.double()) * scale + x.double(), _conv(a.abs(), wr.abs(), b.double().abs())


def forward64(x, ws, bs, scale, slope, given=None):
    """The whole forward.  ``given`` (random data): the device's own c_1..c_4 (fp32), which then are the sources of the later stages --
    an intermediate one fp32 ulp from its float64 value may round to the other bf16 neighbour, which is no error of the kernel.
    Without it (integers) the chain feeds on itself alone.  Returns dict: c (four float64), pre (four pre-activations), y0 (the output
    without the second addend), mag (five magnitude terms)."""
    feats, cs, pres, mags = [x], [], [], []
    for k in range(1, 5):
        c, z, mag = fwd_stage(k, feats, ws[k - 1], bs[k - 1], slope)
        cs.append(c); pres.append(z); mags.append(mag)
        feats.append(given[k - 1] if given is not None else c.float())
    y0, mag = fwd_last(feats, ws[4], bs[4], scale, x)
    return dict(c=cs, pre=pres, y0=y0, mag=mags + [mag])


def fwd_out(y0, post_scale=None, extra=None):
    """out of a forward call: y0, or y0 * post_scale + extra where the call has the second addend"""
    return y0 if extra is None else y0 * post_scale + extra.double()


def _wT(w, lo, hi):
    """The filter whose plain convolution is conv^T[input channels lo:hi]: transposed, taps flipped, bf16-rounded"""
    return r16(w)[:, lo:hi].transpose(0, 1).flip(2, 3).contiguous()


def backward64(dy, acts, ws, scale, slope, skip, skip_scale, extra=None, given=None):
    """The data-gradient chain.  ``given``: the device's own {4: g_4, .., 1: g_1} (fp32) as the sources of the later stages (random
    data).  Returns dict: g ({j: float64}), dx, mag ({j: .., 0: dx's} -- every source of a stage goes through one accumulator: the
    sum over the sources of |g_k| conv |w_k^T|; dx's includes skip_scale |skip| and |extra|)."""
    import torch
    gs = {5: dy * scale}                 # fp32, one rounding: as the kernel forms it before the bf16 conversion
    assert gs[5].dtype == torch.float32
    out, mags = {}, {}
    for j in (4, 3, 2, 1):
        lo = 64 + 32 * (j - 1)
        a = sum(_conv(r16(gs[k]), _wT(ws[k - 1], lo, lo + 32)) for k in range(j + 1, 6))
        mags[j] = sum(_conv(r16(gs[k]).abs(), _wT(ws[k - 1], lo, lo + 32).abs()) for k in range(j + 1, 6))
        out[j] = torch.where(acts[:, lo:lo + 32] > 0, a, a * slope)
        gs[j] = given[j] if given is not None else out[j].float()
    dx = sum(_conv(r16(gs[k]), _wT(ws[k - 1], 0, 64)) for k in range(1, 6)) + skip_scale * skip.double()
    mags[0] = sum(_conv(r16(gs[k]).abs(), _wT(ws[k - 1], 0, 64).abs()) for k in range(1, 6)) + skip_scale * skip.double().abs()
    if extra is not None:
        dx = dx + extra.double()
        mags[0] = mags[0] + extra.double().abs()
    return dict(g=out, dx=dx, mag=mags)


# ------------------------------------------------------------------- the rounding chains of the random-data bound, from rdb.hip
# gamma_k (|a| conv |w| + ..) with k = the fp32 roundings between the exact bf16 x bf16 products and the stored value, each counted at
# the line of rdb.hip that makes it (as step_layers.wino_k does for wino.hip).
def fwd_k(K):
    """forward stage K = 1..4 (epilogue_mid<K, false>)"""
    return (9 * conv_cin(K)      # mma_group: the MFMAs' accumulation of 9 taps x (64 + 32 (K - 1)) channels, in any order
            + 1                  # z = w.acc[i][..] + b[g][e]
            + 1)                 # z * a.slope


def out_k(extra):
    """the forward's last stage (epilogue_out<false>)"""
    return (9 * conv_cin(5)      # mma_group: 9 x 192 products
            + 1                  # w.acc[0][..] + b[e]
            + 1                  # (..) * a.scale
            + 1                  # + xs[g][e]
            + (2 if extra else 0))   # v * a.post_scale; + ex[g]


def bwd_k(j):
    """the backward stage that produces g_j, j = 4..1 (epilogue_mid<5 - j, true>): its 2 + (4 - j) sources of 32 channels -- g_5 as
    two, g_4 .. g_{j+1} -- go through one accumulator"""
    return (9 * 32 * (2 + 4 - j)     # mma_group over every unit of the stage
            + 1)                     # w.acc[i][..] * a.slope


def dx_k(extra):
    """the backward's last stage (epilogue_out<true>)"""
    return (9 * 32 * 6               # six sources: g_5 (two), g_4 .. g_1
            + 1                      # a.skip_scale * xs[g][e]
            + 1                      # w.acc[0][..] + (..)
            + (1 if extra else 0))   # v += ex[g]


# -------------------------------------------------------------------------------------------- the chain of functional._DenseBlock
def chain_forward64(x, blocks, rdb_scale, slope, rrdb_scale):
    """One RRDB as _DenseBlock.forward launches it: block i reads buffer i (x_i, c_1..c_4) and writes x_{i+1} into buffer i + 1; the
    third block takes the first buffer's x as its second addend with post_scale = rrdb_scale.  Returns (per block forward64 dicts,
    the fp32 buffers [x_i, c_1..c_4 as 192 channels], the output float64)."""
    import torch
    res, bufs = [], []
    xi = x
    for i, (ws, bs) in enumerate(blocks):
        r = forward64(xi, ws, bs, rdb_scale, slope)
        out = fwd_out(r['y0'], rrdb_scale, x) if i == 2 else r['y0']
        r['out'] = out
        r['out_mag'] = (r['mag'][4] * rdb_scale + xi.double().abs()) * (rrdb_scale if i == 2 else 1.0) + (x.double().abs() if i == 2 else 0.0)
        res.append(r)
        bufs.append(torch.cat([xi] + [c.float() for c in r['c']], 1))
        xi = out.float()
    return res, bufs, out


def chain_backward64(dy, bufs, blocks, rdb_scale, slope, rrdb_scale):
    """... and _DenseBlock.backward, last block first: the third block sees rrdb_scale of the RRDB's output gradient (scale =
    rrdb_scale * rdb_scale, skip_scale = rrdb_scale), the first adds the RRDB's own skip gradient as `extra`.  Returns the per-block
    backward64 dicts (index = block) and their call arguments."""
    grad, res, args = dy, [None] * 3, [None] * 3
    for i in (2, 1, 0):
        eff = rrdb_scale if i == 2 else 1.0
        a = dict(dy=grad, scale=eff * rdb_scale, skip=grad, skip_scale=eff, extra=dy if i == 0 else None)
        res[i] = backward64(grad, bufs[i], blocks[i][0], a['scale'], slope, grad, eff, a['extra'])
        args[i] = a
        grad = res[i]['dx'].float()
    return res, args


def chain_operands(variant):
    """Three blocks of different integer weights (CHAIN_DENSITY[variant]), x and dy in {-1, 0, 1}"""
    import numpy as np
    import torch
    n, h, w = CHAIN_SHAPE
    blocks = [int_weights('chain block %d' % i, CHAIN_DENSITY[variant]) for i in range(3)]
    rng = _rng('rdb chain data')
    t = lambda: torch.from_numpy(rng.integers(-1, 2, (n, 64, h, w)).astype(np.float32))  # noqa: E731
    return dict(blocks=blocks, x=t(), dy=t())


# --------------------------------------------------------------------------------------------------- the condition of exactness
def quantum(*tensors):
    """The largest power of two q <= 1 of which every element of the (float64) tensors is a whole multiple"""
    q = 1.0
    for t in tensors:
        while not bool((t / q == (t / q).round()).all()):
            q /= 2
            assert q >= 2.0 ** -20
    return q


def assert_exact(what, mag, *values, per=QUARTERS):
    """The condition of the exact tests, for one stage: every term and result is a whole number of 1 / ``per`` and the per-element sum
    of magnitudes (the largest value any partial sum, in any order, can reach) times ``per`` is below 2^24 -- so every partial sum is
    an integer count of 1 / per below 2^24: an fp32 number.  Returns the largest sum of magnitudes."""
    worst = float(mag.max())
    assert 1.0 / quantum(mag, *values) <= per, (what, 'not whole multiples of 1 /', per)
    assert worst * per < EXACT, (what, 'sum of magnitudes', worst, 'x', per, '>= 2^24')
    return worst


# ------------------------------------------------------------------------------------ the exact references, condition included
@functools.lru_cache(maxsize=None)
def exact_forward(shape, variant):
    """The float64 forward of a shape's integer operands, computed on the CPU alone, with the condition of exactness asserted for
    every stage.  dict: c (four), y0 (no second addend), out (with post_scale and extra), worst (five largest sums of magnitudes)."""
    ops, slope = int_operands(shape), VARIANTS[variant]
    r = forward64(ops['x'], ops['ws'], ops['bs'], SCALE, slope)
    tag = 'forward %s %s ' % (shape_id(shape), variant)
    out = fwd_out(r['y0'], POST_SCALE, ops['extra'])
    worst = [assert_exact(tag + 'conv%d' % k, r['mag'][k - 1], r['c'][k - 1], r['pre'][k - 1]) for k in range(1, 5)]
    worst.append(assert_exact(tag + 'conv5', r['mag'][4], r['y0'], out))
    return dict(c=r['c'], y0=r['y0'], out=out, worst=worst)


@functools.lru_cache(maxsize=None)
def exact_backward(shape, variant):
    """... and of the data-gradient chain.  dict: g ({4..1}), dx (with extra), dx0 (without), worst ({4..1, 0: dx})."""
    ops, slope = int_operands(shape), VARIANTS[variant]
    r = backward64(ops['dy'], ops['acts'], ops['ws'], SCALE, slope, ops['skip'], SKIP_SCALE, ops['extra'])
    tag = 'backward %s %s ' % (shape_id(shape), variant)
    dx0 = r['dx'] - ops['extra'].double()
    worst = {j: assert_exact(tag + 'g%d' % j, r['mag'][j], r['g'][j]) for j in (4, 3, 2, 1)}
    worst[0] = assert_exact(tag + 'dx', r['mag'][0], r['dx'], dx0)
    return dict(g=r['g'], dx=r['dx'], dx0=dx0, worst=worst)


@functools.lru_cache(maxsize=None)
def exact_chain(variant):
    """The three-block chain forward and backward on chain_operands(variant), exact in sixteenths.  dict: ops, fwd (per block:
    forward64's dict + out), bufs (the three fp32 block buffers, 192 channels), out, bwd (per block: backward64's dict), bwd_args
    (per block: dy, scale, skip, skip_scale, extra of the call), worst (the largest sum of magnitudes of all)."""
    ops, slope = chain_operands(variant), VARIANTS[variant]
    fwd, bufs, out = chain_forward64(ops['x'], ops['blocks'], SCALE, slope, POST_SCALE)
    bwd, args = chain_backward64(ops['dy'], bufs, ops['blocks'], SCALE, slope, POST_SCALE)
    worst = 0.0
    for i in range(3):
        tag = 'chain %s block %d ' % (variant, i)
        for k in range(1, 5):
            worst = max(worst, assert_exact(tag + 'conv%d' % k, fwd[i]['mag'][k - 1], fwd[i]['c'][k - 1], fwd[i]['pre'][k - 1], per=SIXTEENTHS))
        worst = max(worst, assert_exact(tag + 'conv5', fwd[i]['mag'][4], per=SIXTEENTHS))
        worst = max(worst, assert_exact(tag + 'out', fwd[i]['out_mag'], fwd[i]['y0'], fwd[i]['out'], per=SIXTEENTHS))
        for j in (4, 3, 2, 1):
            worst = max(worst, assert_exact(tag + 'g%d' % j, bwd[i]['mag'][j], bwd[i]['g'][j], per=SIXTEENTHS))
        worst = max(worst, assert_exact(tag + 'dx', bwd[i]['mag'][0], bwd[i]['dx'], per=SIXTEENTHS))
    return dict(ops=ops, fwd=fwd, bufs=bufs, out=out, bwd=bwd, bwd_args=args, worst=worst)
