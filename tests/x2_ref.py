"""What the x2 training tests share: the torch restatement of RRDBNet's x2 input layer and its weight gradient in fp64, the
launch plan of ``srx_unshuffle2_conv_bwd_weight`` through the C ABI, and the seeded operands -- each computed once."""
import ctypes as C
import functools

import torch
import torch.nn.functional as TF

# (N, H, W) of the image: one partial segment; Wo exactly 16 and two images; Wo = 17 (a one-column segment); both axes odd (the
# reflected row and column) and the minimum; odd H with three segments a row; two sizes with several slabs and several segments a
# range, the second the GAN step's own; one whose last workgroup has empty wave ranges
SHAPES = [(1, 4, 4), (2, 8, 32), (1, 6, 34), (1, 7, 9), (1, 3, 3), (2, 5, 66), (4, 64, 64), (16, 64, 64), (2, 10, 34)]
STEP_SHAPES = [(4, 64, 64), (16, 64, 64)]
RAGGED_SHAPE = (2, 10, 34)


def unshuffled(x):
    """[N,3,H,W] -> [N,12,Hp/2,Wp/2]: an odd axis padded by one reflected row / column at the bottom / right, pixel_unshuffle(2)."""
    h, w = x.shape[-2:]
    return TF.pixel_unshuffle(TF.pad(x, (0, w & 1, 0, h & 1), mode='reflect'), 2)


def layer(x, weight, bias):
    return TF.conv2d(unshuffled(x), weight, bias, 1, 1)


def out_hw(h, w):
    return (h + 1) // 2, (w + 1) // 2


def wgrad_fp64(x, dy):
    """The weight gradient [64,12,3,3] of ``layer`` for ``x`` [N,3,H,W] and ``dy`` [N,64,Ho,Wo], by fp64 autograd."""
    w = torch.zeros(64, 12, 3, 3, dtype=torch.float64, requires_grad=True)
    (layer(x.double(), w, None) * dy.double()).sum().backward()
    return w.grad


@functools.lru_cache(maxsize=None)
def operands(shape, kind):
    """``(x [N,3,H,W], dy [N,64,Ho,Wo], dw fp64)``: ``kind`` 'int' -- integers in [-3, 3], so that every partial sum of the largest
    shape (16 * 32 * 32 products of at most 9) stays below 2^24 and fp32 is exact in any order -- or 'rand' (uniform in [-1, 1])."""
    n, h, w = shape
    ho, wo = out_hw(h, w)
    g = torch.Generator().manual_seed(1000 * n + 10 * h + w + (7 if kind == 'int' else 0))
    if kind == 'int':
        x = torch.randint(-3, 4, (n, 3, h, w), generator=g).float()
        dy = torch.randint(-3, 4, (n, 64, ho, wo), generator=g).float()
    else:
        x = torch.rand((n, 3, h, w), generator=g) * 2 - 1
        dy = torch.rand((n, 64, ho, wo), generator=g) * 2 - 1
    return x, dy, wgrad_fp64(x, dy)


def nhwc(x, cs):
    """cpu NCHW -> cpu NHWC with ``cs`` stored channels, the padding 0."""
    n, c, h, w = x.shape
    y = torch.zeros(n, h, w, cs, dtype=x.dtype)
    y[..., :c] = x.permute(0, 2, 3, 1)
    return y.contiguous()


def plan(shape):
    """``{segments, ranges, segs_per_range, slabs, groups}`` of ``srx_unshuffle2_conv_wgrad_plan``."""
    from torchsr_amd import _lib
    out = (C.c_int * 8)()
    _lib.call('srx_unshuffle2_conv_wgrad_plan', *shape, out)
    return dict(zip(('segments', 'ranges', 'segs_per_range', 'slabs', 'groups'), list(out)[:5]))


def ws_floats(shape):
    from torchsr_amd import _lib
    return int(_lib.lib().srx_unshuffle2_conv_wgrad_ws_floats(*shape))


def rel_l2(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert bool(torch.isfinite(got).all())
    return ((got - want).norm() / want.norm().clamp_min(1e-300)).item()
