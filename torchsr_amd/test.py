"""Single-image 4x upscaling -- the ``torchsr test <image>`` path (torchsr/test.py:22-63).

The reference's function cannot run as shipped (it iterates the outer checkpoint dict and leaves
``name`` unbound for keys without the ``module.`` prefix).  This is the intended
behaviour: load ``{model}-gan-best.pth`` (``{"epoch","phase","state"}`` or a bare state_dict, with or
without DDP's ``module.`` prefix), run the generator in eval mode without autograd, write
``upres-<image>``.

Large images (BASELINE config 5: 1080p -> 8K) are processed in spatial tiles with a halo: the
generator is fully convolutional and, in eval mode, BatchNorm is a per-channel affine map, so a tile
whose halo covers the receptive field reproduces the untiled result exactly while every conv call
stays below the kernels' 2^24-pixel / 2^31-element addressing limits.  That holds for SRGAN, whose
receptive field radius is < 40 low-resolution pixels (``Generator.halo`` = 48).  RRDBNet's is ~350 pixels
(69 dense blocks of five 3x3 convs), more than a tile can carry: ESRGAN tiles use a 64-pixel halo and
are an approximation near tile borders (the dense blocks' 0.2 residual scaling makes far pixels count
little); pass ``halo=`` / ``max_tile_pixels=`` to trade time for accuracy.
"""
import os
from argparse import Namespace
from collections import OrderedDict

import torch
from torch import Tensor

from .rrdbnet import generator_to_rrdbnet_state, rrdbnet_geometry, rrdbnet_to_generator_state  # noqa: F401  (host code)

HALO = 48           # LR pixels: default when the generator does not name its own (``Generator.halo``)
MAX_TILE_PIXELS = 600 * 1000  # LR pixels per tile (x16 HR pixels must stay < 2^24)
TRUNK_MAX_PIXELS = 8 * 1000 * 1000  # LR pixels the staged path runs untiled (x256 floats of the sub-pixel conv < 2^31)


def load_generator_state(path: str, ema: bool = False) -> OrderedDict:
    """The generator's state_dict from a checkpoint: this package's ``{"epoch", "phase", "state"}``, Real-ESRGAN's
    ``{"params_ema": ...}`` (preferred) or ``{"params": ...}``, or a bare state_dict; DDP's ``module.`` prefix is dropped.
    ``ema`` (``test --ema``): the averaged weights ``params_ema`` -- which a checkpoint of ``train --ema-decay`` holds next to
    its live ``state`` -- or a ``RuntimeError`` that names the file's keys when it has none."""
    ckpt = torch.load(path, map_location='cpu')
    state = ckpt
    if ema and not (isinstance(ckpt, dict) and isinstance(ckpt.get('params_ema'), dict)):
        keys = sorted(map(str, ckpt))[:6] if isinstance(ckpt, dict) else type(ckpt).__name__
        raise RuntimeError(f'{path} holds no averaged weights ("params_ema"): its keys are {keys}; train with --ema-decay to '
                           'write them, or drop --ema')
    for key in (('params_ema',) if ema else ('state', 'params_ema', 'params')):
        if isinstance(ckpt, dict) and isinstance(ckpt.get(key), dict):
            state = ckpt[key]
            break
    return OrderedDict((k[len('module.'):] if k.startswith('module.') else k, v) for k, v in state.items())


def compact_num_conv(state) -> int:
    """The number of body convs of an SRVGGNetCompact state_dict: its last key is ``body.{2 num_conv + 2}.weight`` / ``.bias``."""
    idx = [int(k.split('.')[1]) for k in state if k.startswith('body.') and k.split('.')[1].isdigit()]
    if not idx or max(idx) < 4 or max(idx) % 2:
        raise RuntimeError(f'not a compact (SRVGGNetCompact) state_dict: keys {list(state)[:4]} ...')
    return (max(idx) - 2) // 2


def compact_scale(state, path: str = 'the file') -> int:
    """The scale of an SRVGGNetCompact state_dict, read off its last conv's output channels 3 s^2: 12 is x2, 48 is x4 (27, x3,
    is refused: untested here)."""
    cout = int(state[f'body.{2 * compact_num_conv(state) + 2}.weight'].shape[0])
    scale = {12: 2, 48: 4}.get(cout)
    if scale is None:
        raise RuntimeError(f'{path}: a compact (SRVGGNetCompact) state_dict whose last conv has {cout} output channels; 12 (x2) '
                           'and 48 (x4) run here' + (' (27 is x3, which is untested here)' if cout == 27 else ''))
    return scale


@torch.no_grad()
def upscale(generator: torch.nn.Module, low_res: Tensor, halo: int = None,
            max_tile_pixels: int = MAX_TILE_PIXELS, scale: int = 4, precision: str = None, staged: bool = True,
            self_ensemble: int = 0, outscale: float = None, color_fix: str = None) -> Tensor:
    """``generator(low_res)`` in eval mode, tiled when the image is large.  ``low_res``: [N,3,h,w].  ``scale``: the generator's
    factor (4; 2 for ``esrgan.Generator(scale_factor=2)``).  A generator with a ``tile_align`` attribute (that x2 net: 2) gets
    tiles whose origins, sizes and halo are multiples of it (``tile_plan``).

    ``precision``: ``'fp32'`` (exact; the reference's ``test`` runs no autocast, test.py:57-62), ``'bf16'`` (bf16
    products with fp32 accumulation in every conv but the 3-channel INPUT conv) or ``'fp16'``
    (a generator with the 16-bit-native chain -- ``Generator.native16``: SRGAN, compact -- only: fp16 products with fp32
    accumulation in every conv, the 64-channel activations stored as fp16; a non-finite output, i.e. an overflow of
    fp16's +-65504, raises ``FloatingPointError``); ``None`` keeps whatever the generator's convs are set to.  The setting
    is restored afterwards.  ``staged=False`` forces the halo tiling for a generator that offers the two-stage interface
    (``_upscale_staged``).

    ``self_ensemble``: 0 / False: off.  8 / True: the geometric self-ensemble (the "+" variants of EDSR / RCAN / ESRGAN) --
    the generator runs on the 8 flips / transposes of the image, every result is mapped back and the 8 are averaged; 4: the
    flips only (all four variants keep the input's shape).  ``n`` generator forwards, each with every other argument as
    given; no new weights.  See ``_upscale_ensemble``.

    ``outscale``: the total factor from ``low_res`` to the result.  ``None`` or ``scale``: the generator's own result, this
    path untouched.  Any other positive number: the generator still runs at x ``scale``, and its full result -- tiles or
    strips assembled, the ensemble averaged, the fp16 check passed -- is resampled ONCE to ``(int(h * outscale + 0.5),
    int(w * outscale + 0.5))`` (at least 1) with the antialiased bicubic the training data is reduced with
    (``F.resize_bicubic_aa``, csrc/resample.hip).  A reduction of the x ``scale`` result by more than 16:1 is refused.

    ``color_fix``: ``None``: off, this path untouched.  ``'wavelet'`` or ``'adain'``: the generator's full x ``scale`` result --
    assembled, averaged and checked as above -- is colour-corrected against the ORIGINAL ``low_res`` (``F.color_fix_wavelet``:
    its high frequencies on the low frequencies of the enlarged input; ``F.color_fix_adain``: every channel mapped to the
    input's mean and standard deviation; csrc/colorfix.hip), and ``outscale`` resamples that."""
    if color_fix is not None:
        from . import functional as F
        if not isinstance(color_fix, str) or color_fix not in F.COLOR_FIX_MODES:
            raise ValueError(f"upscale: color_fix must be None, 'wavelet' or 'adain', got {color_fix!r}")
        size = None if outscale is None else _outscale_size(low_res, outscale, scale)  # its refusals, too, before the generator runs
        full = upscale(generator, low_res, halo, max_tile_pixels, scale, precision, staged, self_ensemble)
        fix = F.color_fix_wavelet if color_fix == 'wavelet' else F.color_fix_adain
        full = fix(full, low_res.contiguous())
        return full if size is None else F.resize_bicubic_aa(full, size)
    if outscale is not None:
        size = _outscale_size(low_res, outscale, scale)
        if size is not None:
            from . import functional as F
            full = upscale(generator, low_res, halo, max_tile_pixels, scale, precision, staged, self_ensemble)
            return F.resize_bicubic_aa(full, size)
    if isinstance(self_ensemble, bool):
        self_ensemble = 8 if self_ensemble else 0
    if not isinstance(self_ensemble, int) or self_ensemble not in (0, 4, 8):
        raise ValueError(f'upscale: self_ensemble must be 0 / False, 4, or 8 / True, got {self_ensemble!r}')
    if self_ensemble:
        return _upscale_ensemble(generator, low_res, halo, max_tile_pixels, scale, precision, staged, self_ensemble)
    from . import _dev
    from .functional import PRECISION_F16
    from .layers import Conv2d, set_conv_precision
    generator.eval()
    if precision is not None:
        if precision not in ('fp32', 'bf16', 'fp16'):
            raise ValueError(f"upscale: precision must be 'fp32', 'bf16' or 'fp16', got {precision!r}")
        if precision == 'fp16' and (not hasattr(generator, 'native16') or _dev.NO_C64 or _dev.NO_T9):
            raise ValueError(f"upscale: precision 'fp16' needs a generator with the 16-bit-native chain (SRGAN, compact; "
                             f"{type(generator).__name__} has none) and its kernels enabled (SRX_NO_C64 / SRX_NO_T9 unset)")
        saved = [(m, m._st.precision) for m in generator.modules() if isinstance(m, Conv2d)]
        if precision == 'fp16':  # inference only: set here, never through set_conv_precision (training has no fp16)
            for m, _ in saved:
                m._st.precision = PRECISION_F16
        else:
            set_conv_precision(generator, precision)
        if precision == 'bf16':  # inference: the 64 -> 3 output conv multiplies bf16 operands too (srx_conv2d_t::precision = 2)
            for m, _ in saved:
                if m.out_channels <= 4 and m.in_channels == 64:
                    m._st.precision = 2
        try:
            out = upscale(generator, low_res, halo, max_tile_pixels, scale, None, staged)
            # fp32 and bf16 share fp32's range: a non-finite value here is an fp16 overflow.  (Every element is finite iff the
            # minimum and the maximum are -- both propagate NaN --: one reduction, where isfinite(out).all() took 0.44 ms at 8K, this 0.17.)
            if precision == 'fp16' and not bool(torch.isfinite(torch.stack(torch.aminmax(out))).all()):
                raise FloatingPointError("upscale: the fp16 result is not finite -- an activation left fp16's range "
                                         "(+-65504); use precision='bf16' or 'fp32' for this model / image")
            return out
        finally:
            for m, p in saved:
                m._st.precision = p
    if halo is None:
        halo = int(getattr(generator, 'halo', HALO))
    n, c, h, w = low_res.shape
    if n * h * w <= max_tile_pixels:
        return generator(low_res)
    if staged and hasattr(generator, 'infer_trunk_nhwc') and n * h * w <= TRUNK_MAX_PIXELS:
        return _upscale_staged(generator, low_res, max_tile_pixels * scale * scale, scale)
    _, _, _, tiles = tile_plan(h, w, halo, max_tile_pixels, int(getattr(generator, 'tile_align', 1)), n)
    out = torch.empty((n, c, h * scale, w * scale), dtype=low_res.dtype, device=low_res.device)
    for y0, y1, x0, x1, ya, yb, xa, xb in tiles:
        sr = generator(low_res[:, :, ya:yb, xa:xb].contiguous())
        out[:, :, y0 * scale:y1 * scale, x0 * scale:x1 * scale] = \
            sr[:, :, (y0 - ya) * scale:(y1 - ya) * scale, (x0 - xa) * scale:(x1 - xa) * scale]
    return out


def tile_plan(h: int, w: int, halo: int, max_tile_pixels: int, tile_align: int = 1, n: int = 1):
    """The halo tiling of an ``n`` x ``h`` x ``w`` image as a pure function: ``(th, tw, halo, tiles)`` -- the interior tile size,
    the halo used, and per tile ``(y0, y1, x0, x1, ya, yb, xa, xb)``: the interior rows / columns it owns and the rows / columns
    the generator runs on, rows outermost.  ``tile_align`` (a generator's ``tile_align``, default 1): tile height, tile width and
    halo are rounded UP to its multiples, so that every tile and every halo starts at a multiple of it -- at 2 the
    pixel-unshuffle phase of a tile is the phase of the whole image, and only a tile at the image's bottom / right edge can have
    an odd size, the image's own.  With 1 nothing is rounded."""
    def up(v):
        return -(-v // tile_align) * tile_align
    halo = up(halo)
    rows = max(1, -(-h * w * n // max_tile_pixels))
    th = up(-(-h // int(rows ** 0.5 + 0.999)))
    tw = max(1, max_tile_pixels // (n * (th + 2 * halo))) - 2 * halo
    tw = up(max(64, min(tw, w)))
    tiles = []
    for y0 in range(0, h, th):
        for x0 in range(0, w, tw):
            y1, x1 = min(h, y0 + th), min(w, x0 + tw)
            ya, xa = max(0, y0 - halo), max(0, x0 - halo)
            yb, xb = min(h, y1 + halo), min(w, x1 + halo)
            tiles.append((y0, y1, x0, x1, ya, yb, xa, xb))
    return th, tw, halo, tiles


def _outscale_size(low_res: Tensor, outscale, scale: int):
    """The size ``upscale(outscale=)`` resamples the x ``scale`` result to; None when ``outscale`` is ``scale`` itself.
    ``ValueError`` for what the resampler would refuse -- here, before the generator runs."""
    import math
    if isinstance(outscale, bool) or not isinstance(outscale, (int, float)) or not math.isfinite(outscale) or not outscale > 0:
        raise ValueError(f'upscale: outscale must be a finite positive number, got {outscale!r}')
    if outscale == scale:
        return None
    h, w = int(low_res.shape[-2]), int(low_res.shape[-1])
    oh, ow = max(1, int(h * outscale + 0.5)), max(1, int(w * outscale + 0.5))
    if h * scale > 16 * oh or w * scale > 16 * ow:
        raise ValueError(f'upscale: outscale = {outscale!r} reduces the x{scale} result {(h * scale, w * scale)} to {(oh, ow)}, '
                         f'more than 16:1 along an axis')
    if oh * ow >= 2 ** 31 or oh * w * scale >= 2 ** 31:
        raise ValueError(f'upscale: outscale = {outscale!r} gives planes of {(oh, ow)}: 2^31 elements or more')
    return oh, ow


def _upscale_ensemble(generator: torch.nn.Module, low_res: Tensor, halo, max_tile_pixels: int, scale: int, precision,
                      staged: bool, n: int) -> Tensor:
    """Geometric self-ensemble: ``mean_k T_k^-1(upscale(T_k(low_res)))`` over the group elements ``k`` (``F.dihedral``: bit 0
    transpose, bit 1 horizontal flip, bit 2 vertical flip) -- all 8, or the 4 without a transpose.  The variants run one after
    another, ``k`` ascending, each through ``upscale`` itself: tiling, the staged trunk, the precision set / restore and the
    fp16 overflow check apply per variant, and an exception from one of them propagates (no partial sum is returned).  One
    kernel per variant maps the result back, scales it and adds it to the sum (csrc/dihedral.hip).
    The result is bit-reproducible: the order of the sum is fixed, and 1 / n is a power of two, so ``y / n`` is exact and
    the kernel's fma ``(1 / n) * y + acc`` rounds once, to the same bits as a multiply followed by an add."""
    from . import functional as F
    acc = None
    for k in range(0, 8, 8 // n):  # n = 4: k = 0, 2, 4, 6
        x_k = low_res if k == 0 else F.dihedral(low_res, k)
        y_k = upscale(generator, x_k, halo, max_tile_pixels, scale, precision, staged)
        if acc is None:
            nb, c, h, w = low_res.shape
            acc = torch.empty((nb, y_k.shape[1], h * scale, w * scale), dtype=torch.float32, device=y_k.device)
        F.dihedral(y_k, F.dihedral_inverse(k), out=acc, alpha=1.0 / n, beta=0.0 if k == 0 else 1.0)
        del x_k, y_k
    return acc


def _upscale_staged(generator: torch.nn.Module, low_res: Tensor, max_out_pixels: int, scale: int) -> Tensor:
    """Large image, generator with a two-stage inference interface (SRGAN): the low-resolution trunk -- 33 of the 36
    convs, receptive field radius 38 pixels -- runs ONCE on the whole image (its largest tensor, h*w*256 floats, stays
    below the kernels' 2^31-element limit up to ``TRUNK_MAX_PIXELS``), and only the last sub-pixel layer + conv3, whose
    tensors are 16x larger, run on row strips of the trunk's feature map with ``head_halo`` rows around.  Exact like the
    halo tiling below, without recomputing the trunk on every tile's halo (1080p: 20 % of the work)."""
    from . import functional as F
    n, c, h, w = low_res.shape
    feat = generator.infer_trunk_nhwc(F.to_nhwc(low_res, 4))
    fh, fw = feat.shape[1], feat.shape[2]
    up = h * scale // fh  # output pixels per feature pixel
    hh = int(generator.head_halo)
    out = torch.empty((n, c, h * scale, w * scale), dtype=low_res.dtype, device=low_res.device)
    rows = max(8, max_out_pixels // (n * fw * up * up) - 2 * hh)  # feature rows per strip
    rows = -(-fh // -(-fh // rows))  # equal strips
    for y0 in range(0, fh, rows):
        y1 = min(fh, y0 + rows)
        ya, yb = max(0, y0 - hh), min(fh, y1 + hh)
        sr = F.to_nchw(generator.infer_head_nhwc(feat[:, ya:yb].contiguous()), c)
        out[:, :, y0 * up:y1 * up] = sr[:, :, (y0 - ya) * up:(y1 - ya) * up]
    return out


def test(args: Namespace, model: object, device) -> None:
    """``test(args, GeneratorClass, device)`` as called from the CLI (torchsr/torchsr.py:253-255)."""
    import numpy as np
    from PIL import Image
    from .srgan.trainer import save_image
    path = getattr(args, 'weights', None) or f'{args.model.lower()}-gan-best.pth'
    try:
        state = load_generator_state(path, ema=bool(getattr(args, 'ema', False)))
    except RuntimeError as exc:
        if not getattr(args, 'ema', False):
            raise
        raise SystemExit(f'torchsr test: {exc}')
    scale = 4
    if args.model.lower() == 'compact':  # a 16-conv and a 32-conv file both load: the depth is the file's
        scale = compact_scale(state, path)  # ... and so is the scale: 12 output channels are x2, 48 are x4
        generator = model(scale_factor=scale, num_conv=compact_num_conv(state)).to(device)
    elif args.model.lower() == 'esrgan':
        # a published RRDBNet file (BasicSR / Real-ESRGAN or xinntao/ESRGAN key names) or one of this package's: the number
        # of blocks (23, or 6 for the anime model) and the scale (x4, or x2 behind pixel_unshuffle) are the file's
        state = rrdbnet_to_generator_state(state)
        num_blocks, scale = rrdbnet_geometry(state)
        generator = model(num_rrdb_blocks=num_blocks, scale_factor=scale).to(device)
        scale = generator.scale_factor
    else:
        generator = model().to(device)
    generator.load_state_dict(state)
    image = np.asarray(Image.open(args.image).convert('RGB'), dtype='float32') / 255.0
    low_res = torch.from_numpy(image).permute(2, 0, 1).unsqueeze(0).contiguous().to(device)
    super_res = upscale(generator, low_res, scale=scale, precision=getattr(args, 'precision', None) or 'fp32',
                        self_ensemble=getattr(args, 'self_ensemble', 0) or 0, outscale=getattr(args, 'outscale', None),
                        color_fix=getattr(args, 'color_fix', None))
    head, tail = os.path.split(args.image)
    save_image(super_res, os.path.join(head, f'upres-{tail}'))
