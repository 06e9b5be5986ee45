"""One ``DeviceLoader`` train batch restated BY HAND: the chain of raw ABI calls (``torchsr_amd._lib.call`` on explicit pointers,
``functional.resize`` and ``functional.poisson_tables`` aside) from the parameters the loader kept in ``last_degradation``.  It
shares no code with ``functional``'s launchers or the loader, so ``torch.equal(lr, blind_by_hand(hr, deg, dev))`` checks both.
Also what the loader tests of the degradation family share: the comparison of two draws and the ten test images."""
import os

import numpy as np
import torch

from guarded import _stream

SIZES = [(120, 150), (97, 96), (200, 130), (96, 96), (140, 101), (60, 80), (128, 128), (110, 99), (100, 100), (150, 97)]


def write_images(directory):
    """The ten random PNGs of test_device_data_pipeline_cli, written into the new ``directory``; returns its path."""
    from PIL import Image
    os.makedirs(directory)
    rng = np.random.RandomState(0)
    for i, (h, w) in enumerate(SIZES):
        Image.fromarray((rng.rand(h, w, 3) * 255).astype('uint8')).save(os.path.join(str(directory), f'{i}.png'))
    return str(directory)


def same_draws(a, b, but=()):
    """Two drawn batches hold the same keys and values, the keys ``but`` aside."""
    assert a.keys() - set(but) == b.keys() - set(but)
    for k in a.keys() - set(but):
        assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k], k


def _noise(x, deg, stage, seed, dev):
    """One noise step: the Poisson call when a sample of the stage drew it, then the Gaussian one (8-bit result)."""
    from torchsr_amd import _lib
    from torchsr_amd import functional as F
    pick = (lambda a: a) if stage is None else (lambda a: a[stage])
    n, _, h, w = x.shape
    sigma, gd = pick(deg['sigma_n']), torch.from_numpy(pick(deg['gray'])).to(dev)
    if 'poisson_scale' in deg:
        scale = pick(deg['poisson_scale'])
        assert ((scale > 0) != (sigma > 0)).all()                          # each sample has exactly one of the two
        if scale.any():
            sd, levels, mid = torch.from_numpy(scale).to(dev), torch.empty((n, 8), dtype=torch.int32, device=dev), torch.empty_like(x)
            _lib.call('srx_add_poisson_noise', x.data_ptr(), mid.data_ptr(), sd.data_ptr(), gd.data_ptr(),
                      F.poisson_tables(dev).data_ptr(), levels.data_ptr(), seed & 0xFFFFFFFF, seed >> 32, n, h, w, 0, _stream())
            x = mid
    out = torch.empty_like(x)
    _lib.call('srx_add_gaussian_noise', x.data_ptr(), out.data_ptr(), torch.from_numpy(sigma).to(dev).data_ptr(), gd.data_ptr(),
              seed & 0xFFFFFFFF, seed >> 32, n, h, w, 1, _stream())
    return out


def _jpeg(x, deg, stage, dev):
    """One JPEG step (8-bit result): ``srx_jpeg_sim2`` with its workspace when any flag of the batch is set, else ``srx_jpeg_sim``."""
    from torchsr_amd import _lib
    pick = (lambda a: a) if stage is None else (lambda a: a[stage])
    n, _, h, w = x.shape
    qd, out = torch.from_numpy(pick(deg['quality'])).to(dev), torch.empty_like(x)
    flags = deg.get('chroma420')
    if flags is None or not flags.any():
        _lib.call('srx_jpeg_sim', x.data_ptr(), out.data_ptr(), qd.data_ptr(), n, h, w, 1, _stream())
        return out
    fd = torch.from_numpy(pick(flags)).to(dev)
    nbytes = _lib.call('srx_jpeg_sim2_workspace', n, h, w)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    _lib.call('srx_jpeg_sim2', x.data_ptr(), out.data_ptr(), qd.data_ptr(), fd.data_ptr(), n, h, w, 1, ws.data_ptr(), nbytes, None,
              _stream())
    return out


def bicubic_by_hand(hr, up, dev):
    """``srx_bicubic_down(quantize=1)``: the low-resolution side of a ``bicubic`` batch."""
    from torchsr_amd import _lib
    n, _, h, w = hr.shape
    lr = torch.empty((n, 3, h // up, w // up), device=dev)
    _lib.call('srx_bicubic_down', hr.data_ptr(), lr.data_ptr(), n, 3, h, w, up, 1, _stream())
    return lr


def blind_by_hand(hr, deg, dev, up=4, stages=False):
    """The calls of one ``blind`` batch: blur, bicubic x1/up (unquantised), the noise step, the JPEG step.  ``stages=True`` returns
    what each of the four produced, the batch last."""
    from torchsr_amd import _lib
    n, _, h, w = hr.shape
    pd, kd = torch.from_numpy(deg['parm']).to(dev), torch.from_numpy(deg['ksize']).to(dev)
    a, b = torch.empty_like(hr), torch.empty((n, 3, h // up, w // up), device=dev)
    _lib.call('srx_blur_aniso', hr.data_ptr(), a.data_ptr(), pd.data_ptr(), kd.data_ptr(), n, 3, h, w, _stream())
    _lib.call('srx_bicubic_down', a.data_ptr(), b.data_ptr(), n, 3, h, w, up, 0, _stream())
    c = _noise(b, deg, None, deg['seed'], dev)
    d = _jpeg(c, deg, None, dev)
    assert not torch.equal(a, hr) and not torch.equal(c, b) and not torch.equal(d, c)   # every stage does something
    return (a, b, c, d) if stages else d


def blind2_by_hand(hr, deg, dev):
    """The calls of one ``blind2`` batch: filter -> resize -> noise -> JPEG, twice, the second JPEG and the final filter around
    the resize to the low-resolution size in the drawn order."""
    from torchsr_amd import _lib
    from torchsr_amd import functional as F
    n = hr.shape[0]
    wd, kd = torch.from_numpy(deg['weights']).to(dev), torch.from_numpy(deg['ksize']).to(dev)
    (s1, s2, lc), modes = deg['sizes'], deg['modes']

    def filt(x, stage, quantize):
        out = torch.empty_like(x)
        _lib.call('srx_filter2d', x.data_ptr(), out.data_ptr(), wd[stage].data_ptr(), kd[stage].data_ptr(), n, 3, x.shape[2],
                  x.shape[3], quantize, _stream())
        return out

    with torch.no_grad():
        a = filt(hr, 0, 0)
        b = F.resize(a, (s1, s1), modes[0])
        c = _noise(b, deg, 0, deg['seed1'], dev)
        d = _jpeg(c, deg, 0, dev)
        e = filt(d, 1, 0)
        f = F.resize(e, (s2, s2), modes[1])
        g = _noise(f, deg, 1, deg['seed2'], dev)
        assert tuple(d.shape) == (n, 3, s1, s1) and tuple(g.shape) == (n, 3, s2, s2)
        assert not torch.equal(a, hr) and not torch.equal(c, b) and not torch.equal(d, c) and not torch.equal(g, f)
        if deg['order'] == 'A':
            return _jpeg(filt(F.resize(g, (lc, lc), modes[2]), 2, 0), deg, 1, dev)
        return filt(F.resize(_jpeg(g, deg, 1, dev), (lc, lc), modes[2]), 2, 1)
