"""``--outscale`` on the GPU: the resampler (``srx_resample_planes``, ``F.resize_bicubic_aa``) against the fp64 formula with
a derived fp32 bound, its reproducibility, plane independence, guard bands and unaligned operands; ``upscale(outscale=)``
against its restatement bit for bit, the fp16 overflow report and the CLI."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24  # fp32 unit roundoff
GUARD = 64        # floats of NaN on either side of a guarded buffer (a multiple of 4: the 16-byte alignment stays)


def dense(n_in, n_out):
    """The fp64 table of one axis as a dense [n_out, n_in] matrix, and the axis' tap count K."""
    from torchsr_amd import functional as F
    start, weight, k = F.resample_tables(n_in, n_out, dtype='float64')
    m = np.zeros((n_out, n_in))
    for i in range(n_out):
        for t in range(k):
            if weight[i, t] != 0.0:
                m[i, start[i] + t] += weight[i, t]
    return torch.from_numpy(m), k


def reference(x, size):
    """``My . x . Mx^T`` in fp64 on the fp32 input, and the bound per element ``(Ky + Kx + 4) 2^-24 |My| |x| |Mx|^T``: one
    rounding of each weight and one per product and per sum of the two dot products (derived, not measured)."""
    (my, ky), (mx, kx) = dense(x.shape[-2], size[0]), dense(x.shape[-1], size[1])
    x64 = x.detach().cpu().double()
    return my @ x64 @ mx.T, (ky + kx + 4) * U32 * (my.abs() @ x64.abs() @ mx.abs().T)


def _offset_view(t):
    """A contiguous copy of ``t`` whose base is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _guarded(shape, dev, offset=0):
    """A NaN-filled buffer and the view of ``shape`` in its middle (``offset`` floats off the 16-byte alignment)."""
    n = int(np.prod(shape))
    buf = torch.full((GUARD + offset + n + GUARD,), float('nan'), device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD + offset:GUARD + offset + n].view(shape)


def _band_kept(buf, view):
    n, lo = view.numel(), (view.data_ptr() - buf.data_ptr()) // 4
    return bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + n:]).all())


def abi_resize(x, size, tables=None, dst_offset=0):
    """``srx_resample_planes`` itself (no identity bypass), dst and the workspace inside NaN guard bands that must survive.
    ``tables``: ``((start_y, weight_y, Ky), (start_x, weight_x, Kx))`` on the device instead of those of the shapes."""
    from torchsr_amd import _lib
    from torchsr_amd import functional as F
    n, c, h, w = x.shape
    oh, ow = size
    ty, tx = tables or (F._resample_device_tables(h, oh, x.device), F._resample_device_tables(w, ow, x.device))
    dbuf, dst = _guarded((n, c, oh, ow), x.device, dst_offset)
    wbuf, ws = _guarded((n, c, oh, w), x.device)
    _lib.call('srx_resample_planes', x.data_ptr(), dst.data_ptr(), n * c, h, w, oh, ow, ty[0].data_ptr(), ty[1].data_ptr(), ty[2],
              tx[0].data_ptr(), tx[1].data_ptr(), tx[2], ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert _band_kept(dbuf, dst), 'the kernel wrote outside dst'
    assert _band_kept(wbuf, ws), 'the kernel wrote outside the workspace'
    assert not torch.isnan(dst).any() and not torch.isnan(ws).any(), 'an element was left unwritten'
    return dst


SHAPES = [(3, 1, 1, 1, 1), (3, 5, 7, 7, 7), (6, 5, 7, 3, 2), (3, 16, 16, 16, 16), (6, 64, 96, 32, 48), (3, 52, 76, 39, 57),
          (3, 40, 44, 60, 66), (3, 37, 53, 11, 97), (3, 28, 36, 7, 9), (6, 130, 258, 65, 129), (3, 300, 200, 173, 111),
          (3, 64, 64, 4, 4), (3, 9, 300, 9, 75)]


@pytest.mark.parametrize('planes,h,w,oh,ow', SHAPES)
def test_resample_kernel_against_fp64(dev, planes, h, w, oh, ow):
    """One element; enlargement and reduction below one chunk; the identity through the ABI; 2:1 with 16-byte rows; 4:3 and
    2:3; mixed per axis; 4:1; one past a 256-lane chunk and past the row groups (65 = 8 * 8 + 1 rows, 6 * 65 = 4 * 97 + 2);
    ragged large; 16:1 (66 taps); rows untouched and columns 4:1."""
    from torchsr_amd import functional as F
    g = torch.Generator().manual_seed(1000 * h + w)
    x = (torch.rand(planes // 3, 3, h, w, generator=g) - 0.25).to(dev)
    with torch.no_grad():
        got = abi_resize(x, (oh, ow))
        want, bound = reference(x, (oh, ow))
        err = (got.cpu().double() - want).abs()
        worst = (err / bound.clamp_min(1e-300)).max().item()
        print(f'{(planes, h, w)} -> {(oh, ow)}: max err {err.max().item():.3e}, at most {worst:.3f} of the bound '
              f'(bound up to {bound.max().item():.3e})')
        assert (err <= bound).all(), (err.max().item(), worst)
        assert torch.equal(abi_resize(x, (oh, ow)), got)                       # the same bits from a second call
        for p in {0, planes - 1}:                                              # a plane alone: the bits it has in the batch
            alone = abi_resize(x.view(1, planes, h, w)[:, p:p + 1].contiguous(), (oh, ow))
            assert torch.equal(alone, got.view(1, planes, oh, ow)[:, p:p + 1]), p
        op = F.resize_bicubic_aa(x, (oh, ow))
        assert op.shape == (planes // 3, 3, oh, ow)
        if (oh, ow) == (h, w):
            assert op is x                                                     # the bypass: no launch, x itself
            out = torch.empty_like(x)
            assert F.resize_bicubic_aa(x, (oh, ow), out=out) is out and torch.equal(out, x)
            assert torch.equal(got, x)                                         # weights 0, 1, 0, 0: exact through the kernel too
        else:
            assert torch.equal(op, got)
            out = torch.full_like(got, float('nan'))
            assert F.resize_bicubic_aa(x, (oh, ow), out=out) is out and torch.equal(out, got)


@pytest.mark.parametrize('planes,h,w,oh,ow', [(3, 64, 96, 32, 48), (3, 40, 44, 60, 66), (3, 37, 52, 11, 97)])
def test_resample_unaligned_bases_give_the_aligned_bits(dev, planes, h, w, oh, ow):
    """W % 4 == 0: src and / or dst 4 bytes off a 16-byte boundary turn the rows pass to its scalar form.  The sums run in
    the same order, so the bits are those of the aligned call (and within the bound of the fp64 formula with them)."""
    x = (torch.rand(1, planes, h, w, generator=torch.Generator().manual_seed(h + w)) - 0.25).to(dev)
    with torch.no_grad():
        got = abi_resize(x, (oh, ow))
        want, bound = reference(x, (oh, ow))
        assert ((got.cpu().double() - want).abs() <= bound).all()
        assert torch.equal(abi_resize(_offset_view(x), (oh, ow)), got)
        assert torch.equal(abi_resize(x, (oh, ow), dst_offset=1), got)
        assert torch.equal(abi_resize(_offset_view(x), (oh, ow), dst_offset=3), got)


@pytest.mark.parametrize('planes,h,w,oh,ow', [(3, 52, 75, 39, 57), (3, 28, 38, 7, 9), (3, 9, 301, 9, 75), (3, 37, 53, 11, 97)])
def test_resample_odd_width_gives_the_bits_of_its_padded_copy(dev, planes, h, w, oh, ow):
    """W % 4 != 0 runs the scalar rows pass.  Its aligned copy: the same rows padded with zeros to the next multiple of 4
    and resampled with the SAME tables (no start + tap reaches the padding but a row's padded taps, whose weight is 0), which
    runs the 16-byte form: equal bits, and both within the bound."""
    from torchsr_amd import functional as F
    assert w % 4
    x = (torch.rand(1, planes, h, w, generator=torch.Generator().manual_seed(h * w)) - 0.25).to(dev)
    wp = (w + 3) // 4 * 4
    xp = torch.zeros(1, planes, h, wp, device=dev)
    xp[..., :w] = x
    with torch.no_grad():
        tables = (F._resample_device_tables(h, oh, dev), F._resample_device_tables(w, ow, dev))
        got = abi_resize(x, (oh, ow))
        want, bound = reference(x, (oh, ow))
        assert ((got.cpu().double() - want).abs() <= bound).all()
        assert torch.equal(abi_resize(xp, (oh, ow), tables=tables), got)
        assert torch.equal(abi_resize(_offset_view(x), (oh, ow), dst_offset=2), got)


def test_resample_clamps_whatever_the_tables_hold(dev):
    """Starts far outside the plane on both sides read the border rows / columns: finite values of the input's range (the
    rows of weights sum to 1), the NaN bands around dst and the workspace intact."""
    h, w, oh, ow = 12, 20, 6, 10
    x = torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(5)).to(dev)

    def table(n_out, k, starts):
        wt = torch.full((n_out, k), 1.0 / k, device=dev)
        return torch.tensor(starts, dtype=torch.int32, device=dev), wt, k

    with torch.no_grad():
        big = 2 ** 31 - 1
        ty = table(oh, 4, [-big - 1, -5, 0, h - 2, h + 7, big])
        tx = table(ow, 8, [-big - 1, -1, 0, 3, w - 8, w - 7, w - 1, w, 10 ** 6, big])
        got = abi_resize(x, (oh, ow), tables=(ty, tx))
        assert got.min() >= x.min() - 1e-6 and got.max() <= x.max() + 1e-6
        # both starts clamped to the last row / column: every tap reads the corner
        assert torch.allclose(got[0, :, 5, 9], x[0, :, h - 1, w - 1], rtol=1e-6, atol=0)
        # start -big-1 is clamped to 0: rows 0..3, columns 0..7
        assert torch.allclose(got[0, :, 0, 0], x[0, :, :4, :8].double().mean(dim=(1, 2)).float(), rtol=1e-5, atol=0)


# ------------------------------------------------------------------------------------------------ upscale(outscale=)
def _srgan_state():
    """``closed_form_state`` with ``blocks.i.bn2`` halved, as the fp16 inference tests do: the activations stay near 1e2,
    inside fp16's range."""
    from oracle.weights import closed_form_state
    from torchsr_amd.srgan.generator import Generator
    sd = closed_form_state(Generator().state_dict())
    for i in range(16):
        for key in ('weight', 'bias'):
            sd[f'blocks.{i}.bn2.{key}'] = sd[f'blocks.{i}.bn2.{key}'] * 0.5
    return sd


def _srgan(dev):
    from torchsr_amd.srgan.generator import Generator
    gen = Generator().to(dev)
    gen.load_state_dict(_srgan_state())
    return gen


def _esrgan(dev):
    from torchsr_amd.esrgan.generator import Generator
    torch.manual_seed(3)
    return Generator(num_rrdb_blocks=1).to(dev)


def _conv_precisions(gen):
    from torchsr_amd.layers import Conv2d
    return [m._st.precision for m in gen.modules() if isinstance(m, Conv2d)]


def _size(h, w, s):
    return max(1, int(h * s + 0.5)), max(1, int(w * s + 0.5))


CASES = [
    ('srgan', dict(precision='fp32')),
    ('srgan', dict(precision='bf16')),
    ('srgan', dict(precision='fp16')),
    ('esrgan', dict(precision='fp32')),
    ('esrgan', dict(precision='bf16')),
    ('srgan', dict(max_tile_pixels=24 * 20, staged=False)),   # halo tiling
    ('srgan', dict(precision='fp32', self_ensemble=4)),       # one resample of the mean
]


@pytest.mark.parametrize('model,kw', CASES, ids=[f'{m}-' + '-'.join(f'{a}={b}' for a, b in kw.items()) for m, kw in CASES])
def test_upscale_outscale_equals_its_restatement_bitwise(dev, model, kw):
    from torchsr_amd import functional as F
    from torchsr_amd.test import upscale
    gen = _srgan(dev) if model == 'srgan' else _esrgan(dev)
    before = _conv_precisions(gen)
    for shape in ((1, 3, 24, 40), (2, 3, 17, 23)):
        lr = torch.rand(*shape, generator=torch.Generator().manual_seed(7)).to(dev)
        plain = upscale(gen, lr, **kw)
        assert plain.shape == (shape[0], 3, 4 * shape[2], 4 * shape[3]) and torch.isfinite(plain).all()
        assert torch.equal(upscale(gen, lr, outscale=None, **kw), plain)
        assert torch.equal(upscale(gen, lr, outscale=4, **kw), plain)
        assert torch.equal(upscale(gen, lr, outscale=4.0, **kw), plain)
        for s in (2, 3, 1.5, 6):
            size = _size(shape[2], shape[3], s)
            got = upscale(gen, lr, outscale=s, **kw)
            assert _conv_precisions(gen) == before
            assert got.shape == (shape[0], 3) + size, (s, got.shape)
            with torch.no_grad():
                want = F.resize_bicubic_aa(plain, size)
            assert torch.equal(got, want), (shape, s, (got - want).abs().max().item())
            assert not torch.equal(got, torch.zeros_like(got))
    assert _conv_precisions(gen) == before


def test_outscale_reports_fp16_overflow(dev):
    """A non-finite fp16 frame still raises and never reaches the resampler."""
    from torchsr_amd import functional as F
    from torchsr_amd.test import upscale
    gen = _srgan(dev)
    with torch.no_grad():
        gen.conv1[0].weight.mul_(1e8)
    lr = torch.rand(1, 3, 32, 40, generator=torch.Generator().manual_seed(9)).to(dev)
    before = _conv_precisions(gen)
    calls = []
    real = F.resize_bicubic_aa
    F.resize_bicubic_aa = lambda *a, **k: calls.append(a) or real(*a, **k)
    try:
        with pytest.raises(FloatingPointError, match='65504'):
            upscale(gen, lr, precision='fp16', outscale=2)
        assert not calls and _conv_precisions(gen) == before
        with pytest.raises(FloatingPointError, match='65504'):
            upscale(gen, lr, precision='fp16', outscale=2, self_ensemble=4)
        assert not calls and _conv_precisions(gen) == before
        out = upscale(gen, lr, precision='fp32', outscale=2)
        assert len(calls) == 1 and out.shape == (1, 3, 64, 80) and torch.isfinite(out).all()
    finally:
        F.resize_bicubic_aa = real
    assert _conv_precisions(gen) == before


def test_cli_outscale(dev, tmp_path, monkeypatch):
    """``torchsr test lr.png --model srgan --outscale 2`` writes what ``upscale(..., outscale=2)`` gives: a 40 x 24 image
    becomes 80 x 48, byte for byte the ``save_image`` of the API result; the file keeps its name."""
    from PIL import Image
    from torchsr_amd.srgan.trainer import save_image
    from torchsr_amd.test import upscale
    from torchsr_amd.torchsr import main
    monkeypatch.chdir(tmp_path)
    torch.save({'epoch': 1, 'phase': 'srgan-gan', 'state': _srgan_state()}, 'srgan-gan-best.pth')
    img = (np.random.RandomState(2).rand(24, 40, 3) * 255).astype('uint8')
    Image.fromarray(img).save('lr.png')
    main(['test', 'lr.png', '--model', 'srgan', '--outscale', '2'])
    with Image.open('upres-lr.png') as f:
        assert f.size == (80, 48)
    low_res = torch.from_numpy(img.astype('float32') / 255.0).permute(2, 0, 1).unsqueeze(0).contiguous().to(dev)
    save_image(upscale(_srgan(dev), low_res, precision='fp32', outscale=2), 'want.png')
    with open('upres-lr.png', 'rb') as a, open('want.png', 'rb') as b:
        assert a.read() == b.read()
    main(['test', 'lr.png', '--model', 'srgan'])
    with Image.open('upres-lr.png') as f:
        assert f.size == (160, 96)
