"""fp16 inference (``test.upscale(precision='fp16')``, conv precision 3): the 64-channel activations of the SRGAN generator
stored as fp16 between the first and the last conv, fp16 products on v_mfma_f32_32x32x16_f16, fp32 sums.

The fp16 arithmetic is restated here, not in the oracle: torch fp64 on operands rounded with ``.half()``.  fp16 has 11
significant bits, so a result rounded once to nearest is within 2^-11 of its value (relative) -- 8x tighter than bf16's 2^-8;
the end-to-end bounds below are the bf16 tests' bounds times that ratio."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

U16 = 2.0 ** -11  # fp16 unit roundoff


def _h(t):
    """fp16 rounding (torch's, round to nearest even) as an fp64 tensor."""
    return t.half().double()


def _halfbits(t):
    return t.contiguous().view(torch.int16)


def test_f32_to_f16_rounds_to_nearest_even_and_back_exactly(dev):
    """``srx_f32_to_f16`` is bitwise torch ``.half()`` (round to nearest even, overflow to inf) on the values where a
    truncating (v_cvt_pkrtz) or flushing conversion would differ; ``srx_f16_to_f32`` is exact on every fp16 bit pattern."""
    from torchsr_amd import _lib
    s = torch.cuda.current_stream().cuda_stream
    special = [0.0, -0.0, 2.0 ** -24, -(2.0 ** -24), 2.0 ** -25, 3 * 2.0 ** -25, 5 * 2.0 ** -25, 1.5 * 2.0 ** -20,
               6.1e-5, 2.0 ** -14 * (1 - 2.0 ** -11),                  # subnormals, ties between subnormals, the normal edge
               1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 2049.0, 2051.0, 1 + 2.0 ** -11 + 2.0 ** -20,  # ties
               65504.0, 65519.0, 65519.996, 65520.0, -65520.0, 1e6, -1e6, float('inf'), float('-inf'), float('nan'),
               0.1, -0.3, 1 / 3, 255.0 / 256.0]
    g = torch.Generator().manual_seed(3)
    rnd = torch.cat([(torch.rand(4000, generator=g) - 0.5) * 10.0 ** torch.randint(-8, 6, (4000,), generator=g).double()]).float()
    x = torch.cat([torch.tensor(special, dtype=torch.float32), rnd])
    x = torch.cat([x, torch.zeros((-x.numel()) % 4)])
    xd = x.to(dev)
    y = torch.empty(x.numel(), dtype=torch.float16, device=dev)
    _lib.call('srx_f32_to_f16', xd.data_ptr(), y.data_ptr(), x.numel(), s)
    torch.cuda.synchronize()
    want = x.half()
    bad = (_halfbits(y.cpu()) != _halfbits(want)).nonzero().flatten()
    assert bad.numel() == 0, [(x[i].item(), hex(_halfbits(y.cpu())[i].item() & 0xffff), hex(_halfbits(want)[i].item() & 0xffff))
                              for i in bad[:8]]
    assert float(y[16].item()) == 65504.0 and float(y[17].item()) == 65504.0 and y[19].item() == float('inf')
    # fp16 -> fp32: all 65536 patterns (NaNs: still NaN)
    pat = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.float16)
    out = torch.empty(pat.numel(), dtype=torch.float32, device=dev)
    _lib.call('srx_f16_to_f32', pat.to(dev).data_ptr(), out.data_ptr(), pat.numel(), s)
    torch.cuda.synchronize()
    ref = pat.float()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(out.cpu()), nan)
    assert torch.equal(out.cpu()[~nan].view(torch.int32), ref[~nan].view(torch.int32))
    # the Python wrappers: to_f16 / to_f32 are the same conversions
    from torchsr_amd import functional as F
    assert torch.equal(_halfbits(F.to_f16(xd).cpu()), _halfbits(want))
    assert torch.equal(F.to_f32(y).cpu()[~torch.isnan(want.float())], want.float()[~torch.isnan(want.float())])


@pytest.mark.parametrize('n,h,w,cout,shuffle,res,slope,y_cs', [
    (1, 40, 150, 64, 0, False, 1.0, 64),      # plain; wide image, ragged last strip
    (1, 37, 64, 64, 0, False, 0.25, 64),      # PReLU slope; 2 x 2 segments (W <= 64), odd row count
    (2, 24, 24, 64, 0, True, 0.25, 64),       # residual addend; narrow image (W <= 32), N > 1
    (3, 9, 33, 128, 0, False, -0.5, 128),     # Cout 128; a slope outside [0, 1]
    (1, 20, 45, 256, 2, False, 0.25, 64),     # sub-pixel layer: PixelShuffle(2) in the store
    (2, 13, 70, 64, 0, True, 1.0, 96),        # output channel stride > 64 (channels 64..95 untouched), ragged H and W
    (1, 300, 200, 64, 0, True, 0.25, 64),     # several row chunks per column strip (one item per workgroup; several:
                                              # test_plan_forms_gpu.py)
])
def test_fp16_conv3x3_c64(dev, n, h, w, cout, shuffle, res, slope, y_cs):
    """``srx_conv3x3_c64_f16_fwd`` against fp64 of fp16-rounded x, W and addend: the kernel sums in fp32 and rounds ONCE to
    nearest, so every output is within half an fp16 ulp (2^-11 relative) plus the fp32 sum's floor."""
    from torchsr_amd import _lib
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(1000 * h + w + cout + 7)
    x = (torch.rand(n, 64, h, w, generator=g) - 0.5).half()
    wt = torch.randn(cout, 64, 3, 3, generator=g) * (2.0 / 576) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    oh, ow, oc = (2 * h, 2 * w, 64) if shuffle else (h, w, cout)
    skip = (torch.rand(n, oc, oh, ow, generator=g) - 0.5).half() if res else None
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    wd, bd = wt.to(dev), b.to(dev)
    assert L.srx_conv3x3_c64_f16_packed_bytes(cout) == L.srx_conv3x3_c64_bf16_packed_bytes(cout)
    pk = torch.empty(L.srx_conv3x3_c64_f16_packed_bytes(cout), dtype=torch.uint8, device=dev)
    _lib.call('srx_conv3x3_c64_f16_pack', wd.data_ptr(), bd.data_ptr(), None, cout, shuffle, pk.data_ptr(), s)
    y = torch.full((n, oh, ow, y_cs), float('nan'), dtype=torch.float16, device=dev)
    sd = None
    if skip is not None:
        sd = torch.zeros(n, oh, ow, y_cs, dtype=torch.float16)
        sd[..., :oc] = skip.permute(0, 2, 3, 1)
        sd = sd.to(dev)
    _lib.call('srx_conv3x3_c64_f16_fwd', n, h, w, cout, shuffle, xd.data_ptr(), pk.data_ptr(), slope,
              None if sd is None else sd.data_ptr(), y.data_ptr(), y_cs, s)
    torch.cuda.synchronize()
    z = TF.conv2d(x.double(), _h(wt), b.double(), 1, 1)
    if shuffle:
        z = TF.pixel_shuffle(z, 2)
    z = torch.where(z > 0, z, z * slope)
    if skip is not None:
        z = z + skip.double()
    yc = y.cpu()
    got = yc[..., :oc].permute(0, 3, 1, 2).double()
    assert torch.isfinite(got).all()
    err = (got - z).abs()
    bound = z.abs() * U16 + 2e-5 * z.abs().max()
    assert (err <= bound).all(), ((err - bound).max().item(), err.max().item())
    # ... and it IS the rounding of the right value on nearly every element (bf16 products or a truncation would not be)
    same = (z.float().half().double() == got).double().mean().item()
    assert same > 0.995, same
    if y_cs > oc:
        assert torch.isnan(yc[..., oc:].float()).all()  # the channels past the layer's are not written


@pytest.mark.parametrize('n,h,w,cout', [(1, 150, 100, 3), (1, 40, 150, 3), (2, 9, 33, 3), (1, 5, 7, 1), (1, 300, 130, 2)])
def test_fp16_output_conv_thin9(dev, n, h, w, cout):
    """``srx_conv9x9_c64_thin_f16_fwd``: fp16 input and weights, fp32 sums and output, against fp64 of the fp16 operands."""
    from torchsr_amd import _lib
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(7 * h + w + 1)
    x = (torch.rand(n, 64, h, w, generator=g) - 0.5).half()
    wt = torch.randn(cout, 64, 9, 9, generator=g) * (1.0 / 5184) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    wd, bd = wt.to(dev), b.to(dev)
    pk = torch.empty(L.srx_conv9x9_c64_thin_f16_packed_bytes(), dtype=torch.uint8, device=dev)
    _lib.call('srx_conv9x9_c64_thin_f16_pack', wd.data_ptr(), bd.data_ptr(), cout, pk.data_ptr(), s)
    y = torch.full((n, h, w, 4), float('nan'), device=dev)
    _lib.call('srx_conv9x9_c64_thin_f16_fwd', n, h, w, xd.data_ptr(), pk.data_ptr(), y.data_ptr(), s)
    torch.cuda.synchronize()
    z = TF.conv2d(x.double(), _h(wt), b.double(), 1, 4)
    got = y.permute(0, 3, 1, 2).cpu().double()
    assert torch.isfinite(got).all()
    assert ((got[:, :cout] - z).abs().max() / z.abs().max()).item() < 2e-5
    assert float(got[:, cout:].abs().max()) == 0.0


def _fp16_range_state():
    """``closed_form_state`` with every residual branch's output BatchNorm (``blocks.i.bn2``) scaled by 1/2.  As it stands the
    closed form doubles the tower's activations block after block -- 6e4 by conv2 on a 96x96 image, past fp16's 65504 on the
    1080p frame (test_fp16_overflow_is_reported is that case) --; halved, the largest activation stays near 1e2."""
    from oracle.weights import closed_form_state
    from torchsr_amd.srgan.generator import Generator
    sd = closed_form_state(Generator().state_dict())
    for i in range(16):
        for k in ('weight', 'bias'):
            sd[f'blocks.{i}.bn2.{k}'] = sd[f'blocks.{i}.bn2.{k}'] * 0.5
    return sd


def _fp16_generator(dev):
    from torchsr_amd.srgan.generator import Generator
    gen = Generator().to(dev)
    sd = _fp16_range_state()
    gen.load_state_dict(sd)
    return gen, sd


def _conv_precisions(gen):
    from torchsr_amd.layers import Conv2d
    return [m._st.precision for m in gen.modules() if isinstance(m, Conv2d)]


def test_fp16_inference_layers_vs_rounded_operands(dev):
    """The arithmetic of ``precision='fp16'``, one fused layer at a time on the layer's OWN (fp16) input: conv [+ folded
    BatchNorm] [+ PReLU] [+ PixelShuffle] [+ skip] against fp64 of ``act(conv(x, fp16(w_folded)) + b_folded) + skip``,
    each fp16 output within half an ulp; the 3-channel input conv multiplies fp16-rounded image and weights into an fp32
    output (``to_f16`` rounds it once), the 64 -> 3 output conv multiplies fp16 operands and returns fp32."""
    from torchsr_amd import functional as F
    gen, _ = _fp16_generator(dev)
    gen.eval()
    for m in gen.modules():
        if hasattr(m, '_st'):
            m._st.precision = F.PRECISION_F16
    nchw = lambda t, c=None: F.to_nchw(t.float(), c).cpu()  # noqa: E731

    def check(name, layer, x, skip=None, shuffle=False, out32=False):
        y = layer(x) if skip is None else layer(x, residual=skip)
        w, b, st = layer.w, layer.b, layer.st
        z = TF.conv2d(_h(nchw(x, st.cin)), _h(w.cpu()), None if b is None else b.cpu().double(), st.stride, st.pad)
        if shuffle:
            z = TF.pixel_shuffle(z, 2)
        if st.act:
            z = torch.where(z > 0, z, z * st.slope)
        if skip is not None:
            z = z + nchw(skip).double()
        got = nchw(y).double()
        assert y.dtype == (torch.float32 if out32 else torch.float16), (name, y.dtype)
        if out32:
            assert ((got - z).abs().max() / z.abs().max()).item() < 2e-5, name
        else:
            err, bound = (got - z).abs(), z.abs() * U16 + 2e-5 * z.abs().max()
            assert (err <= bound).all(), (name, (err - bound).max().item())
        return y

    with torch.no_grad():
        x4 = F.to_nhwc(torch.rand(1, 3, 56, 72, generator=torch.Generator().manual_seed(5)).to(dev), 4)
        gen.forward_nhwc(x4)  # builds the folded layers
        assert gen.native16() == torch.float16
        f = gen.__dict__['_folded']
        c1 = F.to_f16(check('conv1 + PReLU (fp16 products, fp32 out)', f[0], x4, out32=True))
        t = c1
        for i, blk in enumerate(gen.blocks):
            fa, fb = blk.__dict__['_folded']
            a = check(f'blocks.{i}.conv1 + bn1 + PReLU', fa, t)
            t = check(f'blocks.{i}.conv2 + bn2 + x', fb, a, skip=t)
        out = check('conv2 + bn + conv1', f[1], t, skip=c1)
        for i, layer in enumerate(gen.conv_layers):
            out = check(f'conv_layers.{i} + PixelShuffle + PReLU', layer.__dict__['_folded'], out, shuffle=True)
        for name, inp in (('conv3', out),
                          ('conv3, several tiles', F.to_f16(F.to_nhwc(torch.rand(1, 64, 150, 100, generator=torch.Generator().manual_seed(6)).to(dev) - 0.5)))):
            y = F.conv2d_bf16in(gen.conv3, inp)
            z = TF.conv2d(nchw(inp, 64).double(), _h(gen.conv3.weight.detach().cpu()), gen.conv3.bias.detach().cpu().double(), 1, 4)
            assert y.dtype == torch.float32
            assert ((nchw(y, 3).double() - z).abs().max() / z.abs().max()).item() < 2e-5, name


def test_1080p_inference_fp16_vs_oracle(dev):
    """BASELINE config 5 with ``precision='fp16'``: the full 1080p frame on the windows of the bf16 test against the exact
    oracle.  Max error <= 2.5e-3 of the window's range (the bf16 bound 2e-2 times 2^-3, the ratio of the unit roundoffs),
    rms error at most a quarter of bf16's on the same windows (bf16 run here too), and the halo-tiling path (untiled whole
    frame) equal to the staged path bit for bit."""
    from oracle import srgan as O
    from torchsr_amd.test import upscale
    gen, sd = _fp16_generator(dev)
    before = _conv_precisions(gen)
    g = torch.Generator().manual_seed(12)
    frame = torch.rand(1, 3, 1080, 1920, generator=g)
    fd = frame.to(dev)
    out = upscale(gen, fd, precision='fp16')
    assert out.shape == (1, 3, 4320, 7680) and torch.isfinite(out).all()
    assert _conv_precisions(gen) == before
    whole = upscale(gen, fd, precision='fp16', staged=False, max_tile_pixels=10 ** 10)
    assert torch.equal(whole, out)
    del whole
    ob = upscale(gen, fd, precision='bf16')
    rms = lambda t: t.double().square().mean().sqrt().item()  # noqa: E731
    win, ctx = 40, 48
    for y0, x0 in ((0, 0), (1080 - win, 1920 - win), (530, 850)):
        ya, xa, yb, xb = max(0, y0 - ctx), max(0, x0 - ctx), min(1080, y0 + win + ctx), min(1920, x0 + win + ctx)
        cut = frame[:, :, ya:yb, xa:xb].contiguous()
        with torch.no_grad():
            exact = O.generator_forward(sd, cut, training=False)
        exact = exact[:, :, 4 * (y0 - ya):4 * (y0 - ya + win), 4 * (x0 - xa):4 * (x0 - xa + win)]
        got = out[:, :, 4 * y0:4 * (y0 + win), 4 * x0:4 * (x0 + win)].cpu()
        got16 = ob[:, :, 4 * y0:4 * (y0 + win), 4 * x0:4 * (x0 + win)].cpu()
        top = max(exact.abs().max().item(), 1e-3)
        e16, eb = (got - exact).abs().max().item() / top, (got16 - exact).abs().max().item() / top
        r16, rb = rms(got - exact) / top, rms(got16 - exact) / top
        print(f'window ({y0}, {x0}): fp16 max {e16:.2e} rms {r16:.2e}; bf16 max {eb:.2e} rms {rb:.2e} (of the range)')
        assert e16 <= 2.5e-3, (y0, x0, e16)
        assert r16 <= 0.25 * rb, (y0, x0, r16, rb)


def test_fp16_leaves_other_precisions_alone(dev):
    """bf16 -> fp16 -> bf16 on one generator: both bf16 results bitwise equal (no fp16 pack is reused); a following fp32 call
    equals a fresh generator's fp32 result bitwise; the conv precisions are what they were before each call."""
    from torchsr_amd.srgan.generator import Generator
    from torchsr_amd.test import upscale
    gen, sd = _fp16_generator(dev)
    lr = torch.rand(1, 3, 64, 80, generator=torch.Generator().manual_seed(4)).to(dev)
    before = _conv_precisions(gen)
    b1 = upscale(gen, lr, precision='bf16')
    h = upscale(gen, lr, precision='fp16')
    b2 = upscale(gen, lr, precision='bf16')
    assert _conv_precisions(gen) == before
    assert torch.equal(b1, b2)
    assert not torch.equal(h, b1)
    f32 = upscale(gen, lr, precision='fp32')
    fresh = Generator().to(dev)
    fresh.load_state_dict(sd)
    assert torch.equal(f32, upscale(fresh, lr, precision='fp32'))
    # the halo tiling path at fp16 (small tiles of the whole generator) runs too
    tiled = upscale(gen, lr, precision='fp16', halo=48, max_tile_pixels=64 * 40, staged=False)
    assert tiled.shape == h.shape and torch.isfinite(tiled).all()


def test_fp16_overflow_is_reported(dev):
    """conv1's weights scaled until its output leaves fp16's range: ``upscale(..., 'fp16')`` raises FloatingPointError
    (naming the range and the other precisions) instead of returning inf / NaN; the fp32 result of the same generator
    is finite, and the conv precisions are restored after the raise.  The unscaled closed-form generator overflows too
    (its activations double block after block: see ``_fp16_range_state``) on the 1080p frame's first rows."""
    from oracle.weights import closed_form_state
    from torchsr_amd.srgan.generator import Generator
    from torchsr_amd.test import upscale
    gen, _ = _fp16_generator(dev)
    with torch.no_grad():
        gen.conv1[0].weight.mul_(1e8)
    lr = torch.rand(1, 3, 32, 40, generator=torch.Generator().manual_seed(9)).to(dev)
    assert torch.isfinite(upscale(gen, lr, precision='fp32')).all()
    before = _conv_precisions(gen)
    with pytest.raises(FloatingPointError, match='65504.*bf16.*fp32'):
        upscale(gen, lr, precision='fp16')
    assert _conv_precisions(gen) == before
    raw = Generator().to(dev)
    raw.load_state_dict(closed_form_state(raw.state_dict()))
    frame = torch.rand(1, 3, 1080, 1920, generator=torch.Generator().manual_seed(12))[:, :, :270].contiguous().to(dev)
    assert torch.isfinite(upscale(raw, frame, precision='bf16')).all()
    with pytest.raises(FloatingPointError):
        upscale(raw, frame, precision='fp16')


def test_fp16_refusals(dev, monkeypatch):
    """No silent fallback: ESRGAN (no fp16 chain) and a disabled c64 / t9 kernel are refused with ValueError before any
    launch; precision 3 in training mode or with autograd enabled raises."""
    from torchsr_amd import _dev
    from torchsr_amd.esrgan.generator import Generator as ESRGen
    from torchsr_amd.test import upscale
    esr = ESRGen(num_rrdb_blocks=1).to(dev)
    lr = torch.rand(1, 3, 16, 16, device=dev)
    before = _conv_precisions(esr)
    with pytest.raises(ValueError, match='fp16'):
        upscale(esr, lr, precision='fp16')
    assert _conv_precisions(esr) == before
    gen, _ = _fp16_generator(dev)
    for flag in ('NO_C64', 'NO_T9'):
        monkeypatch.setattr(_dev, flag, True)
        with pytest.raises(ValueError, match='SRX_NO_C64'):
            upscale(gen, lr, precision='fp16')
        monkeypatch.setattr(_dev, flag, False)
    for m in gen.modules():
        if hasattr(m, '_st'):
            m._st.precision = 3
    gen.train()
    with pytest.raises(RuntimeError, match='inference-only'):
        gen(lr)
    gen.eval()
    with pytest.raises(RuntimeError, match='inference-only'):
        gen(lr)  # eval mode, but autograd on


def test_cli_test_fp16(dev, tmp_path, monkeypatch):
    """``torchsr test lr.png --model srgan --precision fp16``: the 8-bit PNG differs from the fp32 run's in no more pixels
    than the bf16 run's does."""
    from PIL import Image
    from torchsr_amd.torchsr import main
    monkeypatch.chdir(tmp_path)
    torch.save({'epoch': 1, 'phase': 'srgan-gan', 'state': _fp16_range_state()}, 'srgan-gan-best.pth')
    Image.fromarray((np.random.RandomState(2).rand(72, 96, 3) * 255).astype('uint8')).save('lr.png')
    outs = {}
    for p in ('fp32', 'bf16', 'fp16'):
        main(['test', 'lr.png', '--model', 'srgan', '--precision', p])
        outs[p] = np.asarray(Image.open('upres-lr.png')).astype(np.int16)
        os.remove('upres-lr.png')
    assert outs['fp16'].shape == (288, 384, 3)
    diff = {p: int((outs[p] != outs['fp32']).sum()) for p in ('bf16', 'fp16')}
    print(f'8-bit values that differ from fp32: {diff}')
    assert diff['fp16'] <= diff['bf16'], diff


def test_fp16_input_conv_above_2_24_pixels(dev):
    """The 3 -> 64 9x9 input conv with fp16 products (precision 3) on a call above 2^24 output pixels: the whole-frame
    (BIG) instantiations of ``gconv_kernel<..., PR = 3>`` -- 64-bit tile bases, exact index division -- against fp64 of the
    fp16-rounded image and weights, on a window at each end of the image (the far one past pixel 2^24)."""
    from torchsr_amd import functional as F
    from torchsr_amd.layers import Conv2d
    conv = Conv2d(3, 64, 9, 1, 4).to(dev).eval()
    conv._st.precision = F.PRECISION_F16
    h = w = 4100
    assert h * w >= 1 << 24
    g = torch.Generator(device=dev).manual_seed(21)
    x = torch.rand(1, h, w, 4, device=dev, generator=g)
    x[..., 3] = 0
    with torch.no_grad():
        y = conv(x)
    torch.cuda.synchronize()
    assert y.shape == (1, h, w, 64)
    wt, b = _h(conv.weight.detach().cpu()), conv.bias.detach().cpu().double()
    for y0, x0 in ((0, 0), (h - 40, w - 40)):
        ya, xa, yb, xb = max(0, y0 - 4), max(0, x0 - 4), min(h, y0 + 44), min(w, x0 + 44)
        cut = _h(x[0, ya:yb, xa:xb, :3].permute(2, 0, 1).unsqueeze(0).cpu())
        z = TF.conv2d(TF.pad(cut, (4 - (x0 - xa), 4 - (xb - x0 - 40), 4 - (y0 - ya), 4 - (yb - y0 - 40))), wt, b)
        got = y[0, y0:y0 + 40, x0:x0 + 40].permute(2, 0, 1).unsqueeze(0).cpu().double()
        assert ((got - z).abs().max() / z.abs().max()).item() < 2e-5, (y0, x0)
