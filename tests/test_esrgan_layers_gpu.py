"""Every conv problem of the batch-16 ESRGAN GAN step (BASELINE configs[3]: 23 RRDBs, 128 x 128 crops), at the step's own sizes,
against float64 -- in exact fp32 (--disable-amp) and with bf16 products (the quoted configuration).

The rows are ``step_layers.ESRGAN_STEP_CONVS``; each runs through the entry point the step uses: ``layers.Conv2d`` with the
step's flags (``test_step_layers_gpu.run_conv_case``: nearest-x2 gather, fused LeakyReLU, BatchNorm partial statistics, activation
backwards folded into or away from the data gradient, weight gradients accumulated into a pre-filled ``.grad`` through the
deferred queue), the dense-block convs through the launchers and the queue ``functional._RRDBTrunk`` calls with the descriptors it
builds (192-strided buffers, paired and scaled weight gradients), VGG19 under bf16 through the ``srx_conv3x3_bf16s_*`` ABI with
the argument lists ``functional._FrozenConvStack`` passes.  ``test_esrgan_step_launches_are_covered`` holds the table to the step.

fp32 rows: the checks of ``test_step_layers_gpu.py``, unchanged.  bf16 rows: the reference is the float64 convolution of the
bf16-ROUNDED operands (both factors of every product; the fp32 bias added, bias gradients from the unrounded gradient) -- a
bf16 x bf16 product is exact in fp32, so only the K-term fp32 accumulation separates the kernel from it:

* elementwise: |out - ref64| <= gamma_K (|r(a)| conv |r(b)|), u = 2^-24 (``max err/bound`` is printed per output);
* statistical: relL2(kernel) <= 1.5 x relL2(torch CPU fp32 on the same rounded operands) + 1e-7;
* outputs stored as bf16: |out - ref64| <= 2^-8 |s| + the bound above for the fp32 sum s it rounds (half a bf16 ulp; and
  ``test_bf16s_gpu.within_half_ulp``), and re-rounding the float64 value gives the same bf16 on > 99.5 % of the elements.
"""
import ctypes as C
import zlib

import pytest
import torch
import torch.nn.functional as TF

from step_layers import CONV_LAUNCHES_TESTED_ELSEWHERE, ESRGAN_STEP_CONVS, bf16_round, conv_refs
from test_bf16s_gpu import within_half_ulp
from test_step_layers_gpu import PIN_MARGIN, FormOverBudget, budget, check, gamma, nchw, nhwc, prof_keys, run_conv_case  # noqa: F401  (budget: OVER_F's twin below)

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
PREFILL = 0.01  # scale of what the .grad buffers hold before the backward pass (gradients are O(1) and larger)
# Outputs measured (MI355X) above the statistical budget, as in test_step_layers_gpu.py: '<row id>[<precision>] <output>': ratio.
OVER_F = {'g.up1[fp32] dx': 1.95, 'g.conv3[fp32] dx': 1.98, 'g.conv3[fp32] db': 2.23, 'g.conv4[fp32] db': 5.53,
          'g.conv4[bf16] db': 5.53, 'g.rdb.conv3[fp32] y': 1.98, 'g.rdb.conv4[fp32] y': 2.15, 'd2.adv[fp32] y': 1.99,
          'd8.pair[fp32] y': 2.7, 'd8.adv[fp32] y': 2.7, 'd11.pair[bf16] dx': 2.61, 'd11.adv[bf16] dx': 2.62,
          'd14.pair[fp32] y': 3.74, 'd14.pair[bf16] y': 2.47, 'd17.pair[bf16] y': 2.48, 'd17.pair[bf16] dx': 3.14,
          'd17.adv[bf16] y': 2.48, 'd20.pair[fp32] y': 2.55, 'v21.stack[bf16] y': 2.77}


def _budget(what, mine, theirs, f, report):
    """``test_step_layers_gpu.budget`` with this table's OVER_F"""
    report.append((what, mine, theirs, mine > f * theirs + 1e-7))
    if what in OVER_F:
        assert mine <= PIN_MARGIN * OVER_F[what] * theirs + 1e-7, (what, mine, theirs, OVER_F[what])
    else:
        assert mine <= f * theirs + 1e-7, (what, mine, theirs)


def _seed(case):
    return torch.Generator().manual_seed(zlib.crc32(case['id'].encode()))


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------ the dense-block convs
C0, G, TOTAL = 64, 32, 192   # a dense block's buffer: the block's input, then conv1..4's 32-channel slices
SLOPE, RDB_SCALE = 0.2, 0.2


def _dense_conv(k, precision):
    from torchsr_amd.layers import Conv2d, set_conv_precision
    conv = Conv2d(C0 + k * G, C0 if k == 4 else G, 3, 1, 1, act=0 if k == 4 else 2, slope=0.0 if k == 4 else SLOPE)
    if precision == 'bf16':
        set_conv_precision(conv, 'bf16')
    return conv


def run_dense_conv_case(case, dev, report, precision, u):
    """conv k + 1 of a dense block as ``_RRDBTrunk`` launches it conv by conv (exact fp32): the forward reads ``cin`` channels of
    the 192-strided buffer and writes its slice behind them (conv5: ``conv * scale + x`` into the next block's buffer); the data
    gradient (``srx_conv2d_bwd_data_ex``) writes (conv5), accumulates into (conv2..4) or adds (conv1) the shared gradient buffer
    and applies the LeakyReLU backward to the slice it completes."""
    from torchsr_amd import _lib, functional as F
    n, h, w = case['nhw']
    k = case['dense']
    cin, cout = C0 + k * G, (C0 if k == 4 else G)
    g = _seed(case)
    buf = TF.leaky_relu(torch.randn((n, TOTAL, h, w), generator=g), SLOPE)
    wt = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (cin * 9)) ** 0.5
    b = torch.randn((cout,), generator=g) * 0.1
    conv = _dense_conv(k, precision).to(dev)
    with torch.no_grad():
        conv.weight.copy_(wt)
        conv.bias.copy_(b)
    st = conv._st
    d = _lib.Conv2dDesc(n, h, w, cin, TOTAL, cout, TOTAL, 3, 3, 1, 1, 0, st.act, st.slope, 0, st.precision)
    st.pack(conv.weight, d)
    s = _stream()
    x = buf[:, :cin]
    gbuf_in = nhwc(buf, TOTAL).to(dev)
    pre64, pre32, by = conv_refs('y', x, wt, x.shape, wt.shape, 1, 1, 0, b, precision == 'bf16', u)
    if k == 4:
        nxt = torch.full((n, h, w, TOTAL), 7.0, device=dev)
        F._conv_fwd(d, gbuf_in.data_ptr(), st.wpk_fwd.data_ptr(), conv.bias.data_ptr(), nxt.data_ptr(), gbuf_in, s,
                    residual=(gbuf_in.data_ptr(), RDB_SCALE))
        x0 = buf[:, :C0]
        sc = float(torch.tensor(RDB_SCALE, dtype=torch.float32))
        # (two more roundings: the product with the scale, the sum with x)
        check(f"{case['id']} y", nchw(nxt.cpu(), C0), pre64 * sc + x0.double(), pre32 * sc + x0,
              (1 + 2 * u) * sc * by + 2 * u * (sc * pre64.abs() + x0.double().abs()), False, report)
        assert bool((nxt[..., C0:] == 7.0).all())   # the other channels of the next block's buffer are not this conv's
    else:
        out = gbuf_in.clone()
        F._conv_fwd(d, out.data_ptr(), st.wpk_fwd.data_ptr(), conv.bias.data_ptr(), out.data_ptr() + 4 * cin, out, s)
        torch.cuda.synchronize()
        oc = out.cpu()
        assert torch.equal(oc[..., :cin], nhwc(buf, TOTAL)[..., :cin]) and torch.equal(oc[..., cin + G:], nhwc(buf, TOTAL)[..., cin + G:])
        check(f"{case['id']} y", oc[..., cin:cin + G].permute(0, 3, 1, 2).contiguous(), TF.leaky_relu(pre64, SLOPE), TF.leaky_relu(pre32, SLOPE), by, False, report)
    # the data gradient.  conv5's output gradient is the block's (dense, 64 channels); the others read their slice of the shared
    # gradient buffer, complete and masked
    if k == 4:
        dy = torch.randn((n, C0, h, w), generator=g)
        dyg = nhwc(dy, C0).to(dev)
        gk = dyg.data_ptr()
    else:
        dy = torch.randn((n, G, h, w), generator=g)
        full = torch.randn((n, TOTAL, h, w), generator=g)
        full[:, cin:cin + G] = dy
        dyg = nhwc(full, TOTAL).to(dev)
        gk = dyg.data_ptr() + 4 * cin
    old = torch.randn((n, TOTAL, h, w), generator=g)          # what conv k+2..5 left in the gradient buffer
    skip = torch.randn((n, C0, h, w), generator=g)            # the block's output gradient (the `+ x` of the block)
    e = _lib.DgradEpilogue()
    lo, hi = cin - G, cin
    if k > 0:
        e.act_out, e.act_slope, e.c_lo, e.c_hi = gbuf_in.data_ptr(), SLOPE, lo, hi
    dx64, dx32, bdx = conv_refs('dx', dy, wt, x.shape, wt.shape, 1, 1, 0, None, precision == 'bf16', u)
    dd = d if k < 4 else _lib.Conv2dDesc(n, h, w, cin, TOTAL, cout, cout, 3, 3, 1, 1, 0, st.act, st.slope, 0, st.precision)
    extra = 1
    if k == 4:
        eff = 0.2 * RDB_SCALE                                  # the last block of an RRDB: rrdb_scale * scale_ratio
        skipg = nhwc(skip, C0).to(dev)
        e.out_scale = eff
        e.addend, e.addend_ld, e.addend_channels, e.addend_scale = skipg.data_ptr(), C0, C0, 0.2
        outg = torch.full((n, h, w, TOTAL), 7.0, device=dev)
        eff32, a32 = float(torch.tensor(eff, dtype=torch.float32)), float(torch.tensor(0.2, dtype=torch.float32))
        add64 = torch.zeros_like(dx64)
        add64[:, :C0] = a32 * skip.double()
        want64, want32, bound = eff32 * dx64 + add64, eff32 * dx32 + add64.float(), eff32 * bdx
        extra = 3                                              # the two scalings and the sum
    elif k > 0:
        e.accumulate = 1
        outg = nhwc(old, TOTAL).to(dev)
        add64 = old[:, :cin].double()
        want64, want32, bound = dx64 + add64, dx32 + add64.float(), bdx
    else:
        oldg = nhwc(old, TOTAL).to(dev)
        e.addend, e.addend_ld, e.addend_channels = oldg.data_ptr(), TOTAL, C0
        dd = _lib.Conv2dDesc(n, h, w, C0, C0, cout, TOTAL, 3, 3, 1, 1, 0, st.act, st.slope, 0, st.precision)
        outg = torch.full((n, h, w, C0), 7.0, device=dev)
        add64 = old[:, :C0].double()
        want64, want32, bound = dx64 + add64, dx32 + add64.float(), bdx
    if k > 0:  # the LeakyReLU backward of the conv below on the slice this call completes: one more multiplication
        m64 = torch.where(buf[:, lo:hi] > 0, 1.0, SLOPE).double()
        for t in (want64, want32, bound, add64):
            t[:, lo:hi] *= m64.to(t.dtype)
        extra += 1
    bound = bound * (1 + extra * u) + extra * u * (want64.abs() + add64.abs())
    ddref = C.byref(dd)
    nws = _lib.lib().srx_conv2d_bwd_data_ws_floats(ddref)
    ws = torch.empty(max(int(nws), 4), device=dev)
    _lib.call('srx_conv2d_bwd_data_ex', ddref, gk, st.wpk_bwd.data_ptr(), outg.data_ptr(), C.byref(e), ws.data_ptr() if nws else None, nws, s)
    torch.cuda.synchronize()
    got = nchw(outg.cpu(), cin)
    check(f"{case['id']} dx", got, want64, want32, bound, False, report)
    if k in (1, 2, 3):
        assert torch.equal(outg.cpu()[..., cin:], nhwc(old, TOTAL)[..., cin:])   # channels past Cin belong to the later convs


def run_dense_wgrad_case(case, dev, report, precision, u):
    """The weight (+ riding bias) gradients of a dense block through ``functional.WeightGradQueue`` as ``_RRDBTrunk.backward``
    fills it: conv1 + conv2 and conv3 + conv4 as PAIRS (one 64-column problem on the shared 192-strided buffers,
    ``srx_conv2d_bwd_weight_multi_pair``), conv5 with the block's scale in the reduction (``..._multi_scaled``), all accumulated
    into pre-filled gradients."""
    from torchsr_amd import _lib, functional as F
    n, h, w = case['nhw']
    prec = 1 if precision == 'bf16' else 0
    rounded = precision == 'bf16'
    g = _seed(case)
    buf = TF.leaky_relu(torch.randn((n, TOTAL, h, w), generator=g), SLOPE)
    bufg = nhwc(buf, TOTAL).to(dev)
    m = n * h * w
    outs = []
    with F.deferred_weight_grads() as queue:
        if 'pair' in case:
            lo = case['pair']                      # 0: conv1 + conv2, 2: conv3 + conv4
            gfull = torch.randn((n, TOTAL, h, w), generator=g)
            gg = nhwc(gfull, TOTAL).to(dev)
            cin_lo, cin_hi = C0 + lo * G, C0 + (lo + 1) * G
            dp = _lib.Conv2dDesc(n, h, w, cin_hi, TOTAL, 2 * G, TOTAL, 3, 3, 1, 1, 0, 2, SLOPE, 0, prec)
            sinks = []
            for cin, off in ((cin_lo, cin_lo), (cin_hi, cin_lo + G)):
                w0 = torch.randn((G, cin, 3, 3), generator=g) * PREFILL
                b0 = torch.randn((G,), generator=g) * PREFILL
                sinks.append((w0.to(dev), b0.to(dev)))
                outs.append((f'{case["id"]} conv{cin // G - 1}', buf[:, :cin], gfull[:, off:off + G], w0, b0, sinks[-1], 1.0))
            queue.add_pair(dp, cin_lo, bufg.data_ptr(), gg.data_ptr() + 4 * cin_lo, (sinks[0][0].data_ptr(), sinks[1][0].data_ptr()),
                           (sinks[0][1].data_ptr(), sinks[1][1].data_ptr()), (bufg, gg))
        else:                                      # conv5: a dense 64-channel output gradient, scale in the reduction
            dy = torch.randn((n, C0, h, w), generator=g)
            dyg = nhwc(dy, C0).to(dev)
            d5 = _lib.Conv2dDesc(n, h, w, TOTAL, TOTAL, C0, C0, 3, 3, 1, 1, 0, 0, 0.0, 0, prec)
            w0 = torch.randn((C0, TOTAL, 3, 3), generator=g) * PREFILL
            b0 = torch.randn((C0,), generator=g) * PREFILL
            sink = (w0.to(dev), b0.to(dev))
            scale = 0.2 * RDB_SCALE
            queue.add(d5, bufg.data_ptr(), dyg.data_ptr(), sink[0].data_ptr(), sink[1].data_ptr(), (bufg, dyg), scale)
            outs.append((f'{case["id"]} conv5', buf, dy, w0, b0, sink, float(torch.tensor(scale, dtype=torch.float32))))
    torch.cuda.synchronize()
    for what, x, dy, w0, b0, (gw, gb), sc in outs:
        dw64, dw32, bdw = conv_refs('dW', x, dy, x.shape, w0.shape, 1, 1, 0, None, rounded, u)
        # the sum, its product with the scale (one more rounding) and its landing on what the buffer held (one more)
        extra = 1 if sc == 1.0 else 2
        want = sc * dw64 + w0.double()
        check(f'{what} dW', gw.cpu(), want, sc * dw32 + w0, gamma(m + extra, u) * (sc * bdw / gamma(m, u) + w0.double().abs()), False, report)
        g64 = dy.double()
        check(f'{what} db', gb.cpu(), sc * g64.sum((0, 2, 3)) + b0.double(), sc * dy.sum((0, 2, 3)) + b0,
              gamma(m + extra, u) * (sc * g64.abs().sum((0, 2, 3)) + b0.double().abs()), False, report)


# ------------------------------------------------------------------------------------- VGG19 under bf16: bf16-stored activations
def run_bf16s_case(case, dev, report, precision, u):
    """One VGG19 layer of the perceptual loss under autocast, as ``functional._stack_conv_fwd`` / ``_stack_conv_dgrad`` call
    it: source + target forward as one batch of 32 on bf16-stored input, output fp32 (in front of a pool, the last layer) or
    bf16 (``out16``, every form the step uses at this shape); the source's data gradient at batch 16 from a bf16-stored gradient,
    masked by the layer's own (ReLU) input where a conv made it, written as bf16 (fp32 for the layer behind the 3 -> 64 one)."""
    from torchsr_amd import _lib
    assert precision == 'bf16'
    hw, cin, cout = case['bf16s']
    n2, n = 32, 16
    L, s = _lib.lib(), _stream()
    g = _seed(case)
    x = bf16_round(torch.relu(torch.randn((n2, cin, hw, hw), generator=g)))
    wt = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (cin * 9)) ** 0.5
    b = torch.randn((cout,), generator=g) * 0.1
    dy = bf16_round(torch.randn((n, cout, hw, hw), generator=g))
    wg, bg = wt.to(dev), b.to(dev)
    d2 = _lib.Conv2dDesc(n2, hw, hw, cin, cin, cout, cout, 3, 3, 1, 1, 0, _lib.ACT_RELU, 0.0, 0, 1)
    d1 = _lib.Conv2dDesc(n, hw, hw, cin, cin, cout, cout, 3, 3, 1, 1, 0, _lib.ACT_RELU, 0.0, 0, 1)
    assert L.srx_conv3x3_bf16s_applicable(C.byref(d2)) == 1 and L.srx_conv3x3_bf16s_applicable(C.byref(d1)) == 1
    nb = L.srx_conv3x3_bf16s_packed_bytes(C.byref(d2)) // 2
    wf, wb = torch.empty(nb, dtype=torch.bfloat16, device=dev), torch.empty(nb, dtype=torch.bfloat16, device=dev)
    _lib.call('srx_conv3x3_bf16s_pack', C.byref(d2), wg.data_ptr(), wf.data_ptr(), wb.data_ptr(), s)
    xg = x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(dev)

    def ws_for(dref, mode):
        nws = L.srx_conv3x3_bf16s_ws_floats(dref, mode)
        return torch.empty(max(int(nws), 4), device=dev), nws

    pre64, pre32, by = conv_refs('y', x, wt, x.shape, wt.shape, 1, 1, 0, b, True, u)
    y64, y32 = torch.relu(pre64), torch.relu(pre32)
    for out16 in case['out16']:
        y = torch.empty((n2, hw, hw, cout), dtype=torch.bfloat16 if out16 else torch.float32, device=dev)
        ws, nws = ws_for(C.byref(d2), 0)
        _lib.call('srx_conv3x3_bf16s_fwd', C.byref(d2), xg.data_ptr(), wf.data_ptr(), bg.data_ptr(), 1, y.data_ptr(), out16,
                  ws.data_ptr(), nws, s)
        torch.cuda.synchronize()
        got = y.cpu().permute(0, 3, 1, 2)
        if out16:
            stored_check(f"{case['id']} y16", got, y64, by, report)
        else:
            check(f"{case['id']} y", got.contiguous(), y64, y32, by, False, report)
    # the source half's data gradient, the ReLU that made x folded in
    xs = x[:n]
    dyg = dy.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(dev)
    dx64, dx32, bdx = conv_refs('dx', dy, wt, xs.shape, wt.shape, 1, 1, 0, None, True, u)
    if case['masked']:
        mask = (xs > 0).double()
        dx64, dx32, bdx = dx64 * mask, dx32 * mask.float(), bdx * mask
    dx_out16 = case['dx16']
    dx = torch.empty((n, hw, hw, cin), dtype=torch.bfloat16 if dx_out16 else torch.float32, device=dev)
    ws, nws = ws_for(C.byref(d1), 1)
    _lib.call('srx_conv3x3_bf16s_bwd_data', C.byref(d1), dyg.data_ptr(), wb.data_ptr(), xg[:n].data_ptr() if case['masked'] else None, dx.data_ptr(), dx_out16,
              ws.data_ptr(), nws, s)
    torch.cuda.synchronize()
    got = dx.cpu().permute(0, 3, 1, 2)
    if dx_out16:
        stored_check(f"{case['id']} dx16", got, dx64, bdx, report)
        assert not case['masked'] or bool(((got.float() == 0) | (xs > 0)).all())   # nothing passes a closed ReLU
    else:
        check(f"{case['id']} dx", got.contiguous(), dx64, dx32, bdx, False, report)


def stored_check(what, got16, ref64, bound, report):
    """An output the kernel stores as bf16: the rounding (half an ulp: 2^-8 relative at most) of an fp32 sum s within ``bound``
    of the float64 value -- |got - ref| <= 2^-8 |s| + bound, |s| <= |ref| + bound -- and on nearly every element THE rounding of
    the float64 value itself."""
    got = got16.double()
    err = (got - ref64).abs()
    lim = 2.0 ** -8 * (ref64.abs() + bound) + bound
    print(f'  {what:44s} max err/bound {(err / lim.clamp_min(1e-300)).max().item():.3f}  (bf16-stored)')
    assert (err <= lim).all(), (what, (err - lim).max().item(), err.max().item())
    assert within_half_ulp(got16, ref64), what
    same = (ref64.float().bfloat16().double() == got).double().mean().item()
    print(f'  {what:44s} equal to the re-rounded float64 value on {same:.5f} of the elements')
    assert same > 0.995, (what, same)


def run_first3_bf16s_case(case, dev, report, precision, u):
    """VGG19's 3 -> 64 layer at the head of the bf16-storage stack: ``srx_conv2d_fwd_first3_to_bf16`` on the fp32 images (batch 32,
    bf16 products, bf16 output) and the exact fp32 data gradient of the source half (batch 16) from the gradient the layer above
    hands down as fp32."""
    from torchsr_amd import _lib, functional as F
    from torchsr_amd.layers import Conv2d, set_conv_precision
    hw = case['first3']
    n2, n = 32, 16
    g = _seed(case)
    x = torch.rand((n2, 3, hw, hw), generator=g)
    wt = torch.randn((64, 3, 3, 3), generator=g) * (2.0 / 27) ** 0.5
    b = torch.randn((64,), generator=g) * 0.1
    conv = Conv2d(3, 64, 3, 1, 1, act=_lib.ACT_RELU)
    with torch.no_grad():
        conv.weight.copy_(wt)
        conv.bias.copy_(b)
    conv = conv.to(dev).requires_grad_(False)
    set_conv_precision(conv, 'bf16')
    st, s = conv._st, _stream()
    xg = nhwc(x, 4).to(dev)
    d2 = st.desc(n2, hw, hw)
    st.pack(conv.weight, d2)
    y = torch.empty((n2, hw, hw, 64), dtype=torch.bfloat16, device=dev)
    _lib.call('srx_conv2d_fwd_first3_to_bf16', C.byref(d2), xg.data_ptr(), st.wpk_fwd.data_ptr(), conv.bias.data_ptr(), y.data_ptr(), s)
    torch.cuda.synchronize()
    pre64, _, by = conv_refs('y', x, wt, x.shape, wt.shape, 1, 1, 0, b, True, u)
    stored_check(f"{case['id']} y16", y.cpu().permute(0, 3, 1, 2), torch.relu(pre64), by, report)
    dy = torch.randn((n, 64, hw, hw), generator=g)
    dyg = nhwc(dy, 64).to(dev)
    dx = torch.empty((n, hw, hw, 4), device=dev)
    F._conv_dgrad(st.desc(n, hw, hw), dyg.data_ptr(), st.wpk_bwd.data_ptr(), dx.data_ptr(), dx, s)
    torch.cuda.synchronize()
    dx64, dx32, bdx = conv_refs('dx', dy, wt, (n, 3, hw, hw), wt.shape, 1, 1, 0, None, False, u)
    check(f"{case['id']} dx", nchw(dx.cpu(), 3), dx64, dx32, bdx, False, report)


def run_case(case, dev, report, precision, u=U):
    if 'dense' in case:
        run_dense_conv_case(case, dev, report, precision, u)
    elif 'pair' in case or 'scaled' in case:
        run_dense_wgrad_case(case, dev, report, precision, u)
    elif 'bf16s' in case:
        run_bf16s_case(case, dev, report, precision, u)
    elif 'first3' in case:
        run_first3_bf16s_case(case, dev, report, precision, u)
    else:
        run_conv_case(case, dev, report, precision, u, prefill=PREFILL)


def _params():
    out = []
    for case in ESRGAN_STEP_CONVS:
        for precision in case['precisions']:
            pid = f"{case['id']}-{precision}"
            over = {k: v for k, v in OVER_F.items() if k.split(' ')[0] == f"{case['id']}[{precision}]"}
            marks = ()
            if over:
                why = ', '.join(f'{k} {v:.2f} x' for k, v in over.items())
                marks = pytest.mark.xfail(strict=True, raises=FormOverBudget, reason=f'measured above F (torch fp32 distance): {why}')
            out.append(pytest.param(case, precision, id=pid, marks=marks))
    return out


@pytest.mark.parametrize('case,precision', _params())
def test_esrgan_conv_vs_fp64(dev, monkeypatch, case, precision):
    import test_step_layers_gpu as T
    # (the shared check() files its statistical figures under this table's names and OVER_F)
    monkeypatch.setattr(T, 'budget', lambda what, *a: _budget(what.replace(case['id'], f"{case['id']}[{precision}]", 1), *a))
    report = []
    keys = prof_keys(lambda: run_case(case, dev, report, precision), aux=True)
    print('  launches:', sorted({k.split(' MxNxK=')[0] for k in keys}))
    # every listed kernel family launched: the case tests the forms the step runs, not a fallback
    missing = [f for f in case['kernels'][precision] if not any(k.startswith(f) for k in keys)]
    assert not missing, (case['id'], precision, missing, sorted(set(keys)))
    over = [(what, mine / max(theirs, 1e-300)) for what, mine, theirs, out in report if out]
    if over:
        raise FormOverBudget(over)


def _step_launches(dev, precision):
    import numpy as np
    import os
    from conftest import GOLDEN
    from oracle.weights import seeded_input
    from test_esrgan_gpu import make_trainer
    gold = np.load(os.path.join(GOLDEN, 'esrgan.npz'))
    s_lr, s_hr = (int(v) for v in gold['b4_seeds'])
    lr = seeded_input((4, 3, 32, 32), s_lr).repeat(4, 1, 1, 1).to(dev)
    hr = seeded_input((4, 3, 128, 128), s_hr).repeat(4, 1, 1, 1).to(dev)
    t = make_trainer(dev, batch=16, disable_amp=precision == 'fp32', use_graphs=False)
    t.overlap_branches = False  # bench.py's instrumented pass: one stream
    return set(prof_keys(lambda: t.gan_step(lr, hr), aux=True))


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_esrgan_step_launches_are_covered(dev, monkeypatch, precision):
    """One eager batch-16 ESRGAN GAN step with the launch records on: every conv launch it makes (kernel, template arguments, and
    MxNxK where the name carries it) is one some row of ESRGAN_STEP_CONVS made in this precision, or one of the fused dense
    block's / the pack launches held elsewhere (CONV_LAUNCHES_TESTED_ELSEWHERE).  The records do hold the launches the SRGAN
    step never makes."""
    import test_step_layers_gpu as T
    # (a row over its statistical budget must still run to its end here: its later launches count)
    monkeypatch.setattr(T, 'budget', lambda what, mine, theirs, f, report: None)
    step = _step_launches(dev, precision)
    assert any(k.startswith('wgrad_reduce_rows_kernel') for k in step), sorted(step)
    if precision == 'bf16':
        for fam in ('rdb_kernel<0>', 'rdb_kernel<1>', 'wgrad_rows_bf16_kernel<32>'):
            assert any(k.startswith(fam) for k in step), (fam, sorted(step))
    table = set()
    for case in ESRGAN_STEP_CONVS:
        if precision not in case['precisions']:
            continue

        def run(case=case):
            try:
                run_case(case, dev, [], precision)
            except AssertionError:  # (numerics are test_esrgan_conv_vs_fp64's business; here only the launches count)
                pass
        table |= set(prof_keys(run, aux=True))
    missing = sorted(k for k in step - table if not k.startswith(tuple(CONV_LAUNCHES_TESTED_ELSEWHERE)))
    assert not missing, missing
