"""Host-side operators: ``torch.autograd.Function`` wrappers around the C-ABI HIP kernels.

PyTorch is plumbing here (device memory via the caching allocator, the current
stream, the autograd tape); every device computation on the hot path is a
hand-written gfx950 kernel reached through ``_lib.call``.  Activations are NHWC
fp32 tensors ``[N, H, W, C_s]``; parameters keep the reference's layouts.

Nothing in this module falls back to CPU or to ATen kernels for the hot ops:
non-CUDA inputs raise.
"""
import contextlib
from typing import Optional, Tuple

import torch
from torch import Tensor
from torch.autograd import Function

from . import _dev, _lib
from ._lib import (ACT_LRELU, ACT_NONE, ACT_PRELU, ACT_RELU, HEAD_ESRGAN_D, HEAD_ESRGAN_G, HEAD_SRGAN_D, HEAD_SRGAN_G,  # noqa: F401
                   Conv2dDesc, call)

import ctypes as C


# When enabled (by the trainers, whose parameters' ``.grad`` are persistent views of one flat
# buffer) parameter gradients are accumulated straight into ``param.grad`` by the kernels and the
# Functions return ``None`` for them: no per-parameter AccumulateGrad add kernels (~200 per step).
direct_grads = [False]


def _sink(param: Optional[Tensor]) -> Optional[Tensor]:
    if not direct_grads[0] or param is None or not param.requires_grad or not param.is_leaf:
        return None  # (not a leaf: a spectrally normalised weight, whose gradient goes on through autograd)
    g = param.grad
    if g is None or not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous():
        return None
    return g


# Pause points of the backward pass.  A data-parallel trainer installs a ``ddp.BackwardCuts`` here so that
# ``loss.backward()`` stops where a gradient bucket is complete and the bucket's all-reduce can be launched
# before the rest of the backward pass is issued; without a hook a cut point is the identity.
cut_hook = [None]


def cut_point(name: str, t: Tensor) -> Tensor:
    hook = cut_hook[0]
    return t if hook is None else hook(name, t)


class WeightGradQueue:
    """Weight-gradient work of one backward pass, collected and issued together.

    Autograd reaches a conv's weight gradient right after its data gradient, one layer at a time, but nothing
    reads a weight gradient before the optimiser.  For the generator's 33 identical 3x3 64->64 convs a single
    problem is 0.68 GFLOP -- launched alone it is mostly pipeline fill plus a slab reduction -- so, while a queue
    is installed (``deferred_weight_grads``), the conv Functions only record ``(descriptor, x, dy, sink)`` and the
    queue hands every group of equal-geometry problems to ``srx_conv2d_bwd_weight_multi`` when it is flushed:
    one launch with long loops instead of 33 short ones.  Problems that share a sink (the discriminator's real
    and fake passes) become segments of one gradient.  Only gradients that accumulate straight into the flat
    ``.grad`` buffers are deferred; the queued tensors stay alive until the flush.
    """
    MAXP = 72  # WG_MAXP of wgrad.hip

    def __init__(self):
        self.groups = {}
        self.pairs = {}

    def add(self, d: Conv2dDesc, x_ptr: int, dy_ptr: int, sink_ptr: int, bias_ptr, keep, scale: float = 1.0) -> None:
        """``scale``: the tensor at ``dy_ptr`` stands for ``scale * dy`` (one value per sink)."""
        key = tuple(getattr(d, f) for f, _ in Conv2dDesc._fields_)
        self.groups.setdefault(key, [d, []])[1].append((x_ptr, dy_ptr, sink_ptr, bias_ptr or 0, keep, float(scale)))

    def add_pair(self, d: Conv2dDesc, cin_lo: int, x_ptr: int, dy_ptr: int, sinks, bias_sinks, keep) -> None:
        """Two convs that read the same input buffer and whose output gradients are adjacent channel slices, as ONE
        problem (``srx_conv2d_bwd_weight_multi_pair``): ``sinks`` / ``bias_sinks`` are (first conv, second conv)."""
        key = ('pair', cin_lo, bias_sinks is None) + tuple(getattr(d, f) for f, _ in Conv2dDesc._fields_)
        self.pairs.setdefault(key, [d, cin_lo, []])[2].append((x_ptr, dy_ptr, sinks, bias_sinks, keep))

    def _flush_pairs(self) -> None:
        pairs, self.pairs = self.pairs, {}
        L, s = _lib.lib(), _stream()
        arr = lambda vals: (C.c_void_p * len(vals))(*vals)  # noqa: E731
        for d, cin_lo, items in pairs.values():
            dref = C.byref(d)
            for i in range(0, len(items), self.MAXP):
                part = items[i:i + self.MAXP]
                n = len(part)
                nws = L.srx_conv2d_bwd_weight_multi_ws_floats(dref, n)
                ws = torch.empty(max(int(nws), 4), dtype=torch.float32, device=part[0][4][0].device)
                with_bias = part[0][3] is not None
                call('srx_conv2d_bwd_weight_multi_pair', dref, n, arr([p[0] for p in part]), arr([p[1] for p in part]),
                     arr([p[2][0] for p in part]), arr([p[2][1] for p in part]), cin_lo, 1,
                     arr([p[3][0] for p in part]) if with_bias else None, arr([p[3][1] for p in part]) if with_bias else None,
                     _p(ws), nws, s)

    def flush(self) -> None:
        if self.pairs:
            self._flush_pairs()
        groups, self.groups = self.groups, {}
        if not groups:
            return
        L, s = _lib.lib(), _stream()
        for d, items in groups.values():
            by_sink = {}
            for it in items:
                by_sink.setdefault((it[2], it[3]), []).append(it)
            by_count = {}
            for sink, its in by_sink.items():  # outputs with the same number of segments go into one launch
                by_count.setdefault(len(its), []).append((sink, its))
            dref = C.byref(d)
            for per_out, outs in by_count.items():
                step = max(1, self.MAXP // per_out)
                for i in range(0, len(outs), step):
                    part = outs[i:i + step]
                    probs = [it for _, its in part for it in its]
                    n = len(probs)
                    arr = lambda vals: (C.c_void_p * len(vals))(*vals)  # noqa: E731
                    xs, dys = arr([p[0] for p in probs]), arr([p[1] for p in probs])
                    dws, dbs = arr([sk[0] for sk, _ in part]), arr([sk[1] or None for sk, _ in part])
                    nws = L.srx_conv2d_bwd_weight_multi_ws_floats(dref, n)
                    ws = torch.empty(max(int(nws), 4), dtype=torch.float32, device=probs[0][4][0].device)
                    scales = [its[0][5] for _, its in part]
                    if any(its[k][5] != its[0][5] for _, its in part for k in range(len(its))):
                        raise RuntimeError('WeightGradQueue: the segments of one gradient must share their scale')
                    if all(v == 1.0 for v in scales):
                        call('srx_conv2d_bwd_weight_multi', dref, n, per_out, xs, dys, dws, 1, dbs, _p(ws), nws, s)
                    else:
                        call('srx_conv2d_bwd_weight_multi_scaled', dref, n, per_out, xs, dys, dws, 1, dbs,
                             (C.c_float * len(scales))(*scales), _p(ws), nws, s)


wgrad_queue = [None]


@contextlib.contextmanager
def deferred_weight_grads():
    """Collect the conv weight gradients of the backward passes run inside and issue them on exit."""
    q, old = WeightGradQueue(), wgrad_queue[0]
    wgrad_queue[0] = q
    try:
        yield q
    finally:
        wgrad_queue[0] = old
    q.flush()


def _stream() -> int:
    """The current stream's handle, ``torch.cuda.current_stream().cuda_stream`` without building the Stream object: 0.3 us
    instead of 2.6, which counts where a host-bound caller (a DeviceLoader batch) makes several launches."""
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def _p(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def _chk(t: Tensor, what: str) -> Tensor:
    if not t.is_cuda:
        raise RuntimeError(f'{what}: expected a tensor on the MI355X (cuda) device, got {t.device}; '
                           'torchsr_amd has no CPU fallback')
    if t.dtype != torch.float32:
        raise RuntimeError(f'{what}: expected float32, got {t.dtype}')
    return t if t.is_contiguous() else t.contiguous()


def _chk16(t: Tensor, what: str, dtype: Optional[torch.dtype] = torch.bfloat16) -> Tensor:
    """A 16-bit NHWC activation of the 16-bit-native inference chain (csrc/c64.hip): ``dtype`` (bf16 by default), or either
    storage type with ``dtype=None``."""
    if t.device.type != 'cuda':
        raise RuntimeError(f'{what}: the MI355X path needs a CUDA/HIP tensor, got {t.device} (no CPU fallback)')
    if t.dtype != dtype and not (dtype is None and t.dtype in _STORE16):
        raise RuntimeError(f'{what}: expected a {"bfloat16 or float16" if dtype is None else str(dtype)[6:]} tensor, got {t.dtype}')
    return t if t.is_contiguous() else t.contiguous()


# the 16-bit storage types of the inference chain: bf16 (precision 1 / 2) and fp16 (precision 3, inference only)
_STORE16 = (torch.bfloat16, torch.float16)
PRECISION_F16 = 3


def _chk_f16_inference(st, what: str) -> None:
    """Precision 3 (fp16 storage and products) exists for inference only: no autograd."""
    if st.precision == PRECISION_F16 and torch.is_grad_enabled():
        raise RuntimeError(f'{what}: fp16 precision (3) is inference-only; run it under torch.no_grad() on an eval-mode model')


def to_bf16(x: Tensor) -> Tensor:
    """fp32 -> bf16 (round to nearest even), same shape: the entry of the bf16-native inference chain."""
    x = _chk(x, 'to_bf16.input')
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    call('srx_f32_to_bf16', _p(x), _p(y), x.numel(), _stream())
    return y


def to_f16(x: Tensor) -> Tensor:
    """fp32 -> fp16 (round to nearest even; beyond 65519.99.. -> +-inf), same shape: the entry of the fp16 inference chain."""
    x = _chk(x, 'to_f16.input')
    y = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    call('srx_f32_to_f16', _p(x), _p(y), x.numel(), _stream())
    return y


def to_f32(x: Tensor) -> Tensor:
    """bf16 or fp16 -> fp32 (exact), same shape."""
    x = _chk16(x, 'to_f32.input', None)
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    call('srx_bf16_to_f32' if x.dtype == torch.bfloat16 else 'srx_f16_to_f32', _p(x), _p(y), x.numel(), _stream())
    return y


def conv2d_bf16in(conv, x: Tensor) -> Tensor:
    """The generator's 64 -> 3 output conv on a 16-bit input; fp32 out.  bf16: ``srx_conv2d_fwd_bf16in`` / the thin9 kernel
    (inference, precision 2).  fp16: the thin9 kernel's fp16 form only (precision 3: no other kernel multiplies fp16)."""
    st = conv._st
    x = _chk16(x, 'conv2d_bf16in.input', None)
    n, h, w, cs = x.shape
    f16 = x.dtype == torch.float16
    t9 = st.k == 9 and st.pad == 4 and st.stride == 1 and st.cin == 64 and st.cout <= 3 and not _dev.NO_T9
    if f16:
        _chk_f16_inference(st, 'conv2d_bf16in')
        if st.precision != PRECISION_F16 or not t9:
            raise RuntimeError('conv2d_bf16in: an fp16 input needs precision 3 and a 9x9 64 -> <= 3 channel layer on the thin9 '
                               'kernel (SRX_NO_T9 unset)')
    elif st.precision != 2 or torch.is_grad_enabled():
        return conv(to_f32(x))
    y = torch.empty(st.out_shape(n, h, w), dtype=torch.float32, device=x.device)
    b = None if conv.bias is None else _chk(conv.bias.detach(), 'conv2d.bias')
    if t9:
        # the taps as the GEMM's N (csrc/thin9.hip): 32x32x16 bf16 / fp16 MFMAs instead of 4x4x4.  The pack is keyed by the
        # storage type too: a bf16 call after an fp16 one must not read fp16 weights
        sfx = 'f16' if f16 else 'bf16'
        key = st.pack_key(conv.weight) + (None if b is None else (b.data_ptr(), conv.bias._version), x.dtype)
        st.thin9.ensure(key, x.device, False, lambda: (_lib.lib().srx_conv9x9_c64_thin_bf16_packed_bytes(), 0, torch.uint8),
                        lambda fwd, bwd, _: call(f'srx_conv9x9_c64_thin_{sfx}_pack', _p(_chk(conv.weight.detach(), 'conv2d.weight')),
                                                 _p(b), st.cout, _p(fwd), _stream()))
        call(f'srx_conv9x9_c64_thin_{sfx}_fwd', n, h, w, _p(x), _p(st.thin9.fwd), _p(y), _stream())
        return y
    d = st.desc(n, h, w)
    st.pack(conv.weight, d)
    call('srx_conv2d_fwd_bf16in', C.byref(d), _p(x), _p(st.wpk_fwd), _p(b), _p(y), _stream())
    return y


def _ws(n: int, like: Tensor) -> Tensor:
    return torch.empty(max(int(n), 4), dtype=torch.float32, device=like.device)


def round4(c: int) -> int:
    return (c + 3) // 4 * 4


# --------------------------------------------------------------------------- launchers
# The only places that size a conv, BatchNorm or colsum workspace and name these entry points.  Pointer arguments are raw
# (``_p(t)``, or ``t.data_ptr() + offset`` for a channel slice); ``like`` gives the workspace its device; ``s``: the stream.
def _conv_fwd(d: Conv2dDesc, x_ptr, w_ptr, b_ptr, y_ptr, like: Tensor, s, part_ptr=None, residual=None) -> None:
    """The direct conv forward; ``residual = (ptr, scale)``: ``y = conv * scale + residual`` in the epilogue."""
    dref = C.byref(d)
    nws = _lib.lib().srx_conv2d_fwd_ws_floats(dref)
    ws = _p(_ws(nws, like)) if nws else None
    if residual is None:
        call('srx_conv2d_fwd', dref, x_ptr, w_ptr, b_ptr, y_ptr, part_ptr, ws, nws, s)
    else:
        call('srx_conv2d_fwd_residual', dref, x_ptr, w_ptr, b_ptr, residual[0], residual[1], y_ptr, ws, nws, s)


def _wino_fwd(d: Conv2dDesc, x: Tensor, u: Tensor, b: Optional[Tensor], y: Tensor, part: Optional[Tensor], s) -> None:
    """The Winograd forward, with BatchNorm partial statistics when ``part`` is given."""
    dref = C.byref(d)
    nws = _lib.lib().srx_wino_ws_floats(dref, 0 if part is None else 2)
    ws = _p(_ws(nws, x)) if nws else None
    if part is None:
        call('srx_wino_fwd', dref, _p(x), _p(u), _p(b), _p(y), ws, nws, s)
    else:
        call('srx_wino_fwd_stats', dref, _p(x), _p(u), _p(b), _p(y), _p(part), ws, nws, s)


def _conv_dgrad(d: Conv2dDesc, dy_ptr, w_ptr, dx_ptr, like: Tensor, s, accumulate: int = 0, addend_ptr=None, mask=None,
                nws: Optional[int] = None) -> None:
    """The direct data gradient: plain / accumulating, ``+ addend``, or masked by ``(act_out_ptr, slope, c_lo, c_hi)``."""
    dref = C.byref(d)
    if nws is None:  # (a caller looping over equal layers sizes once and passes it in)
        nws = _lib.lib().srx_conv2d_bwd_data_ws_floats(dref)
    ws = _p(_ws(nws, like)) if nws else None
    if mask is not None:
        call('srx_conv2d_bwd_data_act', dref, dy_ptr, w_ptr, mask[0], mask[1], mask[2], mask[3], accumulate, dx_ptr, ws, nws, s)
    elif addend_ptr is not None:
        call('srx_conv2d_bwd_data_add', dref, dy_ptr, w_ptr, addend_ptr, dx_ptr, ws, nws, s)
    else:
        call('srx_conv2d_bwd_data', dref, dy_ptr, w_ptr, dx_ptr, accumulate, ws, nws, s)


def _layer_dgrad(st, d: Conv2dDesc, master: Tensor, wino: bool, wino_bwd: Optional[Tensor], wpk_bwd: Optional[Tensor], dy: Tensor,
                 x: Tensor, in_act, s) -> Tuple[Tensor, bool]:
    """``(dx, masked)`` of a layer that ran on Winograd or the direct kernel; ``masked``: the backward of ``in_act``, which made ``x``, is in."""
    dx = torch.empty_like(x)
    masked = in_act is not None
    if wino and (not masked or in_act.act == ACT_RELU) and wino_bwd is not None:
        dref = C.byref(d)
        nws = _lib.lib().srx_wino_ws_floats(dref, 1)
        call('srx_wino_bwd_data', dref, _p(dy), _p(wino_bwd), _p(x) if masked else None, _p(dx), _p(_ws(nws, x)) if nws else None,
             nws, s)
        return dx, masked
    if wino:  # (a Winograd forward whose data gradient takes the direct kernel: its packed copy is made now)
        st.pack(master, d)
        wpk_bwd = st.wpk_bwd
    mask = (_p(x), 0.0 if in_act.act == ACT_RELU else in_act.slope, 0, st.cin_s) if masked else None
    _conv_dgrad(d, _p(dy), _p(wpk_bwd), _p(dx), x, s, mask=mask)
    return dx, masked


def _conv_wgrad(d: Conv2dDesc, x_ptr, dy_ptr, dw: Optional[Tensor], sink: Optional[Tensor], b_ptr, keep, like: Tensor, s,
                scale: Optional[float] = None) -> None:
    """Weight (+ riding bias) gradient: accumulated into ``sink`` -- queued, with ``keep``, under a queue -- or written to ``dw``."""
    queue = wgrad_queue[0]
    if queue is not None and sink is not None:
        queue.add(d, x_ptr, dy_ptr, _p(sink), b_ptr, keep, 1.0 if scale is None else scale)
        return
    dref = C.byref(d)
    nws = _lib.lib().srx_conv2d_bwd_weight_ws_floats(dref)
    ws = _ws(nws, like)
    out, acc = (_p(dw), 0) if sink is None else (_p(sink), 1)
    if scale is None:
        call('srx_conv2d_bwd_weight', dref, x_ptr, dy_ptr, out, acc, b_ptr, _p(ws), nws, s)
    else:
        one = lambda v: (C.c_void_p * 1)(v)  # noqa: E731
        call('srx_conv2d_bwd_weight_multi_scaled', dref, 1, 1, one(x_ptr), one(dy_ptr), one(out), acc, one(b_ptr),
             (C.c_float * 1)(scale), _p(ws), nws, s)


def _colsum(src_ptr, rows: int, cols: int, ld: int, out: Tensor, accumulate: int, like: Tensor, s) -> None:
    """Column sums of a ``rows x cols`` matrix (row stride ``ld``) written or accumulated into ``out``."""
    nws = _lib.lib().srx_colsum_ws_floats(rows, cols)
    call('srx_colsum', src_ptr, _p(out), rows, cols, ld, accumulate, _p(_ws(nws, like)), nws, s)


def _conv_param_grads(st, d: Conv2dDesc, x_ptr, dy_ptr, dy_rows: int, dy_ld: int, wparam: Optional[Tensor], bparam: Optional[Tensor],
                      keep, like: Tensor, s, scale: Optional[float] = None):
    """``(dw, db)`` of one conv for autograd, ``None`` where the parameter is ``None`` (no gradient wanted) or its ``.grad`` took it."""
    dev = like.device
    dw = db = sink = b_ptr = None
    if wparam is not None:
        sink = _sink(wparam)
        if sink is None:
            dw = torch.empty((st.cout, st.cin, st.k, st.k), dtype=torch.float32, device=dev)
        # the bias gradient rides along in the weight-gradient kernel (it stages every dy row anyway) when both results go
        # the same way: both accumulated into .grad, or both returned (PixelShuffle layers too: the reduction maps packed
        # columns back)
        if bparam is not None:
            bsink = _sink(bparam)
            if (bsink is None) == (sink is None):
                if bsink is None:
                    db = torch.empty(st.cout, dtype=torch.float32, device=dev)
                b_ptr = _p(db if bsink is None else bsink)
                bparam = None
    if bparam is not None and scale is not None:
        raise RuntimeError('conv gradients: with a scale the bias gradient must ride in the weight-gradient kernel (weight and '
                           'bias both with a gradient sink, or both without)')
    if wparam is not None:
        _conv_wgrad(d, x_ptr, dy_ptr, dw, sink, b_ptr, keep, like, s, scale)
    if bparam is None:
        return dw, db
    if st.shuffle:
        # dy is [N, 2Ho, 2Wo, cps]; bias index co = c*4 + i*2 + j
        w2, cps = st.out_shape(d.N, d.H, d.W)[2], dy_ld
        cols = 2 * w2 * cps
        t = torch.empty(cols, dtype=torch.float32, device=dev)
        _colsum(dy_ptr, dy_rows // (2 * w2), cols, cols, t, 0, like, s)
        # t is [i][wo][j][c]; fold wo (tiny tensor, plumbing) and permute to (c,i,j)
        return dw, t.view(2, w2 // 2, 2, cps).sum(1).permute(2, 0, 1).reshape(-1)[:st.cout].contiguous()
    bsink = _sink(bparam)
    if bsink is None:
        db = torch.empty(st.cout, dtype=torch.float32, device=dev)
    _colsum(dy_ptr, dy_rows, st.cout, dy_ld, db if bsink is None else bsink, 0 if bsink is None else 1, like, s)
    return dw, db


def _bn_train_fwd(y: Tensor, part: Tensor, m: int, c: int, groups: int, bn_eps: float, momentum: Optional[float], gamma: Tensor,
                  beta: Tensor, residual: Optional[Tensor], out: Tensor, act: int, slope: float, prelu: Optional[Tensor],
                  running_mean, running_var, nbt, s) -> Tuple[Tensor, Tensor]:
    """``out = act(BatchNorm(y)) [+ residual]`` from the partial statistics ``part``; returns the batch ``(mean, invstd)``."""
    mean = torch.empty(groups * c, dtype=torch.float32, device=y.device)
    invstd = torch.empty(groups * c, dtype=torch.float32, device=y.device)
    call('srx_bn_train_fwd', _p(y), _p(part), part.shape[0], m, c, groups, bn_eps, 0.1 if momentum is None else momentum, _p(gamma.detach()),
         _p(beta.detach()), _p(residual), _p(out), act, slope, _p(prelu), _p(mean), _p(invstd), _p(running_mean), _p(running_var), _p(nbt), s)
    return mean, invstd


def _bn_act_bwd(dout: Tensor, y: Tensor, mean: Tensor, invstd: Tensor, gamma: Tensor, beta: Tensor, prelu: Optional[Tensor], m: int,
                c: int, groups: int, act: int, slope: float, training: bool, sinks, s, want_dy: bool = True):
    """``(dy, sums)`` of ``act(BatchNorm(y))``; ``sinks``: the ``.grad`` of gamma, beta and the PReLU slope, or ``None`` each."""
    sums = torch.empty(groups * (2 * c + 4), dtype=torch.float32, device=y.device)
    nws = _lib.lib().srx_bn_bwd_ws_floats(m, c)
    dy = torch.empty_like(y) if want_dy else None
    call('srx_bn_act_bwd', _p(dout), _p(y), _p(mean), _p(invstd), _p(gamma.detach()), _p(beta.detach()), _p(sums), _p(dy), m, c, groups, act, slope,
         _p(prelu), 1 if training else 0, _p(sinks[0]), _p(sinks[1]), _p(sinks[2]), _p(_ws(nws, y)), nws, s)
    return dy, sums


# --------------------------------------------------------------------------- layout
class _ToNHWC(Function):
    @staticmethod
    def forward(ctx, x: Tensor, cs: int) -> Tensor:
        ctx.set_materialize_grads(False)
        x = _chk(x, 'to_nhwc')
        n, c, h, w = x.shape
        ctx.c = c
        y = torch.empty((n, h, w, cs), dtype=torch.float32, device=x.device)
        call('srx_nchw_to_nhwc', _p(x), _p(y), n, c, h, w, cs, _stream())
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        dy = _chk(dy, 'to_nhwc.bwd')
        n, h, w, cs = dy.shape
        dx = torch.empty((n, ctx.c, h, w), dtype=torch.float32, device=dy.device)
        call('srx_nhwc_to_nchw', _p(dy), _p(dx), n, ctx.c, h, w, cs, _stream())
        return dx, None


class _ToNCHW(Function):
    @staticmethod
    def forward(ctx, x: Tensor, c: int) -> Tensor:
        ctx.set_materialize_grads(False)
        x = _chk(x, 'to_nchw')
        n, h, w, cs = x.shape
        ctx.cs = cs
        y = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
        call('srx_nhwc_to_nchw', _p(x), _p(y), n, c, h, w, cs, _stream())
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        dy = _chk(dy, 'to_nchw.bwd')
        n, c, h, w = dy.shape
        dx = torch.empty((n, h, w, ctx.cs), dtype=torch.float32, device=dy.device)
        call('srx_nchw_to_nhwc', _p(dy), _p(dx), n, c, h, w, ctx.cs, _stream())
        return dx, None


def to_nhwc(x: Tensor, cs: Optional[int] = None) -> Tensor:
    """NCHW ``[N,C,H,W]`` -> NHWC ``[N,H,W,cs]`` (extra channels zero)."""
    return _ToNHWC.apply(x, round4(x.shape[1]) if cs is None else cs)


def to_nchw(x: Tensor, c: Optional[int] = None) -> Tensor:
    """NHWC ``[N,H,W,cs]`` -> NCHW ``[N,c,H,W]`` (drops padding channels)."""
    return _ToNCHW.apply(x, x.shape[3] if c is None else c)


def flatten_nchw(x: Tensor) -> Tensor:
    """``torch.flatten(out, 1)`` of the reference (srgan/discriminator.py:86): (c,h,w) order."""
    return to_nchw(x).reshape(x.shape[0], -1)


def dihedral_inverse(k: int) -> int:
    """The group element that undoes ``dihedral(., k)``.  ``k``: bit 0 transpose, bit 1 horizontal flip, bit 2 vertical flip,
    the transpose applied first.  Flips are their own inverses and commute; a transpose turns a horizontal flip into a
    vertical one, ``(V^c H^b Tr)^-1 = Tr H^b V^c = V^b H^c Tr``: with bit 0 set, bits 1 and 2 change places."""
    if not isinstance(k, int) or not 0 <= k <= 7:
        raise ValueError(f'dihedral_inverse: k must be an int in 0..7, got {k!r}')
    return k if not k & 1 else 1 | (k & 2) << 1 | (k & 4) >> 1


def dihedral(x: Tensor, k: int, out: Optional[Tensor] = None, alpha: float = 1.0, beta: float = 0.0) -> Tensor:
    """``out = alpha * T_k(x) + beta * out`` on an NCHW tensor, ``T_k`` one of the eight flips / transposes of the last two
    dimensions (``srx_dihedral_planes``; ``dihedral_inverse`` names the bits).  ``out`` is allocated when None (``beta``
    must then be 0: there is nothing to add to) and is [N, C, W, H] for a transposing ``k``.  Inference only."""
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError('dihedral: inference-only (no backward); run it under torch.no_grad()')
    if not isinstance(k, int) or not 0 <= k <= 7:
        raise ValueError(f'dihedral: k must be an int in 0..7, got {k!r}')
    if x.dim() != 4:
        raise ValueError(f'dihedral: expected an NCHW tensor, got shape {tuple(x.shape)}')
    x = _chk(x, 'dihedral.input')
    n, c, h, w = x.shape
    shape = (n, c, w, h) if k & 1 else (n, c, h, w)
    if out is None:
        if beta != 0.0:
            raise ValueError('dihedral: beta != 0 needs the tensor to add to (out=)')
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    else:
        if _chk(out, 'dihedral.out') is not out:
            raise RuntimeError('dihedral: out must be contiguous')
        if tuple(out.shape) != shape or out.device != x.device:
            raise ValueError(f'dihedral: k = {k} maps {tuple(x.shape)} to {shape}, out is {tuple(out.shape)} on {out.device}')
    call('srx_dihedral_planes', _p(x), _p(out), n * c, h, w, k, float(alpha), float(beta), _stream())
    return out


RESAMPLE_MAX_REDUCTION = 16  # n_in <= 16 * n_out: at most 4 * 16 + 2 = 66 taps (srx_resample_planes' limit)


def resample_tables(n_in: int, n_out: int, dtype='float32'):
    """``(start, weight, K)`` of one axis of the antialiased Keys bicubic (a = -0.5) -- PIL's ``BICUBIC``,
    ``F.interpolate(mode='bicubic', antialias=True, align_corners=False)``, the filter ``srx_bicubic_down`` reduces the
    training data with -- from ``n_in`` to ``n_out`` samples: output ``i`` is ``sum_t weight[i, t] * in[start[i] + t]``.
    ``start``: int32 ``[n_out]``; ``weight``: ``[n_out, K]``, ``K`` the largest tap count, rows padded with 0.

    With ``scale = n_in / n_out``, ``support = 2 * max(scale, 1)`` and ``inv = 1 / max(scale, 1)`` the taps of output ``i``
    are ``lo <= j < hi``, ``c = scale * (i + 0.5)``, ``lo = max(0, int(c - support + 0.5))``, ``hi = min(n_in, int(c +
    support + 0.5))``, weighted ``keys((j - c + 0.5) * inv)`` over their sum.  Built in fp64 with numpy, each row normalised
    in fp64 and rounded once to ``dtype`` (``'float64'``: not at all).  ``n_in == n_out`` is the identity."""
    import numpy as np
    for name, v in (('n_in', n_in), ('n_out', n_out)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f'resample_tables: {name} must be a positive int, got {v!r}')
    if n_in > RESAMPLE_MAX_REDUCTION * n_out:
        raise ValueError(f'resample_tables: {n_in} -> {n_out} reduces by more than {RESAMPLE_MAX_REDUCTION}:1')
    scale = n_in / n_out
    support, inv = (2.0 * scale, 1.0 / scale) if scale >= 1.0 else (2.0, 1.0)
    c = scale * (np.arange(n_out, dtype=np.float64) + 0.5)
    lo = np.maximum(0, np.trunc(c - support + 0.5).astype(np.int64))
    hi = np.minimum(n_in, np.trunc(c + support + 0.5).astype(np.int64))
    k = int((hi - lo).max())
    j = lo[:, None] + np.arange(k, dtype=np.int64)[None, :]
    x = np.abs((j - c[:, None] + 0.5) * inv)
    w = np.where(x < 1.0, ((1.5 * x - 2.5) * x) * x + 1.0, np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * -0.5, 0.0))
    w = np.where(j < hi[:, None], w, 0.0)
    w = w / w.sum(axis=1, keepdims=True)
    return lo.astype(np.int32), np.ascontiguousarray(w.astype(dtype)), k


_resample_cache = {}


def _resample_device_tables(n_in: int, n_out: int, device: torch.device):
    """``resample_tables`` on ``device`` (start int32, weight fp32), built and copied once per (n_in, n_out, device)."""
    key = (n_in, n_out, torch.device(device))
    hit = _resample_cache.get(key)
    if hit is None:
        start, weight, k = resample_tables(n_in, n_out)
        hit = _resample_cache[key] = (torch.from_numpy(start).to(device), torch.from_numpy(weight).to(device), k)
    return hit


def resize_bicubic_aa(x: Tensor, size: Tuple[int, int], out: Optional[Tensor] = None) -> Tensor:
    """An NCHW tensor resized to ``size = (OH, OW)`` with the antialiased Keys bicubic of ``resample_tables`` -- any mix of
    reduction (up to 16:1) and enlargement per axis -- in one ``srx_resample_planes`` call: two fp32 dot products per
    output, bit-reproducible.  ``size == (H, W)`` is the identity: ``x`` itself (copied into ``out`` when given), no launch.
    Inference only."""
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError('resize_bicubic_aa: inference-only (no backward); run it under torch.no_grad()')
    if x.dim() != 4:
        raise ValueError(f'resize_bicubic_aa: expected an NCHW tensor, got shape {tuple(x.shape)}')
    try:
        oh, ow = size
    except (TypeError, ValueError):
        raise ValueError(f'resize_bicubic_aa: size must be (OH, OW), got {size!r}') from None
    n, c, h, w = x.shape
    for name, v in (('OH', oh), ('OW', ow), ('H', h), ('W', w), ('N * C', n * c)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f'resize_bicubic_aa: {name} must be a positive int, got {v!r}')
    if h > RESAMPLE_MAX_REDUCTION * oh or w > RESAMPLE_MAX_REDUCTION * ow:  # before anything touches the device
        raise ValueError(f'resize_bicubic_aa: {(h, w)} -> {(oh, ow)} reduces an axis by more than {RESAMPLE_MAX_REDUCTION}:1')
    x = _chk(x, 'resize_bicubic_aa.input')
    shape = (n, c, oh, ow)
    if out is not None:
        if _chk(out, 'resize_bicubic_aa.out') is not out:
            raise RuntimeError('resize_bicubic_aa: out must be contiguous')
        if tuple(out.shape) != shape or out.device != x.device:
            raise ValueError(f'resize_bicubic_aa: the result is {shape} on {x.device}, out is {tuple(out.shape)} on {out.device}')
    if (oh, ow) == (h, w):
        return x if out is None else out.copy_(x)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    sy, wy, ky = _resample_device_tables(h, oh, x.device)
    sx, wx, kx = _resample_device_tables(w, ow, x.device)
    nws = n * c * oh * w
    ws = _ws(nws, x)
    call('srx_resample_planes', _p(x), _p(out), n * c, h, w, oh, ow, _p(sy), _p(wy), ky, _p(sx), _p(wx), kx, _p(ws), nws, _stream())
    return out


COLOR_FIX_MODES = ('wavelet', 'adain')
COLOR_FIX_MAX_LEVELS = 8  # radius 2^7 = 128


def _color_fix_operands(who: str, sr: Tensor, lr: Tensor, out: Optional[Tensor]):
    """The refusals shared by the two colour fixes, all before the device is touched; ``(sr, lr, out)`` with ``out`` allocated."""
    if torch.is_grad_enabled() and (sr.requires_grad or lr.requires_grad):
        raise RuntimeError(f'{who}: inference-only (no backward); run it under torch.no_grad()')
    if sr.dim() != 4 or lr.dim() != 4:
        raise ValueError(f'{who}: expected NCHW tensors, got shapes {tuple(sr.shape)} and {tuple(lr.shape)}')
    if tuple(sr.shape[:2]) != tuple(lr.shape[:2]):
        raise ValueError(f'{who}: sr and lr must agree in N and C, got {tuple(sr.shape)} and {tuple(lr.shape)}')
    if min(sr.shape) < 1 or min(lr.shape) < 1:
        raise ValueError(f'{who}: every dimension must be positive, got {tuple(sr.shape)} and {tuple(lr.shape)}')
    if sr.shape[2] * sr.shape[3] >= 2 ** 31 or lr.shape[2] * lr.shape[3] >= 2 ** 31:
        raise ValueError(f'{who}: a plane must stay below 2^31 elements, got {tuple(sr.shape)} and {tuple(lr.shape)}')
    operands = (('sr', sr), ('lr', lr)) + ((('out', out),) if out is not None else ())
    for name, t in operands:
        if not t.is_contiguous():
            raise RuntimeError(f'{who}: {name} must be contiguous')
    for name, t in operands:
        _chk(t, f'{who}.{name}')
    if lr.device != sr.device:
        raise ValueError(f'{who}: sr is on {sr.device}, lr on {lr.device}')
    if out is None:
        out = torch.empty_like(sr)
    elif tuple(out.shape) != tuple(sr.shape) or out.device != sr.device:
        raise ValueError(f'{who}: the result is {tuple(sr.shape)} on {sr.device}, out is {tuple(out.shape)} on {out.device}')
    return sr, lr, out


def color_fix_wavelet(sr: Tensor, lr: Tensor, levels: int = 5, out: Optional[Tensor] = None) -> Tensor:
    """StableSR's wavelet colour fix: the high frequencies of ``sr`` ([N,C,H,W]) on the low frequencies of ``lr`` ([N,C,h,w])
    enlarged to (H, W) with ``resize_bicubic_aa`` -- ``sr + B(U - sr)``, ``B`` the a-trous blurs with [1 2 1]^T [1 2 1] / 16 at
    the radii 1, 2, ..., 2^(levels - 1), replicate padding.  One ``srx_color_fix_wavelet_level`` launch per level behind the
    resize, the subtraction folded into the first and the addition into the last; fp32, bit-reproducible.  Inference only."""
    who = 'color_fix_wavelet'
    if isinstance(levels, bool) or not isinstance(levels, int) or not 1 <= levels <= COLOR_FIX_MAX_LEVELS:
        raise ValueError(f'{who}: levels must be an int in 1..{COLOR_FIX_MAX_LEVELS}, got {levels!r}')
    sr, lr, out = _color_fix_operands(who, sr, lr, out)
    n, c, h, w = sr.shape
    if lr.shape[2] > RESAMPLE_MAX_REDUCTION * h or lr.shape[3] > RESAMPLE_MAX_REDUCTION * w:
        raise ValueError(f'{who}: lr {tuple(lr.shape[2:])} is more than {RESAMPLE_MAX_REDUCTION}:1 larger than sr {(h, w)}')
    u = resize_bicubic_aa(lr, (h, w))
    s = _stream()
    # the levels between alternate between one workspace and U, which is free once level 0 has read it (lr itself when the sizes
    # are equal: then a second workspace)
    ws = [torch.empty_like(sr) if levels > 1 else None, u if u is not lr else torch.empty_like(sr) if levels > 2 else None]
    src = u
    for i in range(levels):
        last = i == levels - 1
        dst = out if last else ws[i & 1]
        call('srx_color_fix_wavelet_level', _p(src), _p(sr) if i == 0 else None, _p(sr) if last else None, _p(dst), n * c, h, w,
             1 << i, s)
        src = dst
    return out


def plane_moments(x: Tensor) -> Tensor:
    """``[N, C, 2]`` fp64: the mean and the unbiased variance (0 for a one-pixel plane) of every plane of an NCHW fp32 tensor,
    summed in fp64 in a fixed order (``srx_plane_moments``): bit-reproducible.  Inference only."""
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError('plane_moments: inference-only (no backward); run it under torch.no_grad()')
    if x.dim() != 4 or min(x.shape) < 1 or x.shape[2] * x.shape[3] >= 2 ** 31:
        raise ValueError(f'plane_moments: expected an NCHW tensor with planes of 1 .. 2^31 - 1 elements, got shape {tuple(x.shape)}')
    x = _chk(x, 'plane_moments.input')
    n, c, h, w = x.shape
    blocks = _lib.lib().srx_plane_moments_blocks(h, w)
    part = torch.empty(n * c * blocks * 2, dtype=torch.float64, device=x.device)
    stats = torch.empty((n, c, 2), dtype=torch.float64, device=x.device)
    call('srx_plane_moments', _p(x), n * c, h, w, _p(part), part.numel(), _p(stats), _stream())
    return stats


def color_fix_adain(sr: Tensor, lr: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """StableSR's AdaIN colour fix: every plane of ``sr`` ([N,C,H,W]) mapped to the mean and the standard deviation of the same
    plane of ``lr`` ([N,C,h,w], at its own size) -- ``fmaf(sr, s, b)``, ``s = sqrt(var_lr + 1e-5) / sqrt(var_sr + 1e-5)``,
    ``b = mean_lr - mean_sr * s`` from ``plane_moments`` in fp64, each rounded once to fp32 (``srx_color_fix_adain_apply``).
    Bit-reproducible.  Inference only."""
    sr, lr, out = _color_fix_operands('color_fix_adain', sr, lr, out)
    n, c, h, w = sr.shape
    m_sr, m_lr = plane_moments(sr), plane_moments(lr)
    call('srx_color_fix_adain_apply', _p(sr), _p(out), n * c, h, w, _p(m_sr), _p(m_lr), _stream())
    return out


RESIZE_MODES = ('area', 'bilinear', 'bicubic')


def resize_tables(n_in: int, n_out: int, mode: str, dtype='float32'):
    """``(start, weight, K)`` of one axis, in ``resample_tables``' format, of the three resizes Real-ESRGAN's degradation draws
    from: ``F.interpolate(mode=..., align_corners=False, antialias=False)`` from ``n_in`` to ``n_out`` samples.  With
    ``src = (i + 0.5) * n_in / n_out - 0.5``:

    ``'area'`` (adaptive average pooling): taps ``lo <= j < hi``, ``lo = i * n_in // n_out``, ``hi = ceil((i + 1) * n_in /
    n_out)`` in integer arithmetic, each weighted ``1 / (hi - lo)``.
    ``'bilinear'``: ``src = max(src, 0)``, ``i0 = min(floor(src), n_in - 1)``, taps ``i0, i0 + 1`` weighted ``1 - l, l`` with
    ``l = src - i0``; the resampler's own ``min(start + t, n_in - 1)`` is the upper clamp.
    ``'bicubic'``: Keys with a = -0.75 (torch's value; ``resample_tables`` has PIL's -0.5) on the taps ``floor(src) - 1 .. + 2``,
    each index clamped to ``[0, n_in - 1]``; ``start`` is the first clamped index and weights whose clamped indices coincide
    are added into one tap (the resampler clamps at the upper border only).

    Built in fp64 with numpy and rounded once to ``dtype``.  ``n_in == n_out`` is the identity in every mode."""
    import numpy as np
    for name, v in (('n_in', n_in), ('n_out', n_out)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f'resize_tables: {name} must be a positive int, got {v!r}')
    if mode not in RESIZE_MODES:
        raise ValueError(f'resize_tables: mode must be one of {RESIZE_MODES}, got {mode!r}')
    if n_in > RESAMPLE_MAX_REDUCTION * n_out:
        raise ValueError(f'resize_tables: {n_in} -> {n_out} reduces by more than {RESAMPLE_MAX_REDUCTION}:1')
    i = np.arange(n_out, dtype=np.int64)
    src = (i + 0.5) * (n_in / n_out) - 0.5
    if mode == 'area':
        start = (i * n_in) // n_out
        count = -((-(i + 1) * n_in) // n_out) - start
        k = int(count.max())
        w = np.where(np.arange(k)[None, :] < count[:, None], 1.0 / count[:, None], 0.0)
    elif mode == 'bilinear':
        src = np.maximum(src, 0.0)
        start = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
        lam = src - start
        k, w = 2, np.stack([1.0 - lam, lam], axis=1)
    else:
        a = -0.75
        f = np.floor(src)
        t = src - f
        inner = lambda x: ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0      # noqa: E731  |x| <= 1
        outer = lambda x: ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a  # noqa: E731  1 < |x| < 2
        taps = np.stack([outer(t + 1.0), inner(t), inner(1.0 - t), outer(2.0 - t)], axis=1)
        idx = np.clip(f.astype(np.int64)[:, None] - 1 + np.arange(4)[None, :], 0, n_in - 1)
        start = idx[:, 0]
        k, w = 4, np.zeros((n_out, 4), dtype=np.float64)
        for tap in range(4):
            np.add.at(w, (i, idx[:, tap] - start), taps[:, tap])
    if k > 4 * RESAMPLE_MAX_REDUCTION + 2:
        raise ValueError(f'resize_tables: {n_in} -> {n_out} ({mode}) needs {k} taps, srx_resample_planes takes 66')
    return start.astype(np.int32), np.ascontiguousarray(w.astype(dtype)), k


_resize_cache = {}


def _resize_device_tables(n_in: int, n_out: int, mode: str, device: torch.device):
    """``resize_tables`` on ``device`` (start int32, weight fp32), built and copied once per (n_in, n_out, mode, device)."""
    key = (n_in, n_out, mode, torch.device(device))
    hit = _resize_cache.get(key)
    if hit is None:
        start, weight, k = resize_tables(n_in, n_out, mode)
        hit = _resize_cache[key] = (torch.from_numpy(start).to(device), torch.from_numpy(weight).to(device), k)
    return hit


def resize(x: Tensor, size: Tuple[int, int], mode: str, out: Optional[Tensor] = None) -> Tensor:
    """An NCHW tensor resized to ``size = (OH, OW)`` as ``F.interpolate(x, size, mode=mode, align_corners=False)`` does without
    antialiasing, ``mode`` one of ``'area'``, ``'bilinear'``, ``'bicubic'`` (``resize_tables``) -- the resizes of the
    second-order degradation -- in one ``srx_resample_planes`` call: bit-reproducible.  ``size == (H, W)`` is the identity:
    ``x`` itself (copied into ``out`` when given), no launch.  No backward."""
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError('resize: no backward; run it under torch.no_grad()')
    if x.dim() != 4:
        raise ValueError(f'resize: expected an NCHW tensor, got shape {tuple(x.shape)}')
    if mode not in RESIZE_MODES:
        raise ValueError(f'resize: mode must be one of {RESIZE_MODES}, got {mode!r}')
    try:
        oh, ow = size
    except (TypeError, ValueError):
        raise ValueError(f'resize: size must be (OH, OW), got {size!r}') from None
    n, c, h, w = x.shape
    for name, v in (('OH', oh), ('OW', ow), ('H', h), ('W', w), ('N * C', n * c)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f'resize: {name} must be a positive int, got {v!r}')
    if h > RESAMPLE_MAX_REDUCTION * oh or w > RESAMPLE_MAX_REDUCTION * ow:  # before anything touches the device
        raise ValueError(f'resize: {(h, w)} -> {(oh, ow)} reduces an axis by more than {RESAMPLE_MAX_REDUCTION}:1')
    x = _chk(x, 'resize.input')
    shape = (n, c, oh, ow)
    if out is not None:
        if _chk(out, 'resize.out') is not out:
            raise RuntimeError('resize: out must be contiguous')
        if tuple(out.shape) != shape or out.device != x.device:
            raise ValueError(f'resize: the result is {shape} on {x.device}, out is {tuple(out.shape)} on {out.device}')
    if (oh, ow) == (h, w):
        return x if out is None else out.copy_(x)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    sy, wy, ky = _resize_device_tables(h, oh, mode, x.device)
    sx, wx, kx = _resize_device_tables(w, ow, mode, x.device)
    nws = n * c * oh * w
    ws = _ws(nws, x)
    call('srx_resample_planes', _p(x), _p(out), n * c, h, w, oh, ow, _p(sy), _p(wy), ky, _p(sx), _p(wx), kx, _p(ws), nws, _stream())
    return out


USM_MAX_KSIZE = 51  # srx_usm_sharpen's longest filter


def _usm_check_filter(ksize, sigma) -> None:
    import math
    if isinstance(ksize, bool) or not isinstance(ksize, int) or ksize < 3 or ksize > USM_MAX_KSIZE or ksize % 2 == 0:
        raise ValueError(f'usm: ksize must be an odd int in 3..{USM_MAX_KSIZE}, got {ksize!r}')
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not math.isfinite(sigma) or sigma <= 0:
        raise ValueError(f'usm: sigma must be a positive finite number, got {sigma!r}')


def usm_taps(ksize: int = 51, sigma: float = 8.0):
    """The 1-D Gaussian of the unsharp mask: ``g[i] ~ exp(-(i - r)^2 / (2 sigma^2))``, ``i = 0 .. ksize - 1``, ``r = ksize // 2``,
    normalised to sum 1 -- built in fp64 with numpy and rounded once to fp32.  The defaults are Real-ESRGAN's ``USMSharp``:
    radius 50 made odd, and the sigma ``cv2.getGaussianKernel(51, 0)`` derives, ``0.3 * ((ksize - 1) / 2 - 1) + 0.8 = 8``.
    ``sigma`` is always explicit and positive (OpenCV's fixed tables for small sizes with ``sigma <= 0`` are not restated)."""
    import numpy as np
    _usm_check_filter(ksize, sigma)
    d = np.arange(ksize, dtype=np.float64) - ksize // 2
    g = np.exp(-(d * d) / (2.0 * float(sigma) ** 2))
    return (g / g.sum()).astype(np.float32)


_usm_cache = {}


def _usm_device_taps(ksize: int, sigma: float, device: torch.device) -> Tensor:
    """``usm_taps`` on ``device``, built and copied once per (ksize, sigma, device)."""
    key = (ksize, float(sigma), torch.device(device))
    hit = _usm_cache.get(key)
    if hit is None:
        hit = _usm_cache[key] = torch.from_numpy(usm_taps(ksize, sigma)).to(device)
    return hit


def usm_sharpen(x: Tensor, ksize: int = 51, sigma: float = 8.0, weight: float = 0.5, threshold: float = 10.0,
                return_stages: bool = False):
    """Real-ESRGAN's ``USMSharp`` on an NCHW tensor in [0, 1], in one ``srx_usm_sharpen`` call (two launches): with ``G`` the
    separable reflect-padded correlation with ``usm_taps(ksize, sigma)``, ``blur = G(x)``, ``mask = |x - blur| * 255 >
    threshold``, ``soft = G(mask)``, ``out = x + soft * (clamp(x + weight * (x - blur), 0, 1) - x)``.  Returns a new tensor;
    ``return_stages=True`` returns ``(out, blur, mask)``.  Bit-reproducible.  No backward."""
    import math
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError('usm_sharpen: no backward; run it under torch.no_grad()')
    if x.dim() != 4:
        raise ValueError(f'usm_sharpen: expected an NCHW tensor, got shape {tuple(x.shape)}')
    _usm_check_filter(ksize, sigma)
    for name, v in (('weight', weight), ('threshold', threshold)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f'usm_sharpen: {name} must be a finite number, got {v!r}')
    n, c, h, w = x.shape
    if n * c < 1:
        raise ValueError(f'usm_sharpen: empty batch, shape {tuple(x.shape)}')
    if h <= ksize // 2 or w <= ksize // 2:
        raise ValueError(f'usm_sharpen: {h} x {w} planes: a {ksize}-tap reflect needs {ksize // 2 + 1} rows and columns')
    if n * c * h * w >= 1 << 31:
        raise ValueError(f'usm_sharpen: {tuple(x.shape)} holds 2^31 elements or more')
    x = _chk(x, 'usm_sharpen.input')
    taps = _usm_device_taps(ksize, sigma, x.device)
    out, blur, mask = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    call('srx_usm_sharpen', _p(x), _p(out), _p(blur), _p(mask), _p(taps), ksize, n * c, h, w, float(weight), float(threshold),
         _stream())
    return (out, blur, mask) if return_stages else out


_poisson_cache = {}


def poisson_tables(device) -> Tensor:
    """``degradation.poisson_table_words()`` on ``device`` (int32, 2.4 MB): the threshold tables ``srx_add_poisson_noise`` draws
    from, built and copied once per device."""
    key = torch.device(device)
    if key.type == 'cuda' and key.index is None:
        key = torch.device('cuda', torch.cuda.current_device())
    hit = _poisson_cache.get(key)
    if hit is None:
        from .degradation import poisson_table_words
        hit = _poisson_cache[key] = torch.from_numpy(poisson_table_words().copy()).to(key)
    return hit


def add_poisson_noise(x: Tensor, scale, gray, seed: int, quantize: bool = False):
    """Real-ESRGAN's Poisson (shot) noise on an ``[N, 3, H, W]`` tensor in [0, 1], in one ``srx_add_poisson_noise`` call (a clear
    and two launches): per sample, ``q`` the 8-bit level of a value, ``vals`` the number of distinct levels of the sample rounded
    up to a power of two, ``k ~ Poisson(q * vals / 255)``, ``out = x + scale[n] * (k / vals - q / 255)``; ``gray[n] != 0`` takes
    ``q`` from the BT.601 luma and gives the three channels one ``k`` per pixel; ``scale[n] == 0`` copies the sample.  ``scale``
    (float32 ``[N]``) and ``gray`` (int32 ``[N]``) are tensors on ``x``'s device or anything ``torch.as_tensor`` takes; ``seed``
    is the 64-bit Philox key (counter ``(pixel, sample, 1, 0)``: another stream than ``srx_add_gaussian_noise``'s with the same
    seed).  ``quantize`` clamps to [0, 1] and rounds to 8 bits.  Returns ``(out, levels)``, ``levels`` int32 ``[N, 8]`` the
    256-bit mask of the levels each sample holds.  Bit-reproducible.  No backward."""
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError('add_poisson_noise: no backward; run it under torch.no_grad()')
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f'add_poisson_noise: expected an [N, 3, H, W] tensor, got shape {tuple(x.shape)}')
    n, _, h, w = x.shape
    if n < 1 or n > 65535 or h < 1 or w < 1:
        raise ValueError(f'add_poisson_noise: N must be in 1..65535 and the planes non-empty, got shape {tuple(x.shape)}')
    if h * w >= 1 << 31:
        raise ValueError(f'add_poisson_noise: {h} x {w} planes hold 2^31 elements or more')
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
        raise ValueError(f'add_poisson_noise: seed must be an int in 0..2^64 - 1, got {seed!r}')
    scale = torch.as_tensor(scale, dtype=torch.float32)
    gray = torch.as_tensor(gray, dtype=torch.int32)
    if tuple(scale.shape) != (n,) or tuple(gray.shape) != (n,):
        raise ValueError(f'add_poisson_noise: scale and gray must have shape ({n},), got {tuple(scale.shape)} and {tuple(gray.shape)}')
    x = _chk(x, 'add_poisson_noise.input')
    scale, gray = scale.to(x.device).contiguous(), gray.to(x.device).contiguous()
    tables = poisson_tables(x.device)
    out = torch.empty_like(x)
    levels = torch.empty((n, 8), dtype=torch.int32, device=x.device)
    call('srx_add_poisson_noise', _p(x), _p(out), _p(scale), _p(gray), _p(tables), _p(levels), seed & 0xFFFFFFFF, seed >> 32,
         n, h, w, int(bool(quantize)), _stream())
    return out, levels


def pool_exchange(pool_lr: Tensor, pool_hr: Optional[Tensor], lr: Tensor, hr: Optional[Tensor], slots, exchange: bool = True):
    """Real-ESRGAN's training pair pool in one ``srx_pool_exchange`` launch: sample ``i`` of the batch ``(lr, hr)`` and slot
    ``slots[i]`` of the pool ``(pool_lr, pool_hr)`` change places IN PLACE (``exchange=True``), or the sample is stored in the slot
    and the batch left as it is (``exchange=False``, while a pool fills).  ``pool_*`` are ``[cap, ...]``, the batch tensors
    ``[n, ...]`` with the same per-sample shape, ``n <= cap``; ``slots`` is a host sequence of ``n`` distinct ints in
    ``[0, cap)``.  Both sides move in the same launch, so a low-resolution sample and its target never part; ``pool_hr`` and
    ``hr`` may both be None (one tensor only).  Everything is checked on the host before the device is touched.  Returns
    ``(lr, hr)``, the same tensors, now holding the dequeued pairs.  Moves bits only.  No backward."""
    if (pool_hr is None) != (hr is None):
        raise ValueError('pool_exchange: pool_hr and hr must both be given or both be None')
    sides = [('lr', pool_lr, lr)] + ([('hr', pool_hr, hr)] if hr is not None else [])
    for name, pool, batch in sides:
        for what, t in ((f'pool_{name}', pool), (name, batch)):
            if not isinstance(t, Tensor):
                raise ValueError(f'pool_exchange: {what} must be a tensor, got {type(t).__name__}')
            if t.requires_grad:
                raise RuntimeError(f'pool_exchange: no backward; {what} requires grad')
            if t.dtype != torch.float32:
                raise RuntimeError(f'pool_exchange: {what}: expected float32, got {t.dtype}')
            if not t.is_contiguous():
                raise RuntimeError(f'pool_exchange: {what} must be contiguous (it is moved in place), got strides {t.stride()}')
            if t.device != pool_lr.device:
                raise RuntimeError(f'pool_exchange: {what} is on {t.device}, pool_lr on {pool_lr.device}: one device for all')
        if pool.dim() < 2 or batch.dim() != pool.dim() or tuple(pool.shape[1:]) != tuple(batch.shape[1:]):
            raise ValueError(f'pool_exchange: pool_{name} {tuple(pool.shape)} and {name} {tuple(batch.shape)} must be [cap, ...] and '
                             f'[n, ...] with one per-sample shape')
    cap, n = int(pool_lr.shape[0]), int(lr.shape[0])
    if hr is not None and (int(pool_hr.shape[0]) != cap or int(hr.shape[0]) != n):
        raise ValueError(f'pool_exchange: the two sides must agree in capacity and batch size, got pools of {cap} and '
                         f'{int(pool_hr.shape[0])}, batches of {n} and {int(hr.shape[0])}')
    elems = [int(pool[0].numel()) if cap else 0 for _, pool, _ in sides] + [0]
    if n < 1 or n > 65535 or n > cap or elems[0] < 1 or (hr is not None and elems[1] < 1):
        raise ValueError(f'pool_exchange: the batch size must be in 1..65535 and at most the capacity, the samples non-empty; got '
                         f'batch {n}, capacity {cap}, {elems[0]} and {elems[1]} values per sample')
    if cap * max(elems) >= 1 << 31:
        raise ValueError(f'pool_exchange: a pool of {cap} x {max(elems)} values holds 2^31 or more')
    slots = list(slots)
    if len(slots) != n:
        raise ValueError(f'pool_exchange: {len(slots)} slots for a batch of {n}')
    for s in slots:
        if isinstance(s, bool) or not isinstance(s, int) or not 0 <= s < cap:
            raise ValueError(f'pool_exchange: every slot must be an int in [0, {cap}), got {s!r}')
    if len(set(slots)) != n:
        raise ValueError(f'pool_exchange: the slots must be distinct, got {slots}')
    _chk(pool_lr, 'pool_exchange.pool_lr')  # the device: no CPU fallback
    slots_dev = torch.tensor(slots, dtype=torch.int32).to(lr.device)
    call('srx_pool_exchange', _p(pool_lr), _p(lr), elems[0], _p(pool_hr), _p(hr), elems[1], _p(slots_dev), n, cap,
         int(bool(exchange)), _stream())
    return lr, hr


# The launchers of the device data path (dataset.DeviceLoader): one per srx_* call a batch makes.  A batch is host-bound, so they
# check shapes on the host and copy nothing: the per-sample tables arrive on the device, laid out as the kernels read them.
def _chk_image(who: str, x: Tensor, channels: Optional[int] = 3) -> None:
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError(f'{who}: no backward; run it under torch.no_grad()')
    shape = x.shape
    if len(shape) != 4 or (channels is not None and shape[1] != channels):
        raise ValueError(f'{who}: expected an [N, {channels or "C"}, H, W] tensor, got shape {tuple(shape)}')


def _chk_table(who: str, name: str, t: Tensor, shape: tuple, dtype: torch.dtype, x: Tensor) -> None:
    if t.shape != shape or t.dtype is not dtype or t.get_device() != x.get_device() or not t.is_contiguous():
        raise ValueError(f'{who}: {name} must be a contiguous {str(dtype)[6:]} tensor of shape {shape} on {x.device}, got '
                         f'{str(t.dtype)[6:]} {tuple(t.shape)} on {t.device}')


def _chk_seed(who: str, seed) -> None:
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
        raise ValueError(f'{who}: seed must be an int in 0..2^64 - 1, got {seed!r}')


def crop_flip(images, meta, crop: int) -> Tensor:
    """The crops of a batch as float NCHW in [0, 1] (ToTensor), in one ``srx_crop_flip_u8`` launch: ``images`` are the uint8
    ``[H, W, 3]`` device tensors of the samples, ``meta`` their host rows ``{H, W, top, left, hflip, vflip}`` -- uploaded here, with
    the image addresses, in two small copies.  Every crop must lie inside its image."""
    n = len(images)
    meta_t = torch.tensor(meta, dtype=torch.int32)
    if n < 1 or meta_t.shape != (n, 6):
        raise ValueError(f'crop_flip: expected one row {{H, W, top, left, hflip, vflip}} per image, got {n} images and {meta!r}')
    dev, where = images[0].device, images[0].get_device()
    for im, (h, w, top, left, _, _) in zip(images, meta):
        if im.shape != (h, w, 3) or im.dtype is not torch.uint8 or im.get_device() != where or not im.is_contiguous():
            raise ValueError(f'crop_flip: expected contiguous uint8 [{h}, {w}, 3] images on {dev}, got {im.dtype} '
                             f'{tuple(im.shape)} on {im.device}')
        if not (0 <= top <= h - crop and 0 <= left <= w - crop):
            raise ValueError(f'crop_flip: a crop of {crop} at ({top}, {left}) leaves the {h} x {w} image')
    if dev.type != 'cuda':
        raise RuntimeError(f'crop_flip: expected images on the MI355X (cuda) device, got {dev}; torchsr_amd has no CPU fallback')
    ptrs = torch.tensor([im.data_ptr() for im in images], dtype=torch.int64).to(dev)
    meta_t = meta_t.to(dev)
    out = torch.empty((n, 3, crop, crop), dtype=torch.float32, device=dev)
    call('srx_crop_flip_u8', _p(ptrs), _p(meta_t), _p(out), n, crop, _stream())
    return out


def bicubic_down(x: Tensor, up: int, quantize: bool) -> Tensor:
    """``x`` reduced by the integer factor ``up`` with the antialiased Keys bicubic of PIL's BICUBIC, in one ``srx_bicubic_down``
    launch; ``quantize`` clamps to [0, 1] and rounds to 8 bits, as the PIL image does.  No backward."""
    _chk_image('bicubic_down', x, None)
    if isinstance(up, bool) or not isinstance(up, int) or up < 1:
        raise ValueError(f'bicubic_down: up must be a positive int, got {up!r}')
    x = _chk(x, 'bicubic_down.input')
    n, c, h, w = x.shape
    out = torch.empty((n, c, h // up, w // up), dtype=torch.float32, device=x.device)
    call('srx_bicubic_down', _p(x), _p(out), n, c, h, w, up, int(bool(quantize)), _stream())
    return out


def blur_aniso(x: Tensor, parm: Tensor, ksize: Tensor) -> Tensor:
    """Each sample of ``x`` (``[N, 3, H, W]``) blurred with its own rotated Gaussian, reflect-padded, in one ``srx_blur_aniso``
    launch: ``parm`` float32 ``[N, 4]`` = {sigma_x, sigma_y, theta, 0}, ``ksize`` int32 ``[N]`` (odd, up to 21; 0 copies), both on
    ``x``'s device.  No backward."""
    _chk_image('blur_aniso', x)
    n, c, h, w = x.shape
    _chk_table('blur_aniso', 'parm', parm, (n, 4), torch.float32, x)
    _chk_table('blur_aniso', 'ksize', ksize, (n,), torch.int32, x)
    x = _chk(x, 'blur_aniso.input')
    out = torch.empty_like(x)
    call('srx_blur_aniso', _p(x), _p(out), _p(parm), _p(ksize), n, c, h, w, _stream())
    return out


def filter2d(x: Tensor, weights: Tensor, ksize: Tensor, quantize: bool) -> Tensor:
    """Each sample of ``x`` (``[N, 3, H, W]``) correlated with its own kernel, reflect-padded, in one ``srx_filter2d`` launch:
    ``weights`` float32 ``[N, 21, 21]`` (``degradation.kernel_slot``), ``ksize`` int32 ``[N]`` (0 copies), both on ``x``'s device;
    ``quantize`` clamps to [0, 1] and rounds to 8 bits.  No backward."""
    from .degradation import KERNEL_SLOT
    _chk_image('filter2d', x)
    n, c, h, w = x.shape
    _chk_table('filter2d', 'weights', weights, (n, KERNEL_SLOT, KERNEL_SLOT), torch.float32, x)
    _chk_table('filter2d', 'ksize', ksize, (n,), torch.int32, x)
    x = _chk(x, 'filter2d.input')
    out = torch.empty_like(x)
    call('srx_filter2d', _p(x), _p(out), _p(weights), _p(ksize), n, c, h, w, int(bool(quantize)), _stream())
    return out


def add_gaussian_noise(x: Tensor, sigma: Tensor, gray: Tensor, seed: int, quantize: bool = True) -> Tensor:
    """``x + sigma[n] * z`` on an ``[N, 3, H, W]`` tensor in one ``srx_add_gaussian_noise`` launch, ``z`` standard normal from the
    64-bit Philox key ``seed``; ``gray[n] != 0`` gives the three channels of a pixel one ``z``.  ``sigma`` float32 ``[N]`` and
    ``gray`` int32 ``[N]`` are on ``x``'s device; ``quantize`` clamps to [0, 1] and rounds to 8 bits.  No backward."""
    _chk_image('add_gaussian_noise', x)
    n, _, h, w = x.shape
    _chk_table('add_gaussian_noise', 'sigma', sigma, (n,), torch.float32, x)
    _chk_table('add_gaussian_noise', 'gray', gray, (n,), torch.int32, x)
    _chk_seed('add_gaussian_noise', seed)
    x = _chk(x, 'add_gaussian_noise.input')
    out = torch.empty_like(x)
    call('srx_add_gaussian_noise', _p(x), _p(out), _p(sigma), _p(gray), seed & 0xFFFFFFFF, seed >> 32, n, h, w,
         int(bool(quantize)), _stream())
    return out


def jpeg_sim(x: Tensor, quality: Tensor, chroma420: Optional[Tensor] = None, quantize: bool = True) -> Tensor:
    """The JPEG round trip of an ``[N, 3, H, W]`` tensor of whole 8 x 8 blocks at the per-sample ``quality`` (int32 ``[N]`` on
    ``x``'s device; outside 1..100 copies): one ``srx_jpeg_sim`` launch (4:4:4), or -- with ``chroma420``, int32 ``[N]`` flags --
    ``srx_jpeg_sim2``, which stores the flagged samples' chroma 4:2:0; its workspace is taken per call (torch's caching allocator
    hands the same block back).  ``quantize`` rounds the result to 8 bits.  No backward."""
    _chk_image('jpeg_sim', x)
    n, _, h, w = x.shape
    _chk_table('jpeg_sim', 'quality', quality, (n,), torch.int32, x)
    if chroma420 is not None:
        _chk_table('jpeg_sim', 'chroma420', chroma420, (n,), torch.int32, x)
    x = _chk(x, 'jpeg_sim.input')
    out = torch.empty_like(x)
    if chroma420 is None:
        call('srx_jpeg_sim', _p(x), _p(out), _p(quality), n, h, w, int(bool(quantize)), _stream())
        return out
    nbytes = call('srx_jpeg_sim2_workspace', n, h, w)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    call('srx_jpeg_sim2', _p(x), _p(out), _p(quality), _p(chroma420), n, h, w, int(bool(quantize)), _p(ws), nbytes, None, _stream())
    return out


# --------------------------------------------------------------------------- conv2d
class WeightPack:
    """One packed layout of a layer's (or a chain of layers') weights: the forward buffer, the optional backward one, the key
    they were built from and, where the layout has one, the descriptor they were built with -- all ``None`` until built.
    ``ensure`` is THE rule for "is this copy current, and if not, what is allocated and packed"; it runs no device code of
    its own.  Once a buffer exists a repack writes into the same storage (pack tables and captured graphs hold its address)."""
    __slots__ = ('fwd', 'bwd', 'key', 'desc')

    def __init__(self):
        self.fwd = self.bwd = self.key = self.desc = None

    def ensure(self, key, device, need_bwd: bool, size, pack, desc=None) -> None:
        """``size() -> (fwd elements, bwd elements, dtype)``, asked only when the copies are not current; ``pack(fwd, bwd,
        bwd_only)`` writes the buffers it is given -- ``bwd_only``: ``fwd`` is current, only a backward copy is being added."""
        fresh = key == self.key and self.fwd is not None
        if fresh and (self.bwd is not None or not need_bwd):
            return
        n_fwd, n_bwd, dtype = size()
        if self.fwd is None or self.fwd.device != device or self.fwd.numel() != n_fwd or self.fwd.dtype != dtype:
            self.fwd, self.bwd, fresh = torch.empty(n_fwd, dtype=dtype, device=device), None, False
        if need_bwd and self.bwd is None:
            self.bwd = torch.empty(n_bwd, dtype=dtype, device=device)
        pack(self.fwd, self.bwd, fresh)
        self.key, self.desc = key, desc

    def stamp(self, key) -> None:
        """Record ``key`` without packing: someone else (``PackTable.run``) has just rewritten the buffers from it."""
        self.key = key


class ConvState:
    """Per-layer host state: geometry descriptors and packed weight copies."""

    def __init__(self, cin, cout, k, stride, pad, shuffle=0, act=ACT_NONE, slope=0.0, up=0):
        self.cin, self.cout, self.k, self.stride, self.pad = cin, cout, k, stride, pad
        self.shuffle, self.act, self.slope = shuffle, act, float(slope)
        self.up = 2 if up == 2 else 0  # nearest x2 upsampling of the input fused into the gather (srx_conv2d_t::up)
        self.cin_s = round4(cin)
        self.cout_s = round4(cout // 4) if shuffle else round4(cout)
        self._descs = {}
        self.model_epoch = [0]  # replaced by the owning FlatParams' counter
        self.precision = 0  # 1: bf16 products in the forward / stride-1 data gradient; 3: fp16 inference (srx_conv2d_t::precision)
        # (3 reaches srx_conv2d_* only for the <= 4-channel input conv; the 64-channel layers run the _f16 chain entry points)
        # the packed copies of the weights, one slot per kernel family that reads its own layout
        self.direct, self.wino, self.bf16s, self.thin9 = WeightPack(), WeightPack(), WeightPack(), WeightPack()
        # the slots' buffers under the names their readers use: aliases, set again after every ``ensure`` of the slot
        self.wpk_fwd = self.wpk_bwd = self.wino_fwd = self.wino_bwd = self.bf16s_fwd = self.bf16s_bwd = None
        self.fused_only = False  # set while the layer runs inside a fused multi-conv kernel that has its own weight stream
        # not False: the layer packs its own weights on every autograd forward (a trainable Unshuffle2Conv2d; then the buffer,
        # once it exists) and no pack table carries it
        self.own_pack = False

    def desc(self, n, h, w) -> Conv2dDesc:
        _chk_f16_inference(self, 'conv2d')
        d = self._descs.get((n, h, w, self.precision))
        if d is None:
            d = Conv2dDesc(n, h, w, self.cin, self.cin_s, self.cout, self.cout_s, self.k, self.k, self.stride,
                           self.pad, self.shuffle, self.act, self.slope, self.up, self.precision)
            self._descs[(n, h, w, self.precision)] = d
        return d

    def _out_hw(self, h, w):
        uf = 2 if self.up == 2 else 1
        return (uf * h + 2 * self.pad - self.k) // self.stride + 1, (uf * w + 2 * self.pad - self.k) // self.stride + 1

    def out_rows(self, n, h, w) -> int:
        """Rows of the output matrix (pixels the conv computes; before any PixelShuffle)."""
        ho, wo = self._out_hw(h, w)
        return n * ho * wo

    def out_shape(self, n, h, w):
        ho, wo = self._out_hw(h, w)
        return (n, 2 * ho, 2 * wo, self.cout_s) if self.shuffle else (n, ho, wo, self.cout_s)

    def pack_key(self, weight: Tensor):
        """What the packed copies were made from: the tensor, its in-place version, the global epoch (bumped
        when raw-pointer code may have changed any parameter) and the model's own epoch (bumped by its
        optimiser, ``optim.FlatParams.pack_epoch``).  Frozen parameters (VGG19) never repack."""
        if not weight.requires_grad:
            return (weight.data_ptr(), weight._version, -1, -1, self.precision)
        return (weight.data_ptr(), weight._version, _pack_epoch[0], self.model_epoch[0], self.precision)

    def pack(self, weight: Tensor, d: Conv2dDesc) -> None:
        """(Re)build the packed copies of the direct kernels when the master OIHW weight changed.  ``weight`` is the module's
        Parameter: its ``_version`` catches in-place torch updates, the optimiser epoch catches raw-pointer updates by
        ``srx_adam_step`` (frozen parameters such as VGG19's never repack)."""
        dref, L = C.byref(d), _lib.lib
        self.direct.ensure(
            self.pack_key(weight), weight.device, True,
            lambda: (L().srx_conv2d_packed_fwd_floats(dref), max(L().srx_conv2d_packed_bwd_floats(dref), 4), torch.float32),
            lambda fwd, bwd, _: call('srx_conv2d_pack', dref, _p(_chk(weight.detach(), 'conv2d.weight')), _p(fwd), _p(bwd), _stream()),
            d)
        self.wpk_fwd, self.wpk_bwd = self.direct.fwd, self.direct.bwd

    def pack_wino(self, weight: Tensor, d: Conv2dDesc, need_bwd: bool) -> None:
        """The Winograd-domain weights (``srx_wino_pack``: U = G g G^T of the layer and, for its data gradient, of the
        transposed / tap-flipped layer), rebuilt when the master weight changed -- same key as ``pack``."""
        dref = C.byref(d)

        def run(fwd, bwd, bwd_only):
            w = _chk(weight.detach(), 'conv2d.weight')
            if not bwd_only:
                call('srx_wino_pack', dref, _p(w), _p(fwd), 0, _stream())
            if bwd is not None:
                call('srx_wino_pack', dref, _p(w), _p(bwd), 1, _stream())

        self.wino.ensure(self.pack_key(weight), weight.device, need_bwd,
                         lambda: (_lib.lib().srx_wino_packed_floats(dref),) * 2 + (torch.float32,), run, d)
        self.wino_fwd, self.wino_bwd = self.wino.fwd, self.wino.bwd

    def pack_bf16s(self, weight: Tensor, d: Conv2dDesc, need_bwd: bool) -> None:
        """bf16 weight copies of a layer inside a bf16-storage stack (``srx_conv3x3_bf16s_pack``: one kernel writes both, so
        adding a backward copy rewrites the forward one with the same values), same key as ``pack``."""
        dref = C.byref(d)
        self.bf16s.ensure(
            self.pack_key(weight), weight.device, need_bwd,
            lambda: (_lib.lib().srx_conv3x3_bf16s_packed_bytes(dref) // 2,) * 2 + (torch.bfloat16,),
            lambda fwd, bwd, _: call('srx_conv3x3_bf16s_pack', dref, _p(_chk(weight.detach(), 'conv2d.weight')), _p(fwd), _p(bwd),
                                     _stream()), d)
        self.bf16s_fwd, self.bf16s_bwd = self.bf16s.fwd, self.bf16s.bwd


def wino_forward_only_ok(st: ConvState, d: Conv2dDesc) -> bool:
    """A sub-pixel conv (3x3 + nn.PixelShuffle(2), srgan/residual.py:27-28) in exact fp32: its FORWARD runs on Winograd with the
    shuffle in the store (csrc/wino.hip); its data gradient (a gather from the shuffled gradient) keeps the direct kernel."""
    return (not _dev.NO_WINO and st.shuffle == 2 and st.act == ACT_NONE and st.precision == 0
            and _lib.lib().srx_wino_infer_applicable(C.byref(d)) == 1)


def wino_layer_ok(st: ConvState, d: Conv2dDesc) -> bool:
    """Does this layer's forward (and data gradient) run on Winograd F(2x2, 3x3) (csrc/wino.hip) at this size?  Wide 3x3 /
    stride 1 / pad 1 fp32 layers without a fused LeakyReLU; small 64 -> 64 layers keep the row-tile kernel."""
    return (not _dev.NO_WINO and st.act in (ACT_NONE, ACT_RELU) and _lib.lib().srx_wino_applicable(C.byref(d)) == 1)


def wino_forward_runs(st: ConvState, d: Conv2dDesc, want_stats: bool) -> bool:
    """THE decision whether this forward call runs on the Winograd kernel -- shared by ``_Conv2d.forward`` and
    ``conv_stat_tile_rows`` so that the row granularity of a partial-statistics table is always the one of the kernel that
    writes it: the statistics epilogue exists for linear layers only (``srx_wino_fwd_stats``)."""
    return wino_layer_ok(st, d) and (not want_stats or st.act == ACT_NONE)


class PackTable:
    """Every conv of a model repacked by ONE launch after an optimiser step (``srx_pack_table_*``).

    Built once all layers have seen an input (their packed buffers and descriptors exist); the record
    table lives in device memory.  ``run()`` also stamps each layer's pack key, so the lazy per-layer
    ``ConvState.pack`` in the next forward finds nothing to do.
    """

    def __init__(self, convs):
        self.convs = list(convs)
        self.table = None
        self.nrec, self.maxn = 0, 0
        self.fused_sig = None
        self.generation = 0  # bumped by every (re)build

    def _build(self) -> bool:
        # (convs whose packed fp32 copies nothing reads -- dense blocks running as fused bf16 launches, RDBPack -- are left out)
        # ... and so is a layer that packs on every forward (a trainable Unshuffle2Conv2d: ``ConvState.own_pack``)
        every = [(c._st, c.weight) for c in self.convs
                 if c.weight.requires_grad and not c._st.fused_only and c._st.own_pack is False]
        # a layer is ready once it has run: it then has its direct packs (gconv / thin / row-tile kernels), its Winograd-domain
        # copies (wino.hip: such a layer needs no direct pack at all), or both (it took both paths at different sizes)
        direct = [(st, wt) for st, wt in every if st.direct.fwd is not None]
        wino = [(st, wt) for st, wt in every if st.wino.fwd is not None]
        if not direct or any(st.direct.fwd is None and st.wino.fwd is None for st, _ in every):
            return False
        items, n = direct, len(direct)
        descs = (Conv2dDesc * n)(*[st.direct.desc for st, _ in items])
        arr = lambda ptrs: (C.c_void_p * n)(*ptrs)  # noqa: E731
        w, f, b = (arr([wt.data_ptr() for _, wt in items]), arr([st.direct.fwd.data_ptr() for st, _ in items]),
                   arr([st.direct.bwd.data_ptr() for st, _ in items]))
        nbytes = _lib.lib().srx_pack_table_bytes(n + len(wino))
        host = torch.empty(nbytes, dtype=torch.uint8)
        nrec, maxn = C.c_int(0), C.c_longlong(0)
        call('srx_pack_table_build', descs, n, w, f, b, host.data_ptr(), C.byref(nrec), C.byref(maxn))
        # layers that run on Winograd: their transformed weights are refreshed by the same launch
        self.wino_items = wino
        for st, wt in self.wino_items:
            dref = C.byref(st.wino.desc)
            call('srx_pack_table_add_wino', host.data_ptr(), C.byref(nrec), C.byref(maxn), dref, wt.data_ptr(), st.wino.fwd.data_ptr(), 0)
            if st.wino.bwd is not None:
                call('srx_pack_table_add_wino', host.data_ptr(), C.byref(nrec), C.byref(maxn), dref, wt.data_ptr(), st.wino.bwd.data_ptr(), 1)
        self.table = host.to(items[0][1].device)
        self.items, self.nrec, self.maxn = items, nrec.value, maxn.value
        self.fused_sig = self._fused_signature()
        self.generation += 1
        return True

    def _fused_signature(self):
        """what decides the table's records: which convs are left out (fused dense blocks) and which carry Winograd copies"""
        return tuple((bool(c._st.fused_only), c._st.direct.fwd is not None, c._st.wino.fwd is not None, c._st.wino.bwd is not None)
                     for c in self.convs)

    def run(self) -> bool:
        """False (and nothing done) until every layer is ready: the lazy per-layer path still covers that."""
        # ``fused_only`` is re-decided per forward (precision, developer switch): a table built while the dense blocks ran
        # fused leaves their convs out, and would leave their fp32 packs stale after an optimiser step once they run unfused
        if self.table is not None and self.fused_sig != self._fused_signature():
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('PackTable: the set of fused-only convs changed inside a hipGraph capture; run one eager step '
                                   'after switching precision / SRX_NO_RDB_FUSED')
            self.table = None  # rebuilt below; ``generation`` tells holders of captured graphs to drop them
        if self.table is None and (torch.cuda.is_current_stream_capturing() or not self._build()):
            return False
        call('srx_pack_table_run', self.table.data_ptr(), self.nrec, self.maxn, _stream())
        for st, wt in self.items:
            st.direct.stamp(st.pack_key(wt))
        for st, wt in self.wino_items:
            st.wino.stamp(st.pack_key(wt))
        return True


# bumped by the optimiser (optim.FlatAdam.step) because a raw-pointer update does not
# touch ``Tensor._version``
_pack_epoch = [0]


def bump_pack_epoch() -> None:
    _pack_epoch[0] += 1


class ActFold:
    """Token that pairs a PRODUCER conv whose fused ReLU / LeakyReLU backward is skipped (``act_bwd_folded=token``) with the
    ONE consumer conv whose data gradient applies it instead (``in_act=token``: ``srx_conv2d_bwd_data_act``, mask = the
    consumer's input).  The consumer's backward marks the token; the producer's backward refuses to run with an unmarked
    one -- a producer output that reached another consumer, a consumer without an input gradient, or a consumer on a kernel
    without the masked epilogue would otherwise give silently wrong gradients."""
    __slots__ = ('act', 'slope', 'masked', 'consumers')

    def __init__(self, act: int, slope: float):
        self.act, self.slope, self.masked, self.consumers = act, float(slope), False, 0


class _Conv2d(Function):
    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, bias: Optional[Tensor], st: ConvState, want_stats: bool,
                master: Tensor, in_act: Optional[ActFold] = None, act_bwd_folded: Optional[ActFold] = None):
        # in_act: x is the output of a fused ReLU / LeakyReLU whose backward this conv's data gradient applies in its
        # epilogue (srx_conv2d_bwd_data_act, mask = x); the producer is called with the SAME token as act_bwd_folded
        # and skips the elementwise pass (a read of two tensors and a write of one, 226 MB for the discriminator's first
        # layer at batch 32).  Only for a producer whose output feeds this conv and nothing else (see ActFold).
        ctx.set_materialize_grads(False)
        if in_act is not None:
            if not isinstance(in_act, ActFold):
                raise TypeError('conv2d: in_act must be the ActFold token the producer was called with')
            in_act.consumers += 1
            if in_act.consumers > 1:
                raise RuntimeError('conv2d: an ActFold token has one consumer; this producer output feeds a second conv')
        if act_bwd_folded is not None and not isinstance(act_bwd_folded, ActFold):
            raise TypeError('conv2d: act_bwd_folded must be an ActFold token shared with the consumer')
        ctx.in_act, ctx.act_bwd_folded = in_act, act_bwd_folded
        x = _chk(x, 'conv2d.input')
        n, h, w, cs = x.shape
        if cs != st.cin_s:
            raise RuntimeError(f'conv2d: input has {cs} channels (stride), layer expects {st.cin_s}')
        d = st.desc(n, h, w)
        dref = C.byref(d)
        L = _lib.lib()
        y = torch.empty(st.out_shape(n, h, w), dtype=torch.float32, device=x.device)
        b = None if bias is None else _chk(bias.detach(), 'conv2d.bias')
        # wide 3x3 layers: Winograd F(2x2, 3x3), 2.25x fewer fp32 multiplications (csrc/wino.hip) -- the VGG19 features called
        # layer by layer, the discriminators' stride-1 layers (with the BatchNorm partial statistics in the epilogue)
        fwd_only = not want_stats and wino_forward_only_ok(st, d)
        ctx.wino = fwd_only or wino_forward_runs(st, d, want_stats)
        part = None
        if ctx.wino:
            # (trainable layers: PackTable refreshes the Winograd-domain weights inside the captured step)
            st.pack_wino(master, d, need_bwd=ctx.needs_input_grad[0] and not fwd_only)
            if want_stats:
                part = torch.empty((L.srx_wino_stat_rows(dref), st.cout, 2), dtype=torch.float32, device=x.device)
            _wino_fwd(d, x, st.wino_fwd, b, y, part, _stream())
        else:
            st.pack(master, d)
            if want_stats:
                rows = L.srx_conv2d_stat_rows(dref)
                part = torch.empty((rows, st.cout, 2), dtype=torch.float32, device=x.device)
            _conv_fwd(d, _p(x), _p(st.wpk_fwd), _p(b), _p(y), x, _stream(), part_ptr=_p(part))
        ctx.master = master
        ctx.st, ctx.d = st, d
        ctx.has_bias = bias is not None
        ctx.params = (weight, bias)
        ctx.save_for_backward(x, y if st.act != ACT_NONE else None)
        ctx.wpk_bwd = st.wpk_bwd
        ctx.sn_calls = getattr(st, 'sn_calls', None)  # (SNConvState: which normalised weight the packed copies hold)
        if want_stats:
            ctx.mark_non_differentiable(part)
            return y, part
        return y, None

    @staticmethod
    def backward(ctx, dy: Tensor, _dpart):
        st, d = ctx.st, ctx.d
        x, y = ctx.saved_tensors
        dy = _chk(dy, 'conv2d.grad')
        s = _stream()
        if ctx.act_bwd_folded is not None and not ctx.act_bwd_folded.masked:
            raise RuntimeError('conv2d: this layer\'s activation backward was handed to a consumer (ActFold) whose data '
                               'gradient never ran with the mask: the gradients would be wrong')
        if st.act != ACT_NONE and ctx.act_bwd_folded is None:
            g = torch.empty_like(dy)
            call('srx_act_bwd_from_out', _p(dy), _p(y), _p(g), dy.numel(), st.act, st.slope, s)
            dy = g
        dx = None
        if ctx.needs_input_grad[0] and ctx.sn_calls is not None and ctx.sn_calls != st.sn_calls:
            raise RuntimeError('conv2d: this spectrally normalised layer ran forward again before this backward: its one W_sn buffer '
                               'and packed copies now hold the later call\'s weight, and the input gradient would be taken through '
                               'it.  Run the backward of a call before the layer\'s next forward (or both inputs as one batch)')
        if ctx.needs_input_grad[0]:  # ... with the backward of the activation that produced x (in_act)
            dx, masked = _layer_dgrad(st, d, ctx.master, ctx.wino, st.wino_bwd if ctx.wino else None, ctx.wpk_bwd, dy, x, ctx.in_act, s)
            if masked:
                ctx.in_act.masked = True
        wparam, bparam = ctx.params
        dw, db = _conv_param_grads(st, d, _p(x), _p(dy), dy.numel() // st.cout_s, st.cout_s,
                                   wparam if ctx.needs_input_grad[1] else None,
                                   bparam if ctx.has_bias and ctx.needs_input_grad[2] else None, (x, dy), x, s)
        return dx, dw, db, None, None, None, None, None


def conv2d(x: Tensor, weight: Tensor, bias: Optional[Tensor], st: ConvState, want_stats: bool = False,
           master: Optional[Tensor] = None, in_act: Optional[ActFold] = None,
           act_bwd_folded: Optional[ActFold] = None) -> Tuple[Tensor, Optional[Tensor]]:
    """NHWC conv.  Returns ``(y, bn_partials)``; ``bn_partials`` is ``None`` unless requested.  ``in_act`` /
    ``act_bwd_folded``: ONE shared ``ActFold`` token for a producer / consumer pair of convs (see ``_Conv2d.forward``)."""
    return _Conv2d.apply(x, weight, bias, st, want_stats, weight if master is None else master, in_act, act_bwd_folded)


def _unshuffle2_check(x4: Tensor, weight: Tensor, st: ConvState) -> Tensor:
    if st.precision not in (0, 1):
        raise RuntimeError(f"unshuffle2_conv: precision {st.precision} has no kernel ('fp32' and 'bf16' do)")
    x4 = _chk(x4, 'unshuffle2_conv.input')
    n, h, w, cs = x4.shape
    if cs != 4 or tuple(weight.shape) != (64, 12, 3, 3):
        raise RuntimeError(f'unshuffle2_conv: expected an NHWC-4 image and a [64, 12, 3, 3] weight, got {tuple(x4.shape)} and '
                           f'{tuple(weight.shape)}')
    if (h & 1 and h < 3) or (w & 1 and w < 3):
        raise RuntimeError(f'unshuffle2_conv: an odd height or width is padded by reflection and must be at least 3, got {h} x {w}')
    return x4


def _unshuffle2_wgrad(x4: Tensor, dy: Tensor, out: Tensor, accumulate: int, s) -> None:
    """The x2 input layer's weight gradient (``srx_unshuffle2_conv_bwd_weight``), written or accumulated into OIHW ``out``."""
    n, h, w, _ = x4.shape
    nws = _lib.lib().srx_unshuffle2_conv_wgrad_ws_floats(n, h, w)
    call('srx_unshuffle2_conv_bwd_weight', n, h, w, _p(x4), _p(dy), _p(out), accumulate, _p(_ws(nws, x4)), nws, s)


class _Unshuffle2Conv(Function):
    """``unshuffle2_conv`` of a trainable layer.  The packed weights are rebuilt by every forward -- one 6912-float launch, a node
    of a captured step like any other -- into the layer's one persistent buffer, never served from the ``WeightPack`` cache: a
    replayed step must not read a pack from before its Adam update, and no pack table refreshes this layout.  Backward: the
    weight gradient (fp32 whatever ``st.precision``) and the column sum of ``dy``; the input is the image and takes none."""

    @staticmethod
    def forward(ctx, x4: Tensor, weight: Tensor, bias: Optional[Tensor], st: ConvState):
        ctx.set_materialize_grads(False)
        n, h, w, _ = x4.shape
        wpk = st.own_pack
        if not isinstance(wpk, Tensor) or wpk.device != x4.device:
            wpk = st.own_pack = torch.empty(_lib.lib().srx_unshuffle2_conv_packed_floats(), dtype=torch.float32, device=x4.device)
        s = _stream()
        call('srx_unshuffle2_conv_pack', _p(_chk(weight.detach(), 'unshuffle2_conv.weight')), _p(wpk), s)
        b = None if bias is None else _chk(bias.detach(), 'unshuffle2_conv.bias')
        y = torch.empty((n, (h + 1) // 2, (w + 1) // 2, 64), dtype=torch.float32, device=x4.device)
        call('srx_unshuffle2_conv_fwd', n, h, w, _p(x4), _p(wpk), _p(b), _p(y), st.precision, s)
        ctx.params = (weight, bias)
        ctx.save_for_backward(x4)
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        x4, = ctx.saved_tensors
        wparam, bparam = ctx.params
        dy = _chk(dy, 'unshuffle2_conv.grad')
        s = _stream()
        dw = db = None
        if ctx.needs_input_grad[1]:
            sink = _sink(wparam)
            if sink is None:
                dw = torch.empty((64, 12, 3, 3), dtype=torch.float32, device=dy.device)
            _unshuffle2_wgrad(x4, dy, dw if sink is None else sink, 0 if sink is None else 1, s)
        if bparam is not None and ctx.needs_input_grad[2]:
            sink = _sink(bparam)
            if sink is None:
                db = torch.empty(64, dtype=torch.float32, device=dy.device)
            _colsum(_p(dy), dy.numel() // 64, 64, 64, db if sink is None else sink, 0 if sink is None else 1, dy, s)
        return None, dw, db, None


def unshuffle2_conv(x4: Tensor, weight: Tensor, bias: Optional[Tensor], st: ConvState, trainable: bool = False) -> Tensor:
    """RRDBNet's x2 input layer, ``conv2d(pixel_unshuffle(pad(x), 2), weight, bias, padding=1)``, as one launch on the NHWC-4
    image (csrc/unshuffle.hip): ``x4`` [N,H,W,4], ``weight`` OIHW [64,12,3,3] -> [N,Hp/2,Wp/2,64] with an odd H / W padded by
    one reflected row / column inside the gather; ``st.precision`` 0 or 1.  Without autograd the weights are packed once through
    ``st.direct`` (``WeightPack.ensure``, keyed like every other layer's).  With autograd on, a ``trainable`` layer runs as an
    autograd node (``_Unshuffle2Conv``: weight and bias gradients, no input gradient -- an image that requires one is refused);
    any other layer is inference-only there."""
    if torch.is_grad_enabled():
        if not trainable:
            raise RuntimeError('unshuffle2_conv: the x2 input layer is inference-only; run it under torch.no_grad() on an eval-mode '
                               'model (or build the layer with trainable=True)')
        if x4.requires_grad:
            raise RuntimeError('unshuffle2_conv: the x2 input layer has no input gradient (its input is the image); got an image '
                               'that requires grad')
        return _Unshuffle2Conv.apply(_unshuffle2_check(x4, weight, st), weight, bias, st)
    x4 = _unshuffle2_check(x4, weight, st)
    n, h, w, _ = x4.shape
    st.direct.ensure(st.pack_key(weight), weight.device, False,
                     lambda: (_lib.lib().srx_unshuffle2_conv_packed_floats(), 0, torch.float32),
                     lambda fwd, bwd, _: call('srx_unshuffle2_conv_pack', _p(_chk(weight.detach(), 'unshuffle2_conv.weight')), _p(fwd),
                                              _stream()))
    b = None if bias is None else _chk(bias.detach(), 'unshuffle2_conv.bias')
    y = torch.empty((n, (h + 1) // 2, (w + 1) // 2, 64), dtype=torch.float32, device=x4.device)
    call('srx_unshuffle2_conv_fwd', n, h, w, _p(x4), _p(st.direct.fwd), _p(b), _p(y), st.precision, _stream())
    return y


# --------------------------------------------------------------------------- batch norm (+act, +residual)
class _BNAct(Function):
    @staticmethod
    def forward(ctx, y: Tensor, part: Optional[Tensor], gamma: Tensor, beta: Tensor, prelu: Optional[Tensor],
                residual: Optional[Tensor], running_mean: Tensor, running_var: Tensor, nbt: Optional[Tensor],
                training: bool, eps: float, momentum: float, act: int, slope: float, groups: int):
        ctx.set_materialize_grads(False)
        y = _chk(y, 'bn.input')
        c = y.shape[-1]
        m = y.numel() // c
        s = _stream()
        if not training:
            groups = 1  # eval: one set of running statistics for every row
        g = _chk(gamma.detach(), 'bn.weight')
        b = _chk(beta.detach(), 'bn.bias')
        pw = None if prelu is None else _chk(prelu.detach(), 'prelu.weight')
        res = None if residual is None else _chk(residual, 'bn.residual')
        out = torch.empty_like(y)
        if training:
            if part is None:
                rows = _lib.lib().srx_bn_stat_rows(m)
                part = torch.empty((rows, c, 2), dtype=torch.float32, device=y.device)
                call('srx_bn_partial_stats', _p(y), _p(part), m, c, s)
            mean, invstd = _bn_train_fwd(y, part, m, c, groups, eps, momentum, g, b, res, out, act, slope, pw, running_mean,
                                         running_var, nbt, s)
        else:
            mean = torch.empty(c, dtype=torch.float32, device=y.device)
            invstd = torch.empty(c, dtype=torch.float32, device=y.device)
            call('srx_bn_eval_stats', _p(running_mean), _p(running_var), c, eps, _p(mean), _p(invstd), s)
            call('srx_bn_act_fwd', _p(y), _p(mean), _p(invstd), _p(g), _p(b), _p(res), _p(out), m, c, act, slope, _p(pw),
                 s)
        ctx.save_for_backward(y, mean, invstd, g, b, pw)
        ctx.cfg = (m, c, act, slope, training, residual is not None, prelu is not None, groups)
        ctx.params = (gamma, beta, prelu)
        return out

    @staticmethod
    def backward(ctx, dout: Tensor):
        y, mean, invstd, g, b, pw = ctx.saved_tensors
        m, c, act, slope, training, has_res, has_prelu, groups = ctx.cfg
        dout = _chk(dout, 'bn.grad')
        gs, bs, ps = (_sink(t) for t in ctx.params)
        dy, sums = _bn_act_bwd(dout, y, mean, invstd, g, b, pw, m, c, groups, act, slope, training, (gs, bs, ps), _stream(),
                               want_dy=ctx.needs_input_grad[0])
        want = ((ctx.needs_input_grad[2] and gs is None), (ctx.needs_input_grad[3] and bs is None),
                (has_prelu and ctx.needs_input_grad[4] and ps is None))
        dgamma = dbeta = dprelu = None
        if any(want):  # gradients returned to autograd instead of accumulated by the kernel: total over the groups
            per = sums.view(groups, 2 * c + 4)
            tot = per[0] if groups == 1 else per.sum(0)
            dgamma = tot[c:2 * c] if want[0] else None
            dbeta = tot[:c] if want[1] else None
            dprelu = tot[2 * c:2 * c + 1] if want[2] else None
        dres = dout if (has_res and ctx.needs_input_grad[5]) else None
        return (dy, None, dgamma, dbeta, dprelu, dres) + (None,) * 9


def bn_groups_ok(m: int, tile_rows: Optional[int], groups: int) -> bool:
    """Can ``m`` rows be normalised as ``groups`` independent row ranges?  ``tile_rows``: rows per entry of the conv
    epilogue's partial-statistics table (``conv_stat_tile_rows``; ``None``: the statistics come from
    ``srx_bn_partial_stats``).  No conv tile and no row block of the streaming reductions may straddle two groups."""
    if groups == 1:
        return True
    if m % groups:
        return False
    per = m // groups
    if per % _lib.lib().srx_bn_rows_per_block(m):
        return False
    return tile_rows is None or per % tile_rows == 0


def conv_stat_tile_rows(st: ConvState, n: int, h: int, w: int) -> int:
    """Output rows (pixels) summarised by one row of the partial-statistics table ``conv2d(..., want_stats=True)``
    returns for this layer at this input size: the tile height of the launch plan."""
    if wino_forward_runs(st, st.desc(n, h, w), True):
        return 128  # a Winograd tile block: 32 consecutive 2x2 tiles (image-major)
    out = (C.c_int * 6)()
    call('srx_conv2d_plan', C.byref(st.desc(n, h, w)), 0, out)
    return int(out[0])


def bn_act(y, part, bn, act=ACT_NONE, slope=0.0, prelu: Optional[Tensor] = None,
           residual: Optional[Tensor] = None, frozen: bool = False, groups: int = 1) -> Tensor:
    """``act(BatchNorm2d(y)) [+ residual]`` with ``bn`` an ``nn.BatchNorm2d``-compatible module.  ``groups``: the batch
    is that many forward calls of the reference run together (independent batch statistics, see norm.hip)."""
    training = bn.training or bn.running_mean is None
    momentum = 0.1 if bn.momentum is None else bn.momentum
    gamma, beta = (bn.weight.detach(), bn.bias.detach()) if frozen else (bn.weight, bn.bias)
    return _BNAct.apply(y, part, gamma, beta, prelu, residual, bn.running_mean, bn.running_var,
                        bn.num_batches_tracked if training else None, training, bn.eps, momentum, act, float(slope),
                        int(groups))


class _ResidualTower(Function):
    """The chain of SRGAN ``ResidualBlock``s -- each ``x + BN2(conv2(PReLU(BN1(conv1(x)))))`` (srgan/residual.py:86-91;
    srgan/generator.py:42-45,76) -- as ONE autograd node in training mode, for one block or many.  Per block: the skip
    connection's gradient, which autograd would add to conv1's input gradient in a pass of its own, is the epilogue of conv1's
    data gradient (``srx_conv2d_bwd_data_add``); parameter gradients accumulate straight into the flat ``.grad`` buffers; the
    conv weight gradients go to the ``WeightGradQueue`` when one is installed.  And what only a node that sees neighbouring
    layers can do -- the first pass of every BatchNorm backward (the per-channel sums of dz and dz * xhat) rides in the
    epilogue of the data gradient that PRODUCES that BatchNorm's output gradient (``srx_conv2d_bwd_data_bn``): conv2's data
    gradient reduces for bn1 + PReLU of its own block, conv1's (plus the skip gradient) for bn2 of the block BEFORE.  32 of
    the 33 ``bn_bwd_reduce`` launches of a generator backward pass (and their second read of two 2.4 MB tensors each) disappear.
    """

    @staticmethod
    def forward(ctx, x: Tensor, blocks, *params):
        ctx.set_materialize_grads(False)
        x = _chk(x, 'residual_tower.input')
        n, h, w, c = x.shape
        m = n * h * w
        L, s = _lib.lib(), _stream()
        saved, descs = [], None
        # A normalise pass (bn1 + PReLU inside a block, bn2 + skip at its end) is not launched where the NEXT conv can apply it
        # while staging its input (srx_conv2d_fwd_bn_in: `pending` = (y, mean, invstd, gamma, beta, slope, residual, result));
        # the result tensor is written by that conv on the side.  Only the last block's bn2 + skip is a launch of its own.
        pending = None
        fuse = None
        for bi, block in enumerate(blocks):
            convs, bns = (block.conv1, block.conv2), (block.bn1, block.bn2)
            inp, ys, stats = x, [], []
            for i in range(2):
                st, bn = convs[i]._st, bns[i]
                d = st.desc(n, h, w)
                dref = C.byref(d)
                if fuse is None:
                    fuse = L.srx_conv2d_fwd_bn_in_ok(dref) == 1
                st.pack(convs[i].weight, d)
                y = torch.empty_like(x)
                part = torch.empty((L.srx_conv2d_stat_rows(dref), c, 2), dtype=torch.float32, device=x.device)
                if pending is not None:
                    py, pmean, pinv, pg, pb, pslope, pres, pout = pending
                    call('srx_conv2d_fwd_bn_in', dref, _p(py), _p(pmean), _p(pinv), _p(pg), _p(pb), _p(pslope), _p(pres), _p(pout),
                         _p(st.wpk_fwd), None, _p(y), _p(part), s)
                    pending = None
                else:
                    _conv_fwd(d, _p(inp), _p(st.wpk_fwd), None, _p(y), x, s, part_ptr=_p(part))
                out = torch.empty_like(x)
                last = i == 1 and bi == len(blocks) - 1
                if fuse and not last:  # statistics only; the normalise pass rides in the next conv's launch
                    mean = torch.empty(c, dtype=torch.float32, device=x.device)
                    invstd = torch.empty(c, dtype=torch.float32, device=x.device)
                    call('srx_bn_finalize', _p(part), part.shape[0], m, c, bn.eps, 0.1 if bn.momentum is None else bn.momentum,
                         _p(mean), _p(invstd), _p(bn.running_mean), _p(bn.running_var), _p(bn.num_batches_tracked), s)
                    g, b = bn.weight.detach(), bn.bias.detach()
                    pending = (y, mean, invstd, g, b, block.prelu.weight.detach(), None, out) if i == 0 else \
                        (y, mean, invstd, g, b, None, x, out)
                else:  # BN1 + PReLU, or BN2 + skip connection
                    mean, invstd = _bn_train_fwd(y, part, m, c, 1, bn.eps, bn.momentum, bn.weight, bn.bias, None if i == 0 else x, out,
                                                 ACT_PRELU if i == 0 else ACT_NONE, 0.0, block.prelu.weight if i == 0 else None,
                                                 bn.running_mean, bn.running_var, bn.num_batches_tracked, s)
                if i == 0:
                    a1 = inp = out
                ys.append(y)
                stats += [mean, invstd]
                descs = d
            saved += [x, ys[0], a1, ys[1], *stats]
            x = out
        ctx.blocks, ctx.desc = blocks, descs
        ctx.packs = [(b.conv1._st.wpk_bwd, b.conv2._st.wpk_bwd) for b in blocks]
        ctx.save_for_backward(*saved)
        return x

    @staticmethod
    def backward(ctx, dout: Tensor):
        saved, blocks, d = ctx.saved_tensors, ctx.blocks, ctx.desc
        grad = _chk(dout, 'residual_tower.grad')
        n, h, w, c = grad.shape
        m = n * h * w
        L, s = _lib.lib(), _stream()
        dref = C.byref(d)
        rows = L.srx_conv2d_bwd_data_bn_rows(dref)  # 0: the layers do not run on the row-tile kernel at this size
        if _dev.NO_BN_DGRAD_FUSE:  # developer switch (A/B runs): separate reduce launches
            rows = 0
        nws_d = L.srx_conv2d_bwd_data_ws_floats(dref)
        W = 2 * c + 4

        def finish(dz_in, y, mean, invstd, bn, act, prelu, table):
            """dy of act(BN(y)) given dz_in; the reduce pass comes from `table` when the producer of dz_in filled one"""
            pg = None if prelu is None else prelu.grad
            if table is None:
                return _bn_act_bwd(dz_in, y, mean, invstd, bn.weight, bn.bias, prelu, m, c, 1, act, 0.0, True,
                                   (bn.weight.grad, bn.bias.grad, pg), s)[0]
            sums = torch.empty(W, dtype=torch.float32, device=grad.device)
            dy = torch.empty_like(y)
            call('srx_bn_act_bwd_finish', _p(dz_in), _p(y), _p(mean), _p(invstd), _p(bn.weight), _p(bn.bias), _p(table), rows, 2,
                 _p(sums), _p(dy), m, c, act, 0.0, _p(prelu), _p(bn.weight.grad), _p(bn.bias.grad), _p(pg), s)
            return dy

        def dgrad(pack, dy, addend, below):
            """conv^T(dy) [+ addend]; `below` = (y, mean, invstd, bn, prelu) of the BatchNorm the result arrives at, or None"""
            dx = torch.empty_like(dy)
            if below is not None and rows:
                y, mean, invstd, bn, prelu = below
                table = torch.empty((rows, W), dtype=torch.float32, device=dy.device)
                call('srx_conv2d_bwd_data_bn', dref, _p(dy), _p(pack), _p(addend), _p(dx), _p(y), _p(mean), _p(invstd),
                     _p(bn.weight.detach()), _p(bn.bias.detach()), None if prelu is None else _p(prelu.detach()), _p(table), s)
                return dx, table
            _conv_dgrad(d, _p(dy), _p(pack), _p(dx), dy, s, addend_ptr=_p(addend), nws=nws_d)
            return dx, None

        def wgrad(conv, inp, dy):
            _conv_wgrad(d, _p(inp), _p(dy), None, conv.weight.grad, None, (inp, dy), inp, s)

        # With a table from the producer, the APPLY pass of a BatchNorm backward rides in the data gradient that consumes its
        # result too (srx_conv2d_bwd_data_bn_in: the layer's input gradient is formed while the patch is staged and written on
        # the side for the weight gradient): per block two more launches disappear, finalize -> data gradient is all that is left
        fuse_in = bool(rows) and L.srx_conv2d_bwd_data_bn_in_ok(dref) == 1

        def sums_only(y, bn, act, prelu, table):
            """finalize pass alone: the reduced sums (and the parameter gradients) from the producer's table"""
            sums = torch.empty(W, dtype=torch.float32, device=grad.device)
            pw = None if prelu is None else prelu.detach()
            pg = None if prelu is None else _p(prelu.grad)
            call('srx_bn_act_bwd_finish', None, None, None, None, None, None, _p(table), rows, 2, _p(sums), None, m, c, act, 0.0,
                 _p(pw), _p(bn.weight.grad), _p(bn.bias.grad), pg, s)
            return sums

        def dgrad_in(pack, dz_in, above, sums, addend, below):
            """conv^T(dy) [+ addend] with dy = the input gradient of the BatchNorm (+ PReLU) layer `above` = (y, mean, invstd,
            bn, prelu), formed from dz_in on load and returned as well; `below` as in dgrad"""
            y, mean, invstd, bn, prelu = above
            dy, dx = torch.empty_like(y), torch.empty_like(y)
            table = None
            by = bmean = binv = bg = bb = bp = None
            if below is not None:
                table = torch.empty((rows, W), dtype=torch.float32, device=y.device)
                by, bmean, binv, bbn, bprelu = below
                bg, bb = bbn.weight.detach(), bbn.bias.detach()
                bp = None if bprelu is None else bprelu.detach()
            call('srx_conv2d_bwd_data_bn_in', dref, _p(dz_in), _p(y), _p(mean), _p(invstd), _p(bn.weight.detach()),
                 _p(bn.bias.detach()), None if prelu is None else _p(prelu.detach()), _p(sums), _p(dy), _p(pack), _p(addend), _p(dx),
                 _p(by), _p(bmean), _p(binv), _p(bg), _p(bb), _p(bp), _p(table), s)
            return dy, dx, table

        table2 = None  # the reduce pass of the top block's bn2 has no producer inside this node
        for i in range(len(blocks) - 1, -1, -1):
            block = blocks[i]
            x, y1, a1, y2, mean1, inv1, mean2, inv2 = saved[8 * i:8 * i + 8]
            below1 = (y1, mean1, inv1, block.bn1, block.prelu.weight)
            if fuse_in and table2 is not None:
                sums2 = sums_only(y2, block.bn2, ACT_NONE, None, table2)
                dy2, da1, table1 = dgrad_in(ctx.packs[i][1], grad, (y2, mean2, inv2, block.bn2, None), sums2, None, below1)
            else:
                dy2 = finish(grad, y2, mean2, inv2, block.bn2, ACT_NONE, None, table2)
                da1, table1 = dgrad(ctx.packs[i][1], dy2, None, below1)
            wgrad(block.conv2, a1, dy2)
            need_dx = i > 0 or ctx.needs_input_grad[0]
            below = None
            if i > 0:
                pb = blocks[i - 1]
                below = (saved[8 * (i - 1) + 3], saved[8 * (i - 1) + 6], saved[8 * (i - 1) + 7], pb.bn2, None)
            if fuse_in and table1 is not None and need_dx:
                sums1 = sums_only(y1, block.bn1, ACT_PRELU, block.prelu.weight, table1)
                dy1, grad, table2 = dgrad_in(ctx.packs[i][0], da1, below1, sums1, grad, below)
                wgrad(block.conv1, x, dy1)
                continue
            dy1 = finish(da1, y1, mean1, inv1, block.bn1, ACT_PRELU, block.prelu.weight, table1)
            wgrad(block.conv1, x, dy1)
            if need_dx:
                grad, table2 = dgrad(ctx.packs[i][0], dy1, grad, below)
            else:
                grad = None
        return (grad, None) + (None,) * (len(ctx.needs_input_grad) - 2)


def residual_tower(x: Tensor, blocks) -> Tensor:
    """``nn.Sequential(*blocks)(x)`` for ``ResidualBlock`` modules that all satisfy ``residual_block_fused_ok``."""
    ps = []
    for b in blocks:
        ps += [b.conv1.weight, b.bn1.weight, b.bn1.bias, b.prelu.weight, b.conv2.weight, b.bn2.weight, b.bn2.bias]
    return _ResidualTower.apply(x, list(blocks), *ps)


def residual_block_fused_ok(block) -> bool:
    """The one-node form applies in training mode with autograd on, when every parameter of the block accumulates
    its gradient straight into a flat ``.grad`` buffer (``direct_grads``: the trainers)."""
    if not (block.training and torch.is_grad_enabled() and direct_grads[0]):
        return False
    ps = (block.conv1.weight, block.bn1.weight, block.bn1.bias, block.prelu.weight, block.conv2.weight, block.bn2.weight,
          block.bn2.bias)
    return block.bn1.training and block.bn2.training and block.prelu.weight.numel() == 1 and \
        all(p.requires_grad and _sink(p) is not None for p in ps)


def residual_block(x: Tensor, block) -> Tensor:
    """One ``ResidualBlock`` that satisfies ``residual_block_fused_ok``: a tower of one."""
    return residual_tower(x, [block])


# --------------------------------------------------------------------------- activations
class _PReLU(Function):
    @staticmethod
    def forward(ctx, x: Tensor, w: Tensor):
        ctx.set_materialize_grads(False)
        x = _chk(x, 'prelu.input')
        wd = _chk(w.detach(), 'prelu.weight')
        y = torch.empty_like(x)
        call('srx_prelu_fwd', _p(x), _p(wd), _p(y), x.numel(), _stream())
        ctx.save_for_backward(x, wd)
        ctx.param = w
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        x, w = ctx.saved_tensors
        dy = _chk(dy, 'prelu.grad')
        dx = torch.empty_like(x)
        sink = _sink(ctx.param) if ctx.needs_input_grad[1] else None
        dw = None if sink is not None else torch.empty(1, dtype=torch.float32, device=x.device)
        call('srx_prelu_bwd', _p(dy), _p(x), _p(w), _p(dx), _p(dw if sink is None else sink), 0 if sink is None else 1,
             x.numel(), _p(_ws(1024, x)), _stream())
        return dx, dw


def prelu(x: Tensor, w: Tensor) -> Tensor:
    if w.numel() != 1:
        raise RuntimeError('prelu: only the single-slope nn.PReLU() of the reference is implemented')
    return _PReLU.apply(x, w)


def _slopes16(w: Tensor) -> Tensor:
    """The slope vector where the kernels can read it in 16-byte pieces (a parameter inside a flat buffer may start anywhere)."""
    w = _chk(w, 'prelu_channels.weight')
    return w if w.data_ptr() % 16 == 0 else w.clone()


def _prelu_channels_rows(x: Tensor, w: Tensor) -> Tuple[int, int, int]:
    cs, c = x.shape[-1], w.numel()
    if x.dim() < 2 or c > cs or c % 4 or cs % 4:
        raise RuntimeError(f'prelu_channels: {c} slopes on a channel-last tensor of stride {cs}: both must be multiples of 4 and '
                           f'the slopes no more than the stride')
    return x.numel() // cs, c, cs


class _PReLUChannels(Function):
    """``nn.PReLU(C)`` on a channel-last tensor: one slope per channel (csrc/compact.hip)."""

    @staticmethod
    def forward(ctx, x: Tensor, w: Tensor):
        ctx.set_materialize_grads(False)
        x = _chk(x, 'prelu_channels.input')
        wd = _slopes16(w.detach())
        m, c, cs = _prelu_channels_rows(x, wd)
        y = torch.empty_like(x)
        call('srx_prelu_channels_fwd', _p(x), _p(wd), _p(y), m, c, cs, _stream())
        ctx.save_for_backward(x, wd)
        ctx.param = w
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        if dy is None:
            return None, None
        x, w = ctx.saved_tensors
        dy = _chk(dy, 'prelu_channels.grad')
        m, c, cs = _prelu_channels_rows(x, w)
        dx = torch.empty_like(x)
        sink = _sink(ctx.param) if ctx.needs_input_grad[1] else None
        dw = None if sink is not None else torch.empty(c, dtype=torch.float32, device=x.device)
        nws = _lib.lib().srx_prelu_channels_ws_floats(m, c)
        ws = torch.empty((int(nws) + 1) // 2, dtype=torch.float64, device=x.device)  # (fp64 slots: 8-byte aligned)
        call('srx_prelu_channels_bwd', _p(dy), _p(x), _p(w), _p(dx), _p(dw if sink is None else sink), 0 if sink is None else 1,
             m, c, cs, _p(ws), nws, _stream())
        return dx, (None if dw is None else dw.view(ctx.param.shape))


def prelu_channels(x: Tensor, w: Tensor) -> Tensor:
    """``y = x > 0 ? x : w[c] * x`` on NHWC fp32 ``[..., Cs]`` with ``w`` of ``C <= Cs`` slopes (channels past ``C`` pass
    through); differentiable in both arguments."""
    return _PReLUChannels.apply(x, w)


_TAIL_DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


class _ShuffleAddNearest(Function):
    """The compact generator's tail: ``PixelShuffle(s)`` of the last conv's ``3 s^2`` channels plus the nearest-enlarged input."""

    @staticmethod
    def forward(ctx, t: Tensor, x4: Tensor, s: int):
        ctx.set_materialize_grads(False)
        if t.dtype not in _TAIL_DTYPES:
            raise RuntimeError(f'shuffle_add_nearest: expected a float32, bfloat16 or float16 tensor, got {t.dtype}')
        t = _chk(t, 'shuffle_add_nearest.input') if t.dtype == torch.float32 else _chk16(t, 'shuffle_add_nearest.input', None)
        x4 = _chk(x4, 'shuffle_add_nearest.image')
        if t.dim() != 4 or x4.dim() != 4 or x4.shape[3] != 4 or tuple(x4.shape[:3]) != tuple(t.shape[:3]):
            raise RuntimeError(f'shuffle_add_nearest: features {tuple(t.shape)} and NHWC-4 image {tuple(x4.shape)} do not match')
        n, h, w, cs = t.shape
        y4 = torch.empty((n, h * s, w * s, 4), dtype=torch.float32, device=t.device)
        call('srx_shuffle_add_nearest_fwd', _p(t), _TAIL_DTYPES[t.dtype], cs, _p(x4), _p(y4), n, h, w, int(s), _stream())
        ctx.geom = (n, h, w, cs, int(s), t.dtype)
        return y4

    @staticmethod
    def backward(ctx, dy4: Tensor):
        if dy4 is None:
            return None, None, None
        n, h, w, cs, s, dt = ctx.geom
        if dt != torch.float32:
            raise RuntimeError('shuffle_add_nearest: only fp32 features are differentiable')
        dy4 = _chk(dy4, 'shuffle_add_nearest.grad')
        d = torch.empty((n, h, w, cs), dtype=torch.float32, device=dy4.device)
        call('srx_shuffle_add_nearest_bwd', _p(dy4), _p(d), cs, n, h, w, s, _stream())
        return d, None, None  # (the input image is data)


def shuffle_add_nearest(t: Tensor, x4: Tensor, s: int) -> Tensor:
    """``y4[n, s y + i, s x + j, c] = t[n, y, x, c s^2 + i s + j] + x4[n, y, x, c]`` (``c < 3``; channel 3 zero): NHWC-4 fp32 out.
    ``t``: fp32 (differentiable), bf16 or fp16 ``[N, h, w, >= 3 s^2]``; ``s`` in 2, 3, 4."""
    return _ShuffleAddNearest.apply(t, x4, int(s))


class _LReLU(Function):
    @staticmethod
    def forward(ctx, x: Tensor, slope: float):
        ctx.set_materialize_grads(False)
        x = _chk(x, 'lrelu.input')
        y = torch.empty_like(x)
        call('srx_lrelu_fwd', _p(x), _p(y), x.numel(), slope, _stream())
        ctx.slope = slope
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        (y,) = ctx.saved_tensors
        dy = _chk(dy, 'lrelu.grad')
        dx = torch.empty_like(dy)
        call('srx_act_bwd_from_out', _p(dy), _p(y), _p(dx), dy.numel(), ACT_LRELU, ctx.slope, _stream())
        return dx, None


def leaky_relu(x: Tensor, slope: float) -> Tensor:
    return _LReLU.apply(x, float(slope))


class _Sigmoid(Function):
    @staticmethod
    def forward(ctx, x: Tensor):
        ctx.set_materialize_grads(False)
        x = _chk(x, 'sigmoid.input')
        y = torch.empty_like(x)
        call('srx_sigmoid_fwd', _p(x), _p(y), x.numel(), _stream())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        (y,) = ctx.saved_tensors
        dy = _chk(dy, 'sigmoid.grad')
        dx = torch.empty_like(y)
        call('srx_sigmoid_bwd', _p(dy), _p(y), _p(dx), y.numel(), _stream())
        return dx


def sigmoid(x: Tensor) -> Tensor:
    return _Sigmoid.apply(x)


class _Axpby(Function):
    @staticmethod
    def forward(ctx, x: Tensor, z: Tensor, a: float, b: float):
        ctx.set_materialize_grads(False)
        x, z = _chk(x, 'axpby.x'), _chk(z, 'axpby.z')
        y = torch.empty_like(x)
        call('srx_axpby', _p(x), _p(z), _p(y), x.numel(), a, b, _stream())
        ctx.ab = (a, b)
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        a, b = ctx.ab
        dy = _chk(dy, 'axpby.grad')
        s = _stream()
        dx = dz = None
        if ctx.needs_input_grad[0]:
            dx = dy if a == 1.0 else torch.empty_like(dy)
            if a != 1.0:
                call('srx_axpby', _p(dy), _p(dy), _p(dx), dy.numel(), a, 0.0, s)
        if ctx.needs_input_grad[1]:
            dz = dy if b == 1.0 else torch.empty_like(dy)
            if b != 1.0:
                call('srx_axpby', _p(dy), _p(dy), _p(dz), dy.numel(), b, 0.0, s)
        return dx, dz, None, None


def axpby(x: Tensor, z: Tensor, a: float = 1.0, b: float = 1.0) -> Tensor:
    """``a*x + b*z`` (residual adds / scalings)."""
    return _Axpby.apply(x, z, float(a), float(b))


# --------------------------------------------------------------------------- pooling
class _MaxPool(Function):
    @staticmethod
    def forward(ctx, x: Tensor):
        ctx.set_materialize_grads(False)
        x = _chk(x, 'maxpool.input')
        n, h, w, c = x.shape
        y = torch.empty((n, h // 2, w // 2, c), dtype=torch.float32, device=x.device)
        call('srx_maxpool2x2_fwd', _p(x), _p(y), n, h, w, c, _stream())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        (x,) = ctx.saved_tensors
        dy = _chk(dy, 'maxpool.grad')
        n, h, w, c = x.shape
        dx = torch.empty_like(x)
        call('srx_maxpool2x2_bwd', _p(dy), _p(x), _p(dx), n, h, w, c, _stream())
        return dx


def maxpool2x2(x: Tensor) -> Tensor:
    return _MaxPool.apply(x)


# --------------------------------------------------------------------------- frozen conv stacks (the perceptual losses)
# ONE walk over a frozen ``[('conv', layers.Conv2d) | ('pool', None)]`` stack behind both perceptual-loss nodes: per conv the
# choice between the bf16-storage kernels, Winograd and the direct kernel, the rule for which layer writes fp32, and the
# data-gradient chain with the activation backwards folded in.  What differs between the nodes -- the pools, the entry into the
# backward, the loss -- stays in ``_FrozenConvStack`` / ``_FrozenTapStack`` and is passed in.
def _bf16_stack_ok(layers, shape, taps=()) -> bool:
    """May this frozen stack keep its inner activations as bf16 (``_stack_conv_fwd``)?  Every conv multiplies bf16 products
    (autocast), the stack starts with the 3 -> 64 layer, every other conv is a 3x3 / stride 1 / pad 1 layer with channel counts that
    are multiples of 64, pools sit between convs and the stack ends with a conv.  Every conv carries a fused ReLU, except the
    convs at the positions ``taps`` (``_FrozenTapStack``), which carry none: a tap's ReLU is the pool's."""
    if _dev.NO_BF16S or len(layers) < 2 or layers[0][0] != 'conv' or layers[-1][0] != 'conv' or layers[1][0] != 'conv':
        return False
    L = _lib.lib()
    n, h, w, _c = shape
    for i, (kind, conv) in enumerate(layers):
        if kind == 'pool':
            if layers[i - 1][0] != 'conv' or layers[i + 1][0] != 'conv' or h % 2 or w % 2:
                return False
            h, w = h // 2, w // 2
            continue
        st = conv._st
        if st.precision != 1 or st.act != (ACT_NONE if i in taps else ACT_RELU) or st.stride != 1 or st.shuffle or st.k != 3 or st.pad != 1:
            return False
        if i == 0:
            if st.cin > 4 or st.cout != 64:
                return False
        elif L.srx_conv3x3_bf16s_applicable(C.byref(st.desc(n, h, w))) != 1:
            return False
    return True


def _stack_writes_f32(layers, i: int) -> bool:
    """THE rule for a conv's output under bf16 storage: the last conv and a conv in front of a pool write fp32 -- the features go
    to an fp32 loss, a pool compares fp32 values (as the recipe does) --, every other conv writes bf16.  In a tap stack these are
    exactly the taps (``_tap_stack_check``)."""
    return i + 1 == len(layers) or layers[i + 1][0] == 'pool'


def _bf16s_ws(dref, backward: int, like: Tensor):
    """``(workspace pointer, its size)`` of a bf16-storage conv's forward (0) or data gradient (1)."""
    nws = _lib.lib().srx_conv3x3_bf16s_ws_floats(dref, backward)
    return (_p(_ws(nws, like)) if nws else None), nws


def _stack_conv_fwd(layers, i: int, x: Tensor, relu: bool, to_f32: bool, bf16s: bool, need_bwd: bool, who: str, s):
    """The conv at position ``i`` of a frozen stack on ``x``: pack, choose, launch.  ``bf16s`` (``_bf16_stack_ok``): the
    activations BETWEEN the convs are stored as bf16 (csrc/gconv.hip "bf16 STORAGE") -- the same bf16 products as with fp32
    storage, an operand being rounded once, by its producer, at half the bytes and without the loaders' fp32 -> bf16 conversion;
    ``relu``: the ReLU is fused (there the epilogue is an argument; elsewhere it is the layer's own ``act``); ``to_f32``: what the
    conv writes.  Returns the output and the layer's plan entry ``('conv', state, packed weights of the data gradient)``: the
    fp32 paths capture them now (``('wino', U)`` or the direct pack), the bf16-storage path reads its own at backward time (None)."""
    conv = layers[i][1]
    st = conv._st
    n, h, w, _c = x.shape
    d = st.desc(n, h, w)
    dref = C.byref(d)
    y = torch.empty(st.out_shape(n, h, w), dtype=torch.float32 if to_f32 else torch.bfloat16, device=x.device)
    b = None if conv.bias is None else _chk(conv.bias.detach(), who + '.bias')
    if bf16s and i == 0:   # the 3 -> 64 first layer: fp32 image in, its own kernel
        st.pack(conv.weight, d)
        call('srx_conv2d_fwd_first3_to_bf16', dref, _p(x), _p(st.wpk_fwd), _p(b), _p(y), s)
        return y, ('conv', st, None)
    if bf16s:
        st.pack_bf16s(conv.weight, d, need_bwd)
        ws, nws = _bf16s_ws(dref, 0, x)
        call('srx_conv3x3_bf16s_fwd', dref, _p(x), _p(st.bf16s_fwd), _p(b), 1 if relu else 0, _p(y), 0 if to_f32 else 1, ws, nws, s)
        return y, ('conv', st, None)
    if wino_layer_ok(st, d):   # wide 3x3 layers: Winograd F(2x2, 3x3), 2.25x fewer fp32 multiplications (csrc/wino.hip)
        st.pack_wino(conv.weight, d, need_bwd=need_bwd)
        _wino_fwd(d, x, st.wino_fwd, b, y, None, s)
        return y, ('conv', st, ('wino', st.wino_bwd))
    st.pack(conv.weight, d)
    _conv_fwd(d, _p(x), _p(st.wpk_fwd), _p(b), _p(y), x, s)
    return y, ('conv', st, st.wpk_bwd)


def _stack_conv_dgrad(plan, i: int, g: Tensor, x: Tensor, master: Tensor, bf16s: bool, s) -> Tensor:
    """The data gradient of the conv at position ``i`` from the plan of ``_stack_conv_fwd``; ``x``: the conv's input (source
    half).  A conv right below made ``x = act(conv)``: that activation's backward is folded in on the way out."""
    _, st, wpk_bwd = plan[i]
    n, h, w, _c = x.shape
    d = st.desc(n, h, w)
    below = plan[i - 1][1] if i > 0 and plan[i - 1][0] == 'conv' else None
    if not bf16s:
        wino = isinstance(wpk_bwd, tuple)
        return _layer_dgrad(st, d, master, wino, wpk_bwd[1] if wino else None, None if wino else wpk_bwd, g, x, below, s)[0]
    if i == 0:   # the 3 -> 64 first layer: the direct kernel on an fp32 gradient
        dx = torch.empty_like(x)
        _conv_dgrad(d, _p(g), _p(st.wpk_bwd), _p(dx), x, s)
        return dx
    dref = C.byref(d)
    to_f32 = i == 1   # ... which layer 1 therefore writes as fp32
    dx = torch.empty(x.shape, dtype=torch.float32 if to_f32 else torch.bfloat16, device=x.device)
    ws, nws = _bf16s_ws(dref, 1, dx)
    call('srx_conv3x3_bf16s_bwd_data', dref, _p(g), _p(st.bf16s_bwd), _p(x) if below is not None else None, _p(dx), 0 if to_f32 else 1,
         ws, nws, s)
    return dx


def _stack_forward(x: Tensor, layers, taps, bf16s: bool, need_bwd: bool, pool, who: str, s):
    """Every layer of a frozen stack on ``x``; ``pool(i, x) -> y`` launches the node's own pool at position ``i``; the convs at
    the positions ``taps`` write their pre-activation.  Returns ``(saved, plan)``: every layer's input and the last output, and
    one entry per layer for ``_stack_backward``."""
    saved, plan = [x], []
    for i, (kind, _conv) in enumerate(layers):
        if kind == 'pool':
            x = pool(i, x)
            plan.append(('pool', None, None))
        else:
            x, entry = _stack_conv_fwd(layers, i, x, i not in taps, not bf16s or _stack_writes_f32(layers, i), bf16s, need_bwd, who, s)
            plan.append(entry)
        saved.append(x)
    return saved, plan


def _stack_backward(g: Tensor, saved, plan, masters, n: int, bf16s: bool, pool_bwd, s) -> Tensor:
    """The data-gradient chain of the source half (the first ``n`` images: batch-major, so a prefix) from the gradient ``g`` of
    the last conv's output, pre-activation; ``pool_bwd(i, g, x) -> dx`` launches the node's own pool backward on the pool's input."""
    for i in range(len(plan) - 1, -1, -1):
        x = saved[i][:n]
        g = pool_bwd(i, g, x) if plan[i][0] == 'pool' else _stack_conv_dgrad(plan, i, g, x, masters[i], bf16s, s)
    return g


def _stack_weights(layers, who: str):
    weights = [p for _, m in layers if m is not None for p in (m.weight, m.bias) if p is not None]
    if any(p.requires_grad for p in weights):
        raise RuntimeError(who + ': the stack must be frozen (requires_grad = False on every parameter)')
    return weights


class _FrozenConvStack(Function):
    """A frozen stack of ``conv3x3 + ReLU`` and ``MaxPool2d(2)`` layers as ONE autograd node: the VGG19 feature
    extractor of the perceptual loss (srgan/loss.py:30-34,52-53: pretrained, ``requires_grad = False``, eval).

    Forward: ``source`` and ``target`` (loss.py:52 and :53) go through the stack TOGETHER as one batch of 2N -- same
    weights, twice the rows per launch (the 6x6 and 12x12 layers alone fill a quarter of the chip).  Backward: only
    the source half is differentiated (the target is ``high_res.detach()``, srgan/trainer.py:455), weights take no
    gradient, and every ReLU backward rides in the epilogue of the data gradient above it or in the max-pool backward: 16
    data-gradient launches and 4 pool launches, no elementwise passes besides the topmost ReLU.

    The convs and their data gradients are the shared walk's (``_stack_forward`` / ``_stack_backward``), under autocast on bf16
    storage (``_bf16_stack_ok``).  This node's own: the ``(fs, ft)`` views it returns, the plain pools, the topmost
    activation's backward, and in fp32 the general stack -- LeakyReLU convs, a pool whose input is no ReLU output.
    """

    @staticmethod
    def forward(ctx, source: Tensor, target: Optional[Tensor], layers, *weights):
        ctx.set_materialize_grads(False)
        source = _chk(source, 'conv_stack.source')
        n_src = source.shape[0]
        x = source if target is None else torch.cat([source, _chk(target, 'conv_stack.target')], dim=0)
        s = _stream()
        ctx.bf16s = bf16s = _bf16_stack_ok(layers, x.shape)
        for kind, conv in layers:
            if kind == 'conv' and (conv._st.act not in (ACT_RELU, ACT_LRELU) or conv._st.stride != 1 or conv._st.shuffle):
                raise RuntimeError('conv_stack: stride-1 conv + ReLU / LeakyReLU layers only')

        def pool(i: int, x: Tensor) -> Tensor:
            n, h, w, c = x.shape
            y = torch.empty((n, h // 2, w // 2, c), dtype=torch.bfloat16 if bf16s else torch.float32, device=x.device)
            call('srx_maxpool2x2_fwd_to_bf16' if bf16s else 'srx_maxpool2x2_fwd', _p(x), _p(y), n, h, w, c, s)
            return y

        saved, ctx.plan = _stack_forward(x, layers, (), bf16s, ctx.needs_input_grad[0], pool, 'conv_stack', s)
        ctx.n_src = n_src
        ctx.masters = [conv.weight if kind == 'conv' else None for kind, conv in layers]
        ctx.save_for_backward(*saved)
        x = saved[-1]
        if target is None:
            return x, None
        fs, ft = x[:n_src], x[n_src:]
        ctx.mark_non_differentiable(ft)
        return fs, ft

    @staticmethod
    def backward(ctx, dfs: Tensor, _dft=None):
        saved, plan, n, bf16s = ctx.saved_tensors, ctx.plan, ctx.n_src, ctx.bf16s
        if dfs is None or not ctx.needs_input_grad[0]:
            return (None,) * len(ctx.needs_input_grad)
        s = _stream()
        g = _chk(dfs, 'conv_stack.grad')
        # the topmost activation's backward is the only elementwise pass
        top = saved[-1][:n]
        kind, st, _ = plan[-1]
        if bf16s:
            g2 = torch.empty(g.shape, dtype=torch.bfloat16, device=g.device)
            call('srx_act_bwd_from_out_to_bf16', _p(g), _p(top), _p(g2), g.numel(), ACT_RELU, 0.0, s)
            g = g2
        elif kind == 'conv':
            g2 = torch.empty_like(g)
            call('srx_act_bwd_from_out', _p(g), _p(top), _p(g2), g.numel(), st.act, st.slope, s)
            g = g2

        def pool_bwd(i: int, g: Tensor, x: Tensor) -> Tensor:
            _, h, w, c = x.shape
            if bf16s:                             # x: the fp32 output of the conv + ReLU below
                dx = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
                call('srx_maxpool2x2_relu_bwd_bf16', _p(g), _p(x), _p(dx), n, h, w, c, s)
                return dx
            below = plan[i - 1][1] if i > 0 and plan[i - 1][0] == 'conv' else None
            dx = torch.empty_like(x)
            # the pool's input is always a ReLU output in cfg 'E'; a pool fed by something else keeps the plain form
            if below is not None and below.act == ACT_RELU:
                call('srx_maxpool2x2_relu_bwd', _p(g), _p(x), _p(dx), n, h, w, c, s)
                return dx
            call('srx_maxpool2x2_bwd', _p(g), _p(x), _p(dx), n, h, w, c, s)
            if below is None:
                return dx
            g2 = torch.empty_like(dx)
            call('srx_act_bwd_from_out', _p(dx), _p(x), _p(g2), dx.numel(), below.act, below.slope, s)
            return g2

        g = _stack_backward(g, saved, plan, ctx.masters, n, bf16s, pool_bwd, s)
        return (g, None, None) + (None,) * (len(ctx.needs_input_grad) - 3)


def frozen_conv_stack(source: Tensor, target: Optional[Tensor], layers):
    """``layers``: [('conv', layers.Conv2d) | ('pool', None)].  Returns ``(features(source), features(target))``."""
    return _FrozenConvStack.apply(source, target, layers, *_stack_weights(layers, 'frozen_conv_stack'))


def _tap_stack_check(layers, taps) -> None:
    """The shape ``_FrozenTapStack`` is built for (VGG19 cfg 'E' with Real-ESRGAN's taps): 3x3 / stride 1 convs with a fused ReLU,
    except the taps, which write their pre-activation and are the last layer or sit in front of a pool; every pool behind a tap."""
    last = len(layers) - 1
    if not layers or layers[0][0] != 'conv' or 0 in taps or last not in taps or any(i < 0 or i > last for i in taps):
        raise RuntimeError('tap_stack: the stack starts with a conv that is no tap and ends with a tap')
    for i, (kind, conv) in enumerate(layers):
        if kind == 'pool':
            if i - 1 not in taps:
                raise RuntimeError('tap_stack: every pool follows a tap conv (the pool applies that tap\'s ReLU)')
            continue
        st = conv._st
        if st.stride != 1 or st.shuffle or st.act != (ACT_NONE if i in taps else ACT_RELU):
            raise RuntimeError('tap_stack: stride-1 convs, act NONE at the taps and a fused ReLU everywhere else')
        if i in taps and i != last and layers[i + 1][0] != 'pool':
            raise RuntimeError('tap_stack: a tap is the last layer or sits in front of a pool')
    # hence the taps are the convs that write fp32 under bf16 storage: the walk states that rule once, for both nodes
    assert all((i in taps) == _stack_writes_f32(layers, i) for i, (kind, _) in enumerate(layers) if kind == 'conv')


def _tap_stack_run(x: Tensor, n_src: int, layers, taps, tfeats, loss: Optional[Tensor], need_bwd: bool):
    """The forward launches of ``_FrozenTapStack`` on the normalised batch ``x`` (``[source; target]`` when it holds
    ``2 * n_src`` images): the shared walk with this node's pools.  ``loss`` given: every tap's ``weight * mean|fs - ft|`` is
    accumulated into it, ``ft`` being the target half or ``tfeats[k]``.  Returns ``(saved, plan, bf16s)``, as ``_stack_forward``."""
    L, s = _lib.lib(), _stream()
    pair = x.shape[0] == 2 * n_src
    bf16s = _bf16_stack_ok(layers, x.shape, taps)
    ws = _ws(1024, x) if loss is not None else None
    k, first = 0, 1

    def tap_l1(a: Tensor, b: Tensor, weight: float) -> None:
        nonlocal first
        if a.shape != b.shape:
            raise RuntimeError(f'tap_stack: target feature of shape {tuple(b.shape)}, the tap has {tuple(a.shape)}')
        call('srx_tap_l1_fwd', _p(a), _p(b), a.numel(), weight, _p(loss), 0 if first else 1, _p(ws), s)
        first = 0

    def pool(i: int, x: Tensor) -> Tensor:                  # x: the fp32 pre-activation of the tap conv below
        nonlocal k, first
        n, h, w, c = x.shape
        y = torch.empty((n, h // 2, w // 2, c), dtype=torch.bfloat16 if bf16s else torch.float32, device=x.device)
        fused = loss is not None and pair
        call('srx_maxpool2x2_relu_fwd_tap', _p(x), _p(y), 1 if bf16s else 0, n_src, n, h, w, c, _p(ws) if fused else None, s)
        if fused:
            call('srx_tap_l1_finalize', _p(ws), L.srx_tap_blocks(n_src, h, w, c), taps[i - 1] / float(n_src * h * w * c), _p(loss),
                 0 if first else 1, s)
            first = 0
        elif loss is not None:
            tap_l1(x[:n_src], tfeats[k], taps[i - 1])
        k += 1
        return y

    saved, plan = _stack_forward(x, layers, taps, bf16s, need_bwd, pool, 'tap_stack', s)
    if loss is not None:
        x = saved[-1]
        tap_l1(x[:n_src], x[n_src:] if pair else tfeats[k], taps[len(layers) - 1])
    return saved, plan, bf16s


class _FrozenTapStack(Function):
    """Real-ESRGAN's perceptual loss (BasicSR ``PerceptualLoss``: L1 on five VGG19 layers BEFORE their ReLU, ImageNet-normalised
    inputs) as ONE autograd node that returns the scalar ``sum_k w_k * mean|fs_k - ft_k|``; the feature tensors never leave it.

    In cfg 'E' the taps are the last conv in front of each pool plus the last conv, and ``maxpool(relu(x)) == relu(maxpool(x))``
    bit for bit: a tap conv writes its pre-activation (epilogue act NONE), the pool behind it applies the ReLU after the maximum
    and sums ``|fs - ft|`` over the windows it has loaded anyway (``srx_maxpool2x2_relu_fwd_tap``); the other convs keep their
    fused ReLU.  The convs, their plans and the choice between Winograd, the direct kernel and the bf16-storage path are the
    shared walk's (``_stack_forward`` / ``_stack_backward``); under bf16 storage the taps are exactly the layers that write fp32.

    This node's own: the normalisation in front, the tap pools with the L1 terms, and the backward, source half only: the loss
    gradient enters at the last tap (``srx_tap_l1_bwd_top``), descends through the walk's data-gradient calls with the non-tap
    ReLUs folded, and every pool backward adds its tap's L1 gradient in the same pass (``srx_maxpool2x2_relu_bwd_tap``)."""

    @staticmethod
    def forward(ctx, source: Tensor, target: Optional[Tensor], layers, taps, mean, inv_std, tfeats, *weights):
        ctx.set_materialize_grads(False)
        source = _chk(source, 'tap_stack.source')
        n, h, w, c = source.shape
        if c != 4:
            raise RuntimeError(f'tap_stack: NHWC images with 4 stored channels, got {c}')
        if target is not None:
            target = _chk(target, 'tap_stack.target')
            if target.shape != source.shape:
                raise RuntimeError(f'tap_stack: target of shape {tuple(target.shape)}, source {tuple(source.shape)}')
        x = torch.empty((n if target is None else 2 * n, h, w, 4), dtype=torch.float32, device=source.device)
        call('srx_normalize_pair_nhwc4', _p(source), _p(target), _p(x), n, h, w, mean, inv_std, _stream())
        loss = torch.empty((), dtype=torch.float32, device=source.device)
        saved, ctx.plan, ctx.bf16s = _tap_stack_run(x, n, layers, taps, tfeats, loss, ctx.needs_input_grad[0])
        ctx.n_src, ctx.taps, ctx.inv_std, ctx.n_feats = n, taps, inv_std, 0 if tfeats is None else len(tfeats)
        ctx.masters = [conv.weight if kind == 'conv' else None for kind, conv in layers]
        ctx.save_for_backward(*saved, *(tfeats or ()))
        return loss

    @staticmethod
    def backward(ctx, g: Tensor):
        if g is None or not ctx.needs_input_grad[0]:
            return (None,) * len(ctx.needs_input_grad)
        plan, n, taps, bf16s = ctx.plan, ctx.n_src, ctx.taps, ctx.bf16s
        saved = ctx.saved_tensors[:len(plan) + 1]
        tfeats = ctx.saved_tensors[len(plan) + 1:]
        s = _stream()
        gscale = _chk(g, 'tap_stack.grad')
        k = len(taps) - 1                          # the tap whose L1 term enters next, topmost first

        def target_of(feat: Tensor) -> Tensor:     # the other operand of tap k: the batch's second half, or the precomputed one
            return tfeats[k] if ctx.n_feats else feat[n:]

        top = saved[-1]
        fs = top[:n]
        g = torch.empty(fs.shape, dtype=torch.bfloat16 if bf16s else torch.float32, device=fs.device)
        call('srx_tap_l1_bwd_top', _p(fs), _p(target_of(top)), _p(g), 1 if bf16s else 0, taps[len(plan) - 1] / float(fs.numel()),
             _p(gscale), fs.numel(), s)

        def pool_bwd(i: int, g: Tensor, x: Tensor) -> Tensor:   # x: the fp32 pre-activation of tap i - 1
            nonlocal k
            k -= 1
            _, h, w, c = x.shape
            dx = torch.empty(x.shape, dtype=g.dtype, device=x.device)
            call('srx_maxpool2x2_relu_bwd_tap', _p(g), 1 if bf16s else 0, _p(x), _p(target_of(saved[i])), _p(dx), 1 if bf16s else 0,
                 taps[i - 1] / float(x.numel()), _p(gscale), n, h, w, c, s)
            return dx

        # (a conv below a conv is never a tap: the activation the walk folds into a data gradient is always a ReLU)
        g = _stack_backward(g, saved, plan, ctx.masters, n, bf16s, pool_bwd, s)
        dsrc = torch.empty_like(g)
        call('srx_normalize_nhwc4_bwd', _p(g), _p(dsrc), n, g.shape[1], g.shape[2], ctx.inv_std, s)
        return (dsrc,) + (None,) * (len(ctx.needs_input_grad) - 1)


def _tap_stack_args(layers, taps, mean, std):
    weights = _stack_weights(layers, 'frozen_tap_stack')
    taps = {int(i): float(wt) for i, wt in taps.items()}
    _tap_stack_check(layers, taps)
    f3 = C.c_float * 3
    return weights, taps, f3(*[float(m) for m in mean]), f3(*[1.0 / float(v) for v in std])


def frozen_tap_stack(source: Tensor, target: Optional[Tensor], layers, taps, mean, std, target_features=None) -> Tensor:
    """``sum_k taps[i_k] * mean|f_k(source) - f_k(target)|`` over the pre-activation outputs ``f_k`` of the convs at positions
    ``i_k`` of ``layers`` ([('conv', layers.Conv2d) | ('pool', None)]), both images normalised by ``mean`` / ``std`` first.
    ``target`` None: ``target_features`` holds the taps' precomputed target features (``frozen_tap_features``), shallow to deep."""
    weights, taps, mean, inv_std = _tap_stack_args(layers, taps, mean, std)
    if (target is None) == (target_features is None):
        raise RuntimeError('frozen_tap_stack: pass either target or target_features')
    tfeats = None
    if target_features is not None:
        tfeats = [_chk(t, 'tap_stack.target_features') for t in target_features]
        if len(tfeats) != len(taps):
            raise RuntimeError(f'frozen_tap_stack: {len(taps)} taps, {len(tfeats)} target features')
    return _FrozenTapStack.apply(source, target, layers, taps, mean, inv_std, tfeats, *weights)


@torch.no_grad()
def frozen_tap_features(image: Tensor, layers, taps, mean, std):
    """The taps' pre-activation features of ``image`` (a detached target), shallow to deep: ``frozen_tap_stack``'s forward
    launches on a batch of its own, no loss and no autograd state."""
    _, taps, mean, inv_std = _tap_stack_args(layers, taps, mean, std)
    image = _chk(image, 'tap_stack.image')
    n, h, w, c = image.shape
    if c != 4:
        raise RuntimeError(f'tap_stack: NHWC images with 4 stored channels, got {c}')
    x = torch.empty_like(image)
    call('srx_normalize_pair_nhwc4', _p(image), None, _p(x), n, h, w, mean, inv_std, _stream())
    saved, _, _ = _tap_stack_run(x, n, layers, taps, None, None, False)
    return [saved[i + 1] for i in sorted(taps)]


# --------------------------------------------------------------------------- linear
class _Linear(Function):
    @staticmethod
    def forward(ctx, x: Tensor, w: Tensor, bias: Optional[Tensor], act: int, slope: float):
        ctx.set_materialize_grads(False)
        x = _chk(x, 'linear.input')
        wd = _chk(w.detach(), 'linear.weight')
        bsz, k = x.shape
        j = wd.shape[0]
        y = torch.empty((bsz, j), dtype=torch.float32, device=x.device)
        nws = _lib.lib().srx_linear_ws_floats(bsz, k, j)
        b = None if bias is None else _chk(bias.detach(), 'linear.bias')
        call('srx_linear_fwd', _p(x), _p(wd), _p(b), _p(y), bsz, k, j, act, slope, _p(_ws(nws, x)), nws, _stream())
        ctx.cfg = (bsz, k, j, act, slope, bias is not None, nws)
        ctx.params = (w, bias)
        ctx.save_for_backward(x, wd, y if act != ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        x, w, y = ctx.saved_tensors
        bsz, k, j, act, slope, has_bias, nws = ctx.cfg
        dy = _chk(dy, 'linear.grad')
        s = _stream()
        if act != ACT_NONE:
            g = torch.empty_like(dy)
            call('srx_act_bwd_from_out', _p(dy), _p(y), _p(g), dy.numel(), act, slope, s)
            dy = g
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            call('srx_linear_bwd_data', _p(dy), _p(w), _p(dx), bsz, k, j, _p(_ws(nws, x)), nws, s)
        wparam, bparam = ctx.params
        if ctx.needs_input_grad[1]:
            sink = _sink(wparam)
            dw = None if sink is not None else torch.empty_like(w)
            call('srx_linear_bwd_weight', _p(x), _p(dy), _p(dw if sink is None else sink), 0 if sink is None else 1,
                 bsz, k, j, s)
        if has_bias and ctx.needs_input_grad[2]:
            sink = _sink(bparam)
            db = None if sink is not None else torch.empty(j, dtype=torch.float32, device=x.device)
            _colsum(_p(dy), bsz, j, j, db if sink is None else sink, 0 if sink is None else 1, x, s)
        return dx, dw, db, None, None


def linear(x: Tensor, w: Tensor, bias: Optional[Tensor], act: int = ACT_NONE, slope: float = 0.0) -> Tensor:
    return _Linear.apply(x, w, bias, act, float(slope))


class _GanHead(Function):
    """Discriminator head + adversarial loss of a GAN train step as ONE autograd node (csrc/head.hip):
    ``hidden = LeakyReLU(Linear1(x))`` on the streaming linear kernels, then last Linear -> [Sigmoid] -> loss in one
    launch, and in the backward pass one launch for everything between the loss and the hidden layer's pre-activation
    (loss, sigmoid, last Linear, LeakyReLU backwards; both bias gradients and the last weight gradient) followed by the
    hidden layer's data and weight gradients.  Returns ``(loss, aux)``; ``aux`` (8 floats, no gradient) holds the terms.
    """

    @staticmethod
    def forward(ctx, x: Tensor, w1: Tensor, b1: Optional[Tensor], w2: Tensor, b2: Optional[Tensor], mode: int, n_first: int,
                slope: float, adv_weight: float, shift: Optional[Tensor], addend: Optional[Tensor]):
        ctx.set_materialize_grads(False)
        x = _chk(x, 'gan_head.input')
        w1d, w2d = _chk(w1.detach(), 'gan_head.weight1'), _chk(w2.detach(), 'gan_head.weight2')
        bsz, k = x.shape
        j = w1d.shape[0]
        if w2d.numel() != j:
            raise RuntimeError(f'gan_head: the last layer must map {j} hidden units to ONE output, got {tuple(w2d.shape)}')
        s = _stream()
        hidden = torch.empty((bsz, j), dtype=torch.float32, device=x.device)
        nws = _lib.lib().srx_linear_ws_floats(bsz, k, j)
        b1d = None if b1 is None else _chk(b1.detach(), 'gan_head.bias1')
        b2d = None if b2 is None else _chk(b2.detach(), 'gan_head.bias2')
        call('srx_linear_fwd', _p(x), _p(w1d), _p(b1d), _p(hidden), bsz, k, j, ACT_LRELU, slope, _p(_ws(nws, x)), nws, s)
        h = _lib.GanHead(mode, bsz, j, n_first, slope, adv_weight)
        zp = torch.empty(bsz, dtype=torch.float32, device=x.device)
        out = torch.empty(8, dtype=torch.float32, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        sh = None if shift is None else _chk(shift.detach().reshape(1), 'gan_head.shift')
        ad = None if addend is None else _chk(addend.detach().reshape(1), 'gan_head.addend')
        call('srx_gan_head_fwd', C.byref(h), _p(hidden), _p(w2d), _p(b2d), _p(sh), _p(ad), _p(zp), _p(out), _p(loss), s)
        ctx.h, ctx.nws = h, nws
        ctx.params = (w1, b1, w2, b2)
        ctx.save_for_backward(x, w1d, w2d, hidden, zp, out, sh)
        ctx.mark_non_differentiable(out)
        return loss, out

    @staticmethod
    def backward(ctx, g: Tensor, _gaux=None):
        x, w1, w2, hidden, zp, out, sh = ctx.saved_tensors
        h = ctx.h
        bsz, k = x.shape
        j = h.J
        s = _stream()
        g = _chk(g, 'gan_head.grad').reshape(1)
        w1p, b1p, w2p, b2p = ctx.params
        need = ctx.needs_input_grad  # (x, w1, b1, w2, b2, ..., shift, addend)
        dw1 = db1 = dw2 = db2 = None
        sinks = [(_sink(p) if (p is not None and need[i + 1]) else None) for i, p in enumerate(ctx.params)]
        wanted = [p is not None and need[i + 1] for i, p in enumerate(ctx.params)]
        # the small gradients either ALL accumulate into flat .grad buffers (the trainers) or are all returned
        direct = all(sk is not None for sk, wnt in zip(sinks, wanted) if wnt) and any(wanted)
        ptrs = [None, None, None, None]
        if not direct:
            if wanted[1]:
                db1 = torch.empty(j, dtype=torch.float32, device=x.device)
            if wanted[2]:
                dw2 = torch.empty_like(w2)
            if wanted[3]:
                db2 = torch.empty(1, dtype=torch.float32, device=x.device)
            ptrs = [None, _p(db1), _p(dw2), _p(db2)]
        else:
            ptrs = [None] + [_p(sk) if wnt else None for sk, wnt in list(zip(sinks, wanted))[1:]]
        dpre = torch.empty((bsz, j), dtype=torch.float32, device=x.device)
        call('srx_gan_head_bwd', C.byref(h), _p(hidden), _p(w2), _p(zp), _p(out), _p(sh), _p(g), _p(dpre), ptrs[2], ptrs[3],
             ptrs[1], 1 if direct else 0, s)
        dx = None
        if need[0]:
            dx = torch.empty_like(x)
            call('srx_linear_bwd_data', _p(dpre), _p(w1), _p(dx), bsz, k, j, _p(_ws(ctx.nws, x)), ctx.nws, s)
        if wanted[0]:
            sink = sinks[0] if direct else None
            if sink is None:
                dw1 = torch.empty_like(w1)
            call('srx_linear_bwd_weight', _p(x), _p(dpre), _p(dw1 if sink is None else sink), 0 if sink is None else 1, bsz, k, j, s)
        dadd = g.view(()) if need[10] else None
        return dx, dw1, db1, (None if dw2 is None else dw2.view_as(w2p)), db2, None, None, None, None, None, dadd


def gan_head(x: Tensor, lin1, lin2, mode: int, n_first: int = 0, slope: float = 0.2, adv_weight: float = 1.0,
             shift: Optional[Tensor] = None, addend: Optional[Tensor] = None):
    """``(loss, aux)`` of a discriminator's classifier (``lin1`` -> LeakyReLU -> ``lin2`` [-> Sigmoid]) and the adversarial
    loss behind it on the flattened features ``x`` [B, K]; modes and ``aux`` layout: ``srx_gan_head_t`` in include/srx.h.
    ``lin1`` / ``lin2`` are ``layers.Linear`` modules (``no_weight_grad`` is honoured)."""
    from .layers import _w
    return _GanHead.apply(x, _w(lin1.weight), _w(lin1.bias), _w(lin2.weight), _w(lin2.bias), int(mode), int(n_first), float(slope),
                          float(adv_weight), shift, addend)


# --------------------------------------------------------------------------- losses
class _PairLoss(Function):
    """mean((a-b)^2) / mean(|a-b|); ``count``: the mean's divisor when not every stored element is a real one"""

    @staticmethod
    def forward(ctx, a: Tensor, b: Tensor, kind: str, count: int = 0):
        ctx.set_materialize_grads(False)
        a, b = _chk(a, f'{kind}.input'), _chk(b, f'{kind}.target')
        if a.shape != b.shape:
            raise RuntimeError(f'{kind}_loss: shape mismatch {tuple(a.shape)} vs {tuple(b.shape)}')
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        if count:
            call(f'srx_{kind}_fwd_count', _p(a), _p(b), _p(loss), a.numel(), count, _p(_ws(2048, a)), _stream())
        else:
            call(f'srx_{kind}_fwd', _p(a), _p(b), _p(loss), a.numel(), _p(_ws(2048, a)), _stream())
        ctx.kind, ctx.count = kind, count
        ctx.save_for_backward(a, b)
        return loss

    @staticmethod
    def backward(ctx, g: Tensor):
        a, b = ctx.saved_tensors
        g = _chk(g, 'loss.grad')
        da = torch.empty_like(a)
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        if ctx.count:
            call(f'srx_{ctx.kind}_bwd_count', _p(a), _p(b), _p(g), _p(da), _p(db), a.numel(), ctx.count, _stream())
        else:
            call(f'srx_{ctx.kind}_bwd', _p(a), _p(b), _p(g), _p(da), _p(db), a.numel(), _stream())
        return (da if ctx.needs_input_grad[0] else None), db, None, None


def mse_loss(a: Tensor, b: Tensor) -> Tensor:
    """nn.MSELoss() (srgan/trainer.py:163)."""
    return _PairLoss.apply(a, b, 'mse')


def l1_loss(a: Tensor, b: Tensor, count: int = 0) -> Tensor:
    """F.l1_loss / nn.L1Loss() (srgan/loss.py:52).  ``count``: divisor of the mean when the tensors carry padding (NHWC images
    with a zero 4th channel: ``count = 3 * pixels``)."""
    return _PairLoss.apply(a, b, 'l1', int(count))


class _BCE(Function):
    @staticmethod
    def forward(ctx, p: Tensor, target: float):
        ctx.set_materialize_grads(False)
        p = _chk(p, 'bce.input')
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        call('srx_bce_fwd', _p(p), target, _p(loss), p.numel(), _p(_ws(2048, p)), _stream())
        ctx.target = target
        ctx.save_for_backward(p)
        return loss

    @staticmethod
    def backward(ctx, g: Tensor):
        (p,) = ctx.saved_tensors
        g = _chk(g, 'bce.grad')
        dp = torch.empty_like(p)
        call('srx_bce_bwd', _p(p), ctx.target, _p(g), _p(dp), p.numel(), _stream())
        return dp, None


def bce_loss(p: Tensor, target: float) -> Tensor:
    """nn.BCELoss() against a constant label tensor (srgan/trainer.py:439-447)."""
    return _BCE.apply(p, float(target))


class _BCELogits(Function):
    @staticmethod
    def forward(ctx, x: Tensor, shift: Optional[Tensor], target: float):
        ctx.set_materialize_grads(False)
        x = _chk(x, 'bce_logits.input')
        sh = None if shift is None else _chk(shift.detach().reshape(1), 'bce_logits.shift')
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        call('srx_bce_logits_fwd', _p(x), _p(sh), target, _p(loss), x.numel(), _p(_ws(2048, x)), _stream())
        ctx.target = target
        ctx.save_for_backward(x, sh)
        return loss

    @staticmethod
    def backward(ctx, g: Tensor):
        x, sh = ctx.saved_tensors
        g = _chk(g, 'bce_logits.grad')
        dx = torch.empty_like(x)
        call('srx_bce_logits_bwd', _p(x), _p(sh), ctx.target, _p(g), _p(dx), x.numel(), _stream())
        dsh = None
        if sh is not None and ctx.needs_input_grad[1]:
            dsh = -dx.sum()  # one scalar; plumbing
        return dx, dsh, None


def bce_with_logits(x: Tensor, target: float, shift: Optional[Tensor] = None) -> Tensor:
    """nn.BCEWithLogitsLoss()(x - shift, full(target)) (esrgan/trainer.py:451-453)."""
    return _BCELogits.apply(x, shift, float(target))


class _Mean(Function):
    @staticmethod
    def forward(ctx, x: Tensor):
        ctx.set_materialize_grads(False)
        x = _chk(x, 'mean.input')
        out = torch.empty((), dtype=torch.float32, device=x.device)
        call('srx_mean_fwd', _p(x), _p(out), x.numel(), _p(_ws(2048, x)), _stream())
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        (x,) = ctx.saved_tensors
        g = _chk(g, 'mean.grad')
        dx = torch.empty_like(x)
        call('srx_mean_bwd', _p(x), _p(g), _p(dx), x.numel(), _stream())
        return dx


class _SplitBatch(Function):
    """``(x[:n], x[n:])`` of a batch-major tensor as two independent tensors; the backward is one concatenation."""

    @staticmethod
    def forward(ctx, x: Tensor, n: int):
        ctx.set_materialize_grads(False)
        ctx.shape, ctx.n = x.shape, n
        return x[:n].clone(), x[n:].clone()

    @staticmethod
    def backward(ctx, da, db):
        n, shape = ctx.n, ctx.shape
        ref = da if da is not None else db
        if ref is None:
            return None, None
        if da is None:
            da = torch.zeros((n,) + tuple(shape[1:]), dtype=ref.dtype, device=ref.device)
        if db is None:
            db = torch.zeros((shape[0] - n,) + tuple(shape[1:]), dtype=ref.dtype, device=ref.device)
        return torch.cat([da, db], dim=0), None


def split_batch(x: Tensor, n: int):
    return _SplitBatch.apply(x, n)


def mean(x: Tensor) -> Tensor:
    """torch.mean(x) over all elements (esrgan/trainer.py:451-452)."""
    return _Mean.apply(x)


# --------------------------------------------------------------------------- ESRGAN helpers
class _ConcatChannels(Function):
    """torch.cat(tensors, dim=1) of the reference's NCHW tensors == channel concat in NHWC."""

    @staticmethod
    def forward(ctx, *xs: Tensor):
        ctx.set_materialize_grads(False)
        xs = [_chk(x, 'concat.input') for x in xs]
        lead = xs[0].shape[:-1]
        cs = [x.shape[-1] for x in xs]
        m = xs[0].numel() // cs[0]
        out = torch.empty(tuple(lead) + (sum(cs),), dtype=torch.float32, device=xs[0].device)
        off, s = 0, _stream()
        for x, c in zip(xs, cs):
            call('srx_copy_channels', _p(x), c, 0, _p(out), sum(cs), off, c, m, 0, s)
            off += c
        ctx.cs, ctx.m = cs, m
        return out

    @staticmethod
    def backward(ctx, dy: Tensor):
        dy = _chk(dy, 'concat.grad')
        total, s = sum(ctx.cs), _stream()
        grads, off = [], 0
        for i, c in enumerate(ctx.cs):
            if ctx.needs_input_grad[i]:
                g = torch.empty(dy.shape[:-1] + (c,), dtype=torch.float32, device=dy.device)
                call('srx_copy_channels', _p(dy), total, off, _p(g), c, 0, c, ctx.m, 0, s)
                grads.append(g)
            else:
                grads.append(None)
            off += c
        return tuple(grads)


class FoldedConv:
    """Inference form of ``conv [-> BatchNorm2d (running statistics)] [-> PReLU] [+ residual]``: ONE kernel.

    The eval-mode BatchNorm is an affine map per output channel, so it folds into the conv's weights and
    bias (``w' = w * g / sqrt(var + eps)``, ``b' = (b - mean) * g / sqrt(var + eps) + beta``); a
    single-parameter PReLU is the conv epilogue's LeakyReLU with the learnt slope (it commutes with the
    fused PixelShuffle); the skip connection is the epilogue's addend (``srx_conv2d_fwd_residual``).
    Replaces an elementwise pass over the activation per BatchNorm / PReLU of the generator at inference
    (SURVEY.md section 8f row 1).  Folded tensors are cached and rebuilt when any source tensor changes.

    A PReLU with one slope per output channel (the compact generator) stays a vector: the 16-bit chain reads it in the conv's
    epilogue (``srx_conv3x3_c64_*_fwd_slopes``); in fp32 the conv runs without activation and ``srx_prelu_channels_fwd``
    follows in place (``ConvState`` and ``srx_conv2d_t`` keep their single slope).  ``pad16``: a 64-input 3x3 layer with fewer
    than 64 outputs joins the 16-bit chain as a 64-output layer whose surplus filters and biases are zero.
    """

    def __init__(self, conv, bn=None, prelu=None, pad16: bool = False):
        self.conv, self.bn, self.prelu = conv, bn, prelu
        self.pad16 = bool(pad16)
        self.slopes = None  # per-channel PReLU: the slope vector (fp32, on the device)
        self._key = None
        self.st = None
        self.pack16 = WeightPack()  # the weights of the 16-bit-native chain (csrc/c64.hip)

    def _sources(self):
        ts = [self.conv.weight, self.conv.bias]
        if self.bn is not None:
            ts += [self.bn.weight, self.bn.bias, self.bn.running_mean, self.bn.running_var]
        if self.prelu is not None:
            ts.append(self.prelu.weight)
        return [t for t in ts if t is not None]

    def _refresh(self) -> None:
        key = tuple((t.data_ptr(), t._version) for t in self._sources()) + (_pack_epoch[0], self.conv._st.model_epoch[0],
                                                                            self.conv._st.precision)
        if key == self._key:
            return
        conv, bn = self.conv, self.bn
        with torch.no_grad():
            w = conv.weight.detach()
            b = conv.bias.detach() if conv.bias is not None else None
            if bn is not None:
                scale = bn.weight.detach() * torch.rsqrt(bn.running_var + bn.eps)
                w = w * scale.view(-1, 1, 1, 1)
                b = ((b if b is not None else 0.0) - bn.running_mean) * scale + bn.bias.detach()
            self.w = w.contiguous()
            self.b = None if b is None else b.contiguous()
            src = conv._st
            act, slope = src.act, src.slope
            self.slopes = None
            if self.prelu is not None and self.prelu.weight.numel() > 1:
                if self.prelu.weight.numel() != src.cout or src.act != ACT_NONE or src.shuffle:
                    raise RuntimeError('FoldedConv: a per-channel PReLU has one slope per output channel and follows a linear '
                                       'conv without PixelShuffle')
                self.slopes = _slopes16(self.prelu.weight.detach())
            elif self.prelu is not None:
                if self.prelu.weight.numel() != 1 or src.act != ACT_NONE:
                    raise RuntimeError('FoldedConv: PReLU must have one parameter and follow a linear conv')
                act, slope = ACT_LRELU, float(self.prelu.weight.detach().reshape(()).item())
            self.st = ConvState(src.cin, src.cout, src.k, src.stride, src.pad, shuffle=src.shuffle, act=act, slope=slope,
                                up=src.up)
            self.st.precision = src.precision
        self._key = key

    def bf16_native_ok(self) -> bool:
        """3x3 / stride 1 / pad 1, 64 input channels, a multiple of 64 outputs: the layers ``srx_conv3x3_c64_bf16_fwd`` runs."""
        st = self.conv._st
        return (st.k == 3 and st.stride == 1 and st.pad == 1 and st.cin == 64 and st.up == 0
                and (st.cout % 64 == 0 or (self.pad16 and st.cout < 64 and st.shuffle == 0))
                and (st.shuffle == 0 or (st.shuffle == 2 and st.cout == 256)))

    def _call_bf16(self, x: Tensor, residual: Optional[Tensor]) -> Tensor:
        """16 bits in, the same 16 bits out: the 16-bit-native chain (activations stored as bf16 or fp16 -- the input's dtype
        picks ``srx_conv3x3_c64_bf16_*`` or ``srx_conv3x3_c64_f16_*`` --, weights resident in registers)."""
        st = self.st
        if not self.bf16_native_ok():
            raise RuntimeError('folded_conv: a 16-bit input needs a 3x3 / 64-input-channel layer')
        _chk_f16_inference(st, 'folded_conv')
        x = _chk16(x, 'folded_conv.input', None)
        dt = x.dtype
        sfx = 'f16' if dt == torch.float16 else 'bf16'
        n, h, w, cs = x.shape
        if cs != 64:
            raise RuntimeError(f'folded_conv: {sfx} input has {cs} channels, the layer expects 64')
        cout = (st.cout + 63) // 64 * 64  # (pad16: the layer as the kernel sees it)

        def pack(fwd, bwd, _):
            wsrc, bsrc = self.w, self.b
            if cout != st.cout:  # zero filters and biases: the surplus channels come out as 0 and nobody reads them
                wsrc = torch.cat([wsrc, wsrc.new_zeros((cout - st.cout,) + tuple(wsrc.shape[1:]))]).contiguous()
                bsrc = None if bsrc is None else torch.cat([bsrc, bsrc.new_zeros(cout - st.cout)]).contiguous()
            call(f'srx_conv3x3_c64_{sfx}_pack', _p(wsrc), _p(bsrc), None, cout, st.shuffle, _p(fwd), _stream())

        self.pack16.ensure(  # (keyed by the storage type too: fp16 and bf16 packs differ)
            (self._key, dt), x.device, False, lambda: (_lib.lib().srx_conv3x3_c64_bf16_packed_bytes(cout), 0, torch.uint8), pack)
        y = torch.empty(st.out_shape(n, h, w) if cout == st.cout else (n, h, w, cout), dtype=dt, device=x.device)
        slope = 1.0 if st.act == ACT_NONE else (0.0 if st.act == ACT_RELU else st.slope)
        r = None
        if residual is not None:
            r = _chk16(residual, 'folded_conv.residual', dt)
            if r.shape != y.shape:
                raise RuntimeError('folded_conv: residual must have the output shape')
        if self.slopes is not None:
            call(f'srx_conv3x3_c64_{sfx}_fwd_slopes', n, h, w, cout, st.shuffle, _p(x), _p(self.pack16.fwd), _p(self.slopes), _p(r),
                 _p(y), y.shape[3], _stream())
            return y
        call(f'srx_conv3x3_c64_{sfx}_fwd', n, h, w, cout, st.shuffle, _p(x), _p(self.pack16.fwd), float(slope), _p(r), _p(y),
             y.shape[3], _stream())
        return y

    def _finish_slopes(self, y: Tensor, r: Optional[Tensor]) -> Tensor:
        """fp32, per-channel PReLU: the conv ran without activation; the slopes in place, then the addend -- the order of the
        16-bit epilogue."""
        call('srx_prelu_channels_fwd', _p(y), _p(self.slopes), _p(y), y.numel() // y.shape[3], self.st.cout, y.shape[3], _stream())
        if r is not None:
            call('srx_axpby', _p(y), _p(r), _p(y), y.numel(), 1.0, 1.0, _stream())
        return y

    def __call__(self, x: Tensor, residual: Optional[Tensor] = None) -> Tensor:
        self._refresh()
        if x.dtype in _STORE16:
            return self._call_bf16(x, residual)
        st = self.st
        if st.precision == PRECISION_F16 and self.bf16_native_ok():
            raise RuntimeError('folded_conv: with fp16 precision (3) a 64-channel layer takes an fp16 input (no fp32 fallback)')
        x = _chk(x, 'folded_conv.input')
        n, h, w, cs = x.shape
        if cs != st.cin_s:
            raise RuntimeError(f'folded_conv: input has {cs} channels (stride), layer expects {st.cin_s}')
        d = st.desc(n, h, w)
        y = torch.empty(st.out_shape(n, h, w), dtype=torch.float32, device=x.device)
        r = None
        if residual is not None:
            r = _chk(residual, 'folded_conv.residual')
            if r.shape != y.shape:
                raise RuntimeError('folded_conv: residual must have the output shape')
        # exact-fp32 inference: the 3x3 layers of the trunk as Winograd F(2x2, 3x3) (csrc/wino.hip; 4/9 of the multiplications,
        # PReLU / skip in its epilogue) -- at 1080p each 64 -> 64 layer is 16 200 tile blocks
        if (st.precision == 0 and not _dev.NO_WINO and st.act in (ACT_NONE, ACT_RELU, ACT_LRELU)
                and _lib.lib().srx_wino_infer_applicable(C.byref(d)) == 1):
            st.pack_wino(self.w, d, need_bwd=False)
            dref = C.byref(d)
            nws = _lib.lib().srx_wino_ws_floats(dref, 0)
            ws = _ws(nws, x) if nws else None
            call('srx_wino_fwd_act', dref, _p(x), _p(st.wino_fwd), _p(self.b), None if self.slopes is not None else _p(r), _p(y),
                 _p(ws), nws, _stream())
            return y if self.slopes is None else self._finish_slopes(y, r)
        st.pack(self.w, d)
        if self.slopes is not None:
            _conv_fwd(d, _p(x), _p(st.wpk_fwd), _p(self.b), _p(y), x, _stream())
            return self._finish_slopes(y, r)
        _conv_fwd(d, _p(x), _p(st.wpk_fwd), _p(self.b), _p(y), x, _stream(), residual=None if residual is None else (_p(r), 1.0))
        return y


def inference_mode(module) -> bool:
    """The folded single-kernel forms apply when nothing will be differentiated and BatchNorm is in eval mode."""
    return not module.training and not torch.is_grad_enabled()


def concat_channels(xs) -> Tensor:
    return _ConcatChannels.apply(*xs)


class _DenseBlock(Function):
    """ESRGAN's ResidualDenseBlock as ONE autograd node (esrgan/residual.py:65-86).

    ``c_k = LeakyReLU(conv_k(cat(x, c_1..c_{k-1})))`` for k = 1..4, ``y = conv_5(cat(x, c_1..c_4)) * scale + x``.
    The five ``torch.cat`` copies (64+96+128+160+192 channels per pixel, and as many again in the
    backward) are replaced by one ``[N,H,W,64+4*32]`` buffer: conv_k reads its first ``64 + 32(k-1)``
    channels (channel stride 192) and writes its 32 outputs right behind them; in the backward the
    input gradients of all five convs are summed in place in a second buffer of the same shape
    (``srx_conv2d_bwd_data(..., accumulate=1)``), which is exactly the adjoint of the concatenations.
    """

    @staticmethod
    def forward(ctx, x: Tensor, scale: float, states, masters, *wb):
        ctx.set_materialize_grads(False)
        x = _chk(x, 'dense_block.input')
        n, h, w, c0 = x.shape
        g = states[0].cout
        total = c0 + 4 * g
        m = n * h * w
        s = _stream()
        dev = x.device
        buf = torch.empty((n, h, w, total), dtype=torch.float32, device=dev)
        call('srx_copy_channels', _p(x), c0, 0, _p(buf), total, 0, c0, m, 0, s)
        descs = []
        for k in range(5):
            st = states[k]
            cin = c0 + k * g
            last = k == 4
            d = Conv2dDesc(n, h, w, cin, total, st.cout, st.cout if last else total, st.k, st.k, st.stride, st.pad, 0,
                           st.act, st.slope, 0, st.precision)
            descs.append(d)
            st.pack(masters[k], d)
            bias = wb[2 * k + 1]
            bp = None if bias is None else _p(_chk(bias.detach(), 'dense_block.bias'))
            if last:  # y = conv5(...) * scale + x in the conv's epilogue (esrgan/residual.py:86)
                y = torch.empty_like(x)
                _conv_fwd(d, _p(buf), _p(st.wpk_fwd), bp, _p(y), x, s, residual=(_p(x), float(scale)))
            else:
                _conv_fwd(d, _p(buf), _p(st.wpk_fwd), bp, buf.data_ptr() + 4 * cin, x, s)
        ctx.states, ctx.descs, ctx.scale = states, descs, float(scale)
        ctx.dims = (n, h, w, c0, g, total, m)
        ctx.params = wb
        ctx.packs = [st.wpk_bwd for st in states]
        ctx.save_for_backward(buf)
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        (buf,) = ctx.saved_tensors
        dy = _chk(dy, 'dense_block.grad')
        n, h, w, c0, g, total, m = ctx.dims
        s = _stream()
        dev = dy.device
        gbuf = torch.empty((n, h, w, total), dtype=torch.float32, device=dev)
        g5 = torch.empty_like(dy)
        call('srx_axpby', _p(dy), _p(dy), _p(g5), dy.numel(), ctx.scale, 0.0, s)
        grads = [None] * 10
        for k in (4, 3, 2, 1, 0):
            st, d = ctx.states[k], ctx.descs[k]
            cin = c0 + k * g
            if k == 4:
                gk, ldg = g5.data_ptr(), st.cout
            else:  # this conv's output gradient is complete AND masked: the data gradient of conv k+1 finished the slice
                gk, ldg = gbuf.data_ptr() + 4 * cin, total
            grads[2 * k], grads[2 * k + 1] = _conv_param_grads(
                st, d, _p(buf), gk, m, ldg, ctx.params[2 * k] if ctx.needs_input_grad[4 + 2 * k] else None,
                ctx.params[2 * k + 1] if ctx.needs_input_grad[5 + 2 * k] else None, (buf, gbuf, g5), dy, s)
            if k > 0 or ctx.needs_input_grad[0]:
                # conv5 writes all `total` channels; the others add their share to the first `cin`.  The slice of
                # conv k's output, channels [cin - g, cin), is complete with this call (every later conv has added
                # its share): the LeakyReLU backward of conv k (esrgan/residual.py:81-84) is applied to it on the way out
                mask = (_p(buf), ctx.states[k - 1].slope, cin - g, cin) if k > 0 else None
                _conv_dgrad(d, gk, _p(ctx.packs[k]), _p(gbuf), dy, s, accumulate=0 if k == 4 else 1, mask=mask)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(dy)
            call('srx_copy_channels', _p(gbuf), total, 0, _p(dx), c0, 0, c0, m, 0, s)
            call('srx_axpby', _p(dx), _p(dy), _p(dx), dy.numel(), 1.0, 1.0, s)
        return (dx, None, None, None, *grads)


def dense_block(x: Tensor, scale: float, convs) -> Tensor:
    """``convs``: the block's five ``layers.Conv2d`` modules (conv1..conv5)."""
    from .layers import _w
    wb = []
    for c in convs:
        wb += [_w(c.weight), _w(c.bias)]
    return _DenseBlock.apply(x, scale, [c._st for c in convs], [c.weight for c in convs], *wb)


class RDBPack:
    """The bf16 weight streams of a chain of dense blocks for the one-launch forward (``srx_rdb_fwd``): one
    ``srx_rdb_pack`` launch for all blocks, re-run when any weight changed (the same staleness key as ``ConvState.pack``)."""

    def __init__(self):
        self.pack = WeightPack()
        self.table = None  # the masters' addresses, in device memory
        self.per_block = 0

    def ensure(self, states, masters, need_bwd: bool = False) -> None:
        ws = [w for row in masters for w in row]
        key = (ws[0].data_ptr(), len(ws), _pack_epoch[0], states[0][0].model_epoch[0], sum(w._version for w in ws))
        dev = ws[0].device

        def size():
            self.per_block = self.per_block or int(_lib.lib().srx_rdb_packed_bytes())
            return (len(states) * self.per_block,) * 2 + (torch.uint8,)

        def run(fwd, bwd, bwd_only):
            ptrs = [w.data_ptr() for w in ws]
            if self.table is None or self.table.numel() != len(ws) or self.table.device != dev:
                self.table = torch.tensor(ptrs, dtype=torch.int64).to(dev)
            elif self._ptrs != ptrs:
                self.table.copy_(torch.tensor(ptrs, dtype=torch.int64))
            self._ptrs = ptrs
            if not bwd_only:
                call('srx_rdb_pack', _p(self.table), len(states), _p(fwd), _stream())
            if bwd is not None:  # the transposed, tap-flipped streams of the data-gradient chain (srx_rdb_bwd)
                call('srx_rdb_pack_bwd', _p(self.table), len(states), _p(bwd), _stream())

        self.pack.ensure(key, dev, need_bwd, size, run)

    def block_ptr(self, i: int) -> int:
        return self.pack.fwd.data_ptr() + i * self.per_block

    def bwd_ptr(self, i: int) -> int:
        return self.pack.bwd.data_ptr() + i * self.per_block


def rdb_fused_ok(states, wb_row, c0: int) -> bool:
    """The one-launch dense block applies to the reference's geometry (64 + 4 x 32 channels, 3x3 / stride 1 / pad 1,
    LeakyReLU on conv1..4, biases) with bf16 products; ``SRX_NO_RDB_FUSED=1`` keeps the per-conv launches (A/B runs)."""
    if _dev.NO_RDB_FUSED or c0 != 64 or len(states) != 5:
        return False
    for k, st in enumerate(states):
        if (st.precision != 1 or st.k != 3 or st.stride != 1 or st.pad != 1 or st.shuffle or st.up or st.cin != 64 + 32 * k
                or st.cout != (64 if k == 4 else 32) or st.act != (ACT_NONE if k == 4 else ACT_LRELU)):
            return False
        if k < 4 and st.slope != states[0].slope:
            return False
    return all(wb_row[2 * k + 1] is not None for k in range(5))


class _RRDBTrunk(Function):
    """ESRGAN's chain of residual-in-residual dense blocks (esrgan/generator.py:54-56,70; esrgan/residual.py:81-86,
    125-128) as ONE autograd node, so that nothing but convolutions touches the activations.

    Every dense block owns a ``[N,H,W,64+4*32]`` buffer as in ``_DenseBlock``; here the block's INPUT lives in the
    first 64 channels of its own buffer, because the conv5 of the block before wrote it there
    (``conv5 * scale + x`` in the conv epilogue, 192-channel row stride on both sides).  Per dense block the forward
    is five conv launches (before: a channel copy, five convs, and every third block an ``out * 0.2 + x`` pass that
    stays -- it has two addends).  In the backward the block's output gradient ``dy`` is never scaled or copied:
    conv5's data gradient takes ``scale`` and adds ``dy`` onto the first 64 channels (``srx_conv2d_bwd_data_ex``), its
    weight gradient takes ``scale`` in the slab reduction (``srx_conv2d_bwd_weight_multi_scaled``), and conv1's data
    gradient writes the block's input gradient as a dense tensor, adding what conv2..5 left in the shared gradient
    buffer.  Per RRDB one elementwise pass is left in each direction (before: four and ten).

    With bf16 products the scale meets the rounding in the other order than in autograd's graph: conv5's data and weight
    gradient multiply bf16(dy) and apply ``scale`` to the fp32 result, where the chain of separate nodes rounds
    ``scale * dy`` -- two evaluation orders of the same product, both within bf16 rounding of the exact gradient and
    closer to each other than either is to it (``tests/test_esrgan_gpu.py::test_rrdb_modules_alone_equal_the_trunk_node``).
    """

    @staticmethod
    def forward(ctx, x: Tensor, rdb_scales, rrdb_scale: float, states, masters, pack, *wb):
        ctx.set_materialize_grads(False)
        x = _chk(x, 'rrdb_trunk.input')
        n, h, w, c0 = x.shape
        nb = len(states)
        g = states[0][0].cout
        total = c0 + 4 * g
        m = n * h * w
        s = _stream()
        need_bwd = any(ctx.needs_input_grad)
        # without a backward pass four rotating buffers are enough (an RRDB reads its first block's input at its end)
        pool = [torch.empty((n, h, w, total), dtype=torch.float32, device=x.device) for _ in range(nb + 1 if need_bwd else 4)]
        bufs = [pool[i % len(pool)] for i in range(nb + 1)]
        call('srx_copy_channels', _p(x), c0, 0, _p(bufs[0]), total, 0, c0, m, 0, s)
        descs = []
        y = None
        # bf16 products: a whole dense block is ONE launch (srx_rdb_fwd: the five convs on 8x8 pixel tiles with the
        # intermediates resident in LDS); exact fp32 keeps one launch per conv
        fused = pack is not None and all(rdb_fused_ok(states[i], wb[10 * i:10 * i + 10], c0) for i in range(nb))
        if fused:
            pack.ensure(states, masters, need_bwd)
        for i in range(nb):
            buf, nxt = bufs[i], bufs[i + 1]
            row = []
            for k in range(5):
                st = states[i][k]
                cin = c0 + k * g
                d = Conv2dDesc(n, h, w, cin, total, st.cout, total, st.k, st.k, st.stride, st.pad, 0, st.act, st.slope, 0,
                               st.precision)
                row.append(d)
                st.fused_only = fused  # fused: forward and data gradients read RDBPack's bf16 streams, nothing reads wpk_*
                if fused:
                    continue
                st.pack(masters[i][k], d)
                bias = wb[10 * i + 2 * k + 1]
                bp = None if bias is None else _p(_chk(bias.detach(), 'rrdb_trunk.bias'))
                if k == 4:  # the next block's input = conv5 * scale + x, x = the first 64 channels of this buffer (:86)
                    _conv_fwd(d, _p(buf), _p(st.wpk_fwd), bp, _p(nxt), x, s, residual=(_p(buf), float(rdb_scales[i])))
                else:
                    _conv_fwd(d, _p(buf), _p(st.wpk_fwd), bp, buf.data_ptr() + 4 * cin, x, s)
            if fused:
                biases = (C.c_void_p * 5)(*[_p(_chk(wb[10 * i + 2 * k + 1].detach(), 'rrdb_trunk.bias')) for k in range(5)])
                if i % 3 == 2:  # end of an RRDB: its `out * 0.2 + x` (:128) is the second addend of this block's last epilogue
                    out, out_ld = (nxt, total) if i < nb - 1 else (torch.empty_like(x), c0)
                    call('srx_rdb_fwd', n, h, w, _p(buf), total, pack.block_ptr(i), biases, float(rdb_scales[i]),
                         float(states[i][0].slope), float(rrdb_scale), _p(bufs[i - 2]), total, _p(out), out_ld, s)
                    if i == nb - 1:
                        y = out
                else:
                    call('srx_rdb_fwd', n, h, w, _p(buf), total, pack.block_ptr(i), biases, float(rdb_scales[i]),
                         float(states[i][0].slope), 1.0, None, 0, _p(nxt), total, s)
            descs.append(row)
            if i % 3 == 2 and not fused:  # end of an RRDB: out * 0.2 + x, x = the input of its first dense block (:128)
                first = bufs[i - 2]
                if i == nb - 1:
                    y = torch.empty_like(x)
                    call('srx_axpby_channels', _p(nxt), total, 0, _p(first), total, 0, _p(y), c0, 0, c0, m, float(rrdb_scale),
                         1.0, s)
                else:
                    call('srx_axpby_channels', _p(nxt), total, 0, _p(first), total, 0, _p(nxt), total, 0, c0, m,
                         float(rrdb_scale), 1.0, s)
        ctx.states, ctx.descs = states, descs
        ctx.pack = pack if fused else None
        ctx.scales = ([float(v) for v in rdb_scales], float(rrdb_scale))
        ctx.dims = (n, h, w, c0, g, total, m, nb)
        ctx.params = wb
        if need_bwd:
            ctx.save_for_backward(*bufs[:nb])
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        bufs = ctx.saved_tensors
        grad = _chk(dy, 'rrdb_trunk.grad')
        n, h, w, c0, g, total, m, nb = ctx.dims
        rdb_scales, rrdb_scale = ctx.scales
        s = _stream()
        dev = grad.device
        grads = [None] * (10 * nb)
        queue = wgrad_queue[0]
        rrdb_grad = None
        for i in range(nb - 1, -1, -1):
            j = i % 3
            buf = bufs[i]
            gbuf = torch.empty((n, h, w, total), dtype=torch.float32, device=dev)
            # `grad` is the gradient of the value this block produced, up to the factor `eff`: the last block of an RRDB
            # receives the RRDB's output gradient, of which it sees rrdb_scale (out * 0.2 + x, :128)
            if j == 2:
                rrdb_grad, eff = grad, rrdb_scale
            else:
                eff = 1.0
            # the `+ x` of :86 hands eff * grad to the block's input; the first block's input is also the RRDB's x
            skip, skip_scale = grad, eff
            if j == 0 and ctx.pack is None:
                skip = torch.empty_like(grad)
                call('srx_axpby', _p(grad), _p(rrdb_grad), _p(skip), grad.numel(), eff, 1.0, s)
                skip_scale = 1.0
            dx = torch.empty((n, h, w, c0), dtype=torch.float32, device=dev)
            if ctx.pack is not None:
                # bf16 products: the whole data-gradient chain of the block in one launch (srx_rdb_bwd): g5 = eff * scale * dy,
                # the masked slice gradients g4..g1 (what the weight gradients below read) into gbuf, dx = the x share + skip
                # (+ the RRDB's own skip gradient where this block is the first of its RRDB)
                extra = rrdb_grad if j == 0 else None
                call('srx_rdb_bwd', n, h, w, _p(grad), c0, float(eff * rdb_scales[i]), _p(buf), total, ctx.pack.bwd_ptr(i),
                     float(ctx.states[i][0].slope), _p(gbuf), total, _p(skip), c0, float(skip_scale), _p(extra), c0, _p(dx), c0, s)
            keep = (buf, gbuf, grad)
            # conv1 + conv2 and conv3 + conv4 read the same buffer and their output gradients are adjacent slices of gbuf:
            # queued as two 64-column weight-gradient problems instead of four 32-column ones (half a tile of padding each)
            wsinks = [_sink(ctx.params[10 * i + 2 * k]) for k in range(4)]
            bsinks = [_sink(ctx.params[10 * i + 2 * k + 1]) for k in range(4)]
            paired = (queue is not None and all(v is not None for v in wsinks) and all(v is not None for v in bsinks)
                      and all(ctx.needs_input_grad[6 + 10 * i + kk] for kk in range(8)))
            if paired:
                for lo in (0, 2):
                    st = ctx.states[i][lo + 1]
                    dp = Conv2dDesc(n, h, w, c0 + (lo + 1) * g, total, 2 * g, total, st.k, st.k, st.stride, st.pad, 0, st.act,
                                    st.slope, 0, st.precision)
                    queue.add_pair(dp, c0 + lo * g, _p(buf), gbuf.data_ptr() + 4 * (c0 + lo * g),
                                   (_p(wsinks[lo]), _p(wsinks[lo + 1])), (_p(bsinks[lo]), _p(bsinks[lo + 1])), keep)
            for k in (4, 3, 2, 1, 0):
                st, d = ctx.states[i][k], ctx.descs[i][k]
                cin = c0 + k * g
                if k == 4:  # conv5's output gradient is the block's: a dense 64-channel tensor (the forward wrote 192-strided)
                    d = Conv2dDesc(n, h, w, cin, total, st.cout, st.cout, st.k, st.k, st.stride, st.pad, 0, st.act, st.slope, 0,
                                   st.precision)
                    gk, wscale = grad.data_ptr(), eff * rdb_scales[i]
                else:  # complete and masked: the data gradient of conv k+1 finished this slice of the shared buffer
                    gk, wscale = gbuf.data_ptr() + 4 * cin, 1.0
                # (pairs were queued above: the queue runs after the whole backward pass, when every slice of gbuf is complete.
                # With a scale the bias gradient rides in the weight-gradient kernel, or the launcher refuses)
                if not (paired and k < 4):
                    grads[10 * i + 2 * k], grads[10 * i + 2 * k + 1] = _conv_param_grads(
                        st, d, _p(buf), gk, m, d.Cout_s, ctx.params[10 * i + 2 * k] if ctx.needs_input_grad[6 + 10 * i + 2 * k] else None,
                        ctx.params[10 * i + 2 * k + 1] if ctx.needs_input_grad[7 + 10 * i + 2 * k] else None, keep, grad, s, scale=wscale)
                if ctx.pack is not None:
                    continue  # (the block's five data gradients are one launch, below)
                e = _lib.DgradEpilogue()
                if k > 0:  # LeakyReLU backward of conv k on the slice this call completes (esrgan/residual.py:81-84)
                    e.act_out, e.act_slope, e.c_lo, e.c_hi = _p(buf), ctx.states[i][k - 1].slope, cin - g, cin
                if k == 4:    # overwrites all 192 channels; `+ x`: the block's output gradient lands on the first 64
                    e.out_scale = eff * rdb_scales[i]
                    e.addend, e.addend_ld, e.addend_channels, e.addend_scale = _p(skip), c0, c0, skip_scale
                    out, dd = gbuf, d
                elif k > 0:
                    e.accumulate = 1
                    out, dd = gbuf, d
                else:         # the block's input gradient, dense: this conv's share + the first 64 channels of the buffer
                    e.addend, e.addend_ld, e.addend_channels = _p(gbuf), total, c0
                    dd = Conv2dDesc(n, h, w, c0, c0, st.cout, total, st.k, st.k, st.stride, st.pad, 0, st.act, st.slope, 0,
                                    st.precision)
                    out = dx
                ddref = C.byref(dd)
                nws = _lib.lib().srx_conv2d_bwd_data_ws_floats(ddref)
                ws = _ws(nws, grad) if nws else None
                call('srx_conv2d_bwd_data_ex', ddref, gk, _p(st.wpk_bwd), _p(out), C.byref(e), _p(ws), nws, s)
            grad = dx
        return (grad, None, None, None, None, None, *grads)


def rrdb_trunk(x: Tensor, rrdbs) -> Tensor:
    """``rrdbs``: the generator's ``ResidualInResidualDenseBlock`` modules, in order (``nn.Sequential(*blocks)(x)``)."""
    from .layers import _w
    if not rrdbs:
        return x
    states, masters, wb, scales = [], [], [], []
    for rr in rrdbs:
        for rdb in (rr.RDB1, rr.RDB2, rr.RDB3):
            convs = (rdb.conv1[0], rdb.conv2[0], rdb.conv3[0], rdb.conv4[0], rdb.conv5)
            states.append([c._st for c in convs])
            masters.append([c.weight for c in convs])
            scales.append(rdb.scale_ratio)
            for c in convs:
                wb += [_w(c.weight), _w(c.bias)]
    pack = rrdbs[0].__dict__.get('_rdb_pack')
    if pack is None:
        pack = rrdbs[0].__dict__.setdefault('_rdb_pack', RDBPack())
    return _RRDBTrunk.apply(x, scales, 0.2, states, masters, pack, *wb)


class _Upsample2x(Function):
    @staticmethod
    def forward(ctx, x: Tensor):
        ctx.set_materialize_grads(False)
        x = _chk(x, 'upsample.input')
        n, h, w, c = x.shape
        y = torch.empty((n, 2 * h, 2 * w, c), dtype=torch.float32, device=x.device)
        call('srx_upsample_nearest2x_fwd', _p(x), _p(y), n, h, w, c, _stream())
        ctx.shape = (n, h, w, c)
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        dy = _chk(dy, 'upsample.grad')
        n, h, w, c = ctx.shape
        dx = torch.empty((n, h, w, c), dtype=torch.float32, device=dy.device)
        call('srx_upsample_nearest2x_bwd', _p(dy), _p(dx), n, h, w, c, _stream())
        return dx


def upsample_nearest2x(x: Tensor) -> Tensor:
    """F.interpolate(x, scale_factor=2, mode='nearest') (esrgan/generator.py:73,76) on NHWC."""
    return _Upsample2x.apply(x)


class _UpsampleBilinear2x(Function):
    @staticmethod
    def forward(ctx, x: Tensor):
        ctx.set_materialize_grads(False)
        x = _chk(x, 'upsample_bilinear2x.input')
        n, h, w, c = x.shape
        if c % 4:
            raise RuntimeError(f'upsample_bilinear2x: the channel stride must be a multiple of 4, got {c}')
        y = torch.empty((n, 2 * h, 2 * w, c), dtype=torch.float32, device=x.device)
        call('srx_upsample_bilinear2x_fwd', _p(x), _p(y), n, h, w, c, c, _stream())
        ctx.shape = (n, h, w, c)
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        dy = _chk(dy, 'upsample_bilinear2x.grad')
        n, h, w, c = ctx.shape
        dx = torch.empty((n, h, w, c), dtype=torch.float32, device=dy.device)
        call('srx_upsample_bilinear2x_bwd', _p(dy), _p(dx), n, h, w, c, c, _stream())
        return dx


def upsample_bilinear2x(x: Tensor) -> Tensor:
    """F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False) on NHWC (the U-Net discriminator's decoder)."""
    return _UpsampleBilinear2x.apply(x)


# --------------------------------------------------------------------------- spectral normalisation
class SNConvState(ConvState):
    """``ConvState`` of a conv that multiplies a spectrally normalised copy of its weight.  The copy lives in ONE persistent
    buffer per layer (a captured step holds its address) that every ``spectral_norm`` call rewrites by raw pointer, so neither
    its address nor its ``_version`` says that the packed copies are stale: ``sn_calls``, bumped by each call, is part of the
    key.  Such layers stay out of ``PackTable``, whose launch after Adam repacks from the Parameters."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.sn_calls = 0

    def pack_key(self, weight: Tensor):
        return super().pack_key(weight) + (self.sn_calls,)


class _SpectralNorm(Function):
    @staticmethod
    def forward(ctx, w: Tensor, u: Tensor, v: Tensor, out: Tensor, train: bool, master):
        ctx.set_materialize_grads(False)
        w, out = _chk(w, 'spectral_norm.weight'), _chk(out, 'spectral_norm.out')
        u, v = _chk(u, 'spectral_norm.u'), _chk(v, 'spectral_norm.v')
        rows = w.shape[0]
        cols = w.numel() // rows
        if u.numel() != rows or v.numel() != cols or out.numel() != w.numel():
            raise RuntimeError(f'spectral_norm: a {rows} x {cols} weight needs u[{rows}], v[{cols}] and an output of its size, got '
                               f'{u.numel()}, {v.numel()}, {out.numel()}')
        sigma = torch.empty(1, dtype=torch.float32, device=w.device)
        keep = torch.empty(round4(rows) + cols, dtype=torch.float32, device=w.device) if ctx.needs_input_grad[0] else None
        nws = _lib.lib().srx_spectral_norm_ws_floats(rows, cols)
        call('srx_spectral_norm_fwd', _p(w), _p(u), _p(v), _p(out), _p(sigma), _p(keep), rows, cols, int(bool(train)),
             _p(_ws(nws, w)), nws, _stream())
        ctx.w, ctx.keep, ctx.sigma, ctx.master, ctx.dims = w, keep, sigma, master[0], (rows, cols)
        return out.detach()  # (a fresh alias: the persistent buffer itself never carries a grad_fn)

    @staticmethod
    def backward(ctx, g: Tensor):
        if g is None or ctx.keep is None:
            return None, None, None, None, None, None
        g = _chk(g, 'spectral_norm.grad')
        rows, cols = ctx.dims
        sink = _sink(ctx.master)
        dw = sink if sink is not None else torch.empty_like(ctx.w)
        nws = _lib.lib().srx_spectral_norm_ws_floats(rows, cols)
        call('srx_spectral_norm_bwd', _p(g), _p(ctx.w), _p(ctx.keep), ctx.keep.data_ptr() + 4 * round4(rows), _p(ctx.sigma), _p(dw),
             0 if sink is None else 1, rows, cols, _p(_ws(nws, g)), nws, _stream())
        return (dw if sink is None else None), None, None, None, None, None


def spectral_norm(w: Tensor, u: Tensor, v: Tensor, out: Tensor, train: bool, master: Optional[Tensor] = None) -> Tensor:
    """``torch.nn.utils.spectral_norm``'s weight (one power iteration, eps 1e-12) written into the persistent buffer ``out``.

    ``train``: ``u`` and ``v`` take one power iteration in place first (no gradient flows through them); otherwise sigma comes
    from the stored vectors.  The backward is the closed form ``dW = (G - <G, W_sn> u v^T) / sigma`` with the vectors of THIS
    call; it accumulates into ``master.grad`` when the trainers' flat gradient buffers are on (``direct_grads``).  The returned
    tensor aliases ``out``: a later call overwrites it, so a conv that used it must have run (and packed it) before -- and its
    backward too: ``_Conv2d.backward`` refuses an ``SNConvState`` layer whose call counter has moved since its forward."""
    # (the Parameter travels in a tuple: as a tensor argument it would make the output require a gradient under no_weight_grad)
    return _SpectralNorm.apply(w, u, v, out, train, (w if master is None else master,))
