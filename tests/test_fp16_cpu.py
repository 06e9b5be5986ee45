"""fp16 inference without a GPU: the fp16 entry points refuse bad arguments before any launch, and the host refuses
precision 3 (fp16) wherever it cannot run -- training, autograd, a generator without the 16-bit-native chain."""
import ctypes as C

import pytest
import torch


def test_abi_refuses_bad_fp16_arguments_without_a_gpu():
    """The fp16 mirrors of the bf16 chain validate like their namesakes: null pointers, element counts that are not whole
    quads, channel counts that are not multiples of 64, in-place and stride errors -- with fake pointers, so a missed check
    would fault here rather than on a device."""
    from torchsr_amd import _lib
    if torch.cuda.is_available():
        pytest.skip('fake pointers: argument validation is exercised where a missed check cannot reach a device')
    lib = _lib.lib()
    fake = 0x10000  # never dereferenced: the calls below must fail in argument validation

    def refused(rc, what):
        buf = C.create_string_buffer(256)
        lib.srx_last_error(buf, 256)
        msg = buf.value.decode()
        return rc != 0 and what in msg and 'f16' in msg

    # conversions
    assert refused(lib.srx_f32_to_f16(None, fake, 8, None), 'multiple of 4')
    assert refused(lib.srx_f32_to_f16(fake, None, 8, None), 'multiple of 4')
    assert refused(lib.srx_f32_to_f16(fake, fake, 6, None), 'multiple of 4')
    assert refused(lib.srx_f32_to_f16(fake, fake, 0, None), 'multiple of 4')
    assert refused(lib.srx_f16_to_f32(fake, fake, 10, None), 'multiple of 4')
    assert refused(lib.srx_f16_to_f32(None, fake, 8, None), 'multiple of 4')
    # 3x3 / 64-channel conv
    assert lib.srx_conv3x3_c64_f16_packed_bytes(96) == 0
    assert lib.srx_conv3x3_c64_f16_packed_bytes(128) == lib.srx_conv3x3_c64_bf16_packed_bytes(128) > 0
    assert refused(lib.srx_conv3x3_c64_f16_pack(None, None, None, 64, 0, fake, None), 'multiple of 64')
    assert refused(lib.srx_conv3x3_c64_f16_pack(fake, None, None, 96, 0, fake, None), 'multiple of 64')
    assert refused(lib.srx_conv3x3_c64_f16_pack(fake, None, None, 128, 2, fake, None), 'PixelShuffle')
    fwd = lib.srx_conv3x3_c64_f16_fwd
    assert refused(fwd(1, 8, 8, 64, 0, None, fake, 1.0, None, fake + 4096, 64, None), 'null pointer')
    assert refused(fwd(1, 8, 8, 64, 0, fake, None, 1.0, None, fake + 4096, 64, None), 'null pointer')
    assert refused(fwd(1, 8, 8, 64, 0, fake, fake, 1.0, None, None, 64, None), 'null pointer')
    assert refused(fwd(1, 8, 8, 96, 0, fake, fake, 1.0, None, fake + 4096, 96, None), 'multiple of 64')
    assert refused(fwd(1, 8, 8, 64, 0, fake, fake, 1.0, None, fake + 4096, 60, None), 'channel stride')
    assert refused(fwd(1, 8, 8, 64, 0, fake, fake, 1.0, None, fake, 64, None), 'in place')
    assert refused(fwd(1, 8, 8, 256, 2, fake, fake, 1.0, fake + 8192, fake + 4096, 64, None), 'addend')
    # 9x9 output conv
    assert lib.srx_conv9x9_c64_thin_f16_packed_bytes() == lib.srx_conv9x9_c64_thin_bf16_packed_bytes()
    assert refused(lib.srx_conv9x9_c64_thin_f16_pack(fake, None, 4, fake, None), 'output channels')
    assert refused(lib.srx_conv9x9_c64_thin_f16_pack(None, None, 3, fake, None), 'output channels')
    assert refused(lib.srx_conv9x9_c64_thin_f16_fwd(1, 8, 8, None, fake, fake, None), 'bad argument')
    assert refused(lib.srx_conv9x9_c64_thin_f16_fwd(1, 0, 8, fake, fake, fake, None), 'bad argument')


def test_fp16_precision_refused_off_inference_without_a_gpu():
    """Precision 3 exists for inference only: a layer asked for it with autograd on, or in training mode, raises before
    it builds a descriptor; ``upscale(..., 'fp16')`` refuses a generator without the fp16 chain (ESRGAN) with ValueError
    and leaves its precisions alone; training has no 'fp16' setting."""
    from torchsr_amd import functional as F
    from torchsr_amd.esrgan.generator import Generator as ESRGen
    from torchsr_amd.layers import Conv2d, set_conv_precision
    from torchsr_amd.test import upscale
    st = F.ConvState(64, 64, 3, 1, 1)
    st.precision = F.PRECISION_F16
    with pytest.raises(RuntimeError, match='inference-only'):
        st.desc(1, 8, 8)
    from torchsr_amd import _lib
    with torch.no_grad():
        d = st.desc(1, 8, 8)
        d1 = F.ConvState(3, 64, 9, 1, 4)
        d1.precision = F.PRECISION_F16
        d1 = d1.desc(1, 8, 8)
    lib = _lib.lib()
    # the library takes 3 for the forward of a <= 4-channel input layer only, and refuses its backward
    assert lib.srx_conv2d_packed_fwd_floats(C.byref(d)) == 0 and 'precision' in _lib.last_error()
    assert lib.srx_conv2d_packed_fwd_floats(C.byref(d1)) > 0
    if not torch.cuda.is_available():  # (fake pointers)
        assert lib.srx_conv2d_bwd_data(C.byref(d1), 0x10000, 0x10000, 0x20000, 0, None, 0, None) != 0
        assert 'forward-only' in _lib.last_error()
    conv = Conv2d(64, 64, 3, 1, 1)
    conv._st.precision = F.PRECISION_F16
    with pytest.raises(RuntimeError, match='inference-only'):
        conv(torch.zeros(1, 8, 8, 64))
    esr = ESRGen(num_rrdb_blocks=1)
    before = [m._st.precision for m in esr.modules() if isinstance(m, Conv2d)]
    with pytest.raises(ValueError, match='fp16'):
        upscale(esr, torch.zeros(1, 3, 8, 8), precision='fp16')
    assert [m._st.precision for m in esr.modules() if isinstance(m, Conv2d)] == before
    with pytest.raises(ValueError, match='fp16'):
        upscale(esr, torch.zeros(1, 3, 8, 8), precision='half')
    with pytest.raises(KeyError):
        set_conv_precision(esr, 'fp16')


def test_cli_offers_fp16_without_a_gpu():
    from torchsr_amd.torchsr import parse_args
    assert parse_args(['test', 'x.png', '--precision', 'fp16']).precision == 'fp16'
