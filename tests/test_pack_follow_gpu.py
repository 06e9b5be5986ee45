"""Every packed weight layout follows its master weight: one layer per pack kind (functional.WeightPack), at the smallest
shape that takes that kind's kernels -- asserted by the slot being populated, so a test cannot quietly run another kernel.

The layer runs three times: as built (``y1``), after ``w.mul_(2)`` under ``no_grad`` (an in-place update: ``_version``), and
after ``w.data.mul_(2)`` (no version bump, as a raw-pointer optimiser step leaves none) plus ``bump_pack_epoch()``.  A stale
pack shows as last call's output.  Scaling a weight by a power of two commutes exactly with every product, sum, rounding to
bf16 and ReLU / LeakyReLU involved, so ``y2 == 2 * y1`` and ``y3 == 4 * y1`` bit for bit: no tolerance.  Inputs lie in
[0.5, 1), weights within +-2e-2: nothing nears overflow or the denormal range at x4.  A bias is scaled with its weight.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def uniform(shape, lo, hi, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * (hi - lo) + lo).to(dev)


def small_weights(module, seed=1):
    for i, p in enumerate(module.parameters()):
        p.data.copy_(uniform(p.shape, -2e-2, 2e-2, seed + i, p.device))


def follow(run, params, populated, frozen=False):
    """``run() -> tuple of tensors``; each must double with every doubling of ``params``."""
    from torchsr_amd import functional as F
    first = run()
    populated()
    assert all(bool(t.abs().max() > 0) and bool(torch.isfinite(t).all()) for t in first)
    with torch.no_grad():
        for p in params:
            p.mul_(2)
    for a, b in zip(run(), first):
        assert torch.equal(a.float(), 2 * b.float())
    versions = [p._version for p in params]
    if frozen:  # (a frozen parameter's key has no epochs -- ConvState.pack_key: such weights change by versioned updates only)
        for p in params:
            p.mul_(2)
    else:
        for p in params:
            p.data.mul_(2)
        assert [p._version for p in params] == versions
        F.bump_pack_epoch()
    for a, b in zip(run(), first):
        assert torch.equal(a.float(), 4 * b.float())


def with_input_grad(conv, x, g):
    def run():
        y = conv(x)
        return y.detach(), torch.autograd.grad(y, x, g)[0]
    return run


def test_direct_pack_follows_the_weight(dev):
    from torchsr_amd.layers import Conv2d
    conv = Conv2d(8, 8, 3, padding=1, bias=False).to(dev)
    small_weights(conv)
    x = uniform((1, 8, 8, 8), 0.5, 1.0, 2, dev).requires_grad_(True)
    st = conv._st

    def populated():
        assert st.direct.fwd is not None and st.direct.bwd is not None and st.wino.fwd is None
        assert st.direct.key == st.pack_key(conv.weight)

    follow(with_input_grad(conv, x, uniform((1, 8, 8, 8), 0.5, 1.0, 3, dev)), [conv.weight], populated)


def test_winograd_pack_follows_the_weight(dev):
    """256 -> 256 at 32 x 24 x 24: the size tests/test_wino_gpu.py shows on Winograd in training (``srx_wino_applicable``
    weighs the layer against the chip: a smaller one goes back to the direct kernel)."""
    import ctypes as C
    from torchsr_amd import _lib
    from torchsr_amd.layers import Conv2d
    conv = Conv2d(256, 256, 3, padding=1, bias=False).to(dev)
    small_weights(conv)
    x = uniform((32, 24, 24, 256), 0.5, 1.0, 2, dev).requires_grad_(True)
    st = conv._st
    assert _lib.lib().srx_wino_applicable(C.byref(st.desc(32, 24, 24))) == 1

    def populated():
        assert st.wino.fwd is not None and st.wino.bwd is not None and st.direct.fwd is None
        assert st.wino.key == st.pack_key(conv.weight)

    follow(with_input_grad(conv, x, uniform((32, 24, 24, 256), 0.5, 1.0, 3, dev)), [conv.weight], populated)


def test_bf16_storage_pack_follows_the_weight(dev):
    """The 3 -> 64 layer every bf16-storage stack starts with, then the 64 -> 64 layer whose bf16 copy is under test.  The
    stack is frozen by contract, so its third run follows a second versioned update: an epoch bump is not in a frozen key."""
    from torchsr_amd import functional as F
    from torchsr_amd.layers import ACT_RELU, Conv2d, set_conv_precision
    stack = torch.nn.Sequential(Conv2d(3, 64, 3, padding=1, bias=False, act=ACT_RELU),
                                Conv2d(64, 64, 3, padding=1, bias=False, act=ACT_RELU)).to(dev).requires_grad_(False)
    small_weights(stack)
    set_conv_precision(stack, 'bf16')
    layers = [('conv', stack[0]), ('conv', stack[1])]
    x = F.to_nhwc(uniform((1, 3, 8, 8), 0.5, 1.0, 2, dev), 4)
    assert F._bf16_stack_ok(layers, tuple(x.shape))
    st = stack[1]._st

    def run():
        with torch.no_grad():
            return (F.frozen_conv_stack(x, None, layers)[0],)

    def populated():
        assert st.bf16s.fwd is not None and st.direct.fwd is None and st.wino.fwd is None
        assert st.bf16s.key == st.pack_key(stack[1].weight)

    follow(run, [stack[1].weight], populated, frozen=True)


def test_c64_16bit_pack_follows_the_weight(dev):
    from torchsr_amd import functional as F
    from torchsr_amd.layers import Conv2d
    conv = Conv2d(64, 64, 3, padding=1).to(dev).eval()
    small_weights(conv)
    conv._st.precision = 2
    folded = F.FoldedConv(conv)
    x = F.to_bf16(uniform((1, 8, 32, 64), 0.5, 1.0, 2, dev))

    def run():
        with torch.no_grad():
            return (folded(x),)

    def populated():
        assert folded.pack16.fwd is not None and folded.pack16.key == (folded._key, torch.bfloat16)
        assert folded.st.direct.fwd is None and folded.st.wino.fwd is None

    follow(run, [conv.weight, conv.bias], populated)


def test_thin9_pack_follows_the_weight(dev):
    from torchsr_amd import functional as F
    from torchsr_amd.layers import Conv2d
    conv = Conv2d(64, 3, 9, padding=4).to(dev).eval()
    small_weights(conv)
    conv._st.precision = 2
    x = F.to_bf16(uniform((1, 16, 32, 64), 0.5, 1.0, 2, dev))

    def run():
        with torch.no_grad():
            return (F.conv2d_bf16in(conv, x),)

    def populated():
        assert conv._st.thin9.fwd is not None and conv._st.direct.fwd is None

    follow(run, [conv.weight, conv.bias], populated)


def test_dense_block_streams_follow_the_weights(dev):
    """One RRDB on the fused one-launch dense blocks (bf16 products).  Its skip connections make the output no homogeneous
    function of the weights, so doubling them predicts nothing; instead every run must equal, bit for bit, a twin built from
    scratch on the same weights (fresh states, fresh RDBPack: nothing of it can be stale), and differ from the run before."""
    from torchsr_amd import functional as F
    from torchsr_amd.esrgan.residual import ResidualInResidualDenseBlock
    from torchsr_amd.layers import Conv2d, set_conv_precision

    def build(state=None):
        m = ResidualInResidualDenseBlock().to(dev)
        if state is None:
            small_weights(m)
        else:
            m.load_state_dict(state)
        set_conv_precision(m, 'bf16')
        return m

    def run(m):
        with torch.no_grad():
            y = F.rrdb_trunk(x, [m])
        pack = m.__dict__['_rdb_pack'].pack
        assert pack.fwd is not None and all(c._st.fused_only and c._st.direct.fwd is None for c in m.modules() if isinstance(c, Conv2d))
        return y

    rrdb = build()
    x = uniform((1, 16, 16, 64), 0.5, 1.0, 2, dev)
    params = list(rrdb.parameters())
    y1 = run(rrdb)
    assert bool(torch.isfinite(y1).all())
    with torch.no_grad():
        for p in params:
            p.mul_(2)
    y2 = run(rrdb)
    assert not torch.equal(y2, y1) and torch.equal(y2, run(build(rrdb.state_dict())))
    for p in params:
        p.data.mul_(2)
    F.bump_pack_epoch()
    y3 = run(rrdb)
    assert not torch.equal(y3, y2) and torch.equal(y3, run(build(rrdb.state_dict())))
