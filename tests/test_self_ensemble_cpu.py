"""Self-ensemble inference without a GPU: the group-element encoding and its inverse rule, the ``self_ensemble`` argument of
``upscale`` and of the CLI, and the refusals of ``srx_dihedral_planes`` before any launch."""
import ctypes as C

import pytest
import torch


def T(x, k):
    """The index map of ``srx_dihedral_planes`` restated with torch: transpose (bit 0) first, then the horizontal (bit 1) and
    the vertical (bit 2) flip."""
    if k & 1:
        x = x.transpose(-1, -2)
    if k & 2:
        x = x.flip(-1)
    if k & 4:
        x = x.flip(-2)
    return x


def test_dihedral_inverse_undoes_every_element():
    from torchsr_amd import functional as F
    x = torch.arange(2 * 3 * 5 * 7).reshape(2, 3, 5, 7)
    for k in range(8):
        inv = F.dihedral_inverse(k)
        assert 0 <= inv <= 7 and F.dihedral_inverse(inv) == k
        assert T(x, k).shape == ((2, 3, 7, 5) if k & 1 else (2, 3, 5, 7))
        assert torch.equal(T(T(x, k), inv), x), k
        if k & 1 and bool(k & 2) != bool(k & 4):  # the two rotations by 90 degrees: not their own inverses
            assert inv != k
            assert T(T(x, k), k).shape == x.shape and not torch.equal(T(T(x, k), k), x), k
        else:
            assert inv == k
    assert sorted(F.dihedral_inverse(k) for k in range(8)) == list(range(8))
    for bad in (-1, 8, 1.0, None):
        with pytest.raises(ValueError):
            F.dihedral_inverse(bad)


def test_cli_self_ensemble_flag():
    from torchsr_amd.torchsr import parse_args
    assert parse_args(['test', 'x.png']).self_ensemble == 0
    assert parse_args(['test', 'x.png', '--self-ensemble']).self_ensemble == 8
    assert parse_args(['test', 'x.png', '--self-ensemble', '4']).self_ensemble == 4
    assert parse_args(['test', 'x.png', '--self-ensemble', '8', '--precision', 'bf16', '--model', 'esrgan']).self_ensemble == 8
    with pytest.raises(SystemExit):
        parse_args(['test', 'x.png', '--self-ensemble', '3'])


def test_upscale_refuses_other_ensemble_sizes_before_the_generator_runs():
    from torchsr_amd.test import upscale

    class Stub(torch.nn.Module):
        calls = 0

        def forward(self, x):
            Stub.calls += 1
            return x

        def eval(self):
            Stub.calls += 1
            return self

    stub = Stub()
    for bad in (3, 1, 2, 16, -8, 8.0, '8', None):
        with pytest.raises(ValueError, match='self_ensemble'):
            upscale(stub, torch.zeros(1, 3, 8, 8), self_ensemble=bad)
    assert Stub.calls == 0
    # off is today's path: the stub (no convs, identity) is called once, positionally as the recursive call does
    for off in (0, False):
        Stub.calls = 0
        x = torch.rand(1, 3, 8, 8)
        assert upscale(stub, x, None, 10 ** 6, 4, None, True, off) is x
        assert Stub.calls == 2


def test_dihedral_refuses_autograd_and_bad_arguments_without_a_gpu():
    from torchsr_amd import functional as F
    x = torch.zeros(1, 3, 4, 4, requires_grad=True)
    with pytest.raises(RuntimeError, match='inference-only'):
        F.dihedral(x, 1)
    with torch.no_grad():
        with pytest.raises(ValueError, match='0..7'):
            F.dihedral(x, 8)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            F.dihedral(x, 1)  # a CPU tensor: no fallback


def test_abi_refuses_bad_dihedral_arguments_without_a_gpu():
    """Fake pointers: every call below must fail in argument validation (a missed check would fault here, not on a device)."""
    from torchsr_amd import _lib
    if torch.cuda.is_available():
        pytest.skip('fake pointers: argument validation is exercised where a missed check cannot reach a device')
    lib = _lib.lib()
    src, dst = 0x100000, 0x900000  # 8 MiB apart; never dereferenced
    f = lib.srx_dihedral_planes

    def refused(rc, what):
        buf = C.create_string_buffer(256)
        lib.srx_last_error(buf, 256)
        msg = buf.value.decode()
        return rc != 0 and what in msg and 'dihedral_planes' in msg

    nan, inf = float('nan'), float('inf')
    assert refused(f(src, dst, 3, 8, 8, 8, 1.0, 0.0, None), 'group element')
    assert refused(f(src, dst, 3, 8, 8, -1, 1.0, 0.0, None), 'group element')
    assert refused(f(src, dst, 3, 0, 8, 1, 1.0, 0.0, None), 'positive')
    assert refused(f(src, dst, 3, 8, 0, 1, 1.0, 0.0, None), 'positive')
    assert refused(f(src, dst, 3, 8, -4, 1, 1.0, 0.0, None), 'positive')
    assert refused(f(src, dst, 0, 8, 8, 1, 1.0, 0.0, None), 'positive')
    assert refused(f(src, dst, -2, 8, 8, 1, 1.0, 0.0, None), 'positive')
    assert refused(f(None, dst, 3, 8, 8, 1, 1.0, 0.0, None), 'null pointer')
    assert refused(f(src, None, 3, 8, 8, 1, 1.0, 0.0, None), 'null pointer')
    assert refused(f(src, dst, 3, 8, 8, 1, nan, 0.0, None), 'finite')
    assert refused(f(src, dst, 3, 8, 8, 1, 1.0, nan, None), 'finite')
    assert refused(f(src, dst, 3, 8, 8, 0, inf, 0.0, None), 'finite')
    assert refused(f(src, dst, 3, 8, 8, 0, 1.0, -inf, None), 'finite')
    assert refused(f(src, src, 3, 8, 8, 1, 1.0, 0.0, None), 'overlap')          # in place
    assert refused(f(src, src, 3, 8, 8, 0, 1.0, 0.0, None), 'overlap')          # ... also where it would be harmless
    assert refused(f(src, src + 4, 3, 8, 8, 3, 1.0, 0.0, None), 'overlap')      # dst inside src's range
    assert refused(f(src, src + 3 * 64 * 4 - 4, 3, 8, 8, 5, 1.0, 1.0, None), 'overlap')  # its last element
    assert refused(f(src + 3 * 64 * 4 - 4, src, 3, 8, 8, 5, 1.0, 1.0, None), 'overlap')  # src inside dst's range
    assert refused(f(src, dst, 1 << 20, 1 << 10, 1 << 10, 1, 1.0, 0.0, None), 'overlap')  # 4 TiB each: the ranges meet
    assert refused(f(src, dst, 1 << 40, 1 << 15, 1 << 15, 1, 1.0, 0.0, None), '2^60')
    assert refused(f(src + 2, dst, 3, 8, 8, 1, 1.0, 0.0, None), 'aligned')
