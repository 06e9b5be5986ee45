"""The gradient guard (srx_grad_guard / srx_adam_step_guarded, optim.FlatAdam(max_grad_norm, skip_nonfinite), the
``--clip-grad-norm`` / ``--skip-nonfinite-steps`` flags) as far as it goes without a GPU: argument validation, the
workspace size query and the command line."""
import ctypes as C

import pytest
import torch

# lengths tests/test_grad_guard_gpu.py runs the guard at
SIZES = (1, 3, 4, 5, 1023, 1027, 4097, 4096 * 1024 + 1024 + 1, 4096 * 1024 + 1024 + 2, 4096 * 1024 + 1024 + 3)


def test_abi_refuses_bad_guard_arguments_without_a_gpu():
    """Null pointers, n <= 0, a zero / non-finite grad_scale, a NaN max_norm, a short workspace and misaligned buffers are
    refused before any launch -- with fake pointers, so a missed check would fault here rather than on a device."""
    from torchsr_amd import _lib
    if torch.cuda.is_available():
        pytest.skip('fake pointers: argument validation is exercised where a missed check cannot reach a device')
    lib = _lib.lib()
    fake = 0x10000  # never dereferenced: the calls below must fail in argument validation
    nan, inf = float('nan'), float('inf')

    def refused(rc, what):
        buf = C.create_string_buffer(256)
        lib.srx_last_error(buf, 256)
        msg = buf.value.decode()
        return rc != 0 and what in msg

    n = 4097
    ws = lib.srx_grad_guard_ws_bytes(n)
    guard = lib.srx_grad_guard
    assert refused(guard(None, n, 1.0, 0.0, 1, fake, ws, fake, None), 'grad_guard: bad argument')
    assert refused(guard(fake, n, 1.0, 0.0, 1, None, ws, fake, None), 'grad_guard: bad argument')
    assert refused(guard(fake, n, 1.0, 0.0, 1, fake, ws, None, None), 'grad_guard: bad argument')
    assert refused(guard(fake, 0, 1.0, 0.0, 1, fake, ws, fake, None), 'grad_guard: bad argument')
    assert refused(guard(fake, -4, 1.0, 0.0, 1, fake, ws, fake, None), 'grad_guard: bad argument')
    for scale in (0.0, nan, inf, -inf):
        assert refused(guard(fake, n, scale, 0.0, 1, fake, ws, fake, None), 'grad_scale')
    assert refused(guard(fake, n, 1.0, nan, 1, fake, ws, fake, None), 'max_norm')
    assert refused(guard(fake, n, 1.0, 1.0, 1, fake, ws - 1, fake, None), 'workspace too small')
    assert refused(guard(fake, n, 1.0, 1.0, 1, fake, 0, fake, None), 'workspace too small')
    assert refused(guard(fake + 4, n, 1.0, 1.0, 1, fake, ws, fake, None), 'aligned')
    assert refused(guard(fake, n, 1.0, 1.0, 1, fake + 4, ws, fake, None), 'aligned')
    assert refused(guard(fake, n, 1.0, 1.0, 1, fake, ws, fake + 4, None), 'aligned')

    adam = lib.srx_adam_step_guarded
    good = [fake, fake, fake, fake, n, fake, 0.9, 0.999, 1e-8, 1.0, fake, fake, None]
    for at in (0, 1, 2, 3, 5, 10, 11):  # p, g, m, v, lr, step, state
        args = list(good)
        args[at] = None
        assert refused(adam(*args), 'adam_step_guarded: bad argument'), at
    args = list(good)
    args[4] = 0
    assert refused(adam(*args), 'adam_step_guarded: bad argument')
    for at in (0, 1, 2, 3, 11):
        args = list(good)
        args[at] = fake + 4
        assert refused(adam(*args), 'aligned'), at


def test_guard_workspace_size_is_positive_and_monotone():
    from torchsr_amd import _lib
    lib = _lib.lib()
    sizes = [lib.srx_grad_guard_ws_bytes(n) for n in sorted(SIZES)]
    assert all(s > 0 and s % 8 == 0 for s in sizes), sizes
    assert sizes == sorted(sizes), sizes
    assert lib.srx_grad_guard_ws_bytes(0) == 0 and lib.srx_grad_guard_ws_bytes(-1) == 0


def test_cli_flags_of_the_gradient_guard():
    from torchsr_amd.torchsr import parse_args
    args = parse_args(['train', '--clip-grad-norm', '0.5', '--skip-nonfinite-steps'])
    assert args.clip_grad_norm == 0.5 and args.skip_nonfinite_steps is True
    args = parse_args(['train'])
    assert args.clip_grad_norm is None and args.skip_nonfinite_steps is False
    for bad in ('0', '-1', 'nan', 'x'):
        with pytest.raises(SystemExit):
            parse_args(['train', '--clip-grad-norm', bad])


def test_flat_adam_refuses_a_non_positive_clip_norm():
    from torchsr_amd import optim
    flat = optim.FlatParams(torch.nn.Linear(3, 2))
    for bad in (0, 0.0, -1.0, float('nan')):
        with pytest.raises(ValueError):
            optim.FlatAdam(flat, max_grad_norm=bad)
    with pytest.raises(ValueError):
        optim.FlatAdam(flat, max_grad_norm=0, skip_nonfinite=True)
