"""Training at x2, the parts that need no GPU: ``train --scale``, the plan / workspace arithmetic and the refusals of
``srx_unshuffle2_conv_bwd_weight`` (nothing is launched: the pointers are made up), the ``trainable`` flag of
``esrgan.Generator`` / ``layers.Unshuffle2Conv2d``, and the scale-mismatch messages."""
import copy
import ctypes as C

import pytest
import torch

import compact_ref
import x2_ref


# ------------------------------------------------------------------ command line
def test_scale_parses_for_esrgan_and_compact_and_defaults_to_4():
    from torchsr_amd.torchsr import parse_args
    for model in ('esrgan', 'compact'):
        assert parse_args(['train', '--model', model]).scale == 4
        assert parse_args(['train', '--model', model, '--scale', '2']).scale == 2
        assert parse_args(['train', '--model', model, '--scale', '4']).scale == 4
    assert parse_args(['train', '--model', 'srgan']).scale == 4


def test_scale_2_is_refused_for_srgan_with_the_reason(capsys):
    from torchsr_amd.torchsr import parse_args
    with pytest.raises(SystemExit):
        parse_args(['train', '--scale', '2', '--model', 'srgan'])
    err = capsys.readouterr().err
    assert '--scale 2 trains with --model esrgan or --model compact; --model srgan' in err
    for bad in ('3', '8', 'x'):
        with pytest.raises(SystemExit):
            parse_args(['train', '--model', 'esrgan', '--scale', bad])
        assert '--scale' in capsys.readouterr().err


def test_compact_init_file_must_have_the_runs_scale(tmp_path, capsys):
    from torchsr_amd.torchsr import parse_args
    paths = {}
    for s in (2, 3, 4):
        paths[s] = str(tmp_path / f'x{s}.pth')
        torch.save({'params_ema': compact_ref.CompactRef(scale_factor=s, num_conv=2).state_dict()}, paths[s])
    assert parse_args(['train', '--model', 'compact', '--scale', '2', '--init-generator', paths[2]]).num_conv == 2
    assert parse_args(['train', '--model', 'compact', '--init-generator', paths[4]]).scale == 4
    with pytest.raises(SystemExit):
        parse_args(['train', '--model', 'compact', '--init-generator', paths[2]])
    assert 'x2 is inference-only unless the run is started with --scale 2' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(['train', '--model', 'compact', '--scale', '2', '--init-generator', paths[4]])
    err = capsys.readouterr().err
    assert 'an x4 SRVGGNetCompact file' in err and '--scale 2' in err and '--scale 4' in err
    with pytest.raises(SystemExit):
        parse_args(['train', '--model', 'compact', '--init-generator', paths[3]])
    assert '27' in capsys.readouterr().err


def test_scale_messages_and_the_scale_read_off_a_compact_file():
    from torchsr_amd.esrgan.trainer import read_scale, scale_conflict
    from torchsr_amd.test import compact_scale
    from argparse import Namespace
    assert read_scale(Namespace()) == 4 and read_scale(Namespace(scale=2)) == 2 and read_scale(Namespace(scale=None)) == 4
    with pytest.raises(RuntimeError, match='--scale 3'):
        read_scale(Namespace(scale=3))
    assert 'x2 is inference-only unless the run is started with --scale 2' in scale_conflict('--init-generator f', 'RRDBNet', 2, 4)
    msg = scale_conflict('checkpoint c.pth', 'generator', 4, 2)
    assert 'checkpoint c.pth' in msg and 'x4' in msg and '--scale 2' in msg and 'inference-only' not in msg
    for s, cout in ((2, 12), (4, 48)):
        assert compact_scale(compact_ref.CompactRef(scale_factor=s, num_conv=1).state_dict()) == s
    with pytest.raises(RuntimeError, match='27 output channels'):
        compact_scale(compact_ref.CompactRef(scale_factor=3, num_conv=1).state_dict(), 'f.pth')


# ------------------------------------------------------------------ modules
def test_trainable_flag_of_the_layer_and_the_generator():
    from torchsr_amd.esrgan.generator import Generator
    from torchsr_amd.layers import Unshuffle2Conv2d
    assert Unshuffle2Conv2d().trainable is False and Unshuffle2Conv2d(trainable=True).trainable is True
    assert Unshuffle2Conv2d()._st.own_pack is False and Unshuffle2Conv2d(trainable=True)._st.own_pack is None
    plain, train = Generator(1, scale_factor=2), Generator(1, scale_factor=2, trainable=True)
    assert plain.trainable is False and plain.conv1.trainable is False and train.conv1.trainable is True
    assert list(plain.state_dict()) == list(train.state_dict())
    assert tuple(train.state_dict()['conv1.weight'].shape) == (64, 12, 3, 3)
    x4 = Generator(1, scale_factor=4, trainable=True)  # accepted, changes nothing
    assert list(x4.state_dict()) == list(Generator(1).state_dict()) and not isinstance(x4.conv1, Unshuffle2Conv2d)
    for gen in (plain, train):
        twin = copy.deepcopy(gen)
        assert twin.trainable is gen.trainable and twin.conv1.trainable is gen.conv1.trainable
        assert isinstance(twin.conv1, Unshuffle2Conv2d) and twin.conv1._st.own_pack is gen.conv1._st.own_pack
        assert all(torch.equal(a, b) for a, b in zip(twin.state_dict().values(), gen.state_dict().values()))
        assert twin.conv1.weight.data_ptr() != gen.conv1.weight.data_ptr()


def test_default_x2_stays_inference_only_and_a_trainable_one_gets_past_the_refusal():
    from torchsr_amd.esrgan.generator import Generator
    x = torch.zeros(1, 3, 4, 4)
    with pytest.raises(RuntimeError, match='inference-only'):
        Generator(1, scale_factor=2)(x)
    # a trainable one passes the module's checks and stops where the first device call refuses a CPU tensor
    with pytest.raises(RuntimeError) as exc:
        Generator(1, scale_factor=2, trainable=True)(x)
    assert 'inference-only' not in str(exc.value)


def test_an_image_that_requires_grad_is_refused():
    from torchsr_amd import functional as F
    from torchsr_amd.layers import Unshuffle2Conv2d
    m = Unshuffle2Conv2d(trainable=True)
    with pytest.raises(RuntimeError, match='no input gradient'):
        F.unshuffle2_conv(torch.zeros(1, 4, 4, 4, requires_grad=True), m.weight, m.bias, m._st, True)
    with pytest.raises(RuntimeError, match='inference-only'):
        F.unshuffle2_conv(torch.zeros(1, 4, 4, 4), m.weight, m.bias, m._st)


def test_pack_table_leaves_a_trainable_x2_layer_out():
    """The table's filter, without a device: a layer that packs per forward is not waited for and gets no record."""
    from torchsr_amd import functional as F
    from torchsr_amd.layers import Conv2d, Unshuffle2Conv2d
    table = F.PackTable([Unshuffle2Conv2d(trainable=True), Conv2d(64, 64, 3, 1, 1)])
    assert table._build() is False  # the 64 -> 64 layer has not run: nothing is ready, and nothing touched the device
    assert [c._st.own_pack for c in table.convs] == [None, False]


# ------------------------------------------------------------------ the C ABI: plan, workspace, refusals
def _cus():
    from torchsr_amd import _lib
    return _lib.lib().srx_plan_cus()


@pytest.mark.parametrize('shape', x2_ref.SHAPES + [(1, 2, 2), (3, 33, 47), (1, 1024, 1024)])
def test_plan_and_workspace_arithmetic(shape):
    n, h, w = shape
    p = x2_ref.plan(shape)
    ho, wo = x2_ref.out_hw(h, w)
    assert p['groups'] in (1, 2, 3) and 6 % p['groups'] == 0
    assert p['segments'] == n * ho * -(-wo // 16)
    assert 1 <= p['ranges'] <= max(1, (_cus() * 8) // p['groups'])
    assert p['segs_per_range'] * p['ranges'] >= p['segments'] > p['segs_per_range'] * (p['ranges'] - 1)  # the last range holds one
    assert p['slabs'] == -(-p['ranges'] // 4)
    assert x2_ref.ws_floats(shape) == p['slabs'] * 4 * 36 * 64


def test_the_plans_the_gpu_tests_rely_on():
    for shape in x2_ref.STEP_SHAPES:
        p = x2_ref.plan(shape)
        assert p['slabs'] > 1 and p['segs_per_range'] > 1, (shape, p)
    p = x2_ref.plan(x2_ref.RAGGED_SHAPE)
    assert p['ranges'] % 4 != 0 or p['segments'] % p['segs_per_range'] != 0, p  # an empty wave range or a short last one


FAKE = 0x10000  # never dereferenced: every call below is refused before a launch


def _bwd(shape, x=FAKE, dy=FAKE, dw=FAKE, ws=FAKE, ws_floats=None, accumulate=0):
    from torchsr_amd import _lib
    n = x2_ref.ws_floats(shape) if ws_floats is None else ws_floats
    rc = _lib.lib().srx_unshuffle2_conv_bwd_weight(*shape, x, dy, dw, accumulate, ws, n, None)
    return rc, _lib.last_error()


def test_refusals_with_made_up_pointers():
    from torchsr_amd import _lib
    for name in ('x', 'dy', 'dw', 'ws'):
        rc, msg = _bwd((1, 4, 4), **{name: None})
        assert rc == 1 and 'null pointer' in msg, (name, rc, msg)
    for shape, word in (((0, 4, 4), 'positive'), ((1, 0, 4), 'positive'), ((1, 4, -2), 'positive'), ((1, 1, 4), 'odd H'),
                        ((1, 4, 1), 'odd W'), ((1, 4096, 4096), '2^24'), ((4, 2047, 2048), '2^24')):
        rc, msg = _bwd(shape, ws_floats=1 << 30)
        assert rc == 1 and word in msg, (shape, rc, msg)
        assert x2_ref.ws_floats(shape) == 0
        out = (C.c_int * 8)()
        assert _lib.lib().srx_unshuffle2_conv_wgrad_plan(*shape, out) == 1
    assert _lib.lib().srx_unshuffle2_conv_wgrad_plan(1, 4, 4, None) == 1
    need = x2_ref.ws_floats((4, 64, 64))
    for n in (0, need - 1):
        rc, msg = _bwd((4, 64, 64), ws_floats=n)
        assert rc == 4 and 'workspace' in msg and str(need) in msg, (n, rc, msg)
