"""Published RRDBNet checkpoints without a GPU: the key maps against the restatement in ``tests/rrdbnet_ref.py`` (whose
``state_dict()`` has BasicSR's key names), the geometry read off the keys, every refusal, the x2 generator's schema and the
tile rounding of ``test.upscale`` as a pure function."""
from collections import OrderedDict

import pytest
import torch

from rrdbnet_ref import RRDBNetRef, seeded_state, xinntao_names


def _shapes(sd):
    return {k: tuple(v.shape) for k, v in sd.items()}


@pytest.mark.parametrize('scale', [4, 2])
def test_basicsr_state_translates_to_the_generators_schema(scale):
    from torchsr_amd.esrgan.generator import Generator
    from torchsr_amd.test import rrdbnet_to_generator_state
    pub = seeded_state(RRDBNetRef(num_block=2, scale=scale))
    got = rrdbnet_to_generator_state(pub)
    gen = Generator(2, scale_factor=scale)
    want = gen.state_dict()
    assert list(got) == list(want)
    assert _shapes(got) == _shapes(want)
    assert tuple(got['conv1.weight'].shape) == (64, 3 if scale == 4 else 12, 3, 3)
    gen.load_state_dict(got)  # key for key, strict
    # the tensors themselves, each where the architecture puts it
    assert got['conv1.weight'] is pub['conv_first.weight'] and got['conv4.bias'] is pub['conv_last.bias']
    assert got['blocks.1.RDB3.conv2.0.weight'] is pub['body.1.rdb3.conv2.weight']
    assert got['blocks.0.RDB1.conv5.bias'] is pub['body.0.rdb1.conv5.bias']
    assert got['conv2.weight'] is pub['conv_body.weight'] and got['conv3.0.weight'] is pub['conv_hr.weight']
    assert got['upsample1.weight'] is pub['conv_up1.weight'] and got['upsample2.bias'] is pub['conv_up2.bias']


@pytest.mark.parametrize('scale', [4, 2])
def test_xinntao_names_translate_to_the_same_state(scale):
    from torchsr_amd.test import rrdbnet_to_generator_state
    pub = seeded_state(RRDBNetRef(num_block=2, scale=scale), seed=1)
    old = xinntao_names(pub)
    assert 'RRDB_trunk.1.RDB2.conv3.weight' in old and 'trunk_conv.bias' in old and 'HRconv.weight' in old
    a, b = rrdbnet_to_generator_state(pub), rrdbnet_to_generator_state(old)
    assert list(a) == list(b)
    assert all(a[k] is b[k] for k in a)


def test_own_names_pass_through():
    from torchsr_amd.esrgan.generator import Generator
    from torchsr_amd.test import rrdbnet_to_generator_state
    own = Generator(2).state_dict()
    got = rrdbnet_to_generator_state(own)
    assert list(got) == list(own) and all(got[k] is own[k] for k in own)
    assert isinstance(got, OrderedDict)


def test_geometry_from_the_keys_alone():
    from torchsr_amd.test import rrdbnet_geometry, rrdbnet_to_generator_state
    for blocks, scale in ((2, 4), (2, 2), (6, 4), (23, 4)):
        # shapes are all the geometry reads: meta tensors, nothing allocated
        with torch.device('meta'):
            pub = RRDBNetRef(num_block=blocks, scale=scale).state_dict()
        assert rrdbnet_geometry(pub) == (blocks, scale)
        assert rrdbnet_geometry(xinntao_names(pub)) == (blocks, scale)
        assert rrdbnet_geometry(rrdbnet_to_generator_state(pub)) == (blocks, scale)


def _pub(**kw):
    with torch.device('meta'):
        return RRDBNetRef(**{'num_block': 2, **kw}).state_dict()


def test_refusals_name_the_key_or_shape():
    from torchsr_amd.test import rrdbnet_geometry, rrdbnet_to_generator_state

    def refused(state, *words):
        for fn in (rrdbnet_to_generator_state, rrdbnet_geometry):
            with pytest.raises(RuntimeError) as e:
                fn(state)
            for word in words:
                assert word in str(e.value), (word, str(e.value))

    x1 = _pub()
    x1['conv_first.weight'] = torch.empty(64, 48, 3, 3, device='meta')
    refused(x1, 'conv_first.weight', '(64, 48, 3, 3)', 'x1')                          # 48 input channels: x1
    refused(_pub(num_feat=48), 'conv_first.weight', '(48, 3, 3, 3)', 'num_feat')      # num_feat != 64
    refused(_pub(num_grow_ch=16), 'body.0.rdb1.conv1.weight', '(16, 64, 3, 3)', 'growth')  # growth != 32
    missing = _pub()
    del missing['body.1.rdb2.conv4.bias']
    refused(missing, 'missing', 'body.1.rdb2.conv4.bias')
    hole = OrderedDict((k, v) for k, v in _pub(num_block=3).items() if not k.startswith('body.1.'))
    refused(hole, 'missing', 'body.1.rdb1.conv1.weight', 'contiguous')                 # blocks 0 and 2 only
    headless = _pub()
    del headless['conv_first.weight']
    refused(headless, 'missing', 'conv_first.weight')
    surplus = _pub()
    surplus['conv_extra.weight'] = torch.empty(64, 64, 3, 3, device='meta')
    refused(surplus, 'surplus', 'conv_extra.weight')
    stats = _pub()
    stats['body.0.rdb1.conv1.num_batches_tracked'] = torch.empty((), device='meta')
    refused(stats, 'surplus', 'body.0.rdb1.conv1.num_batches_tracked')
    mixed = _pub()
    mixed['trunk_conv.weight'] = mixed.pop('conv_body.weight')                         # one xinntao name among BasicSR's
    refused(mixed, 'mix', 'trunk_conv.weight')
    mixed2 = _pub()
    mixed2['conv1.weight'] = mixed2.pop('conv_first.weight')                           # one own name among BasicSR's
    refused(mixed2, 'mix', 'conv1.weight')
    refused({'features.0.weight': torch.empty(1, device='meta')}, 'not an RRDBNet')


def test_generator_to_rrdbnet_state_round_trips():
    from torchsr_amd.esrgan.generator import Generator
    from torchsr_amd.test import generator_to_rrdbnet_state, rrdbnet_to_generator_state
    for scale in (4, 2):
        pub = seeded_state(RRDBNetRef(num_block=2, scale=scale), seed=2)
        back = generator_to_rrdbnet_state(rrdbnet_to_generator_state(pub))
        assert list(back) == list(pub) and all(back[k] is pub[k] for k in pub)
        own = Generator(2, scale_factor=scale).state_dict()
        there = generator_to_rrdbnet_state(own)
        RRDBNetRef(num_block=2, scale=scale).load_state_dict(there)  # a generator trained here loads into RRDBNet, strict
        again = rrdbnet_to_generator_state(there)
        assert list(again) == list(own) and all(again[k] is own[k] for k in own)


def test_generator_scale_factor():
    from torchsr_amd.esrgan.generator import Generator
    from torchsr_amd.layers import Conv2d, Unshuffle2Conv2d
    for bad in (3, 1, 8, 0):
        with pytest.raises(ValueError):
            Generator(2, scale_factor=bad)
    a, b = Generator(2), Generator(2, scale_factor=4)
    assert _shapes(a.state_dict()) == _shapes(b.state_dict()) and list(a.state_dict()) == list(b.state_dict())
    assert [type(m) for m in a.modules()] == [type(m) for m in b.modules()]
    assert type(b.conv1) is Conv2d and b.halo == 64 and not hasattr(b, 'tile_align') and b.scale_factor == 4
    x2 = Generator(2, scale_factor=2)
    assert type(x2.conv1) is Unshuffle2Conv2d and x2.tile_align == 2 and x2.halo == 128 and x2.scale_factor == 2
    assert [k for k in x2.state_dict()] == [k for k in a.state_dict()]
    with pytest.raises(RuntimeError, match='inference-only'):  # before any device work: a CPU tensor gets this far
        x2.train()(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match='inference-only'):
        x2.eval()(torch.zeros(1, 3, 8, 8))  # autograd enabled
    with torch.no_grad(), pytest.raises(RuntimeError, match='at least 3'):
        x2.eval()(torch.zeros(1, 3, 1, 8))


def _tiles_today(n, h, w, halo, max_tile_pixels):
    """The tile arithmetic of ``test.upscale`` as it stood before ``tile_plan`` existed, restated."""
    rows = max(1, -(-h * w * n // max_tile_pixels))
    th = -(-h // int(rows ** 0.5 + 0.999))
    tw = max(1, max_tile_pixels // (n * (th + 2 * halo))) - 2 * halo
    tw = max(64, min(tw, w))
    tiles = []
    for y0 in range(0, h, th):
        for x0 in range(0, w, tw):
            y1, x1 = min(h, y0 + th), min(w, x0 + tw)
            tiles.append((y0, y1, x0, x1, max(0, y0 - halo), min(h, y1 + halo), max(0, x0 - halo), min(w, x1 + halo)))
    return th, tw, tiles


# (h, w, halo, max_tile_pixels) of test_tiled_inference_equals_untiled, of test_esrgan_tiled_inference_border_error (both
# halos), of the default 1080p call, and odd sizes
TILE_CASES = [(150, 210, 48, 150 * 110), (320, 352, 64, 128 * 256), (320, 352, 128, 128 * 256), (1080, 1920, 64, 600 * 1000),
              (97, 140, 40, 3000), (97, 141, 39, 2999), (33, 700, 7, 5000)]


@pytest.mark.parametrize('case', TILE_CASES)
def test_tile_plan_with_align_1_is_todays_tiling(case):
    from torchsr_amd.test import tile_plan
    h, w, halo, mtp = case
    for n in (1, 2):
        th, tw, tiles = _tiles_today(n, h, w, halo, mtp)
        assert tile_plan(h, w, halo, mtp, 1, n) == (th, tw, halo, tiles)
    assert tile_plan(h, w, halo, mtp) == tile_plan(h, w, halo, mtp, 1, 1)
    assert len(tile_plan(150, 210, 48, 150 * 110)[3]) > 1


@pytest.mark.parametrize('case', TILE_CASES)
def test_tile_plan_with_align_2_is_even(case):
    from torchsr_amd.test import tile_plan
    h, w, halo, mtp = case
    th, tw, halo2, tiles = tile_plan(h, w, halo, mtp, 2)
    assert th % 2 == 0 and tw % 2 == 0 and halo2 % 2 == 0 and halo <= halo2 <= halo + 1
    cover = torch.zeros(h, w, dtype=torch.int32)
    for y0, y1, x0, x1, ya, yb, xa, xb in tiles:
        assert y0 % 2 == 0 and x0 % 2 == 0 and ya % 2 == 0 and xa % 2 == 0       # every origin even: the image's unshuffle phase
        assert (y1 - y0) % 2 == 0 or y1 == h
        assert (x1 - x0) % 2 == 0 or x1 == w                                     # an odd size only at the image's own odd edge
        assert (yb % 2 == 0 or yb == h) and (xb % 2 == 0 or xb == w)
        assert ya <= y0 < y1 <= yb and xa <= x0 < x1 <= xb
        assert ya == max(0, y0 - halo2) and yb == min(h, y1 + halo2) and xa == max(0, x0 - halo2) and xb == min(w, x1 + halo2)
        cover[y0:y1, x0:x1] += 1
    assert bool((cover == 1).all())  # the interiors tile the image exactly once
