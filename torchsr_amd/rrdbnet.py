"""Published RRDBNet checkpoints as ``esrgan.Generator`` states: key maps and the net's geometry, host code only.

``esrgan.Generator`` IS RRDBNet (3 -> 64 conv, RRDBs of three 5-conv dense blocks with 0.2 scaling, a trunk conv, two nearest-x2
+ conv + LeakyReLU stages, the 64 -> 64 and 64 -> 3 convs); only the parameter names differ.  Three namings are understood:

=====================  ==============================  ==================================  ===========================
                       this package ("own")            BasicSR / Real-ESRGAN ("basicsr")   xinntao/ESRGAN new arch ("xinntao")
=====================  ==============================  ==================================  ===========================
input conv             ``conv1``                       ``conv_first``                      ``conv_first``
dense conv k <= 4      ``blocks.i.RDBj.convk.0``       ``body.i.rdbj.convk``               ``RRDB_trunk.i.RDBj.convk``
dense conv 5           ``blocks.i.RDBj.conv5``         ``body.i.rdbj.conv5``               ``RRDB_trunk.i.RDBj.conv5``
trunk conv             ``conv2``                       ``conv_body``                       ``trunk_conv``
x2 stages              ``upsample1``, ``upsample2``    ``conv_up1``, ``conv_up2``          ``upconv1``, ``upconv2``
64 -> 64, 64 -> 3      ``conv3.0``, ``conv4``          ``conv_hr``, ``conv_last``          ``HRconv``, ``conv_last``
=====================  ==============================  ==================================  ===========================

(each with ``.weight`` and ``.bias``).  ``RealESRGAN_x4plus`` and ``ESRGAN_SRx4_DF2KOST_official`` are 23 blocks at x4,
``RealESRGAN_x4plus_anime_6B`` 6 blocks, ``RealESRGAN_x2plus`` 23 blocks behind ``pixel_unshuffle(2)``: its input conv takes 12
channels.  Everything is checked here, before any device work; what does not fit is refused with a ``RuntimeError`` that names
the key or the shape.
"""
import re
from collections import OrderedDict

NUM_FEAT, GROWTH = 64, 32

_HEAD = {'own': 'conv1', 'basicsr': 'conv_first', 'xinntao': 'conv_first'}
_TAIL = {'own': ('conv2', 'upsample1', 'upsample2', 'conv3.0', 'conv4'),
         'basicsr': ('conv_body', 'conv_up1', 'conv_up2', 'conv_hr', 'conv_last'),
         'xinntao': ('trunk_conv', 'upconv1', 'upconv2', 'HRconv', 'conv_last')}
_BLOCK = {'own': re.compile(r'^blocks\.(\d+)\.RDB([1-3])\.conv(?:([1-4])\.0|(5))$'),
          'basicsr': re.compile(r'^body\.(\d+)\.rdb([1-3])\.conv(?:([1-4])|(5))$'),
          'xinntao': re.compile(r'^RRDB_trunk\.(\d+)\.RDB([1-3])\.conv(?:([1-4])|(5))$')}
_BLOCK_FMT = {'own': lambda i, j, k: f'blocks.{i}.RDB{j}.conv{k}' + ('.0' if k <= 4 else ''),
              'basicsr': lambda i, j, k: f'body.{i}.rdb{j}.conv{k}',
              'xinntao': lambda i, j, k: f'RRDB_trunk.{i}.RDB{j}.conv{k}'}
# names that only one naming uses: the first of them met decides, and one from another naming is a mix
_MARKS = {'own': ('conv1', 'blocks', 'conv2', 'upsample1', 'upsample2', 'conv3', 'conv4'),
          'basicsr': ('body', 'conv_body', 'conv_up1', 'conv_up2', 'conv_hr'),
          'xinntao': ('RRDB_trunk', 'trunk_conv', 'upconv1', 'upconv2', 'HRconv')}


def _naming(state) -> str:
    found = {}
    for key in state:
        for naming, marks in _MARKS.items():
            if key.split('.')[0] in marks:
                found.setdefault(naming, key)
    if not found:
        raise RuntimeError(f'not an RRDBNet state_dict: no key of a known naming among {list(state)[:4]} ...')
    if len(found) > 1:
        raise RuntimeError('an RRDBNet state_dict in a mix of namings: '
                           + ', '.join(f'{key!r} ({naming})' for naming, key in sorted(found.items())))
    return next(iter(found))


def _layout(state, naming: str):
    """``[(module name in ``naming``, own module name, weight shape)]`` of the net this state holds, after checking that it
    holds exactly that net: contiguous blocks, no missing or surplus key, 64 features, growth 32, 3 or 12 input channels."""
    modules = {}
    for key in state:
        mod, _, leaf = key.rpartition('.')
        if leaf not in ('weight', 'bias') or not mod:
            raise RuntimeError(f'surplus key {key!r}: RRDBNet holds only conv weights and biases')
        modules.setdefault(mod, set()).add(leaf)
    blocks = set()
    for mod in modules:
        m = _BLOCK[naming].match(mod)
        if m:
            blocks.add(int(m.group(1)))
    if not blocks:
        raise RuntimeError(f'an RRDBNet state_dict without a block: no key like {_BLOCK_FMT[naming](0, 1, 1)!r}.weight')
    num_blocks = max(blocks) + 1
    for i in range(num_blocks):
        if i not in blocks:
            raise RuntimeError(f'missing key {_BLOCK_FMT[naming](i, 1, 1) + ".weight"!r}: block {i} of 0..{num_blocks - 1} is absent '
                               '(the block indices must be contiguous from 0)')
    head = _HEAD[naming]
    if head + '.weight' not in state:
        raise RuntimeError(f'missing key {head + ".weight"!r}')
    first = tuple(state[head + '.weight'].shape)
    if len(first) != 4 or first[0] != NUM_FEAT or first[2:] != (3, 3):
        raise RuntimeError(f'{head}.weight has shape {first}: num_feat must be {NUM_FEAT} and the kernel 3x3 '
                           f'([{NUM_FEAT}, 3 or 12, 3, 3])')
    if first[1] == 48:
        raise RuntimeError(f'{head}.weight has shape {first}: 48 input channels are RRDBNet at x1 (pixel_unshuffle(4)), which has '
                           'no kernel here; x4 (3 channels) and x2 (12 channels) do')
    if first[1] not in (3, 12):
        raise RuntimeError(f'{head}.weight has shape {first}: 3 input channels (x4) or 12 (x2) expected')
    layout = [(head, 'conv1', first)]
    for i in range(num_blocks):
        for j in (1, 2, 3):
            for k in (1, 2, 3, 4, 5):
                shape = (GROWTH if k <= 4 else NUM_FEAT, NUM_FEAT + (k - 1) * GROWTH, 3, 3)
                layout.append((_BLOCK_FMT[naming](i, j, k), _BLOCK_FMT['own'](i, j, k), shape))
    for mod, own in zip(_TAIL[naming], _TAIL['own']):
        layout.append((mod, own, (3 if own == 'conv4' else NUM_FEAT, NUM_FEAT, 3, 3)))
    for mod, _, shape in layout:
        for leaf, want in (('weight', shape), ('bias', shape[:1])):
            key = f'{mod}.{leaf}'
            if key not in state:
                raise RuntimeError(f'missing key {key!r}')
            if tuple(state[key].shape) != want:
                what = ''
                if _BLOCK[naming].match(mod):
                    what = f' (num_feat must be {NUM_FEAT} and the growth {GROWTH})'
                raise RuntimeError(f'{key} has shape {tuple(state[key].shape)}, expected {want}{what}')
    known = {mod for mod, _, _ in layout}
    for mod in modules:
        if mod not in known:
            raise RuntimeError(f'surplus key {mod + "." + sorted(modules[mod])[0]!r}: no such layer in RRDBNet with {num_blocks} blocks')
    return layout, num_blocks, {3: 4, 12: 2}[first[1]]


def rrdbnet_geometry(state):
    """``(num_blocks, scale)`` of an RRDBNet state in any of the three namings: the blocks from the highest block index (contiguous
    from 0), the scale from the input conv's channels (3 -> 4, 12 -> 2).  ``RuntimeError`` for what ``rrdbnet_to_generator_state``
    refuses."""
    _, num_blocks, scale = _layout(state, _naming(state))
    return num_blocks, scale


def rrdbnet_to_generator_state(state) -> OrderedDict:
    """An RRDBNet state_dict in BasicSR / Real-ESRGAN naming, xinntao/ESRGAN "new arch" naming or this package's own, as
    ``esrgan.Generator(num_blocks, scale_factor)``'s state_dict (the tensors themselves, in the generator's key order).
    ``RuntimeError``, naming the key or shape: 48 input channels (x1), ``num_feat`` other than 64, a growth other than 32, a
    missing or surplus key, a mix of namings."""
    layout, _, _ = _layout(state, _naming(state))
    out = OrderedDict()
    for mod, own, _ in layout:
        out[own + '.weight'] = state[mod + '.weight']
        out[own + '.bias'] = state[mod + '.bias']
    return out


def generator_to_rrdbnet_state(state) -> OrderedDict:
    """The inverse: an ``esrgan.Generator`` state (or either published naming) in BasicSR / Real-ESRGAN naming, for
    Real-ESRGAN's own tools (``{'params_ema': generator_to_rrdbnet_state(g.state_dict())}``)."""
    naming = _naming(state)
    layout, _, _ = _layout(state, naming)
    names = [_HEAD['basicsr']] + [None] * (len(layout) - 6) + list(_TAIL['basicsr'])
    out = OrderedDict()
    for (mod, own, _), name in zip(layout, names):
        if name is None:
            i, j, k4, k5 = _BLOCK['own'].match(own).groups()
            name = _BLOCK_FMT['basicsr'](int(i), int(j), int(k4 or k5))
        out[name + '.weight'] = state[mod + '.weight']
        out[name + '.bias'] = state[mod + '.bias']
    return out
