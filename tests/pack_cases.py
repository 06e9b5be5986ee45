"""The layers test_pack_table_gpu.py and test_pack_table_cpu.py pack: conv layers of both models and the edges of
``pack_table_kernel``'s indexing (csrc/convpack.hip), and the layers whose Winograd-domain weights ride in the same table.

A case gives the layer, never a packed size: those come from the library (``srx_conv2d_packed_*_floats``,
``srx_wino_packed_floats``).  ``thin`` says which side of the layer runs on thin.hip's 3-channel kernels and so is packed in
their ``p[c][tap][ch]`` layout; test_pack_table_cpu.py asks the library (``srx_thin_plan``) that it agrees.

No shape was refused by ``check_desc`` or ``srx_conv2d_pack``: nothing had to leave the list.
"""
N, H, W = 1, 8, 8   # the descriptor's image: as small as check_desc admits for every kernel size here (9 x 9 at pad 4 included)


def _case(id, cin, cout, k, stride=1, pad=None, shuffle=0, up=0, precision=0, bwd=True, thin=None, cin_s=None):
    return dict(id=id, cin=cin, cout=cout, k=k, stride=stride, pad=(k - 1) // 2 if pad is None else pad, shuffle=shuffle, up=up,
                precision=precision, bwd=bwd, thin=thin, cin_s=cin_s)


CASES = [
    # ---- layers of the two models
    _case('c64.k3', 64, 64, 3),
    _case('first.k9', 3, 64, 9, thin='dgrad'),                  # SRGAN generator, first conv: thin kind 3
    _case('last.k9', 64, 3, 9, thin='fwd'),                     # ... and last: thin kind 2
    _case('last.k3', 64, 3, 3, thin='fwd'),                     # ESRGAN generator, last conv
    _case('first.k3', 3, 64, 3, thin='dgrad'),                  # ... first conv; both discriminators
    _case('shuffle', 64, 256, 3, shuffle=2),
    _case('c64.s2', 64, 64, 3, stride=2),
    _case('c512.s2', 512, 512, 3, stride=2),                    # the largest records: 512 x 512 work items each
    _case('rdb.192to32', 192, 32, 3, cin_s=192),                # dense-block convs reading the 192-strided buffer
    _case('rdb.160to32', 160, 32, 3, cin_s=192),
    _case('c64.up2', 64, 64, 3, up=2),
    _case('c64.k3.bf16', 64, 64, 3, precision=1),               # the 64-channel ones again with bf16 products
    _case('last.k9.bf16', 64, 3, 9, precision=1, thin='fwd'),
    _case('last.k3.bf16', 64, 3, 3, precision=1, thin='fwd'),
    _case('shuffle.bf16', 64, 256, 3, shuffle=2, precision=1),
    _case('c64.s2.bf16', 64, 64, 3, stride=2, precision=1),
    _case('c64.up2.bf16', 64, 64, 3, up=2, precision=1),
    # ---- edges of the table kernel's indexing
    _case('e8to12', 8, 12, 3),                                  # Cout and Cin below any tile
    _case('e4to8.s2', 4, 8, 3, stride=2),
    _case('e16to20.k5', 16, 20, 5),                             # 25 taps: nine at a time with a tail of seven
    _case('e32.k1', 32, 32, 1),                                 # one tap
    _case('e24to40.s3', 24, 40, 3, stride=3, pad=1),            # nine classes of one tap
    _case('e16.k4.s2', 16, 16, 4, stride=2, pad=1),             # four classes of four taps
    _case('e12to8.k7', 12, 8, 7),                               # 49 taps: a tail of four
    _case('e16to24.s4', 16, 24, 3, stride=4, pad=1),            # sixteen classes, seven of them without any tap
    _case('e3to16', 3, 16, 3),                                  # Ck = 4 > Cin = 3 on a layer that is not thin: a zero channel
    _case('c64.s2.nobwd', 64, 64, 3, stride=2, bwd=False),      # wpk_bwd = NULL
]
for _i, _c in enumerate(CASES):
    _c['w_offset'] = 1 - _i % 2   # floats between the weight and its 16-byte aligned allocation: 1 in every other case

# layers of the one-table test that are packed forward-only there although the case has a data gradient (a NULL wpk_bwd entry)
TABLE_FWD_ONLY = ('e16to20.k5', 'c64.k3.bf16')

# 3x3 / stride 1 / pad 1 layers whose U = G g G^T is refreshed by kind 4, 5 (transpose) and 6 (shuffle) records
WINO_CASES = [
    dict(id='w64', cin=64, cout=64, shuffle=0),
    dict(id='w32to96', cin=32, cout=96, shuffle=0),
    dict(id='w96to32', cin=96, cout=32, shuffle=0),
    dict(id='w256', cin=256, cout=256, shuffle=0),
    dict(id='w64to256.shuffle', cin=64, cout=256, shuffle=2),
]


def round4(c):
    return (c + 3) // 4 * 4


def desc_fields(c):
    """The fields of ``srx_conv2d_t`` (``_lib.Conv2dDesc``) of a case."""
    cout_s = round4(c['cout'] // 4) if c['shuffle'] else round4(c['cout'])
    return (N, H, W, c['cin'], c['cin_s'] or round4(c['cin']), c['cout'], cout_s, c['k'], c['k'], c['stride'], c['pad'],
            c['shuffle'], 0, 0.0, c['up'], c['precision'])


def wino_desc_fields(c):
    cout_s = c['cout'] // 4 if c['shuffle'] else c['cout']
    return (N, H, W, c['cin'], c['cin'], c['cout'], cout_s, 3, 3, 1, 1, c['shuffle'], 0, 0.0, 0, 0)


def predicted_nrec(c, bwd=None):
    """Records ``srx_pack_table_build`` writes for the layer: the forward pack and, with a backward destination, either the one
    thin record or one per stride-parity class.  ``bwd_classes`` (csrc/gconv.hip) emits all stride^2 classes -- one without a
    tap keeps a row of zero padding, K = 0 and Kp = 32 -- and drops none; strides above 4 are refused, so at most 1 + 16."""
    bwd = c['bwd'] if bwd is None else bwd
    if not bwd:
        return 1
    return 2 if c['thin'] == 'dgrad' else 1 + c['stride'] ** 2


def wino_records(c):
    """(transpose, kind) of the layer's records: a PixelShuffle layer has no Winograd data gradient."""
    return [(0, 6)] if c['shuffle'] else [(0, 4), (1, 5)]


def by_id(cases):
    return [c['id'] for c in cases]
