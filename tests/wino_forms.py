"""Every launch form of the Winograd F(2x2, 3x3) convolution (wino.hip): wino_kernel<32> / <64> through its five entry points --
srx_wino_fwd, srx_wino_bwd_data, srx_wino_fwd_stats, srx_wino_fwd_act and the PixelShuffle store of srx_wino_fwd_act -- with the
channel split of every tile (wino_fixup_kernel) and the cut tiles of the last round (wino_tail_fixup_kernel<32> / <64>), forced
through srx_wino_force_plan and held to the form by srx_wino_plan.

Data only (and the integer operands both test files share).  test_wino_forms_cpu.py holds every case to the form it is here for
through the host-only planner -- a planner change that makes a case vacuous fails there, without a GPU --;
test_wino_forms_gpu.py runs the launches: exact on integers, inside a derived bound of fp64 on random data.

A case: ``geo`` (N, H, W, Cin, Cout) of the LAYER (a data gradient contracts Cout channels into Cin columns); ``entry``: 'fwd', 'dgrad',
'stats', 'act' or 'shuffle' (srx_wino_fwd_act with shuffle = 2); the epilogue: ``bias``, ``relu``, ``mask`` (dgrad: the ReLU mask of
the layer below), ``slope`` (LeakyReLU, 0: none), ``addend``; ``force`` = (bn, zsplit, tsplit) of srx_wino_force_plan or None for the
cost model's own choice; ``expect`` = (bn, zsplit, tsplit, workgroups, tile blocks, chunks per workgroup): what srx_wino_plan must
answer (out[0], out[1], out[5], out[2], out[3], out[4]); ``kernels``: the launch records the case must leave under
srx_prof_start_aux, in order.  ``data``: the row whose operands the case uses (variants of a row share them and their references).

Rules of the table.  The geometries are the smallest at which each form exists: a tail needs more than CUS work items, tsplit = 8
needs Cin >= 256, zsplit = 16 needs Cin = 512; T = N (H / 2) (W / 2) tiles in blocks of 32.  Tail cases (``tail``) exist only on a
256-CU plan: where srx_plan_cus() != CUS they are skipped with TAIL_SKIP, never passed.  The table stays on the free chip (reserved
CUs: test_plan_forms_gpu.py)."""

CUS = 256
TAIL_SKIP = 'the cut tiles of a last round exist on a %d-CU plan only (srx_plan_cus() = %%d)' % CUS
WT = 32      # tiles per tile block
WKC = 32     # input channels per chunk of the packed weights: the unit of a split
SLOPE = 0.25  # a power of two: an integer times the slope is a whole number of quarters

MAIN = {32: 'wino_kernel<32>', 64: 'wino_kernel<64>'}
FIXUP = 'wino_fixup_kernel'
TAIL_FIXUP = {32: 'wino_tail_fixup_kernel<32>', 64: 'wino_tail_fixup_kernel<64>'}
ALL_KERNELS = sorted(MAIN.values()) + [FIXUP] + sorted(TAIL_FIXUP.values())

# srx_wino_plan / srx_wino_ws_floats: the launch a case's entry plans as
WHICH_FWD, WHICH_DGRAD, WHICH_STATS, WHICH_ACT = 0, 1, 2, 3

CASES = []


def _add(id_, geo, entry, force, expect, data=None, **epi):
    """One case; the kernels follow from the plan it expects: the main kernel, then the fix-up of a split or of the last round's parts."""
    bn, zs, ts = expect[:3]
    kernels = [MAIN[bn]] + ([FIXUP] if zs > 1 else []) + ([TAIL_FIXUP[bn]] if ts > 1 else [])
    case = dict(id=id_, data=data or id_.split('.')[0], geo=geo, entry=entry, force=force, expect=expect, kernels=kernels, tail=ts > 1,
                bias=False, relu=False, mask=False, slope=0.0, addend=False, wkeep=0.5)
    assert set(epi) <= set(case), epi
    case.update(epi)
    CASES.append(case)


# ---------------------------------------------------------------------------------------- the cut tiles of the last round (256 CUs)
# T1: 33 blocks x 8 channel blocks = 264 items: a tail of 8 tiles in 2 parts.  T = 1050: the last block has 26 valid tiles and is a tail tile
_add('T1', (7, 20, 30, 64, 256), 'fwd', (32, 1, 2), (32, 1, 2, 272, 33, 2), bias=True, relu=True)
# T2: the same on wino_tail_fixup_kernel<64> (512 threads): 66 x 4 = 264
_add('T2', (14, 20, 30, 64, 256), 'fwd', (64, 1, 2), (64, 1, 2, 272, 66, 2))
# T3: 5 parts: the second trip of the tail fix-up's 4-wide load loop, its loads clamped; nch = 5, one chunk per part
_add('T3', (7, 20, 30, 160, 256), 'fwd', (32, 1, 5), (32, 1, 5, 296, 33, 5), bias=True)
# T4: the most parts; BatchNorm statistics formed in the tail fix-up, the ragged block among its tiles
_add('T4.bias', (7, 20, 30, 256, 256), 'stats', (32, 1, 8), (32, 1, 8, 320, 33, 8), bias=True)
_add('T4.nobias', (7, 20, 30, 256, 256), 'stats', (32, 1, 8), (32, 1, 8, 320, 33, 8))
# ... and the same layer on whole tiles (264 items, nothing cut): the other side of the linearity check of T4
_add('T4.whole', (7, 20, 30, 256, 256), 'stats', (32, 1, 1), (32, 1, 1, 264, 33, 8), bias=True)
# T5: statistics in tail_fixup<64> and in the main kernel's NJ = 2 reduce (its ragged block: 20 valid tiles), in one launch
_add('T5', (14, 20, 30, 64, 256), 'stats', (64, 1, 2), (64, 1, 2, 272, 66, 2))
# T6: the mask read in the tail fix-up; the data gradient contracts 128 channels into 256 columns
_add('T6', (7, 20, 30, 256, 128), 'dgrad', (32, 1, 4), (32, 1, 4, 288, 33, 4), mask=True)

# ------------------------------------------------------------------------------------------------- the channel split of every tile
# Z1: the most splits: two full trips of wino_fixup_kernel's 8-wide loop; 9 tiles in one block
_add('Z1', (1, 6, 6, 512, 64), 'fwd', (64, 16, 1), (64, 16, 1, 16, 1, 1), bias=True, relu=True)
_add('Z1.whole', (1, 6, 6, 512, 64), 'fwd', (64, 1, 1), (64, 1, 1, 1, 1, 16), bias=True, relu=True)
# Z2: 9 splits over 10 chunks: uneven [kc0, kc1), the second trip clamped
_add('Z2', (1, 6, 6, 320, 64), 'fwd', (32, 9, 1), (32, 9, 1, 18, 1, 2), bias=True)
# Z3: one tile row (all of the vertical halo lies outside), 5 tiles, Cout = 32, chunks 1 / 1 / 2
_add('Z3', (1, 2, 10, 128, 32), 'fwd', (32, 3, 1), (32, 3, 1, 3, 1, 2))
# Z4: TW = 5 (odd), blocks that span images, the mask in wino_fixup_kernel
_add('Z4', (3, 6, 10, 128, 64), 'dgrad', (64, 2, 1), (64, 2, 1, 8, 2, 1), mask=True)
# Z5: the cost model's own split of that layer's forward
_add('Z5', (3, 6, 10, 128, 64), 'fwd', None, (32, 4, 1, 16, 2, 1), bias=True, relu=True)

# ------------------------------------------------------------------------------------------------------------------ whole tiles
# P1: one tile column, Cin = one chunk, Cout = 96 (no BN 64), 3 items: full < 8 in the XCD remap
_add('P1', (1, 10, 2, 32, 96), 'fwd', (32, 1, 1), (32, 1, 1, 3, 1, 1), bias=True)
# P2: 180 tiles = 6 blocks: 12 and 24 items, full % 8 = 4 and 0
_add('P2.bn64', (5, 12, 12, 64, 128), 'fwd', (64, 1, 1), (64, 1, 1, 12, 6, 2), relu=True)
_add('P2.bn32', (5, 12, 12, 64, 128), 'fwd', (32, 1, 1), (32, 1, 1, 24, 6, 2), relu=True)
# ST1: statistics of whole tiles in both epilogues, with a bias, the last block ragged (T = 120: 24 valid tiles)
_add('ST1.bn64', (2, 12, 20, 64, 128), 'stats', (64, 1, 1), (64, 1, 1, 8, 4, 2), bias=True)
_add('ST1.bn32', (2, 12, 20, 64, 128), 'stats', (32, 1, 1), (32, 1, 1, 16, 4, 2), bias=True)

# ------------------------------------------------------------------------------------- inference: LeakyReLU, addend, PixelShuffle
# A1: addend / LeakyReLU in the NJ = 2 and NJ = 1 epilogues, the last block ragged (T = 120)
for _tag, _epi in (('lrelu', dict(slope=SLOPE)), ('add', dict(addend=True)), ('lrelu_add', dict(slope=SLOPE, addend=True)),
                   ('relu_add', dict(relu=True, addend=True))):
    _add(f'A1.{_tag}.bn64', (2, 12, 20, 64, 128), 'act', (64, 1, 1), (64, 1, 1, 8, 4, 2), bias=True, **_epi)
    _add(f'A1.{_tag}.bn32', (2, 12, 20, 64, 128), 'act', (32, 1, 1), (32, 1, 1, 16, 4, 2), bias=True, **_epi)
# A2: 288 tiles = 9 blocks, 18 items: full % 8 = 2
_add('A2', (3, 16, 24, 64, 128), 'act', (64, 1, 1), (64, 1, 1, 18, 9, 2), slope=SLOPE, addend=True)
# A3: srx_wino_fwd_act with none of the three is a plain forward and plans as one: Z5's layer, Z5's split, through the other entry
_add('A3', (3, 6, 10, 128, 64), 'act', None, (32, 4, 1, 16, 2, 1), data='Z5', bias=True, relu=True)
# S1: the shuffled store and the bias's (cc * 4 + ij) order in both BN; ws = NULL
_add('S1.bn64', (2, 12, 20, 64, 256), 'shuffle', (64, 1, 1), (64, 1, 1, 16, 4, 2), bias=True, slope=SLOPE)
_add('S1.bn32', (2, 12, 20, 64, 256), 'shuffle', (32, 1, 1), (32, 1, 1, 32, 4, 2), bias=True, slope=SLOPE)
# S2: Cout / 4 = 32: a 32-column pass is exactly one sub-pixel
_add('S2', (1, 6, 6, 128, 128), 'shuffle', (32, 1, 1), (32, 1, 1, 4, 1, 4), bias=True)

# the random-data rows, one per kernel path (T4.whole and Z1.whole: the linearity of a split -- both plans of one layer meet the bound)
RANDOM_IDS = ['T1', 'T4.bias', 'T4.whole', 'T6', 'Z1', 'Z1.whole', 'Z4', 'A1.lrelu_add.bn64', 'S1.bn64', 'S1.bn32']

# ----------------------------------------------------------------------------------------------- R: fall-backs and refusals
# (geometry, entry, forced plan, why the launch cannot take it): srx_wino_plan must answer what it answers with nothing forced
FALLBACKS = [
    ((7, 20, 30, 256, 256), 'stats', (32, 4, 1), 'statistics come from whole outputs: no split of every tile'),
    ((2, 12, 20, 64, 128), 'act', (64, 2, 1), 'the fix-up pass knows no LeakyReLU / addend: no split'),
    ((14, 20, 30, 64, 256), 'act', (64, 1, 2), '... and no cut tiles'),
    ((2, 12, 20, 64, 256), 'shuffle', (32, 1, 2), 'nor with a PixelShuffle store'),
    ((2, 12, 20, 64, 256), 'shuffle', (32, 2, 1), 'nor a split'),
    ((7, 20, 30, 128, 256), 'dgrad', (32, 1, 4), '33 x 4 = 132 items: no last round to cut'),
    ((7, 20, 30, 128, 256), 'dgrad', (32, 2, 2), 'a split and cut tiles exclude each other'),
    ((10, 20, 30, 256, 256), 'fwd', (32, 1, 8), '47 x 8 = 376 items: tail 120 x 8 parts > 2 x 256'),
    ((1, 10, 2, 32, 96), 'fwd', (64, 1, 1), 'BN 64 does not divide Cout = 96'),
    ((1, 2, 10, 128, 32), 'fwd', (32, 5, 1), 'more splits than the 4 chunks of 32 input channels'),
    ((7, 20, 30, 64, 256), 'fwd', (32, 1, 3), 'more parts than the 2 chunks'),
]
BAD_FORCE = [(48, 1, 1), (64, 17, 1), (32, 1, 9), (0, 1, 1)]


def by_id(cases):
    return [c['id'] for c in cases]


def case(id_):
    return next(c for c in CASES if c['id'] == id_)


def which(entry, slope=0.0, addend=False):
    """The launch kind srx_wino_plan / srx_wino_ws_floats describe for an entry"""
    if entry == 'act':
        return WHICH_ACT if (slope or addend) else WHICH_FWD
    return {'fwd': WHICH_FWD, 'dgrad': WHICH_DGRAD, 'stats': WHICH_STATS, 'shuffle': WHICH_ACT}[entry]


def desc_fields(geo, entry, relu=False, slope=0.0):
    """Conv2dDesc fields: N, H, W, Cin, Cin_s, Cout, Cout_s, KH, KW, stride, pad, shuffle, act, slope, up, precision"""
    n, h, w, cin, cout = geo
    sh = 2 if entry == 'shuffle' else 0
    act = 2 if slope else 1 if relu else 0
    return (n, h, w, cin, cin, cout, cout // 4 if sh else cout, 3, 3, 1, 1, sh, act, float(slope), 0, 0)


def gemm_dims(c):
    """(contracted channels, output columns) of the case's launch: swapped for a data gradient"""
    cin, cout = c['geo'][3:]
    return (cout, cin) if c['entry'] == 'dgrad' else (cin, cout)


def int_inputs(c):
    """The integer operands of a case's exact check (numpy integer arrays, NCHW / OIHW; the tests cast them to fp32), seeded by the
    case's data row: ``x`` in {-1, 0, 1} (a data gradient: the output gradient, Cout channels); ``w`` in {-4, 0, 4}, a fraction
    ``wkeep`` non-zero -- with multiples of 4 every entry of G g G^T is an integer --; ``bias``: a channel-dependent integer;
    ``addend``: integers in [-3, 3], laid out like the conv's output; ``below``: the integer pre-activation of the layer below a data
    gradient, whose ReLU (exact zeros) is the mask.  Every product, times SLOPE, is a whole number of quarters."""
    import zlib
    import numpy as np
    rng = np.random.default_rng(zlib.crc32(c['data'].encode()))
    n, h, w, cin, cout = c['geo']
    d = dict(x=rng.integers(-1, 2, (n, cout if c['entry'] == 'dgrad' else cin, h, w), dtype=np.int8))
    keep = rng.random((cout, cin, 3, 3), dtype=np.float32) < c['wkeep']
    d['w'] = (4 * rng.integers(-1, 2, (cout, cin, 3, 3), dtype=np.int8) * keep).astype(np.int8)
    d['bias'] = ((np.arange(cout) * 7) % 11 - 5).astype(np.int8)
    d['addend'] = rng.integers(-3, 4, (n, cout, h, w), dtype=np.int8)
    d['below'] = rng.integers(-1, 3, (n, cin, h, w), dtype=np.int8)
    return d
