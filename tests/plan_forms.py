"""Launch forms that real runs reach and the step-size tables (step_layers.py) do not: the 48-pixel row tile, persistent inference
workgroups that walk several work items, and the plans the planners cut when compute units are reserved for a collective's
channel kernels (srx_set_reserved_cus: ddp.GradBuckets opens such a window inside every data-parallel step); and every launch
form of the kernels with a 3-channel side (thin.hip, section 4).

Data only.  test_plan_forms_cpu.py holds every case to the form it is here for through the host-only planners (a planner change
that makes a case vacuous fails there, without a GPU); test_plan_forms_gpu.py and test_thin_forms_gpu.py run the launches against
fp64.  All plans below are
those of a 256-CU part -- what srx_plan_cus() reports on the MI355X and, by default, without a GPU."""

CUS = 256

# ------------------------------------------------------------------------------------------------------------ 1. row tile, 48 pixels
# 3x3 / 64 -> 64 / stride 1 / fp32 layers (rowtile.hip).  tile_pixels() takes 48 when M / 36 > plan CUs >= M / 48:
# (N, H, W, NB = patch-load batches per thread (the kernel's first template argument), reserved CUs).  With nothing reserved 11 520
# pixels are 320 tiles of 36 or 240 of 48; at the reference batch (9216 pixels: 256 tiles of 36) any reservation from 8 to 64 CUs
# moves the plan to 192 tiles of 48 -- the form every data-parallel SRGAN step runs inside its communication windows.
ROW_TILE_48 = [(20, 24, 24, 1, 0), (5, 48, 48, 2, 0), (16, 24, 24, 1, 8)]
ROW_TILE_PIXELS = 48


def row_tile_desc(n, h, w, act=0, slope=0.0):
    """Conv2dDesc fields of the row-tile layer."""
    return (n, h, w, 64, 64, 64, 64, 3, 3, 1, 1, 0, act, slope, 0, 0)


# ------------------------------------------------------------------------------------------- 2. persistent kernels, several items each
# c64.hip (bf16 and fp16): a workgroup walks item = blockIdx.x, += gridDim.x over (image, column strip, row chunk), gridDim.x =
# min(items, plan CUs / (Cout / 64)).  The chunk planner never makes more items than workgroups while N x strips fits the grid,
# so only N x strips > grid sends a workgroup through the loop twice.  min_chunks / min_strips: what the case is there for on top.
C64_MULTI_ITEM = [
    dict(id='260x5x9.c64.res', shape=(260, 5, 9), cout=64, shuffle=0, res=True, min_chunks=1, min_strips=1),      # 260 items on 256
    dict(id='70x6x20.c256.shuffle', shape=(70, 6, 20), cout=256, shuffle=2, res=False, min_chunks=1, min_strips=1),  # 70 items on 64
    # 3 chunks x 2 strips per image, 774 items on 256 workgroups: 256 = 42 x 6 + 4, so a workgroup's next item is another image,
    # the other strip (128 + 2 columns: a ragged one) and another chunk
    dict(id='129x15x130.c64.res', shape=(129, 15, 130), cout=64, shuffle=0, res=True, min_chunks=3, min_strips=2),
]
# The per-channel-PReLU instantiations (srx_conv3x3_c64_{bf16,f16}_fwd_slopes: c64_kernel<.., PC = true>, the compact generator's
# body): each tile form <RW, CW> -- <4, 1> up to 32 pixels per row, <2, 2> up to 64, <1, 4> beyond -- one item per workgroup and
# several (multi: more items than workgroups, as above), with and without an addend, and two channel groups (Cout 128: the
# slopes 64..127 belong to group 1).
C64_SLOPES = [
    dict(id='1x37x64.c64', shape=(1, 37, 64), cout=64, res=False, form=(2, 2), multi=False),            # odd rows, the widest <2, 2> frame
    dict(id='1x40x150.c64.res', shape=(1, 40, 150), cout=64, res=True, form=(1, 4), multi=False),       # a ragged second strip
    dict(id='3x9x33.c128', shape=(3, 9, 33), cout=128, res=False, form=(2, 2), multi=False),            # two channel groups
    dict(id='260x5x9.c64.res', shape=(260, 5, 9), cout=64, res=True, form=(4, 1), multi=True),          # 260 items on 256 workgroups
    dict(id='260x6x40.c64', shape=(260, 6, 40), cout=64, res=False, form=(2, 2), multi=True),           # 260 items on 256 workgroups
    dict(id='129x15x130.c64.res', shape=(129, 15, 130), cout=64, res=True, form=(1, 4), multi=True),    # 774 items
    dict(id='130x5x9.c128', shape=(130, 5, 9), cout=128, res=False, form=(4, 1), multi=True),           # 130 items on 128 workgroups
]
C64_SLOPES_FORMS = [(4, 1), (2, 2), (1, 4)]

# thin9.hip (bf16 and fp16) has no plan query; its grid is min(items, plan CUs) and items >= N x ceil(W / 128), so
# N x ceil(W / 128) > 256 forces several items per workgroup whatever chunk height the planner takes.  (N, H, W, Cout);
# H = 5 is shorter than the 9-row window, H = 12 longer than the ring of 10 output rows.
THIN9_STRIP = 128
THIN9_MULTI_ITEM = [(260, 5, 7, 3), (260, 12, 7, 3)]
# 130 x ceil(40 / 128) = 130 strips on 256 workgroups: one item each under today's planner (its span model prefers one 12-row
# chunk per strip), so this shape is NOT a multi-item case and the host-only test does not claim it; it runs on the GPU with the others
THIN9_OTHER = [(130, 12, 40, 3)]

# ----------------------------------------------------------------------------------------------------- 3. plans under a reservation
# desc: Conv2dDesc fields (N, H, W, Cin, Cin_s, Cout, Cout_s, KH, KW, stride, pad, shuffle, act, slope, up, precision); k: reserved
# CUs; fields: what must differ from the plan with nothing reserved; plan0 / plan: the planner's answer at 0 and at k CUs reserved.
# gconv plans (srx_conv2d_plan): [BM, BN, tail split, workgroups, KS, multi]; Winograd (srx_wino_plan): [BN, channel splits,
# workgroups, tile blocks, chunks per workgroup, parts per tile of the last round]; c64: [rows per chunk, chunks, strips].
GCONV_FIELDS = {'tile': 0, 'split': 2, 'workgroups': 3, 'ks': 4}
WINO_FIELDS = {'bn': 0, 'zsplit': 1, 'workgroups': 2}


def _conv(n, h, w, cin, cout, k, prec=0, cin_s=None):
    return (n, h, w, cin, cin_s or cin, cout, cout, k, k, 1, k // 2, 0, 0, 0.0, 0, prec)


# the dense block's conv2 (esrgan/residual.py:82): 96 of the 192-strided buffer's channels -> 32
_DENSE2 = (4, 32, 32, 96, 192, 32, 32, 3, 3, 1, 1, 0, 0, 0.0, 0, 0)
# 3 -> 64, 9 x 9 with the image stored in 8-channel pixels: at Cin_s = 4 srx_conv2d_bwd_data hands the layer to the 3-channel
# kernel (thin.hip, one plan at these sizes whatever is reserved) and the K-split tail below never runs
_IMG9 = _conv(1, 96, 96, 3, 64, 9, cin_s=8)

RESERVED_GCONV = [
    dict(id='fwd.4x32x32.96of192to32.k8', which=0, desc=_DENSE2, k=8, fields=('split', 'workgroups'),
         plan0=[64, 32, 4, 256, 2, 0], plan=[64, 32, 3, 192, 2, 0]),
    dict(id='dgrad.1x96x96.3to64.9x9.k8', which=1, desc=_IMG9, k=8, fields=('split',),
         plan0=[64, 32, 7, 1008, 2, 0], plan=[64, 32, 5, 720, 2, 0]),
    dict(id='dgrad.1x96x96.3to64.9x9.k32', which=1, desc=_IMG9, k=32, fields=('split',),
         plan0=[64, 32, 7, 1008, 2, 0], plan=[64, 32, 3, 432, 2, 0]),
    dict(id='dgrad.1x96x96.3to64.9x9.k64', which=1, desc=_IMG9, k=64, fields=('split',),
         plan0=[64, 32, 7, 1008, 2, 0], plan=[64, 32, 4, 576, 2, 0]),
    dict(id='dgrad.3x40x40.64to256.k32', which=1, desc=_conv(3, 40, 40, 64, 256, 3), k=32, fields=('tile', 'workgroups'),
         plan0=[128, 64, 6, 228, 1, 0], plan=[144, 64, 6, 204, 1, 0]),
    dict(id='dgrad.3x40x40.64to256.k64', which=1, desc=_conv(3, 40, 40, 64, 256, 3), k=64, fields=('split', 'workgroups'),
         plan0=[128, 64, 6, 228, 1, 0], plan=[128, 64, 5, 190, 1, 0]),
    dict(id='dgrad.4x24x24.128to256.bf16.k64', which=1, desc=_conv(4, 24, 24, 128, 256, 3, prec=1), k=64,
         fields=('tile', 'split', 'workgroups', 'ks'), plan0=[64, 64, 3, 216, 2, 0], plan=[128, 64, 5, 180, 1, 0]),
]
# Winograd F(2x2, 3x3), forward and data gradient: 64-column workgroups with every tile's channels split three ways (and a
# workspace) become 32-column workgroups without a split (and without a workspace)
RESERVED_WINO = [
    dict(id='wino.4x24x24.256to256.k64', desc=_conv(4, 24, 24, 256, 256, 3), k=64, fields=('bn', 'zsplit', 'workgroups'),
         plan0=[64, 3, 216, 18, 3, 1], plan=[32, 1, 144, 18, 8, 1], ws0=1769472, ws=0),
]
# the bf16 / fp16 inference conv: chunk geometry of one 300 x 200 frame
RESERVED_C64 = [dict(id='c64.1x300x200.k64', shape=(1, 300, 200), cout=64, k=64, plan0=[3, 100, 2], plan=[4, 75, 2])]
# weight gradients through srx_conv2d_bwd_weight_multi (two problems): the row splits move with the CUs, and with them the
# workspace (ws0 / ws: srx_conv2d_bwd_weight_multi_ws_floats at 0 / k reserved)
RESERVED_WGRAD = [
    dict(id='wgrad.2x32x32.64to64.k32', desc=_conv(2, 32, 32, 64, 64, 3), nprob=2, k=32, ws0=960128, ws=812416),
    dict(id='wgrad.2x32x32.64to64.k64', desc=_conv(2, 32, 32, 64, 64, 3), nprob=2, k=64, ws0=960128, ws=738560),
    dict(id='wgrad.3x40x40.64to256.k8', desc=_conv(3, 40, 40, 64, 256, 3), nprob=2, k=8, ws0=2067968, ws=2954240),
]


def by_id(cases):
    return [c['id'] for c in cases]


# ------------------------------------------------------------------------------------ 4. the kernels with a 3-channel side (thin.hip)
# Plans: srx_thin_plan (which = 0 forward / 1 data gradient: [R, tiles_h, tiles_w, workgroups]; 2 weight gradient: [groups, nseg,
# segs_per_range, nranges, nslabs]; 3 first3x3_fwd_kernel: [ntiles, workgroups]).  test_thin_forms_gpu.py runs every case below.
THIN_ROWS = (3, 4, 6)      # rows per wave srx_thin_force_rows accepts besides 0; thin_fwd2_bf16_kernel exists with 3 and 6
THIN_KS = (3, 9)


def thin_out_desc(n, h, w, k, cthin=3, prec=0):
    """64 -> cthin channels: forward on thin_fwd2_kernel / thin_fwd2_bf16_kernel, weight gradient on thin_wgrad_kernel<.., -1>."""
    return (n, h, w, 64, 64, cthin, 4, k, k, 1, k // 2, 0, 0, 0.0, 0, prec)


def thin_in_desc(n, h, w, k, cthin=3, prec=0, act=0, slope=0.0):
    """cthin -> 64 channels: data gradient on thin_fwd2_kernel, weight gradient on thin_wgrad_kernel<.., +1>, forward (3 x 3) on
    first3x3_fwd_kernel."""
    return (n, h, w, cthin, 4, 64, 64, k, k, 1, k // 2, 0, act, slope, 0, prec)


def thin_fwd_forced_shapes(r):
    """(N, H, W) per forced R (tiles of 4 R rows x 32 pixels): one row and one column short of a tile; one row and one column into
    the second tile; an image shorter than the halo and three tiles wide with a ragged last one; three row tiles with a ragged
    last one under two whole column tiles."""
    return [(1, 4 * r - 1, 31), (2, 4 * r + 1, 33), (1, 2, 70), (3, 8 * r + 5, 64)]


THIN_FWD_FORCED = [(r, k, s) for r in THIN_ROWS for k in THIN_KS for s in thin_fwd_forced_shapes(r)]
# thin channel counts other than 3, one (R, K, shape) each: (cthin, R, K, (N, H, W))
THIN_FWD_CTHIN = [(1, 3, 3, (2, 13, 33)), (2, 4, 9, (2, 17, 33)), (4, 6, 3, (2, 25, 33))]
# the planner's own R = 6 (N x ceil(H / 24) x ceil(W / 32) >= 4 x plan CUs): 130 x 2 x 2 = 520 tiles >= 4 x 128; with nothing
# reserved the same shape runs R = 3.  (N, H, W), reserved CUs, plan
THIN_FWD_OWN_R6 = dict(shape=(130, 25, 33), k=128, plan=[6, 2, 2, 520], plan0=[3, 3, 2, 780])

# weight gradient: K, reserved CUs, (N, H, W), plan.  ranges = min(plan CUs x 8 / groups, nseg): 682 / 341 (9 x 9: three groups of
# kernel rows) and 2048 / 1024 (3 x 3) at 0 / 128 reserved; wave slots = 4 x nslabs, `empty` of them past the last range.
THIN_WGRAD = [
    # ranges of two segments over rows of five (72 = 4 x 16 + 8: a ragged last one): they cross row and image ends
    dict(id='k9.4x41x72', K=9, k=0, shape=(4, 41, 72), plan=[3, 820, 2, 410, 103], empty=2),
    dict(id='k9.3x41x40.r128', K=9, k=128, shape=(3, 41, 40), plan=[3, 369, 2, 185, 47], empty=3),   # last range: one segment
    dict(id='k3.6x41x72.r128', K=3, k=128, shape=(6, 41, 72), plan=[1, 1230, 2, 615, 154], empty=1),
    # three segments per range, 820 = 273 x 3 + 1
    dict(id='k9.4x41x72.r128', K=9, k=128, shape=(4, 41, 72), plan=[3, 820, 3, 274, 69], empty=2),
    # one segment per range; slab counts on both sides of the reduction's 4-way (r < slabs) and 16-way (r + 12 < slabs) loops
    dict(id='k3.1x12x7', K=3, k=0, shape=(1, 12, 7), plan=[1, 12, 1, 12, 3], empty=0),
    dict(id='k9.2x8x16', K=9, k=0, shape=(2, 8, 16), plan=[3, 16, 1, 16, 4], empty=0),
    dict(id='k3.1x17x9', K=3, k=0, shape=(1, 17, 9), plan=[1, 17, 1, 17, 5], empty=3),
    dict(id='k9.3x10x20', K=9, k=0, shape=(3, 10, 20), plan=[3, 60, 1, 60, 15], empty=0),
    dict(id='k3.2x16x23', K=3, k=0, shape=(2, 16, 23), plan=[1, 64, 1, 64, 16], empty=0),
    dict(id='k9.1x13x70', K=9, k=0, shape=(1, 13, 70), plan=[3, 65, 1, 65, 17], empty=3),
    dict(id='k3.1x1x5', K=3, k=0, shape=(1, 1, 5), plan=[1, 1, 1, 1, 1], empty=3),
    dict(id='k9.1x1x5', K=9, k=0, shape=(1, 1, 5), plan=[3, 1, 1, 1, 1], empty=3),
    dict(id='k3.2x3x16', K=3, k=0, shape=(2, 3, 16), plan=[1, 6, 1, 6, 2], empty=2),
    dict(id='k9.2x3x16', K=9, k=0, shape=(2, 3, 16), plan=[3, 6, 1, 6, 2], empty=2),
]
# thin channel counts other than 3 on the weight gradient, each at 3 x 3 and at 9 x 9, thin side in and out: (cthin, case id)
THIN_WGRAD_CTHIN = [(1, 'k3.1x17x9'), (2, 'k9.2x8x16'), (4, 'k3.2x16x23'), (4, 'k9.3x10x20')]

# first3x3_fwd_kernel: tiles of 32 pixels, min(ceil(ntiles / 4), 3 x plan CUs) workgroups of four waves.  (N, H, W), reserved, plan
THIN_FIRST3 = [
    # M = 49 500 = 1546 x 32 + 28: 1547 tiles on 384 x 4 = 1536 waves -- eleven waves walk a second tile, the last tile is ragged
    dict(id='5x100x99.r128', shape=(5, 100, 99), k=128, plan=[1547, 384], multi=True),
    dict(id='1x3x5', shape=(1, 3, 5), k=0, plan=[1, 1], multi=False),      # M = 15 < 32
    dict(id='2x7x1', shape=(2, 7, 1), k=0, plan=[1, 1], multi=False),      # one pixel per row: every tap to the left and right is padding
]
