"""Every launch form of nn.Linear (csrc/linear.hip): the plain kernels linear_*_kernel<NB> and the fast ones
linear_*_fast_kernel<NB> (raw buffer loads, double-buffered trips), chosen per 64-row launch by linear_fast_ok and NB <= 2, here
forced through srx_linear_force and held to the form by srx_linear_plan.

Data only.  test_linear_forms_cpu.py holds every case to the plan written next to it (host code: no GPU; a planner change that
makes a case vacuous fails there) and checks that the table as a whole still covers what section "coverage" of that file lists;
test_linear_forms_gpu.py runs the three passes of every case against fp64.

A case: (id, B, K, J, form, splits, act, bias, why) -- form / splits are the arguments of srx_linear_force (0 = the model's
choice, 1 plain, 2 fast); act / bias the forward's epilogue (0 none, 1 ReLU, 2 LeakyReLU 0.2).  PLANS[id] = the answer of
srx_linear_plan for (forward, data gradient, weight gradient) under that forcing: [splits launched, elements per split, 64-row
launches, NB of the last launch (weight gradient: batch trips of 32 rows), form of the first launch, form of the last], or None
where the forced pass is refused (SRX_E_UNSUPPORTED) -- the GPU test runs the passes that have a plan.

Shapes are the smallest that reach each form: a fast forward wave makes trips of 256 k over its split (the four waves interleave
64-wide slices), a data-gradient wave trips of 16 j, the weight gradient trips of 32 rows.  The activations sit on cases with
K <= 1088 only: an output whose fp64 pre-activation is within its own error bound of 0 may land on either side of the kink and is
compared before the activation instead, and the test keeps those under 1 % of a tensor; with unit-variance outputs and the bound
gamma(K) sum|x||w| ~ 0.64 K^1.5 2^-24 that is 0.1 % of the elements at K = 1024 but 2 % at 8192 and 8 % at 18432, whatever the seed.
"""

SLOPE = 0.2
CASES = []


def _case(cid, b, k, j, form, splits, act, bias, why):
    CASES.append((cid, b, k, j, form, splits, act, bias, why))


def _pair(name, b, k, j, splits, act, bias, why, forms=(1, 2)):
    """the same shape under two forcings: the GPU test holds the second to the first bitwise"""
    for f in forms:
        _case('%s.%s' % (name, {0: 'model', 1: 'plain', 2: 'fast'}[f]), b, k, j, f, splits, act, bias, why)


# ---------------------------------------------------------------------------------------------------------------------- rows
# K = 256 (one trip of wave 0..3), J = 16 (one tile).  B <= 32 runs either form; above, a 64-row launch of the forward / data
# gradient with NB > 2 is plain whatever is forced (form 2 is refused there: test_linear_forms_cpu.py), so the second forcing is
# the model's: plain <3> / <4> launches, a fast last launch where NB <= 2, and the fast weight gradient over the whole batch.
for _b, _why in [(1, 'NB = 1, one row'), (3, 'NB = 1, ragged'), (16, 'NB = 1, whole'), (17, 'NB = 2, one row in the second block'),
                 (24, 'NB = 2, ragged second block'), (31, 'NB = 2, one row short'), (32, 'NB = 2, whole; one whole batch trip')]:
    _pair('rows%d' % _b, _b, 256, 16, 0, _b % 3, _b % 2, _why)
for _b, _why in [(33, 'plain <3>; two batch trips, one row in the second'), (64, 'plain <4>; two whole batch trips'),
                 (70, 'plain <4> then fast <1> with 6 rows; three batch trips'), (81, 'plain <4> then fast <2> with 17 rows'),
                 (112, 'two plain launches <4>, <3>; four batch trips, the last of 16 rows')]:
    _pair('rows%d' % _b, _b, 256, 16, 0, _b % 3, _b % 2, _why, forms=(1, 0))

# ------------------------------------------------------------------------------------------------------------------------- K
# B = 17 (NB = 2 with a ragged block), J = 64 (four tiles; up to four j splits of one trip)
for _k in (20, 68, 260):
    _case('k%d.plain' % _k, 17, _k, 64, 1, 0, _k % 3, _k % 2, 'K no multiple of 64: plain only, a partial 64-wide slice')
_pair('k64', 17, 64, 64, 0, 1, 1, 'one 64-wide slice: waves 1..3 never enter the trip loop')
_pair('k320', 17, 320, 64, 0, 2, 0, 'two splits, the last one 64-wide slice')
_pair('k1088', 17, 1088, 64, 0, 0, 1, 'five splits, the last one 64-wide slice')
_pair('k256.s1', 17, 256, 64, 1, 1, 0, 'one trip per wave: leaves the two-set loop at its first exit')
_pair('k512.s1', 17, 512, 64, 1, 2, 1, 'two trips per wave: the second exit')
_pair('k768.s1', 17, 768, 64, 1, 0, 0, 'three trips per wave: the first exit after a whole round')
_pair('k1024.s4', 17, 1024, 64, 4, 1, 1, 'four forced splits of one trip; four j splits of one trip')
_pair('k1024', 17, 1024, 64, 0, 2, 0, "the model's splits")

# ------------------------------------------------------------------------------------------------------------------------- J
# B = 17, K = 256.  J no multiple of 16: the fast forward reads weight rows past J as zeros (the last tile is ragged); the two
# gradients have no fast form there and forcing one is refused.
for _j in (1, 5, 40, 100):
    _pair('j%d' % _j, 17, 256, _j, 0, _j % 3, (_j + 1) % 2, 'ragged last j tile in the forward; gradients plain only')
_pair('j16', 17, 256, 16, 0, 0, 0, 'one j trip of the data gradient')
_pair('j48', 17, 256, 48, 0, 1, 1, 'one split of three j trips')
_pair('j80', 17, 256, 80, 0, 2, 0, 'jper = 48: splits of three and of two j trips')
_pair('j144', 17, 256, 144, 0, 0, 1, 'three splits of three j trips')
_pair('j32.s1', 17, 256, 32, 1, 1, 0, 'two j trips in one split')
_pair('j64.s1', 17, 256, 64, 1, 2, 1, 'four j trips in one split')

# ---------------------------------------------------------------------------------------------------------- the product shapes
# SRGAN's classifier at batch 16 and at the discriminator update's real + fake 32 (75.5 MB of weight), ESRGAN's at 32
PRODUCT = [(16, 18432, 1024), (32, 18432, 1024), (32, 8192, 100)]
for _b, _k, _j in PRODUCT:
    _pair('product%dx%dx%d' % (_b, _k, _j), _b, _k, _j, 0, 0, 1, 'a shape the train steps run')

# what srx_linear_plan answers: (forward, data gradient, weight gradient)
PLANS = {
    'rows1.plain': ([1, 256, 1, 1, 1, 1], [1, 16, 1, 1, 1, 1], [1, 0, 1, 1, 1, 1]),
    'rows1.fast': ([1, 256, 1, 1, 2, 2], [1, 16, 1, 1, 2, 2], [1, 0, 1, 1, 2, 2]),
    'rows3.plain': ([1, 256, 1, 1, 1, 1], [1, 16, 1, 1, 1, 1], [1, 0, 1, 1, 1, 1]),
    'rows3.fast': ([1, 256, 1, 1, 2, 2], [1, 16, 1, 1, 2, 2], [1, 0, 1, 1, 2, 2]),
    'rows16.plain': ([1, 256, 1, 1, 1, 1], [1, 16, 1, 1, 1, 1], [1, 0, 1, 1, 1, 1]),
    'rows16.fast': ([1, 256, 1, 1, 2, 2], [1, 16, 1, 1, 2, 2], [1, 0, 1, 1, 2, 2]),
    'rows17.plain': ([1, 256, 1, 2, 1, 1], [1, 16, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'rows17.fast': ([1, 256, 1, 2, 2, 2], [1, 16, 1, 2, 2, 2], [1, 0, 1, 1, 2, 2]),
    'rows24.plain': ([1, 256, 1, 2, 1, 1], [1, 16, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'rows24.fast': ([1, 256, 1, 2, 2, 2], [1, 16, 1, 2, 2, 2], [1, 0, 1, 1, 2, 2]),
    'rows31.plain': ([1, 256, 1, 2, 1, 1], [1, 16, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'rows31.fast': ([1, 256, 1, 2, 2, 2], [1, 16, 1, 2, 2, 2], [1, 0, 1, 1, 2, 2]),
    'rows32.plain': ([1, 256, 1, 2, 1, 1], [1, 16, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'rows32.fast': ([1, 256, 1, 2, 2, 2], [1, 16, 1, 2, 2, 2], [1, 0, 1, 1, 2, 2]),
    'rows33.plain': ([1, 256, 1, 3, 1, 1], [1, 16, 1, 3, 1, 1], [1, 0, 1, 2, 1, 1]),
    'rows33.model': ([1, 256, 1, 3, 1, 1], [1, 16, 1, 3, 1, 1], [1, 0, 1, 2, 2, 2]),
    'rows64.plain': ([1, 256, 1, 4, 1, 1], [1, 16, 1, 4, 1, 1], [1, 0, 1, 2, 1, 1]),
    'rows64.model': ([1, 256, 1, 4, 1, 1], [1, 16, 1, 4, 1, 1], [1, 0, 1, 2, 2, 2]),
    'rows70.plain': ([1, 256, 2, 1, 1, 1], [1, 16, 2, 1, 1, 1], [1, 0, 1, 3, 1, 1]),
    'rows70.model': ([1, 256, 2, 1, 1, 2], [1, 16, 2, 1, 1, 2], [1, 0, 1, 3, 2, 2]),
    'rows81.plain': ([1, 256, 2, 2, 1, 1], [1, 16, 2, 2, 1, 1], [1, 0, 1, 3, 1, 1]),
    'rows81.model': ([1, 256, 2, 2, 1, 2], [1, 16, 2, 2, 1, 2], [1, 0, 1, 3, 2, 2]),
    'rows112.plain': ([1, 256, 2, 3, 1, 1], [1, 16, 2, 3, 1, 1], [1, 0, 1, 4, 1, 1]),
    'rows112.model': ([1, 256, 2, 3, 1, 1], [1, 16, 2, 3, 1, 1], [1, 0, 1, 4, 2, 2]),
    'k20.plain': ([1, 256, 1, 2, 1, 1], [1, 64, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'k68.plain': ([1, 256, 1, 2, 1, 1], [1, 64, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'k260.plain': ([2, 256, 1, 2, 1, 1], [1, 64, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'k64.plain': ([1, 256, 1, 2, 1, 1], [1, 64, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'k64.fast': ([1, 256, 1, 2, 2, 2], [1, 64, 1, 2, 2, 2], [1, 0, 1, 1, 2, 2]),
    'k320.plain': ([2, 256, 1, 2, 1, 1], [1, 64, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'k320.fast': ([2, 256, 1, 2, 2, 2], [1, 64, 1, 2, 2, 2], [1, 0, 1, 1, 2, 2]),
    'k1088.plain': ([5, 256, 1, 2, 1, 1], [1, 64, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'k1088.fast': ([5, 256, 1, 2, 2, 2], [1, 64, 1, 2, 2, 2], [1, 0, 1, 1, 2, 2]),
    'k256.s1.plain': ([1, 256, 1, 2, 1, 1], [1, 64, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'k256.s1.fast': ([1, 256, 1, 2, 2, 2], [1, 64, 1, 2, 2, 2], [1, 0, 1, 1, 2, 2]),
    'k512.s1.plain': ([1, 512, 1, 2, 1, 1], [1, 64, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'k512.s1.fast': ([1, 512, 1, 2, 2, 2], [1, 64, 1, 2, 2, 2], [1, 0, 1, 1, 2, 2]),
    'k768.s1.plain': ([1, 768, 1, 2, 1, 1], [1, 64, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'k768.s1.fast': ([1, 768, 1, 2, 2, 2], [1, 64, 1, 2, 2, 2], [1, 0, 1, 1, 2, 2]),
    'k1024.s4.plain': ([4, 256, 1, 2, 1, 1], [4, 16, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'k1024.s4.fast': ([4, 256, 1, 2, 2, 2], [4, 16, 1, 2, 2, 2], [1, 0, 1, 1, 2, 2]),
    'k1024.plain': ([4, 256, 1, 2, 1, 1], [1, 64, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'k1024.fast': ([4, 256, 1, 2, 2, 2], [1, 64, 1, 2, 2, 2], [1, 0, 1, 1, 2, 2]),
    'j1.plain': ([1, 256, 1, 2, 1, 1], [1, 16, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'j1.fast': ([1, 256, 1, 2, 2, 2], None, None),
    'j5.plain': ([1, 256, 1, 2, 1, 1], [1, 16, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'j5.fast': ([1, 256, 1, 2, 2, 2], None, None),
    'j40.plain': ([1, 256, 1, 2, 1, 1], [1, 48, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'j40.fast': ([1, 256, 1, 2, 2, 2], None, None),
    'j100.plain': ([1, 256, 1, 2, 1, 1], [2, 64, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'j100.fast': ([1, 256, 1, 2, 2, 2], None, None),
    'j16.plain': ([1, 256, 1, 2, 1, 1], [1, 16, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'j16.fast': ([1, 256, 1, 2, 2, 2], [1, 16, 1, 2, 2, 2], [1, 0, 1, 1, 2, 2]),
    'j48.plain': ([1, 256, 1, 2, 1, 1], [1, 48, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'j48.fast': ([1, 256, 1, 2, 2, 2], [1, 48, 1, 2, 2, 2], [1, 0, 1, 1, 2, 2]),
    'j80.plain': ([1, 256, 1, 2, 1, 1], [2, 48, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'j80.fast': ([1, 256, 1, 2, 2, 2], [2, 48, 1, 2, 2, 2], [1, 0, 1, 1, 2, 2]),
    'j144.plain': ([1, 256, 1, 2, 1, 1], [3, 48, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'j144.fast': ([1, 256, 1, 2, 2, 2], [3, 48, 1, 2, 2, 2], [1, 0, 1, 1, 2, 2]),
    'j32.s1.plain': ([1, 256, 1, 2, 1, 1], [1, 32, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'j32.s1.fast': ([1, 256, 1, 2, 2, 2], [1, 32, 1, 2, 2, 2], [1, 0, 1, 1, 2, 2]),
    'j64.s1.plain': ([1, 256, 1, 2, 1, 1], [1, 64, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'j64.s1.fast': ([1, 256, 1, 2, 2, 2], [1, 64, 1, 2, 2, 2], [1, 0, 1, 1, 2, 2]),
    'product16x18432x1024.plain': ([15, 1280, 1, 1, 1, 1], [13, 80, 1, 1, 1, 1], [1, 0, 1, 1, 1, 1]),
    'product16x18432x1024.fast': ([15, 1280, 1, 1, 2, 2], [13, 80, 1, 1, 2, 2], [1, 0, 1, 1, 2, 2]),
    'product32x18432x1024.plain': ([15, 1280, 1, 2, 1, 1], [13, 80, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'product32x18432x1024.fast': ([15, 1280, 1, 2, 2, 2], [13, 80, 1, 2, 2, 2], [1, 0, 1, 1, 2, 2]),
    'product32x8192x100.plain': ([32, 256, 1, 2, 1, 1], [2, 64, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]),
    'product32x8192x100.fast': ([32, 256, 1, 2, 2, 2], None, None),
}

IDS = [c[0] for c in CASES]
