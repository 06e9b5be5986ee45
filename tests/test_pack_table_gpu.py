"""The one-launch weight repack (``pack_table_kernel``: ``srx_pack_table_build`` / ``_add_wino`` / ``_run``, csrc/convpack.hip)
against the per-layer packers (``srx_conv2d_pack``: ``pack_all_kernel`` and thin.hip's ``thin_pack_kernel``; ``srx_wino_pack``:
``wino_pack_kernel``), bit for bit, and the dense-block weight streams (``srx_rdb_pack`` / ``srx_rdb_pack_bwd``) of several
blocks against one-block packs.

Which side is the yardstick.  The per-layer packs are what every kernel-level conv test reads its weights through
(test_ops_gpu.py, test_forced_paths_gpu.py, test_plan_forms_gpu.py, test_thin_forms_gpu.py, test_wino_gpu.py,
test_esrgan_layers_gpu.py): those tests compare conv outputs and data gradients with fp64, so a wrong per-layer layout fails
there.  The table kernel restates every one of those layouts with its own indexing and its own launch geometry, and the
trainers read ITS output from the second step on; nothing else compares what it writes.  Here the table's bytes must equal
the per-layer pack's.  Two things are checked on the per-layer side itself: with weights 1, 2, 3, ... every packed buffer
holds each weight exactly once and zeros elsewhere, and the Winograd-domain weights are held to an fp64 ``G g G^T`` within a
derived bound.

Conventions.  Element i of an OIHW weight is the fp32 value i + 1 (exact and distinct below 2^24): a misplaced element never
equals the right one, and 0 means padding.  Every other case reads its weight one float into a 16-byte aligned allocation, as
a slice of a flat parameter buffer may lie.  Destinations live in one arena between guard gaps of at least 64 floats and every
comparison runs under two prefills, NaN and -7.0: what both packers leave unwritten shows as a difference BETWEEN the
prefills, so each buffer must come out the same under both -- over every float the library sizes it for.  The one exception
is known and stated: thin.hip's ``p[c][tap][ch]`` layout is 4 x taps x 64 floats at the head of a buffer that
``srx_conv2d_packed_*_floats`` sizes for the generic layout; both packers write that head and the thin kernels read nothing
behind it, so for the thin side of a 3-channel layer the head must agree under both prefills and the rest must keep its
prefill under both packers.  Guards keep their prefill bit for bit.  All comparisons are ``torch.equal`` on int32 views.
"""
import contextlib
import ctypes as C
import sys

import numpy as np
import pytest
import torch

import pack_cases as PC

pytestmark = pytest.mark.gpu

GUARD = 64
PREFILLS = (float('nan'), -7.0)


def bits(t):
    return t.view(torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Arena:
    """Destinations of the given sizes (floats) in ONE buffer, at least GUARD floats before, between and behind them."""

    def __init__(self, sizes, prefill, dev):
        offs, off = [], GUARD
        for n in sizes:
            offs.append(off)
            off = (off + n + 3) // 4 * 4 + GUARD
        self.prefill = prefill
        self.buf = torch.full((off,), prefill, dtype=torch.float32, device=dev)
        self.views = [self.buf[o:o + n] for o, n in zip(offs, sizes)]
        self.guard = torch.ones(off, dtype=torch.bool, device=dev)
        for o, n in zip(offs, sizes):
            self.guard[o:o + n] = False
        assert int(self.guard.sum()) >= GUARD * (len(sizes) + 1)

    def kept_prefill(self, t):
        want = bits(torch.tensor([self.prefill], dtype=torch.float32)).item()
        return bool((bits(t) == want).all())

    def guards_intact(self):
        return self.kept_prefill(self.buf[self.guard])


def int_weight(numel, offset, dev, first=1):
    """fp32 values first, first + 1, ... starting ``offset`` floats into a 16-byte aligned allocation."""
    buf = torch.empty(numel + 4, dtype=torch.float32, device=dev)
    w = buf[offset:offset + numel]
    w.copy_(torch.arange(first, first + numel, dtype=torch.float32, device=dev))
    assert w.data_ptr() % 16 == 4 * offset and first + numel < 1 << 24
    return w


def case_weight(c, dev):
    return int_weight(c['cout'] * c['cin'] * c['k'] ** 2, c['w_offset'], dev)


def case_desc(c):
    from torchsr_amd import _lib
    return _lib.Conv2dDesc(*PC.desc_fields(c))


def case_sizes(d):
    from torchsr_amd import _lib
    L = _lib.lib()
    nf, nb = L.srx_conv2d_packed_fwd_floats(C.byref(d)), L.srx_conv2d_packed_bwd_floats(C.byref(d))
    assert nf > 0 and nb > 0, _lib.last_error()
    return nf, nb


def written_floats(c, nf, nb, bwd):
    """Floats of the forward / backward buffer a packer writes: all of them, or the head that is thin.hip's layout (see the
    module docstring), or none of a backward buffer that was not asked for."""
    thin = 4 * c['k'] ** 2 * 64
    assert not c['thin'] or thin < min(nf, nb)
    return (thin if c['thin'] == 'fwd' else nf), (0 if not bwd else thin if c['thin'] == 'dgrad' else nb)


def build_table(layers, winos=()):
    """The host table over ``layers`` = [(desc, weight, fwd, bwd or None)] and ``winos`` = [(desc, weight, upk, transpose)], sized as
    functional.PackTable sizes it: (table, nrec, max_elems)."""
    from torchsr_amd import _lib
    L = _lib.lib()
    n = len(layers)
    n_wino_layers = len({id(w[0]) for w in winos})
    nbytes = L.srx_pack_table_bytes(n + n_wino_layers)
    rec = L.srx_pack_table_bytes(1) // 17
    assert nbytes == (n + n_wino_layers) * 17 * rec and nbytes >= (17 * n + len(winos)) * rec
    host = torch.zeros(nbytes, dtype=torch.uint8)
    nrec, maxn = C.c_int(0), C.c_longlong(0)
    if n:
        descs = (_lib.Conv2dDesc * n)(*[la[0] for la in layers])
        arr = lambda ptrs: (C.c_void_p * n)(*ptrs)  # noqa: E731
        _lib.call('srx_pack_table_build', descs, n, arr([la[1].data_ptr() for la in layers]), arr([la[2].data_ptr() for la in layers]),
                  arr([None if la[3] is None else la[3].data_ptr() for la in layers]), host.data_ptr(), C.byref(nrec), C.byref(maxn))
    for d, w, upk, transpose in winos:
        _lib.call('srx_pack_table_add_wino', host.data_ptr(), C.byref(nrec), C.byref(maxn), C.byref(d), w.data_ptr(), upk.data_ptr(), transpose)
    assert 0 < nrec.value <= 17 * n + len(winos)
    return host, nrec.value, maxn.value


def pack_table(dev, layers, winos=()):
    """``build_table``, the table copied to the device and run once: (nrec, max_elems)."""
    from torchsr_amd import _lib
    host, nrec, maxn = build_table(layers, winos)
    table = host.to(dev)
    _lib.call('srx_pack_table_run', table.data_ptr(), nrec, maxn, _stream())
    torch.cuda.synchronize()
    return nrec, maxn


def pack_layer(d, w, fwd, bwd):
    from torchsr_amd import _lib
    _lib.call('srx_conv2d_pack', C.byref(d), w.data_ptr(), fwd.data_ptr(), None if bwd is None else bwd.data_ptr(), _stream())


def holds_each_weight_once(packed, numel):
    """With weights 1 .. numel: the non-zero entries of a packed buffer are those values, each once."""
    nz = packed[packed != 0]
    return nz.numel() == numel and torch.equal(nz.sort().values, torch.arange(1, numel + 1, dtype=torch.float32, device=packed.device))


def check_layer(c, w, per_layer, table, bwd):
    """``per_layer`` / ``table``: {prefill: (arena, fwd view, bwd view)} of one layer packed either way."""
    nf, nb = per_layer[PREFILLS[0]][1].numel(), per_layer[PREFILLS[0]][2].numel()
    wf, wb = written_floats(c, nf, nb, bwd)
    for p in PREFILLS:
        (_, af, ab), (_, bf, bb) = per_layer[p], table[p]
        assert same(af, bf), (c['id'], 'forward', p)
        assert same(ab, bb), (c['id'], 'backward', p)
    for name, packs in (('per-layer', per_layer), ('table', table)):
        (a0, f0, b0), (a1, f1, b1) = packs[PREFILLS[0]], packs[PREFILLS[1]]
        # written where it must be: the same under both prefills ...
        assert same(f0[:wf], f1[:wf]) and same(b0[:wb], b1[:wb]), (c['id'], name)
        # ... and nothing behind a thin layout's head, nothing at all in a backward buffer that was not asked for
        assert a0.kept_prefill(f0[wf:]) and a1.kept_prefill(f1[wf:]) and a0.kept_prefill(b0[wb:]) and a1.kept_prefill(b1[wb:]), (c['id'], name)
    _, f, b = per_layer[PREFILLS[0]]
    assert holds_each_weight_once(f[:wf], w.numel()), c['id']
    assert wb == 0 or holds_each_weight_once(b[:wb], w.numel()), c['id']


# ------------------------------------------------------------------------------------------------ 1. one record table per layer
@pytest.mark.parametrize('case', PC.CASES, ids=PC.by_id(PC.CASES))
def test_single_layer_table_equals_the_per_layer_pack(dev, case):
    d = case_desc(case)
    nf, nb = case_sizes(d)
    w = case_weight(case, dev)
    per_layer, table = {}, {}
    for p in PREFILLS:
        a, b = Arena([nf, nb], p, dev), Arena([nf, nb], p, dev)
        pack_layer(d, w, a.views[0], a.views[1] if case['bwd'] else None)
        nrec, maxn = pack_table(dev, [(d, w, b.views[0], b.views[1] if case['bwd'] else None)])
        assert nrec == PC.predicted_nrec(case) and maxn > 0
        assert a.guards_intact() and b.guards_intact(), (case['id'], p)
        per_layer[p], table[p] = (a, *a.views), (b, *b.views)
    check_layer(case, w, per_layer, table, case['bwd'])


# ------------------------------------------------------------------------------------------------ 3. Winograd records
def wino_desc(c):
    from torchsr_amd import _lib
    d = _lib.Conv2dDesc(*PC.wino_desc_fields(c))
    n = _lib.lib().srx_wino_packed_floats(C.byref(d))
    assert n > 0
    return d, n


def wino_weight(c, dev, seed=3):
    """Random normal weights (the fp64 comparison wants rounding errors, not small integers), one float off alignment."""
    g = torch.Generator().manual_seed(seed + c['cin'] + c['cout'])
    host = torch.randn(c['cout'], c['cin'], 3, 3, generator=g)
    buf = torch.empty(host.numel() + 4, dtype=torch.float32, device=dev)
    w = buf[1:1 + host.numel()]
    w.copy_(host.reshape(-1).to(dev))
    assert w.data_ptr() % 16 == 4
    return host, w


GAMMA4 = 4 * 2.0 ** -24 / (1 - 4 * 2.0 ** -24)
G = np.array([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]])


def wino_reference(w32, mode):
    """(U, bound) in the packed order: U = G g G^T in float64 of the fp32 weights, placed by ``srx_wino_pack_one``'s index formula
    (csrc/srx_common.h) restated here.  mode 1 (the data gradient): channels swapped, taps flipped; mode 2 (PixelShuffle store):
    row r reads output channel (r % (Cout / 4)) * 4 + r / (Cout / 4).  bound = gamma_4 |G| |g| |G|^T: every entry is a sum of
    products of g by entries of G that are 0, 1 or +-0.5 -- exact -- and passes through at most four fp32 additions."""
    w = w32.astype(np.float64)
    cout = w.shape[0]
    if mode == 1:
        g = w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]
    elif mode == 2:
        r = np.arange(cout)
        g = w[(r % (cout // 4)) * 4 + r // (cout // 4)]
    else:
        g = w
    R, K = g.shape[:2]
    u = np.einsum('ia,rkab,jb->rkij', G, g, G)
    bound = GAMMA4 * np.einsum('ia,rkab,jb->rkij', np.abs(G), np.abs(g), np.abs(G))
    r = np.arange(R).reshape(R, 1, 1, 1)
    k = np.arange(K).reshape(1, K, 1, 1)
    xi = 4 * np.arange(4).reshape(1, 1, 4, 1) + np.arange(4).reshape(1, 1, 1, 4)
    jg, mrow, kc, kk = r >> 5, r & 31, k // 32, k % 32
    quad, e = kk >> 2, kk & 3
    s, hh = quad >> 1, quad & 1
    idx = np.broadcast_to((((((xi * (R // 32) + jg) * (K // 32) + kc) * 4 + s) * 64 + hh * 32 + mrow) * 4 + e), u.shape).ravel()
    assert np.unique(idx).size == 16 * R * K and idx.min() == 0 and idx.max() == 16 * R * K - 1   # a permutation of the buffer
    out, bnd = np.empty(16 * R * K), np.empty(16 * R * K)
    out[idx], bnd[idx] = u.ravel(), bound.ravel()
    return out, bnd


@pytest.mark.parametrize('case', PC.WINO_CASES, ids=PC.by_id(PC.WINO_CASES))
def test_winograd_records_equal_wino_pack_and_fp64(dev, case):
    from torchsr_amd import _lib
    d, n = wino_desc(case)
    host, w = wino_weight(case, dev)
    records = PC.wino_records(case)
    assert [k for _, k in records] == ([6] if case['shuffle'] else [4, 5])
    packs = {}
    for p in PREFILLS:
        a, b = Arena([n] * len(records), p, dev), Arena([n] * len(records), p, dev)
        for (transpose, _), upk in zip(records, a.views):
            _lib.call('srx_wino_pack', C.byref(d), w.data_ptr(), upk.data_ptr(), transpose, _stream())
        nrec, maxn = pack_table(dev, [], [(d, w, upk, transpose) for (transpose, _), upk in zip(records, b.views)])
        assert nrec == len(records) and maxn == case['cin'] * case['cout']
        assert a.guards_intact() and b.guards_intact()
        assert same(a.buf, b.buf), (case['id'], p)
        packs[p] = (a, b)
    for i in range(len(records)):      # every float written: the same under both prefills
        assert same(packs[PREFILLS[0]][0].views[i], packs[PREFILLS[1]][0].views[i])
        assert same(packs[PREFILLS[0]][1].views[i], packs[PREFILLS[1]][1].views[i])
    worst = 0.0
    for i, (transpose, kind) in enumerate(records):
        want, bound = wino_reference(host.numpy(), 1 if transpose else (2 if case['shuffle'] else 0))
        assert (bound > 0).all()
        for name, arena in zip(('srx_wino_pack', 'table'), packs[PREFILLS[0]]):
            err = np.abs(arena.views[i].cpu().numpy().astype(np.float64) - want)
            ratio = float((err / bound).max())
            print(f'{case["id"]} kind {kind} {name}: worst error / bound {ratio:.3f}')
            worst = max(worst, ratio)
            assert (err <= bound).all(), (case['id'], kind, name, ratio)
    print(f'{case["id"]}: worst error / bound {worst:.3f}')


# ------------------------------------------------------------------------------------------------ 2. one table for all of them
def test_one_table_for_every_layer(dev):
    """Every layer of the list and the Winograd records of WINO_CASES behind them in ONE table and one launch.  The launch is
    as wide as the largest record (a 512 -> 512 layer's, in the middle of the table), so every other record's surplus threads
    leave on ``idx >= n_elems``; three layers in the middle have no backward destination."""
    from torchsr_amd import _lib
    descs = [case_desc(c) for c in PC.CASES]
    sizes = [case_sizes(d) for d in descs]
    weights = [case_weight(c, dev) for c in PC.CASES]
    with_bwd = [c['bwd'] and c['id'] not in PC.TABLE_FWD_ONLY for c in PC.CASES]
    assert with_bwd.count(False) == len(PC.TABLE_FWD_ONLY) + 1
    wino = [(c, *wino_desc(c), wino_weight(c, dev)[1]) for c in PC.WINO_CASES]
    wino_recs = [(d, n, w, transpose) for c, d, n, w in wino for transpose, _ in PC.wino_records(c)]
    flat = [n for nf, nb in sizes for n in (nf, nb)] + [n for _, n, _, _ in wino_recs]
    wv = 2 * len(sizes)      # the arena's views: forward and backward buffer of every layer, then the Winograd records'

    def layers_into(arena):
        return [(d, w, arena.views[2 * i], arena.views[2 * i + 1] if with_bwd[i] else None) for i, (d, w) in enumerate(zip(descs, weights))]

    def winos_into(arena):
        return [(d, w, arena.views[wv + j], transpose) for j, (d, n, w, transpose) in enumerate(wino_recs)]

    per_layer, table = {}, {}
    for p in PREFILLS:
        a, b = Arena(flat, p, dev), Arena(flat, p, dev)
        for d, w, fwd, bwd in layers_into(a):
            pack_layer(d, w, fwd, bwd)
        for d, w, upk, transpose in winos_into(a):
            _lib.call('srx_wino_pack', C.byref(d), w.data_ptr(), upk.data_ptr(), transpose, _stream())
        nrec, maxn = pack_table(dev, layers_into(b), winos_into(b))
        # what test_pack_table_cpu.py predicts: the counts add up, the width is the widest record's -- each layer's from a
        # host build of its own, a Winograd record's one work item per channel pair
        alone = [build_table([la]) for la in layers_into(b)] + [build_table([], [wi]) for wi in winos_into(b)]
        assert nrec == sum(PC.predicted_nrec(c, f) for c, f in zip(PC.CASES, with_bwd)) + len(wino_recs) == sum(t[1] for t in alone)
        assert maxn == max(t[2] for t in alone) and maxn == alone[PC.by_id(PC.CASES).index('c512.s2')][2]
        assert all(t[2] == d.Cin * d.Cout for t, (d, _, _, _) in zip(alone[len(descs):], wino_recs))
        assert nrec <= 17 * len(PC.CASES) + len(wino_recs)
        assert a.guards_intact() and b.guards_intact(), p
        assert same(a.buf, b.buf), p                    # every destination and every gap in one comparison
        per_layer[p], table[p] = a, b
    for i, (c, w) in enumerate(zip(PC.CASES, weights)):
        pick = lambda arenas: {p: (arenas[p], arenas[p].views[2 * i], arenas[p].views[2 * i + 1]) for p in PREFILLS}  # noqa: E731
        check_layer(c, w, pick(per_layer), pick(table), with_bwd[i])
    for j in range(len(wino_recs)):                     # the Winograd records write every float of theirs
        assert same(table[PREFILLS[0]].views[wv + j], table[PREFILLS[1]].views[wv + j])
        assert same(per_layer[PREFILLS[0]].views[wv + j], per_layer[PREFILLS[1]].views[wv + j])


# ------------------------------------------------------------------------------------------------ 4. PackTable as the trainers use it
@contextlib.contextmanager
def recorded_calls(monkeypatch):
    """Names of every ``_lib.call`` made inside the block, through every module-level alias of it in the package (the method of
    step_layers.record_op_calls, which leaves the conv family out)."""
    from torchsr_amd import _lib
    import torchsr_amd.esrgan.trainer  # noqa: F401  (every module that binds `call` is loaded BEFORE the patch)
    import torchsr_amd.srgan.trainer  # noqa: F401
    import torchsr_amd.functional  # noqa: F401
    import torchsr_amd.optim  # noqa: F401
    real = _lib.call
    names = []

    def spy(name, *args):
        names.append(name)
        return real(name, *args)

    for mod_name, mod in list(sys.modules.items()):
        if mod is None or not (mod_name == 'torchsr_amd' or mod_name.startswith('torchsr_amd.')):
            continue
        for attr, val in list(vars(mod).items()):
            if val is real:
                monkeypatch.setattr(mod, attr, spy)
    try:
        yield names
        torch.cuda.synchronize()
    finally:
        monkeypatch.undo()


def test_pack_table_refreshes_every_layer_in_the_trainers_flow(dev, monkeypatch):
    """The method of test_pack_follow_gpu.py::follow on layers of every pack kind, with ``PackTable.run`` in the place the
    per-layer packers have there: after ``p.data.mul_(2)`` (no version bump) and the optimiser's epoch bump, one table launch
    must leave every layer's output and input gradient exactly doubled -- scaling a weight by two commutes with every product,
    sum and LeakyReLU -- without one per-layer pack call.  Each layer runs on an input of its own, so each doubles by itself."""
    from test_pack_follow_gpu import small_weights, uniform
    from torchsr_amd import _lib, functional as F, optim
    from torchsr_amd.layers import ACT_LRELU, Conv2d
    seq = torch.nn.Sequential(
        Conv2d(64, 64, 3, padding=1, bias=False, act=ACT_LRELU, slope=0.25),   # direct 3x3 (a fused LeakyReLU keeps it off Winograd)
        Conv2d(64, 64, 3, stride=2, padding=1, bias=False),
        Conv2d(64, 256, 3, padding=1, bias=False, shuffle=2),
        Conv2d(3, 64, 3, padding=1, bias=False),                               # thin data gradient
        Conv2d(64, 3, 9, padding=4, bias=False),                               # thin forward
        Conv2d(256, 256, 3, padding=1, bias=False),                            # on Winograd at 32 x 24 x 24 (test_pack_follow_gpu.py)
    ).to(dev)
    shapes = [(1, 8, 8, 64), (1, 8, 8, 64), (1, 8, 8, 64), (1, 8, 8, 4), (1, 8, 8, 64), (32, 24, 24, 256)]
    flat = optim.FlatParams(seq)       # the weights become slices of one flat buffer and share its epoch, as in the trainers
    small_weights(seq)
    xs = [uniform(s, 0.5, 1.0, 20 + i, dev).requires_grad_(True) for i, s in enumerate(shapes)]
    gs = [None] * len(xs)

    def run():
        out = []
        for i, (conv, x) in enumerate(zip(seq, xs)):
            y = conv(x)
            if gs[i] is None:
                gs[i] = uniform(tuple(y.shape), 0.5, 1.0, 40 + i, dev)
            out += [y.detach(), torch.autograd.grad(y, x, gs[i])[0]]
        return out

    assert _lib.lib().srx_wino_applicable(C.byref(seq[5]._st.desc(32, 24, 24))) == 1
    first = run()
    assert all(bool(t.abs().max() > 0) and bool(torch.isfinite(t).all()) for t in first)
    for conv in list(seq)[:5]:
        assert conv._st.direct.fwd is not None and conv._st.direct.bwd is not None
    assert seq[5]._st.wino.fwd is not None and seq[5]._st.wino.bwd is not None and seq[5]._st.direct.fwd is None
    table = F.PackTable(list(seq))
    params = list(seq.parameters())
    versions = [p._version for p in params]
    for p in params:
        p.data.mul_(2)
    assert [p._version for p in params] == versions
    flat.pack_epoch[0] += 1            # optim.FlatAdam.step, behind its srx_adam_step
    for conv in seq:                   # every packed copy is stale now: without the table each layer would repack by itself
        st = conv._st
        assert (st.wino if st.direct.fwd is None else st.direct).key != st.pack_key(conv.weight)
    with recorded_calls(monkeypatch) as names:
        assert table.run() is True
        second = run()
    assert names.count('srx_pack_table_run') == 1
    assert 'srx_conv2d_pack' not in names and 'srx_wino_pack' not in names
    assert any(n.startswith('srx_wino_fwd') for n in names) and 'srx_wino_bwd_data' in names   # (the spy does see the layers run)
    assert table.wino_items and len(table.items) >= 5
    for i, (a, b) in enumerate(zip(second, first)):
        assert torch.equal(a, 2 * b), ('layer', i // 2, 'dx' if i % 2 else 'y')


# ------------------------------------------------------------------------------------------------ 5. dense-block streams
RDB_SHAPES = [(32 if k < 4 else 64, 64 + 32 * k, 3, 3) for k in range(5)]


def rdb_weights(modulus, dev, aligned_copy_of=None):
    """Three blocks of five convs; element i of a block (counted through its convs) is (i % modulus + 1) * 2^-8 * 2^(8 * block):
    eight significant bits, exact in bf16, and no value of one block occurs in another (block b spans [2^(8b - 8), 2^(8b)))."""
    blocks = []
    for b in range(3):
        convs, i0 = [], 0
        for shape in RDB_SHAPES:
            n = int(np.prod(shape))
            i = torch.arange(i0, i0 + n, dtype=torch.int64)
            vals = (i % modulus + 1).to(torch.float32) * 2.0 ** (8 * b - 8)
            off = 1 if b == 1 else 0       # every conv of the middle block starts one float into its allocation
            buf = torch.empty(n + 4, dtype=torch.float32, device=dev)
            w = buf[off:off + n]
            w.copy_(vals.to(dev))
            assert w.data_ptr() % 16 == 4 * off
            convs.append(w)
            i0 += n
        blocks.append(convs)
    return blocks


@pytest.mark.parametrize('entry', ['srx_rdb_pack', 'srx_rdb_pack_bwd'])
def test_dense_block_streams_of_three_blocks(dev, entry):
    """``nblk = 3`` in one launch, the middle block's weights 4 but not 16 bytes aligned (the forward's scalar read path), against
    three one-block packs of 16-byte aligned copies, byte for byte, under prefills 0x00 and 0xFF (every byte written) with 256
    guard bytes on either side.  Values repeat every ``modulus`` elements, so tap, channel and block placement is checked up to
    that period; the second pass with 251 in place of 255 leaves no mistake consistent with both periods (they are coprime)."""
    from torchsr_amd import _lib
    per = _lib.lib().srx_rdb_packed_bytes()
    assert per > 0 and per % 16 == 0

    def pack(convs_of_blocks, dst):
        table = torch.tensor([w.data_ptr() for convs in convs_of_blocks for w in convs], dtype=torch.int64).to(dev)
        _lib.call(entry, table.data_ptr(), len(convs_of_blocks), dst.data_ptr(), _stream())
        torch.cuda.synchronize()

    seen = []
    for modulus in (255, 251):
        blocks = rdb_weights(modulus, dev)
        assert torch.equal(torch.cat(blocks[0]).to(torch.bfloat16).float(), torch.cat(blocks[0]))      # the values survive bf16
        assert float(torch.cat(blocks[0]).max()) < float(torch.cat(blocks[1]).min()) and float(torch.cat(blocks[1]).max()) < float(torch.cat(blocks[2]).min())
        want = []
        for convs in blocks:
            copies = [w.clone() for w in convs]
            assert all(c.data_ptr() % 16 == 0 for c in copies)
            one = torch.full((per,), 0x5A, dtype=torch.uint8, device=dev)
            pack([copies], one)
            want.append(one)
        want = torch.cat(want)
        got = []
        for prefill in (0x00, 0xFF):
            buf = torch.full((256 + 3 * per + 256,), prefill, dtype=torch.uint8, device=dev)
            pack(blocks, buf[256:256 + 3 * per])
            assert bool((buf[:256] == prefill).all()) and bool((buf[256 + 3 * per:] == prefill).all()), (modulus, prefill)
            assert torch.equal(buf[256:256 + 3 * per], want), (modulus, prefill)
            got.append(buf[256:256 + 3 * per])
        assert torch.equal(got[0], got[1])
        seen.append(want)
    assert not torch.equal(seen[0], seen[1])
