"""``srx_pack_table_build`` / ``srx_pack_table_add_wino`` are host code: the record count and the launch width they report for
every layer of pack_cases.py, and what they refuse, asked without a GPU.  The pointers are never dereferenced on the host, so
arbitrary non-null integers stand in for device memory.

The rule for the record count (pack_cases.predicted_nrec, read from csrc/conv_host.h and ``bwd_classes`` in csrc/gconv.hip): one
record for the forward pack; with a backward destination one more for a thin data gradient, else one per stride-parity class,
stride^2 of them -- ``bwd_classes`` drops none, a class without a tap is a row block of zero padding -- and never more than 16,
since strides above 4 are refused.  ``srx_pack_table_run`` checks its arguments before it launches anything
(``SRX_REQUIRE(dev_table && nrec > 0 && nrec <= 65535 && max_elems > 0)`` stands ahead of the launch), so its refusals are
tested here too.
"""
import ctypes as C

import pytest

import pack_cases as PC

W_PTR, F_PTR, B_PTR = 0x10000000, 0x20000000, 0x30000000   # never dereferenced


def _m():
    from torchsr_amd import _lib
    return _lib


def _build(cases, bwd_flags, w=None, fwd=None):
    """(rc, nrec, max_elems) of one srx_pack_table_build over ``cases``."""
    m = _m()
    L = m.lib()
    n = len(cases)
    descs = (m.Conv2dDesc * max(n, 1))(*[m.Conv2dDesc(*PC.desc_fields(c)) for c in cases])
    arr = lambda ptrs: (C.c_void_p * max(n, 1))(*ptrs)  # noqa: E731
    wp = arr(w if w is not None else [W_PTR + (i << 20) for i in range(n)])
    fp = arr(fwd if fwd is not None else [F_PTR + (i << 20) for i in range(n)])
    bp = arr([B_PTR + (i << 20) if b else None for i, b in enumerate(bwd_flags)])
    host = (C.c_ubyte * L.srx_pack_table_bytes(max(n, 1)))()
    nrec, maxn = C.c_int(-1), C.c_longlong(-1)
    rc = L.srx_pack_table_build(descs, n, wp, fp, bp, host, C.byref(nrec), C.byref(maxn))
    return rc, nrec.value, maxn.value


def test_the_list_keeps_what_the_table_kernel_needs():
    taps = lambda c: c['k'] ** 2  # noqa: E731
    assert any(taps(c) > 9 and taps(c) % 9 for c in PC.CASES)                 # nine at a time with a tail
    assert any(c['stride'] >= 3 for c in PC.CASES) and any(c['shuffle'] for c in PC.CASES)
    assert {'fwd', 'dgrad'} <= {c['thin'] for c in PC.CASES}                  # both thin kinds
    assert any(not c['bwd'] for c in PC.CASES)
    assert 2 * sum(c['w_offset'] for c in PC.CASES) >= len(PC.CASES)          # at least half on weights 4 bytes off alignment
    ids = PC.by_id(PC.CASES)
    assert len(set(ids)) == len(ids) and set(PC.TABLE_FWD_ONLY) <= set(ids)
    big = ids.index('c512.s2')
    assert 0 < big < len(ids) - 1                                             # the largest record neither first nor last
    assert all(0 < ids.index(i) < len(ids) - 1 for i in PC.TABLE_FWD_ONLY)    # forward-only layers in the middle


@pytest.mark.parametrize('case', PC.CASES, ids=PC.by_id(PC.CASES))
def test_thin_flags_are_the_librarys(case):
    """``thin``: the library's own answer (srx_thin_plan refuses a layer whose forward / data gradient is not thin.hip's)."""
    m = _m()
    d = m.Conv2dDesc(*PC.desc_fields(case))
    out = (C.c_int * 8)()
    assert (m.lib().srx_thin_plan(C.byref(d), 0, out) == 0) == (case['thin'] == 'fwd')
    assert (m.lib().srx_thin_plan(C.byref(d), 1, out) == 0) == (case['thin'] == 'dgrad')


@pytest.mark.parametrize('case', PC.CASES, ids=PC.by_id(PC.CASES))
def test_record_count_of_a_layer(case):
    m = _m()
    L = m.lib()
    d = m.Conv2dDesc(*PC.desc_fields(case))
    assert L.srx_conv2d_packed_fwd_floats(C.byref(d)) > 0, m.last_error()
    assert L.srx_conv2d_packed_bwd_floats(C.byref(d)) > 0      # every stride here is <= 4: the layer has data-gradient classes
    rc, nrec, maxn = _build([case], [True])
    assert rc == 0, m.last_error()
    assert nrec == PC.predicted_nrec(case, True) and 1 < nrec <= 17 and maxn > 0
    assert nrec == (2 if case['thin'] == 'dgrad' else 1 + case['stride'] ** 2)
    rc, nrec0, maxn0 = _build([case], [False])
    assert rc == 0, m.last_error()
    assert nrec0 == 1 == PC.predicted_nrec(case, False) and 0 < maxn0 <= maxn


def test_record_count_of_the_whole_list():
    """One build over every layer: the counts add up, the launch width is the widest layer's."""
    m = _m()
    flags = [c['bwd'] and c['id'] not in PC.TABLE_FWD_ONLY for c in PC.CASES]
    each = [_build([c], [b]) for c, b in zip(PC.CASES, flags)]
    rc, nrec, maxn = _build(PC.CASES, flags)
    assert rc == 0, m.last_error()
    assert nrec == sum(PC.predicted_nrec(c, b) for c, b in zip(PC.CASES, flags)) == sum(e[1] for e in each)
    assert maxn == max(e[2] for e in each) and nrec <= 17 * len(PC.CASES)


@pytest.mark.parametrize('case', PC.WINO_CASES, ids=PC.by_id(PC.WINO_CASES))
def test_winograd_records_append(case):
    m = _m()
    L = m.lib()
    d = m.Conv2dDesc(*PC.wino_desc_fields(case))
    assert L.srx_wino_packed_floats(C.byref(d)) == 16 * case['cin'] * case['cout']
    host = (C.c_ubyte * L.srx_pack_table_bytes(1))()
    nrec, maxn = C.c_int(0), C.c_longlong(0)
    for i, (transpose, _) in enumerate(PC.wino_records(case)):
        assert L.srx_pack_table_add_wino(host, C.byref(nrec), C.byref(maxn), C.byref(d), W_PTR, F_PTR, transpose) == 0, m.last_error()
        assert nrec.value == i + 1 and maxn.value == case['cin'] * case['cout']   # one work item per channel pair
    maxn.value = 1 << 40                                                          # a wider record already in the table stays the width
    assert L.srx_pack_table_add_wino(host, C.byref(nrec), C.byref(maxn), C.byref(d), W_PTR, F_PTR, 0) == 0
    assert maxn.value == 1 << 40


def test_build_refuses_with_a_message():
    m = _m()
    case = PC.CASES[0]
    for kw, said in ((dict(cases=[], bwd_flags=[]), 'bad argument'),                               # n = 0
                     (dict(cases=[case], bwd_flags=[True], w=[None]), 'null pointer in layer 0'),
                     (dict(cases=[case], bwd_flags=[True], fwd=[None]), 'null pointer in layer 0'),
                     (dict(cases=[case, case], bwd_flags=[True, True], fwd=[F_PTR, None]), 'null pointer in layer 1')):
        rc, _, _ = _build(**kw)
        assert rc != 0 and 'pack_table_build' in m.last_error() and said in m.last_error(), m.last_error()


def test_add_wino_refuses_with_a_message():
    m = _m()
    L = m.lib()
    host = (C.c_ubyte * L.srx_pack_table_bytes(1))()
    nrec, maxn = C.c_int(0), C.c_longlong(0)
    shuffle = m.Conv2dDesc(*PC.wino_desc_fields(PC.WINO_CASES[-1]))
    assert PC.WINO_CASES[-1]['shuffle'] == 2
    assert L.srx_pack_table_add_wino(host, C.byref(nrec), C.byref(maxn), C.byref(shuffle), W_PTR, F_PTR, 1) != 0
    assert 'no Winograd data gradient' in m.last_error()
    others = [m.Conv2dDesc(*PC.desc_fields(c)) for c in PC.CASES if c['id'] in ('c64.s2', 'first.k3', 'e16to20.k5', 'e8to12')]
    assert len(others) == 4                      # stride 2, three input channels, 5 x 5, channels no multiple of 32
    for d in others:
        for transpose in (0, 1):
            assert L.srx_pack_table_add_wino(host, C.byref(nrec), C.byref(maxn), C.byref(d), W_PTR, F_PTR, transpose) != 0
            assert 'not a Winograd layer' in m.last_error()
    ok = m.Conv2dDesc(*PC.wino_desc_fields(PC.WINO_CASES[0]))
    for args in ((None, C.byref(nrec), C.byref(maxn), C.byref(ok), W_PTR, F_PTR, 0),
                 (host, C.byref(nrec), C.byref(maxn), C.byref(ok), None, F_PTR, 0),
                 (host, C.byref(nrec), C.byref(maxn), C.byref(ok), W_PTR, None, 0)):
        assert L.srx_pack_table_add_wino(*args) != 0 and 'pack_table_add_wino: bad argument' in m.last_error()
    assert nrec.value == 0 and maxn.value == 0   # a refusal appends nothing


@pytest.mark.parametrize('nrec,maxn', [(0, 256), (-1, 256), (65536, 256), (1, 0)])
def test_run_refuses_before_any_launch(nrec, maxn):
    """(the table pointer is not read: the arguments are refused first)"""
    m = _m()
    assert m.lib().srx_pack_table_run(F_PTR, nrec, maxn, None) != 0
    assert 'pack_table_run: bad argument' in m.last_error()
    assert m.lib().srx_pack_table_run(None, 1, 256, None) != 0 and 'pack_table_run: bad argument' in m.last_error()
