"""Every case of linear_forms.py reaches the launch form it is there for -- asked of srx_linear_plan alone, which plans with the
function the launches of linear.hip plan with (host code: no GPU).  A planner change that makes a case vacuous fails here, loudly,
instead of leaving test_linear_forms_gpu.py to pass on the other kernel form."""
import ctypes as C

import pytest

import linear_forms as LF

OK, BADARG, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4
CASES = {c[0]: c for c in LF.CASES}


def cdiv(a, b):
    return -(-a // b)


@pytest.fixture
def lib():
    """The library with nothing forced; whatever a test forces is gone afterwards, and that checked on a shape whose plan
    shows both settings."""
    from torchsr_amd import _lib
    L = _lib.lib()
    assert L.srx_linear_force(0, 0) == 0
    try:
        yield L
    finally:
        assert L.srx_linear_force(0, 0) == 0
        assert plan(L, 16, 1024, 64, 0) == [4, 256, 1, 1, 2, 2]


_scratch = []


def pointer():
    """An address for calls that must be refused before anything is launched.  Without a GPU a fake one, never dereferenced: a
    missed check ends in a failed launch.  With one, 4 MB of device memory -- more than any tensor or workspace of the shapes
    below -- so that a missed check cannot send a kernel to memory nobody owns."""
    import torch
    if not torch.cuda.is_available():
        return C.c_void_p(16)
    if not _scratch:
        _scratch.append(torch.zeros(1 << 20, device='cuda'))
    return C.c_void_p(_scratch[0].data_ptr())


def plan(L, b, k, j, which):
    """srx_linear_plan's answer, or None for a refusal (which must carry a message)"""
    from torchsr_amd import _lib
    out = (C.c_int * 6)(*([-1] * 6))
    rc = L.srx_linear_plan(b, k, j, which, out)
    if rc == UNSUPPORTED:
        assert 'refused' in _lib.last_error(), _lib.last_error()
        return None
    assert rc == OK, (rc, _lib.last_error())
    return list(out)


def plans(L, case):
    cid, b, k, j, form, splits = case[:6]
    assert L.srx_linear_force(form, splits) == 0
    return [plan(L, b, k, j, which) for which in (0, 1, 2)]


def trips(total, per, unit, lanes=1):
    """trips of every split (and, with lanes = 4, of every wave of it: the waves interleave 64-wide slices of a split, a trip is
    one slice out of four): [[trips of wave 0, ...], ...]"""
    out = []
    for beg in range(0, total, per):
        n = cdiv(min(total, beg + per) - beg, unit)
        out.append([cdiv(max(n - w, 0), lanes) for w in range(lanes)])
    return out


def test_every_case_has_a_plan_entry():
    assert sorted(LF.PLANS) == sorted(CASES) and len(CASES) == len(LF.CASES)


@pytest.mark.parametrize('cid', LF.IDS)
def test_case_plans_what_it_is_there_for(lib, cid):
    case = CASES[cid]
    b, k, j, form, splits = case[1:6]
    got = plans(lib, case)
    assert got == [None if p is None else list(p) for p in LF.PLANS[cid]], (cid, got)
    fwd, dgrad, wgrad = got
    assert any(p is not None for p in got), 'a case that runs nothing'
    # the forcing is what the plan shows: a forced form on every launch, forced splits before their rounding to whole trips
    for which, p in enumerate(got):
        if p is None:
            assert form == 2
            continue
        if form:
            assert p[4] == form and p[5] == form
        if which < 2:
            total, unit = (k, 256) if which == 0 else (j, 16)
            assert p[2] == cdiv(b, 64) and p[3] == cdiv(min(64, b - 64 * (p[2] - 1)), 16)
            assert p[1] % unit == 0 and p[0] == cdiv(total, p[1])
            if splits:
                assert p[1] == cdiv(cdiv(total, splits), unit) * unit
            if p[5] == 2:
                assert p[3] <= 2 and k % 64 == 0 and (which == 0 or j % 16 == 0)
        else:
            assert p[:4] == [1, 0, 1, cdiv(b, 32)]
    # the workspace a forced call needs: the slabs of the planned splits, nothing for a refused pass
    need = max(0 if fwd is None else fwd[0] * b * j, 0 if dgrad is None else dgrad[0] * b * k)
    assert lib.srx_linear_ws_floats(b, k, j) == need


def test_table_covers_the_forms(lib):
    """coverage: what the table as a whole must reach, computed from the plans the library reports"""
    seen = set()
    for case in LF.CASES:
        cid, b, k, j, form, splits, act, bias = case[:8]
        fwd, dgrad, wgrad = plans(lib, case)
        for name, p in (('fwd', fwd), ('dgrad', dgrad)):
            if p is None:
                continue
            seen.add((name, 'first', p[4], min(4, cdiv(b, 16))))
            seen.add((name, 'last', p[5], p[3], 'whole' if b % 16 == 0 else 'ragged'))
            if p[2] > 1:
                seen.add((name, 'launches', p[4], p[5], p[3]))
        if fwd is not None:
            seen.add(('epilogue', fwd[5], act, bias))
            seen.add(('fwd', fwd[5], 'j', 'whole' if j % 16 == 0 else 'ragged'))
            seen.add(('fwd', fwd[5], 'k', 'slices' if k % 64 == 0 else 'partial slice'))
            for waves in trips(k, fwd[1], 64, 4):
                seen.add(('fwd', fwd[5], 'trips of wave 0', waves[0]))
                seen.add(('fwd', fwd[5], 'idle waves', waves.count(0)))
            seen.add(('fwd', fwd[5], 'slices of the last split', sum(trips(k, fwd[1], 64, 4)[-1])))
            seen.add(('fwd', fwd[5], 'splits', min(fwd[0], 4)))
        if dgrad is not None:
            per_split = [t[0] for t in trips(j, dgrad[1], 16)]
            for t in per_split:
                seen.add(('dgrad', dgrad[5], 'trips', t))
            if len(set(per_split)) > 1:
                seen.add(('dgrad', dgrad[5], 'short last split'))
            seen.add(('dgrad', dgrad[5], 'splits', min(dgrad[0], 4)))
        if wgrad is not None:
            seen.add(('wgrad', wgrad[4], 'trips', wgrad[3], 'whole' if b % 32 == 0 else 'ragged'))
    want = set()
    for f in (1, 2):
        want |= {('fwd', 'last', f, 1, 'ragged'), ('fwd', 'last', f, 1, 'whole'), ('fwd', 'last', f, 2, 'ragged'), ('fwd', 'last', f, 2, 'whole')}
        want |= {('dgrad', 'last', f, 1, 'ragged'), ('dgrad', 'last', f, 1, 'whole'), ('dgrad', 'last', f, 2, 'ragged'), ('dgrad', 'last', f, 2, 'whole')}
        want |= {('epilogue', f, act, bias) for act in (0, 1, 2) for bias in (0, 1)}
        want |= {('fwd', f, 'j', 'whole'), ('fwd', f, 'j', 'ragged'), ('fwd', f, 'k', 'slices')}
        want |= {('fwd', f, 'trips of wave 0', t) for t in (1, 2, 3)}          # both exits of the two-set loop, and a whole round
        want |= {('fwd', f, 'idle waves', 3), ('fwd', f, 'idle waves', 0)}     # K = 64 and a one-slice last split
        want |= {('fwd', f, 'slices of the last split', 1), ('fwd', f, 'splits', 1), ('fwd', f, 'splits', 2), ('fwd', f, 'splits', 4)}
        want |= {('dgrad', f, 'trips', t) for t in (1, 2, 3, 4)} | {('dgrad', f, 'short last split')}
        want |= {('dgrad', f, 'splits', s) for s in (1, 2, 3, 4)}
        want |= {('wgrad', f, 'trips', 1, 'ragged'), ('wgrad', f, 'trips', 1, 'whole'), ('wgrad', f, 'trips', 2, 'ragged'),
                 ('wgrad', f, 'trips', 2, 'whole'), ('wgrad', f, 'trips', 3, 'ragged'), ('wgrad', f, 'trips', 4, 'ragged')}
    want |= {('fwd', 1, 'k', 'partial slice'), ('fwd', 'first', 1, 3), ('fwd', 'first', 1, 4), ('dgrad', 'first', 1, 3), ('dgrad', 'first', 1, 4)}
    # a plain <4> launch, then a fast <1> / <2> one (B = 70, 81), and two plain ones (B = 112)
    for name in ('fwd', 'dgrad'):
        want |= {(name, 'launches', 1, 2, 1), (name, 'launches', 1, 2, 2), (name, 'launches', 1, 1, 3)}
    assert not want - seen, sorted(want - seen, key=str)


def test_defaults_of_the_product_shapes(lib):
    """with nothing forced the train steps' shapes run what they ran before the override existed"""
    assert [plan(lib, 16, 18432, 1024, w) for w in (0, 1, 2)] == [[15, 1280, 1, 1, 2, 2], [13, 80, 1, 1, 2, 2], [1, 0, 1, 1, 2, 2]]
    assert [plan(lib, 32, 18432, 1024, w) for w in (0, 1, 2)] == [[15, 1280, 1, 2, 2, 2], [13, 80, 1, 2, 2, 2], [1, 0, 1, 1, 2, 2]]
    assert [plan(lib, 32, 8192, 100, w) for w in (0, 1, 2)] == [[32, 256, 1, 2, 2, 2], [2, 64, 1, 2, 1, 1], [1, 0, 1, 1, 1, 1]]
    assert lib.srx_linear_ws_floats(32, 18432, 1024) == 13 * 32 * 18432


REFUSED = [  # (B, K, J, form, splits, passes refused)
    (17, 20, 64, 2, 0, (0, 1, 2)), (17, 68, 64, 2, 0, (0, 1, 2)), (17, 260, 64, 2, 0, (0, 1, 2)),   # K no multiple of 64
    (17, 256, 1, 2, 0, (1, 2)), (17, 256, 5, 2, 0, (1, 2)), (17, 256, 40, 2, 0, (1, 2)), (17, 256, 100, 2, 0, (1, 2)),  # ragged J: no fast gradient
    (33, 256, 16, 2, 0, (0, 1)), (64, 256, 16, 2, 0, (0, 1)), (70, 256, 16, 2, 0, (0, 1)), (112, 256, 16, 2, 0, (0, 1)),  # a launch with NB > 2
    (17, 1024, 64, 0, 5, (0, 1)), (17, 256, 16, 1, 2, (0, 1)), (17, 1024, 48, 2, 4, (1,)),           # more splits than trips
]


@pytest.mark.parametrize('b,k,j,form,splits,refused', REFUSED)
def test_refusals_leave_the_forcing_alone(lib, b, k, j, form, splits, refused):
    from torchsr_amd import _lib
    assert lib.srx_linear_force(form, splits) == 0
    before = [plan(lib, 16, 1024, 64, w) for w in (0, 1, 2)]
    one = pointer()
    big = 1 << 40
    for which in (0, 1, 2):
        p = plan(lib, b, k, j, which)
        assert (p is None) == (which in refused), (which, p)
        if which in refused:
            rc = [lambda: lib.srx_linear_fwd(one, one, None, one, b, k, j, 0, 0.0, one, big, None),
                  lambda: lib.srx_linear_bwd_data(one, one, one, b, k, j, one, big, None),
                  lambda: lib.srx_linear_bwd_weight(one, one, one, 0, b, k, j, None)][which]()
            assert rc == UNSUPPORTED and 'refused' in _lib.last_error()
    assert [plan(lib, 16, 1024, 64, w) for w in (0, 1, 2)] == before


def test_bad_force_arguments_change_nothing(lib):
    assert lib.srx_linear_force(2, 4) == 0
    before = [plan(lib, 16, 1024, 64, w) for w in (0, 1, 2)]
    assert before[0] == [4, 256, 1, 1, 2, 2]
    for bad in [(-1, 0), (3, 0), (0, -1)]:
        assert lib.srx_linear_force(*bad) == BADARG
    assert [plan(lib, 16, 1024, 64, w) for w in (0, 1, 2)] == before
    out = (C.c_int * 6)()
    for bad in [(0, 64, 16, 0), (16, 0, 16, 0), (16, 64, 0, 0), (16, 64, 16, 3), (16, 64, 16, -1)]:
        assert lib.srx_linear_plan(*bad, out) == BADARG
    assert lib.srx_linear_plan(16, 64, 16, 0, None) == BADARG


@pytest.mark.parametrize('form', [0, 1, 2])
def test_checks_sit_before_the_first_launch(lib, form):
    """K % 4 and the workspace size are refused by host code that runs before any launch: without a device, and with pointers
    nothing may read, the calls return their codes"""
    from torchsr_amd import _lib
    assert lib.srx_linear_force(form, 0) == 0
    one = pointer()
    assert lib.srx_linear_fwd(one, one, None, one, 16, 66, 16, 0, 0.0, one, 1 << 40, None) == BADARG and 'multiple of 4' in _lib.last_error()
    assert lib.srx_linear_bwd_data(one, one, one, 16, 66, 16, one, 1 << 40, None) == BADARG and 'multiple of 4' in _lib.last_error()
    assert lib.srx_linear_bwd_weight(one, one, one, 0, 16, 66, 16, None) == BADARG and 'multiple of 4' in _lib.last_error()
    b, k, j = 17, 1024, 64
    fwd, dgrad = plan(lib, b, k, j, 0), plan(lib, b, k, j, 1)
    assert fwd[0] == 4 and dgrad[0] == 1
    assert lib.srx_linear_fwd(one, one, None, one, b, k, j, 0, 0.0, one, fwd[0] * b * j - 1, None) == WORKSPACE
    assert 'workspace' in _lib.last_error()
    assert lib.srx_linear_bwd_data(one, one, one, b, k, j, one, dgrad[0] * b * k - 1, None) == WORKSPACE
    assert 'workspace' in _lib.last_error()
