"""``--pair-pool`` without a GPU: the CLI flag's and the loader's refusals, the fourth random stream and the slots it gives, the
mixing the GPU loader test relies on, the ABI's refusals, the host checks of ``functional.pool_exchange``, and self-checks of
the restatement (pool_ref.py) the GPU tests compare against."""
import random

import numpy as np
import pytest
import torch

import pool_ref as R


# ------------------------------------------------------------------------------------------------------- the CLI
def test_cli_pair_pool_flag(capsys):
    from torchsr_amd.torchsr import parse_args
    assert parse_args(['train']).pair_pool == 0
    assert parse_args(['train', '--pair-pool', '0']).pair_pool == 0                                # off: nothing to refuse
    on = ['train', '--device-data', '--degradation', 'blind2', '--batch-size', '12']
    assert parse_args(on + ['--pair-pool', '180']).pair_pool == 180
    assert parse_args(['train', '--device-data', '--degradation', 'blind', '--batch-size', '16', '--pair-pool', '16']).pair_pool == 16
    for argv in (['train', '--batch-size', '4', '--pair-pool', '8'],
                 ['train', '--degradation', 'blind2', '--batch-size', '4', '--pair-pool', '8'],    # without --device-data
                 ['train', '--device-data', '--batch-size', '4', '--pair-pool', '8'],              # bicubic
                 ['train', '--device-data', '--degradation', 'bicubic', '--batch-size', '4', '--pair-pool', '8']):
        with pytest.raises(SystemExit) as exc:
            parse_args(argv)
        err = capsys.readouterr().err
        assert exc.value.code == 2 and '--pair-pool' in err and '--device-data' in err, argv
        assert '--degradation blind' in err and 'blind2' in err, argv
    for n, nearest in ((181, 'nearest: 180 and 192'), (100, 'nearest: 96 and 108'), (5, 'nearest: 12')):
        with pytest.raises(SystemExit) as exc:
            parse_args(on + ['--pair-pool', str(n)])
        err = ' '.join(capsys.readouterr().err.split())
        assert exc.value.code == 2 and '--pair-pool' in err and '--batch-size 12' in err and err.endswith(nearest), (n, err)
    for bad in ('-1', '1.5', 'many'):
        with pytest.raises(SystemExit) as exc:
            parse_args(on + ['--pair-pool', bad])
        assert exc.value.code == 2 and '--pair-pool' in capsys.readouterr().err, bad
    with pytest.raises(SystemExit):
        parse_args(['train', '--help'])
    text = ' '.join(capsys.readouterr().out.split())
    assert '--pair-pool N' in text and 'multiple of --batch-size' in text and 'per process' in text and 'not checkpointed' in text


# ------------------------------------------------------------------------------------------------------- the loader
def _images():
    return [torch.zeros((120 + i, 130, 3), dtype=torch.uint8) for i in range(9)]


def _loader(degradation='blind2', test=False, seed=3, rank=0, batch=4, **kw):
    from torchsr_amd.dataset import DeviceLoader
    return DeviceLoader(_images(), torch.device('cpu'), batch, 96, 4, test, seed, rank=rank, degradation=degradation, **kw)


@pytest.mark.parametrize('bad', [True, False, -1, -4, 1.0, 8.0, '8', None, [8]])
def test_device_loader_refuses_bad_pair_pool(bad):
    with pytest.raises(ValueError, match='pair_pool'):
        _loader(pair_pool=bad)


def test_device_loader_pair_pool_argument():
    import inspect
    from torchsr_amd.dataset import DeviceLoader, initialize_device_datasets
    with pytest.raises(ValueError, match='pair_pool.*multiple of the batch size 4.*4 and 8'):
        _loader(pair_pool=6)
    with pytest.raises(ValueError, match='pair_pool.*multiple of the batch size 4.*0 \\(off\\) and 4'):
        _loader(pair_pool=3)
    with pytest.raises(ValueError, match='pair_pool.*train'):
        _loader(test=True, pair_pool=8)
    with pytest.raises(ValueError, match='pair_pool.*blind'):
        _loader('bicubic', pair_pool=8)
    for degradation in ('bicubic', 'blind', 'blind2'):
        off = _loader(degradation, pair_pool=0)
        assert off.pair_pool == 0 and off.pool_rng is None and off.pool_lr is None and off.pool_hr is None
    assert _loader('bicubic', test=True, pair_pool=0).pool_rng is None
    for degradation in ('blind', 'blind2'):
        on = _loader(degradation, pair_pool=8)
        assert on.pair_pool == 8 and on.pool_rng is not None and on.pool_lr is None and on.pool_filled == 0   # the tensors come lazily
    for fn in (DeviceLoader.__init__, initialize_device_datasets):
        p = inspect.signature(fn).parameters['pair_pool']
        assert p.default == 0 and not isinstance(p.default, bool)


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k], k


@pytest.mark.parametrize('degradation,prob', [('blind', 0.0), ('blind2', 0.0), ('blind', 0.5), ('blind2', 0.5)])
def test_pair_pool_leaves_the_other_streams_alone(degradation, prob):
    """With one seed: the sample indices, the crop / flip rows, the degradation parameters and their Poisson branch of ``_plan()``
    are the same without the argument, with ``pair_pool=0`` and with a pool -- whether or not the pool's slots are drawn in
    between -- and the three older streams end in the same state.  The streams themselves are today's: drawn again by hand."""
    plain, off, on = _loader(degradation, poisson_prob=prob), _loader(degradation, poisson_prob=prob, pair_pool=0), \
        _loader(degradation, poisson_prob=prob, pair_pool=8)
    batches = 0
    for _ in range(3):  # epochs of 2 batches: the pool is full from the second epoch on
        for (ip, mp, dp), (i0, m0, d0), (i1, m1, d1) in zip(plain._plan(), off._plan(), on._plan()):
            assert ip == i0 == i1 and mp == m0 == m1
            _same(dp, d0)
            _same(dp, d1)
            on._draw_pool_slots()
            batches += 1
    assert batches == 6
    for other in (off, on):
        assert other.rng.getstate() == plain.rng.getstate() and other.deg_rng.getstate() == plain.deg_rng.getstate()
        assert (other.poi_rng is None) == (prob == 0) and (prob == 0 or other.poi_rng.getstate() == plain.poi_rng.getstate())
    # the seeds of the three older streams are what they were
    fresh = _loader(degradation, poisson_prob=prob, pair_pool=8)
    assert fresh.rng.getstate() == random.Random(3 * 7919 + 0).getstate()
    assert fresh.deg_rng.getstate() == random.Random(3 * 15485863 + 0 + 982451653).getstate()
    assert prob == 0 or fresh.poi_rng.getstate() == random.Random(3 * 32452843 + 0 + 472882027).getstate()
    for state in (fresh.rng.getstate(), fresh.deg_rng.getstate()):
        assert fresh.pool_rng.getstate() != state


def test_pool_slot_draws():
    """The first cap / batch batches are stores to consecutive slots and draw nothing; later ones exchange ``batch`` distinct
    slots in range; the draws depend on (seed, rank) alone and differ between ranks and seeds."""
    cap, b = 12, 4
    loader = _loader(pair_pool=cap)
    start = loader.pool_rng.getstate()
    for k in range(cap // b):
        assert loader._draw_pool_slots() == (list(range(k * b, (k + 1) * b)), 0)
    assert loader.pool_filled == cap and loader.pool_rng.getstate() == start          # the fill draws nothing
    draws = [loader._draw_pool_slots() for _ in range(200)]
    seen = set()
    for slots, mode in draws:
        assert mode == 1 and len(slots) == b == len(set(slots)) and all(isinstance(s, int) and 0 <= s < cap for s in slots)
        seen.update(slots)
    assert seen == set(range(cap)) and loader.pool_filled == cap
    assert any(slots != sorted(slots) for slots, _ in draws)                          # an order, not a set: positions are shuffled too

    def run(**kw):
        ld = _loader(pair_pool=cap, **kw)
        return [ld._draw_pool_slots() for _ in range(cap // b + 20)]

    assert run() == run() and run(rank=1) == run(rank=1) and run(seed=4) == run(seed=4)
    assert run() != run(rank=1) and run() != run(seed=4) and run(rank=1) != run(seed=4)
    assert run()[:cap // b] == run(rank=1)[:cap // b]                                 # the fill is the same everywhere
    assert run() == run(degradation='blind') == run(poisson_prob=0.5)                 # and the stream is the pool's own
    # a pool of one batch: every exchange takes the whole pool, in a drawn order
    one = _loader(pair_pool=b)
    assert one._draw_pool_slots() == (list(range(b)), 0)
    assert all(sorted(one._draw_pool_slots()[0]) == list(range(b)) for _ in range(5))


def test_the_gpu_loader_case_mixes_batches():
    """The condition the GPU loader test relies on, for its seed and sizes: within its steps a yielded batch holds pairs of two
    or more generated batches, and a pair generated after the fill is yielded later."""
    from torchsr_amd.dataset import DeviceLoader
    c = R.LOADER
    images = [torch.zeros((2 * c['crop'], 2 * c['crop'], 3), dtype=torch.uint8)] * c['images']
    loader = DeviceLoader(images, torch.device('cpu'), c['batch'], c['crop'], c['scale'], False, c['seed'], degradation='blind2',
                          pair_pool=c['cap'])
    assert len(loader) * c['epochs'] == R.LOADER_STEPS
    fill = c['cap'] // c['batch']
    yielded = R.simulate(c['cap'], c['batch'], R.LOADER_STEPS, loader._draw_pool_slots)
    assert yielded[:fill] == [[(t, i) for i in range(c['batch'])] for t in range(fill)]
    mixed, late = R.mixes(yielded, fill)
    print(f'seed {c["seed"]}: yielded {yielded}')
    assert mixed and late
    per_epoch = R.LOADER_STEPS // c['epochs']
    assert any(t < per_epoch for pairs in yielded[per_epoch:] for t, _ in pairs)      # a pair crosses the epoch boundary
    # the fill's batches are trained on as generated AND pooled (basicsr's behaviour); from then on a pair leaves the pool once
    flat = [p for pairs in yielded[fill:] for p in pairs]
    assert len(flat) == len(set(flat))


# ------------------------------------------------------------------------------------------------------- the restatement
def test_reference_exchange_and_simulate():
    words = R.special_words(6 * 5 + 3 * 5 + 6 * 2 + 3 * 2, 1)
    assert len(set(words.tolist())) == len(words) and words.dtype == np.int32
    as_float = words.view(np.float32)
    assert np.isnan(as_float).sum() >= 2 and np.isinf(as_float).sum() == 2 and np.signbit(as_float[0]) and as_float[0] == 0
    pa, ba, pb, bb = words[:30].reshape(6, 5), words[30:45].reshape(3, 5), words[45:57].reshape(6, 2), words[57:].reshape(3, 2)
    slots = (5, 0, 3)
    qa, ca, qb, cb = R.exchange(pa, ba, pb, bb, slots, 0)
    assert np.array_equal(ca, ba) and np.array_equal(cb, bb)
    for i, s in enumerate(slots):
        assert np.array_equal(qa[s], ba[i]) and np.array_equal(qb[s], bb[i])
    for s in (1, 2, 4):
        assert np.array_equal(qa[s], pa[s]) and np.array_equal(qb[s], pb[s])
    qa, ca, qb, cb = R.exchange(pa, ba, pb, bb, slots, 1)
    for i, s in enumerate(slots):
        assert np.array_equal(qa[s], ba[i]) and np.array_equal(ca[i], pa[s]) and np.array_equal(qb[s], bb[i]) and np.array_equal(cb[i], pb[s])
    back = R.exchange(qa, ca, qb, cb, slots, 1)
    assert all(np.array_equal(u, v) for u, v in zip(back, (pa, ba, pb, bb)))
    qa, ca, none_p, none_b = R.exchange(pa, ba, None, None, (-1, 6, 2), 1)            # out of range: that sample and the pool stay
    assert none_p is None and none_b is None
    assert np.array_equal(ca[:2], ba[:2]) and np.array_equal(ca[2], pa[2]) and np.array_equal(qa[2], ba[2])
    assert np.array_equal(np.delete(qa, 2, axis=0), np.delete(pa, 2, axis=0))
    assert np.array_equal(pa, words[:30].reshape(6, 5))                               # the inputs are left alone
    script = iter([([0, 1], 0), ([2, 3], 0), ([3, 0], 1), ([0, 1], 1)])
    assert R.simulate(4, 2, 4, lambda: next(script)) == [[(0, 0), (0, 1)], [(1, 0), (1, 1)], [(1, 1), (0, 0)], [(2, 1), (0, 1)]]
    assert R.mixes([[(0, 0), (0, 1)], [(1, 0), (1, 1)], [(1, 1), (0, 0)], [(2, 1), (0, 1)]], 2) == (True, True)
    assert R.mixes([[(0, 0), (0, 1)], [(1, 0), (1, 1)], [(0, 0), (0, 1)], [(1, 0), (1, 1)]], 2) == (False, False)


# ------------------------------------------------------------------------------------------------------- the ABI
def test_abi_refuses_bad_pool_exchange_arguments_without_a_gpu():
    """srx_pool_exchange refuses with a status code BEFORE the launch -- so the checks run here, with fake pointers, on CPU."""
    import ctypes as C
    from torchsr_amd import _lib
    if torch.cuda.is_available():
        pytest.skip('fake pointers: argument validation is exercised where a missed check cannot reach a device')
    assert 'pool.hip' in _lib.SOURCES and 'srx_pool_exchange' in _lib.EXPORTS
    lib = _lib.lib()
    pool_a, batch_a, pool_b, batch_b, slots = (0x10000000 + i * 0x1000000 for i in range(5))  # never dereferenced; 16 MB apart

    def err():
        buf = C.create_string_buffer(512)
        lib.srx_last_error(buf, 512)
        return buf.value.decode()

    def refused(word, pool_a=pool_a, batch_a=batch_a, elems_a=48, pool_b=pool_b, batch_b=batch_b, elems_b=768, slots=slots, n=2,
                cap=4, mode=1):
        rc = lib.srx_pool_exchange(pool_a, batch_a, elems_a, pool_b, batch_b, elems_b, slots, n, cap, mode, None)
        return rc != 0 and 'pool_exchange' in err() and word in err()

    for name in ('pool_a', 'batch_a', 'slots'):
        assert refused('null pointer', **{name: None}), name
    assert refused('both', pool_b=None) and refused('both', batch_b=None)
    assert refused('elems_b', pool_b=None, batch_b=None) and refused('elems_b', pool_b=None, batch_b=None, elems_b=1)
    assert refused('elems_b', elems_b=0)                                              # a given pair without elements
    assert refused('element counts', elems_a=0) and refused('element counts', elems_a=-4) and refused('element counts', elems_b=-1)
    assert refused('1..65535', n=0) and refused('1..65535', n=-1) and refused('1..65535', n=65536, cap=70000)
    assert refused('hold a batch', cap=0, n=1) and refused('hold a batch', cap=-3, n=1) and refused('hold a batch', cap=1) and refused('hold a batch', n=5)
    assert refused('too large', elems_a=1 << 29) and refused('too large', elems_b=1 << 29)
    assert refused('too large', elems_a=(1 << 31) - 1) and refused('too large', elems_b=(1 << 40))
    assert refused('too large', pool_b=None, batch_b=None, elems_b=0, elems_a=1 << 31, cap=1, n=1)
    assert refused('mode', mode=2) and refused('mode', mode=-1)
    assert refused('overlap', batch_a=pool_a) and refused('overlap', batch_a=pool_a + 4 * 48 * 4 - 4)  # the pool's last float
    assert refused('overlap', pool_a=batch_a + 2 * 48 * 4 - 4)
    assert refused('overlap', batch_b=pool_b + 768 * 4) and refused('overlap', pool_b=pool_a) and refused('overlap', batch_b=batch_a)
    assert refused('overlap', pool_b=batch_a + 4) and refused('overlap', batch_b=pool_a + 16)
    assert refused('overlap', pool_b=None, batch_b=None, elems_b=0, batch_a=pool_a + 48 * 4)
    # touching ranges are apart: the mode, checked last, is what fails
    assert refused('mode', batch_a=pool_a + 4 * 48 * 4, mode=7) and refused('mode', pool_b=batch_a + 2 * 48 * 4, mode=7)


# ------------------------------------------------------------------------------------------------------- the wrapper
def test_functional_pool_exchange_checks_arguments_before_the_device(monkeypatch):
    from torchsr_amd import functional as F
    monkeypatch.setattr(F, 'call', lambda *a: pytest.fail('a device call after bad arguments'))

    def args(**kw):
        base = dict(pool_lr=torch.zeros(6, 3, 4, 4), pool_hr=torch.zeros(6, 3, 16, 16), lr=torch.zeros(3, 3, 4, 4),
                    hr=torch.zeros(3, 3, 16, 16), slots=[5, 0, 3])
        base.update(kw)
        return base

    for slots in ([5, 0, 5], [0, 0, 0],                                               # duplicates
                  [5, 0, 6], [-1, 0, 3], [5, 0, 1 << 31],                             # out of range
                  [5, 0], [5, 0, 3, 1], [],                                           # a wrong count
                  [5, 0, 3.0], [5, 0, True], [5, 0, '3'], [5, 0, None]):              # not ints
        with pytest.raises(ValueError, match='slot'):
            F.pool_exchange(**args(slots=slots))
    with pytest.raises(ValueError, match='slot'):
        F.pool_exchange(**args(slots=torch.tensor([5, 0, 3])))                        # a host sequence of ints, not a tensor's scalars
    for kw in (dict(lr=torch.zeros(3, 3, 4, 5)), dict(hr=torch.zeros(3, 3, 16, 8)), dict(pool_lr=torch.zeros(6, 1, 4, 4)),
               dict(lr=torch.zeros(3, 48)), dict(hr=torch.zeros(2, 3, 16, 16)), dict(pool_hr=torch.zeros(5, 3, 16, 16)),
               dict(lr=torch.zeros(7, 3, 4, 4), hr=torch.zeros(7, 3, 16, 16), slots=[0, 1, 2, 3, 4, 5, 0]),   # a batch above the capacity
               dict(lr=torch.zeros(0, 3, 4, 4), hr=torch.zeros(0, 3, 16, 16), slots=[]), dict(pool_lr=torch.zeros(6), lr=torch.zeros(3)),
               dict(hr=None), dict(pool_hr=None), dict(lr=[[0.0]])):
        with pytest.raises(ValueError):
            F.pool_exchange(**args(**kw))
    for kw in (dict(lr=torch.zeros(3, 3, 4, 4, dtype=torch.float64)), dict(pool_hr=torch.zeros(6, 3, 16, 16, dtype=torch.float16)),
               dict(hr=torch.zeros(3, 3, 16, 16, dtype=torch.int32))):
        with pytest.raises(RuntimeError, match='float32'):
            F.pool_exchange(**args(**kw))
    for kw in (dict(lr=torch.zeros(3, 3, 4, 8)[..., ::2]), dict(pool_hr=torch.zeros(3, 6, 16, 16).transpose(0, 1)),
               dict(hr=torch.zeros(6, 3, 16, 16)[::2])):
        with pytest.raises(RuntimeError, match='contiguous'):
            F.pool_exchange(**args(**kw))
    with pytest.raises(RuntimeError, match='one device'):
        F.pool_exchange(**args(hr=torch.zeros(3, 3, 16, 16, device='meta')))
    with pytest.raises(RuntimeError, match='no backward'):
        F.pool_exchange(**args(lr=torch.zeros(3, 3, 4, 4, requires_grad=True)))
    with pytest.raises(RuntimeError, match='no CPU fallback'):   # legal arguments: the tensors' device is what is refused
        F.pool_exchange(**args())
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.pool_exchange(**args(pool_hr=None, hr=None))           # one tensor only is legal too
