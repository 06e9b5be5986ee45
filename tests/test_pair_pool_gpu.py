"""``--pair-pool`` on the GPU: ``srx_pool_exchange`` against its restatement (pool_ref.py), bit for bit -- the kernel only moves
floats, so nothing here has a tolerance --, ``functional.pool_exchange``, the ``pair_pool`` DeviceLoader against the identity of
every pair that pool_ref.simulate predicts from the loader's own slot draws, and the CLI."""
import os

import numpy as np
import pytest
import torch

import pool_ref as R
from degrade_chain import same_draws
from guarded import _stream

pytestmark = pytest.mark.gpu

GUARD = 64            # words of a sentinel on either side of every buffer: a store outside it shows
SENTINEL = 0x5A5A5A5A


def _guarded(words, shape, dev):
    """``words`` (int32) on the device between two guards: the buffer and its float32 view of shape ``shape``."""
    buf = torch.full((GUARD + words.size + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    buf[GUARD:GUARD + words.size] = torch.from_numpy(words.reshape(-1).copy()).to(dev)
    return buf, buf[GUARD:GUARD + words.size].view(torch.float32).view(shape)


def _read(buf, shape):
    host = buf.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all()
    return host[GUARD:-GUARD].reshape(shape)


def _case(elems_a, elems_b, cap, n, seed):
    """Distinct words for the four arrays (the float32 oddities among them): int32 ``(pool_a, batch_a, pool_b, batch_b)``, the
    ``_b`` pair None when ``elems_b`` is 0."""
    sizes = [cap * elems_a, n * elems_a, cap * elems_b, n * elems_b]
    words = R.special_words(sum(sizes), seed)
    parts = np.split(words, np.cumsum(sizes)[:-1])
    shapes = [(cap, elems_a), (n, elems_a), (cap, elems_b), (n, elems_b)]
    return [p.reshape(s) if s[1] else None for p, s in zip(parts, shapes)]


def _run(arrays, slots, cap, n, mode, dev, times=1):
    """The raw ABI call, ``times`` times, on guarded device copies of ``arrays``: what the four buffers hold afterwards (int32)."""
    from torchsr_amd import _lib
    held = [(None, None) if a is None else _guarded(a, a.shape, dev) for a in arrays]
    (_, pa), (_, ba), (_, pb), (_, bb) = held
    slot_buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    slot_buf[GUARD:GUARD + n] = torch.tensor(list(slots), dtype=torch.int32).to(dev)
    slot_dev = slot_buf[GUARD:GUARD + n]
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    for _ in range(times):
        _lib.call('srx_pool_exchange', p(pa), p(ba), arrays[0].shape[1], p(pb), p(bb), 0 if pb is None else arrays[2].shape[1],
                  slot_dev.data_ptr(), n, cap, mode, _stream())
    torch.cuda.synchronize()
    assert slot_buf[GUARD:GUARD + n].cpu().tolist() == [int(np.int32(s)) for s in slots]          # the slots are only read
    return [None if a is None else _read(buf, a.shape) for a, (buf, _) in zip(arrays, held)]


def _equal(got, want):
    return all((g is None and w is None) or np.array_equal(g, w) for g, w in zip(got, want))


ELEMS = [(105, 192),                           # an odd count: the scalar path, sample bases that are not 16-byte aligned
         (192, 3072),                          # 16-byte units on both sides
         (4, 0),                               # one tensor only: a null _b pair
         (3 * 32 * 32, 3 * 128 * 128)]         # the training shape: several blocks per sample, several units per thread
SLOTS = {'cap6-n3': (6, 3, (5, 0, 3)),         # not monotonic
         'full-reversed': (5, 5, (4, 3, 2, 1, 0)),
         'n1': (3, 1, (1,)),
         'out-of-range': (6, 4, (-1, 2, 6, 2 ** 31 - 1))}


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('slots', list(SLOTS))
@pytest.mark.parametrize('elems', ELEMS, ids=lambda e: f'{e[0]}x{e[1]}')
def test_kernel_against_the_restatement(dev, elems, slots, mode):
    cap, n, slot = SLOTS[slots]
    arrays = _case(elems[0], elems[1], cap, n, seed=cap * 10 + n)
    want = R.exchange(*arrays, slot, mode)
    got = _run(arrays, slot, cap, n, mode, dev)
    assert _equal(got, want)
    # the restatement's own properties, stated on the device's result
    touched = [s for s in slot if 0 <= s < cap]
    for side in (0, 2):
        if arrays[side] is None:
            continue
        pool, batch, pool0, batch0 = got[side], got[side + 1], arrays[side], arrays[side + 1]
        rest = [s for s in range(cap) if s not in touched]
        assert np.array_equal(pool[rest], pool0[rest])                                           # untouched slots: bit-identical
        for i, s in enumerate(slot):
            if not 0 <= s < cap:
                assert np.array_equal(batch[i], batch0[i])                                       # an out-of-range slot: the sample stays
            else:
                assert np.array_equal(pool[s], batch0[i]) and np.array_equal(batch[i], batch0[i] if mode == 0 else pool0[s])
    if mode == 0:
        assert np.array_equal(got[1], arrays[1]) and (arrays[3] is None or np.array_equal(got[3], arrays[3]))   # the batch is left as it was
        assert _equal(_run(arrays, slot, cap, n, 0, dev, times=2), want)                         # storing twice stores the same
    else:
        assert _equal(_run(arrays, slot, cap, n, 1, dev, times=2), arrays)                       # exchanging twice puts everything back


def test_samples_larger_than_one_pass_of_the_grid(dev):
    """The blocks per sample are capped at 64 x 256 threads: beyond 16384 units a thread walks the grid-stride loop.  65793
    16-byte units with a ragged last pass on one side, an odd 65795 floats on the other."""
    elems = (4 * (64 * 512 * 2 + 257), 64 * 512 * 2 + 259)
    arrays = _case(elems[0], elems[1], 2, 1, seed=3)
    for mode in (0, 1):
        assert _equal(_run(arrays, (1,), 2, 1, mode, dev), R.exchange(*arrays, (1,), mode))


def test_slots_all_out_of_range_change_nothing(dev):
    for elems in ((105, 192), (192, 3072)):
        arrays = _case(elems[0], elems[1], 6, 2, seed=5)
        for mode in (0, 1):
            assert _equal(_run(arrays, (-1, 6), 6, 2, mode, dev), arrays)
            assert _equal(_run(arrays, (-2 ** 31, 1 << 20), 6, 2, mode, dev), arrays)


def test_reserved_compute_units_change_nothing(dev):
    """The grid comes from the element counts and the batch size: a reservation of the planner's changes no bit."""
    from torchsr_amd import _lib
    L = _lib.lib()
    prior = L.srx_device_cus() - L.srx_plan_cus()
    arrays = _case(3 * 32 * 32, 3 * 128 * 128, 6, 3, seed=9)
    want = R.exchange(*arrays, (5, 0, 3), 1)
    try:
        for k in (0, 64, 128):  # 128: the most the planner admits
            _lib.call('srx_set_reserved_cus', k)
            assert _equal(_run(arrays, (5, 0, 3), 6, 3, 1, dev), want), k
    finally:
        _lib.call('srx_set_reserved_cus', prior)
    assert L.srx_device_cus() - L.srx_plan_cus() == prior


def test_functional_pool_exchange(dev):
    """The wrapper returns the tensors it was given, now holding the dequeued pairs; a low-resolution sample and its target move
    together; a store leaves the batch alone; the ABI's own refusals come back as errors."""
    from torchsr_amd import functional as F
    cap, n = 6, 3
    # sample k of either side holds the value 100 pool + k everywhere: a pair that parted would show as two different values
    pool_lr = (torch.arange(cap, device=dev, dtype=torch.float32) + 100).view(cap, 1, 1, 1).expand(cap, 3, 8, 8).contiguous()
    pool_hr = (torch.arange(cap, device=dev, dtype=torch.float32) + 100).view(cap, 1, 1, 1).expand(cap, 3, 32, 32).contiguous()
    lr = torch.arange(n, device=dev, dtype=torch.float32).view(n, 1, 1, 1).expand(n, 3, 8, 8).contiguous()
    hr = torch.arange(n, device=dev, dtype=torch.float32).view(n, 1, 1, 1).expand(n, 3, 32, 32).contiguous()
    out = F.pool_exchange(pool_lr, pool_hr, lr, hr, [4, 1, 5])
    assert out[0] is lr and out[1] is hr
    ident = lambda t: t.flatten(1)[:, 0].tolist()  # noqa: E731
    for t in (pool_lr, pool_hr, lr, hr):
        assert bool((t.flatten(1) == t.flatten(1)[:, :1]).all())                       # every sample still one value
    assert ident(lr) == ident(hr) == [104.0, 101.0, 105.0]
    assert ident(pool_lr) == ident(pool_hr) == [100.0, 1.0, 102.0, 103.0, 0.0, 2.0]
    out = F.pool_exchange(pool_lr, pool_hr, lr, hr, (0, 2, 3), exchange=False)         # a store: the batch stays
    assert out[0] is lr and out[1] is hr and ident(lr) == ident(hr) == [104.0, 101.0, 105.0]
    assert ident(pool_lr) == ident(pool_hr) == [104.0, 1.0, 101.0, 105.0, 0.0, 2.0]
    only = F.pool_exchange(pool_lr, None, lr, None, [1, 4, 5])                         # one tensor only
    assert only[0] is lr and only[1] is None and ident(lr) == [1.0, 0.0, 2.0] and ident(pool_lr) == [104.0, 104.0, 101.0, 105.0, 101.0, 105.0]
    assert ident(pool_hr) == [104.0, 1.0, 101.0, 105.0, 0.0, 2.0]
    with pytest.raises(ValueError, match='distinct'):
        F.pool_exchange(pool_lr, pool_hr, lr, hr, [1, 1, 2])
    with pytest.raises(RuntimeError, match='overlap'):                                 # a batch that is a view of its pool
        F.pool_exchange(pool_lr, pool_hr, pool_lr[:3], hr, [3, 4, 5])
    with pytest.raises(RuntimeError, match='one device'):
        F.pool_exchange(pool_lr, pool_hr, lr.cpu(), hr, [3, 4, 5])


# ---------------------------------------------------------------------------------------------------------------- the loader
def _loaders(dev, degradation, **kw):
    from torchsr_amd.dataset import initialize_device_datasets
    c = R.LOADER
    return initialize_device_datasets(f'synthetic:{c["images"]}', dev, batch_size=c['batch'], crop_size=c['crop'], seed=c['seed'],
                                      degradation=degradation, **kw)[:2]


def _spy_slots(loader):
    """Record what ``loader._draw_pool_slots`` returns, in call order."""
    drawn, real = [], loader._draw_pool_slots

    def spy():
        out = real()
        drawn.append((list(out[0]), out[1]))
        return out
    loader._draw_pool_slots = spy
    return drawn


@pytest.mark.parametrize('gt_usm', [False, True])
def test_pair_pool_loader(dev, gt_usm):
    """Two epochs of a ``blind2`` loader with a pool of two batches beside the same loader without one: every yielded sample is,
    bit for bit, the generated pair -- low-resolution image AND target of one generated sample -- that pool_ref.simulate predicts
    from the loader's own slot draws."""
    c = R.LOADER
    cap, b, fill = c['cap'], c['batch'], c['cap'] // c['batch']
    kw = dict(gt_usm=gt_usm, poisson_prob=0.5)
    (pooled, pooled_test), (plain, plain_test) = _loaders(dev, 'blind2', pair_pool=cap, **kw), _loaders(dev, 'blind2', **kw)
    assert pooled.pair_pool == cap and plain.pair_pool == 0 and pooled_test.pair_pool == 0 and pooled_test.pool_rng is None
    assert len(pooled) == len(plain) == c['images'] // b and pooled.pool_lr is None
    drawn = _spy_slots(pooled)
    generated, yielded = [], []
    for epoch in range(c['epochs']):
        for (lr, hr), (lr_g, hr_g) in zip(pooled, plain):
            assert lr.shape == lr_g.shape == (b, 3, c['crop'] // c['scale'], c['crop'] // c['scale']) and hr.shape == hr_g.shape
            same_draws(pooled.last_degradation, plain.last_degradation)        # it describes the batch that was GENERATED
            generated.append((lr_g, hr_g))
            yielded.append((lr, hr))
        assert len(yielded) == (epoch + 1) * len(plain)
        assert pooled.pool_filled == cap and tuple(pooled.pool_lr.shape) == (cap, 3, 16, 16) and tuple(pooled.pool_hr.shape) == (cap, 3, 64, 64)
    assert len(yielded) == R.LOADER_STEPS == len(drawn)
    assert [d for d in drawn[:fill]] == [(list(range(k * b, (k + 1) * b)), 0) for k in range(fill)] and all(m == 1 for _, m in drawn[fill:])
    replay = iter(drawn)
    who = R.simulate(cap, b, R.LOADER_STEPS, lambda: next(replay))
    for step, ((lr, hr), pairs) in enumerate(zip(yielded, who)):
        for pos, (t, i) in enumerate(pairs):
            assert torch.equal(lr[pos].view(torch.int32), generated[t][0][i].view(torch.int32)), (step, pos, t, i)
            assert torch.equal(hr[pos].view(torch.int32), generated[t][1][i].view(torch.int32)), (step, pos, t, i)
    for step in range(fill):                                                          # while it fills: the pool-less loader's batches
        assert torch.equal(yielded[step][0], generated[step][0]) and torch.equal(yielded[step][1], generated[step][1])
    mixed, late = R.mixes(who, fill)
    assert mixed and late                                                             # pinned for this seed in test_pair_pool_cpu.py
    per_epoch = len(plain)
    assert any(t < per_epoch for pairs in who[per_epoch:] for t, _ in pairs)          # the pool outlives the epoch
    # generated samples differ from each other, so "equals the predicted pair" is "equals no other"
    flat = [generated[t][0][i] for t in range(R.LOADER_STEPS) for i in range(b)]
    assert all(not torch.equal(flat[0], other) for other in flat[1:])
    # what the pool holds at the end is what the simulation leaves there
    holds = [None] * cap
    for t, (slots, _) in enumerate(drawn):
        for i, s in enumerate(slots):
            holds[s] = (t, i)
    for s, (t, i) in enumerate(holds):
        assert torch.equal(pooled.pool_lr[s], generated[t][0][i]) and torch.equal(pooled.pool_hr[s], generated[t][1][i])
    seen = 0
    for x, y in zip(pooled_test, plain_test):                                         # the test loader is untouched
        assert len(x) == 3 and all(torch.equal(u, v) for u, v in zip(x, y))
        seen += 1
    assert seen == len(plain_test) >= 1


def test_pair_pool_loader_blind(dev):
    """``blind``: one epoch and a half through a pool of one batch -- after the fill every batch is the one before it, reordered."""
    c = R.LOADER
    b = c['batch']
    pooled, plain = _loaders(dev, 'blind', pair_pool=b)[0], _loaders(dev, 'blind')[0]
    drawn = _spy_slots(pooled)
    generated, yielded = [], []
    for _ in range(2):
        for (lr, hr), pair in zip(pooled, plain):
            generated.append(pair)
            yielded.append((lr, hr))
    assert drawn[0] == (list(range(b)), 0) and torch.equal(yielded[0][0], generated[0][0]) and torch.equal(yielded[0][1], generated[0][1])
    for step in range(1, len(yielded)):
        slots, mode = drawn[step]
        assert mode == 1 and sorted(slots) == list(range(b))
    replay = iter(drawn)
    who = R.simulate(b, b, len(yielded), lambda: next(replay))
    for (lr, hr), pairs in zip(yielded, who):
        for pos, (t, i) in enumerate(pairs):
            assert torch.equal(lr[pos], generated[t][0][i]) and torch.equal(hr[pos], generated[t][1][i])
    assert all({t for t, _ in pairs} == {step - 1} for step, pairs in enumerate(who) if step >= 1)


@pytest.mark.parametrize('degradation', ['blind', 'blind2'])
def test_pair_pool_zero_changes_nothing(dev, degradation, monkeypatch):
    """``pair_pool=0``: the calls of a loader built without the argument -- no ``srx_pool_exchange`` -- and the same bits; with a
    pool, one ``srx_pool_exchange`` behind every batch's own calls and nothing else."""
    from step_layers import record_op_calls
    c = R.LOADER
    off, default = _loaders(dev, degradation, pair_pool=0)[0], _loaders(dev, degradation)[0]
    assert off.pool_rng is None and default.pool_rng is None
    got, want = {}, {}
    calls_off = record_op_calls(monkeypatch, lambda: got.update(enumerate(off)))
    calls_default = record_op_calls(monkeypatch, lambda: want.update(enumerate(default)))
    names = [name for name, _ in calls_off]
    assert calls_off == calls_default and 'srx_pool_exchange' not in names and names.count('srx_crop_flip_u8') == len(off)
    assert len(got) == len(want) == len(off) and all(torch.equal(u, v) for i in got for u, v in zip(got[i], want[i]))
    assert off.pool_lr is None and off.pool_hr is None
    on = _loaders(dev, degradation, pair_pool=c['cap'])[0]
    calls_on = record_op_calls(monkeypatch, lambda: [None for _ in on])
    names_on = [name for name, _ in calls_on]
    assert names_on.count('srx_pool_exchange') == len(on) and [name for name in names_on if name != 'srx_pool_exchange'] == names
    assert [call for call in calls_on if call[0] != 'srx_pool_exchange'] == calls_off
    lc = c['crop'] // c['scale']
    modes = [args for name, args in calls_on if name == 'srx_pool_exchange']
    fill = c['cap'] // c['batch']
    assert modes == [(3 * lc * lc, 3 * c['crop'] ** 2, c['batch'], c['cap'], int(k >= fill)) for k in range(len(on))]
    starts = [i for i, name in enumerate(names_on) if name == 'srx_crop_flip_u8'] + [len(names_on)]
    assert all(names_on[end - 1] == 'srx_pool_exchange' for end in starts[1:])         # the last call of every batch


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_pair_pool_cli(dev, tmp_path, monkeypatch, capsys):
    """The command of test_poisson_noise_prob_cli with a ``--pair-pool`` of two batches: one pre-training and one GAN epoch of
    four steps each.  The pool fills in the first two steps; the third step of either phase is captured and replayed as a graph."""
    from torchsr_amd.torchsr import main
    monkeypatch.chdir(tmp_path)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'LOCAL_WORLD_SIZE', 'SLURM_NTASKS'):
        monkeypatch.delenv(k, raising=False)
    main(['train', '--model', 'srgan', '--train-dir', 'synthetic:16', '--batch-size', '4', '--epochs', '1',
          '--pretrain-epochs', '1', '--disable-amp', '--seed', '5', '--device-data', '--skip-image-save',
          '--vgg-weights', 'random', '--degradation', 'blind2', '--pair-pool', '8'])
    out = capsys.readouterr().out
    assert 'training pair pool: 8 pairs per process' in out and 'MB' in out
    assert 'hipGraph capture' not in out                                               # no capture failed: the steps ran as graphs
    psnr = [float(line.split('PSNR:')[1].split(',')[0]) for line in out.splitlines() if line.startswith('PSNR:')]
    assert len(psnr) >= 1 and all(np.isfinite(psnr))
    assert os.path.exists('srgan-gan-latest.pth')
    ckpt = torch.load('srgan-gan-latest.pth', map_location='cpu')
    assert all(torch.isfinite(v).all() for v in ckpt['state'].values() if v.is_floating_point())
    assert not any('pool' in key for key in ckpt) and not any('pool' in key for key in ckpt.get('resume', {}))   # not checkpointed
