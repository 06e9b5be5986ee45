"""Restatement of the training pair pool in numpy / plain Python: ``exchange`` is ``srx_pool_exchange`` (csrc/pool.hip) on host
arrays, ``simulate`` follows the identity of every pair through a pool driven by ``DeviceLoader._draw_pool_slots``.  Both move
things and compute nothing, so the GPU tests compare bit for bit."""
import numpy as np

# the loader case of test_pair_pool_gpu.py; test_pair_pool_cpu.py pins that this seed mixes batches within these steps
LOADER = {'seed': 11, 'batch': 2, 'cap': 4, 'crop': 64, 'scale': 4, 'images': 8, 'epochs': 2}
LOADER_STEPS = LOADER['epochs'] * (LOADER['images'] // LOADER['batch'])


def exchange(pool_a, batch_a, pool_b, batch_b, slots, mode):
    """``srx_pool_exchange`` on arrays ``[cap, ...]`` / ``[n, ...]`` of any one dtype (the tests pass the int32 views of their
    floats): returns new ``(pool_a, batch_a, pool_b, batch_b)``, the inputs are left alone.  ``pool_b`` and ``batch_b`` may both be
    None.  mode 0: ``pool[slots[i]] = batch[i]``; mode 1: the two change places.  A slot outside ``[0, cap)`` leaves sample ``i``
    and the pool as they are.  Distinct slots are the caller's duty, as in the kernel."""
    assert mode in (0, 1) and (pool_b is None) == (batch_b is None)
    out = []
    for pool, batch in ((pool_a, batch_a), (pool_b, batch_b)):
        if pool is None:
            out += [None, None]
            continue
        pool, batch = np.array(pool, copy=True), np.array(batch, copy=True)
        assert pool.dtype == batch.dtype and pool.shape[1:] == batch.shape[1:] and len(slots) == batch.shape[0]
        for i, s in enumerate(slots):
            s = int(s)
            if not 0 <= s < pool.shape[0]:
                continue
            if mode == 0:
                pool[s] = batch[i]
            else:
                kept = pool[s].copy()
                pool[s] = batch[i]
                batch[i] = kept
        out += [pool, batch]
    return tuple(out)


def simulate(cap, batch, n_steps, draw_slots):
    """Who is where: step ``t`` generates the pairs ``(t, 0) .. (t, batch - 1)``; ``draw_slots()`` gives ``(slots, mode)`` of the
    next batch.  Returns a list of ``n_steps`` lists: the generated ``(step, sample)`` pair that sits in each yielded position."""
    pool = [None] * cap
    yielded = []
    for t in range(n_steps):
        generated = [(t, i) for i in range(batch)]
        slots, mode = draw_slots()
        assert len(slots) == batch == len(set(slots)) and all(0 <= s < cap for s in slots)
        if mode == 0:
            for s, pair in zip(slots, generated):
                pool[s] = pair
            yielded.append(generated)
        else:
            assert all(pool[s] is not None for s in slots), 'an exchange with a slot that was never stored'
            yielded.append([pool[s] for s in slots])
            for s, pair in zip(slots, generated):
                pool[s] = pair
    return yielded


def mixes(yielded, fill_steps):
    """The two things the loader test relies on, from a ``simulate`` result: a yielded batch that holds pairs of two or more
    generated batches, and a pair generated after the fill that is yielded later."""
    mixed = any(len({t for t, _ in pairs}) >= 2 for pairs in yielded)
    late = any(fill_steps <= t < step for step, pairs in enumerate(yielded) for t, _ in pairs)
    return mixed, late


def special_words(count, seed):
    """``count`` distinct 32-bit patterns as int32, the float32 oddities first: -0.0, the smallest denormal, +inf, -inf, a quiet
    NaN with a payload and a signalling NaN pattern -- a move through float arithmetic would change some of them."""
    first = np.array([0x80000000, 0x00000001, 0x7F800000, 0xFF800000, 0x7FC12345, 0x7F800001, 0xFFFFFFFF, 0x00000000], dtype=np.uint32)
    rest = np.random.RandomState(seed).permutation(np.arange(16, 16 + max(count - len(first), 0), dtype=np.uint32)) * np.uint32(2654435761)
    words = np.concatenate([first, rest])[:count]
    return words.view(np.int32)
