"""``--poisson-noise-prob`` without a GPU: the threshold tables against exact arithmetic, the packed windows against the full
rows, the CLI flag's and the loader's refusals, the third random stream, the ABI's refusals, and self-checks of the restatement
(poisson_ref.py) the GPU tests compare against."""
import numpy as np
import pytest
import torch

import poisson_ref as P


# ------------------------------------------------------------------------------------------------------- the tables
TABLE_LEVELS = (0, 1, 2, 17, 128, 254, 255)


@pytest.mark.parametrize('vals', [1, 2, 4, 8, 16, 32, 64, 128, 256])
def test_thresholds_against_exact_arithmetic(vals):
    """T[level][k] against floor(CDF(k) 2^31) from 80-digit decimals on the rational lambda: within one count; rows do not
    decrease and reach 2^31 (the exact floor stays at 2^31 - 1: the documented last step up)."""
    from torchsr_amd.degradation import POISSON_K, poisson_thresholds
    t = poisson_thresholds(vals)
    assert t.shape == (256, POISSON_K) and t.dtype == np.uint32 and not t.flags.writeable
    ti = t.astype(np.int64)
    assert (np.diff(ti, axis=1) >= 0).all() and (ti[:, -1] == 1 << 31).all() and ti.max() == 1 << 31
    assert (ti[0] == 1 << 31).all()                                      # lambda = 0: k = 0 for every word
    worst = below = 0
    for lv in TABLE_LEVELS:
        exact = np.array(P.exact_thresholds(lv, vals, POISSON_K), dtype=np.int64)
        worst = max(worst, int(np.abs(ti[lv] - exact).max()))
        first_full = int(np.argmax(ti[lv] == 1 << 31))
        below = max(below, int(np.abs(ti[lv] - exact)[:first_full].max()) if first_full else 0)
        # the step to 2^31 is taken only on top of the last exact value (lambda = 0 is the one distribution whose CDF reaches 1)
        assert exact[first_full] == (1 << 31) - (0 if lv == 0 else 1)
    print(f'vals {vals}: largest |T - exact| over levels {TABLE_LEVELS} = {worst} ({below} below the step to 2^31)')
    assert worst <= 1


def test_threshold_rows_are_narrow_and_the_windows_hold_them():
    from torchsr_amd.degradation import POISSON_VALS, POISSON_WINDOW, poisson_table_words, poisson_thresholds
    words = poisson_table_words()
    assert words.dtype == np.int32 and words.shape == (9 * 256 + 9 * 256 * POISSON_WINDOW,) and not words.flags.writeable
    first = words[:9 * 256].reshape(9, 256)
    win = words[9 * 256:].view(np.uint32).reshape(9, 256, POISSON_WINDOW).astype(np.int64)
    assert (win[:, :, -1] == 1 << 31).all() and (np.diff(win, axis=2) >= 0).all() and (first >= 0).all()
    widest = 0
    us = np.concatenate([[0, 1, (1 << 31) - 1, (1 << 31) - 2], np.random.RandomState(2).randint(0, 1 << 31, 500)]).astype(np.int64)
    for v, vals in enumerate(POISSON_VALS):
        t = poisson_thresholds(vals).astype(np.int64)
        inner = ((t > 0) & (t < 1 << 31)).sum(axis=1)
        widest = max(widest, int(inner.max()))
        for lv in (0, 1, 2, 17, 100, 128, 200, 254, 255):
            want = np.searchsorted(t[lv], us, side='right')              # the smallest k with u < T[k]
            got = first[v, lv] + np.searchsorted(win[v, lv], us, side='right')
            assert np.array_equal(got, want) and want.max() < 512, (vals, lv)
    print(f'widest part of a row that is neither 0 nor 2^31: {widest} entries')
    assert widest < 200
    with pytest.raises(ValueError):
        poisson_thresholds(3)
    with pytest.raises(ValueError):
        poisson_thresholds(512)


# ------------------------------------------------------------------------------------------------------- the CLI
def test_cli_poisson_noise_prob_flag(capsys):
    from torchsr_amd.torchsr import parse_args
    assert parse_args(['train']).poisson_noise_prob == 0.0
    assert parse_args(['train', '--device-data', '--degradation', 'blind', '--poisson-noise-prob', '0.5']).poisson_noise_prob == 0.5
    assert parse_args(['train', '--device-data', '--degradation', 'blind2', '--poisson-noise-prob', '1']).poisson_noise_prob == 1.0
    assert parse_args(['train', '--poisson-noise-prob', '0']).poisson_noise_prob == 0.0          # off: nothing to refuse
    for argv in (['train', '--poisson-noise-prob', '0.5'],
                 ['train', '--degradation', 'blind2', '--poisson-noise-prob', '0.5'],                 # without --device-data
                 ['train', '--device-data', '--poisson-noise-prob', '0.5'],                           # bicubic
                 ['train', '--device-data', '--degradation', 'bicubic', '--poisson-noise-prob', '0.5']):
        with pytest.raises(SystemExit) as exc:
            parse_args(argv)
        err = capsys.readouterr().err
        assert exc.value.code == 2 and '--poisson-noise-prob' in err and '--device-data' in err, argv
        assert '--degradation blind' in err and 'blind2' in err, argv
    for bad in ('1.5', '-0.1', 'nan', 'inf', 'half'):
        with pytest.raises(SystemExit) as exc:
            parse_args(['train', '--device-data', '--degradation', 'blind', '--poisson-noise-prob', bad])
        assert exc.value.code == 2 and '--poisson-noise-prob' in capsys.readouterr().err, bad


# ------------------------------------------------------------------------------------------------------- the loader
def _images():
    return [torch.zeros((120 + i, 130, 3), dtype=torch.uint8) for i in range(9)]


def _loader(degradation, **kw):
    from torchsr_amd.dataset import DeviceLoader
    return DeviceLoader(_images(), torch.device('cpu'), 4, 96, 4, False, 3, degradation=degradation, **kw)


@pytest.mark.parametrize('bad', [-0.1, 1.5, float('nan'), float('inf'), None, '0.5', True, [0.5]])
def test_device_loader_refuses_bad_poisson_prob(bad):
    with pytest.raises(ValueError, match='poisson_prob'):
        _loader('blind', poisson_prob=bad)


def test_device_loader_poisson_prob_argument():
    import inspect
    from torchsr_amd.dataset import DeviceLoader, initialize_device_datasets
    with pytest.raises(ValueError, match='poisson_prob'):
        _loader('bicubic', poisson_prob=0.5)
    assert _loader('bicubic', poisson_prob=0.0).poisson_prob == 0.0 and _loader('bicubic', poisson_prob=0).poi_rng is None
    assert _loader('blind', poisson_prob=1).poisson_prob == 1.0 and _loader('blind2', poisson_prob=0.5).poi_rng is not None
    for fn in (DeviceLoader.__init__, initialize_device_datasets):
        names = list(inspect.signature(fn).parameters)
        assert names[-2:] == ['poisson_prob', 'degradation'] and inspect.signature(fn).parameters['poisson_prob'].default == 0.0


def _same(a, b, but=()):
    for k in a:
        if k in but:
            continue
        assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k], k


@pytest.mark.parametrize('degradation', ['blind', 'blind2'])
def test_poisson_draw(degradation):
    """With one seed: every existing key is what the loader without the flag draws, except sigma_n where Poisson was chosen;
    probability 1 zeroes every sigma_n; the Poisson stream advances by the same two draws per sample and stage whatever comes
    out; probability 0 creates no stream and leaves the keys as they were."""
    import random
    plain, half, one, off = (_loader(degradation), _loader(degradation, poisson_prob=0.5), _loader(degradation, poisson_prob=1.0),
                             _loader(degradation, poisson_prob=0.0))
    assert off.poi_rng is None and plain.poi_rng is None
    stages, hi = (1, (3.0,)) if degradation == 'blind' else (2, (3.0, 2.5))
    replay = random.Random(3 * 32452843 + 0 + 472882027)        # the stream, drawn again by hand
    chosen_total = batches = 0
    for _ in range(2):  # epochs
        for (ip, mp, dp), (ih, mh, dh), (i1, m1, d1), (i0, m0, d0) in zip(plain._plan(), half._plan(), one._plan(), off._plan()):
            assert ip == ih == i1 == i0 and mp == mh == m1 == m0
            assert 'poisson_scale' not in dp and d0.keys() == dp.keys() and dh.keys() == d1.keys() == dp.keys() | {'poisson_scale'}
            _same(dp, d0)
            _same(dp, dh, but=('sigma_n',))
            _same(dp, d1, but=('sigma_n',))
            n = len(ip)
            want = np.zeros((stages, n), dtype=np.float32)
            for i in range(n):
                for s in range(stages):
                    u, sc = replay.random(), replay.uniform(0.05, hi[s])
                    want[s, i] = sc if u < 0.5 else 0.0
            want = want.reshape(dp['sigma_n'].shape)
            ps = dh['poisson_scale']
            assert ps.dtype == np.float32 and ps.shape == dp['sigma_n'].shape and np.array_equal(ps, want)
            assert np.array_equal(dh['sigma_n'], np.where(ps > 0, 0, dp['sigma_n']))
            assert ((ps == 0) | ((ps >= 0.05) & (ps <= 3.0))).all()
            if stages == 2:
                assert (ps[1] <= 2.5).all()
            assert (d1['sigma_n'] == 0).all() and (d1['poisson_scale'] > 0).all()
            # the same scales come out at probability 1 where 0.5 chose Poisson: the position does not depend on outcomes
            assert np.array_equal(d1['poisson_scale'][ps > 0], ps[ps > 0])
            chosen_total += int((ps > 0).sum())
            batches += 1
    assert batches == 4 and 0 < chosen_total < 4 * 4 * stages
    assert half.poi_rng.getstate() == one.poi_rng.getstate() == replay.getstate()
    assert half.deg_rng.getstate() == plain.deg_rng.getstate() and half.rng.getstate() == plain.rng.getstate()


# ------------------------------------------------------------------------------------------------------- the ABI
def test_abi_refuses_bad_add_poisson_noise_arguments_without_a_gpu():
    """srx_add_poisson_noise refuses with a status code BEFORE the clear and the launches -- so the checks run here, with fake
    pointers, on CPU."""
    import ctypes as C
    from torchsr_amd import _lib
    if torch.cuda.is_available():
        pytest.skip('fake pointers: argument validation is exercised where a missed check cannot reach a device')
    lib = _lib.lib()
    x, out, scale, gray, tables, levels = (0x1000000 + i * 0x100000 for i in range(6))  # never dereferenced

    def err():
        buf = C.create_string_buffer(256)
        lib.srx_last_error(buf, 256)
        return buf.value.decode()

    def refused(word, x=x, out=out, scale=scale, gray=gray, tables=tables, levels=levels, n=2, h=24, w=24, quantize=0):
        rc = lib.srx_add_poisson_noise(x, out, scale, gray, tables, levels, 1, 2, n, h, w, quantize, None)
        return rc != 0 and 'add_poisson_noise' in err() and word in err()

    for name in ('x', 'out', 'scale', 'gray', 'tables', 'levels'):
        assert refused('null pointer', **{name: None}), name
    assert refused('bad shape', n=0) and refused('bad shape', n=-1) and refused('bad shape', n=65536)
    assert refused('bad shape', h=0) and refused('bad shape', w=0) and refused('bad shape', h=-24) and refused('bad shape', w=-1)
    assert refused('too large', h=1 << 16, w=1 << 15) and refused('too large', h=46341, w=46341)
    assert refused('too large', h=0x7fffffff, w=0x7fffffff)


def test_functional_add_poisson_noise_checks_arguments_before_the_device():
    from torchsr_amd import functional as F
    x = torch.zeros(2, 3, 8, 8)
    ok = dict(scale=[1.0, 1.0], gray=[0, 1], seed=5)
    for shape in ((3, 8, 8), (2, 1, 8, 8), (2, 4, 8, 8), (0, 3, 8, 8), (2, 3, 0, 8)):
        with pytest.raises(ValueError):
            F.add_poisson_noise(torch.zeros(shape), [1.0] * shape[0], [0] * shape[0], 5)
    for kw in (dict(scale=[1.0]), dict(gray=[0, 1, 0]), dict(scale=[[1.0, 1.0]]), dict(seed=-1), dict(seed=1 << 64), dict(seed=0.5),
               dict(seed=True)):
        with pytest.raises(ValueError):
            F.add_poisson_noise(x, **{**ok, **kw})
    with pytest.raises(RuntimeError, match='no backward'):
        F.add_poisson_noise(torch.zeros(2, 3, 8, 8, requires_grad=True), **ok)
    with pytest.raises(RuntimeError, match='no CPU fallback'):   # legal arguments: the tensor's device is what is refused
        F.add_poisson_noise(x, **ok)


# ------------------------------------------------------------------------------------------------------- the restatement
def test_reference_levels_and_vals():
    cases = P.level_images()
    x, scale, gray, _ = cases['constant-8x8']
    m = P.level_masks(x, scale, gray)
    assert m.shape == (1, 8) and m.view(np.uint32)[0, 77 >> 5] == 1 << (77 & 31) and P.vals_of(m).tolist() == [1]
    x, scale, gray, _ = cases['128-and-129-levels']
    assert P.vals_of(P.level_masks(x, scale, gray)).tolist() == [128, 256]
    x, scale, gray, _ = cases['odd-17x29']
    m = P.level_masks(x, scale, gray)
    assert (m[2] == 0).all() and P.vals_of(m).tolist() == [256, 256, 1]                 # the copied sample keeps an empty mask
    q = P.sample_levels(x, gray)
    assert np.array_equal(q[1, 0], q[1, 1]) and np.array_equal(q[1, 0], q[1, 2]) and not np.array_equal(q[0, 0], q[0, 1])
    assert np.abs(q[1, 0] - np.rint(255 * (0.299 * x[1, 0] + 0.587 * x[1, 1] + 0.114 * x[1, 2].astype(np.float64)))).max() <= 1
    x, scale, gray, _ = cases['edges-8x8']
    q = P.sample_levels(x, gray)
    assert q.min() == 0 and q.max() == 255 and (x < 0).any() and (x > 1).any()
    assert P.vals_of(np.zeros((1, 8), dtype=np.int32)).tolist() == [1]
    assert P.vals_of(np.array([[3, 0, 0, 0, 0, 0, 0, 0], [7, 0, 0, 0, 0, 0, 0, 0], [-1] * 8], dtype=np.int32)).tolist() == [2, 4, 256]


def test_grey_triples_tell_a_contracted_luma_from_the_right_one():
    """The grey case of the exactness tests is a real check: at every one of its 64 pixels each contracted form of the luma has
    another level than the float32 luma rounded after every operation -- so their masks differ, and so does every draw whose
    level moved: a kernel that fuses the luma, in either launch, cannot pass test_levels_are_exact and test_draws_are_exact."""
    x, scale, gray, seed = P.level_images()['grey-triples-8x8']
    assert x.shape == (1, 3, 8, 8) and gray.tolist() == [1] and len(set(P.GREY_TRIPLES)) == 64
    assert np.array_equal(np.rint(x.astype(np.float64) * 255).reshape(3, 64).T, np.array(P.GREY_TRIPLES))
    right = P.level(P.luma(x))
    assert np.array_equal(P.sample_levels(x, gray)[0, 0], right[0])
    (fused_a, fused_b, reordered), ambiguous = P.wrong_lumas(x)
    assert not ambiguous.any()
    for wrong in (fused_a, fused_b):
        assert (P.level(wrong) != right).all() and (np.abs(P.level(wrong) - right) == 1).all()
    assert (P.level(reordered) != right).sum() >= 24
    masks = P.level_masks(x, scale, gray)
    k, q, vals = P.draws(x, scale, gray, seed)
    for wrong in (fused_a, fused_b, reordered):
        lv = P.level(wrong)[0]
        wrong_mask = np.zeros(8, dtype=np.uint32)
        for v in np.unique(lv):
            wrong_mask[v >> 5] |= np.uint32(1 << (v & 31))
        assert not np.array_equal(wrong_mask.view(np.int32), masks[0])
        # the draws such a luma leads to, with the right vals: other k at most of the pixels whose level moved
        from torchsr_amd.degradation import poisson_thresholds
        t = poisson_thresholds(int(vals[0])).astype(np.int64)
        u = (P.words(1, 8, 8, seed)[0, 0] >> np.uint32(1)).astype(np.int64)
        k_wrong = np.array([np.searchsorted(t[a], b, side='right') for a, b in zip(lv.reshape(-1), u.reshape(-1))]).reshape(8, 8)
        noise_right = k[0, 0] / vals[0] - q[0, 0] / 255.0
        noise_wrong = k_wrong / vals[0] - lv / 255.0
        assert (np.abs(noise_right - noise_wrong)[lv != right[0]] > 1e-3).all()      # far beyond the result's fp32 bound
    assert vals.tolist() == [64] and len(np.unique(q)) > 32


def test_reference_draws_are_recoverable_and_poisson():
    """recover_k inverts result64 on every test image within the bound's margin, and on the cycle image the restatement's own draws
    pass the two moment checks the GPU test makes, within 3 standard errors for its fixed seed."""
    for name, (x, scale, gray, seed) in P.level_images().items():
        k, q, vals = P.draws(x, scale, gray, seed)
        want = P.result64(x, scale, k, q, vals)
        assert np.array_equal(P.recover_k(want, x, scale, q, vals), k), name
        live = np.asarray(scale) != 0
        margin = (P.result_bound(x, scale, k, q, vals)[live] * (vals[live] / np.asarray(scale, dtype=np.float64)[live])[:, None, None, None]).max()
        assert margin < 0.01, (name, margin)                             # a device result within the bound recovers the same k
        assert (k[~live] == 0).all()
    z_mean, z_var, lam = P.moment_scores(*P.cycle_draws()[:2])
    print(f'restatement: mean score {z_mean:+.2f}, variance score {z_var:+.2f}')
    assert abs(z_mean) <= 3 and abs(z_var) <= 3 and lam.max() == 256.0
