"""The gradient guard on the MI355X: srx_grad_guard (global l2 norm in fp64, non-finite test, clip coefficient) and
srx_adam_step_guarded, through the C ABI, through optim.FlatAdam and inside the trainers' steps (eager, replayed hipGraph,
two ranks).

Where two runs are said to be equal they are compared bit for bit: with the guard idle (scale == 1) the guarded Adam is the
plain one, and every decision is taken on the device from bytes that are the same in both runs.
"""
import hashlib
import os
import struct
import warnings
from argparse import Namespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -24  # unit roundoff of fp32
BIG = 4096 * 1024 + 1024  # one full grid-stride pass of the streaming kernels (4096 workgroups x 256 threads x 4 floats) + 1024
NORM_SIZES = [1, 3, 4, 5, 1023, 4097, BIG + 1, BIG + 2, BIG + 3]


def bits(t):
    """the tensor's bytes (NaNs compare equal to themselves, -0.0 differs from 0.0)"""
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu()


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


class Guard:
    """srx_grad_guard through the C ABI on buffers of its own."""

    def __init__(self, dev, n):
        from torchsr_amd._lib import call
        self.n = n
        self.ws_bytes = int(call('srx_grad_guard_ws_bytes', n))
        self.ws = torch.empty(self.ws_bytes // 8, dtype=torch.float64, device=dev)
        self.state = torch.zeros(4, dtype=torch.int64, device=dev)

    def run(self, g, grad_scale=1.0, max_norm=0.0, skip_nonfinite=0):
        from torchsr_amd._lib import call
        assert g.numel() == self.n and g.dtype == torch.float32 and g.data_ptr() % 16 == 0
        call('srx_grad_guard', g.data_ptr(), self.n, grad_scale, max_norm, skip_nonfinite, self.ws.data_ptr(), self.ws_bytes,
             self.state.data_ptr(), torch.cuda.current_stream().cuda_stream)
        raw = self.state.cpu().numpy().tobytes()
        scale, skip, norm, _, skipped, clipped = struct.unpack('<fifiqq', raw)
        return {'scale': scale, 'skip': skip, 'norm': norm, 'skipped': skipped, 'clipped': clipped, 'raw': raw}


def gradient(rng, n):
    """randn * 10**randint(-6, 4): eleven decades in one buffer"""
    return (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 4, n)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- 1. norm
@pytest.mark.parametrize('n', NORM_SIZES)
def test_norm_and_clip_coefficient_against_fp64(dev, n):
    """norm, scale and the counters against numpy's float64, at one element, around a quad, below and above one workgroup,
    and past one grid-stride pass with each ragged tail.  The kernel's sum IS an fp64 sum of exact squares: what separates
    it from numpy's are the order of that sum (a few 2^-53) and ONE rounding to fp32 (2^-24): 2^-23 relative."""
    rng = np.random.default_rng(1000 + n % 977)
    g = gradient(rng, n)
    gd = torch.from_numpy(g).to(dev)
    g64 = g.astype(np.float64)
    for grad_scale in (1.0, 0.5):
        guard = Guard(dev, n)
        norm64 = grad_scale * float(np.sqrt(np.sum(g64 * g64)))
        a = guard.run(gd, grad_scale)
        print(f'  n {n} grad_scale {grad_scale}: norm {a["norm"]!r} vs {norm64!r}, rel {abs(a["norm"] - norm64) / norm64:.3e}')
        assert abs(a['norm'] - norm64) <= 2.0 ** -23 * norm64, (n, grad_scale, a['norm'], norm64)
        assert a['scale'] == 1.0 and a['skip'] == 0 and a['skipped'] == 0 and a['clipped'] == 0, a
        b = guard.run(gd, grad_scale)
        assert b['raw'] == a['raw'], (n, grad_scale, 'a second call wrote other bits')
        # skip_nonfinite on, still no clipping: nothing changes
        assert guard.run(gd, grad_scale, 0.0, 1)['raw'] == a['raw']
        # clipping: max_norm below the norm ...
        below = float(F32(0.5 * norm64))
        c = guard.run(gd, grad_scale, below)
        want = float(F32(min(1.0, below / (norm64 + 1e-6))))
        assert want < 1.0
        assert abs(c['scale'] - want) <= 2.0 ** -23 * want, (n, grad_scale, c['scale'], want)
        assert c['clipped'] == 1 and c['skipped'] == 0 and c['skip'] == 0 and c['norm'] == a['norm'], c
        # ... and above it (the 1e-6 of clip_grad_norm_'s denominator matters for a norm of 1e-6)
        above = float(F32(2.0 * norm64 + 1e-5))
        d = guard.run(gd, grad_scale, above)
        assert d['scale'] == 1.0 and d['clipped'] == 1 and d['skipped'] == 0, d
        e = guard.run(gd, grad_scale, below, 1)
        assert e['scale'] == c['scale'] and e['clipped'] == 2 and e['skipped'] == 0, e


# ------------------------------------------------------------------------------------------------ 2. non-finite detection
NONFINITE = [
    ('inf-first', 4097, 0, float('inf')),
    ('inf-first-big', BIG + 3, 0, float('inf')),
    ('nan-tail', 5, 4, float('nan')),                    # n % 4 == 1: the scalar tail
    ('nan-tail-3', 4099, 4098, float('nan')),            # n % 4 == 3: the tail's last lane
    ('nan-tail-big', BIG + 3, BIG + 2, float('nan')),
    ('neginf-second-pass', BIG + 3, 4096 * 1024 + 500, float('-inf')),  # a quad of the second grid-stride pass
    ('nan-single', 1, 0, float('nan')),
]


@pytest.mark.parametrize('name,n,at,value', NONFINITE, ids=[c[0] for c in NONFINITE])
def test_nonfinite_elements_are_found_where_a_kernel_can_miss_them(dev, name, n, at, value):
    rng = np.random.default_rng(7 + n % 101)
    g = gradient(rng, n)
    g[at] = value
    gd = torch.from_numpy(g).to(dev)
    guard = Guard(dev, n)
    a = guard.run(gd, 1.0, 0.0, 1)
    assert a['skip'] == 1 and a['scale'] == 0.0 and a['skipped'] == 1, (name, a)
    assert not np.isfinite(a['norm']), (name, a)
    b = guard.run(gd, 1.0, 0.0, 0)  # detection without the skip: torch's clip_grad_norm_(error_if_nonfinite=False)
    assert b['skip'] == 0 and b['skipped'] == 1, (name, b)
    c = guard.run(gd, 1.0, 1.0, 0)  # ... whose coefficient is then NaN (NaN norm) or 0 (inf norm)
    assert c['skip'] == 0 and (np.isnan(c['scale']) if np.isnan(a['norm']) else c['scale'] == 0.0), (name, c)
    g[at] = 1.0
    d = guard.run(torch.from_numpy(g).to(dev), 1.0, 0.0, 1)  # the same buffer without the element: a step again
    assert d['skip'] == 0 and d['scale'] == 1.0 and d['skipped'] == 1 and np.isfinite(d['norm']), (name, d)


@pytest.mark.parametrize('n,at', [(5, 4), (4097, 17), (BIG + 3, 4096 * 1024 + 500)])
def test_a_finite_gradient_whose_square_overflows_fp32_is_not_skipped(dev, n, at):
    """3e38 squared is +inf in fp32 and 9e76 in fp64: squaring in fp32 would skip a step that torch takes."""
    g = np.zeros(n, dtype=F32)
    g[at] = 3e38
    a = Guard(dev, n).run(torch.from_numpy(g).to(dev), 1.0, 0.0, 1)
    assert a['skip'] == 0 and a['scale'] == 1.0 and a['skipped'] == 0, a
    assert np.isfinite(a['norm']) and a['norm'] == float(F32(3e38)), a


# ------------------------------------------------------------------------------------------- 3.-5. through optim.FlatAdam
def make_adam(dev, n, p0, **guard):
    """A FlatAdam over n floats plus sentinel padding that belongs to nobody (as run_adam of tests/test_step_ops_gpu.py)."""
    from torchsr_amd import optim
    pad = p0.size - n
    holder = torch.nn.Module()
    holder.w = torch.nn.Parameter(torch.zeros(n + pad, device=dev))
    flat = optim.FlatParams(holder)
    flat.numel = n
    opt = optim.FlatAdam(flat, lr=1e-4, **guard)
    opt.grad_scale = 0.5
    flat.data.copy_(torch.from_numpy(p0).to(dev))
    sentinel = torch.from_numpy((np.arange(pad) + 1.5).astype(F32)).to(dev)
    for buf in (flat.data, opt.exp_avg, opt.exp_avg_sq):
        buf[n:] = sentinel
    opt.holder = holder
    return opt


def adam_state(opt):
    return [opt.flat.data.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_count.clone()]


def assert_same_state(a, b, what):
    for name, x, y in zip(('p', 'm', 'v', 'step'), a, b):
        assert same_bits(x, y), (what, name)


def start(rng, n):
    pad = 8 + (-n) % 4
    return (rng.standard_normal(n + pad) * 0.05).astype(F32), pad


def step_gradient(rng, n, pad):
    return (rng.standard_normal(n + pad) * 10.0 ** rng.integers(-6, 0, n + pad)).astype(F32)


@pytest.mark.parametrize('n', [BIG + 3, 1027])
def test_guarded_adam_with_an_idle_guard_is_plain_adam_bit_for_bit(dev, n):
    rng = np.random.default_rng(31 + n % 13)
    p0, pad = start(rng, n)
    plain = make_adam(dev, n, p0)
    guarded = make_adam(dev, n, p0, skip_nonfinite=True, max_grad_norm=1e30)
    assert guarded.guarded and not plain.guarded
    sentinel = (np.arange(pad) + 1.5).astype(F32)
    for step in range(1, 6):
        g = torch.from_numpy(step_gradient(rng, n, pad)).to(dev)
        for opt in (plain, guarded):
            opt.flat.grad.copy_(g)
            opt.step()
        assert_same_state(adam_state(plain), adam_state(guarded), f'n {n} step {step}')
        for buf in (guarded.flat.data, guarded.exp_avg, guarded.exp_avg_sq):
            assert np.array_equal(buf[n:].cpu().numpy(), sentinel), (n, step, 'padding past n was written')
        stats = guarded.guard_stats()
        assert stats['scale'] == 1.0 and stats['skip'] == 0 and stats['skipped'] == 0 and stats['clipped'] == 0, stats
    assert int(guarded.step_count.item()) == 5


@pytest.mark.parametrize('where', ['body', 'tail'])
def test_a_nonfinite_gradient_skips_the_step_and_leaves_no_trace(dev, where):
    n = 4099
    at = 2049 if where == 'body' else n - 1
    rng = np.random.default_rng(57)
    p0, pad = start(rng, n)
    twin = make_adam(dev, n, p0, skip_nonfinite=True)   # never sees the bad gradient
    opt = make_adam(dev, n, p0, skip_nonfinite=True)
    grads = [torch.from_numpy(step_gradient(rng, n, pad)).to(dev) for _ in range(3)]
    for g in grads[:2]:
        for o in (twin, opt):
            o.flat.grad.copy_(g)
            o.step()
    before = adam_state(opt)
    bad = grads[2].clone()
    bad[at] = float('nan')
    opt.flat.grad.copy_(bad)
    opt.step()
    assert_same_state(before, adam_state(opt), f'skipped step ({where})')
    assert int(opt.step_count.item()) == 2
    stats = opt.guard_stats()
    assert stats['skip'] == 1 and stats['skipped'] == 1 and stats['scale'] == 0.0, stats
    for o in (twin, opt):
        o.flat.grad.copy_(grads[2])
        o.step()
    assert_same_state(adam_state(twin), adam_state(opt), f'the step after the skipped one ({where})')
    assert int(opt.step_count.item()) == 3
    stats = opt.guard_stats()
    assert stats['skip'] == 0 and stats['skipped'] == 1 and twin.guard_stats()['skipped'] == 0, stats


def test_clipped_adam_steps_against_fp64(dev):
    """Five steps with gradients of norm ~10 (5 after grad_scale) clipped to 1: after every step p, m, v against ONE float64
    Adam step from the kernel's own previous state, the gradient multiplied by float32(grad_scale * scale) with the scale
    the guard wrote.  The guarded kernel rounds where adam_kernel rounds, so the bounds are run_adam's
    (tests/test_step_ops_gpu.py): 5 U B_m, 6 U v', 18 U B_p."""
    n = 4097
    rng = np.random.default_rng(99)
    p0, pad = start(rng, n)
    opt = make_adam(dev, n, p0, max_grad_norm=1.0)
    b1, b2, eps = (float(F32(x)) for x in (0.9, 0.999, 1e-8))
    omb1, omb2 = float(F32(1) - F32(0.9)), float(F32(1) - F32(0.999))
    lr = 1e-4
    p, m, v = p0[:n].astype(np.float64), np.zeros(n), np.zeros(n)
    for step in range(1, 6):
        g = (rng.standard_normal(n + pad) * (10.0 / np.sqrt(n))).astype(F32)
        opt.flat.grad.copy_(torch.from_numpy(g).to(dev))
        opt.step()
        stats = opt.guard_stats()
        norm64 = 0.5 * float(np.sqrt(np.sum(g[:n].astype(np.float64) ** 2)))
        assert abs(stats['norm'] - norm64) <= 2.0 ** -23 * norm64 and 4.0 < norm64 < 6.0, (stats, norm64)
        want = float(F32(1.0 / (norm64 + 1e-6)))
        assert abs(stats['scale'] - want) <= 2.0 ** -23 * want and stats['clipped'] == step, (stats, want)
        mult = float(F32(0.5) * F32(stats['scale']))  # one fp32 product, as the kernel forms it
        gs = g[:n].astype(np.float64) * mult
        bc1 = float(F32(1.0 - b1 ** step))
        bc2s = float(np.sqrt(F32(1.0 - b2 ** step)))
        ss = float(F32(float(F32(lr)) / bc1))
        bm = np.abs(b1 * m) + np.abs(omb1 * gs)
        m_ref = b1 * m + omb1 * gs
        v_ref = b2 * v + omb2 * gs * gs
        den = np.sqrt(v_ref) / bc2s + eps
        p_ref = p - ss * (m_ref / den)
        pk, mk, vk = (t[:n].cpu().numpy().astype(np.float64) for t in (opt.flat.data, opt.exp_avg, opt.exp_avg_sq))
        for what, got, ref, bound in (('m', mk, m_ref, 5 * U * bm), ('v', vk, v_ref, 6 * U * v_ref + 1e-300),
                                      ('p', pk, p_ref, 18 * U * (np.abs(p) + ss * (np.abs(m_ref) + bm) / den))):
            over = np.abs(got - ref) - bound
            assert over.max() <= 0, (step, what, float(over.max()), int(over.argmax()))
        p, m, v = pk, mk, vk
    assert int(opt.step_count.item()) == 5


# ------------------------------------------------------------------------------------------------------- 6.-8. trainers
def srgan_batch(dev):
    gold = np.load(os.path.join(GOLDEN, 'srgan_steps.npz'))
    return torch.from_numpy(gold['low_res']).to(dev), torch.from_numpy(gold['high_res']).to(dev)


def make_guarded(module, monkeypatch, clip, skip, *args, **kwargs):
    """``module.make_trainer(...)`` whose ``args`` carry the two optional extras (the trainer reads them like use_graphs)."""
    with monkeypatch.context() as mp:
        mp.setattr(module, 'Namespace', lambda **kw: Namespace(clip_grad_norm=clip, skip_nonfinite_steps=skip, **kw))
        return module.make_trainer(*args, **kwargs)


def trainer_state(t):
    out = {'G': t.gen_flat.data, 'D': t.disc_flat.data}
    for name in ('psnr_optimizer', 'gen_optimizer', 'disc_optimizer'):
        opt = getattr(t, name)
        out.update({f'{name}.m': opt.exp_avg, f'{name}.v': opt.exp_avg_sq, f'{name}.step': opt.step_count})
    return out


def assert_trainers_equal(a, b, what):
    sa, sb = trainer_state(a), trainer_state(b)
    for k in sa:
        assert same_bits(sa[k], sb[k]), (what, k)


@pytest.mark.parametrize('use_graphs', [True, False], ids=['graphs', 'eager'])
def test_srgan_trainer_with_an_idle_guard_equals_the_default_trainer(dev, monkeypatch, use_graphs):
    import test_step_gpu as S
    lr, hr = srgan_batch(dev)
    plain = S.make_trainer(dev, use_graphs)
    guarded = make_guarded(S, monkeypatch, 1e30, True, dev, use_graphs)
    assert guarded.disc_optimizer.guarded and not plain.disc_optimizer.guarded
    for t in (plain, guarded):
        for _ in range(2):
            t.pretrain_step(lr, hr)
        for _ in range(2):
            t.gan_step(lr, hr)
    assert_trainers_equal(plain, guarded, f'SRGAN, use_graphs={use_graphs}')
    for opt, steps in ((guarded.psnr_optimizer, 2), (guarded.gen_optimizer, 2), (guarded.disc_optimizer, 2)):
        stats = opt.guard_stats()
        assert int(opt.step_count.item()) == steps and stats['skipped'] == 0 and stats['clipped'] == 0, stats
        assert stats['scale'] == 1.0 and np.isfinite(stats['norm']) and stats['norm'] > 0, stats


def test_esrgan_trainer_with_an_idle_guard_equals_the_default_trainer(dev, monkeypatch):
    import test_esrgan_gpu as E
    gold = np.load(os.path.join(GOLDEN, 'esrgan.npz'))
    lr, hr = torch.from_numpy(gold['low_res']).to(dev), torch.from_numpy(gold['high_res']).to(dev)
    plain = E.make_trainer(dev)
    guarded = make_guarded(E, monkeypatch, 1e30, True, dev)
    assert guarded.gen_optimizer.guarded
    for t in (plain, guarded):
        t.gan_step(lr, hr)
    assert_trainers_equal(plain, guarded, 'ESRGAN')
    assert guarded.gen_optimizer.guard_stats()['scale'] == 1.0 and guarded.disc_optimizer.guard_stats()['scale'] == 1.0


def test_clipping_trainer_replayed_graph_equals_eager(dev, monkeypatch):
    import test_step_gpu as S
    lr, hr = srgan_batch(dev)
    probe = make_guarded(S, monkeypatch, None, True, dev, False)
    probe.gan_step(lr, hr)
    norm = probe.disc_optimizer.guard_stats()['norm']
    assert np.isfinite(norm) and norm > 0
    del probe
    eager = make_guarded(S, monkeypatch, 0.5 * norm, False, dev, False)
    graph = make_guarded(S, monkeypatch, 0.5 * norm, False, dev, True)
    for _ in range(3):  # graph trainer: two eager warm-ups, capture and replay at the third call
        eager.gan_step(lr, hr)
        graph.gan_step(lr, hr)
    assert 'gan.all' in graph._graphs
    assert_trainers_equal(eager, graph, 'clipping, graph vs eager')
    for t in (eager, graph):
        stats = t.disc_optimizer.guard_stats()
        assert stats['clipped'] >= 1 and stats['skipped'] == 0, stats
    assert eager.disc_optimizer.guard_stats() == graph.disc_optimizer.guard_stats()
    assert eager.gen_optimizer.guard_stats() == graph.gen_optimizer.guard_stats()


def test_a_nonfinite_target_skips_a_replayed_pretraining_step(dev, monkeypatch):
    """high_res[0, 0, 0, 0] = inf: the generator's forward pass stays finite (BatchNorm statistics included), the MSE and the
    whole gradient do not.  In the replayed graph nothing on the host sees it; the guard leaves parameters, Adam state and
    step count as they were and counts the step."""
    import test_step_gpu as S
    lr, hr = srgan_batch(dev)
    t = make_guarded(S, monkeypatch, None, True, dev, True)
    for _ in range(3):
        assert np.isfinite(t.pretrain_step(lr, hr).item())
    assert 'psnr.all' in t._graphs
    opt = t.psnr_optimizer
    before = [t.gen_flat.data.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_count.clone()]
    bad = hr.clone()
    bad[0, 0, 0, 0] = float('inf')
    loss = t.pretrain_step(lr, bad).item()
    assert not np.isfinite(loss), loss
    after = [t.gen_flat.data, opt.exp_avg, opt.exp_avg_sq, opt.step_count]
    assert_same_state(before, after, 'pre-training step on a non-finite target')
    stats = opt.guard_stats()
    assert stats['skip'] == 1 and stats['skipped'] == 1 and int(opt.step_count.item()) == 3, stats
    assert np.isfinite(t.pretrain_step(lr, hr).item())
    stats = opt.guard_stats()
    assert stats['skip'] == 0 and stats['skipped'] == 1 and int(opt.step_count.item()) == 4, stats
    assert not same_bits(before[0], t.gen_flat.data)
    assert bool(torch.isfinite(t.gen_flat.data).all())


# ------------------------------------------------------------------------------------------------------------ 9. two ranks
DDP_CLIP = 1e-4  # far below any gradient norm of the step: the clip is active on the clean step (asserted)


def _digest(t):
    return hashlib.sha256(bits(t).numpy().tobytes()).hexdigest()


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY='0')
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from oracle.weights import closed_form_state, seeded_input
        from torchsr_amd.srgan.trainer import SRGANTrainer
        dev = torch.device('cuda', 0)
        torch.cuda.set_device(dev)
        args = Namespace(disable_amp=True, batch_size=2, epochs=8, gan_checkpoint=None, local_rank=0, pretrain_epochs=1,
                         psnr_checkpoint=None, skip_image_save=True, world_size=world, rank=rank, use_graphs=False,
                         vgg_weights='random', clip_grad_norm=DDP_CLIP, skip_nonfinite_steps=True)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            t = SRGANTrainer(dev, args, [], [], 2, 2, distributed=True)
        t.generator.load_state_dict(closed_form_state(t.generator.state_dict()))
        t.generator.train()
        lr = seeded_input((2, 3, 24, 24), 170 + rank).to(dev)
        hr = seeded_input((2, 3, 96, 96), 180 + rank).to(dev)
        report = {'start': _digest(t.gen_flat.data)}
        bad = hr.clone()
        if rank == 1:
            bad[0, 0, 0, 0] = float('inf')
        report['bad_loss'] = t.pretrain_step(lr, bad).item()
        report['after_bad'] = _digest(t.gen_flat.data)
        report['bad_stats'] = t.psnr_optimizer.guard_stats()
        report['bad_step'] = int(t.psnr_optimizer.step_count.item())
        report['clean_loss'] = t.pretrain_step(lr, hr).item()
        report['after_clean'] = _digest(t.gen_flat.data)
        report['clean_stats'] = t.psnr_optimizer.guard_stats()
        report['clean_step'] = int(t.psnr_optimizer.step_count.item())
        out[rank] = report
        torch.cuda.synchronize()
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_take_the_same_decision_without_a_collective_of_its_own(dev):
    """Only rank 1's batch holds the inf; the guard runs behind the all-reduce, so both ranks see the same (non-finite) mean
    gradient and skip; a clean, clipped step then leaves them bitwise equal with the same norm."""
    import torch.multiprocessing as mp
    from test_ddp_gpu import _free_port
    world, port = 2, _free_port()
    mgr = mp.get_context('spawn').Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    assert len(out) == world
    r0, r1 = out[0], out[1]
    assert np.isfinite(r0['bad_loss']) and not np.isfinite(r1['bad_loss']), (r0['bad_loss'], r1['bad_loss'])
    for r in (r0, r1):
        assert r['bad_stats']['skip'] == 1 and r['bad_stats']['skipped'] == 1 and r['bad_step'] == 0, r
        assert r['after_bad'] == r['start'] == r0['start'], 'a skipped step moved the generator'
        assert r['clean_stats']['skip'] == 0 and r['clean_stats']['skipped'] == 1 and r['clean_step'] == 1, r
        assert r['clean_stats']['scale'] < 1.0 and np.isfinite(r['clean_stats']['norm']), r
        assert r['after_clean'] != r['start']
    assert r0['after_clean'] == r1['after_clean'], 'the ranks parted ways'
    assert r0['clean_stats'] == r1['clean_stats'], (r0['clean_stats'], r1['clean_stats'])
