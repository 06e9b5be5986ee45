"""The weight-pack staleness rule (functional.WeightPack.ensure) on CPU tensors: a fake size query and a fake packer that
records its calls, keys from a real ConvState.pack_key.  Needs neither the built library nor a GPU."""
import torch
from torch import nn

from torchsr_amd import functional as F

CPU = torch.device('cpu')


class Packer:
    """A kind's two parts: ``size`` (counted) and ``pack`` (recorded as (fwd address, bwd address or None, bwd_only))."""

    def __init__(self, n_fwd=12, n_bwd=20, dtype=torch.float32):
        self.n_fwd, self.n_bwd, self.dtype = n_fwd, n_bwd, dtype
        self.calls, self.sized = [], 0

    def size(self):
        self.sized += 1
        return self.n_fwd, self.n_bwd, self.dtype

    def pack(self, fwd, bwd, bwd_only):
        self.calls.append((fwd.data_ptr(), None if bwd is None else bwd.data_ptr(), bwd_only))


def layer(requires_grad=True):
    st = F.ConvState(8, 8, 3, 1, 1)
    return st, nn.Parameter(torch.full((8, 8, 3, 3), 0.01), requires_grad=requires_grad)


def ensure(slot, st, w, p, need_bwd=False):
    slot.ensure(st.pack_key(w), CPU, need_bwd, p.size, p.pack)


def test_first_ensure_packs_once_and_a_second_is_a_no_op():
    (st, w), p = layer(), Packer()
    ensure(st.direct, st, w, p)
    fwd = st.direct.fwd
    assert len(p.calls) == 1 and p.calls[0] == (fwd.data_ptr(), None, False)
    assert fwd.numel() == 12 and fwd.dtype == torch.float32 and st.direct.bwd is None and st.direct.key == st.pack_key(w)
    ensure(st.direct, st, w, p)
    assert len(p.calls) == 1 and p.sized == 1 and st.direct.fwd is fwd  # fresh: no pack, no size query


def _bump_version(st, w):
    with torch.no_grad():
        w.mul_(1.0)


def _bump_global(st, w):
    F.bump_pack_epoch()


def _bump_model(st, w):
    st.model_epoch[0] += 1


def _switch_precision(st, w):
    st.precision = 1 - st.precision


INGREDIENTS = (_bump_version, _bump_global, _bump_model, _switch_precision)


def test_each_key_ingredient_alone_repacks_once_into_the_same_storage():
    (st, w), p = layer(), Packer()
    ensure(st.direct, st, w, p, need_bwd=True)
    fwd, bwd = st.direct.fwd, st.direct.bwd
    ptrs = (fwd.data_ptr(), bwd.data_ptr())
    for i, change in enumerate(INGREDIENTS):
        change(st, w)
        ensure(st.direct, st, w, p, need_bwd=True)
        assert len(p.calls) == 2 + i, change.__name__
        assert p.calls[-1] == ptrs + (False,), change.__name__
        assert st.direct.fwd is fwd and st.direct.bwd is bwd and (fwd.data_ptr(), bwd.data_ptr()) == ptrs, change.__name__
        ensure(st.direct, st, w, p, need_bwd=True)
        assert len(p.calls) == 2 + i, change.__name__


def test_a_frozen_parameter_repacks_on_an_in_place_update_only():
    (st, w), p = layer(requires_grad=False), Packer()
    ensure(st.direct, st, w, p)
    for change in (_bump_global, _bump_model):
        change(st, w)
        ensure(st.direct, st, w, p)
        assert len(p.calls) == 1, change.__name__
    ptr = st.direct.fwd.data_ptr()
    w.mul_(1.0)
    ensure(st.direct, st, w, p)
    assert len(p.calls) == 2 and p.calls[-1] == (ptr, None, False)


def test_a_backward_copy_is_added_to_a_fresh_forward_one():
    (st, w), p = layer(), Packer()
    ensure(st.wino, st, w, p, need_bwd=False)
    fwd = st.wino.fwd
    assert st.wino.bwd is None
    ensure(st.wino, st, w, p, need_bwd=True)
    assert st.wino.fwd is fwd and st.wino.bwd is not None and st.wino.bwd.numel() == 20
    assert p.calls == [(fwd.data_ptr(), None, False), (fwd.data_ptr(), st.wino.bwd.data_ptr(), True)]  # "backward only"
    ensure(st.wino, st, w, p, need_bwd=False)  # a backward copy that is not needed now stays, and stays current
    ensure(st.wino, st, w, p, need_bwd=True)
    assert len(p.calls) == 2
    _bump_version(st, w)
    ensure(st.wino, st, w, p, need_bwd=False)
    assert len(p.calls) == 3 and p.calls[-1] == (fwd.data_ptr(), st.wino.bwd.data_ptr(), False)


def test_stamp_makes_the_next_ensure_a_no_op_for_that_slot_only():
    (st, w), p = layer(), Packer()
    for slot in (st.direct, st.wino, st.bf16s):
        ensure(slot, st, w, p)
    assert len(p.calls) == 3
    _bump_model(st, w)
    st.direct.stamp(st.pack_key(w))
    ensure(st.direct, st, w, p)
    assert len(p.calls) == 3
    assert st.wino.key != st.pack_key(w) and st.bf16s.key != st.pack_key(w)
    ensure(st.wino, st, w, p)
    ensure(st.bf16s, st, w, p)
    assert len(p.calls) == 5


def test_a_changed_size_reallocates_fwd_and_drops_bwd():
    (st, w), p = layer(), Packer()
    ensure(st.direct, st, w, p, need_bwd=True)
    fwd = st.direct.fwd
    p.n_fwd = 16
    _bump_version(st, w)
    ensure(st.direct, st, w, p, need_bwd=False)
    assert st.direct.fwd is not fwd and st.direct.fwd.numel() == 16 and st.direct.bwd is None
    assert p.calls[-1] == (st.direct.fwd.data_ptr(), None, False)


def test_a_fresh_state_exposes_every_pack_as_none():
    st = F.ConvState(8, 8, 3, 1, 1)
    for name in ('wpk_fwd', 'wpk_bwd', 'wino_fwd', 'wino_bwd', 'bf16s_fwd', 'bf16s_bwd'):
        assert getattr(st, name) is None, name
    for slot in (st.direct, st.wino, st.bf16s, st.thin9):
        assert slot.fwd is None and slot.bwd is None and slot.key is None and slot.desc is None
