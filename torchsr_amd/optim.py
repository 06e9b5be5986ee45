"""Flat parameter / gradient buffers and the fused Adam of the trainers.

The reference builds three ``torch.optim.Adam`` instances over ~150 small tensors
(torchsr/srgan/trainer.py:171-185) and lets DDP bucket the gradients.  Here each
model's parameters are re-pointed into ONE contiguous fp32 buffer (and ``.grad``
into a second one), so that

* the optimiser is a single HBM-bound kernel launch (``srx_adam_step``),
* the data-parallel exchange is one RCCL all-reduce per model on the flat gradient
  buffer, with no flatten / unflatten copies,
* ``zero_grad`` is one memset,

while ``state_dict()`` / ``load_state_dict()`` keep working on the (now view) parameters.
"""
import struct
from typing import Iterable, List

import torch
from torch import nn, Tensor

from . import functional as F
from ._lib import call


class FlatParams:
    """Re-point ``module``'s parameters and gradients into flat, 16-byte aligned buffers."""

    ALIGN = 4  # floats

    def __init__(self, module: nn.Module):
        params = [p for p in module.parameters() if p.requires_grad]
        if not params:
            raise RuntimeError('FlatParams: module has no trainable parameters')
        dev, dt = params[0].device, params[0].dtype
        if dt != torch.float32:
            raise RuntimeError('FlatParams: fp32 parameters expected')
        offs, total = [], 0
        for p in params:
            offs.append(total)
            total += (p.numel() + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.data = torch.zeros(total, dtype=dt, device=dev)
        self.grad = torch.zeros(total, dtype=dt, device=dev)
        self.params: List[nn.Parameter] = params
        self.offsets: List[int] = offs
        self.numel = total
        # bumped by every optimiser step on this buffer: the convs of THIS model repack, other models' do not
        self.pack_epoch = [0]
        for m in module.modules():
            st = getattr(m, '_st', None)
            if isinstance(st, F.ConvState):
                st.model_epoch = self.pack_epoch
        with torch.no_grad():
            for p, o in zip(params, offs):
                n = p.numel()
                self.data[o:o + n].copy_(p.detach().reshape(-1))
                p.data = self.data[o:o + n].view(p.shape)
                p.grad = self.grad[o:o + n].view(p.shape)

    def offsets_by_name(self, module: nn.Module) -> dict:
        """``{parameter name: offset (floats) in the flat buffers}`` for the module this buffer was built from."""
        where = {id(p): o for p, o in zip(self.params, self.offsets)}
        return {n: where[id(p)] for n, p in module.named_parameters() if id(p) in where}

    def zero_grad(self) -> None:
        """One memset; re-attaches the views in case something set ``.grad = None``."""
        self.grad.zero_()
        off = 0
        for p in self.params:
            n = p.numel()
            if p.grad is None or p.grad.data_ptr() != self.grad.data_ptr() + off * 4:
                p.grad = self.grad[off:off + n].view(p.shape)
            off += (n + self.ALIGN - 1) // self.ALIGN * self.ALIGN


class FlatAdam:
    """``torch.optim.Adam(params, lr, betas)`` semantics on a :class:`FlatParams` buffer.

    Several instances may share one ``FlatParams`` (the reference keeps ``psnr_optimizer`` and
    ``gen_optimizer`` as separate Adam states over the same generator, trainer.py:171-185).
    ``lr`` and the step count live on the device (hipGraph friendly).
    """

    def __init__(self, flat: FlatParams, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_grad_norm: float = None, skip_nonfinite: bool = False):
        if max_grad_norm is not None and not float(max_grad_norm) > 0:  # (also NaN)
            raise ValueError(f'FlatAdam: max_grad_norm must be > 0, got {max_grad_norm}')
        self.flat = flat
        self.betas, self.eps = betas, eps
        dev = flat.data.device
        self.exp_avg = torch.zeros_like(flat.data)
        self.exp_avg_sq = torch.zeros_like(flat.data)
        self.step_count = torch.zeros((), dtype=torch.int64, device=dev)
        self.lr_dev = torch.tensor(float(lr), dtype=torch.float32, device=dev)
        self._lr = float(lr)
        self.grad_scale = 1.0
        self.pack_table = None  # functional.PackTable of the model's convs (set by the trainer)
        self.param_groups = [{'lr': float(lr), 'initial_lr': float(lr)}]  # StepLR-style access
        # gradient guard (off by default: ``step`` is then the single srx_adam_step call): the global l2 norm of the
        # flat gradient is clipped to ``max_grad_norm`` (torch.nn.utils.clip_grad_norm_) and / or a step whose gradient
        # holds an inf or a NaN is skipped (what GradScaler.step does) -- decided on the device, so it replays in a hipGraph
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = self.max_grad_norm is not None or self.skip_nonfinite
        if self.guarded:
            # allocated once: a captured graph holds these pointers
            self.guard_state = torch.zeros(4, dtype=torch.int64, device=dev)  # srx_grad_guard_t, 32 bytes
            ws_bytes = int(call('srx_grad_guard_ws_bytes', flat.numel))
            self.guard_ws = torch.empty(max(1, ws_bytes // 8), dtype=torch.float64, device=dev)

    @property
    def lr(self) -> float:
        return self._lr

    def set_lr(self, lr: float) -> None:
        self._lr = float(lr)
        self.param_groups[0]['lr'] = float(lr)
        self.lr_dev.fill_(float(lr))

    def zero_grad(self) -> None:
        self.flat.zero_grad()

    @torch.no_grad()
    def step(self) -> None:
        f = self.flat
        st = torch.cuda.current_stream().cuda_stream
        if self.guarded:
            call('srx_grad_guard', f.grad.data_ptr(), f.numel, self.grad_scale, self.max_grad_norm or 0.0,
                 int(self.skip_nonfinite), self.guard_ws.data_ptr(), self.guard_ws.numel() * 8, self.guard_state.data_ptr(), st)
            call('srx_adam_step_guarded', f.data.data_ptr(), f.grad.data_ptr(), self.exp_avg.data_ptr(),
                 self.exp_avg_sq.data_ptr(), f.numel, self.lr_dev.data_ptr(), self.betas[0], self.betas[1], self.eps,
                 self.grad_scale, self.step_count.data_ptr(), self.guard_state.data_ptr(), st)
        else:
            call('srx_adam_step', f.data.data_ptr(), f.grad.data_ptr(), self.exp_avg.data_ptr(),
                 self.exp_avg_sq.data_ptr(), f.numel, self.lr_dev.data_ptr(), self.betas[0], self.betas[1], self.eps,
                 self.grad_scale, self.step_count.data_ptr(), st)
        # (on a skipped step the repack rewrites the same weights: the launch sequence of a captured step stays static)
        self.flat.pack_epoch[0] += 1
        if self.pack_table is not None:  # every conv of the model repacked by one launch
            self.pack_table.run()

    def guard_stats(self) -> dict:
        """The guard's device state after the last ``step`` (one device -> host copy, which synchronises): ``norm`` of the
        scaled gradient, the ``scale`` applied, whether the step was ``skip``-ped, and the running ``skipped`` / ``clipped``
        counts (a skipped step has scale 0 and counts as both).  The counts are not part of ``state_dict``: they restart
        with the process."""
        if not self.guarded:
            raise RuntimeError('FlatAdam.guard_stats: no gradient guard (max_grad_norm / skip_nonfinite) on this optimiser')
        scale, skip, norm, _, skipped, clipped = struct.unpack('<fifiqq', self.guard_state.cpu().numpy().tobytes())
        return {'norm': norm, 'scale': scale, 'skip': skip, 'skipped': skipped, 'clipped': clipped}

    def state_dict(self):
        return {'exp_avg': self.exp_avg, 'exp_avg_sq': self.exp_avg_sq, 'step': self.step_count, 'lr': self._lr}

    def load_state_dict(self, sd) -> None:
        self.exp_avg.copy_(sd['exp_avg'])
        self.exp_avg_sq.copy_(sd['exp_avg_sq'])
        self.step_count.copy_(sd['step'])
        self.set_lr(sd['lr'])


class FlatEMA:
    """Exponential moving average of a :class:`FlatParams` buffer (Real-ESRGAN's ``ema_decay``): ``update()`` is one launch,
    ``ema <- decay * ema + (1 - decay) * p`` in fp32 over the whole flat buffer (``srx_ema_update``).  The alignment gaps are 0
    in both buffers and stay 0.  ``data`` is allocated once, here: a captured graph holds its address.  ``1 - decay`` is formed
    in double and rounded once, on its way into the call.

    ``pack_epoch`` is the staleness counter of a module whose parameters are views into ``data`` (``shadow``): nothing bumps it
    per step -- whoever evaluates that module bumps it first (``refresh``)."""

    def __init__(self, flat: FlatParams, decay: float):
        decay = float(decay)
        if not 0.0 <= decay < 1.0:  # (also NaN)
            raise ValueError(f'FlatEMA: decay must be in [0, 1), got {decay}')
        self.flat, self.decay, self.one_minus_decay = flat, decay, 1.0 - decay
        self.data = flat.data.clone()
        self.pack_epoch = [0]

    @torch.no_grad()
    def reset(self) -> None:
        """Start the average again from the weights as they are now."""
        self.data.copy_(self.flat.data)
        self.pack_epoch[0] += 1

    @torch.no_grad()
    def update(self) -> None:
        call('srx_ema_update', self.data.data_ptr(), self.flat.data.data_ptr(), self.flat.numel, self.decay,
             self.one_minus_decay, torch.cuda.current_stream().cuda_stream)

    def refresh(self) -> None:
        """Before an evaluation of ``shadow``'s module: its packed weights are as old as the last one."""
        self.pack_epoch[0] += 1

    def shadow(self, module: nn.Module) -> nn.Module:
        """A never-trained copy of ``module`` (the one ``flat`` was built from) whose parameters are views into the average, in
        eval mode; its convs follow ``pack_epoch``, not the optimiser's counter."""
        import copy
        twin = copy.deepcopy(module).to(self.data.device)  # (a conv's __deepcopy__ builds its copy on the host)
        twin.__dict__.pop('_folded', None)  # (inference caches of the original point at the original's layers)
        params = [p for p in twin.parameters() if p.requires_grad]
        if [p.shape for p in params] != [p.shape for p in self.flat.params]:
            raise RuntimeError('FlatEMA.shadow: the module is not the one this buffer was built from')
        for p, o in zip(params, self.flat.offsets):
            p.data = self.data[o:o + p.numel()].view(p.shape)
        for m in twin.modules():
            st = getattr(m, '_st', None)
            if isinstance(st, F.ConvState):
                st.model_epoch = self.pack_epoch
        return twin.eval()

    def state_dict(self, module: nn.Module) -> dict:
        """The averaged weights under ``module``'s own key names, on the CPU (a buffer, which has no average, as it is)."""
        where = self.flat.offsets_by_name(module)
        out = {}
        for k, v in module.state_dict().items():
            src = self.data[where[k]:where[k] + v.numel()].view(v.shape) if k in where else v
            out[k] = src.detach().clone().cpu()
        return out

    @torch.no_grad()
    def load_state_dict(self, module: nn.Module, sd) -> None:
        where = self.flat.offsets_by_name(module)
        shapes = {k: v.shape for k, v in module.named_parameters()}
        missing = sorted(set(where) - set(sd))
        if missing:
            raise RuntimeError(f'FlatEMA.load_state_dict: the averaged weights lack {missing[:4]} ...')
        for k, o in where.items():
            if tuple(sd[k].shape) != tuple(shapes[k]):
                raise RuntimeError(f'FlatEMA.load_state_dict: {k} has shape {tuple(sd[k].shape)}, expected {tuple(shapes[k])}')
            self.data[o:o + sd[k].numel()].copy_(sd[k].reshape(-1))
        self.pack_epoch[0] += 1


class StepLR:
    """torch.optim.lr_scheduler.StepLR(step_size, gamma) as used at torchsr/srgan/trainer.py:186-195.

    The reference passes ``step_size=epochs // 8``, which is 0 (ZeroDivisionError at the first
    ``step()``) for ``--epochs < 8``; here the step size is clamped to 1 instead.
    """

    def __init__(self, optimizer: FlatAdam, step_size: int, gamma: float = 0.1):
        self.optimizer, self.step_size, self.gamma = optimizer, max(1, int(step_size)), gamma
        self.base_lr = optimizer.lr
        self.last_epoch = 0

    def step(self) -> None:
        self.last_epoch += 1
        self.optimizer.set_lr(self.base_lr * self.gamma ** (self.last_epoch // self.step_size))

    def get_last_lr(self):
        return [self.optimizer.lr]

    def state_dict(self):
        return {'last_epoch': self.last_epoch, 'base_lr': self.base_lr}

    def load_state_dict(self, sd) -> None:
        self.last_epoch, self.base_lr = sd['last_epoch'], sd['base_lr']
        self.optimizer.set_lr(self.base_lr * self.gamma ** (self.last_epoch // self.step_size))
