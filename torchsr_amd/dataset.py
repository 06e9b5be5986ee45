"""Training / test data for the CLI -- contract of torchsr/dataset.py:364-428.

``initialize_datasets`` returns ``(train_loader, test_loader, train_len, test_len)``; train batches
are ``(low_res, high_res)``, test batches ``(low_res, bicubic, high_res)``, float NCHW in [0, 1].
The reference's PIL / torchvision / sklearn pipeline is CPU image I/O and outside the accelerated
hot path; this module restates its behaviour with PIL + torch only (random
crop, horizontal / vertical flips, PIL bicubic x1/4 which quantises LR to 8 bits, 90/10 split) and
adds a synthetic source (``train_dir='synthetic:N'``) used by smoke runs and benchmarks.
"""
import os
import random
from typing import List, Tuple

import torch
from torch.utils.data import DataLoader, Dataset
from torch.utils.data.distributed import DistributedSampler

from . import functional as F

SUPPORTED_IMAGES = ('.jpg', '.jpeg', '.png', '.bmp')  # dataset.py:29
# how DeviceLoader makes a low-resolution train batch ('Blind degradation' and 'Second-order degradation')
DEGRADATIONS = ('bicubic', 'blind', 'blind2')
BLIND2_KINDS = ('iso', 'aniso', 'generalized-iso', 'generalized-aniso', 'plateau-iso', 'plateau-aniso')
BLIND2_KIND_CDF = (0.45, 0.70, 0.82, 0.85, 0.97, 1.0)  # probabilities 0.45, 0.25, 0.12, 0.03, 0.12, 0.03
BLIND2_MODES = ('area', 'bilinear', 'bicubic')


def _image_dataset(directory: str) -> List[str]:
    """dataset.py:32-52."""
    return [os.path.join(directory, f) for f in sorted(os.listdir(directory)) if f.lower().endswith(SUPPORTED_IMAGES)]


class _Pairs(Dataset):
    def __init__(self, images, crop_size, upscale_factor, multiplier, test):
        self.images, self.crop, self.up, self.mult, self.test = images, crop_size, upscale_factor, multiplier, test

    def __len__(self):
        return len(self.images) * self.mult

    def __getitem__(self, index):
        import numpy as np
        from PIL import Image
        img = Image.open(self.images[index % len(self.images)]).convert('RGB')
        w, h = img.size
        if w < self.crop or h < self.crop:
            img = img.resize((max(w, self.crop), max(h, self.crop)), Image.BICUBIC)
            w, h = img.size
        x0, y0 = random.randint(0, w - self.crop), random.randint(0, h - self.crop)
        hr = img.crop((x0, y0, x0 + self.crop, y0 + self.crop))
        if not self.test:
            if random.random() < 0.5:
                hr = hr.transpose(Image.FLIP_LEFT_RIGHT)
            if random.random() < 0.5:
                hr = hr.transpose(Image.FLIP_TOP_BOTTOM)
        lr = hr.resize((self.crop // self.up, self.crop // self.up), Image.BICUBIC)
        to_t = lambda im: torch.from_numpy(np.asarray(im, dtype='float32') / 255.0).permute(2, 0, 1).contiguous()  # noqa: E731
        if self.test:
            return to_t(lr), to_t(lr.resize((self.crop, self.crop), Image.BICUBIC)), to_t(hr)
        return to_t(lr), to_t(hr)


class _Synthetic(Dataset):
    def __init__(self, n, crop_size, upscale_factor, test, seed):
        self.n, self.crop, self.up, self.test, self.seed = n, crop_size, upscale_factor, test, seed

    def __len__(self):
        return self.n

    def __getitem__(self, index):
        g = torch.Generator().manual_seed(self.seed * 1000003 + index)
        hr = torch.rand(3, self.crop, self.crop, generator=g)
        lr = torch.nn.functional.interpolate(hr[None], scale_factor=1 / self.up, mode='bicubic', antialias=True,
                                             align_corners=False).clamp(0, 1)[0]
        if self.test:
            bic = torch.nn.functional.interpolate(lr[None], scale_factor=self.up, mode='bicubic',
                                                  align_corners=False).clamp(0, 1)[0]
            return lr, bic, hr
        return lr, hr


def _needs_blind(what: str, why: str, degradation: str) -> None:
    if degradation not in ('blind', 'blind2'):
        raise ValueError(f'DeviceLoader: {what} needs degradation blind or blind2 ({why}), got {degradation!r}')


class DeviceLoader:
    """Train / test batches produced ON the MI355X.

    The reference runs RandomCrop + flips + PIL bicubic x1/4 in 16 DataLoader workers per GPU for every
    sample (dataset.py:88-99,121-125); at ~11 ms per batch-16 step that pipeline, not the GPU, sets the
    pace.  Here every image is decoded once, kept in HBM as uint8 HWC, and a batch is two kernels:
    ``srx_crop_flip_u8`` (crop + flips + ToTensor) and ``srx_bicubic_down`` (antialiased Keys bicubic, the
    filter PIL's BICUBIC and ``F.interpolate(..., antialias=True)`` use; LR rounded to 8 bits like the PIL
    image the reference converts back).  PIL's resampler also rounds its horizontal pass to 8 bits, so
    low-resolution pixels agree with the reference's to the last 8-bit step, not bit for bit.
    Same contract as the DataLoader it replaces: ``len()``, iteration yields ``(low_res, high_res)`` or
    ``(low_res, bicubic, high_res)`` float NCHW in [0, 1]; the last partial batch is dropped when training
    (fixed hipGraph shapes) and kept when testing.
    """

    def __init__(self, images, device, batch_size: int, crop_size: int, upscale_factor: int, test: bool, seed: int,
                 multiplier: int = 1, rank: int = 0, world_size: int = 1, gt_usm: bool = False, pair_pool: int = 0,
                 jpeg420_prob: float = 0.0, poisson_prob: float = 0.0, degradation: str = 'bicubic'):
        if degradation not in DEGRADATIONS:
            raise ValueError(f'DeviceLoader: degradation must be one of {DEGRADATIONS}, got {degradation!r}')
        if degradation in ('blind', 'blind2') and (crop_size <= 10 or crop_size % upscale_factor or (crop_size // upscale_factor) % 8):
            raise ValueError(f'DeviceLoader: blind degradation needs a crop of more than 10 pixels whose low-resolution side is '
                             f'a multiple of 8 (JPEG blocks), got crop {crop_size} / {upscale_factor}')
        if degradation == 'blind2':
            # the sizes _draw_degradation2 can draw: the final filter needs more than 10 low-resolution rows, and no resize may
            # reduce by more than 16:1 (functional.resize) -- the largest first size over the smallest second one
            lc = crop_size // upscale_factor
            s1_max, s2_min = 8 * int(1.5 * crop_size / 8 + 0.5), max(16, 8 * int(0.3 * lc / 8 + 0.5))
            if lc <= 10 or s1_max > 16 * s2_min:
                raise ValueError(f'DeviceLoader: blind2 degradation needs a low-resolution side of more than 10 pixels and resizes of '
                                 f'at most 16:1; crop {crop_size} / {upscale_factor} can draw {s1_max} -> {s2_min}')
        if not isinstance(gt_usm, bool):
            raise ValueError(f'DeviceLoader: gt_usm must be a bool, got {gt_usm!r}')
        if gt_usm and crop_size <= 25:
            raise ValueError(f'DeviceLoader: gt_usm needs a crop of more than 25 pixels (the 51-tap unsharp mask reflects 25), '
                             f'got crop {crop_size}')
        for name, prob, why in (('poisson_prob', poisson_prob, 'bicubic adds no noise'),
                                ('jpeg420_prob', jpeg420_prob, 'bicubic has no JPEG stage')):
            if isinstance(prob, bool) or not isinstance(prob, (int, float)) or not 0.0 <= prob <= 1.0:
                raise ValueError(f'DeviceLoader: {name} must be a number in [0, 1], got {prob!r}')
            if prob > 0:
                _needs_blind(name, why, degradation)
        if isinstance(pair_pool, bool) or not isinstance(pair_pool, int) or pair_pool < 0:
            raise ValueError(f'DeviceLoader: pair_pool must be a non-negative int (pairs in the pool; 0: off), got {pair_pool!r}')
        if pair_pool > 0:
            if test:
                raise ValueError('DeviceLoader: pair_pool is for train loaders (a test loader yields its own batches)')
            _needs_blind('pair_pool', 'bicubic batches share no drawn parameters to mix', degradation)
            if batch_size < 1 or pair_pool % batch_size:
                b = max(batch_size, 1)
                below, above = pair_pool // b * b, -(-pair_pool // b) * b
                raise ValueError(f'DeviceLoader: pair_pool must be a multiple of the batch size {batch_size} (every step takes a whole '
                                 f'batch out of a full pool), got {pair_pool}; the nearest are {below}{"" if below else " (off)"} and {above}')
        self.device, self.batch, self.crop, self.up, self.test = device, batch_size, crop_size, upscale_factor, test
        self.images = [self._fit(im).to(device) for im in images]          # uint8 [H][W][3]
        self.sizes = [(int(im.shape[0]), int(im.shape[1])) for im in self.images]
        self.order = [i for _ in range(multiplier) for i in range(len(self.images))]
        self.rank, self.world = rank, world_size
        self.rng = random.Random(seed * 7919 + rank)
        # ``blind`` / ``blind2`` train batches only: the degradation parameters and the noise seeds come from a stream of their own, so
        # the crop / flip stream above -- and with it every high-resolution batch -- is the same in both modes
        self.degradation = degradation
        # train batches only: the crop is unsharp-masked (functional.usm_sharpen, Real-ESRGAN's defaults) before it is yielded AND
        # before it is degraded; this draws from neither stream ('Sharpened targets')
        self.gt_usm = gt_usm
        self.deg_rng = random.Random(seed * 15485863 + rank + 982451653)
        # ``blind`` / ``blind2`` train batches with ``poisson_prob`` > 0 only: which samples get Poisson noise in place of the Gaussian
        # one, and its scale, come from a third stream, so the two above are what they were ('Poisson noise')
        self.poisson_prob = float(poisson_prob)
        self.poi_rng = random.Random(seed * 32452843 + rank + 472882027) if self.poisson_prob > 0 else None
        # train batches with ``pair_pool`` > 0 only: the pool's slots come from a fourth stream, so the three above produce exactly the
        # pairs they produce without a pool; only the order in which pairs reach the trainer changes ('Training pair pool')
        self.pair_pool = pair_pool
        self.pool_rng = random.Random(seed * 49979687 + rank + 715225739) if pair_pool > 0 else None
        # ``blind`` / ``blind2`` train batches with ``jpeg420_prob`` > 0 only: which samples of a JPEG stage are stored 4:2:0 comes from
        # a fifth stream, so the four above are what they were ('Chroma subsampling')
        self.jpeg420_prob = float(jpeg420_prob)
        self.j420_rng = random.Random(seed * 67867967 + rank + 236887691) if self.jpeg420_prob > 0 else None
        self.pool_lr = self.pool_hr = None     # [pair_pool, 3, crop / scale, crop / scale] and [pair_pool, 3, crop, crop], made at the first batch
        self.pool_filled = 0                   # pairs stored so far; the pool outlives the epochs
        self.last_degradation = None
        self.epoch = 0

    def _fit(self, im: torch.Tensor) -> torch.Tensor:
        """Images smaller than the crop are enlarged first (the reference's RandomCrop would raise)."""
        h, w = int(im.shape[0]), int(im.shape[1])
        if h >= self.crop and w >= self.crop:
            return im.contiguous()
        f = torch.nn.functional.interpolate(im.permute(2, 0, 1)[None].float(), size=(max(h, self.crop), max(w, self.crop)),
                                            mode='bicubic', align_corners=False)
        return f[0].permute(1, 2, 0).clamp(0, 255).round().to(torch.uint8).contiguous()

    def _shard(self, order):
        """This rank's samples: what ``DistributedSampler`` hands out (dataset.py:279,343-360) -- the order padded to a
        multiple of the world size by wrapping around, then every world-th sample -- so that every rank holds the
        same number of samples (none is empty, none runs an extra batch and waits in a collective alone)."""
        if self.world > 1 and len(order) % self.world:
            pad = self.world - len(order) % self.world
            order = order + (order * (-(-pad // len(order))))[:pad]
        return order[self.rank::self.world]

    def __len__(self) -> int:
        n = -(-len(self.order) // self.world)  # the same on every rank
        # the reference's train loader drops nothing either (dataset.py:280-293), but a replayed hipGraph needs
        # one batch shape, so the last partial TRAIN batch is dropped; the eager test pass keeps it (:345-360)
        return -(-n // self.batch) if self.test else n // self.batch

    def _draw_meta(self, idx):
        """``srx_crop_flip_u8``'s rows {H, W, top, left, hflip, vflip} of the samples ``idx``, drawn from the crop / flip stream."""
        meta = []
        for i in idx:
            h, w = self.sizes[i]
            top, left = self.rng.randint(0, h - self.crop), self.rng.randint(0, w - self.crop)
            hflip = 0 if self.test else int(self.rng.random() < 0.5)
            vflip = 0 if self.test else int(self.rng.random() < 0.5)
            meta.append([h, w, top, left, hflip, vflip])
        return meta

    def _draw_degradation(self, n: int) -> dict:
        """The ``blind`` parameters of a batch of ``n`` samples, drawn on the host from the degradation stream: the first-order
        recipe of Real-ESRGAN without its sinc branch (its Poisson branch: ``_draw_poisson``).  Numpy arrays, laid out as the kernels read them:
        ``parm`` float32 [n][4] = {sigma_x, sigma_y, theta, 0}, ``ksize`` int32 [n], ``sigma_n`` float32 [n], ``gray`` int32 [n],
        ``quality`` int32 [n]; and ``seed``, the batch's 64-bit noise seed."""
        import math
        import numpy as np
        rng = self.deg_rng
        parm, ksize = np.zeros((n, 4), dtype=np.float32), np.zeros(n, dtype=np.int32)
        sigma_n, gray, quality = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        for i in range(n):
            ksize[i] = 2 * rng.randint(3, 10) + 1                       # odd, 7 .. 21
            if rng.random() < 0.5:                                      # isotropic
                sx = sy = rng.uniform(0.2, 3.0)
                theta = 0.0
            else:
                sx, sy = rng.uniform(0.2, 3.0), rng.uniform(0.2, 3.0)
                theta = -math.pi + 2.0 * math.pi * rng.random()         # [-pi, pi)
            parm[i, :3] = sx, sy, theta
            sigma_n[i] = rng.uniform(1.0, 30.0) / 255.0
            gray[i] = int(rng.random() < 0.4)
            quality[i] = rng.randint(30, 95)
        return {'parm': parm, 'ksize': ksize, 'sigma_n': sigma_n, 'gray': gray, 'quality': quality, 'seed': rng.getrandbits(64)}

    def _draw_kernel(self, sigma_hi: float):
        """One blur kernel of the second-order recipe from the degradation stream: ``(kind, ksize, weights)``, the weights
        float64 [ksize][ksize].  Draw order: the size; one uniform (< 0.1: sinc, then its cutoff); else one uniform for the
        kind, then sigma_x, for the anisotropic kinds sigma_y and theta, for the generalised and plateau kinds beta."""
        import math
        from .degradation import kernel_weights
        rng = self.deg_rng
        ks = 2 * rng.randint(3, 10) + 1                                 # odd, 7 .. 21
        if rng.random() < 0.1:
            omega = rng.uniform(math.pi / 3 if ks < 13 else math.pi / 5, math.pi)
            return 'sinc', ks, kernel_weights('sinc', ks, omega_c=omega)
        u = rng.random()
        kind = BLIND2_KINDS[next(i for i, c in enumerate(BLIND2_KIND_CDF) if u < c)]
        sx = sy = rng.uniform(0.2, sigma_hi)
        theta = 0.0
        if kind.endswith('aniso'):
            sy = rng.uniform(0.2, sigma_hi)
            theta = -math.pi + 2.0 * math.pi * rng.random()             # [-pi, pi)
        if kind.startswith('generalized'):
            return kind, ks, kernel_weights('generalized', ks, sx, sy, theta, beta=rng.uniform(0.5, 4.0))
        if kind.startswith('plateau'):
            return kind, ks, kernel_weights('plateau', ks, sx, sy, theta, beta=rng.uniform(1.0, 2.0))
        return kind, ks, kernel_weights('gauss', ks, sx, sy, theta)

    def _draw_degradation2(self, n: int) -> dict:
        """The ``blind2`` parameters of a batch of ``n`` samples, drawn on the host from the degradation stream: the second-order
        recipe of Real-ESRGAN (x4plus options); its Poisson branch is ``_draw_poisson``.  One fixed order.  Per BATCH first, so that the
        batch stays rectangular: the first resize (one uniform for up / down / keep, the factor unless kept, the mode), the
        second resize likewise, the final resize's mode, the final order.  Then per SAMPLE: the first kernel
        (``_draw_kernel(3.0)``), sigma, grey flag and JPEG quality of the first pass; one uniform (< 0.2: no second blur), else
        the second kernel (``_draw_kernel(1.5)``); sigma and grey flag of the second pass; one uniform (< 0.8: the final sinc,
        then its size and cutoff, else the pulse); the final JPEG quality.  Last the two 64-bit noise seeds.

        Numpy arrays, laid out as the kernels read them: ``weights`` float32 [3][n][21][21] (K1, K2, K3 of ``srx_filter2d``),
        ``ksize`` int32 [3][n] (0: no filter), ``sigma_n`` float32 [2][n], ``gray`` int32 [2][n], ``quality`` int32 [2][n]; and
        ``sizes`` (S1, S2, crop / scale), ``modes`` (three of ``BLIND2_MODES``), ``order`` ('A' or 'B'), ``seed1``, ``seed2``,
        ``kinds`` (three lists of names, what each kernel is)."""
        import math
        import numpy as np
        from .degradation import KERNEL_SLOT, kernel_slot, kernel_weights
        rng = self.deg_rng
        lc = self.crop // self.up

        def factor(p_up, p_down, up_hi, down_lo):
            u = rng.random()
            if u < p_up:
                return rng.uniform(1.0, up_hi)
            return rng.uniform(down_lo, 1.0) if u < p_up + p_down else 1.0

        s1 = factor(0.2, 0.7, 1.5, 0.15)
        mode1 = BLIND2_MODES[rng.randrange(3)]
        s2 = factor(0.3, 0.4, 1.2, 0.3)
        mode2 = BLIND2_MODES[rng.randrange(3)]
        mode3 = BLIND2_MODES[rng.randrange(3)]
        order = 'A' if rng.random() < 0.5 else 'B'
        # multiples of 8: srx_jpeg_sim takes whole blocks (Real-ESRGAN pads instead)
        sizes = (max(16, 8 * int(self.crop * s1 / 8 + 0.5)), max(16, 8 * int(lc * s2 / 8 + 0.5)), lc)
        weights, ksize = np.zeros((3, n, KERNEL_SLOT, KERNEL_SLOT), dtype=np.float32), np.zeros((3, n), dtype=np.int32)
        sigma_n, gray, quality = np.zeros((2, n), dtype=np.float32), np.zeros((2, n), dtype=np.int32), np.zeros((2, n), dtype=np.int32)
        kinds = [[], [], []]

        def put(stage, i, kind, ks, w):
            kinds[stage].append(kind)
            ksize[stage, i] = ks
            kernel_slot(w, out=weights[stage, i])

        for i in range(n):
            put(0, i, *self._draw_kernel(3.0))
            sigma_n[0, i] = rng.uniform(1.0, 30.0) / 255.0
            gray[0, i] = int(rng.random() < 0.4)
            quality[0, i] = rng.randint(30, 95)
            if rng.random() < 0.2:
                put(1, i, 'skip', 0, None)
            else:
                put(1, i, *self._draw_kernel(1.5))
            sigma_n[1, i] = rng.uniform(1.0, 25.0) / 255.0
            gray[1, i] = int(rng.random() < 0.4)
            if rng.random() < 0.8:
                ks = 2 * rng.randint(3, 10) + 1
                put(2, i, 'sinc', ks, kernel_weights('sinc', ks, omega_c=rng.uniform(math.pi / 3, math.pi)))
            else:
                put(2, i, 'pulse', 0, None)
            quality[1, i] = rng.randint(30, 95)
        return {'weights': weights, 'ksize': ksize, 'sigma_n': sigma_n, 'gray': gray, 'quality': quality, 'sizes': sizes,
                'modes': (mode1, mode2, mode3), 'order': order, 'seed1': rng.getrandbits(64), 'seed2': rng.getrandbits(64),
                'kinds': kinds}

    def _draw_poisson(self, deg: dict) -> dict:
        """The Poisson branch of a drawn batch, from the Poisson stream; ``deg`` is changed in place and returned.  One fixed order:
        per SAMPLE, per noise STAGE of the recipe (one for ``blind``, two for ``blind2``): one uniform (< ``poisson_prob``: Poisson),
        then the scale -- ``uniform(0.05, 3.0)`` in the first stage, ``uniform(0.05, 2.5)`` in the second -- which is drawn whether or
        not Poisson was chosen, so the stream's position depends on no outcome.  ``deg`` gains ``poisson_scale``, float32 shaped like
        ``sigma_n``: the scale where Poisson was chosen, else 0; there ``sigma_n`` becomes 0."""
        import numpy as np
        rng, sigma_n = self.poi_rng, deg['sigma_n']
        scale = np.zeros(sigma_n.shape, dtype=np.float32)
        sig, sc = sigma_n.reshape(-1, sigma_n.shape[-1]), scale.reshape(-1, sigma_n.shape[-1])   # views: [stages][n]
        for i in range(sig.shape[1]):
            for stage in range(sig.shape[0]):
                chosen = rng.random() < self.poisson_prob
                s = rng.uniform(0.05, 3.0 if stage == 0 else 2.5)
                if chosen:
                    sc[stage, i], sig[stage, i] = s, 0.0
        deg['poisson_scale'] = scale
        return deg

    def _draw_jpeg420(self, deg: dict) -> dict:
        """The chroma subsampling of a drawn batch, from its own stream; ``deg`` is changed in place and returned.  Per SAMPLE, per
        JPEG STAGE of the recipe (one for ``blind``, two for ``blind2``): one uniform (< ``jpeg420_prob``: 4:2:0), drawn whether or not
        the stage's quality is a JPEG quality, so the stream's position depends on no outcome.  ``deg`` gains ``chroma420``, int32
        shaped like ``quality``: 1 where 4:2:0 was chosen, else 0."""
        import numpy as np
        rng, quality = self.j420_rng, deg['quality']
        flags = np.zeros(quality.shape, dtype=np.int32)
        fl = flags.reshape(-1, quality.shape[-1])   # a view: [stages][n]
        for i in range(fl.shape[1]):
            for stage in range(fl.shape[0]):
                fl[stage, i] = int(rng.random() < self.jpeg420_prob)
        deg['chroma420'] = flags
        return deg

    def _draw_pool_slots(self):
        """The pool's part of the next train batch: ``(slots, mode)`` for ``srx_pool_exchange``.  While the pool fills -- its first
        ``pair_pool / batch`` batches -- the next free slots in order and mode 0 (store: the batch is yielded as generated, what
        basicsr does until its queue is full), with no draw; from then on ``batch`` distinct uniform slots from the pool stream
        and mode 1 (exchange).  Real-ESRGAN shuffles its pool, takes the first ``batch`` pairs and puts the new ones in their
        place: the same distribution of what is dequeued, without moving the other pairs."""
        if self.pool_filled < self.pair_pool:
            slots = list(range(self.pool_filled, self.pool_filled + self.batch))
            self.pool_filled += self.batch
            return slots, 0
        return self.pool_rng.sample(range(self.pair_pool), self.batch), 1

    def _pool(self, lr, hr):
        """A generated train batch through the pair pool: stored (while the pool fills) or exchanged in place for ``batch`` pooled
        pairs; returns ``(lr, hr)``, the tensors it was given.  The pool tensors are made at the first batch."""
        if self.pool_lr is None:
            self.pool_lr = torch.empty((self.pair_pool,) + tuple(lr.shape[1:]), dtype=torch.float32, device=lr.device)
            self.pool_hr = torch.empty((self.pair_pool,) + tuple(hr.shape[1:]), dtype=torch.float32, device=hr.device)
        slots, mode = self._draw_pool_slots()
        with torch.no_grad():
            return F.pool_exchange(self.pool_lr, self.pool_hr, lr, hr, slots, exchange=bool(mode))

    def _plan(self):
        """Host side of one epoch: per batch the sample indices, the crop / flip rows and -- ``blind`` and ``blind2`` train batches
        only, and after the rows, from the other stream -- the degradation parameters (else None); with ``poisson_prob`` > 0 their
        Poisson branch after them, from the third; with ``jpeg420_prob`` > 0 their chroma subsampling last, from the fifth."""
        order = list(self.order)
        if not self.test:
            random.Random(self.epoch * 104729 + 17).shuffle(order)  # same permutation on every rank
        self.epoch += 1
        order = self._shard(order)
        for b in range(len(self)):
            idx = order[b * self.batch:(b + 1) * self.batch]
            meta = self._draw_meta(idx)
            blind = self.degradation == 'blind' and not self.test   # the test set stays bicubic: PSNR comparable across runs
            blind2 = self.degradation == 'blind2' and not self.test
            deg = self._draw_degradation(len(idx)) if blind else self._draw_degradation2(len(idx)) if blind2 else None
            if deg is not None and self.poi_rng is not None:
                deg = self._draw_poisson(deg)
            if deg is not None and self.j420_rng is not None:
                deg = self._draw_jpeg420(deg)
            yield idx, meta, deg

    def _upload(self, deg, keys):
        """The drawn tables of a batch on the device, shaped as drawn, in as few copies as the batch allows: one per key of ``keys``;
        ``quality`` with the 4:2:0 flags riding in its copy -- ``chroma420`` is None, and the batch then takes ``srx_jpeg_sim`` as a
        loader without ``jpeg420_prob`` does, unless a sample drew 4:2:0; ``poisson_scale``, every stage in one copy, only when a
        sample drew Poisson (else None)."""
        import numpy as np
        dev = self.device
        t = {k: torch.from_numpy(deg[k]).to(dev) for k in keys}
        flags, scale = deg.get('chroma420'), deg.get('poisson_scale')
        if flags is None or not flags.any():
            t['quality'], t['chroma420'] = torch.from_numpy(deg['quality']).to(dev), None
        else:
            t['quality'], t['chroma420'] = torch.from_numpy(np.stack([deg['quality'], flags])).to(dev)
        t['poisson_scale'] = torch.from_numpy(scale).to(dev) if scale is not None and scale.any() else None
        return t

    def _noise(self, x, deg, t, seed, stage=None):
        """One noise stage, 8-bit result (``stage``: its row in the tables; None: they have one stage).  ``F.add_poisson_noise``,
        unquantised, on the samples that drew it -- nothing is launched unless a sample of THIS stage did -- then
        ``F.add_gaussian_noise``, which adds exactly 0 to those samples (their sigma is 0) and rounds all to 8 bits."""
        at = (lambda a: a) if stage is None else (lambda a: a[stage])
        gray = at(t['gray'])
        if t['poisson_scale'] is not None and at(deg['poisson_scale']).any():
            x = F.add_poisson_noise(x, at(t['poisson_scale']), gray, seed)[0]
        return F.add_gaussian_noise(x, at(t['sigma_n']), gray, seed)

    def _degrade(self, hr, deg):
        """``blind``: blur -> bicubic x1/scale (unquantised) -> Poisson or Gaussian noise -> 8 bits -> JPEG -> 8 bits."""
        t = self._upload(deg, ('parm', 'ksize', 'sigma_n', 'gray'))
        lr = F.bicubic_down(F.blur_aniso(hr, t['parm'], t['ksize']), self.up, False)
        return F.jpeg_sim(self._noise(lr, deg, t, deg['seed']), t['quality'], t['chroma420'])

    def _degrade2(self, hr, deg):
        """``blind2``: filter -> resize -> noise -> JPEG, twice, the second JPEG and the final sinc filter around the resize to
        the low-resolution size in either order ('Second-order degradation')."""
        t = self._upload(deg, ('weights', 'ksize', 'sigma_n', 'gray'))  # the three weight tables in one copy
        (s1, s2, lc), modes = deg['sizes'], deg['modes']

        def filt(x, stage, quantize):
            return F.filter2d(x, t['weights'][stage], t['ksize'][stage], quantize)

        def jpeg(x, stage):
            return F.jpeg_sim(x, t['quality'][stage], None if t['chroma420'] is None else t['chroma420'][stage])

        with torch.no_grad():
            x = jpeg(self._noise(F.resize(filt(hr, 0, False), (s1, s1), modes[0]), deg, t, deg['seed1'], 0), 0)
            x = self._noise(F.resize(filt(x, 1, False), (s2, s2), modes[1]), deg, t, deg['seed2'], 1)
            if deg['order'] == 'A':
                return jpeg(filt(F.resize(x, (lc, lc), modes[2]), 2, False), 1)
            return filt(F.resize(jpeg(x, 1), (lc, lc), modes[2]), 2, True)

    def __iter__(self):
        for idx, meta, deg in self._plan():
            hr = F.crop_flip([self.images[i] for i in idx], meta, self.crop)
            if self.gt_usm and not self.test:
                with torch.no_grad():
                    hr = F.usm_sharpen(hr)
            if deg is not None:
                self.last_degradation = deg
                lr = (self._degrade2 if self.degradation == 'blind2' else self._degrade)(hr, deg)
                yield self._pool(lr, hr) if self.pair_pool else (lr, hr)
                continue
            lr = F.bicubic_down(hr, self.up, True)
            if self.test:  # the bicubic up-sampled image of TestData (dataset.py:175-190): only ever displayed
                bic = torch.nn.functional.interpolate(lr, size=(self.crop, self.crop), mode='bicubic',
                                                      align_corners=False).clamp(0, 1)
                yield lr, bic, hr
            else:
                yield lr, hr


def _decode(path: str) -> torch.Tensor:
    import numpy as np
    from PIL import Image
    return torch.from_numpy(np.asarray(Image.open(path).convert('RGB'), dtype='uint8').copy())


def initialize_device_datasets(train_directory: str, device, batch_size: int = 64, crop_size: int = 96,
                               upscale_factor: int = 4, dataset_multiplier: int = 1, distributed: bool = False,
                               seed: int = 0, rank: int = 0, world_size: int = 1, gt_usm: bool = False, pair_pool: int = 0,
                               jpeg420_prob: float = 0.0, poisson_prob: float = 0.0, degradation: str = 'bicubic'):
    """``initialize_datasets`` with the augmentation on the device (``--device-data``).  ``synthetic:N`` draws N
    seeded random 2*crop x 2*crop images.  ``degradation='blind'`` degrades the TRAIN batches' low-resolution side with blur,
    noise and JPEG (``--degradation``), ``'blind2'`` with the second-order recipe; ``gt_usm`` unsharp-masks the TRAIN batches'
    high-resolution crop, which is then both the target and what is degraded (``--gt-usm``); ``poisson_prob`` gives each sample of
    each noise stage of ``blind`` / ``blind2`` Poisson noise with that probability in place of the Gaussian one
    (``--poisson-noise-prob``); ``jpeg420_prob`` stores each sample of each JPEG stage of ``blind`` / ``blind2`` with 4:2:0 chroma
    subsampling with that probability (``--jpeg-420-prob``); ``pair_pool`` > 0 sends the TRAIN batches through a pool of that many pairs, so that a step sees
    pairs of several generated batches (``--pair-pool``); the test loader stays bicubic and unsharpened and never has a pool."""
    if train_directory.startswith('synthetic:'):
        n = int(train_directory.split(':')[1])
        g = torch.Generator().manual_seed(seed)
        images = [torch.randint(0, 256, (2 * crop_size, 2 * crop_size, 3), generator=g, dtype=torch.uint8)
                  for _ in range(n + max(1, n // 10))]
    else:
        paths = _image_dataset(train_directory)
        if not paths:
            raise RuntimeError(f'no images ({", ".join(SUPPORTED_IMAGES)}) found in {train_directory}')
        random.Random(seed or None).shuffle(paths)
        images = [_decode(p) for p in paths]
    n_test = max(1, len(images) // 10)
    if not distributed:
        rank, world_size = 0, 1
    train = DeviceLoader(images[n_test:] or images, device, batch_size, crop_size, upscale_factor, False, seed,
                         dataset_multiplier, rank, world_size, degradation=degradation, gt_usm=gt_usm, poisson_prob=poisson_prob,
                         pair_pool=pair_pool, jpeg420_prob=jpeg420_prob)
    # dataset.py:343-360: the test set is multiplied like the train set, sharded over the ranks, nothing dropped
    test = DeviceLoader(images[:n_test], device, batch_size, crop_size, upscale_factor, True, seed + 1,
                        dataset_multiplier, rank, world_size)
    return train, test, len(train.order), len(test.order)


def initialize_datasets(train_directory: str, batch_size: int = 64, crop_size: int = 96, upscale_factor: int = 4,
                        dataset_multiplier: int = 1, workers: int = 16, distributed: bool = False,
                        seed: int = 0) -> Tuple[DataLoader, DataLoader, int, int]:
    """dataset.py:364-428."""
    if train_directory.startswith('synthetic:'):
        n = int(train_directory.split(':')[1])
        n_test = max(1, n // 10)
        train = _Synthetic(n, crop_size, upscale_factor, False, seed)
        test = _Synthetic(n_test, crop_size, upscale_factor, True, seed + 1)
        workers = 0
    else:
        images = _image_dataset(train_directory)
        if not images:
            raise RuntimeError(f'no images ({", ".join(SUPPORTED_IMAGES)}) found in {train_directory}')
        rng = random.Random(seed or None)
        rng.shuffle(images)
        n_test = max(1, len(images) // 10)  # sklearn train_test_split(test_size=0.1), dataset.py:412
        train = _Pairs(images[n_test:] or images, crop_size, upscale_factor, dataset_multiplier, False)
        test = _Pairs(images[:n_test], crop_size, upscale_factor, dataset_multiplier, True)  # dataset.py:343-345

    def loader(ds, shuffle, drop_last):
        sampler = DistributedSampler(ds, seed=seed, shuffle=shuffle) if distributed else None
        return DataLoader(ds, batch_size=batch_size, shuffle=shuffle and sampler is None, sampler=sampler,
                          num_workers=workers, drop_last=drop_last, pin_memory=True,
                          persistent_workers=distributed and workers > 0)

    # train: the replayed hipGraph needs one batch shape, so the last partial batch is dropped; test: eager, and the
    # reference's test loader drops nothing (dataset.py:345-360) -- a shard smaller than --batch-size still gets tested
    return loader(train, True, True), loader(test, False, False), len(train), len(test)
