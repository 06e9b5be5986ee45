"""A torch CPU restatement of Real-ESRGAN's ``UNetDiscriminatorSN``, written from its architecture description:

    conv0 3x3 (3 -> F, bias) | SN conv1..3 4x4 s2 p1 (F -> 2F -> 4F -> 8F) | bilinear x2 + SN conv4 3x3 (+ x2) |
    bilinear x2 + SN conv5 (+ x1) | bilinear x2 + SN conv6 (+ x0) | SN conv7, conv8 3x3 | conv9 3x3 (F -> 1, bias)

LeakyReLU(0.2) behind every conv but the last; the skips are added behind the activation.  Stock ``torch.nn``,
``torch.nn.utils.spectral_norm`` and ``F.interpolate`` only, so it runs in fp32 and, after ``.double()``, in fp64: the tests'
reference and the measure of fp32's own distance from fp64.  Also the closed forms the kernels implement, in numpy, and a
restatement of the GAN losses.
"""
import numpy as np
import torch
import torch.nn.functional as TF
from torch import nn
from torch.nn.utils import spectral_norm


class UNetRef(nn.Module):
    def __init__(self, num_in_ch: int = 3, num_feat: int = 64, skip_connection: bool = True):
        super().__init__()
        self.skip_connection = skip_connection
        f = num_feat
        self.conv0 = nn.Conv2d(num_in_ch, f, 3, 1, 1)
        self.conv1 = spectral_norm(nn.Conv2d(f, f * 2, 4, 2, 1, bias=False))
        self.conv2 = spectral_norm(nn.Conv2d(f * 2, f * 4, 4, 2, 1, bias=False))
        self.conv3 = spectral_norm(nn.Conv2d(f * 4, f * 8, 4, 2, 1, bias=False))
        self.conv4 = spectral_norm(nn.Conv2d(f * 8, f * 4, 3, 1, 1, bias=False))
        self.conv5 = spectral_norm(nn.Conv2d(f * 4, f * 2, 3, 1, 1, bias=False))
        self.conv6 = spectral_norm(nn.Conv2d(f * 2, f, 3, 1, 1, bias=False))
        self.conv7 = spectral_norm(nn.Conv2d(f, f, 3, 1, 1, bias=False))
        self.conv8 = spectral_norm(nn.Conv2d(f, f, 3, 1, 1, bias=False))
        self.conv9 = nn.Conv2d(f, 1, 3, 1, 1)

    def forward(self, x):
        act = lambda t: TF.leaky_relu(t, 0.2)  # noqa: E731
        up = lambda t: TF.interpolate(t, scale_factor=2, mode='bilinear', align_corners=False)  # noqa: E731
        x0 = act(self.conv0(x))
        x1 = act(self.conv1(x0))
        x2 = act(self.conv2(x1))
        x3 = act(self.conv3(x2))
        x4 = act(self.conv4(up(x3)))
        if self.skip_connection:
            x4 = x4 + x2
        x5 = act(self.conv5(up(x4)))
        if self.skip_connection:
            x5 = x5 + x1
        x6 = act(self.conv6(up(x5)))
        if self.skip_connection:
            x6 = x6 + x0
        out = act(self.conv7(x6))
        out = act(self.conv8(out))
        return self.conv9(out)


def seeded_state(ref: nn.Module, seed: int = 0):
    """Conv weights at He scale (LeakyReLU 0.2), small biases, ``u`` a seeded unit vector and ``v = normalize(W^T u)`` -- the
    state ``spectral_norm`` itself starts from, with every value a function of ``seed``."""
    g = torch.Generator().manual_seed(seed)
    sd, base = {}, ref.state_dict()
    for k, v in base.items():
        if v.dim() == 4:
            sd[k] = torch.randn(v.shape, generator=g) * (2.0 / (1.04 * v.shape[1] * v.shape[2] * v.shape[3])) ** 0.5
        elif k.endswith('.bias'):
            sd[k] = (torch.rand(v.shape, generator=g) - 0.5) * 0.2
    for k, v in base.items():
        if k.endswith('.weight_u'):
            w = sd[k[:-2] + '_orig']
            u = TF.normalize(torch.randn(v.shape, generator=g), dim=0, eps=1e-12)
            sd[k] = u
            sd[k[:-2] + '_v'] = TF.normalize(w.reshape(w.shape[0], -1).t().mv(u), dim=0, eps=1e-12)
    return {k: sd[k] for k in base}


# ---- the closed forms of csrc/specnorm.hip, in numpy (any float dtype)
def sn_forward(w, u, v, train: bool, eps: float = 1e-12):
    """``(w_sn, sigma, u, v)`` of one ``spectral_norm`` forward on the matrix ``w`` [rows, cols]."""
    if train:
        t = w.T @ u
        v = t / max(np.linalg.norm(t), eps)
        s = w @ v
        u = s / max(np.linalg.norm(s), eps)
    sigma = u @ (w @ v)
    return w / sigma, sigma, u, v


def sn_backward(g, w_sn, u, v, sigma):
    """``dL/dW`` from ``g = dL/dW_sn``: ``(G - <G, W_sn> u v^T) / sigma`` (u, v: constants of the forward)."""
    return (g - (g * w_sn).sum() * np.outer(u, v)) / sigma


# ---- bilinear x2, align_corners=False: the forward table of one axis and, as its transpose, the backward
def bilinear2x_table(n: int, dtype=np.float64):
    """``T`` [2n, n]: output o = 2 i + p takes 0.75 of input i and 0.25 of i - 1 (p = 0) / i + 1 (p = 1), clamped."""
    t = np.zeros((2 * n, n), dtype=dtype)
    for o in range(2 * n):
        i = o // 2
        j = min(max(i + (1 if o % 2 else -1), 0), n - 1)
        t[o, i] += 0.75
        t[o, j] += 0.25
    return t


def bilinear2x_forward(x):
    """x: [N, C, H, W] numpy."""
    th, tw = bilinear2x_table(x.shape[2], x.dtype), bilinear2x_table(x.shape[3], x.dtype)
    return np.einsum('oh,nchw,pw->ncop', th, x, tw)


def bilinear2x_backward(dy):
    """dy: [N, C, 2H, 2W] numpy -> [N, C, H, W]: the transposed tables."""
    th, tw = bilinear2x_table(dy.shape[2] // 2, dy.dtype), bilinear2x_table(dy.shape[3] // 2, dy.dtype)
    return np.einsum('oh,ncop,pw->nchw', th, dy, tw)


# ---- the losses the trainer forms with this discriminator
def pair_loss(ref: nn.Module, real, fake):
    """``BCEWithLogits(D(real), 1) + BCEWithLogits(D(fake), 0)`` from ONE forward of the 2N batch (one power iteration)."""
    out = ref(torch.cat([real, fake], dim=0))
    n = real.shape[0]
    return (TF.binary_cross_entropy_with_logits(out[:n], torch.ones_like(out[:n]))
            + TF.binary_cross_entropy_with_logits(out[n:], torch.zeros_like(out[n:])))


def adversarial_loss(ref: nn.Module, fake, addend, weight: float):
    out = ref(fake)
    return addend + weight * TF.binary_cross_entropy_with_logits(out, torch.ones_like(out))


# ---- the GAN step of ``train --discriminator unet``: D first, then G against the updated D
class StateModel(nn.Module):
    """A functional forward ``fn(state, x)`` (the oracle's generators) over trainable copies of ``state``'s tensors."""

    def __init__(self, state, fn):
        super().__init__()
        self.names = list(state)
        self.values = nn.ParameterList([nn.Parameter(v.detach().clone()) for v in state.values()])
        self.fn = fn

    def state(self):
        return {k: p.detach() for k, p in zip(self.names, self.values)}

    def forward(self, x):
        return self.fn(dict(zip(self.names, self.values)), x)


class GanStepRef:
    """One step: ``sr = G(lr)``; ``disc_loss = BCE(D(hr), 1) + BCE(D(sr), 0)`` from ONE training-mode forward of the 2N batch, D
    backward, D Adam; then ``gen_loss = 0.01 L1(sr, hr) + content(sr, hr) + 0.1 BCE(D(sr), 1)`` from a second training-mode
    forward of the UPDATED D (its second power iteration of the step), G backward, G Adam.  Adam(lr 1e-4, (0.9, 0.999), 1e-8)."""

    def __init__(self, gen: nn.Module, disc: nn.Module, content_loss, adv_weight: float = 0.1):
        self.gen, self.disc, self.content_loss, self.adv_weight = gen.train(), disc.train(), content_loss, adv_weight
        self.gen_opt = torch.optim.Adam(gen.parameters(), lr=1e-4, betas=(0.9, 0.999), eps=1e-8)
        self.disc_opt = torch.optim.Adam(disc.parameters(), lr=1e-4, betas=(0.9, 0.999), eps=1e-8)

    def step(self, low, high):
        self.disc_opt.zero_grad()
        sr = self.gen(low)
        disc_loss = pair_loss(self.disc, high, sr.detach())
        disc_loss.backward()
        self.disc_opt.step()
        self.gen_opt.zero_grad()
        pixel, content = TF.l1_loss(sr, high), self.content_loss(sr, high)
        out = self.disc(sr)
        adv = TF.binary_cross_entropy_with_logits(out, torch.ones_like(out))
        gen_loss = 0.01 * pixel + content + self.adv_weight * adv
        gen_loss.backward()
        self.gen_opt.step()
        return {'gan/disc-loss': disc_loss.detach(), 'gan/pixel-loss': pixel.detach(), 'gan/content-loss': content.detach(),
                'gan/adversarial-loss': adv.detach(), 'gan/train-loss': gen_loss.detach()}
