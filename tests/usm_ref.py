"""Float64 restatement of ``srx_usm_sharpen`` (Real-ESRGAN's ``USMSharp.forward``) and the images its tests run on.  Torch on
the CPU only: reflect pad plus ``conv2d`` with ``g (x) g``, and the formula of DESIGN.md, 'Sharpened targets'."""
import numpy as np
import torch

import degrade_ref as R


def taps64(ksize: int, sigma: float) -> np.ndarray:
    """g[i] ~ exp(-(i - r)^2 / (2 sigma^2)), r = ksize // 2, sum 1, float64."""
    d = np.arange(ksize, dtype=np.float64) - ksize // 2
    g = np.exp(-(d * d) / (2.0 * sigma * sigma))
    return g / g.sum()


def gauss(x, g) -> torch.Tensor:
    """G(x): every plane of NCHW ``x`` correlated with g (x) g in float64, borders reflected without repeating the edge."""
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64)
    g = torch.as_tensor(np.asarray(g), dtype=torch.float64)
    n, c, h, w = x.shape
    k, r = g.numel(), g.numel() // 2
    p = torch.nn.functional.pad(x.reshape(n * c, 1, h, w), (r, r, r, r), mode='reflect')
    return torch.nn.functional.conv2d(p, torch.outer(g, g).reshape(1, 1, k, k)).reshape(n, c, h, w)


def blend(x, blur, mask, g, weight: float) -> torch.Tensor:
    """The last three lines of the formula from a given blur and mask: soft = G(mask), sharp, out."""
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64)
    blur = torch.as_tensor(np.asarray(blur), dtype=torch.float64)
    soft = gauss(mask, g)
    sharp = (x + weight * (x - blur)).clamp(0, 1)
    return x + soft * (sharp - x)


def usm(x, g, weight: float, threshold: float):
    """``(out, blur, mask, t)`` in float64; ``t = |x - blur| * 255`` is what the mask compares with ``threshold``."""
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64)
    blur = gauss(x, g)
    t = (x - blur).abs() * 255
    mask = (t > threshold).to(torch.float64)
    return blend(x, blur, mask, g, weight), blur, mask, t


def images(n: int, h: int, w: int) -> np.ndarray:
    """The test images, float32 [n][3][h][w], 8-bit valued: ``degrade_ref.jpeg_images(n, h, w, 7)`` with the region
    [:, :, h // 3:, w // 2:] flattened by v -> 0.3 v + 0.6, so that the mask holds both values in quantity."""
    img = R.jpeg_images(n, h, w, 7).astype(np.float64)
    img[:, :, h // 3:, w // 2:] = 0.3 * img[:, :, h // 3:, w // 2:] + 0.6
    return (np.rint(np.clip(img, 0, 1) * 255) / 255).astype(np.float32)
