"""The judge of the multi-scale resize (ly_resize_u8), shared by tests/test_multiscale_host.py and tests/test_gpu_multiscale.py:
float64 bilinear interpolation of p / 255 with the half-pixel formula of F.interpolate(mode='bilinear', align_corners=False),

    scale = in / out,  src = max(scale * (dst + 0.5) - 0.5, 0),  i0 = floor(src),  i1 = i0 + (i0 < in - 1),  w1 = src - i0,  w0 = 1 - w1,

and the bound an fp32 evaluation must keep to it.  Not fp32 F.interpolate: near coordinate 640 an fp32 result depends on how
`scale * (dst + 0.5) - 0.5` is rounded (ATen and a literal fp32 restatement differ by up to 2.8e-5 at 640 -> 960), and both lie at the
same distance from this one.

The bound.  The source coordinate takes at most about 2 fp32 roundings at a magnitude below max(H, W), so it — and with it each axis
weight — moves by at most 2 ulp32(max(H, W) - 1) per axis; tap differences are at most 1 (values in [0, 1]), so the two axes move the
result by at most 4 ulp32(max(H, W) - 1).  The blend's own roundings, and a `p * (1 / 255)` tap in place of a correctly rounded division,
add at most 4 ulp32(1):

    |got - exact| <= 4 * ulp32(max(H, W) - 1) + 4 * ulp32(1)          (2.45e-4 at 640, 3.1e-5 at 128)"""
import numpy as np
import torch

# (source (h, w), output (h, w)) of the kernel tests: up and down, non-square, and the full-size coordinates
CASES = [((128, 128), (64, 64)), ((128, 128), (96, 96)), ((128, 128), (160, 160)), ((128, 128), (192, 192)),
         ((96, 160), (64, 96)), ((96, 160), (128, 224)),
         ((640, 640), (320, 320)), ((640, 640), (960, 960))]


def ulp32(v):
    return float(np.spacing(np.float32(v)))


def bound(h, w):
    return 4 * ulp32(max(h, w) - 1) + 4 * ulp32(1)


def noise(shape, seed):
    """uint8 noise [n, c, h, w]"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)


def _taps(n_in, n_out, shift=0.0, corners=False, scale=None):
    dst = np.arange(n_out, dtype=np.float64)
    if corners:
        src = dst * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    else:
        src = np.maximum((n_in / n_out if scale is None else scale) * (dst + 0.5 + shift) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    w1 = src - i0
    return i0, i1, 1.0 - w1, w1


def resize_f64(x, size, shift=0.0, corners=False, div=255.0, swap=False):
    """x uint8 [n, c, h, w] (torch, CPU) -> float64 numpy [n, c, ho, wo].  shift / corners / div / swap (each axis steps with the other
    axis' scale) plant defects: the tests of the judge"""
    p = x.numpy().astype(np.float64) / div
    sy, sx = (p.shape[3] / size[1], p.shape[2] / size[0]) if swap else (None, None)
    y0, y1, wy0, wy1 = _taps(p.shape[2], size[0], shift, corners, sy)
    x0, x1, wx0, wx1 = _taps(p.shape[3], size[1], shift, corners, sx)
    top = p[:, :, y0][:, :, :, x0] * wx0 + p[:, :, y0][:, :, :, x1] * wx1
    bot = p[:, :, y1][:, :, :, x0] * wx0 + p[:, :, y1][:, :, :, x1] * wx1
    return top * wy0[:, None] + bot * wy1[:, None]


def max_err(got, want):
    """max |got - want|, got a float32 tensor (any device), want float64 numpy"""
    return float(np.abs(got.detach().cpu().numpy().astype(np.float64) - want).max())
