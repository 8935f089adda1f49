"""The image-space loss of rm_image_loss restated in torch, parametrised by dtype: the SSIM map, the loss, the
per-view sums and the gradient by autograd, plus a numpy closed form of the gradient through A, B, C
(include/raymarch.h has the definitions). The GPU tests compare against the float64 run; their bounds come from
the float32 run's own error (bounds())."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

RADIUS, TAPS, SIGMA = 5, 11, 1.5
C1, C2 = 1e-4, 9e-4

# (V, H, W): the smallest image; narrower than the window both ways; odd sizes and three views; one pixel past a
# 32- and a 16-wide tile; exactly 16 x 16; interior tiles with halos on every side -- and, for the kernels' own
# 32 x 8 tiles, one row and one column past a tile with a second tile row that is full.
CASES = ((1, 1, 1), (2, 5, 7), (3, 19, 23), (2, 33, 17), (2, 16, 16), (1, 48, 40), (1, 17, 65))
WEIGHTS = ((0.8, 0.2), (0.0, 1.0), (1.0, 0.0))
PROGRESS = (0.0, 0.5)


def taps(dtype=torch.float64):
    """g: the 11-tap Gaussian of sigma 1.5 normalised to sum 1 (in fp64, then cast)."""
    d = torch.arange(TAPS, dtype=torch.float64) - RADIUS
    g = torch.exp(-d * d / (2.0 * SIGMA * SIGMA))
    return (g / g.sum()).to(dtype)


def window(dtype=torch.float64):
    g = taps(dtype)
    return g[:, None] * g[None, :]


def blur(a, dtype, separable=False):
    """F(a) for a [V, H, W, 3]: zero padding, every view and channel its own image. separable: the horizontal pass,
    then the vertical one (the kernels' order); otherwise one 11 x 11 convolution."""
    v, h, w, _ = a.shape
    p = a.permute(0, 3, 1, 2).reshape(3 * v, 1, h, w)
    if separable:
        g = taps(dtype)
        p = F.conv2d(p, g.reshape(1, 1, 1, TAPS), padding=(0, RADIUS))
        p = F.conv2d(p, g.reshape(1, 1, TAPS, 1), padding=(RADIUS, 0))
    else:
        p = F.conv2d(p, window(dtype).reshape(1, 1, TAPS, TAPS), padding=RADIUS)
    return p.reshape(v, 3, h, w).permute(0, 2, 3, 1)


def ssim_map(x, y, c1=C1, c2=C2, separable=False):
    dt = x.dtype
    mx, my = blur(x, dt, separable), blur(y, dt, separable)
    sx = blur(x * x, dt, separable) - mx * mx
    sy = blur(y * y, dt, separable) - my * my
    sxy = blur(x * y, dt, separable) - mx * my
    return (2 * mx * my + c1) * (2 * sxy + c2) / ((mx * mx + my * my + c1) * (sx + sy + c2))


def l1_weight_map(y32, progress=0.0, plain=False):
    """W per pixel [V, H, W, 1], float32, from the float32 target exactly as the kernels form it:
    (t0 + t1 + t2) > 0.01f ? 10 : fmaf(progress, 4, 1)."""
    y32 = np.asarray(y32, np.float32)
    if plain:
        return np.ones(y32.shape[:3] + (1,), np.float32)
    s = (y32[..., 0] + y32[..., 1]) + y32[..., 2]
    bg = np.float32(np.float64(progress) * 4.0 + 1.0)  # one rounding, as fmaf
    return np.where(s > np.float32(0.01), np.float32(10.0), bg).astype(np.float32)[..., None]


def run(x32, y32, dtype=torch.float64, *, l1_weight=0.8, ssim_weight=0.2, progress=0.0, plain=False, inv_count=None,
        c1=C1, c2=C2, separable=False, grad=True):
    """{"loss", "view_stats" [V, 3], "ssim_map", "grad", "l1_elems", "sq_elems"} as numpy, computed in dtype from
    the float32 images."""
    x = torch.tensor(np.asarray(x32, np.float32)).to(dtype).requires_grad_(grad)
    y = torch.tensor(np.asarray(y32, np.float32)).to(dtype)
    w = torch.tensor(l1_weight_map(y32, progress, plain)).to(dtype)
    if inv_count is None:
        inv_count = 1.0 / x.numel()
    s = ssim_map(x, y, c1, c2, separable)
    l1e = w * (x - y).abs()
    sqe = (x - y) ** 2
    loss = inv_count * (l1_weight * l1e.sum() + ssim_weight * (1 - s).sum())
    out = {"loss": loss.detach().numpy(), "ssim_map": s.detach().numpy(), "l1_elems": l1e.detach().numpy(),
           "sq_elems": sqe.detach().numpy(),
           "view_stats": torch.stack([l1e.sum((1, 2, 3)), sqe.sum((1, 2, 3)), s.sum((1, 2, 3))], 1).detach().numpy()}
    if grad:
        (g,) = torch.autograd.grad(loss, x)
        out["grad"] = g.numpy()
    return out


def _blur_np(a):
    return blur(torch.tensor(a), torch.float64).numpy()


def closed_form_grad(x32, y32, *, l1_weight=0.8, ssim_weight=0.2, progress=0.0, plain=False, inv_count=None, c1=C1,
                     c2=C2):
    """The header's gradient in numpy fp64: W sign(x - y) l1_weight inv_count
    - ssim_weight inv_count (F(A) + 2 x F(B) + y F(C))."""
    x, y = np.asarray(x32, np.float64), np.asarray(y32, np.float64)
    if inv_count is None:
        inv_count = 1.0 / x.size
    mx, my = _blur_np(x), _blur_np(y)
    sx, sy, sxy = _blur_np(x * x) - mx * mx, _blur_np(y * y) - my * my, _blur_np(x * y) - mx * my
    n1, n2, d1, d2 = 2 * mx * my + c1, 2 * sxy + c2, mx * mx + my * my + c1, sx + sy + c2
    s = n1 * n2 / (d1 * d2)
    b, c = -s / d2, 2 * n1 / (d1 * d2)
    a = 2 * my * n2 / (d1 * d2) - 2 * mx * s / d1 - 2 * mx * b - my * c
    w = l1_weight_map(y32, progress, plain).astype(np.float64)
    return w * np.sign(x - y) * l1_weight * inv_count - ssim_weight * inv_count * (_blur_np(a) + 2 * x * _blur_np(b)
                                                                                   + y * _blur_np(c))


def l1_grad_f32(x32, y32, progress=0.0, plain=False, inv_count=None, l1_weight=1.0):
    """The L1 part as the kernels form it, float32 throughout: (W * sign(x - y)) * s, s = l1_weight * inv_count."""
    x, y = np.asarray(x32, np.float32), np.asarray(y32, np.float32)
    if inv_count is None:
        inv_count = 1.0 / x.size
    s = np.float32(l1_weight) * np.float32(inv_count)
    return (l1_weight_map(y, progress, plain) * np.sign(x - y).astype(np.float32)) * s


@functools.lru_cache(maxsize=None)
def images(v, h, w, seed=0):
    """(x, y) float32 [V, H, W, 3]: a disc of colour on black (so both branches of W occur) times uniform noise;
    the render x is the target with its disc shifted and its colour and noise changed."""
    rng = np.random.default_rng(1000 * seed + 100 * v + 10 * h + w)
    rows, cols = np.mgrid[0:h, 0:w]

    def disc(cy, cx, rad, col):
        inside = ((rows - cy) ** 2 + (cols - cx) ** 2 <= rad * rad)[None, :, :, None]
        return inside * col.reshape(v, 1, 1, 3) * rng.uniform(0.5, 1.0, (v, h, w, 3))

    rad = max(0.35 * min(h, w), 0.6)
    col = rng.uniform(0.2, 1.0, (v, 3))
    y = disc((h - 1) / 2.0, (w - 1) / 2.0, rad, col)
    x = disc((h - 1) / 2.0 + 0.08 * h, (w - 1) / 2.0 - 0.05 * w, 1.1 * rad, np.clip(col + rng.uniform(-0.15, 0.15, (v, 3)),
                                                                                  0.0, 1.0))
    return x.astype(np.float32), y.astype(np.float32)


def max_err(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return float(d.max()) if d.size else 0.0


@functools.lru_cache(maxsize=None)
def bounds():
    """The GPU parity bounds, measured: 8 x the largest error of the float32 run (in the kernels' separable order)
    against the fp64 run over the whole case set, weights and progress values, per element of ssim_map, of grad
    relative to the case's largest gradient magnitude, and of the L1 and squared-error terms. The figures of the
    dense 11 x 11 float32 run are returned next to them for the record."""
    worst = {"ssim_map": 0.0, "grad_rel": 0.0, "l1_elems": 0.0, "sq_elems": 0.0}
    dense = dict(worst)
    for case in CASES:
        x, y = images(*case)
        for (lw, sw) in WEIGHTS:
            for pr in PROGRESS:
                for plain in (False, True):
                    kw = dict(l1_weight=lw, ssim_weight=sw, progress=pr, plain=plain)
                    r64 = run(x, y, torch.float64, **kw)
                    gmax = max(float(np.abs(r64["grad"]).max()), 1e-300)
                    for acc, sep in ((worst, True), (dense, False)):
                        r32 = run(x, y, torch.float32, separable=sep, **kw)
                        acc["ssim_map"] = max(acc["ssim_map"], max_err(r32["ssim_map"], r64["ssim_map"]))
                        acc["grad_rel"] = max(acc["grad_rel"], max_err(r32["grad"], r64["grad"]) / gmax)
                        acc["l1_elems"] = max(acc["l1_elems"], max_err(r32["l1_elems"], r64["l1_elems"]))
                        acc["sq_elems"] = max(acc["sq_elems"], max_err(r32["sq_elems"], r64["sq_elems"]))
    return {k: 8.0 * v for k, v in worst.items()}, {k: 8.0 * v for k, v in dense.items()}


def metrics(x32, y32):
    """{"psnr", "ssim", "l1"} per view in fp64 (peak 1)."""
    r = run(x32, y32, torch.float64, plain=True, grad=False)
    n = 3.0 * np.asarray(x32).shape[1] * np.asarray(x32).shape[2]
    st = r["view_stats"]
    with np.errstate(divide="ignore"):
        return {"psnr": -10.0 * np.log10(st[:, 1] / n), "ssim": st[:, 2] / n, "l1": st[:, 0] / n}


def golden_pair():
    """tests/golden/target_0.png and target_1.png as float32 [1, H, W, 3] in [0, 1]."""
    import os
    from PIL import Image
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    load = lambda n: (np.asarray(Image.open(os.path.join(here, n)).convert("RGB"), np.float32) / np.float32(255.0))[None]
    return load("target_0.png"), load("target_1.png")


if __name__ == "__main__":  # python tests/ssim_ref.py: record tests/golden/ssim_targets.json from the fp64 run
    import json
    import os
    m = metrics(*golden_pair())
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim_targets.json")
    with open(path, "w") as f:
        json.dump({"pair": ["target_0.png", "target_1.png"], **{k: float(v[0]) for k, v in m.items()}}, f, indent=1)
        f.write("\n")
    print(open(path).read())
