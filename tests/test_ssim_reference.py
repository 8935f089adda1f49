"""CPU tests of the restatement behind the image loss's GPU tests (tests/ssim_ref.py), independent of the
kernels: the window, the map against a direct per-pixel double loop, S's identities, the closed-form gradient
against fp64 autograd, the L1 seed's float32 bits, the golden metrics, and the measured parity bounds."""
import json
import os

import numpy as np
import torch

import ssim_ref as R
from conftest import GOLDEN


def test_window_sums_to_one_and_is_separable():
    g, w = R.taps().numpy(), R.window().numpy()
    assert abs(g.sum() - 1.0) < 1e-15 and abs(w.sum() - 1.0) < 1e-15
    assert np.array_equal(w, np.outer(g, g))
    assert np.array_equal(g, g[::-1]) and g.argmax() == R.RADIUS
    # the kernels' literals (csrc/rm_loss.h) are these taps
    src = open(os.path.join(os.path.dirname(GOLDEN), "..", "burn_raymarching_amd", "csrc", "rm_loss.h")).read()
    body = src[src.index("constexpr float g[kLossTaps]"):]
    lits = [float(t.rstrip("f")) for t in body[body.index("{") + 1:body.index("}")].replace("\n", " ").split(",")]
    assert np.array_equal(np.float32(lits), g.astype(np.float32))


def direct_map(x, y, c1=R.C1, c2=R.C2):
    """S by a non-separable double loop over the window at every pixel, numpy fp64, zero padding."""
    w = R.window().numpy()
    v, h, wd, _ = x.shape
    out = np.zeros_like(x, dtype=np.float64)

    def f(a, vi, r, c, ch):
        acc = 0.0
        for i in range(R.TAPS):
            for j in range(R.TAPS):
                rr, cc = r + i - R.RADIUS, c + j - R.RADIUS
                if 0 <= rr < h and 0 <= cc < wd:
                    acc += w[i, j] * a[vi, rr, cc, ch]
        return acc

    for vi in range(v):
        for r in range(h):
            for c in range(wd):
                for ch in range(3):
                    mx, my = f(x, vi, r, c, ch), f(y, vi, r, c, ch)
                    sx, sy = f(x * x, vi, r, c, ch) - mx * mx, f(y * y, vi, r, c, ch) - my * my
                    sxy = f(x * y, vi, r, c, ch) - mx * my
                    out[vi, r, c, ch] = (2 * mx * my + c1) * (2 * sxy + c2) / ((mx * mx + my * my + c1) * (sx + sy + c2))
    return out


def test_map_equals_direct_double_loop():
    x, y = (a.astype(np.float64) for a in R.images(1, 7, 9))
    ref = direct_map(x, y)
    for sep in (False, True):
        got = R.ssim_map(torch.tensor(x), torch.tensor(y), separable=sep).numpy()
        assert np.abs(got - ref).max() < 1e-12, sep


def test_identity_and_symmetry():
    x, y = (torch.tensor(a, dtype=torch.float64) for a in R.images(3, 19, 23))
    assert np.abs(R.ssim_map(x, x).numpy() - 1.0).max() < 1e-12
    assert np.abs(R.ssim_map(x, y).numpy() - R.ssim_map(y, x).numpy()).max() < 1e-14


def test_closed_form_gradient_equals_autograd():
    for case in R.CASES:
        x, y = R.images(*case)
        for lw, sw in R.WEIGHTS:
            kw = dict(l1_weight=lw, ssim_weight=sw, progress=0.5)
            e = R.max_err(R.closed_form_grad(x, y, **kw), R.run(x, y, torch.float64, **kw)["grad"])
            print(f"ssim closed form vs autograd {case} {lw}/{sw}: {e:.3e}")
            assert e <= 1e-12, (case, lw, sw, e)


def test_l1_gradient_bits():
    """ssim_weight 0, l1_weight 1: the gradient is W * sign * inv_count in float32 bit for bit, with a pixel at
    x == y (sign 0) and a target sum exactly at the 0.01 threshold (not above it: background)."""
    x, y = (a.copy() for a in R.images(3, 19, 23))
    x[0, 9, 11] = y[0, 9, 11]                                # sign(0) = 0 inside the disc
    y[1, 0, 0] = np.float32([0.0025, 0.0025, 0.005])         # (t0 + t1) + t2 == 0.01f exactly
    assert (y[1, 0, 0, 0] + y[1, 0, 0, 1]) + y[1, 0, 0, 2] == np.float32(0.01)
    y[1, 0, 1] = np.float32([0.0025, 0.0025, 0.0051])        # just above
    for pr in R.PROGRESS:
        inv = np.float32(1.0 / x.size)
        want = R.l1_grad_f32(x, y, pr)
        g32 = R.run(x, y, torch.float32, l1_weight=1.0, ssim_weight=0.0, progress=pr, inv_count=float(inv))["grad"]
        assert g32.dtype == np.float32 and g32.tobytes() == want.tobytes()
        w = R.l1_weight_map(y, pr)
        assert w[1, 0, 0, 0] == np.float32(1.0 + 4.0 * pr) and w[1, 0, 1, 0] == 10.0 and w[0, 9, 11, 0] == 10.0
        assert np.all(want[0, 9, 11] == 0.0) and np.all(np.abs(want[1, 0, 1]) == np.float32(10.0) * inv)


def test_golden_metrics():
    """PSNR, SSIM and L1 of target_0.png against target_1.png: the recorded fp64 figures."""
    rec = json.load(open(os.path.join(GOLDEN, "ssim_targets.json")))
    m = R.metrics(*R.golden_pair())
    for k in ("psnr", "ssim", "l1"):
        print(f"ssim golden {k}: {m[k][0]:.12g} recorded {rec[k]:.12g}")
        assert abs(m[k][0] - rec[k]) <= 1e-9 * max(1.0, abs(rec[k])), k
    x, _ = R.golden_pair()
    same = R.metrics(x, x)
    assert np.isinf(same["psnr"][0]) and abs(same["ssim"][0] - 1.0) < 1e-12 and same["l1"][0] == 0.0


def test_parity_bounds_are_measured():
    """The GPU bounds: 8 x the float32 restatement's own error against fp64 over the case set (nothing fixed by
    hand); they are far below the quantities they bound."""
    sep, dense = R.bounds()
    for k in sep:
        print(f"ssim bound {k}: separable-order float32 {sep[k]:.3e}, dense float32 {dense[k]:.3e}")
        assert 0.0 < sep[k] < 1e-3, (k, sep[k])
