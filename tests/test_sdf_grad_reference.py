"""CPU tests of the reference behind the distance field's backward (tests/sdf_grad_ref.py): the analytic
formulas of include/raymarch.h equal torch autograd of the restatement in fp64; the GPU tests' bounds (8
times the restatement's own fp32 error) reject a gradient with one planted fault; the fit demonstration
reaches its bar with the restatement itself."""
import numpy as np
import pytest
import torch

import sdf_grad_ref as R
from test_gpu_sdf import CSHARP, K, pool


def _small_scene(m, seed):
    rng = np.random.default_rng(seed)
    return {"centers": rng.uniform(-0.6, 0.6, (m, 3)).astype(np.float32),
            "colors": rng.uniform(0.05, 0.95, (m, 3)).astype(np.float32),
            "radius": rng.uniform(0.08, 0.3, m).astype(np.float32)}


def _points(sc, n, seed):
    """n points: exactly on the centre of sphere 0, one 1e3 away, the rest uniform in [-1, 1]^3."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    pts[0] = sc["centers"][0]
    pts[1] = np.array([600.0, -700.0, 400.0], np.float32)
    return pts


@pytest.mark.parametrize("m,n,cs", [(33, 257, 10.0), (1, 65, 10.0), (33, 65, 0.0), (5, 9, 3.5)])
def test_analytic_formulas_equal_autograd_fp64(m, n, cs):
    sc = _small_scene(m, 100 + m)
    pts = _points(sc, n, 7)
    for name, (gD, gC) in R.seed_sets(n).items():
        ref = R.autograd(pts, sc, K, cs, gD, gC, torch.float64)
        got = R.analytic(pts, sc, K, cs, gD, gC)
        for key in R.KEYS:
            scale = max(1.0, float(np.abs(ref[key]).max()))
            e = R.max_err(got[key], ref[key])
            print(f"analytic vs autograd fp64 M={m} N={n} cs={cs} seeds={name} {key}: {e:.3e} (scale {scale:.3e})")
            assert e <= 1e-12 * scale, (m, n, cs, name, key, e)
        # the point on the centre: its sphere's term is dropped, in both
        assert np.isfinite(got["points"]).all()
    if m == 1:
        assert not ref["points"][0].any() and not got["points"][0].any()


FAULTS = {"point_dropped": dict(drop_point=None), "row_shifted": dict(shift_row=7), "no_colour_term": dict(no_color_term=True),
          "mask_ignored": dict(no_mask=True)}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_bounds_reject_a_planted_fault(fault):
    """On the m33 pool's first 257 points with both seeds: the exact fp64 gradient passes every bound, and
    with one fault planted at least one output misses its bound. The pool's centre point has e = 0 exactly,
    where the mask changes nothing, so point 9 is moved to 5e-4 from the centre of sphere 0: under the clamp
    (q = 2.5e-7 < 1e-6) with e != 0."""
    sc, pts, far, _, _ = pool("m33")
    pts = pts.copy()
    pts[9] = sc["centers"][0] + np.array([5e-4, 0.0, 0.0], np.float32)
    gD, gC = R.seed_sets(len(pts))["both"]
    bound, _ = R.bounds(pts, far, sc, K, CSHARP, gD, gC)
    n = 257
    ref = R.autograd(pts[:n], sc, K, CSHARP, gD[:n], gC[:n], torch.float64)
    clean = R.errors(R.analytic(pts[:n], sc, K, CSHARP, gD[:n], gC[:n]), ref, far[:n])
    assert all(clean[q] <= bound[q] for q in clean), (clean, bound)
    kw = dict(FAULTS[fault])
    if fault == "point_dropped":
        kw["drop_point"] = 8 + int(np.argmax(np.abs(gD[8:n])))  # a near point with the largest distance seed
    bad = R.errors(R.analytic(pts[:n], sc, K, CSHARP, gD[:n], gC[:n], **kw), ref, far[:n])
    missed = {q: (bad[q], bound[q]) for q in bad if bad[q] > bound[q]}
    print(f"fault {fault}: misses {missed}")
    assert missed, (fault, bad, bound)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_fit_demonstration_with_the_restatement(dtype):
    pts, tcol, start = R.fit_problem()
    assert len(pts) >= 600  # most of the 1200 samples lie within 0.02 of the blended surface
    p, tc = torch.from_numpy(pts).to(dtype), torch.from_numpy(tcol).to(dtype)
    first, last = R.fit_run(lambda x, c, col, r: R.field_t(x, c, col, r, R.FIT_K, R.FIT_CS), p, tc, start)
    print(f"fit with the restatement {dtype}: loss {first:.5f} -> {last:.5f} ({last / first:.4f} of the start)")
    assert last <= 0.025 * first, (first, last)
