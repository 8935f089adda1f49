"""The escape proof of the unsplit march (bound_proof in rm_ray.h) restated in numpy
fp64 (tests/escape_ref.py: run), against the true march and the fp32 oracle, on 216 seeded scenes.

The bound trajectory u <- u + L(p(u)), L(p) = |p - c0| - R_soft - margins, R_soft = (1/k) ln sum_j
exp(k (|c_j - c0| + r_j)), must stay at or behind the march t <- t + D(p(t)) step for step, and a ray
it accepts (the bound point receding at distance (1 - 2e-5) dist >= T(steps left)) must end with
mask exactly 0 in the fp32 oracle. Coincident spheres make the bound tight (L = D up to the
margins there), so a margin of the wrong sign, a radius 2 % short or a dropped member count (the
sum over the spheres replaced by its largest term) each break the first property."""
import numpy as np
import pytest

from escape_ref import rays, run, scene

SEEDS = range(216)


@pytest.fixture(scope="module")
def results(oracle):
    out = []
    for seed in SEEDS:
        sc, eye, k, S, kind = scene(seed)
        o, d = rays(oracle, eye, seed)
        accepted, violations = run(sc, o, d, k, S)
        mask = oracle.render_diff_debug(o.astype(np.float32), d.astype(np.float32), sc, S, k, "f32")[:, 10]
        out.append((seed, kind, accepted, violations, np.asarray(mask)))
    return out


def test_bound_trajectory_never_passes_the_march(results):
    bad = [(seed, v) for seed, _, _, v, _ in results if v]
    assert not bad, bad[:8]


def test_accepted_rays_end_with_mask_zero_in_fp32(results):
    total = 0
    by_kind = {}
    for seed, kind, accepted, _, mask in results:
        assert np.all(mask[accepted] == 0.0), (seed, kind, mask[accepted].max())
        total += int(accepted.sum())
        by_kind[kind] = by_kind.get(kind, 0) + int(accepted.sum())
    # not vacuous: rays are accepted in every kind of scene (inside the cloud: the scenes that look away)
    assert total > 2000 and all(by_kind.get(kd, 0) > 50 for kd in ("cloud", "outlier", "coincident")), by_kind


@pytest.mark.parametrize("mutant", [dict(margin=-1.0), dict(radius_scale=0.98), dict(count=False)],
                         ids=["margin-sign", "radius-2pct-short", "count-dropped"])
def test_mutants_break_the_bound(oracle, mutant):
    violations = 0
    for seed in SEEDS:
        sc, eye, k, S, kind = scene(seed)
        if kind != "coincident":
            continue
        o, d = rays(oracle, eye, seed)
        assert run(sc, o, d, k, S)[1] == 0
        violations += run(sc, o, d, k, S, **mutant)[1]
    assert violations > 0
