"""The escape proof of the unsplit march (bound_proof in rm_ray.h) restated in numpy
fp64, against the true march and the fp32 oracle, on 216 seeded scenes.

The bound trajectory u <- u + L(p(u)), L(p) = |p - c0| - R_soft - margins, R_soft = (1/k) ln sum_j
exp(k (|c_j - c0| + r_j)), must stay at or behind the march t <- t + D(p(t)) step for step, and a ray
it accepts (the bound point receding at distance (1 - 2e-5) dist >= T(steps left)) must end with
mask exactly 0 in the fp32 oracle. Coincident spheres make the bound tight (L = D up to the
margins there), so a margin of the wrong sign, a radius 2 % short or a dropped member count (the
sum over the spheres replaced by its largest term) each break the first property."""
import math

import numpy as np
import pytest

MSHARP = 15.0
GONE_D = max(6.0, 130.0 / (MSHARP * 1.44269504))


def scene(seed):
    """(scene dict, eye, k, S, kind): M 12 / 48 / 300; unit-ball cloud, one outlier at 3x the cloud
    radius, coincident spheres, eye inside the cloud; k 5 / 32; S 8 / 32."""
    rng = np.random.default_rng(1000 + seed)
    M = (12, 48, 300)[seed % 3]
    kind = ("cloud", "outlier", "coincident", "inside")[(seed // 3) % 4]
    k = (5.0, 32.0)[(seed // 12) % 2]
    S = (8, 32)[(seed // 24) % 2]
    v = rng.normal(size=(M, 3))
    c = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.random((M, 1)) ** (1 / 3)
    r = rng.uniform(0.03, 0.12, M)
    if kind == "outlier":
        c[0] = 3.0 * v[0] / np.linalg.norm(v[0])
    if kind == "coincident":
        c[:] = rng.uniform(-0.3, 0.3, 3)
        r[:] = rng.uniform(0.1, 0.5)
    a = rng.uniform(0, 2 * math.pi)
    eye = np.array([2.5 * math.cos(a), rng.uniform(-0.5, 0.8), 2.5 * math.sin(a)])
    if kind == "inside":
        eye = rng.uniform(-0.25, 0.25, 3)
    sc = {"centers": c.astype(np.float32), "radius": r.astype(np.float32),
          "colors": rng.uniform(0.05, 0.95, (M, 3)).astype(np.float32),
          "light_dir": np.array([-0.5, 0.5, -1.0], np.float32), "ambient": np.array([0.2], np.float32)}
    return sc, eye, k, S, kind


def rays(oracle, eye, seed):
    """8x8 rays of a 70 degree view towards a point near the origin, every third scene looking away"""
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(-0.4, 0.4, 3) if seed % 3 else 2.0 * eye + rng.uniform(-0.4, 0.4, 3)
    o, d = oracle.camera_rays(8, 8, eye.astype(np.float32), tgt.astype(np.float32), 70.0, precision="f32")
    return o.astype(np.float64), d.astype(np.float64)


def soft_min(p, c, r, k):
    x = -k * (np.linalg.norm(p[:, None, :] - c, axis=-1) - r)
    m = x.max(-1)
    return -(m + np.log(np.exp(x - m[:, None]).sum(-1))) / k


def threshold_table(S, rp):
    """T(n) of write_bound"""
    T = [(GONE_D + rp) * (1 + 1e-6)]
    for _ in range(S):
        y = T[-1] * 1.0000101
        T.append((rp + math.sqrt(2 * y * y * (1 + 1e-6) - rp * rp)) * 0.5 * (1 + 1e-5) + 1e-6)
    return np.asarray(T) * (1 + 1e-6)


def run(sc, o, d, k, S, margin=1.0, radius_scale=1.0, count=True):
    """The march and the bound march side by side: (rays accepted, violations of u <= t)."""
    c, r = sc["centers"].astype(np.float64), sc["radius"].astype(np.float64)
    c0 = 0.5 * (c.min(0) + c.max(0))
    reach = np.linalg.norm(c - c0, axis=1) + r
    R = reach.max() * (1 + 1e-5) + 1e-6
    slack = math.log(len(r)) / k * (1 + 1e-6) + 1e-7
    rsoft = R + math.log(np.exp(k * (reach - R)).sum() * (1 + 1e-5)) / k if count else R
    rsoft = min(rsoft * (1 + 1e-5) + 1e-6, R + slack) * radius_scale
    rs = (rsoft + margin * 1e-3) * (1 + 1e-6) + margin * 1e-3
    T = threshold_table(S, (R + slack + 1e-3) * (1 + 1e-6))
    n = len(o)
    t, u = np.zeros(n), np.zeros(n)
    active = np.ones(n, bool)   # the bound march of the ray still runs
    accepted = np.zeros(n, bool)
    violations = 0
    for st in range(S):
        e = o + d * u[:, None] - c0
        dist = np.linalg.norm(e, axis=1)
        accepted |= active & ((e * d).sum(1) >= 0) & (dist * (1 - margin * 2e-5) >= T[S - st])
        active &= ~accepted
        Lb = dist - rs
        active &= Lb > 0          # a ray the bound cannot move is given up
        t = t + soft_min(o + d * t[:, None], c, r, k)
        u = np.where(active, u + Lb, u)
        violations += int((active & (u > t)).sum())
    return accepted, violations


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
