"""The tile proof of the camera-mode escape proof (rm_tile_proof_kernel in rm_sdf.h) as
tests/escape_ref.py restates it (the tile reader: cone, bound, tile_proof; the formulas and the margins are at
the top of that module), against the true soft-min and the fp32 oracle march.

One bound trajectory per 8x8 pixel tile (a wave of the per-ray kernel): with the tile's four corner rays d_k
(float32, the rays of the tile's own corner pixels), d_c their normalised sum and delta of cone(), every ray r
of the tile has |d_r - d_c| <= delta. The mutants: the step without |u| delta or with the previous step's u in
it, the cone built from the pixel centres, the lattice points taken half a cell from where G was evaluated, and
the receding test on the centre ray alone. The scenes, views and the oracle march are escape_ref's, computed once
for this module and test_escape_lattice_reference.

Counts of the restated proofs on the GPU test's views (tests/test_gpu_tile_proof.py), 48x80, 60 waves each:
gap scene 50 waves by the cone, 0 by the soft ball, 50 by the per-ray one-cell lattice proof this one replaces;
the 520-sphere scene 55 by the cone, 49 by the soft ball, 55 by the per-ray lattice proof
(test_counts_on_the_gpu_views prints them).
"""
import numpy as np
import pytest

import escape_ref
from escape_ref import (BALL_ABS, CORNERS, ESCAPE_REL, F, FAR_VIEW, GAP_CAM, PROOF_REL, SCENES, VIEWS, Geometry, bound,
                        cloud_scene, cone, gap_scene, lattice_bound, model_taken, soft_min, tile_proof, view_rays,
                        wave_tiles, waves_taken)


@pytest.fixture(scope="module")
def sampled():
    return escape_ref.sampled()


@pytest.fixture(scope="module")
def cones(oracle):
    return escape_ref.cones(oracle)


def _run(m, **mutant):
    return tile_proof(m["g"], m["o"][0], m["d4"], m["t1"], **mutant)


# ---- the bound ---------------------------------------------------------------------------------

def test_neighbour_bound_is_below_the_soft_min(sampled):
    tight = 0
    for kind, M, k, g, p, D in sampled:
        assert len(p) == 100000
        L, ball = bound(g, p)
        assert np.all(L <= D), (kind, M, k, float((L - D).max()))
        tight += int((L > ball).sum())
    assert tight > 100000  # not vacuous: at a quarter of the points the lattice term is the larger


def test_neighbour_bound_beats_the_cell_bound(sampled):
    """what the 8 actual distances buy over the one cell's half-diagonal slack, inside the cube"""
    for kind, M, k, g, p, D in sampled[:2]:
        inside = (np.abs(p - g.c0) < g.half - g.h).all(1)
        assert np.mean(lattice_bound(g, p[inside]) + BALL_ABS >= g.bound(p[inside])[0]) > 0.99


def test_centres_offset_by_half_a_cell_break_the_bound(sampled):
    """mutant 3: the distance taken to a lattice point half a cell from where G was evaluated"""
    bad = 0
    for kind, M, k, g, p, D in sampled:
        bad += int((bound(g, p, plus_half=False)[0] > D).sum())
    assert bad > 0


# ---- the cone ----------------------------------------------------------------------------------

def test_delta_covers_every_ray_of_the_tile(cones):
    for m in cones:
        dc, delta = cone(m["d4"])
        dev = np.linalg.norm(m["d"][m["tiles"]].astype(np.float64) - dc[:, None, :], axis=2).max(1)
        assert np.all(dev <= delta), (m["kind"], float((dev - delta).max()))


def test_delta_from_the_pixel_centres_misses_rays(oracle):
    """mutant 2: the ray of pixel x runs through x / W, the pixel's corner, not through (x + 0.5) / W. A cone
    built from the rays through the CENTRES of the tile's four corner pixels spans the same 7 pixels, half a
    pixel off: the tile's own first ray (its top-left pixel's) then lies outside it, in most tiles of every view.
    The centre rays are the odd pixels of the view at twice the resolution, whose even pixels are the view's own
    rays (asserted: that is the mapping x / W)."""
    tiles = wave_tiles(32, 32)
    views = [cam for kind, _, _, _ in SCENES for cam in VIEWS[kind]] + [FAR_VIEW]
    for cam in views:
        d = view_rays(oracle, 32, 32, cam)[1]
        d2 = view_rays(oracle, 64, 64, cam)[1].reshape(64, 64, 3)
        assert np.abs(d2[0::2, 0::2].reshape(-1, 3) - d).max() <= 2e-7
        centres = d2[1::2, 1::2].reshape(-1, 3)
        dc, delta = cone(centres[tiles[:, CORNERS]])
        dev = np.linalg.norm(d[tiles].astype(np.float64) - dc[:, None, :], axis=2)
        # the top-left ray, half a pixel further out on both axes (towards an image corner the perspective
        # squeezes the rays together and a tile there may still hold it: most tiles of every view do not)
        assert np.sum(dev[:, 0] > delta) >= 8, cam
        # the same construction from the tile's own corner rays holds them all (the kernel's cone)
        dc, delta = cone(d[tiles[:, CORNERS]])
        assert np.all(np.linalg.norm(d[tiles].astype(np.float64) - dc[:, None, :], axis=2) <= delta[:, None]), cam


def _step_violations(m, **mutant):
    """the march's induction step in float64: from the same u, no ray of the tile steps less than the cone,
    u + L(p_c) - |u| delta <= u + D(p_r(u)) -- with t + D(p_r(t)) non-decreasing in t that keeps u <= t"""
    g = m["g"]
    _, traj, _ = _run(m, **mutant)
    bad = steps = 0
    for n in range(1, g.S):
        run = ~np.isnan(traj[n]) & ~np.isnan(traj[n + 1])
        for w in np.flatnonzero(run):
            idx = m["tiles"][w]
            p = m["o"][idx].astype(np.float64) + m["d"][idx].astype(np.float64) * traj[n, w]
            bad += int((traj[n + 1, w] > traj[n, w] + soft_min(p, g.c, g.r, g.k)).sum())
            steps += 1
    return bad, steps


def test_cone_steps_no_further_than_any_ray(cones):
    steps = 0
    for m in cones:
        bad, n = _step_violations(m)
        assert bad == 0, (m["kind"], m["M"], m["k"], m["S"])
        steps += n
    assert steps > 500


def test_cone_stays_behind_the_oracle_march(cones):
    """u against every ray's fp32 oracle march, step for step (rays gone at the eye step by the ball's bound and need
    no proof)"""
    steps = 0
    for m in cones:
        _, traj, _ = _run(m)
        for w, idx in enumerate(m["tiles"]):
            run = ~np.isnan(traj[:, w])
            live = idx[~m["gone0"][idx]]
            assert np.all(traj[run, w][:, None] <= m["t"][run][:, live]), (m["kind"], m["M"], m["k"], m["S"], w)
            steps += int(run.sum())
    assert steps > 1000


@pytest.mark.parametrize("mutant", ["drop_ud", "stale_ud"])
def test_mutants_of_the_step_overtake_a_ray(cones, mutant):
    """mutants 1 and 4: the step without |u| delta, and with the previous step's u in it"""
    assert sum(_step_violations(m, **{mutant: True})[0] for m in cones) > 0


def _proofs_without_the_test(m, **mutant):
    """tiles proven at a u where wave_escaped's test does not hold for every ray at p_r(u)"""
    g = m["g"]
    taken, traj, at = _run(m, **mutant)
    bad = 0
    for w in np.flatnonzero(taken):
        idx = m["tiles"][w]
        d = m["d"][idx].astype(np.float64)
        e = m["o"][idx].astype(np.float64) + d * traj[at[w], w] - g.c0
        ok = ((e * d).sum(1) >= 0) & (np.linalg.norm(e, axis=1) * (1 - PROOF_REL) >= g.T[g.S - at[w]])
        bad += int(not ok.all())
    return bad, int(taken.sum())


def test_a_proven_tile_meets_the_escape_test_for_every_ray(cones):
    total = 0
    for m in cones:
        bad, n = _proofs_without_the_test(m)
        assert bad == 0, (m["kind"], m["M"], m["k"], m["S"])
        total += n
    assert total > 0  # per kind of scene: test_no_false_proofs


def test_receding_tested_on_the_centre_ray_alone_proves_too_early(cones):
    """mutant 5"""
    assert sum(_proofs_without_the_test(m, centre_recedes=True)[0] for m in cones) > 0


def test_no_false_proofs(cones):
    """every ray of a tile the cone takes meets the march's own escape test along the fp32 oracle march and
    ends with mask exactly 0"""
    waves = {}
    for m in cones:
        g, S = m["g"], m["S"]
        o, d = m["o"].astype(np.float64), m["d"].astype(np.float64)
        gone = np.zeros(len(o), bool)
        for n in range(S + 1):
            e = o + d * m["t"][n].astype(np.float64)[:, None] - g.c0
            gone |= ((e * d).sum(-1) >= 0) & (np.linalg.norm(e, axis=1) * (1 - ESCAPE_REL) >= g.T[S - n])
        taken = _run(m)[0]
        for w in np.flatnonzero(taken):
            idx = m["tiles"][w]
            assert gone[idx].all() and np.all(m["mask"][idx] == 0.0), (m["kind"], m["M"], m["k"], S, w)
        waves[m["kind"]] = waves.get(m["kind"], 0) + int(taken.sum())
    assert all(waves.get(kd, 0) > 0 for kd in ("gap", "outlier", "coincident", "cloud", "far")), waves


# ---- the views of tests/test_gpu_tile_proof.py ----------------------------------------------------

def test_counts_on_the_gpu_views(oracle):
    """not vacuous: the gap view and the 520-sphere view of the GPU test, where the cone must take strictly more
    waves than the soft ball (the counts are the module docstring's)"""
    for sc, cam in ((gap_scene(128), GAP_CAM), (cloud_scene(520), ([0.0, 0.5, 2.5], [1.2, 0.5, 0.0], 40.0))):
        cone_set, ball, ray = model_taken(oracle, sc, cam, 48, 80, 32, 32.0)
        print(len(cone_set), len(ball), len(ray))
        assert len(cone_set | ball) > len(ball)


def test_rows_order_view_is_not_vacuous(oracle):
    """the 40x40 view of the GPU test marches in row order (no multiple of 16): a wave is 64 consecutive pixels, 25
    waves, and its launch keeps the per-ray lattice proof. That proof takes waves there and the soft ball none."""
    sc = gap_scene(128)
    g = Geometry(sc, 32.0, 32)
    o, d = view_rays(oracle, 40, 40, GAP_CAM)
    t1 = np.asarray(oracle.render_diff(o, d, sc, 1, 32.0, precision="f32", with_t=True)[1], F)
    rows = np.arange(1600).reshape(25, 64)
    ray, ball = waves_taken(g, o, d, t1, rows)[0], waves_taken(g, o, d, t1, rows, lattice=False)[0]
    print(len(ray), len(ball))
    assert len(ray) >= 5 and len(ball) == 0


def test_inside_the_cloud_the_cone_adds_nothing(oracle):
    """tests/test_gpu_escape_lattice.py asserts the soft ball's counters for this view: the cone may take no wave
    there that the soft ball does not"""
    cone_set, ball, _ = model_taken(oracle, cloud_scene(300), ([0.05, 0.0, -0.1], [1.0, 0.3, 0.2], 70.0), 48, 80, 32, 32.0)
    assert cone_set <= ball
