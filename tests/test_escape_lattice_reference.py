"""The lattice bound of the camera-mode escape proof (bound_proof in rm_ray.h;
write_bound, rm_lattice_kernel) as tests/escape_ref.py restates it (the cell reader: Geometry.bound, proof,
waves_taken; the formulas and the margins are at the top of that module), against the true soft-min in
fp64 and the fp32 oracle march.

D is 1-Lipschitz, so L <= D everywhere; the bound march u <- u + L(p(u)) then stays at or behind the
march step for step, and a wave the proof takes ends with every ray gone. The mutants show that the
sampled points and rays can tell: each of them breaks L <= D on the same inputs.

The fourth mutant drops the inside test and reads the cell the unclamped index addresses in the
table (the index modulo N). Dropping the test but keeping the kernel's clamp is no mutant: every
sphere lies inside the cube, so clamping a point onto the cube moves it no further from any centre
and the clamped cell's bound holds outside the cube too.
"""
import numpy as np
import pytest

import escape_ref
from escape_ref import GAP_CAM, ESCAPE_REL, F, Geometry, gap_scene, view_rays, wave_tiles, waves_taken


@pytest.fixture(scope="module")
def sampled():
    return escape_ref.sampled()


def test_lattice_bound_is_below_the_soft_min(sampled):
    tight = 0
    for kind, M, k, g, p, D in sampled:
        assert len(p) == 100000
        L, ball = g.bound(p)
        assert np.all(L <= D), (kind, M, k, float((L - D).max()))
        tight += int((L > ball).sum())
    assert tight > 100000  # not vacuous: at a quarter of the points the lattice is the larger bound


MUTANTS = {"slack-halved": dict(slack_scale=0.5), "cell-off-by-one": dict(index_shift=1),
           "centres-without-half": dict(plus_half=False), "lattice-alone-outside-the-cube": dict(wrap=True)}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutants_break_the_bound(sampled, mutant):
    bad = 0
    for kind, M, k, g, p, D in sampled:
        L, _ = g.bound(p, **MUTANTS[mutant])
        bad += int((L > D).sum())
    assert bad > 0


# ---- the bound march and the proof of a wave --------------------------------------------------

@pytest.fixture(scope="module")
def marched(oracle):
    return escape_ref.marched(oracle)


def test_bound_march_stays_behind_the_oracle_march(marched):
    steps = 0
    for m in marched:
        run = ~np.isnan(m["traj"])
        assert np.all(m["traj"][run] <= m["t"][run]), (m["kind"], m["M"], m["k"], m["S"])
        steps += int(run.sum())
    assert steps > 20000


def test_no_false_proofs(marched):
    """every ray of a wave the proof takes meets the march's own escape test along the fp32 oracle march
    and ends with mask exactly 0"""
    waves = {}
    for m in marched:
        g, S = m["g"], m["S"]
        o, d = m["o"].astype(np.float64), m["d"].astype(np.float64)
        gone = np.zeros(len(o), bool)
        for n in range(S + 1):
            e = o + d * m["t"][n].astype(np.float64)[:, None] - g.c0
            gone |= ((e * d).sum(-1) >= 0) & (np.linalg.norm(e, axis=1) * (1 - ESCAPE_REL) >= g.T[S - n])
        tiles = wave_tiles(32, 32)
        for w in m["taken"]:
            assert gone[tiles[w]].all() and np.all(m["mask"][tiles[w]] == 0.0), (m["kind"], m["M"], m["k"], S, w)
        waves[m["kind"]] = waves.get(m["kind"], 0) + len(m["taken"])
    assert all(waves.get(kd, 0) > 0 for kd in ("gap", "outlier", "coincident", "cloud")), waves


# ---- the gap scene of tests/test_gpu_escape_lattice.py ---------------------------------------

def test_gap_scene_is_not_vacuous(oracle):
    """the restated lattice proof takes waves of the GPU test's gap view and the soft-ball proof none"""
    sc = gap_scene(128)
    S, k = 32, 32.0
    g = Geometry(sc, k, S)
    assert g.rs > 0.8 + 0.3  # R_soft covers the gap and both clusters
    for w, h in ((48, 80), (64, 64)):
        o, d = view_rays(oracle, w, h, GAP_CAM)
        t1 = np.asarray(oracle.render_diff(o, d, sc, 1, k, precision="f32", with_t=True)[1], F)
        tiles = wave_tiles(w, h)
        assert len(waves_taken(g, o, d, t1, tiles)[0]) > 0
        assert len(waves_taken(g, o, d, t1, tiles, lattice=False)[0]) == 0
