"""The lattice bound of the camera-mode escape proof (bound_proof in rm_ray.h;
write_bound, rm_lattice_kernel) restated in numpy, against the true soft-min in fp64 and the fp32
oracle march.

The lattice: N^3 cells over the cube of half-side R' + margin about c_0, cell i's centre at
-half + (i + 0.5) h per axis, G[cell] the soft-min at the centre (float32, direct-form distances as
the lattice kernel's). The bound of a point p, e = p - c_0:

    L(p) = max(|e| - R_soft - 2e-3, inside ? G[floor((e + half) / h)] - slack - 2e-3 : -inf)
    slack = h sqrt(3)/2 (1 + 1e-4) + 1e-3

D is 1-Lipschitz, so L <= D everywhere; the bound march u <- u + L(p(u)) then stays at or behind the
march step for step, and a wave the proof takes ends with every ray gone. The mutants show that the
sampled points and rays can tell: each of them breaks L <= D on the same inputs.

The fourth mutant drops the inside test and reads the cell the unclamped index addresses in the
table (the index modulo N). Dropping the test but keeping the kernel's clamp is no mutant: every
sphere lies inside the cube, so clamping a point onto the cube moves it no further from any centre
and the clamped cell's bound holds outside the cube too.
"""
import math

import numpy as np
import pytest

from test_escape_proof_reference import soft_min, threshold_table

N = 64          # kLatticeN
MARGIN = 0.25   # kLatticeMargin
MIN_STEP = 0.02  # kProofMinStep
F = np.float32


# ---- scenes (shared with tests/test_gpu_escape_lattice.py) -----------------------------------

def _scene(c, r, seed):
    rng = np.random.default_rng(seed)
    M = len(r)
    return {"centers": np.asarray(c, F), "radius": np.asarray(r, F),
            "colors": rng.uniform(0.05, 0.95, (M, 3)).astype(F),
            "light_dir": np.array([-0.5, 0.5, -1.0], F), "ambient": np.array([0.2], F)}


def _ball(rng, M, radius):
    v = rng.normal(size=(M, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True) * rng.random((M, 1)) ** (1 / 3) * radius


def cloud_scene(M, seed=7, centre=(0.0, 0.0, 0.0)):
    """a ball of radius 0.6 of small spheres"""
    rng = np.random.default_rng(seed)
    return _scene(_ball(rng, M, 0.6) + np.asarray(centre), rng.uniform(0.03, 0.1, M), seed)


def outlier_scene(M, seed=8):
    """the cloud with an eighth of its spheres thrown out to 1.0-1.3 (what the optimizer does to the bench scene)"""
    rng = np.random.default_rng(seed)
    c = _ball(rng, M, 0.6)
    n = M // 8
    v = rng.normal(size=(n, 3))
    c[:n] = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(1.0, 1.3, (n, 1))
    return _scene(c, rng.uniform(0.03, 0.1, M), seed)


def gap_scene(M=128, seed=9):
    """two clusters of M / 2 spheres (radius 0.3) at x = +-0.8: the soft ball about the midpoint covers the gap"""
    rng = np.random.default_rng(seed)
    c = _ball(rng, M, 0.3)
    c[: M // 2, 0] -= 0.8
    c[M // 2:, 0] += 0.8
    return _scene(c, rng.uniform(0.03, 0.08, M), seed)


def coincident_scene(M, seed=10):
    """all spheres on one centre: the bounding sphere, and with it the lattice's h, at its smallest"""
    rng = np.random.default_rng(seed)
    return _scene(np.tile(rng.uniform(-0.2, 0.2, 3), (M, 1)), np.full(M, 0.25), seed)


# ---- the restatement -------------------------------------------------------------------------

class Geometry:
    """write_bound's figures for a scene: bounding sphere, R', R_soft, T(n), the lattice's layout"""

    def __init__(self, sc, k, S=32):
        c, r = sc["centers"].astype(np.float64), sc["radius"].astype(np.float64)
        self.c, self.r, self.k, self.S = c, r, k, S
        self.c0 = 0.5 * (c.min(0) + c.max(0))
        reach = np.linalg.norm(c - self.c0, axis=1) + r
        R = reach.max() * (1 + 1e-5) + 1e-6
        lse_slack = math.log(len(r)) / k * (1 + 1e-6) + 1e-7
        rsoft = R + math.log(np.exp(k * (reach - R)).sum() * (1 + 1e-5)) / k
        rsoft = min(rsoft * (1 + 1e-5) + 1e-6, R + lse_slack)
        self.rs = (rsoft + 1e-3) * (1 + 1e-6) + 1e-3
        self.rprime = (R + lse_slack + 1e-3) * (1 + 1e-6)
        self.T = threshold_table(S, self.rprime)
        self.half = float(F(self.rprime + MARGIN))
        self.h = float(F(2.0 * self.half / N))
        self.inv_h = float(F(1.0 / self.h))
        self.slack = self.h * (0.8660254 * (1 + 1e-4)) + 1e-3

    def centres(self, idx, plus_half=True):
        """float32 cell centres as the lattice kernel forms them: origin + (float)i * h"""
        origin = (self.c0.astype(F) - F(self.half)) + F(0.5 if plus_half else 0.0) * F(self.h)
        return origin + idx.astype(F) * F(self.h)

    def cell_values(self, idx, plus_half=True):
        """G at the cells idx [n, 3]: the soft-min at the centre, float32, direct-form distances"""
        out = np.empty(len(idx), F)
        c, r, k = self.c.astype(F), self.r.astype(F), F(self.k)
        for i in range(0, len(idx), 8192):
            e = self.centres(idx[i:i + 8192], plus_half)[:, None, :] - c
            d = np.sqrt(np.maximum((e * e).sum(-1, dtype=F), F(1e-6))) - r
            dmin = d.min(-1)
            out[i:i + 8192] = dmin - np.log(np.exp(-k * (d - dmin[:, None])).sum(-1, dtype=F)) / k
        return out

    def bound(self, p, dtype=np.float64, slack_scale=1.0, index_shift=0, plus_half=True, wrap=False):
        """L(p) for points p [n, 3]; the keyword arguments are the mutants"""
        p = np.asarray(p, dtype)
        e = p - self.c0.astype(dtype)
        dist = np.sqrt((e * e).sum(-1))
        f = np.clip((e + dtype(self.half)) * dtype(self.inv_h), -1.0, float(N))
        i = np.floor(f).astype(np.int64)
        inside = ((i >= 0) & (i < N)).all(-1)
        if wrap:  # no inside test: the cell the unclamped index addresses in the table
            i = np.floor((e + dtype(self.half)) * dtype(self.inv_h)).astype(np.int64)
            cell, use = i % N, np.ones(len(p), bool)
        else:
            cell, use = np.clip(i, 0, N - 1), inside
        cell = np.clip(cell + np.array([index_shift, 0, 0]), 0, N - 1)
        g = np.full(len(p), -np.inf, dtype)
        if use.any():
            uniq, inv = np.unique(cell[use], axis=0, return_inverse=True)
            g[use] = self.cell_values(uniq, plus_half)[inv.reshape(-1)].astype(dtype) - dtype(slack_scale * self.slack + 2e-3)
        ball = dist - dtype(self.rs)
        return np.maximum(ball, g), ball


SCENES = [("gap", gap_scene, 128, 32.0), ("outlier", outlier_scene, 300, 32.0),
          ("coincident", coincident_scene, 128, 5.0), ("cloud", cloud_scene, 300, 5.0),
          ("outlier", outlier_scene, 128, 5.0), ("coincident", coincident_scene, 300, 32.0)]


def sample_points(g, seed):
    """1e5 points: uniform over the cube and a rim about it; on cell faces, edges and corners (exactly on
    the lattice planes and a few ulps to either side); just inside and outside the cube; inside spheres."""
    rng = np.random.default_rng(seed)
    half, h = g.half, g.h
    pts = [rng.uniform(-1.3 * half, 1.3 * half, (25000, 3))]
    for axes, n in ((1, 15000), (2, 15000), (3, 15000)):  # faces, edges, corners
        e = rng.uniform(-half, half, (n, 3))
        planes = -half + rng.integers(0, N + 1, (n, 3)) * h + rng.choice([0.0, 1e-6, -1e-6, 1e-4, -1e-4], (n, 3)) * h
        on = np.argsort(rng.random((n, 3)), axis=1) < axes
        pts.append(np.where(on, planes, e))
    e = rng.uniform(-half, half, (10000, 3))  # one coordinate at the cube's boundary, to either side
    ax = rng.integers(0, 3, 10000)
    e[np.arange(10000), ax] = rng.choice([-1.0, 1.0], 10000) * half * (1 + rng.uniform(-1e-3, 1e-3, 10000))
    pts.append(e)
    j = rng.integers(0, len(g.r), 20000)  # inside spheres
    v = rng.normal(size=(20000, 3))
    pts.append(g.c[j] - g.c0 + v / np.linalg.norm(v, axis=1, keepdims=True) * (g.r[j] * rng.random(20000))[:, None])
    return np.concatenate(pts) + g.c0


@pytest.fixture(scope="module")
def sampled():
    """per scene: the geometry, the points and the true soft-min there, computed once"""
    out = []
    for n, (kind, make, M, k) in enumerate(SCENES[:4]):
        g = Geometry(make(M), k)
        p = sample_points(g, 100 + n)
        D = np.concatenate([soft_min(p[i:i + 20000], g.c, g.r, k) for i in range(0, len(p), 20000)])
        out.append((kind, M, k, g, p, D))
    return out


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

def view_rays(oracle, w, h, cam):
    eye, target, fov = cam
    return oracle.camera_rays(w, h, np.float32(eye), np.float32(target), fov, precision="f32")


def wave_tiles(w, h):
    """ray indices of the 8x8 pixel tiles of a w x h view (a wave of the 16x16-tile order), [waves, 64]"""
    idx = np.arange(w * h).reshape(h, w)
    return np.stack([idx[y:y + 8, x:x + 8].reshape(-1) for y in range(0, h, 8) for x in range(0, w, 8)])


def oracle_march(oracle, o, d, sc, S, k):
    """t of the fp32 oracle march after 0..S steps, [S + 1, n]"""
    return np.stack([np.zeros(len(o), F)] + [np.asarray(oracle.render_diff(o, d, sc, s, k, precision="f32", with_t=True)[1], F)
                                            for s in range(1, S + 1)])


def proof(g, o, d, t1, lattice=True, **mutant):
    """bound_proof from step 1 in float32 for the rays o, d [n, 3] at march distance t1 (the shared
    origin step taken): (u per step [S + 1, n], nan where the bound march of the ray has ended; proven;
    given_up: a ray's bound step fell to kProofMinStep before it was proven)."""
    S = g.S
    o, d = o.astype(F), d.astype(F)
    c0 = g.c0.astype(F)
    e = o - c0
    gone = ((e * d).sum(-1) >= 0) & (np.sqrt((e * e).sum(-1)) * F(1 - 1e-5) >= F(g.T[S]))  # wave_escaped(0)
    u = t1.astype(F).copy()
    proven = gone.copy()
    given_up = np.zeros(len(o), bool)
    traj = np.full((S + 1, len(o)), np.nan, F)
    for n in range(1, S):
        act = ~proven & ~given_up
        traj[n, act] = u[act]
        p = o + d * u[:, None]
        e = p - c0
        dist = np.sqrt((e * e).sum(-1, dtype=F))
        proven |= act & ((e * d).sum(-1) >= 0) & (dist * F(1 - 2e-5) >= F(g.T[S - n]))
        if lattice:
            Lb = g.bound(p, F, **mutant)[0]
        else:
            Lb = dist - F(g.rs)
        given_up |= ~proven & ~(Lb > F(MIN_STEP))
        u = np.where(proven | given_up, u, u + Lb).astype(F)
    return traj, proven, given_up


def guard_ok(g, o):
    return np.abs(o).sum(-1) + np.abs(g.c0).sum() + 3.0 * g.T[0] <= 256.0


def waves_taken(g, o, d, t1, tiles, lattice=True):
    """the waves the restated proof takes: the magnitude guard holds for every ray and every ray is proven
    (a ray whose bound step falls to kProofMinStep is never proven here; in the kernel it ends its wave's
    proof at that step: the same waves)"""
    traj, proven, _ = proof(g, o, d, t1, lattice)
    taken = [w for w, idx in enumerate(tiles) if guard_ok(g, o[idx]).all() and proven[idx].all()]
    return np.asarray(taken, int), traj, proven


VIEWS = {  # per kind of scene: views of 32x32 rays (16 waves each) that pass beside, through and into the scene
    "gap": [([0.0, 0.1, 2.6], [0.0, 0.0, 0.0], 40.0), ([1.5, 0.4, 2.2], [0.0, 0.0, 0.0], 60.0)],
    "outlier": [([0.0, 0.5, 2.5], [0.0, 0.0, 0.0], 60.0), ([2.4, -0.3, 0.4], [0.3, 0.9, 0.0], 60.0)],
    "coincident": [([0.0, 0.3, 2.0], [0.6, 0.0, 0.0], 60.0)],
    "cloud": [([0.0, 0.5, 2.5], [0.9, 0.5, 0.0], 50.0), ([0.9, 0.2, 0.6], [0.0, 0.0, 0.0], 70.0)],
}


@pytest.fixture(scope="module")
def marched(oracle):
    out = []
    for kind, make, M, k in SCENES:
        sc = make(M)
        for S in (8, 32):
            g = Geometry(sc, k, S)
            for cam in VIEWS[kind]:
                o, d = view_rays(oracle, 32, 32, cam)
                t = oracle_march(oracle, o, d, sc, S, k)
                mask = np.asarray(oracle.render_diff_debug(o, d, sc, S, k, "f32")[:, 10])
                taken, traj, proven = waves_taken(g, o, d, t[1], wave_tiles(32, 32))
                out.append(dict(kind=kind, M=M, k=k, S=S, g=g, o=o, d=d, t=t, mask=mask, taken=taken, traj=traj,
                                proven=proven))
    return out


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
            gone |= ((e * d).sum(-1) >= 0) & (np.linalg.norm(e, axis=1) * (1 - 1e-5) >= g.T[S - n])
        tiles = wave_tiles(32, 32)
        for w in m["taken"]:
            assert gone[tiles[w]].all() and np.all(m["mask"][tiles[w]] == 0.0), (m["kind"], m["M"], m["k"], S, w)
        waves[m["kind"]] = waves.get(m["kind"], 0) + len(m["taken"])
    assert all(waves.get(kd, 0) > 0 for kd in ("gap", "outlier", "coincident", "cloud")), waves


# ---- the gap scene of tests/test_gpu_escape_lattice.py ---------------------------------------

GAP_CAM = ([0.0, 0.0, 2.2], [0.0, 0.0, 0.0], 50.0)  # the eye on the z axis, looking through the gap: both clusters show


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
