"""The escape proof of the unsplit march (csrc/rm_proof.h) restated in numpy: the one CPU
model of write_bound (rm_records.h), wave_escaped and bound_proof (rm_ray.h) and rm_tile_proof_kernel
(rm_sdf.h). Shared by tests/test_escape_proof_reference.py, test_escape_lattice_reference.py,
test_tile_proof_reference.py (CPU) and test_gpu_escape_lattice.py, test_gpu_tile_proof.py. The module imports
numpy alone: the oracle, and for _train torch and the package, are handed in by the caller, so it loads on a
machine without a GPU.

The margins below carry rm_proof.h's names in upper case, with its values (tests/test_source_guards.py compares
the two files). The formulas, once, for a scene with bounding sphere (c_0, R) and e = p - c_0:

    R'     = (R + ln(M)/k + MARCH_ABS) (1 + RADIUS_REL)
    rs     = (R_soft + MARCH_ABS) (1 + RADIUS_REL) + BOUND_STEP_ABS,   R_soft = (1/k) ln sum_j exp(k (|c_j - c_0| + r_j))
    T(n):    a receding ray at (1 - ESCAPE_REL) |e| >= T(n) with n steps left ends gone (threshold_table)
    escape:  e . d >= 0 and |e| (1 - ESCAPE_REL) >= T(steps left)          wave_escaped, on the march's point
             e . d >= 0 and |e| (1 - PROOF_REL)  >= T(steps left)          the proofs, on the bound point
    guard:   |o|_1 + |c_0|_1 + 3 T(0) <= PROOF_MAX_MAGNITUDE
    ball     L(p) = |e| - rs                                               (run; proof with lattice=False)
    cell     L(p) = max(ball, inside ? G[floor((e + half) / h)] - slack - BALL_ABS : -inf)       (Geometry.bound)
             slack = h LATTICE_HALF_DIAG (1 + LATTICE_CELL_REL) + LATTICE_KERNEL_ABS
    tile     L(p) = max(ball, max over the 8 lattice points n around p of
                              G[n] - |p - x_n| (1 + TILE_LATTICE_REL) - TILE_LATTICE_ABS)         (bound)
             delta = max_k |d_k - d_c| (1 + TILE_CONE_REL) + TILE_CONE_ABS                       (cone)
             u    <- u + L(p_c(u)) - |u| delta, given up at a net step <= PROOF_MIN_STEP          (tile_proof)
             proven: (o - c_0) . d_c - |o - c_0| delta + u (1 - TILE_RECEDE_REL) >= 0
                     and |e| - |u| delta >= T(steps left) PROOF_DIST_UP

The lattice: N^3 cells (N = LATTICE_N) over the cube of half-side R' + LATTICE_MARGIN about c_0, cell i's centre
at -half + (i + 0.5) h per axis, G[cell] the soft-min at the centre (float32, direct-form distances as the lattice kernel's). D is
1-Lipschitz, so every L <= D; the bound march u <- u + L(p(u)) then stays at or behind the march t <- t + D(p(t))
step for step, and a wave a proof takes ends with every ray gone. The per-ray proofs run in float32 as
bound_proof does; the tile proof's cone state is float64, its square roots float32 taken TILE_ROOT_REL to the
safe side (sqrt_up, sqrt_down) and its lattice term float32 throughout, x_n = origin + (float)i h being the
point G[n] was evaluated at and the base index held to [0, N - 2] with no inside test.
"""
import functools
import math

import numpy as np

F = np.float32

# ---- rm_proof.h --------------------------------------------------------------------------------
PROOF_MIN_SPHERES = 128
LATTICE_N = 64
LATTICE_MARGIN = 0.25
PROOF_MIN_STEP = 0.02
MARCH_ABS = 1e-3
BOUND_STEP_ABS = 1e-3
RADIUS_REL = 1e-6
ESCAPE_REL = 1e-5
PROOF_REL = 2e-5
PROOF_MAX_MAGNITUDE = 256.0
LATTICE_HALF_DIAG = 0.8660254
LATTICE_CELL_REL = 1e-4
LATTICE_KERNEL_ABS = 1e-3
TILE_ROOT_REL = 1e-6
TILE_ROOT_FLOOR = 1e-15
TILE_LATTICE_REL = 2e-6
TILE_ROUND_ABS = 1e-4
TILE_CONE_REL = 1e-4
TILE_CONE_ABS = 2e-6
TILE_RECEDE_REL = 2e-6
BALL_ABS = MARCH_ABS + BOUND_STEP_ABS
TILE_LATTICE_ABS = MARCH_ABS + BOUND_STEP_ABS + LATTICE_KERNEL_ABS + TILE_ROUND_ABS
PROOF_DIST_UP = 1.0000200005

MSHARP = 15.0
GONE_D = max(6.0, 130.0 / (MSHARP * 1.44269504))


# ---- scenes and rays ---------------------------------------------------------------------------

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


# ---- write_bound ---------------------------------------------------------------------------------

def soft_min(p, c, r, k):
    x = -k * (np.linalg.norm(p[:, None, :] - c, axis=-1) - r)
    m = x.max(-1)
    return -(m + np.log(np.exp(x - m[:, None]).sum(-1))) / k


def threshold_table(S, rp):
    """T(n) of write_bound, with its own round-ups (not the proof's allowances: rm_records.h)"""
    T = [(GONE_D + rp) * (1 + 1e-6)]
    for _ in range(S):
        y = T[-1] * 1.0000101
        T.append((rp + math.sqrt(2 * y * y * (1 + 1e-6) - rp * rp)) * 0.5 * (1 + 1e-5) + 1e-6)
    return np.asarray(T) * (1 + 1e-6)


class Geometry:
    """write_bound's figures for a scene: bounding sphere, R', R_soft, rs, T(n), the lattice's layout. The
    keyword arguments are the mutants of the soft ball: every allowance of rs and of the proof's distance test
    scaled by `margin`, R_soft by `radius_scale`, and with count=False the sum over the spheres replaced by its
    largest term."""

    def __init__(self, sc, k, S=32, margin=1.0, radius_scale=1.0, count=True):
        c, r = sc["centers"].astype(np.float64), sc["radius"].astype(np.float64)
        self.c, self.r, self.k, self.S = c, r, k, S
        self.c0 = 0.5 * (c.min(0) + c.max(0))
        reach = np.linalg.norm(c - self.c0, axis=1) + r
        R = reach.max() * (1 + 1e-5) + 1e-6
        lse_slack = math.log(len(r)) / k * (1 + 1e-6) + 1e-7
        rsoft = R + math.log(np.exp(k * (reach - R)).sum() * (1 + 1e-5)) / k if count else R
        rsoft = min(rsoft * (1 + 1e-5) + 1e-6, R + lse_slack) * radius_scale
        self.rs = (rsoft + margin * MARCH_ABS) * (1 + RADIUS_REL) + margin * BOUND_STEP_ABS
        self.proof_rel = margin * PROOF_REL
        self.rprime = (R + lse_slack + MARCH_ABS) * (1 + RADIUS_REL)
        self.T = threshold_table(S, self.rprime)
        self.half = float(F(self.rprime + LATTICE_MARGIN))
        self.h = float(F(2.0 * self.half / LATTICE_N))
        self.inv_h = float(F(1.0 / self.h))
        self.slack = self.h * (LATTICE_HALF_DIAG * (1 + LATTICE_CELL_REL)) + LATTICE_KERNEL_ABS

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
        """the cell reader's L(p) for points p [n, 3] and its soft-ball term; the keyword arguments are the mutants"""
        p = np.asarray(p, dtype)
        e = p - self.c0.astype(dtype)
        dist = np.sqrt((e * e).sum(-1))
        f = np.clip((e + dtype(self.half)) * dtype(self.inv_h), -1.0, float(LATTICE_N))
        i = np.floor(f).astype(np.int64)
        inside = ((i >= 0) & (i < LATTICE_N)).all(-1)
        if wrap:  # no inside test: the cell the unclamped index addresses in the table
            i = np.floor((e + dtype(self.half)) * dtype(self.inv_h)).astype(np.int64)
            cell, use = i % LATTICE_N, np.ones(len(p), bool)
        else:
            cell, use = np.clip(i, 0, LATTICE_N - 1), inside
        cell = np.clip(cell + np.array([index_shift, 0, 0]), 0, LATTICE_N - 1)
        g = np.full(len(p), -np.inf, dtype)
        if use.any():
            uniq, inv = np.unique(cell[use], axis=0, return_inverse=True)
            g[use] = self.cell_values(uniq, plus_half)[inv.reshape(-1)].astype(dtype) - dtype(slack_scale * self.slack + BALL_ABS)
        ball = dist - dtype(self.rs)
        return np.maximum(ball, g), ball


def guard_ok(g, o):
    return np.abs(o).sum(-1) + np.abs(g.c0).sum() + 3.0 * g.T[0] <= PROOF_MAX_MAGNITUDE


# ---- the soft ball against the true march, in fp64 ---------------------------------------------

def run(sc, o, d, k, S, **mutant):
    """The march and the soft ball's bound march side by side: (rays accepted, violations of u <= t)."""
    g = Geometry(sc, k, S, **mutant)
    c, r, c0, T = g.c, g.r, g.c0, g.T
    n = len(o)
    t, u = np.zeros(n), np.zeros(n)
    active = np.ones(n, bool)   # the bound march of the ray still runs
    accepted = np.zeros(n, bool)
    violations = 0
    for st in range(S):
        e = o + d * u[:, None] - c0
        dist = np.linalg.norm(e, axis=1)
        accepted |= active & ((e * d).sum(1) >= 0) & (dist * (1 - g.proof_rel) >= T[S - st])
        active &= ~accepted
        Lb = dist - g.rs
        active &= Lb > 0          # a ray the bound cannot move is given up
        t = t + soft_min(o + d * t[:, None], c, r, k)
        u = np.where(active, u + Lb, u)
        violations += int((active & (u > t)).sum())
    return accepted, violations


# ---- bound_proof: the per-ray bound march and the proof of a wave ------------------------------

def proof(g, o, d, t1, lattice=True, **mutant):
    """bound_proof from step 1 in float32 for the rays o, d [n, 3] at march distance t1 (the shared
    origin step taken): (u per step [S + 1, n], nan where the bound march of the ray has ended; proven;
    given_up: a ray's bound step fell to kProofMinStep before it was proven)."""
    S = g.S
    o, d = o.astype(F), d.astype(F)
    c0 = g.c0.astype(F)
    e = o - c0
    gone = ((e * d).sum(-1) >= 0) & (np.sqrt((e * e).sum(-1)) * F(1 - ESCAPE_REL) >= F(g.T[S]))  # wave_escaped(0)
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
        proven |= act & ((e * d).sum(-1) >= 0) & (dist * F(1 - PROOF_REL) >= F(g.T[S - n]))
        if lattice:
            Lb = g.bound(p, F, **mutant)[0]
        else:
            Lb = dist - F(g.rs)
        given_up |= ~proven & ~(Lb > F(PROOF_MIN_STEP))
        u = np.where(proven | given_up, u, u + Lb).astype(F)
    return traj, proven, given_up


def waves_taken(g, o, d, t1, tiles, lattice=True):
    """the waves the restated proof takes: the magnitude guard holds for every ray and every ray is proven
    (a ray whose bound step falls to kProofMinStep is never proven here; in the kernel it ends its wave's
    proof at that step: the same waves)"""
    traj, proven, _ = proof(g, o, d, t1, lattice)
    taken = [w for w, idx in enumerate(tiles) if guard_ok(g, o[idx]).all() and proven[idx].all()]
    return np.asarray(taken, int), traj, proven


# ---- rm_tile_proof_kernel ------------------------------------------------------------------------

CORNERS = [0, 7, 56, 63]  # of an 8x8 tile in row order: the tile's extreme rays


def sqrt_up(x):
    """the kernel's square roots are fp32, each taken TILE_ROOT_REL relative to the safe side"""
    return np.sqrt(np.asarray(x, np.float64).astype(F)).astype(np.float64) * (1 + TILE_ROOT_REL) + TILE_ROOT_FLOOR


def sqrt_down(x):
    return np.sqrt(np.asarray(x, np.float64).astype(F)).astype(np.float64) * (1 - TILE_ROOT_REL)


def lattice_bound(g, p, plus_half=True):
    """the lattice term of the tile reader's L at points p [n, 3] (float64): max over the 8 lattice points around p"""
    p = np.asarray(p, np.float64)
    e = (p - g.c0).astype(F)
    f = np.clip((e + F(g.half)) * F(g.inv_h) - F(0.5), F(0), F(LATTICE_N - 2))  # float32, as the kernel's: any index is valid
    i0 = f.astype(np.int64)
    best = np.full(len(p), -np.inf, F)
    idx = np.concatenate([i0 + np.array([c & 1, (c >> 1) & 1, c >> 2]) for c in range(8)])
    uniq, inv = np.unique(idx, axis=0, return_inverse=True)
    G = g.cell_values(uniq)[inv.reshape(-1)].reshape(8, len(p))
    for c in range(8):
        xn = g.centres(idx[c * len(p):(c + 1) * len(p)], plus_half)  # float32: G's own points unless mutated
        q = p.astype(F) - xn
        q2 = q * q
        dn = np.sqrt((q2[:, 0] + q2[:, 1]) + q2[:, 2])
        best = np.maximum(best, G[c] - dn * F(1 + TILE_LATTICE_REL))
    return best.astype(np.float64) - TILE_LATTICE_ABS


def bound(g, p, **mutant):
    """the tile reader's L(p) and its soft-ball term"""
    ball = sqrt_down(((np.asarray(p, np.float64) - g.c0) ** 2).sum(1)) - g.rs
    return np.maximum(ball, lattice_bound(g, p, **mutant)), ball


def cone(d4, delta_scale=1.0):
    """(d_c, delta) of tiles with corner rays d4 [tiles, 4, 3] (float32)"""
    d4 = d4.astype(np.float64)
    dc = (d4[:, 0] + d4[:, 1]) + (d4[:, 2] + d4[:, 3])
    dc *= (F(1) / np.sqrt((dc * dc).sum(1).astype(F))).astype(np.float64)[:, None]  # an fp32 reciprocal square root
    delta = sqrt_up(((d4 - dc[:, None, :]) ** 2).sum(2)).max(1)
    return dc, delta_scale * delta * (1 + TILE_CONE_REL) + TILE_CONE_ABS


def tile_proof(g, eye, d4, u0, st0=1, lattice=True, drop_ud=False, delta_scale=1.0, plus_half=True, stale_ud=False,
               centre_recedes=False):
    """rm_tile_proof_kernel for tiles of one view: (taken [tiles]; u at the top of every bound step [S + 1, tiles],
    nan where the tile's bound march has ended; the step at which a taken tile was proven). The keyword
    arguments after `lattice` are the mutants."""
    S = g.S
    eye = np.asarray(eye, F).astype(np.float64)
    dc, delta = cone(d4, delta_scale)
    nt = len(dc)
    oc = eye - g.c0
    rec0 = dc @ oc - (0.0 if centre_recedes else sqrt_up((oc * oc).sum())) * delta
    ok = np.abs(eye).sum() + np.abs(g.c0).sum() + 3.0 * g.T[0] <= PROOF_MAX_MAGNITUDE
    u = np.full(nt, float(u0))
    u_prev = u.copy()
    run = np.full(nt, bool(ok))
    taken = np.zeros(nt, bool)
    at = np.full(nt, -1)
    traj = np.full((S + 1, nt), np.nan)
    for n in range(st0, S):
        if not run.any():
            break
        traj[n, run] = u[run]
        p = eye + dc * u[:, None]
        dist = sqrt_down(((p - g.c0) ** 2).sum(1))
        ud = np.abs(u_prev if stale_ud else u) * delta
        proven = run & (rec0 + u * np.where(u >= 0, 1 - TILE_RECEDE_REL, 1 + TILE_RECEDE_REL) >= 0) & \
            (dist - ud >= g.T[S - n] * PROOF_DIST_UP)
        taken |= proven
        at[proven] = n
        run &= ~proven
        Lb = dist - g.rs
        if lattice and run.any():
            Lb[run] = np.maximum(Lb[run], lattice_bound(g, p[run], plus_half))
        step = Lb - (0.0 if drop_ud else ud)
        run &= step > PROOF_MIN_STEP
        u_prev = u.copy()
        u = np.where(run, u + step, u)
    return taken, traj, at


def shared_t1(m_t1, o, d, g):
    """the t every ray of a view that is not gone at the eye has after the origin step"""
    e = o[0].astype(np.float64) - g.c0
    gone0 = (d.astype(np.float64) @ e >= 0) & (np.linalg.norm(e) * (1 - ESCAPE_REL) >= g.T[g.S])
    live = np.flatnonzero(~gone0)
    return (m_t1[live[0]] if len(live) else m_t1[0]), gone0


def model_bytes(oracle, sc, cam, w, h, S, k):
    """the kernel's byte per tile of one view, in wave_tiles(w, h)'s order, and the view's rays and their t after
    the origin step"""
    g = Geometry(sc, k, S)
    o, d = view_rays(oracle, w, h, cam)
    t1 = np.asarray(oracle.render_diff(o, d, sc, 1, k, precision="f32", with_t=True)[1], F)
    tiles = wave_tiles(w, h)
    u0, gone0 = shared_t1(t1, o, d, g)
    return tile_proof(g, o[0], d[tiles[:, CORNERS]], u0)[0], (g, o, d, t1, tiles, gone0)


def model_taken(oracle, sc, cam, w, h, S, k):
    """(tiles the cone takes, tiles the soft-ball proof takes, tiles the per-ray lattice proof took) of one view,
    as index sets over wave_tiles(w, h); a tile whose rays are all gone at the eye counts for none"""
    taken, (g, o, d, t1, tiles, gone0) = model_bytes(oracle, sc, cam, w, h, S, k)
    ball = waves_taken(g, o, d, t1, tiles, lattice=False)[0]
    ray = waves_taken(g, o, d, t1, tiles)[0]
    keep = set(np.flatnonzero(~gone0[tiles].all(1)))
    return set(np.flatnonzero(taken)) & keep, set(ball) & keep, set(ray) & keep


# ---- the scenes and views of the tests, and what is computed once for them ---------------------

SCENES = [("gap", gap_scene, 128, 32.0), ("outlier", outlier_scene, 300, 32.0),
          ("coincident", coincident_scene, 128, 5.0), ("cloud", cloud_scene, 300, 5.0),
          ("outlier", outlier_scene, 128, 5.0), ("coincident", coincident_scene, 300, 32.0)]

VIEWS = {  # per kind of scene: views of 32x32 rays (16 waves each) that pass beside, through and into the scene
    "gap": [([0.0, 0.1, 2.6], [0.0, 0.0, 0.0], 40.0), ([1.5, 0.4, 2.2], [0.0, 0.0, 0.0], 60.0)],
    "outlier": [([0.0, 0.5, 2.5], [0.0, 0.0, 0.0], 60.0), ([2.4, -0.3, 0.4], [0.3, 0.9, 0.0], 60.0)],
    "coincident": [([0.0, 0.3, 2.0], [0.6, 0.0, 0.0], 60.0)],
    "cloud": [([0.0, 0.5, 2.5], [0.9, 0.5, 0.0], 50.0), ([0.9, 0.2, 0.6], [0.0, 0.0, 0.0], 70.0)],
}

GAP_CAM = ([0.0, 0.0, 2.2], [0.0, 0.0, 0.0], 50.0)  # the eye on the z axis, looking through the gap: both clusters show
FAR_VIEW = ([0.0, 0.5, 12.0], [0.0, 0.0, 0.0], 90.0)  # a far eye, a wide field: the rays turn to receding at different u


def sample_points(g, seed):
    """1e5 points: uniform over the cube and a rim about it; on cell faces, edges and corners (exactly on
    the lattice planes and a few ulps to either side); just inside and outside the cube; inside spheres."""
    rng = np.random.default_rng(seed)
    half, h = g.half, g.h
    pts = [rng.uniform(-1.3 * half, 1.3 * half, (25000, 3))]
    for axes, n in ((1, 15000), (2, 15000), (3, 15000)):  # faces, edges, corners
        e = rng.uniform(-half, half, (n, 3))
        planes = -half + rng.integers(0, LATTICE_N + 1, (n, 3)) * h + rng.choice([0.0, 1e-6, -1e-6, 1e-4, -1e-4], (n, 3)) * h
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


@functools.lru_cache(maxsize=None)
def sampled():
    """per scene: the geometry, the points and the true soft-min there. Computed once for every module that
    asks; read, never written."""
    out = []
    for n, (kind, make, M, k) in enumerate(SCENES[:4]):
        g = Geometry(make(M), k)
        p = sample_points(g, 100 + n)
        D = np.concatenate([soft_min(p[i:i + 20000], g.c, g.r, k) for i in range(0, len(p), 20000)])
        out.append((kind, M, k, g, p, D))
    return tuple(out)


def _marched_view(oracle, kind, M, k, S, sc, cam):
    g = Geometry(sc, k, S)
    o, d = view_rays(oracle, 32, 32, cam)
    return dict(kind=kind, M=M, k=k, S=S, g=g, o=o, d=d, t=oracle_march(oracle, o, d, sc, S, k),
                mask=np.asarray(oracle.render_diff_debug(o, d, sc, S, k, "f32")[:, 10]))


@functools.lru_cache(maxsize=None)
def marched(oracle):
    """per scene, step count and view: the fp32 oracle march and mask of its 32x32 rays and the per-ray proof's
    waves. Computed once (`oracle`: the oracle module); read, never written."""
    out = []
    for kind, make, M, k in SCENES:
        sc = make(M)
        for S in (8, 32):
            for cam in VIEWS[kind]:
                m = _marched_view(oracle, kind, M, k, S, sc, cam)
                m["taken"], m["traj"], m["proven"] = waves_taken(m["g"], m["o"], m["d"], m["t"][1], wave_tiles(32, 32))
                out.append(m)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cones(oracle):
    """per marched view, and a far wide one: its 16 tiles, their corner rays and the t they share after the
    origin step, for the tile proof. Copies: marched()'s own entries stay as they are."""
    out = [dict(m) for m in marched(oracle)]
    out.append(dict(_marched_view(oracle, "far", 300, 32.0, 32, cloud_scene(300), FAR_VIEW)))
    tiles = wave_tiles(32, 32)
    for m in out:
        m["tiles"] = tiles
        m["d4"] = m["d"][tiles[:, CORNERS]]
        m["t1"], m["gone0"] = shared_t1(m["t"][1], m["o"], m["d"], m["g"])
    return tuple(out)


# ---- the GPU tests' cases ------------------------------------------------------------------------

def _plane_cams(sc, k):
    """eye and target on a cell face of the lattice (y = a lattice plane): the central ray runs along it"""
    g = Geometry(sc, k)
    y = g.c0[1] - g.half + 40 * g.h
    return [([g.c0[0] + 0.3, y, g.c0[2] + 2.5], [g.c0[0] - 0.5, y, g.c0[2]], 50.0)]


TWO_BLOCK_CAM = ([0.0, 0.5, 2.5], [1.2, 0.5, 0.0], 40.0)

FAR = np.array([29.0, -29.0, 29.0])  # 50.2 from the origin

# name: (scene, cameras, (w, h), march steps, k)
CASES = {
    "beside": lambda: (cloud_scene(300), [([0.0, 0.5, 2.5], [2.2, 0.5, 0.0], 20.0)], (48, 80), 32, 32.0),
    "gap": lambda: (gap_scene(128), [GAP_CAM], (48, 80), 32, 32.0),
    "gap-two-views": lambda: (gap_scene(128), [GAP_CAM, ([0.3, 0.2, -2.6], [0.0, 0.0, 0.0], 30.0)], (64, 64), 32, 32.0),
    "in-cube-outside-cloud": lambda: (cloud_scene(300), [([0.9, 0.35, 0.3], [0.0, 1.6, 0.0], 70.0)], (64, 64), 32, 32.0),
    "inside-cloud": lambda: (cloud_scene(300), [([0.05, 0.0, -0.1], [1.0, 0.3, 0.2], 70.0)], (48, 80), 32, 32.0),
    "far-from-origin": lambda: (cloud_scene(128, centre=FAR), [(list(FAR + [0.0, 0.5, 2.5]), list(FAR + [1.6, 0.5, 0.0]), 40.0)],
                                (64, 64), 8, 32.0),
    "one-centre": lambda: (coincident_scene(128), [([0.0, 0.3, 2.0], [0.6, 0.0, 0.0], 60.0)], (48, 80), 8, 5.0),
    "outliers-k5": lambda: (outlier_scene(300), [([0.0, 0.5, 3.5], [2.0, 0.5, 0.0], 40.0)], (64, 64), 32, 5.0),
    "lattice-plane": lambda: (outlier_scene(128), _plane_cams(outlier_scene(128), 32.0), (64, 64), 32, 32.0),
    # 520 spheres: Mpad = 544, 272 pairs, two blocks of the record kernel -- the smallest scene whose record
    # buffer has partial headers, so the lattice geometry (and every section behind the header) sits
    # elsewhere than in the one-block cases above. The eye is "beside"'s, turned towards the cloud: at
    # "beside" itself both proofs take all 60 waves.
    "two-record-blocks": lambda: (cloud_scene(520), [TWO_BLOCK_CAM], (48, 80), 32, 32.0),
}


def _train(mods, sc, cams, w, h, S, k):
    """one camera train step on the GPU and its rm_stats counters; mods = (torch, model, render, native)"""
    torch, _, render, _ = mods
    tgt = torch.full((len(cams) * w * h, 3), 0.25, device="cuda")
    out = torch.empty_like(tgt)
    ctx = render.context()
    ctx.stats(True)
    ctx.collect_stats(reset=True)
    loss, g, _ = render.train_step_camera(cams, w, h, tgt, sc, k, 0.5, S, out=out)
    torch.cuda.synchronize()
    st = ctx.collect_stats(reset=True)
    ctx.stats(False)
    return dict(loss=loss.clone(), out=out.clone(), **{key: v.clone() for key, v in g.items()}), st
