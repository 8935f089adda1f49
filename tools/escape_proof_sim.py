"""Study (numpy, float32; not product code): how many waves of the bench workload a lower-bound
march proves gone before they march ("Exact early exits"), what that saves and
what the proof itself costs, per bound family.

The march is tools/march_pack_sim.py's: random 8x8 wave tiles of the ring views, expansion-form
q in float32, escape exit, cycle exit, packed column blocks. The proof runs at the top of a step
(step 1, right after the shared origin step; retries at later steps) on the waves still marching:
every lane that is not gone marches the bound trajectory
    u <- u + L(p(u)) - 1e-3         L <= the soft-min, 1-Lipschitz
from its t for the steps left and is proven once the bound point recedes from c_0 at distance
dist (1 - 2e-5) >= T(steps left). u <= t at every step (t + L(p(t)) is non-decreasing in t), so
the ray itself is then receding and at least as far out: the march's own escape test holds for it.
A wave whose lanes are all gone or proven stops; otherwise nothing changes.

Bound families:
  ball      L = |p - c_0| - R'                                        (the gone rays' step)
  radial    L = softmin_j(|rho - rho_j| - r_j), rho = |p - c_0|       (exact, no table error)
  softball  L = |p - c_0| - R_soft, R_soft = (1/k) ln sum_j exp(k (|c_j - c_0| + r_j)): the radial bound
            past every centre, valid everywhere (|rho - rho_j| >= rho - rho_j)
  radtab    the radial bound read from a table, a variant that was built and not kept (HISTORY.md §3): 255 cell
            bounds (L(i h) + L((i + 1) h) - h) / 2 over [0, R'), the soft ball outside
  ballsK    L = -(1/k) ln sum_c n_c exp(-k (|p - C_c| - R_c)) - 1e-3, K balls over Morton-order
            runs of the spheres, R_c >= |c_j - C_c| + r_j, n_c members
  gridN[:m] the larger of the soft ball and a lattice bound: N^3 cell-centre soft-min values (direct-form distances,
            float32) over the cube of half-side R' + m (default 0.25) about c_0, spacing h = 2 (R' + m) / N, each less
            h sqrt(3)/2 (1 + 1e-5) + 1e-3 -- the soft-min is 1-Lipschitz and no point of a cell is further than the
            half-diagonal from its centre; the cell is floor((p - c_0 + half) / h) per axis, and outside the cube the
            bound is the soft ball alone. One table read per bound step whatever N: K = 1 in the cost model, the
            lattice build (N^3 M evaluations per call) not counted
  ngridN[:m] the same lattice read at the 8 points around p, each with its actual distance: max_n G[n] - |p - x_n|
            (1 + 1e-6) - 2e-3, and the soft ball. No half-diagonal slack, no inside test. K = 8
  cone:FAM  FAM's bound marched once per tile instead of once per ray (rm_tile_proof_kernel): the centre direction
            of the tile's corner rays, every step less |u| delta, the conservative distance and receding tests
            (prove_cone). Cost: a 64th of a wave's bound step per tile step

softball, radial and radtab print the same figures on the bench scenes: every proof the radial bound finds
comes from rho past the outermost centre, where it is exactly rho - R_soft. That is the finding the kernel
rests on (it steps by the soft ball alone); the three rows are kept to show it.

Cost of the proof in real-step units: (bound steps a wave runs) x (K + 1) / Mpad, the wave
stopping when every lane is proven or a lane's bound step is <= 0 (it cannot be proven).

    python tools/escape_proof_sim.py [--params DIR/params_activated.npy] [--spheres 256] [--k 32]
                                     [--steps 32] [--size 512] [--tiles 3000]
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from burn_raymarching_amd import model as rmm  # noqa: E402
from tools.march_pack_sim import camera_rays, escape_table  # noqa: E402

F = np.float32
TRIES = (1, 3, 6, 10)


def morton_balls(c, r, K):
    """K bounding balls (C, R, n) over Morton-order runs of ceil(M / K) spheres."""
    lo, hi = c.min(0), c.max(0)
    g = np.minimum(((c - lo) / np.maximum(hi - lo, 1e-12) * 1024).astype(np.int64), 1023)
    code = np.zeros(len(c), np.int64)
    for b in range(10):
        for ax in range(3):
            code |= ((g[:, ax] >> b) & 1) << (3 * b + ax)
    order = np.argsort(code, kind="stable")
    run = -(-len(c) // K)
    C, R, n = [], [], []
    for i in range(0, len(c), run):
        j = order[i:i + run]
        cc = 0.5 * (c[j].min(0) + c[j].max(0))
        C.append(cc)
        R.append((np.linalg.norm(c[j] - cc, axis=1) + r[j]).max() * (1 + 1e-5) + 1e-6)
        n.append(len(j))
    return np.asarray(C, F), np.asarray(R, F), np.asarray(n, F)


def bound_fn(family, c, r, c0, rp, k):
    """L(p) for points p [..., 3] (float32), and the family's K for the cost model."""
    if family == "ball":
        return (lambda p: np.sqrt(((p - c0) ** 2).sum(-1)) - F(rp)), 1
    if family == "radial":
        rho_j = np.linalg.norm(c - c0, axis=1).astype(F)

        def L(p):
            rho = np.sqrt(((p - c0) ** 2).sum(-1))
            x = -k * (np.abs(rho[..., None] - rho_j) - r)
            m = x.max(-1)
            return -(m + np.log(np.exp(x - m[..., None]).sum(-1, dtype=F))) / k - F(1e-3)
        return L, 1
    if family in ("softball", "radtab"):
        # past every centre the radial bound is rho - R_soft, R_soft = (1/k) ln sum_j exp(k (rho_j + r_j)),
        # and |rho - rho_j| >= rho - rho_j makes that a bound everywhere: the ball without ln(M)/k
        x = k * (np.linalg.norm(c - c0, axis=1).astype(F) + r)
        rs = F((x.max() + np.log(np.exp(x - x.max()).sum(dtype=F))) / k * F(1 + 1e-5) + F(1e-3))
    if family == "softball":
        return (lambda p: np.sqrt(((p - c0) ** 2).sum(-1)) - rs), 1
    if family == "radtab":  # the radial bound as a kernel would read it from a table (not kept): 255 cells over [0, R')
        Lr = bound_fn("radial", c, r, c0, rp, k)[0]
        h = F(rp / 255)
        s = Lr(c0 + np.outer(np.arange(256) * h, np.asarray([1, 0, 0], F)).astype(F)) + F(1e-3)
        tab = (F(0.5) * (s[:-1] + s[1:] - h) - F(1e-3)).astype(F)

        def L(p):
            rho = np.sqrt(((p - c0) ** 2).sum(-1))
            cell = np.minimum((rho / h).astype(np.int64), 254)
            return np.where(rho / h < 255, np.maximum(tab[cell], rho - rs), rho - rs)
        return L, 1
    if family.startswith("grid") or family.startswith("ngrid"):
        name, _, mg = family.partition(":")
        neighbours = name.startswith("n")
        N, margin = int(name[5 if neighbours else 4:]), float(mg) if mg else 0.25
        Ls = bound_fn("softball", c, r, c0, rp, k)[0]
        half = F(rp + margin)
        h = F(2) * half / F(N)
        inv_h = F(1) / h
        ax = -half + (np.arange(N, dtype=F) + F(0.5)) * h
        G = np.empty((N, N, N), F)  # [iz, iy, ix]
        gy, gx = np.meshgrid(ax, ax, indexing="ij")
        for iz in range(N):
            e = (c0 + np.stack([gx, gy, np.full_like(gx, ax[iz])], -1))[..., None, :] - c
            x = -k * (np.sqrt(np.maximum((e * e).sum(-1), F(1e-6))) - r)
            m = x.max(-1)
            G[iz] = -(m + np.log(np.exp(x - m[..., None]).sum(-1, dtype=F))) / k
        if neighbours:
            def Ln(p):  # the 8 lattice points around p, each with its actual distance; no inside test (base index held)
                e = (p - c0).astype(np.float64)
                i0 = np.floor(np.clip((e + half) * inv_h - 0.5, 0, N - 2)).astype(np.int64)
                best = Ls(p).astype(np.float64)
                for cnr in range(8):
                    i = i0 + np.array([cnr & 1, (cnr >> 1) & 1, cnr >> 2])
                    dn = np.sqrt(((e - ax[i]) ** 2).sum(-1))
                    best = np.maximum(best, G[i[..., 2], i[..., 1], i[..., 0]] - dn * (1 + 1e-6) - 2e-3)
                return best.astype(F)
            return Ln, 8
        G -= h * F(math.sqrt(3) / 2 * (1 + 1e-5)) + F(1e-3)

        def L(p):
            i = np.floor((p - c0 + half) * inv_h)
            inside = ((i >= 0) & (i < N)).all(-1)
            i = np.clip(i, 0, N - 1).astype(np.int64)
            return np.maximum(Ls(p), np.where(inside, G[i[..., 2], i[..., 1], i[..., 0]], -np.inf)).astype(F)
        return L, 1
    C, R, n = morton_balls(c, r, int(family[5:]))
    ln_n = np.log(n)

    def L(p):
        x = ln_n - k * (np.sqrt(((p[..., None, :] - C) ** 2).sum(-1)) - R)
        m = x.max(-1)
        return -(m + np.log(np.exp(x - m[..., None]).sum(-1, dtype=F))) / k - F(1e-3)
    return L, len(C)


def prove(L, o, d, t, gone, st, S, c0, T, min_step=0.0):
    """The bound march of the lanes [n, 64] from step st: lanes proven, bound steps the wave runs."""
    u = t.copy()
    proven = gone.copy()
    alive = np.ones(len(u), bool)  # the wave's proof still runs
    steps_run = np.zeros(len(u))
    for n in range(st, S):
        p = o + d * u[..., None]
        e = p - c0
        dist = np.sqrt((e * e).sum(-1))
        proven |= alive[:, None] & ((e * d).sum(-1) >= 0) & (dist * F(1 - 2e-5) >= T[S - n])
        alive &= ~proven.all(1)
        if not alive.any():
            break
        step = (L(p[alive]) - F(1e-3)).astype(F)
        stuck = ((step <= min_step) & ~proven[alive]).any(1)
        steps_run[alive] += 1
        ua = u[alive] + np.maximum(step, 0)
        u[alive] = np.where(proven[alive], u[alive], ua)
        idx = np.flatnonzero(alive)
        alive[idx[stuck]] = False
    return proven.all(1), steps_run


def prove_cone(L, o, d, t, gone, st, S, c0, T, min_step=0.0):
    """One bound march per tile [n, 64] (rm_tile_proof_kernel's conservative cone): d_c the normalised sum of the
    tile's corner rays, delta >= |d_r - d_c|, u <- u + L(p_c(u)) - 1e-3 - |u| delta from the smallest t of the lanes
    not gone; proven once (o - c_0) . d_c - |o - c_0| delta + u (1 - 2e-6) >= 0 and
    |p_c - c_0| - |u| delta >= T(steps left) / (1 - 2e-5)."""
    d4 = d[:, [0, 7, 56, 63]].astype(np.float64)
    dc = d4.sum(1)
    dc /= np.linalg.norm(dc, axis=-1, keepdims=True)
    delta = np.linalg.norm(d4 - dc[:, None], axis=-1).max(1) * (1 + 1e-4) + 2e-6
    eye = o[:, 0].astype(np.float64)
    oc = eye - c0
    rec0 = (oc * dc).sum(-1) - np.linalg.norm(oc, axis=-1) * delta
    alive = ~gone.all(1)
    u = np.where(gone, np.inf, t).min(1).astype(np.float64)
    u[~alive] = 0.0
    ok = ~alive
    steps_run = np.zeros(len(u))
    for n in range(st, S):
        p = eye + dc * u[:, None]
        dist = np.linalg.norm(p - c0, axis=-1)
        ud = np.abs(u) * delta
        prov = alive & (rec0 + u * (1 - 2e-6) >= 0) & (dist - ud >= T[S - n] / (1 - 2e-5))
        ok |= prov
        alive &= ~prov
        if not alive.any():
            break
        step = L(p[alive].astype(F)).astype(np.float64) - 1e-3 - ud[alive]
        steps_run[alive] += 1
        idx = np.flatnonzero(alive)
        stuck = step <= min_step
        u[idx] += np.where(stuck, 0.0, step)
        alive[idx[stuck]] = False
    return ok, steps_run / 64.0  # one lane per tile: a 64th of a wave's bound step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", default=None, help="params_activated.npy of bench.py --dump-outputs")
    ap.add_argument("--spheres", type=int, default=256)
    ap.add_argument("--k", type=float, default=32.0)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--tiles", type=int, default=3000)
    ap.add_argument("--min-step", type=float, default=0.0, help="the proof gives a wave up at a bound step <= this")
    ap.add_argument("--families", default="ball,softball,radial,radtab,balls4,balls8,balls16,balls32")
    ap.add_argument("--mask-sharpness", type=float, default=15.0)
    args = ap.parse_args()
    S, k = args.steps, F(args.k)
    if args.params:
        buf = np.load(args.params).astype(F)
        M = (len(buf) - 4) // 7
        sc = rmm.unpack(buf, M)
    else:
        M = args.spheres
        sc = rmm.synthetic_scene(M, seed=0)
    c, r = np.asarray(sc["centers"], F), np.asarray(sc["radius"], F)
    Mpad = (M + 15) // 16 * 16
    cc = (c * c).sum(1)
    c0 = F(0.5) * (c.min(0) + c.max(0))
    R = float((np.linalg.norm(c - c0, axis=1) + r).max())
    gone_d = max(6.0, 130.0 / (args.mask_sharpness * 1.44269504))
    rp = (R + math.log(M) / args.k + 1e-3) * (1 + 1e-6)
    T = escape_table(S, gone_d, rp)

    rng = np.random.default_rng(0)
    cams = rmm.ring_cameras(80)  # the bench ring
    rays = [camera_rays(args.size, *cam) for cam in cams]
    n = args.tiles
    o = np.empty((n, 64, 3), F)
    d = np.empty((n, 64, 3), F)
    for i in range(n):
        eye, dv = rays[i % len(cams)]
        ty, tx = rng.integers(0, args.size // 8, 2)
        o[i] = eye
        d[i] = dv[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8].reshape(64, 3)

    # ---- the march as it is: per step the waves running and their packed column blocks
    t = np.zeros((n, 64), F)
    t1 = np.full((n, 64), np.nan, F)
    t2 = np.full((n, 64), np.nan, F)
    gone = np.zeros((n, 64), bool)
    running = np.ones(n, bool)
    ran = np.zeros((S, n), bool)
    blocks = np.zeros((S, n))
    snap = {}
    end = np.zeros(n, int)  # 0 runs all steps, 1 escape exit, 2 cycle exit
    for st in range(S):
        p = o + d * t[..., None]
        e = p - c0
        dist = np.sqrt((e * e).sum(-1))
        gone |= ((e * d).sum(-1) >= 0) & (dist * F(1 - 1e-5) >= T[S - st])
        esc = running & gone.all(1)
        end[esc] = 1
        running &= ~esc
        if st in TRIES:
            snap[st] = (t.copy(), gone.copy(), running.copy())
        q = (p * p).sum(-1)[..., None] - F(2) * (p @ c.T) + cc
        x = -k * (np.sqrt(np.maximum(q, F(1e-6))) - r)
        m = x.max(-1, keepdims=True)
        D = -(m[..., 0] + np.log(np.exp(x - m).sum(-1, dtype=F))) / k
        live = ~gone & ~((t == t1) | (t == t2))
        if st > 0:
            ran[st] = running
            blocks[st] = np.where(running, (live.sum(1) + 15) // 16, 0)
        cyc = running & (gone | (t == t2)).all(1)
        end[cyc] = 2
        running &= ~cyc
        t2, t1 = t1, t
        t = np.minimum(np.where(gone, t + (dist - F(rp)), t + D).astype(F), F(1e15))
        if not running.any():
            break
    ws, cb = ran.sum(), blocks.sum()
    src = args.params or f"synthetic seed 0, {M} spheres"
    print(f"scene {src}: M {M}, k {args.k:g}, steps {S}, {args.size}x{args.size}, tiles {n}")
    print(f"  bounding sphere R {R:.3f} (R' {rp:.3f}), centre spread max |c - c0| {np.linalg.norm(c - c0, axis=1).max():.3f}")
    print(f"  wave-steps executed {int(ws)} of {n * (S - 1)}; packed column blocks {int(cb)}")
    for code, name in ((1, "escape exit"), (2, "cycle exit"), (0, "runs all steps")):
        w = end == code
        print(f"  {name:15s} waves {w.mean():.3f}  wave-steps {ran[:, w].sum() / ws:.3f}  blocks {blocks[:, w].sum() / cb:.3f}")
    print("  family    waves proven@1  (retries)  wave-steps saved@1 (retries)  blocks saved@1 (retries)"
          "  cost@1 (retries)  net wave-steps@1 (retries)")
    for family in args.families.split(","):
        is_cone = family.startswith("cone:")
        L, K = bound_fn(family[5:] if is_cone else family, c, r, c0, rp, k)
        done = np.zeros(n, bool)
        res = []
        sv_w = sv_b = cost = 0.0
        for st in TRIES:
            ts, gs, rs = snap.get(st, (None, None, np.zeros(n, bool)))
            w = rs & ~done
            if w.any():
                ok, steps_run = (prove_cone if is_cone else prove)(L, o[w], d[w], ts[w], gs[w], st, S, c0, T, args.min_step)
                idx = np.flatnonzero(w)[ok]
                done[idx] = True
                sv_w += ran[st:, idx].sum()
                sv_b += blocks[st:, idx].sum()
                cost += steps_run.sum() * (K + 1) / Mpad
            res.append((done.mean(), sv_w / ws, sv_b / cb, cost / ws))
        a, b = res[0], res[-1]
        print(f"  {family:{max(8, len(family))}s}  {a[0]:.3f}          ({b[0]:.3f})    {a[1]:.3f}              ({b[1]:.3f})"
              f"       {a[2]:.3f}          ({b[2]:.3f})    {a[3]:.4f} ({b[3]:.4f})  {a[1] - a[3]:.3f}             ({b[1] - b[3]:.3f})")


if __name__ == "__main__":
    main()
