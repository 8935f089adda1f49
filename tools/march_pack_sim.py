"""Study (numpy, float32; not product code): how much of the march's matrix-core work the rays
of the bench workload need, step by step, and what packing the live rays of a wave into fewer
16-ray column blocks (lse_mfma) can recover.

Random 8x8 wave tiles of the ring views march the seed-0 scene with the expansion-form q in
float32. Per step a ray is
  gone   once the doubling bound of write_bound proves that it escapes (sticky),
  known  when its t equals its t one or two steps back (its D is the D of that step),
  live   otherwise;
a wave runs until every ray is gone (escape exit) or every ray that is not gone repeats with
period 2 (cycle exit). Step 0 is the shared origin step of camera mode and is not counted.

Printed: the live share of the executed lane-steps, the share of column blocks whose 16 rays are
all not live for the 8x2-pixel grouping (the kernel's lane map) and for a 4x4 grouping, the
column blocks ceil(live / 16) a packed wave multiplies as a share of the four it multiplies
today, overall and per band of 8 steps, and the same with escape alone (no per-ray memo).

    python tools/march_pack_sim.py [--spheres 256] [--k 32] [--steps 32] [--size 512] [--tiles 1500]
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from burn_raymarching_amd import model as rmm  # noqa: E402

F = np.float32


def camera_rays(size, eye, target, fov):
    eye, target = np.asarray(eye, float), np.asarray(target, float)
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    th = math.tan(math.radians(fov) / 2)
    ys, xs = np.mgrid[0:size, 0:size]
    u = ((xs + 0.5) / size * 2 - 1) * th
    v = (1 - (ys + 0.5) / size * 2) * th
    d = fwd + u[..., None] * right + v[..., None] * up
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return eye.astype(F), d.astype(F)


def escape_table(steps, gone_d, rp):
    """T(n) of write_bound: a receding ray at distance >= T(n) with n steps left ends gone."""
    T = [(gone_d + rp) * (1 + 1e-6)]
    for _ in range(steps):
        y = T[-1] * 1.0000101
        T.append((rp + math.sqrt(2 * y * y * (1 + 1e-6) - rp * rp)) * 0.5 * (1 + 1e-5) + 1e-6)
    return np.asarray(T, F) * F(1 + 1e-6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spheres", type=int, default=256)
    ap.add_argument("--k", type=float, default=32.0)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--tiles", type=int, default=1500)
    ap.add_argument("--mask-sharpness", type=float, default=15.0)
    args = ap.parse_args()
    S, k = args.steps, F(args.k)
    sc = rmm.synthetic_scene(args.spheres, seed=0)
    c, r = np.asarray(sc["centers"], F), np.asarray(sc["radius"], F)
    cc = (c * c).sum(1)
    # the escape proof's scene bound and thresholds (scene_bound / write_bound)
    c0 = F(0.5) * (c.min(0) + c.max(0))
    R = float((np.linalg.norm(c - c0, axis=1) + r).max())
    gone_d = max(6.0, 130.0 / (args.mask_sharpness * 1.44269504))
    rp = (R + math.log(args.spheres) / args.k + 1e-3) * (1 + 1e-6)
    T = escape_table(S, gone_d, rp)

    rng = np.random.default_rng(0)
    cams = rmm.ring_cameras(10)
    rays = [camera_rays(args.size, *cam) for cam in cams]
    n = args.tiles
    o = np.empty((n, 64, 3), F)
    d = np.empty((n, 64, 3), F)
    for i in range(n):
        eye, dv = rays[i % len(cams)]
        ty, tx = rng.integers(0, args.size // 8, 2)
        o[i] = eye
        d[i] = dv[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8].reshape(64, 3)  # lane = 8 y + x

    # lane -> 16-ray column block: 8x2 pixels (the kernel's map, lane >> 4) and 4x4 pixels
    ly, lx = np.divmod(np.arange(64), 8)
    groups = {"8x2": np.arange(64) >> 4, "4x4": 2 * (ly >> 2) + (lx >> 2)}

    t = np.zeros((n, 64), F)
    t1 = np.full((n, 64), np.nan, F)
    t2 = np.full((n, 64), np.nan, F)
    gone = np.zeros((n, 64), bool)
    running = np.ones(n, bool)
    nb = (S + 7) // 8
    wave_steps = np.zeros(nb)
    live_lanes = np.zeros(nb)
    packed = np.zeros(nb)
    packed_escape = np.zeros(nb)
    dead_blocks = {g: 0.0 for g in groups}
    for st in range(S):
        p = o + d * t[..., None]
        e = p - c0
        dist = np.sqrt((e * e).sum(-1))
        receding = (e * d).sum(-1) >= 0
        gone |= receding & (dist * F(1 - 1e-5) >= T[S - st])
        running &= ~gone.all(1)  # escape exit
        # expansion-form squared distances, clamp, soft-min
        q = (p * p).sum(-1)[..., None] - F(2) * (p @ c.T) + cc
        rho = np.sqrt(np.maximum(q, F(1e-6)))
        x = -k * (rho - r)
        m = x.max(-1, keepdims=True)
        D = -(m[..., 0] + np.log(np.exp(x - m).sum(-1, dtype=F))) / k
        known = (t == t1) | (t == t2)
        live = ~gone & ~known
        if st > 0:  # step 0: the shared origin step
            b = st // 8
            w = running
            wave_steps[b] += w.sum()
            live_lanes[b] += live[w].sum()
            packed[b] += ((live[w].sum(1) + 15) // 16).sum()
            packed_escape[b] += (((~gone[w]).sum(1) + 15) // 16).sum()
            for g, lane_block in groups.items():
                for blk in range(4):
                    dead_blocks[g] += (~live[w][:, lane_block == blk]).all(1).sum()
        # cycle exit: every ray that is not gone repeats with period 2 (this step's state is known)
        running &= ~(gone | (t == t2)).all(1)
        t2, t1 = t1, t
        t = np.where(gone, t + (dist - F(rp)), t + D).astype(F)
        t = np.minimum(t, F(1e15))
        if not running.any():
            break

    ws = wave_steps.sum()
    print(f"spheres {args.spheres}, k {args.k:g}, steps {S}, {args.size}x{args.size}, tiles {n}: "
          f"wave-steps executed {int(ws)} of {n * (S - 1)}")
    print(f"  live lane share of the executed lane-steps: {live_lanes.sum() / (64 * ws):.3f}")
    for g in groups:
        print(f"  column blocks with no live ray, {g} grouping: {dead_blocks[g] / (4 * ws):.3f}")
    print(f"  packed column blocks ceil(live / 16), share of today's: {packed.sum() / (4 * ws):.3f}")
    print(f"  saved by escape alone (no per-ray memo): {1 - packed_escape.sum() / (4 * ws):.3f}")
    print("  steps   packed share   wave-steps")
    for b in range(nb):
        if wave_steps[b] > 0:
            share = packed[b] / (4 * wave_steps[b])
            print(f"  {8 * b:2d}-{min(8 * b + 7, S - 1):2d}   {share:.3f}          {int(wave_steps[b])}")


if __name__ == "__main__":
    main()
