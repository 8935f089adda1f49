"""Numpy restatement of the viewer's frame render (rm_view), written from its specification:

  rays    ux = (2 (i + .5) / W - 1) W / H, uy = 1 - 2 (j + .5) / H, row 0 at the top;
          ww = normalize(forward), uu = normalize(ww x up), vv = normalize(uu x ww),
          rd = normalize(ux uu + uy vv + focal ww), ro = pos
  trace   t = 0; at most max_steps times: d = D(ro + t rd); d < hit_eps -> hit, stop; else
          t > t_max -> miss, stop; else t += d. Out of iterations: a miss.
  D(p)    -log(sum_j exp(-k (|p - c_j| - r_j))) / k as a shifted log-sum-exp
  shade   n = normalize(sum_s s D(p + eps s)), s in {(1,-1,-1), (-1,-1,1), (-1,1,-1), (1,1,1)};
          col = sum_j c_j exp(-csharp d_j) / (sum_j exp(-csharp d_j) + 1e-5);
          out = col (ambient + max(n . normalize(light), 0) (1 - ambient)); a zero tap sum gives
          diff = 0; a miss is exactly 0
  depth   t at the hit, +inf for a miss

fp64 by default; dtype=np.float32 runs every operation in fp32 (the precision study of
tests/test_view_reference.py). Shared by the CPU and the GPU tests.
"""
import math

import numpy as np

TAPS = np.array([[1, -1, -1], [-1, -1, 1], [-1, 1, -1], [1, 1, 1]], np.float64)
DEFAULTS = dict(max_steps=100, smooth_k=32.0, hit_eps=1e-3, t_max=20.0, normal_eps=1e-3, color_sharpness=10.0,
                focal=1.5)

# the poses of the parity cases: (pos, yaw, pitch)
POSES = [((0.0, 0.0, -2.5), math.pi / 2, 0.0), ((1.2, 0.6, -1.6), 2.2, -0.3), ((0.0, 0.05, -0.9), math.pi / 2, 0.0),
         ((-2.0, 1.5, 1.0), -0.4, -0.55), ((1.4, 0.9, -1.5), 2.3, -0.4)]


def view_camera(pos, yaw, pitch):
    """(pos, forward, up) of the viewer's camera, the components rounded to fp32 once."""
    f = np.array([math.cos(yaw) * math.cos(pitch), math.sin(pitch), math.sin(yaw) * math.cos(pitch)])
    f /= np.linalg.norm(f)
    r = np.cross(f, [0.0, 1.0, 0.0])
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    u /= np.linalg.norm(u)
    r32 = lambda v: tuple(float(np.float32(x)) for x in v)
    return r32(pos), r32(f), r32(u)


def golden_scene(path):
    """A scene.json as the viewer draws it: the stored radii, without the training activation's +0.01."""
    import json
    sc = json.load(open(path))
    return {"centers": np.array(sc["centers"], np.float32).reshape(-1, 3),
            "colors": np.array(sc["colors"], np.float32).reshape(-1, 3),
            "radius": np.array(sc["radii"], np.float32).reshape(-1),
            "light_dir": np.array(sc["light_dir"], np.float32).reshape(3),
            "ambient": np.array(sc["ambient_intensity"], np.float32).reshape(-1)[:1]}


def synthetic_scene(m, seed):
    """The parity cases' scenes: centres U(-0.6, 0.6)^3, colours U(0, 1), radii U(0.03, 0.12),
    light (0.4, 0.8, -0.5), ambient 0.2; fp32 values."""
    rng = np.random.default_rng(seed)
    return dict(centers=rng.uniform(-0.6, 0.6, (m, 3)).astype(np.float32),
                colors=rng.uniform(0.0, 1.0, (m, 3)).astype(np.float32),
                radius=rng.uniform(0.03, 0.12, (m,)).astype(np.float32),
                light_dir=np.array([0.4, 0.8, -0.5], np.float32), ambient=np.array([0.2], np.float32))


def sdf(p, centers, radius, k):
    """D at points p [n, 3]: shifted log-sum-exp, in the dtype of p."""
    e = p[:, None, :] - centers[None, :, :]
    v = -k * (np.sqrt((e * e).sum(-1)) - radius[None, :])
    m = v.max(-1)
    return -(np.log(np.exp(v - m[:, None]).sum(-1)) + m) / k


def sdf_fold(p, centers, radius, k):
    """The shader's pairwise smin fold, unshifted (for the equivalence test)."""
    e = p[:, None, :] - centers[None, :, :]
    dist = np.sqrt((e * e).sum(-1)) - radius[None, :]
    d = dist[:, 0]
    for j in range(1, dist.shape[1]):
        d = -np.log(np.exp(-k * d) + np.exp(-k * dist[:, j])) / k
    return d


def rays(cam, width, height, focal, dtype=np.float64):
    T = dtype
    pos, fwd, up = (np.asarray(x, T) for x in cam)
    nrm = lambda v: v / np.sqrt((v * v).sum(-1, keepdims=True)).astype(T)
    ww = nrm(fwd)
    uu = nrm(np.cross(ww, up).astype(T))
    vv = nrm(np.cross(uu, ww).astype(T))
    i = np.arange(width, dtype=T)
    j = np.arange(height, dtype=T)
    ux = ((T(2) * (i + T(0.5)) / T(width) - T(1)) * (T(width) / T(height)))[None, :]
    uy = (T(1) - T(2) * (j + T(0.5)) / T(height))[:, None]
    rd = ux[..., None] * uu + uy[..., None] * vv + T(focal) * ww
    rd = nrm(rd.astype(T)).reshape(-1, 3)
    return np.broadcast_to(pos, rd.shape).astype(T), rd.astype(T)


def view(cam, width, height, scene, dtype=np.float64, return_iters=False, **params):
    """One frame: (rgb [H, W, 3], depth [H, W]) in `dtype` (and the per-ray soft-min evaluation
    count of the trace with return_iters)."""
    T = dtype
    pr = dict(DEFAULTS, **params)
    c = np.asarray(scene["centers"], T)
    col = np.asarray(scene["colors"], T)
    r = np.asarray(scene["radius"], T).reshape(-1)
    light = np.asarray(scene["light_dir"], T).reshape(3)
    amb = T(np.asarray(scene["ambient"], T).reshape(-1)[0])
    k, hit_eps, t_max, eps = T(pr["smooth_k"]), T(pr["hit_eps"]), T(pr["t_max"]), T(pr["normal_eps"])
    ro, rd = rays(cam, width, height, pr["focal"], T)
    n = rd.shape[0]
    t = np.zeros(n, T)
    hit = np.zeros(n, bool)
    live = np.ones(n, bool)
    iters = np.zeros(n, np.int64)
    for _ in range(int(pr["max_steps"])):
        idx = np.nonzero(live)[0]
        if idx.size == 0:
            break
        d = sdf((ro[idx] + t[idx, None] * rd[idx]).astype(T), c, r, k).astype(T)
        iters[idx] += 1
        is_hit = d < hit_eps
        is_far = ~is_hit & (t[idx] > t_max)
        go = ~is_hit & ~is_far
        hit[idx[is_hit]] = True
        live[idx[is_hit | is_far]] = False
        t[idx[go]] = (t[idx[go]] + d[go]).astype(T)
    rgb = np.zeros((n, 3), T)
    depth = np.full(n, np.inf, T)
    h = np.nonzero(hit)[0]
    if h.size:
        p = (ro[h] + t[h, None] * rd[h]).astype(T)
        taps = TAPS.astype(T)
        nsum = np.zeros((h.size, 3), T)
        for s in taps:
            nsum = (nsum + s[None, :] * sdf((p + eps * s[None, :]).astype(T), c, r, k)[:, None]).astype(T)
        ln = np.sqrt((nsum * nsum).sum(-1)).astype(T)
        ok = ln > 0
        nrm = np.where(ok[:, None], nsum / np.where(ok, ln, T(1))[:, None], T(0)).astype(T)
        lu = (light / np.sqrt((light * light).sum())).astype(T)
        diff = np.maximum((nrm * lu[None, :]).sum(-1), T(0)).astype(T)
        e = p[:, None, :] - c[None, :, :]
        dj = np.sqrt((e * e).sum(-1)) - r[None, :]
        w = np.exp(-T(pr["color_sharpness"]) * dj).astype(T)
        colr = ((w[:, :, None] * col[None, :, :]).sum(1) / (w.sum(1) + T(1e-5))[:, None]).astype(T)
        rgb[h] = colr * (amb + diff * (T(1) - amb))[:, None]
        depth[h] = t[h]
    out = (rgb.reshape(height, width, 3), depth.reshape(height, width))
    return out + (iters.reshape(height, width),) if return_iters else out


def srgb8(x):
    """The piecewise sRGB encode of linear values, in fp64, before rounding: 255 * encode(x)."""
    x = np.clip(np.asarray(x, np.float64), 0.0, 1.0)
    return 255.0 * np.where(x < 0.0031308, 12.92 * x, 1.055 * np.power(x, 1.0 / 2.4) - 0.055)


def parity_cases(golden_scene):
    """(name, scene, width, height, [(pos, yaw, pitch)]) of the parity study: scene.json at 64x48
    and 96x64 from four poses, 80x48 synthetic scenes of (M, seed) = (64, 0), (300, 1), (33, 2)
    from two poses."""
    cases = [("golden_64x48", golden_scene, 64, 48, POSES[:4]), ("golden_96x64", golden_scene, 96, 64, POSES[:4])]
    for m, seed in ((64, 0), (300, 1), (33, 2)):
        cases.append((f"synth_M{m}_s{seed}", synthetic_scene(m, seed), 80, 48, [POSES[0], POSES[4]]))
    return cases


def compare(rgb, depth, ref_rgb, ref_depth, rgb_tol=1e-3):
    """Parity figures of one frame against the fp64 reference: hit/miss disagreements, pixels over
    the colour tolerance among the agreeing ones, and over the rest the max / mean colour error and
    the max depth error."""
    rgb, depth = np.asarray(rgb, np.float64), np.asarray(depth, np.float64)
    hit, ref_hit = np.isfinite(depth), np.isfinite(ref_depth)
    flips = hit != ref_hit
    err = np.abs(rgb - ref_rgb).max(-1)
    over = ~flips & (err > rgb_tol)
    keep = ~flips & ~over
    both = keep & hit
    return dict(pixels=int(hit.size), hits=int(ref_hit.sum()), flips=int(flips.sum()), over=int(over.sum()),
                rgb_max=float(err[keep].max()) if keep.any() else 0.0,
                rgb_mean=float(np.abs(rgb - ref_rgb)[keep].mean()) if keep.any() else 0.0,
                depth_max=float(np.abs(depth[both] - ref_depth[both]).max()) if both.any() else 0.0,
                miss_exact=bool((rgb[~hit] == 0).all()))
