"""Restatements for the distance field's backward (rm_sdf_query_backward, render.sdf_field): TEST
INFRASTRUCTURE ONLY.

The reference is torch autograd of the field as tests/sdf_ref.py restates it -- oracle.autodiff_ref's
scene_sdf_value for D and the burn_softmax colour blend of renderer_diff.rs:64-80 -- with the points and
the scene requiring grad, for arbitrary upstream gradients gD [N] and gC [N,3]. Every function takes a
dtype: float64 is the anchor, float32 the run of the same restatement whose own error sets the GPU
bounds (8 times it, the project's convention; tests/test_gpu_sdf.py).

Also here: the analytic formulas of include/raymarch.h restated in numpy (with switches that plant the
faults the checks must catch), and the fit demonstration shared by the CPU and GPU tests."""
import numpy as np
import torch

from oracle import autodiff_ref as A

KEYS = ("centers", "colors", "radius", "points")
SEEDS = ("dist", "color", "both")


def _t(x, dtype):
    return torch.from_numpy(np.array(x, dtype=np.float32)).to(dtype)


def field_t(p, c, col, r, k, csharp):
    """(D [N], colour [N,3]) of the restatement as differentiable torch (sdf_ref.field's operations)."""
    r = r.reshape(-1, 1)
    d = A.scene_sdf_value(p, c, r, float(k)).reshape(-1)
    q = p.pow(2).sum(1, keepdim=True) + c.pow(2).sum(1, keepdim=True).t() - (p @ c.t()) * 2.0
    dists = q.clamp_min(1e-6).sqrt() - r.t()
    w = A.burn_softmax(dists * (-A._f32(csharp)), 1)
    return d, (col.unsqueeze(0) * w.unsqueeze(2)).sum(1)


def autograd(points, scene, k, csharp, g_dist, g_color, dtype=torch.float64):
    """d sum(gD D + gC . C) / d (centers, colors, radius, points) by torch autograd in dtype; fp64 numpy.
    g_dist / g_color: float32 values or None."""
    p = _t(points, dtype).reshape(-1, 3).requires_grad_(True)
    c = _t(scene["centers"], dtype).requires_grad_(True)
    col = _t(scene["colors"], dtype).requires_grad_(True)
    r = _t(scene["radius"], dtype).reshape(-1).requires_grad_(True)
    d, mixed = field_t(p, c, col, r, k, csharp)
    loss = torch.zeros((), dtype=dtype)
    if g_dist is not None:
        loss = loss + (d * _t(g_dist, dtype).reshape(-1)).sum()
    if g_color is not None:
        loss = loss + (mixed * _t(g_color, dtype).reshape(-1, 3)).sum()
    gc, gcol, gr, gp = torch.autograd.grad(loss, (c, col, r, p), allow_unused=True)
    z = lambda g, like: (torch.zeros_like(like) if g is None else g).double().numpy()
    return {"centers": z(gc, c), "colors": z(gcol, col), "radius": z(gr, r), "points": z(gp, p)}


def analytic(points, scene, k, csharp, g_dist, g_color, *, drop_point=None, shift_row=None, no_color_term=False,
             no_mask=False):
    """The header's formulas in fp64 numpy (e in direct form; the clamp decided on the restatement's
    expansion-form q). The keyword switches plant one fault each: a point left out of the scene sums, one
    sphere's rows written one sphere further, a_j without its colour term, u_j without the clamp's mask."""
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    c = np.asarray(scene["centers"], np.float32).astype(np.float64)
    col = np.asarray(scene["colors"], np.float32).astype(np.float64)
    r = np.asarray(scene["radius"], np.float32).astype(np.float64).reshape(-1)
    n, m = p.shape[0], c.shape[0]
    gD = np.zeros(n) if g_dist is None else np.asarray(g_dist, np.float32).astype(np.float64).reshape(-1)
    gC = np.zeros((n, 3)) if g_color is None else np.asarray(g_color, np.float32).astype(np.float64).reshape(-1, 3)
    cs = A._f32(csharp)
    e = p[:, None, :] - c[None, :, :]
    q = (p * p).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2.0 * (p @ c.T)
    rho = np.sqrt(np.maximum(q, 1e-6))
    d = rho - r[None, :]
    beta = np.exp(-k * (d - d.min(1, keepdims=True)))
    beta /= beta.sum(1, keepdims=True)
    w = np.exp(-cs * (d - d.min(1, keepdims=True)))
    w /= w.sum(1, keepdims=True)
    C = w @ col
    a = gD[:, None] * beta
    if not no_color_term:
        a = a - cs * w * ((gC[:, None, :] * (col[None, :, :] - C[:, None, :])).sum(2))
    mask = np.ones_like(q, bool) if no_mask else q >= 1e-6
    u = np.where(mask[:, :, None], e / rho[:, :, None], 0.0)
    au = a[:, :, None] * u
    keep = np.ones(n, bool)
    if drop_point is not None:
        keep[drop_point] = False
    out = {"centers": -au[keep].sum(0), "radius": -a[keep].sum(0), "colors": w[keep].T @ gC[keep], "points": au.sum(1)}
    if shift_row is not None:
        for key in ("centers", "radius", "colors"):
            g = out[key]
            g[(shift_row + 1) % m] = g[shift_row]
            g[shift_row] = 0.0
    return out


def max_err(a, b, rows=None):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    x = np.abs(a - b)
    if rows is not None:
        x = x[rows]
    return float(x.max()) if x.size else 0.0


def seed_sets(n, seed=22):
    """The three seed sets of the parity tests for n points: {"dist": (gD, None), "color": (None, gC),
    "both": (gD, gC)}, float32 standard normals."""
    rng = np.random.default_rng(seed)
    gD = rng.normal(size=n).astype(np.float32)
    gC = rng.normal(size=(n, 3)).astype(np.float32)
    return {"dist": (gD, None), "color": (None, gC), "both": (gD, gC)}


def bounds(points, far, scene, k, csharp, g_dist, g_color):
    """8 x the fp32 restatement's max error against fp64 over the whole pool, per output; the point
    gradient separately over the near and the far points. Returns ({output: bound}, fp64 gradients)."""
    g64 = autograd(points, scene, k, csharp, g_dist, g_color, torch.float64)
    g32 = autograd(points, scene, k, csharp, g_dist, g_color, torch.float32)
    b = {key: 8.0 * max_err(g32[key], g64[key]) for key in ("centers", "colors", "radius")}
    b["points_near"] = 8.0 * max_err(g32["points"], g64["points"], ~far)
    b["points_far"] = 8.0 * max_err(g32["points"], g64["points"], far)
    return b, g64


def errors(got, ref, far):
    """The figures `bounds` bounds, of gradients `got` against the fp64 `ref` at the same points."""
    e = {key: max_err(got[key], ref[key]) for key in ("centers", "colors", "radius") if got.get(key) is not None}
    if got.get("points") is not None:
        e["points_near"] = max_err(got["points"], ref["points"], ~far)
        e["points_far"] = max_err(got["points"], ref["points"], far)
    return e


# ---- the fit demonstration ---------------------------------------------------------------------
FIT_K, FIT_CS, FIT_STEPS, FIT_LR = 32.0, 10.0, 200, 0.01


def fit_problem(seed=22):
    """Target: three spheres on the y axis; samples: 400 seeded unit directions per sphere as surface
    points, those with |D_target| < 0.02 kept, target colours from the fp64 restatement; model start:
    centres displaced by 0.08 per axis, radii 0.15, colours 0.5. float32 numpy throughout."""
    target = {"centers": np.array([[0, -0.4, 0], [0, 0, 0], [0, 0.4, 0]], np.float32),
              "radius": np.array([0.25, 0.22, 0.20], np.float32),
              "colors": np.array([[0.9, 0.2, 0.1], [0.2, 0.8, 0.3], [0.1, 0.3, 0.9]], np.float32)}
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(3, 400, 3))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    pts = (target["centers"][:, None, :] + target["radius"][:, None, None] * u).reshape(-1, 3).astype(np.float32)
    with torch.no_grad():
        d, col = field_t(_t(pts, torch.float64), _t(target["centers"], torch.float64), _t(target["colors"], torch.float64),
                         _t(target["radius"], torch.float64), FIT_K, FIT_CS)
    keep = d.abs().numpy() < 0.02
    start = {"centers": (target["centers"] + np.float32(0.08)).astype(np.float32),
             "radius": np.full(3, 0.15, np.float32), "colors": np.full((3, 3), 0.5, np.float32)}
    return pts[keep], col.numpy()[keep].astype(np.float32), start


def fit_run(field, points, target_color, start):
    """200 Adam steps (lr 0.01) on mean|D| + mean|C - C_target| through field(points, centers, colors,
    radius) -> (D, C); the tensors arrive in the dtype and on the device of `points`. Returns (initial
    loss, final loss), the final one evaluated after the last step."""
    par = {k: torch.from_numpy(v.copy()).to(points).requires_grad_(True) for k, v in start.items()}
    opt = torch.optim.Adam(list(par.values()), lr=FIT_LR)

    def loss_of():
        d, c = field(points, par["centers"], par["colors"], par["radius"])
        return d.abs().mean() + (c - target_color).abs().mean()

    first = None
    for _ in range(FIT_STEPS):
        opt.zero_grad()
        loss = loss_of()
        first = float(loss.detach()) if first is None else first
        loss.backward()
        opt.step()
    with torch.no_grad():
        last = float(loss_of())
    return first, last
