"""Shared helpers of the ray / camera-pose gradient tests (test_raygrad_reference.py on the CPU,
test_gpu_raygrad.py on the GPU): a differentiable torch restatement of create_camera_rays
(camera.rs:41-79; cross, normalize and tan are formulas), torch autograd of
oracle/autodiff_ref.render_diff with the rays or the camera requiring grad, and the closed form
of the gradient the kernels implement (names as in oracle/rm_oracle_impl.h: backward_ray)."""
import math

import numpy as np
import torch

from oracle import autodiff_ref as ar


def normalize(v):
    """math::normalize (camera.rs:7-14): zeros for a zero vector, and then a zero Jacobian."""
    ln = v.pow(2).sum().sqrt()
    if float(ln.detach()) == 0.0:
        return v * 0.0
    return v / ln


def camera_rays_t(width, height, eye, target, fov_deg):
    """create_camera_rays on torch tensors (eye [3], target [3], fov_deg []), differentiable."""
    dt = eye.dtype
    fwd = normalize(target - eye)
    up_w = torch.tensor([0.0, 1.0, 0.0], dtype=dt)
    right = normalize(torch.linalg.cross(fwd, up_w))
    up = torch.linalg.cross(right, fwd)
    aspect = width / height
    hh = torch.tan(fov_deg * (math.pi / 180.0) / 2.0)
    hw = aspect * hh
    x = torch.arange(width, dtype=dt)
    y = torch.arange(height, dtype=dt)
    u = (x / width) * 2.0 - 1.0
    v = -((y / height) * 2.0 - 1.0)
    rs = (u * hw)[None, :, None]
    us = (v * hh)[:, None, None]
    raw = right[None, None, :] * rs + up[None, None, :] * us + fwd[None, None, :]
    d = (raw / raw.pow(2).sum(dim=2, keepdim=True).sqrt()).reshape(-1, 3)
    o = eye[None, :].expand(d.shape[0], 3)
    return o, d


def scene_t(sc, dtype=torch.float64):
    """The scene dict (numpy) as torch tensors in the shapes autodiff_ref.render_diff takes."""
    return {"centers": torch.tensor(np.asarray(sc["centers"], np.float64).reshape(-1, 3), dtype=dtype),
            "colors": torch.tensor(np.asarray(sc["colors"], np.float64).reshape(-1, 3), dtype=dtype),
            "radius": torch.tensor(np.asarray(sc["radius"], np.float64).reshape(-1, 1), dtype=dtype),
            "light_dir": torch.tensor(np.asarray(sc["light_dir"], np.float64).reshape(3), dtype=dtype),
            "ambient": torch.tensor(np.asarray(sc["ambient"], np.float64).reshape(1), dtype=dtype)}


DEFAULTS = {"normal_eps": ar.EPS_F32, "color_sharpness": 10.0, "mask_sharpness": 15.0}


def _render(o, d, s, k, steps, **consts):
    """consts: normal_eps, color_sharpness, mask_sharpness (the reference's values by default)."""
    return ar.render_diff(o, d, s["centers"], s["colors"], s["radius"], s["light_dir"], s["ambient"], k, steps,
                          **consts)


def ray_grads(o, d, sc, k, steps, gout, dtype=torch.float64, with_centers=False, **consts):
    """Autograd of sum(render_diff * gout) w.r.t. ray_org and ray_dir ([N,3] numpy each), in the
    reference's op order at `dtype`; with_centers adds dL/dcenters."""
    s = scene_t(sc, dtype)
    ot = torch.tensor(np.asarray(o, np.float64), dtype=dtype).requires_grad_()
    dd = torch.tensor(np.asarray(d, np.float64), dtype=dtype).requires_grad_()
    if with_centers:
        s["centers"].requires_grad_()
    out = _render(ot, dd, s, k, steps, **consts)
    (out * torch.tensor(np.asarray(gout, np.float64), dtype=dtype)).sum().backward()
    res = (ot.grad.double().numpy(), dd.grad.double().numpy())
    return res + (s["centers"].grad.double().numpy(),) if with_centers else res


def camera_grads(cam, width, height, sc, k, steps, gout, dtype=torch.float64, **consts):
    """Autograd of sum(render_diff(create_camera_rays(cam)) * gout) w.r.t. eye, target, fov_deg."""
    s = scene_t(sc, dtype)
    eye = torch.tensor(np.asarray(cam[0], np.float32).astype(np.float64), dtype=dtype).requires_grad_()
    tgt = torch.tensor(np.asarray(cam[1], np.float32).astype(np.float64), dtype=dtype).requires_grad_()
    fov = torch.tensor(float(np.float32(cam[2])), dtype=dtype).requires_grad_()
    o, d = camera_rays_t(width, height, eye, tgt, fov)
    out = _render(o, d, s, k, steps, **consts)
    (out * torch.tensor(np.asarray(gout, np.float64), dtype=dtype)).sum().backward()
    return eye.grad.double().numpy(), tgt.grad.double().numpy(), float(fov.grad)


def closed_form_ray_grads(o, d, sc, k, steps, gout, **consts):
    """The closed form the kernels implement, in fp64 without autograd: sweep 1 at p_f gives g_p,
    sweep 2 at p_a gives g_pa = (g_p . d) grad D(p_a); g_org = g_p + g_pa, g_dir = t_f g_p + t g_pa."""
    cs = {key: ar._f32(consts.get(key, v)) for key, v in DEFAULTS.items()}
    eps, csharp, msharp = cs["normal_eps"], cs["color_sharpness"], cs["mask_sharpness"]
    with torch.no_grad():
        s = scene_t(sc)
        c, col, r, ld, amb = s["centers"], s["colors"], s["radius"], s["light_dir"], s["ambient"]
        o = torch.tensor(np.asarray(o, np.float64))
        d = torch.tensor(np.asarray(d, np.float64))
        g = torch.tensor(np.asarray(gout, np.float64))
        t = torch.zeros((o.shape[0], 1), dtype=torch.float64)
        for _ in range(steps):
            t = t + ar.scene_sdf_value(o + d * t, c, r, k)

        def dists(p):  # q [N,M], rho [N,M], delta [N,M]
            q = p.pow(2).sum(1, keepdim=True) + c.pow(2).sum(1, keepdim=True).t() - (p @ c.t()) * 2.0
            rho = q.clamp_min(1e-6).sqrt()
            return q, rho, rho - r.t()

        pa = o + d * t
        qa, rhoa, da = dists(pa)
        alpha = torch.softmax(-k * da, dim=1)
        tf = t + ar.scene_sdf_value(pa, c, r, k)
        pf = o + d * tf
        q, rho, dl = dists(pf)
        n = ar.calc_normal_scene(pf, c, r, k, eps=eps)
        sdot = n @ (ld / ld.pow(2).sum().sqrt())
        L = (amb + sdot.clamp_min(0.0) * (1.0 - amb)).unsqueeze(1)
        w = torch.softmax(-csharp * dl, dim=1)
        beta = torch.softmax(-k * dl, dim=1)
        mix = w @ col
        mu = torch.sigmoid(-msharp * ar.scene_sdf_value(pf, c, r, k))
        gm = g * L * mu
        gmu = (g * mix).sum(1, keepdim=True) * L
        cmu = gmu * mu * (1.0 - mu) * (-msharp)
        mg = (mix * gm).sum(1, keepdim=True)
        gdl = -csharp * w * (gm @ col.t() - mg) + cmu * beta
        gate = (q >= 1e-6).double()
        unit = (pf.unsqueeze(1) - c.unsqueeze(0)) / rho.unsqueeze(2)
        gp = ((gdl * gate).unsqueeze(2) * unit).sum(1)
        gt = (gp * d).sum(1, keepdim=True)
        gate_a = (qa >= 1e-6).double()
        unit_a = (pa.unsqueeze(1) - c.unsqueeze(0)) / rhoa.unsqueeze(2)
        gpa = gt * ((alpha * gate_a).unsqueeze(2) * unit_a).sum(1)
        return (gp + gpa).numpy(), (tf * gp + t * gpa).numpy()


# ---- the per-ray measure ---------------------------------------------------------------------------
# max |a - b| / max |b| over the whole [N,3] array lets a ray whose gradient is small next to the
# largest be wrong by 100 %. Per ray: |a_i - b_i| / |b_i| (vector norms) for every ray whose reference
# norm is at least floor x the largest, in the tiers of conftest.REL_ELEM["bwd"] (5e-2 from 1e-2 of the
# largest, 1e-1 from 1e-3). torch fp32 in the reference's op order has its own figure (a grazing ray's
# gradient is ill-conditioned), so the bound is max(tier, PER_RAY_MARGIN x torch fp32's figure at the
# case), and at most PER_RAY_CAP x the tier -- envelope_ref's rule, MARGIN and CAP_FACTOR.
PER_RAY_MARGIN = 4.0
PER_RAY_CAP = 10.0


def per_ray_errors(a, b, tiers):
    """[(floor, worst |a_i - b_i| / |b_i| over the rays with |b_i| >= floor max|b|)] for [N,3] arrays."""
    a, b = np.asarray(a, np.float64).reshape(-1, 3), np.asarray(b, np.float64).reshape(-1, 3)
    nb = np.sqrt((b * b).sum(1))
    err = np.sqrt(((a - b) ** 2).sum(1))
    out = []
    for floor, _ in tiers:
        big = (nb >= floor * nb.max()) & (nb > 0)
        out.append((floor, float((err[big] / nb[big]).max()) if big.any() else 0.0))
    return out


def per_ray_bounds(f32_errors, tiers):
    """[(floor, bound, within the cap)] from torch fp32's per_ray_errors at the same case."""
    return [(floor, max(rel, PER_RAY_MARGIN * e), PER_RAY_MARGIN * e <= PER_RAY_CAP * rel)
            for (floor, e), (_, rel) in zip(f32_errors, tiers)]


def per_ray_check(got, f32, ref, tiers):
    """[(floor, the figure of `got`, its bound, torch fp32's figure, the bound is within the cap)] per
    tier, for a device result and torch fp32's against the fp64 reference (all [N,3])."""
    fe = per_ray_errors(f32, ref, tiers)
    return [(floor, e, bound, f, ok) for (floor, e), (_, bound, ok), (_, f) in
            zip(per_ray_errors(got, ref, tiers), per_ray_bounds(fe, tiers), fe)]


def camera_tail(cam, width, height, g_org, g_dir):
    """The camera chain of the ray gradients in fp64 (numpy): the 13 sums over the view's rays and
    the 13 -> 7 tail. Returns (g_eye [3], g_target [3], g_fov)."""
    eye = np.asarray(cam[0], np.float32).astype(np.float64)
    tgt = np.asarray(cam[1], np.float32).astype(np.float64)
    fov = float(np.float32(cam[2]))

    def nrm(v):
        ln = np.sqrt((v * v).sum())
        return (v * 0.0, 0.0) if ln == 0.0 else (v / ln, ln)

    def nrm_bwd(x, ln, gx):
        return gx * 0.0 if ln == 0.0 else (gx - x * (x * gx).sum()) / ln

    up_w = np.array([0.0, 1.0, 0.0])
    fwd, flen = nrm(tgt - eye)
    right, rlen = nrm(np.cross(fwd, up_w))
    up = np.cross(right, fwd)
    hh = math.tan(fov * math.pi / 360.0)
    aspect = width / height
    u = (np.arange(width) / width) * 2.0 - 1.0
    v = -((np.arange(height) / height) * 2.0 - 1.0)
    uu, vv = np.meshgrid(u, v)  # [H,W], rows y then x
    rs = (uu * aspect * hh).reshape(-1, 1)
    us = (vv * hh).reshape(-1, 1)
    raw = right[None] * rs + up[None] * us + fwd[None]
    ln = np.sqrt((raw * raw).sum(1, keepdims=True))
    dd = raw / ln
    g_dir = np.asarray(g_dir, np.float64)
    g_raw = (g_dir - dd * (dd * g_dir).sum(1, keepdims=True)) / ln
    G_o = np.asarray(g_org, np.float64).sum(0)
    G_f = g_raw.sum(0)
    G_r = (rs * g_raw).sum(0)
    G_u = (us * g_raw).sum(0)
    g_hh = (((uu.reshape(-1, 1) * aspect) * right[None] + vv.reshape(-1, 1) * up[None]) * g_raw).sum()
    g_right = G_r + np.cross(fwd, G_u)          # up = right x fwd
    g_fwd = G_f + np.cross(G_u, right)
    g_rr = nrm_bwd(right, rlen, g_right)        # right = normalize(fwd x up_w)
    g_fwd = g_fwd + np.cross(up_w, g_rr)
    g_fr = nrm_bwd(fwd, flen, g_fwd)            # fwd = normalize(target - eye)
    return G_o - g_fr, g_fr, g_hh * (1.0 + hh * hh) * math.pi / 360.0
