#!/usr/bin/env python3
"""Time of the view-dependent colour calls (rm_render_diff_sh_camera, rm_render_diff_sh_backward_camera) at
degree 1 and 2 against the calls they extend (rm_render_diff_camera + rm_render_diff_backward_camera with the
saved march t) and against a dense torch graph of the same post-march loss on the same GPU. One JSON line per
step: device events around each call after warm-up, median and min / max of the repetitions, and the summed
time of the call's per-ray kernel launches (rm_timing_collect: the march and the shade kernel of a forward,
rm_sh_grad_kernel of a backward; the record, pack and reduction launches are the rest of the call).

  v10_m256    10 ring views of 512 x 512, model.synthetic_scene(256, 0), 32 march steps
  v1_m4096    one view of 512 x 512, profiles/r05a_grown_scene_4096.json, 128 march steps

Per shape:
  base_forward / base_backward      rm_render_diff_camera (out and t), rm_render_diff_backward_camera (saved t)
  sh{1,2}_forward / sh{1,2}_backward  the SH calls, coefficients from N(0, 0.5); the backward with every output
  torch_sh2                         the post-march graph of degree 2 from the saved t as dense torch (rays x
                                    spheres intermediates, the normal detached), forward + backward, in chunks
                                    of rays that keep a chunk's intermediates within ~1 GB

    python3 tools/sh_time.py                    # both shapes, each in a child process under `timeout`
    python3 tools/sh_time.py --shape v10_m256
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, CS, MS, EPS = 32.0, 10.0, 15.0, 1e-4
SHAPES = {"v10_m256": (10, 256, 32), "v1_m4096": (1, 4096, 128)}
WIDTH = 512
SHAPE_LIMIT = 420  # seconds per shape
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)


def load_scene(m):
    import numpy as np
    from burn_raymarching_amd import model
    if m != 4096:
        return model.synthetic_scene(m, 0)
    sc = json.load(open(os.path.join(ROOT, "profiles", "r05a_grown_scene_4096.json")))
    return {"centers": np.array(sc["centers"], np.float32).reshape(-1, 3),
            "colors": np.array(sc["colors"], np.float32).reshape(-1, 3),
            "radius": np.array(sc["radii"], np.float32).reshape(-1),
            "light_dir": np.array(sc.get("light_dir", [-0.5, 0.5, -1.0]), np.float32),
            "ambient": np.array([sc.get("ambient_intensity", 0.2)], np.float32).reshape(1)}


def torch_sh_loss(o, d, t, c, col, sh, r, ld, amb, g):
    """sum(out * g) of the post-march graph (renderer_diff.rs:28-90 with a_j(u)) as a user would write it in
    torch: dense rays x spheres tensors. The normal is the detached analytic gradient of the soft-min, the
    eps -> 0 limit of calc_normal's differences that the kernels use too, not calc_normal itself: the graph is
    there for its cost, which the rays x spheres tensors set, and is held to no parity bound."""
    import torch

    def dists(p):
        q = p.pow(2).sum(1, keepdim=True) + c.pow(2).sum(1, keepdim=True).t() - (p @ c.t()) * 2.0
        return q.clamp_min(1e-6).sqrt() - r.reshape(1, -1)

    pa = o + d * t
    tf = t - torch.logsumexp(dists(pa) * (-K), dim=1, keepdim=True) / K
    p = o + d * tf
    dl = dists(p)
    with torch.no_grad():
        beta = torch.softmax(dl * (-K), dim=1)
        e = p.unsqueeze(1) - c.unsqueeze(0)
        grad = (beta.unsqueeze(2) * e / (dl + r.reshape(1, -1)).unsqueeze(2)).sum(1)
        nrm = grad / (grad.pow(2).sum(1, keepdim=True) + 1e-6 / (2 * EPS) ** 2).sqrt()
        u = d / d.norm(dim=1, keepdim=True).clamp_min(1e-30)  # u = d / |d| as the kernels form it, Y = 0 at d = 0
        x, y, z = u[:, 0], u[:, 1], u[:, 2]
        Y = torch.stack([-C1 * y, C1 * z, -C1 * x, C2[0] * x * y, C2[1] * y * z, C2[2] * (2 * z * z - x * x - y * y),
                         C2[3] * x * z, C2[4] * (x * x - y * y)], dim=1)
    L = amb + (nrm @ (ld / ld.norm())).clamp_min(0.0) * (1.0 - amb)
    a = (col.unsqueeze(0) + torch.einsum("nb,mbc->nmc", Y, sh)).clamp_min(0.0)
    mix = (a * torch.softmax(dl * (-CS), dim=1).unsqueeze(2)).sum(1)
    mu = torch.sigmoid(torch.logsumexp(dl * (-K), dim=1) / K * MS)
    return (mix * (L * mu).unsqueeze(1) * g).sum()


def timed(name, fn, ctx, extra):
    import torch
    reps = 10
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ctx.collect_timing(reset=True)
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    kernel_ms, launches = ctx.collect_timing(reset=True)
    print(json.dumps(dict(extra, step=name, reps=reps, median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4),
                          max_ms=round(max(ms), 4), ray_kernel_ms=round(kernel_ms / reps, 4),
                          ray_kernel_launches=launches // reps)), flush=True)


def run_shape(shape):
    import numpy as np
    import torch
    from burn_raymarching_amd import model, render
    views, m, steps = SHAPES[shape]
    raw = load_scene(m)
    scene = render.Scene(*[torch.from_numpy(np.asarray(raw[k], np.float32)).cuda()
                           for k in ("centers", "colors", "radius", "light_dir", "ambient")])
    cams = model.ring_cameras(views)
    n = views * WIDTH * WIDTH
    gen = torch.Generator(device="cuda").manual_seed(22)
    g = torch.randn((n, 3), device="cuda", generator=gen)
    ctx = render.context()
    ctx.timing(True)
    extra = {"shape": shape, "views": views, "spheres": m, "march_steps": steps, "rays": n}
    _, t = render.render_diff_camera(cams, WIDTH, WIDTH, scene, K, steps, return_t=True)
    timed("base_forward", lambda: render.render_diff_camera(cams, WIDTH, WIDTH, scene, K, steps, return_t=True), ctx, extra)
    timed("base_backward", lambda: render.render_diff_backward_camera(cams, WIDTH, WIDTH, scene, K, g, steps, t_march=t), ctx,
          extra)
    sh2 = None
    for deg, nb in ((1, 3), (2, 8)):
        sh = (torch.randn((m, nb, 3), device="cuda", generator=gen) * 0.5).contiguous()
        sh2 = sh
        timed(f"sh{deg}_forward",
              lambda: render.render_diff_sh_camera(cams, WIDTH, WIDTH, scene, sh, K, steps, return_t=True), ctx, extra)
        timed(f"sh{deg}_backward",
              lambda: render.render_diff_sh_backward_camera(cams, WIDTH, WIDTH, scene, sh, K, g, steps, t_march=t), ctx, extra)
    # the dense torch graph from the same saved t, in chunks of rays
    rays = [render.create_camera_rays(WIDTH, WIDTH, *cam) for cam in cams]
    o, d = torch.cat([r[0] for r in rays]), torch.cat([r[1] for r in rays])
    chunk = max(1024, min(n, (1 << 30) // (4 * 24 * m)))  # about 24 rays x spheres float32 intermediates alive
    leaves = [x.clone().requires_grad_(True) for x in (scene.centers, scene.colors, sh2, scene.radius, scene.light_dir,
                                                       scene.ambient)]

    def torch_fn():
        for x in leaves:
            x.grad = None
        for i in range(0, n, chunk):
            s = slice(i, i + chunk)
            torch_sh_loss(o[s], d[s], t[s].reshape(-1, 1), *leaves, g[s]).backward()

    timed("torch_sh2", torch_fn, ctx, dict(extra, chunk_rays=chunk))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        run_shape(sys.argv[2])
        return 0
    for name in SHAPES:  # a fresh process per shape, each under its own limit; stop at the first failure
        rc = subprocess.run(["timeout", "-k", "10", str(SHAPE_LIMIT), sys.executable, os.path.abspath(__file__), "--shape",
                             name]).returncode
        if rc != 0:
            print(json.dumps({"shape": name, "failed": rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
