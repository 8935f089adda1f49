#!/usr/bin/env python3
"""Time of the distance field's backward (rm_sdf_query_backward) for N = 2^20 uniform points in [-1, 1]^3
against what a user had before it: a plain-torch N x M autograd implementation of the same loss on the
same GPU. One JSON line per step; device events around each call after warm-up, median and min / max of
the repetitions, sphere evaluations per second = points x spheres / median.

  m9      model.synthetic_scene(9, 0)
  m256    model.synthetic_scene(256, 0)
  m4096   profiles/r05a_grown_scene_4096.json (the grown 4096-sphere model)

Per scene:
  forward          rm_sdf_query, dist and color (what sdf_field's forward runs)
  backward         rm_sdf_query_backward, both seeds, the scene gradient and grad_points
  backward_scene   the same without grad_points (no point-gradient sweep)
  backward_points  grad_points alone (no sphere-gradient sweep, no reduction)
  torch            sum(gD D + gC . C) of a dense torch graph, forward + backward, in chunks of points
                   that keep a chunk's N x M intermediates within ~1 GB; the scene's gradients accumulate
                   over the chunks

    python3 tools/sdf_grad_time.py                 # every scene, each in a child process under `timeout`
    python3 tools/sdf_grad_time.py --scene m256
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 1 << 20
K, CS = 32.0, 10.0
SCENES = ("m9", "m256", "m4096")
KINDS = ("forward", "backward", "backward_scene", "backward_points", "torch")
SCENE_LIMIT = 300  # seconds per scene


def load_scene(name):
    import numpy as np
    from burn_raymarching_amd import model
    if name != "m4096":
        return model.synthetic_scene(int(name[1:]), 0)
    sc = json.load(open(os.path.join(ROOT, "profiles", "r05a_grown_scene_4096.json")))
    return {"centers": np.array(sc["centers"], np.float32).reshape(-1, 3),
            "colors": np.array(sc["colors"], np.float32).reshape(-1, 3),
            "radius": np.array(sc["radii"], np.float32).reshape(-1)}


def torch_field_loss(p, c, col, r, gD, gC):
    """The restatement's operations (scene.rs:60-79, sdf.rs:30-44, renderer_diff.rs:64-80) as a user
    would write them in torch."""
    import torch
    q = p.pow(2).sum(1, keepdim=True) + c.pow(2).sum(1, keepdim=True).t() - (p @ c.t()) * 2.0
    d = q.clamp_min(1e-6).sqrt() - r.reshape(1, -1)
    dist = -torch.logsumexp(d * (-K), dim=1) / K
    w = torch.softmax(d * (-CS), dim=1)
    return (dist * gD).sum() + ((w @ col) * gC).sum()


def run_scene(scene_name):
    import torch
    from burn_raymarching_amd import render
    raw = load_scene(scene_name)
    c, col, r = (torch.from_numpy(raw[k]).cuda() for k in ("centers", "colors", "radius"))
    m = int(c.shape[0])
    gen = torch.Generator(device="cuda").manual_seed(22)
    pts = torch.rand((N, 3), device="cuda", generator=gen) * 2 - 1
    gD = torch.randn((N,), device="cuda", generator=gen)
    gC = torch.randn((N, 3), device="cuda", generator=gen)
    for kind in KINDS:
        run_kind(f"{scene_name}:{kind}", kind, m, pts, gD, gC, c, col, r)


def run_kind(name, kind, m, pts, gD, gC, c, col, r):
    import torch
    from burn_raymarching_amd import render
    if kind == "forward":
        light, amb = torch.tensor([0.0, -1.0, 0.0], device="cuda"), torch.tensor([0.3], device="cuda")
        scene = render.Scene(c, col, r, light, amb)

        def fn():
            render.sdf_query(pts, scene, K, color_sharpness=CS, grad=False)
    elif kind == "torch":
        chunk = max(1024, min(N, (1 << 30) // (4 * 8 * m)))  # about eight N x M float32 intermediates alive
        leaves = [t.clone().requires_grad_(True) for t in (c, col, r)]

        def fn():
            for t in leaves:
                t.grad = None
            for i in range(0, N, chunk):
                p = pts[i:i + chunk].clone().requires_grad_(True)
                torch_field_loss(p, *leaves, gD[i:i + chunk], gC[i:i + chunk]).backward()
    else:
        want = {"backward": ("centers", "colors", "radius", "points"), "backward_scene": ("centers", "colors", "radius"),
                "backward_points": ("points",)}[kind]

        def fn():
            render.sdf_query_backward(pts, c, col, r, K, color_sharpness=CS, grad_dist=gD, grad_color=gC, want=want)
    reps = 10
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    print(json.dumps({"step": name, "points": N, "spheres": m, "reps": reps, "median_ms": round(med, 4),
                      "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                      "sphere_evals_per_s": float(f"{N * m / med * 1e3:.4g}")}), flush=True)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--scene":
        run_scene(sys.argv[2])
        return 0
    for name in SCENES:  # a fresh process per scene, each under its own limit; stop at the first failure
        rc = subprocess.run(["timeout", "-k", "10", str(SCENE_LIMIT), sys.executable, os.path.abspath(__file__),
                             "--scene", name]).returncode
        if rc != 0:
            print(json.dumps({"scene": name, "failed": rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
