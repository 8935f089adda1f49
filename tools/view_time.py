#!/usr/bin/env python3
"""Kernel time of the viewer's frame render (rm_view) for one 1920x1080 frame from the viewer's
start pose (pos (0, 0, -2.5), yaw pi/2, pitch 0), via the C ABI's kernel timing (rm_timing_collect)
after warm-up, next to the forward rm_render_diff at S = 40, k = 32 on the same rays and spheres as
a yardstick (it does different work -- a fixed-step march with the mask and the reconnect sweep --
so it is context, not a threshold). One JSON line per step.

  golden   tests/golden/scene.json (6 spheres)
  synth    model.synthetic_scene(256, 0)
  grown    profiles/r05a_grown_scene_4096.json (the grown 4096-sphere model)

    python3 tools/view_time.py               # every step, each in a child process under `timeout`
    python3 tools/view_time.py --step grown:view

Scenes from a scene.json are drawn as the viewer draws them: the stored radii, no +0.01. The mean
iterations per ray is the trace's soft-min evaluation count (RM_VIEW_COUNT_ITERATIONS: the
specified trace, without the exact skips), per wave the largest count of each 8x8 pixel tile (what a
wave runs with the skips off); `exit_off` times the kernel with RM_MARCH_NO_EARLY_EXIT.
"""
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080
SCENES = ("golden", "synth", "grown")
STEPS = [f"{s}:{k}" for s in SCENES for k in ("view", "exit_off", "forward40")]
STEP_LIMIT = 240  # seconds per step


def load_scene(name):
    import numpy as np
    from burn_raymarching_amd import model
    if name == "synth":
        return model.synthetic_scene(256, 0)
    path = os.path.join(ROOT, "tests", "golden", "scene.json") if name == "golden" else \
        os.path.join(ROOT, "profiles", "r05a_grown_scene_4096.json")
    sc = json.load(open(path))
    return {"centers": np.array(sc["centers"], np.float32).reshape(-1, 3),
            "colors": np.array(sc["colors"], np.float32).reshape(-1, 3),
            "radius": np.array(sc["radii"], np.float32).reshape(-1),
            "light_dir": np.array(sc["light_dir"], np.float32).reshape(3),
            "ambient": np.array(sc["ambient_intensity"], np.float32).reshape(-1)[:1]}


def viewer_rays(cam, focal=1.5):
    """The viewer's rays of a W x H frame (shader.wgsl:89-98) as fp32 arrays, for the yardstick."""
    import numpy as np
    pos, fwd, up = (np.asarray(x, np.float64) for x in cam)
    ww = fwd / np.linalg.norm(fwd)
    uu = np.cross(ww, up)
    uu /= np.linalg.norm(uu)
    vv = np.cross(uu, ww)
    vv /= np.linalg.norm(vv)
    ux = ((2.0 * (np.arange(W) + 0.5) / W - 1.0) * (W / H))[None, :, None]
    uy = (1.0 - 2.0 * (np.arange(H) + 0.5) / H)[:, None, None]
    rd = ux * uu + uy * vv + focal * ww
    rd /= np.linalg.norm(rd, axis=-1, keepdims=True)
    rd = rd.reshape(-1, 3).astype(np.float32)
    return np.broadcast_to(pos.astype(np.float32), rd.shape).copy(), rd


def run_step(name):
    import torch
    from burn_raymarching_amd import model, native, render
    scene_name, kind = name.split(":")
    raw = load_scene(scene_name)
    sc = model.scene_tensors(raw)
    cam = render.view_camera(*render.VIEW_START)
    ctx = render.context()
    extra = {}
    if kind == "forward40":
        o, d = viewer_rays(cam)
        o, d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()

        def fn():
            render.render_diff_forward(o, d, sc, 32.0, 40)
    else:
        params = native.view_params(flags=native.RM_MARCH_NO_EARLY_EXIT if kind == "exit_off" else 0)
        _, depth = render.view([cam], W, H, sc, depth=True, params=params)
        _, iters = render.view([cam], W, H, sc, depth=True,
                               params=native.view_params(flags=native.RM_VIEW_COUNT_ITERATIONS))
        extra = {"hit_fraction": round(float(torch.isfinite(depth).float().mean()), 5),
                 "mean_iterations_per_ray": round(float(iters.mean()), 3),
                 # what a wave runs: the slowest ray of each 8x8 pixel tile (W and H are multiples of 8)
                 "mean_iterations_per_wave": round(float(iters[0].reshape(H // 8, 8, W // 8, 8).amax((1, 3)).mean()), 3),
                 "max_iterations": int(iters.max())}

        def fn():
            render.view([cam], W, H, sc, params=params)
    reps = 10
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ctx.collect_timing(reset=True)
    ctx.timing(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    ctx.timing(False)
    ms, n = ctx.collect_timing(reset=True)
    print(json.dumps(dict({"step": name, "width": W, "height": H, "spheres": int(raw["centers"].shape[0]),
                           "kernel_ms_per_frame": round(ms / reps, 4), "launches_per_frame": n / reps,
                           "mrays_per_s": round(W * H / (ms / reps) / 1e3, 1)}, **extra)), flush=True)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        run_step(sys.argv[2])
        return 0
    for name in STEPS:  # a fresh process per step, each under its own limit; stop at the first failure
        rc = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__),
                             "--step", name]).returncode
        if rc != 0:
            print(json.dumps({"step": name, "failed": rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
