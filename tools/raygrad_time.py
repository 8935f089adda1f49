#!/usr/bin/env python3
"""Kernel time of the camera-pose gradient (rm_render_diff_backward_cameras, saved t) next to the
parameter backward (rm_render_diff_backward_camera, saved t) at the same shapes, via the C ABI's
hipEvent kernel timing (rm_timing_collect). One JSON line per step.

  one_view   1 view of 512x512, 256 spheres, 32 steps
  ten_views  the ten cameras.json poses at 256x256, 64 spheres, 32 steps

    python3 tools/raygrad_time.py            # every step, each in a child process under `timeout`
    python3 tools/raygrad_time.py --step one_view:cameras

The timed figure is the per-ray kernel alone (the record kernel and the per-view finish / the
gradient reduction run outside the event pair), summed over the launches of one call.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"one_view": (512, 256, 32, 1), "ten_views": (256, 64, 32, 10)}
STEPS = [f"{s}:{k}" for s in SHAPES for k in ("cameras", "params")]
STEP_LIMIT = 180  # seconds per step


def run_step(name):
    import torch
    from burn_raymarching_amd import model, render
    shape, kind = name.split(":")
    W, M, S, V = SHAPES[shape]
    cams = json.load(open(os.path.join(ROOT, "tests", "golden", "cameras.json")))
    cams = [(c["origin"], c["target"], c["fov"]) for c in cams][:V]
    sc = model.scene_tensors(model.synthetic_scene(M, 0))
    ctx = render.context()
    _, t = render.render_diff_camera(cams, W, W, sc, 32.0, S, return_t=True)
    g = torch.randn((V * W * W, 3), device="cuda", generator=torch.Generator("cuda").manual_seed(0))
    if kind == "cameras":
        def fn():
            render.render_diff_backward_cameras(cams, W, W, sc, 32.0, g, S, t_march=t)
    else:
        def fn():
            render.render_diff_backward_camera(cams, W, W, sc, 32.0, g, S, t_march=t)
    reps = 20
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
    print(json.dumps({"step": name, "width": W, "spheres": M, "march_steps": S, "views": V,
                      "kernel_ms_per_call": round(ms / reps, 4), "launches_per_call": n / reps,
                      "mrays_per_s": round(V * W * W / (ms / reps) / 1e3, 1)}), flush=True)


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
