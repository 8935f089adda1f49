#!/usr/bin/env python3
"""Kernel time of the distance-field query on a 256^3 lattice over [-1, 1]^3 (rm_sdf_grid), via the
C ABI's kernel timing (rm_timing_collect) after warm-up, as sphere evaluations per second (lattice
points x spheres / kernel time), and the grid / copy / extraction / refinement split of
`rm_train mesh --res 256` on the same scenes. One JSON line per step.

  golden   tests/golden/scene.json (6 spheres)
  synth    model.synthetic_scene(256, 0)
  grown    profiles/r05a_grown_scene_4096.json (the grown 4096-sphere model)

    python3 tools/sdf_time.py               # every step, each in a child process under `timeout`
    python3 tools/sdf_time.py --step grown:grid

Steps per scene: `grid` (the distance alone: the mesh extraction's launch), `grid_color` (distance and
blended colour: the full sweep), `query` (distance, gradient and colour at the lattice's points
from a point array), `mesh` (the CLI; scene.json radii + 0.01, the box of the scene, not [-1, 1]^3).
For context: the viewer's kernel with its exits off ran 1.08e11 sphere evaluations
in 40.5 ms at 4096 spheres.
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 256
SCENES = ("golden", "synth", "grown")
STEPS = [f"{s}:{k}" for s in SCENES for k in ("grid", "grid_color", "query", "mesh")]
STEP_LIMIT = 240  # seconds per step


def scene_path(name):
    return os.path.join(ROOT, "tests", "golden", "scene.json") if name == "golden" else \
        os.path.join(ROOT, "profiles", "r05a_grown_scene_4096.json")


def load_scene(name):
    import numpy as np
    from burn_raymarching_amd import model
    if name == "synth":
        return model.synthetic_scene(256, 0)
    sc = json.load(open(scene_path(name)))
    return {"centers": np.array(sc["centers"], np.float32).reshape(-1, 3),
            "colors": np.array(sc["colors"], np.float32).reshape(-1, 3),
            "radius": np.array(sc["radii"], np.float32).reshape(-1),
            "light_dir": np.array(sc["light_dir"], np.float32).reshape(3),
            "ambient": np.array(sc["ambient_intensity"], np.float32).reshape(-1)[:1]}


def run_mesh(scene_name):
    from burn_raymarching_amd import _build, host
    raw = load_scene(scene_name)
    with tempfile.TemporaryDirectory() as td:
        path = scene_path(scene_name)
        if scene_name == "synth":  # the CLI reads a scene.json
            path = os.path.join(td, "scene.json")
            host.scene_save(path, raw["centers"], raw["colors"], raw["radius"], raw["light_dir"], raw["ambient"])
        out = subprocess.run([_build.EXE, "mesh", "--scene", path, "--out", os.path.join(td, "mesh.ply"), "--res", str(N)],
                             capture_output=True, text=True, check=True).stdout
        line = json.loads(out.strip().splitlines()[-1])
        line["ply_bytes"] = os.path.getsize(os.path.join(td, "mesh.ply"))
    print(json.dumps(dict({"step": f"{scene_name}:mesh", "res": N, "spheres": int(raw["centers"].shape[0])}, **line)),
          flush=True)


def run_step(name):
    scene_name, kind = name.split(":")
    if kind == "mesh":
        return run_mesh(scene_name)
    import torch
    from burn_raymarching_amd import model, render
    raw = load_scene(scene_name)
    sc = model.scene_tensors(raw)
    ctx = render.context()
    origin, spacing, shape = (-1.0, -1.0, -1.0), 2.0 / (N - 1), (N, N, N)
    if kind == "query":
        ax = torch.arange(N, device="cuda", dtype=torch.float32) * spacing - 1.0
        z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
        pts = torch.stack([x, y, z], -1).reshape(-1, 3).contiguous()

        def fn():
            render.sdf_query(pts, sc, 32.0)
    else:
        def fn():
            render.sdf_grid(origin, spacing, shape, sc, 32.0, color=kind == "grid_color")
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
    m = int(raw["centers"].shape[0])
    print(json.dumps({"step": name, "points": N ** 3, "spheres": m, "kernel_ms": round(ms / reps, 4),
                      "launches": n / reps, "sphere_evals_per_s": float(f"{N ** 3 * m / (ms / reps) * 1e3:.4g}"),
                      "padded_sphere_evals_per_s": float(f"{N ** 3 * ((m + 31) // 32 * 32) / (ms / reps) * 1e3:.4g}"),
                      "mpoints_per_s": round(N ** 3 / (ms / reps) / 1e3, 1)}), flush=True)


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
