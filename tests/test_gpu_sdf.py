"""GPU tests of the distance-field query (rm_sdf_query, rm_sdf_grid, render.sdf_query / sdf_grid) and
the mesh export over it (host.mesh_extract, `rm_train mesh`), against the fp64 restatement
(tests/sdf_ref.py: oracle.autodiff_ref's scene_sdf_value, its autograd gradient, the burn_softmax
colour blend).

Parity bounds. Nothing is fixed by hand: for each scene and each of D, gradient and colour the bound
is 8 times the max error of the float32 run of the same restatement against fp64 (the project's
convention that the fp32 reference sits within 1/8 of a bound), computed here from the reference
alone. The error is taken over the scene's whole point pool (the special points, then uniform points
in [-1, 1]^3, 1000 in all) and the bound holds for every point count N = 1, 257, 1000, whose points
are the pool's first N: the fp32 error of a single point is a matter of luck (it can be exactly 0),
the pool's maximum is not. The points 1e3 units away form a group of their own with its own bound
(their rounding, 6e-5 per ulp of a coordinate, would otherwise set the bound of every other point).
Measured figures are printed and recorded (conftest.record_margin); profiles/r18_sdf_parity.txt
holds a run's figures."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import sdf_ref as S
from conftest import GOLDEN, final1_scene, gpu_available, record_margin

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

SCENE_JSON = os.path.join(GOLDEN, "scene.json")
K, CSHARP = 32.0, 10.0
NFAR = 6


def _synthetic(m, seed):
    from burn_raymarching_amd import model
    return model.synthetic_scene(m, seed)


def _one():
    g = final1_scene()
    return dict(centers=np.array([[0.1, -0.05, 0.0]], np.float32), colors=np.array([[0.8, 0.3, 0.2]], np.float32),
                radius=np.array([0.45], np.float32), light_dir=g["light_dir"], ambient=g["ambient"])


SCENES = {"golden": final1_scene, "one": _one, "m33": lambda: _synthetic(33, 3), "m300": lambda: _synthetic(300, 4)}
# 520 spheres: 272 pairs, two blocks of the record kernel -- the smallest scene whose record buffer has
# partial headers (test_two_record_blocks)
TWO_BLOCKS = {"m520": lambda: _synthetic(520, 5)}
_CACHE = {}


def pool(name):
    """(scene, points [1000,3], far mask, fp64 (D, g, col), fp32 (D, g, col)), computed once. Points:
    exactly the centre of sphere 0 (the clamp, the dropped gradient term), a point on its surface,
    NFAR points 1e3 units away, then uniform points in [-1, 1]^3."""
    if name not in _CACHE:
        sc = {**SCENES, **TWO_BLOCKS}[name]()
        rng = np.random.default_rng(18)
        c0, r0 = sc["centers"][0].astype(np.float32), np.float32(sc["radius"][0])
        u = rng.normal(size=(1 + NFAR, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        special = [c0, (c0 + r0 * u[0].astype(np.float32)).astype(np.float32)] + \
                  [(1e3 * u[1 + i]).astype(np.float32) for i in range(NFAR)]
        pts = np.concatenate([np.stack(special), rng.uniform(-1, 1, (1000 - len(special), 3))]).astype(np.float32)
        far = np.zeros(1000, bool)
        far[2:2 + NFAR] = True
        pts.setflags(write=False)
        _CACHE[name] = (sc, pts, far, S.field(pts, sc, K, CSHARP, torch.float64), S.field(pts, sc, K, CSHARP, torch.float32))
    return _CACHE[name]


def err(a, b, mask):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b)[mask].max()) if mask.any() else 0.0


@pytest.fixture(scope="module")
def rm():
    from burn_raymarching_amd import _build
    _build.build_host()
    from burn_raymarching_amd import host, native, render
    torch.cuda.init()
    return render, native, host


def scene_t(sc, half=False):
    from burn_raymarching_amd.render import Scene
    t = {k: torch.from_numpy(np.ascontiguousarray(sc[k], np.float32)).cuda() for k in sc}
    return Scene(t["centers"], t["colors"].half() if half else t["colors"], t["radius"], t["light_dir"], t["ambient"])


def bits(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.mark.parametrize("n", [1, 257, 1000])
@pytest.mark.parametrize("name", list(SCENES))
def test_query_parity_against_fp64(rm, name, n):
    render, _, _ = rm
    sc, pts, far, ref64, ref32 = pool(name)
    d, g, col = render.sdf_query(torch.from_numpy(pts[:n].copy()).cuda(), scene_t(sc), K, color_sharpness=CSHARP)
    got = (d.cpu().numpy(), g.cpu().numpy(), col.cpu().numpy())
    assert all(np.isfinite(x).all() for x in got)
    for group, mask in (("near", ~far), ("far", far)):
        sel = mask[:n]
        for what, a, r64, r32 in zip(("dist", "grad", "color"), got, ref64, ref32):
            bound = 8.0 * err(r32, r64, mask)  # the reference's own fp32 error over the whole pool
            e = err(a, r64[:n], sel)
            print(f"sdf parity {name} N={n} {group} {what}: gpu {e:.3e} fp32 {err(r32, r64, mask):.3e} bound {bound:.3e}")
            record_margin(f"sdf_{what}_{group}_{name}_{n}", e, bound)
            assert e <= bound, (name, n, group, what, e, bound)
    if n >= 2 + NFAR:
        # a point 1e3 units away: finite D next to its distance, a unit gradient, a colour in range
        f = np.where(far)[0]
        assert np.allclose(got[0][f], np.linalg.norm(pts[f].astype(np.float64), axis=1), atol=2.0)
        assert np.abs(np.linalg.norm(got[1][f].astype(np.float64), axis=1) - 1.0).max() <= 1e-5
        assert (got[2][f] >= 0).all() and (got[2][f] <= 1).all()
    if name == "one":
        assert not got[1][0].any()  # exactly at the only sphere's centre: its term is dropped


@pytest.mark.parametrize("name", ["golden", "m300"])
def test_grid_equals_query_bit_for_bit(rm, name):
    render, _, _ = rm
    sc = SCENES[name]()
    scene = scene_t(sc)
    origin, spacing, shape = (-0.8, -0.4, -0.2), 0.1, (17, 9, 5)
    gd, gc = render.sdf_grid(origin, spacing, shape, scene, K, color_sharpness=CSHARP, color=True)
    assert tuple(gd.shape) == (5, 9, 17) and tuple(gc.shape) == (5, 9, 17, 3)
    pts = S.lattice(origin, spacing, shape).reshape(-1, 3)
    qd, qc = render.sdf_query(torch.from_numpy(pts).cuda(), scene, K, color_sharpness=CSHARP, grad=False)
    assert bits(gd) == bits(qd) and bits(gc) == bits(qc)
    assert bits(render.sdf_grid(origin, spacing, shape, scene, K)) == bits(gd)  # the distance-only instance


def test_two_record_blocks(rm):
    """M = 520: sdf_query at the pool's first 257 points and sdf_grid on a 5x4x3 lattice, against the fp64
    restatement under the file's bound (8 times the restatement's own fp32 error over the scene's pool,
    near points). The lattice's points are not the pool's, so the restatement's fp32 run is first held to
    that bound at them."""
    render, _, _ = rm
    sc, pts, far, ref64, ref32 = pool("m520")
    near = ~far
    bounds = {what: 8.0 * err(r32, r64, near) for what, r32, r64 in zip(("dist", "grad", "color"), ref32, ref64)}
    n = 257
    d, g, col = render.sdf_query(torch.from_numpy(pts[:n].copy()).cuda(), scene_t(sc), K, color_sharpness=CSHARP)
    for what, a, r64 in zip(("dist", "grad", "color"), (d, g, col), ref64):
        e = err(a.cpu().numpy(), r64[:n], near[:n])
        print(f"sdf parity m520 N={n} near {what}: gpu {e:.3e} bound {bounds[what]:.3e}")
        record_margin(f"sdf_{what}_near_m520_{n}", e, bounds[what])
        assert np.isfinite(a.cpu().numpy()).all() and e <= bounds[what], (what, e, bounds[what])
    origin, spacing, shape = (-0.5, -0.4, -0.3), 0.25, (5, 4, 3)
    lat = S.lattice(origin, spacing, shape).reshape(-1, 3)
    l64, l32 = S.field(lat, sc, K, CSHARP, torch.float64), S.field(lat, sc, K, CSHARP, torch.float32)
    every = np.ones(len(lat), bool)
    gd, gc = render.sdf_grid(origin, spacing, shape, scene_t(sc), K, color_sharpness=CSHARP, color=True)
    assert tuple(gd.shape) == (3, 4, 5) and tuple(gc.shape) == (3, 4, 5, 3)
    for what, a, i in (("dist", gd.reshape(-1), 0), ("color", gc.reshape(-1, 3), 2)):
        e32, e = err(l32[i], l64[i], every), err(a.cpu().numpy(), l64[i], every)
        print(f"sdf grid m520 {what}: gpu {e:.3e} fp32 {e32:.3e} bound {bounds[what]:.3e}")
        record_margin(f"sdf_grid_{what}_m520", e, bounds[what])
        assert e32 <= bounds[what], ("the reference's fp32 run", what, e32, bounds[what])
        assert e <= bounds[what], (what, e, bounds[what])


def test_fp16_colours(rm):
    render, _, _ = rm
    sc, pts, _, _, _ = pool("m33")
    p = torch.from_numpy(pts[:257].copy()).cuda()
    rounded = dict(sc, colors=sc["colors"].astype(np.float16).astype(np.float32))
    h = render.sdf_query(p, scene_t(sc, half=True), K)
    f = render.sdf_query(p, scene_t(rounded), K)
    base = render.sdf_query(p, scene_t(sc), K)
    assert bits(h[2]) == bits(f[2]) and bits(h[2]) != bits(base[2])
    assert bits(h[0]) == bits(base[0]) and bits(h[1]) == bits(base[1])


def test_call_behaviour(rm):
    render, native, _ = rm
    import ctypes
    sc, pts, _, _, _ = pool("m300")
    scene = scene_t(sc)
    n = 257
    p = torch.from_numpy(pts[:n].copy()).cuda()
    ctx = render.context(p.device)
    cs, par = scene.c_struct(), native.sdf_params()

    def call(want, num=n, params=par):
        out = [torch.full(s, float("nan"), device=p.device) if w else None for w, s in zip(want, ((n,), (n, 3), (n, 3)))]
        rc = ctx._lib.rm_sdf_query(ctx.handle, ctypes.c_void_p(p.data_ptr()), num, ctypes.byref(cs), ctypes.byref(params),
                                   *[ctypes.c_void_p(o.data_ptr()) if o is not None else None for o in out])
        return rc, out

    rc, full = call((True, True, True))
    assert rc == native.RM_OK
    rc, again = call((True, True, True))
    assert rc == native.RM_OK and all(bits(a) == bits(b) for a, b in zip(full, again))
    for want in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        rc, part = call(want)
        assert rc == native.RM_OK
        assert all(o is None or bits(o) == bits(f) for o, f in zip(part, full)), want
    rc, untouched = call((True, True, True), num=0)
    assert rc == native.RM_OK and all(torch.isnan(o).all() for o in untouched)

    def refused(rc):
        msg = ctx._lib.rm_last_error(ctx.handle).decode()
        assert rc == 1 and msg, (rc, msg)  # RM_ERR_INVALID_ARG with a message
        return msg

    refused(call((False, False, False))[0])
    assert "smooth_k" in refused(call((True, False, False), params=native.sdf_params(smooth_k=0.0))[0])
    assert "smooth_k" in refused(call((True, False, False), params=native.sdf_params(smooth_k=-1.0))[0])
    assert "flags" in refused(call((True, False, False), params=native.sdf_params(flags=native.RM_MARCH_SPLIT))[0])
    assert "num_points" in refused(call((True, False, False), num=-1)[0])
    d = torch.empty(8, device=p.device)
    org = (ctypes.c_float * 3)(0.0, 0.0, 0.0)

    def grid(spacing, nx, ny, nz, dist=d):
        return ctx._lib.rm_sdf_grid(ctx.handle, ctypes.byref(org), spacing, nx, ny, nz, ctypes.byref(cs), ctypes.byref(par),
                                    ctypes.c_void_p(dist.data_ptr()) if dist is not None else None, None)

    assert grid(0.5, 2, 2, 2) == native.RM_OK
    assert "spacing" in refused(grid(0.0, 2, 2, 2))
    assert "spacing" in refused(grid(-0.5, 2, 2, 2))
    for ext in ((0, 2, 2), (2, -1, 2), (2, 2, 0)):
        assert "extents" in refused(grid(0.5, *ext))
    refused(grid(0.5, 2, 2, 2, dist=None))
    with pytest.raises(native.RaymarchError, match="RM_ERR_INVALID_ARG"):
        render.sdf_query(p, scene, 0.0)
    torch.cuda.synchronize()


_MESH = {}


def extracted(host, refine):
    if refine not in _MESH:
        _MESH[refine] = host.mesh_extract(SCENE_JSON, res=48, refine=refine)
    return _MESH[refine]


def test_mesh_extract(rm):
    _, _, host = rm
    sc = final1_scene()  # scene.json with the default radius_offset 0.01
    dmax = {}
    for refine in (0, 2):
        mesh = extracted(host, refine)
        rep = S.mesh_report(mesh.vertices, mesh.faces)
        print(f"mesh_extract refine={refine}:", rep, "timing ms", mesh.timing_ms)
        assert rep["open_edges"] == 0 and mesh.open_edges == 0 and rep["unpaired"] == 0 and rep["unused"] == 0, rep
        assert rep["components"] == 1 and rep["euler"] == 2 and rep["volume"] > 0, rep
        dmax[refine] = float(np.abs(S.distance(mesh.vertices, sc, K)).max())
        assert mesh.normals.shape == mesh.vertices.shape == mesh.colors.shape
        assert np.abs(np.linalg.norm(mesh.normals.astype(np.float64), axis=1) - 1.0).max() <= 1e-5
        assert (mesh.colors >= 0).all() and (mesh.colors <= 1).all()
    assert np.array_equal(extracted(host, 0).faces, extracted(host, 2).faces)
    # res = 48 cells along the longest extent of the box of c +- (r + 0.01 + margin 0.05)
    reach = sc["radius"] + np.float32(0.05)
    ext = (sc["centers"] + reach[:, None]).max(0) - (sc["centers"] - reach[:, None]).min(0)
    L = np.sqrt(3.0) * float(ext.max()) / 48.0
    print(f"mesh_extract max |D_fp64(v)|: refine 0 {dmax[0]:.3e} (bound L/2 {L / 2:.3e}), refine 2 {dmax[2]:.3e} "
          f"(bound {dmax[0] / 100:.3e})")
    record_margin("mesh_refine0_dmax", dmax[0], L / 2)
    record_margin("mesh_refine2_dmax", dmax[2], dmax[0] / 100)
    assert dmax[0] <= L / 2, (dmax[0], L / 2)
    assert dmax[2] <= dmax[0] / 100, (dmax[2], dmax[0])


def test_mesh_colours_and_ply(rm, tmp_path):
    _, _, host = rm
    mesh = extracted(host, 2)
    path = os.path.join(tmp_path, "mesh.ply")
    host.mesh_write_ply(mesh, path)
    _, verts, faces = S.parse_ply(path)
    assert np.stack([verts["x"], verts["y"], verts["z"]], 1).tobytes() == mesh.vertices.tobytes()
    assert np.stack([verts["nx"], verts["ny"], verts["nz"]], 1).tobytes() == mesh.normals.tobytes()
    assert np.array_equal(faces["v"], mesh.faces)
    rgb = np.stack([verts["red"], verts["green"], verts["blue"]], 1).astype(np.int64)
    # the sRGB encode of rm_view's RGBA8 output, to one code (float32 pow against float64)
    assert np.abs(rgb - S.srgb8(mesh.colors).astype(np.int64)).max() <= 1


def test_rm_train_mesh_cli(rm, tmp_path):
    from burn_raymarching_amd import _build
    path = os.path.join(tmp_path, "out", "mesh.ply")
    res = subprocess.run([_build.EXE, "mesh", "--scene", SCENE_JSON, "--out", path, "--res", "32"], capture_output=True,
                         text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    line = json.loads(res.stdout.strip().splitlines()[-1])
    print("rm_train mesh:", line)
    _, verts, faces = S.parse_ply(path)
    assert len(verts) == line["vertices"] > 0 and len(faces) == line["faces"] > 0 and line["open_edges"] == 0
    assert all(k in line for k in ("grid_ms", "copy_ms", "extract_ms", "refine_ms"))
    bad = subprocess.run([_build.EXE, "mesh", "--scene", SCENE_JSON], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "mesh" in bad.stderr
