"""CPU tests of the viewer's frame render (rm_view): the numpy restatement (tests/view_ref.py)
against known answers, the shader's pairwise fold against the log-sum-exp, the restatement's own
fp32 error on the GPU test's cases (so the reference alone is shown to stay inside the caps of
tests/test_gpu_view.py), and the entry points at the C-ABI boundary. No kernel runs here."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import view_ref as V
from conftest import GOLDEN, ROOT

HEADER = os.path.join(ROOT, "include", "raymarch.h")


def golden_scene():
    """tests/golden/scene.json as the viewer draws it: the stored radii, no +0.01."""
    return V.golden_scene(os.path.join(GOLDEN, "scene.json"))


# ---- 1. known answers --------------------------------------------------------------------------
def test_single_sphere_centre_ray():
    c, r, colour = np.array([[0.1, -0.05, 0.3]]), 0.35, np.array([[0.2, 0.7, 0.4]])
    light, amb = np.array([0.4, 0.8, -0.5]), 0.2
    scene = dict(centers=c, colors=colour, radius=np.array([r]), light_dir=light, ambient=np.array([amb]))
    pos = np.array([0.1, -0.05, -2.2])  # the sphere centre straight ahead: the middle of an odd frame
    cam = (pos, (0.0, 0.0, 1.0), (0.0, 1.0, 0.0))
    rgb, depth = V.view(cam, 5, 5, scene)
    want_t = np.linalg.norm(pos - c[0]) - r
    assert abs(want_t - depth[2, 2]) < 1e-3, (want_t, depth[2, 2])  # stops within hit_eps of the surface
    # one sphere: D = |p - c| - r exactly, the normal is radial: here (0, 0, -1)
    lu = light / np.linalg.norm(light)
    w = math.exp(-10.0 * (want_t - depth[2, 2]))
    want = colour[0] * (w / (w + 1e-5)) * (amb + max(-lu[2], 0.0) * (1 - amb))
    np.testing.assert_allclose(rgb[2, 2], want, rtol=0, atol=1e-6)
    # the corners look past the sphere: exact zeros and +inf
    assert (rgb[0, 0] == 0).all() and np.isinf(depth[0, 0])


def test_miss_and_inside_and_far():
    sc = golden_scene()
    away = V.view(V.view_camera((0.0, 0.0, -2.5), -math.pi / 2, 0.0), 16, 12, sc)
    assert (away[0] == 0).all() and np.isinf(away[1]).all()
    inside = V.view(V.view_camera(tuple(sc["centers"][0]), 1.0, 0.2), 16, 12, sc)
    assert (inside[1] == 0).all() and (inside[0].sum(-1) > 0).all()  # every ray hits at t = 0
    far = V.view(V.view_camera((0.0, 0.0, -6.0), math.pi / 2, 0.0), 96, 64, sc)
    # the shifted soft-min still sees the scene from 6 units: the centre pixels hit near t = 6 - r
    assert np.isfinite(far[1][30:34, 44:52]).any() and 5.0 < far[1][np.isfinite(far[1])].min() < 6.0


def test_iteration_count_and_zero_tap_sum():
    sc = golden_scene()
    _, depth, it = V.view(V.view_camera(*V.POSES[0]), 32, 24, sc, return_iters=True)
    assert it.min() >= 1 and it.max() <= 100
    assert (it[np.isfinite(depth)] < 100).all()
    # a point where the four taps cancel exactly (the centre of a lone sphere): diff = 0, not NaN
    one = dict(centers=np.zeros((1, 3)), colors=np.ones((1, 3)), radius=np.array([0.5]),
               light_dir=np.array([0.0, 1.0, 0.0]), ambient=np.array([0.25]))
    rgb, d = V.view(((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0)), 1, 1, one)
    assert d[0, 0] == 0.0 and np.isfinite(rgb).all()
    np.testing.assert_allclose(rgb[0, 0], 0.25 * (1.0 / (1.0 + 1e-5 / math.exp(5.0))), rtol=1e-12)


# ---- 2. the shader's fold is the log-sum-exp ---------------------------------------------------
@pytest.mark.parametrize("m,seed", [(6, None), (64, 0), (33, 2)])
def test_pairwise_fold_equals_lse_fp64(m, seed):
    sc = golden_scene() if seed is None else V.synthetic_scene(m, seed)
    c, r = sc["centers"].astype(np.float64), sc["radius"].astype(np.float64)
    rng = np.random.default_rng(7)
    p = rng.uniform(-1.0, 1.0, (4000, 3)) * 2.6
    near = np.sqrt(((p[:, None] - c[None]) ** 2).sum(-1)).min(-1) <= 2.0  # within 2 units of the scene
    p = p[near]
    assert len(p) > 1000
    np.testing.assert_allclose(V.sdf_fold(p, c, r, 32.0), V.sdf(p, c, r, 32.0), rtol=0, atol=1e-12)


# ---- 3. the restatement's own fp32 error on the GPU test's cases -------------------------------
CASES = V.parity_cases(golden_scene())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fp32_restatement_stays_inside_the_caps(case):
    name, scene, w, h, poses = case
    for pose in poses:
        cam = V.view_camera(*pose)
        ref = V.view(cam, w, h, scene)
        lo = V.view(cam, w, h, scene, dtype=np.float32)
        f = V.compare(lo[0], lo[1], ref[0], ref[1])
        print(name, pose, f)
        assert f["flips"] == 0 and f["over"] == 0, (name, pose, f)
        assert f["rgb_max"] <= 1e-3 and f["rgb_mean"] <= 1e-5 and f["miss_exact"], (name, pose, f)
    assert ref[0].shape == (h, w, 3)


# ---- 4. the C-ABI boundary ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    from burn_raymarching_amd import _build, native as nat
    _build.build_lib()
    return nat


def test_header_declares_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+rm_view\s*\(", text)
    assert re.search(r"\bvoid\s+rm_view_params_default\s*\(", text)
    assert "typedef struct rm_view_camera" in text and "typedef struct rm_view_params" in text


def test_library_exports_and_binding_has_them(native):
    lib = ctypes.CDLL(native.LIB_PATH)
    for name in ("rm_view", "rm_view_params_default"):
        assert hasattr(lib, name), name
        assert name in native.SIGNATURES, name
    assert len(native.SIGNATURES["rm_view"][1]) == 10
    p = native.view_params()
    assert (p.max_steps, p.smooth_k, p.t_max, p.color_sharpness, p.focal, p.flags) == (100, 32.0, 20.0, 10.0, 1.5, 0)
    assert p.hit_eps == np.float32(1e-3) and p.normal_eps == np.float32(1e-3)
    assert ctypes.sizeof(native.RmViewCamera) == 36 and ctypes.sizeof(native.RmViewParams) == 32


def test_null_context_is_rejected(native):
    cams = native.view_cameras([((0, 0, -2.5), (0, 0, 1), (0, 1, 0))])
    assert native.lib().rm_view(None, cams, 1, 8, 8, None, None, None, None, None) == 1


def test_kernel_header_is_a_hashed_source():
    from burn_raymarching_amd import _build
    assert "rm_view.h" in [os.path.basename(p) for p in _build.KERNEL_SOURCES]
    src = open(os.path.join(ROOT, "burn_raymarching_amd", "csrc", "rm_kernels.hip")).read()
    assert '#include "rm_view.h"' in src


def test_host_view_camera_start_pose():
    from burn_raymarching_amd import _build, host, render
    _build.build_host()
    pose = host.view_camera((0.0, 0.0, -2.5), math.pi / 2, 0.0)
    np.testing.assert_allclose(list(pose.forward), [0.0, 0.0, 1.0], rtol=0, atol=1e-7)
    np.testing.assert_allclose(list(pose.up), [0.0, 1.0, 0.0], rtol=0, atol=1e-7)
    assert list(pose.pos) == [0.0, 0.0, -2.5]
    # the torch-side helper and the restatement agree with it at an oblique pose
    a = host.view_camera((1.2, 0.6, -1.6), 2.2, -0.3)
    for other in (render.view_camera((1.2, 0.6, -1.6), 2.2, -0.3), V.view_camera((1.2, 0.6, -1.6), 2.2, -0.3)):
        np.testing.assert_allclose(list(a.forward), other[1], rtol=0, atol=1e-7)
        np.testing.assert_allclose(list(a.up), other[2], rtol=0, atol=1e-7)


def test_rgba_png_round_trip(tmp_path):
    from burn_raymarching_amd import _build, host
    _build.build_host()
    px = np.random.default_rng(0).integers(0, 256, (5, 7, 4), dtype=np.uint8)
    host.png_write_rgba(str(tmp_path / "a.png"), px)
    assert (host.png_read_rgba(str(tmp_path / "a.png")) == px).all()
    assert (host.png_read(str(tmp_path / "a.png")) == px[..., :3]).all()
