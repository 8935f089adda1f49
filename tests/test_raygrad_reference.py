"""CPU pins of the checker the ray / camera-pose gradient tests use (tests/raygrad_ref.py): the
torch restatement of create_camera_rays against the oracle's, the two exact identities of the
reference's graph under torch fp64 autograd of oracle/autodiff_ref.render_diff, and the closed
form the kernels implement against that autograd. No kernel runs here."""
import json
import os

import numpy as np
import pytest
import torch

import raygrad_ref as rr
from conftest import FINAL1_CAMERA, GOLDEN, final1_scene

CAMS = json.load(open(os.path.join(GOLDEN, "cameras.json")))


def cam(i):
    c = CAMS[i]
    return (c["origin"], c["target"], c["fov"])


def random_scene(m, seed):
    from burn_raymarching_amd.model import synthetic_scene
    return synthetic_scene(m, seed)


# (scene, camera, width, height, k, steps): the shapes of the GPU cases, smaller images
CASES = [
    ("final1", cam(1), 12, 12, 32.0, 40),
    ("final1", cam(9), 12, 12, 5.0, 16),
    ("rand20", cam(3), 10, 10, 32.0, 24),
    ("final1", FINAL1_CAMERA, 8, 12, 32.0, 40),
]


def scene_of(name):
    return final1_scene() if name == "final1" else random_scene(20, 3)


@pytest.mark.parametrize("i", [1, 3, 5, 8, 9])
def test_camera_rays_match_the_oracle(oracle, i):
    c = cam(i)
    for w, h in ((24, 24), (16, 24)):
        o64, d64 = oracle.camera_rays(w, h, c[0], c[1], c[2], precision="f64")
        o, d = rr.camera_rays_t(w, h, torch.tensor(np.asarray(c[0], np.float32).astype(np.float64)),
                                torch.tensor(np.asarray(c[1], np.float32).astype(np.float64)),
                                torch.tensor(float(np.float32(c[2])), dtype=torch.float64))
        assert np.abs(o.numpy() - o64).max() <= 1e-12
        assert np.abs(d.numpy() - d64).max() <= 1e-12


@pytest.fixture(scope="module")
def case_grads(oracle):
    """Per case: rays, seeded grad_out and the autograd gradients (computed once)."""
    res = []
    for name, c, w, h, k, steps in CASES:
        sc = scene_of(name)
        o, d = oracle.camera_rays(w, h, c[0], c[1], c[2], precision="f64")
        gout = np.random.default_rng(11).standard_normal((w * h, 3))
        g_org, g_dir, g_cen = rr.ray_grads(o, d, sc, k, steps, gout, with_centers=True)
        res.append((sc, c, w, h, k, steps, o, d, gout, g_org, g_dir, g_cen))
    return res


def test_identity_origin_gradient_is_minus_centre_gradient(case_grads):
    """A shift of every sphere centre by s equals a shift of every ray origin by -s."""
    for sc, c, w, h, k, steps, o, d, gout, g_org, g_dir, g_cen in case_grads:
        assert np.abs(g_org).max() > 0
        assert np.abs(g_org.sum(0) + g_cen.sum(0)).max() <= 1e-10 * max(1.0, np.abs(g_cen).max())


def test_identity_rigid_camera_shift(case_grads):
    """g_eye + g_target = sum_i g_org[i]: a rigid shift of the camera leaves the directions alone."""
    for sc, c, w, h, k, steps, o, d, gout, g_org, g_dir, g_cen in case_grads:
        g_eye, g_tgt, _ = rr.camera_grads(c, w, h, sc, k, steps, gout)
        assert np.abs(g_eye + g_tgt - g_org.sum(0)).max() <= 1e-10 * max(1.0, np.abs(g_org).max())


def test_closed_form_equals_autograd(case_grads):
    for sc, c, w, h, k, steps, o, d, gout, g_org, g_dir, g_cen in case_grads:
        co, cd = rr.closed_form_ray_grads(o, d, sc, k, steps, gout)
        assert np.abs(co - g_org).max() <= 1e-9 * max(1.0, np.abs(g_org).max())
        assert np.abs(cd - g_dir).max() <= 1e-9 * max(1.0, np.abs(g_dir).max())
        # and the camera chain (13 sums + tail) against autograd through create_camera_rays
        g_eye, g_tgt, g_fov = rr.camera_grads(c, w, h, sc, k, steps, gout)
        t_eye, t_tgt, t_fov = rr.camera_tail(c, w, h, g_org, g_dir)
        scale = max(1.0, np.abs(g_eye).max(), np.abs(g_tgt).max())
        assert np.abs(t_eye - g_eye).max() <= 1e-9 * scale
        assert np.abs(t_tgt - g_tgt).max() <= 1e-9 * scale
        assert abs(t_fov - g_fov) <= 1e-9 * max(1.0, abs(g_fov))


def test_vertical_view_is_finite():
    """An exactly vertical view: forward x world-up is zero, math::normalize returns zeros and its
    Jacobian is taken as zero, so the pose gradient is finite (and flows only through forward)."""
    sc = final1_scene()
    c = ([0.0, 2.5, 0.0], [0.0, 0.0, 0.0], 50.0)
    gout = np.random.default_rng(5).standard_normal((64, 3))
    g_eye, g_tgt, g_fov = rr.camera_grads(c, 8, 8, sc, 32.0, 16, gout)
    assert np.isfinite(g_eye).all() and np.isfinite(g_tgt).all() and np.isfinite(g_fov)
    o, d = rr.camera_rays_t(8, 8, torch.tensor(c[0], dtype=torch.float64), torch.tensor(c[1], dtype=torch.float64),
                            torch.tensor(50.0, dtype=torch.float64))
    g_org, g_dir = rr.ray_grads(o.numpy(), d.numpy(), sc, 32.0, 16, gout)
    t_eye, t_tgt, t_fov = rr.camera_tail(c, 8, 8, g_org, g_dir)
    assert np.isfinite(t_eye).all() and np.isfinite(t_tgt).all() and np.isfinite(t_fov)
    assert np.abs(t_eye - g_eye).max() <= 1e-9 * max(1.0, np.abs(g_eye).max())
