"""GPU tests of the ray and camera-pose gradients (rm_render_diff_backward_rays,
rm_render_diff_backward_cameras, render.render_diff with rays requiring grad,
render.render_diff_cameras) against torch fp64 autograd of oracle/autodiff_ref.render_diff.

Bounds are the project's own gradient bounds (conftest): normwise GRAD_TOL = 3e-3 and relative L2
REL_L2["bwd"] = 1e-3 over the whole [N,3] array; torch fp32 in the reference's op order sits at
6e-6 to 7e-4 and 4e-6 to 4e-4 on C1 to C4 and is recorded next to the GPU's error in every case.
The cases are the smallest shapes at which the kernel can still go wrong (see CASES)."""
import json
import os

import numpy as np
import pytest

import raygrad_ref as rr
from conftest import FINAL1_CAMERA, GOLDEN, GRAD_TOL, REL_ELEM, REL_L2, final1_scene, gpu_available, record_margin

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

CAMS = json.load(open(os.path.join(GOLDEN, "cameras.json")))


def cam(i):
    c = CAMS[i]
    return (c["origin"], c["target"], c["fov"])


def one_sphere():
    sc = final1_scene()
    return {"centers": np.array([[0.1, -0.05, 0.0]], np.float32), "colors": np.array([[0.8, 0.3, 0.2]], np.float32),
            "radius": np.array([0.45], np.float32), "light_dir": sc["light_dir"], "ambient": sc["ambient"]}


def synthetic(m, seed):
    from burn_raymarching_amd.model import synthetic_scene
    return synthetic_scene(m, seed)


# name -> (scene, k, steps, width, height, cameras): the array-mode cases take the rays of the
# listed cameras (C8, C10: plus one ray, 577 and 257 in all)
CASES = {
    "C1": (final1_scene, 32.0, 40, 24, 24, [1]),
    "C2": (final1_scene, 5.0, 16, 24, 24, [9]),
    "C3": (lambda: synthetic(64, 7), 32.0, 32, 24, 24, [3]),
    "C4": (final1_scene, 32.0, 40, 16, 24, [5]),            # non-square; 384 rays, no multiple of 256
    "C5": (one_sphere, 32.0, 16, 24, 24, [1]),               # M = 1
    "C6": (lambda: synthetic(70, 8), 32.0, 16, 24, 24, [3]),  # odd pair padding
    "C7": (lambda: synthetic(300, 9), 32.0, 16, 20, 24, [1]),  # several 64-sphere groups, above 256
    "C8": (final1_scene, 32.0, 40, 24, 24, [1]),             # array mode, 577 rays: partial wave and block
    "C9": (final1_scene, 32.0, 40, 20, 24, [1, 3, 5]),       # view boundaries inside 256-ray blocks (row order)
    # 520 spheres: 272 pairs, two blocks of the record kernel (partial headers in the record buffer); array
    # mode 257 rays (one 16x16 view plus one ray)
    "C10": (lambda: synthetic(520, 10), 32.0, 16, 16, 16, [1]),
}
RAY_CASES = ["C1", "C2", "C3", "C4", "C5", "C6", "C7", "C8", "C10"]
CAM_CASES = ["C1", "C2", "C3", "C4", "C7", "C9", "C10"]


@pytest.fixture(scope="module")
def rm():
    import torch
    from burn_raymarching_amd import _build
    _build.build_lib()
    from burn_raymarching_amd import native, render
    torch.cuda.init()
    return render, native


def dev(x, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def scene_dev(render, sc, half_colors=False):
    col = dev(sc["colors"]).half() if half_colors else dev(sc["colors"])
    return render.Scene(dev(sc["centers"]), col, dev(sc["radius"]), dev(sc["light_dir"]), dev(sc["ambient"]))


_CACHE = {}


def case(oracle, name):
    """The case's inputs and its fp64 reference gradients, computed once and left unchanged."""
    if name in _CACHE:
        return _CACHE[name]
    make, k, steps, w, h, cams = CASES[name]
    sc = make()
    os_, ds_ = [], []
    for i in cams:
        c = cam(i)
        o, d = oracle.camera_rays(w, h, c[0], c[1], c[2], precision="f32")
        os_.append(o)
        ds_.append(d)
    o, d = np.concatenate(os_), np.concatenate(ds_)
    if name in ("C8", "C10"):
        o, d = np.concatenate([o, o[100:101]]), np.concatenate([d, d[100:101]])
    gout = np.random.default_rng(sum(map(ord, name))).standard_normal(o.shape).astype(np.float32)
    ref_o, ref_d = rr.ray_grads(o, d, sc, k, steps, gout)
    c = dict(sc=sc, k=k, steps=steps, w=w, h=h, cams=[cam(i) for i in cams], o=o, d=d, gout=gout, ref_o=ref_o,
             ref_d=ref_d)
    _CACHE[name] = c
    return c


def errors(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return np.abs(a - b).max() / np.abs(b).max(), np.linalg.norm(a - b) / np.linalg.norm(b)


def bits(t):
    return host(t).view(np.uint32)


# ---- 1. per-ray parity ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", RAY_CASES)
def test_ray_gradients_match_autograd(rm, oracle, name):
    import torch
    render, _ = rm
    c = case(oracle, name)
    nz = (np.abs(c["ref_o"]).max(1) > 0) | (np.abs(c["ref_d"]).max(1) > 0)
    assert nz.sum() >= 30, ("the case proves nothing", int(nz.sum()))
    g_org, g_dir = render.render_diff_backward_rays(dev(c["o"]), dev(c["d"]), scene_dev(render, c["sc"]), c["k"],
                                                    dev(c["gout"]), c["steps"])
    g_org, g_dir = host(g_org), host(g_dir)
    f32_o, f32_d = rr.ray_grads(c["o"], c["d"], c["sc"], c["k"], c["steps"], c["gout"], dtype=torch.float32)
    assert np.isfinite(g_org).all() and np.isfinite(g_dir).all()
    for what, got, f32, ref in (("g_org", g_org, f32_o, c["ref_o"]), ("g_dir", g_dir, f32_d, c["ref_d"])):
        norm, rl2 = errors(got, ref)
        fn, fl = errors(f32, ref)
        print(f"{name} {what}: gpu normwise {norm:.3e} relL2 {rl2:.3e} | torch fp32 {fn:.3e} {fl:.3e} | "
              f"non-zero rays {int(nz.sum())}")
        record_margin(f"raygrad_{what}", norm, GRAD_TOL)
        record_margin(f"raygrad_relL2_{what}", rl2, REL_L2["bwd"])
        record_margin(f"raygrad_torch_f32_{what}", fn, GRAD_TOL)
        record_margin(f"raygrad_torch_f32_relL2_{what}", fl, REL_L2["bwd"])
        assert norm <= GRAD_TOL, (name, what, "normwise", norm, "torch fp32", fn)
        assert rl2 <= REL_L2["bwd"], (name, what, "relL2", rl2, "torch fp32", fl)
        # per ray (raygrad_ref.per_ray_errors): a ray that is small next to the largest is held too
        for floor, err, bound, f32_err, cap_ok in rr.per_ray_check(got, f32, ref, REL_ELEM["bwd"]):
            print(f"{name} {what}: rays >= {floor:g} of the largest: gpu {err:.3e} (bound {bound:.3g}) | torch fp32 {f32_err:.3e}")
            record_margin(f"raygrad_per_ray{floor:g}_{what}", err, bound)
            assert cap_ok, (name, what, floor, "torch fp32 breaks the cap", f32_err)
            assert err <= bound, (name, what, f"per ray (|g| >= {floor:g} max)", err, bound, "torch fp32", f32_err)
    # escaped rays: exact zeros in the reference, exact zeros on the GPU
    assert (g_org[~nz] == 0).all() and (g_dir[~nz] == 0).all()


# ---- 2. identity on the GPU ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C1", "C3", "C7"])
def test_origin_gradient_sums_to_minus_centre_gradient(rm, oracle, name):
    render, _ = rm
    c = case(oracle, name)
    scene = scene_dev(render, c["sc"])
    o, d, g = dev(c["o"]), dev(c["d"]), dev(c["gout"])
    g_org, _ = render.render_diff_backward_rays(o, d, scene, c["k"], g, c["steps"], want_dir=False)
    grads = render.render_diff_backward(o, d, scene, c["k"], g, c["steps"])
    a = host(g_org).astype(np.float64).sum(0)
    b = -host(grads["centers"]).astype(np.float64).sum(0)
    err = np.abs(a - b).max() / np.abs(b).max()
    record_margin("raygrad_identity_centers", err, GRAD_TOL)
    assert err <= GRAD_TOL, (a, b)


# ---- 3. camera parity ----------------------------------------------------------------------------
def camera_call(render, native, c, flags=0, t_march=None, **kw):
    return render.render_diff_backward_cameras(c["cams"], c["w"], c["h"], scene_dev(render, c["sc"]), c["k"],
                                               dev(c["gout"][:len(c["cams"]) * c["w"] * c["h"]]), c["steps"],
                                               t_march=t_march, flags=flags, **kw)


def check_camera(name, got, c, oracle_tag=""):
    npix = c["w"] * c["h"]
    for v, cm in enumerate(c["cams"]):
        ref_eye, ref_tgt, ref_fov = rr.camera_grads(cm, c["w"], c["h"], c["sc"], c["k"], c["steps"],
                                                    c["gout"][v * npix:(v + 1) * npix])
        e_eye = np.abs(got[v, 0:3] - ref_eye).max() / np.abs(ref_eye).max()
        e_tgt = np.abs(got[v, 3:6] - ref_tgt).max() / np.abs(ref_tgt).max()
        e_fov = abs(got[v, 6] - ref_fov) / abs(ref_fov)
        print(f"{name}{oracle_tag} view {v}: g_eye {e_eye:.3e} g_target {e_tgt:.3e} g_fov {e_fov:.3e}")
        record_margin("raygrad_cam_eye", e_eye, GRAD_TOL)
        record_margin("raygrad_cam_target", e_tgt, GRAD_TOL)
        record_margin("raygrad_cam_fov", e_fov, GRAD_TOL)
        assert e_eye <= GRAD_TOL and e_tgt <= GRAD_TOL and e_fov <= GRAD_TOL, (name, v, e_eye, e_tgt, e_fov)


@pytest.mark.parametrize("name", CAM_CASES)
def test_camera_gradients_match_autograd(rm, oracle, name):
    render, native = rm
    c = case(oracle, name)
    got = host(camera_call(render, native, c)).astype(np.float64)
    assert got.shape == (len(c["cams"]), 7) and np.isfinite(got).all()
    check_camera(name, got, c)
    if name == "C9":  # rows instead of tiles: view boundaries fall inside 256-ray blocks of the row order
        got = host(camera_call(render, native, c, flags=native.RM_MARCH_ROW_ORDER)).astype(np.float64)
        check_camera(name, got, c, " (row order)")


def test_near_vertical_views_are_finite(rm, oracle):
    """cameras.json[8] looks almost along world-up (1 / |forward x up| ~ 2500) and an exactly
    vertical view has forward x up = 0: finite values only."""
    render, native = rm
    c = dict(case(oracle, "C1"))
    c["cams"] = [cam(8), ([0.0, 2.5, 0.0], [0.0, 0.0, 0.0], 50.0)]
    c["gout"] = np.concatenate([c["gout"], c["gout"]])
    got = host(camera_call(render, native, c))
    assert np.isfinite(got).all()


# ---- 4. consistency ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C1", "C4", "C9"])
def test_camera_mode_equals_array_mode(rm, oracle, name):
    render, native = rm
    c = case(oracle, name)
    npix = c["w"] * c["h"]
    scene = scene_dev(render, c["sc"])
    got = host(camera_call(render, native, c)).astype(np.float64)
    for v, cm in enumerate(c["cams"]):
        o, d = render.create_camera_rays(c["w"], c["h"], cm[0], cm[1], cm[2])
        g_org, g_dir = render.render_diff_backward_rays(o, d, scene, c["k"], dev(c["gout"][v * npix:(v + 1) * npix]),
                                                        c["steps"])
        eye, tgt, fov = rr.camera_tail(cm, c["w"], c["h"], host(g_org), host(g_dir))
        assert np.abs(got[v, 0:3] - eye).max() <= GRAD_TOL * np.abs(eye).max()
        assert np.abs(got[v, 3:6] - tgt).max() <= GRAD_TOL * np.abs(tgt).max()
        assert abs(got[v, 6] - fov) <= GRAD_TOL * abs(fov)
        # a rigid shift of the camera: g_eye + g_target = sum_i g_org[i]
        s = host(g_org).astype(np.float64).sum(0)
        assert np.abs(got[v, 0:3] + got[v, 3:6] - s).max() <= GRAD_TOL * np.abs(s).max()


@pytest.mark.parametrize("name", ["C3", "C8"])
def test_rays_saved_t_replay_determinism_accumulate_and_null_outputs(rm, oracle, name):
    import torch
    render, _ = rm
    c = case(oracle, name)
    scene = scene_dev(render, c["sc"])
    o, d, g = dev(c["o"]), dev(c["d"]), dev(c["gout"])
    _, t = render.render_diff_forward(o, d, scene, c["k"], c["steps"], return_t=True)
    a_o, a_d = render.render_diff_backward_rays(o, d, scene, c["k"], g, c["steps"], t_march=t)
    b_o, b_d = render.render_diff_backward_rays(o, d, scene, c["k"], g, c["steps"])  # the march replayed
    assert (bits(a_o) == bits(b_o)).all() and (bits(a_d) == bits(b_d)).all()
    c_o, c_d = render.render_diff_backward_rays(o, d, scene, c["k"], g, c["steps"], t_march=t)
    assert (bits(a_o) == bits(c_o)).all() and (bits(a_d) == bits(c_d)).all()
    # accumulate = 1 after accumulate = 0: twice the value, bit for bit
    render.render_diff_backward_rays(o, d, scene, c["k"], g, c["steps"], t_march=t, grad_org=c_o, grad_dir=c_d,
                                     accumulate=True)
    assert (bits(c_o) == bits(a_o * 2)).all() and (bits(c_d) == bits(a_d * 2)).all()
    # one NULL output leaves the other's bits unchanged (and the skipped tensor untouched)
    only_o, none_d = render.render_diff_backward_rays(o, d, scene, c["k"], g, c["steps"], t_march=t, want_dir=False)
    none_o, only_d = render.render_diff_backward_rays(o, d, scene, c["k"], g, c["steps"], t_march=t, want_org=False)
    assert none_d is None and none_o is None
    assert (bits(only_o) == bits(a_o)).all() and (bits(only_d) == bits(a_d)).all()
    assert torch.isfinite(a_o).all() and torch.isfinite(a_d).all()


def test_cameras_saved_t_replay_determinism_and_accumulate(rm, oracle):
    render, native = rm
    c = case(oracle, "C9")
    scene = scene_dev(render, c["sc"])
    _, t = render.render_diff_camera(c["cams"], c["w"], c["h"], scene, c["k"], c["steps"], return_t=True)
    a = camera_call(render, native, c, t_march=t)
    b = camera_call(render, native, c)
    assert (bits(a) == bits(b)).all()
    a2 = camera_call(render, native, c, t_march=t)
    assert (bits(a) == bits(a2)).all()
    camera_call(render, native, c, t_march=t, grad_cams=a2, accumulate=True)
    assert (bits(a2) == bits(a * 2)).all()


def test_more_views_than_one_call_takes(rm, oracle):
    """130 views run as chunks of RM_MAX_VIEWS_PER_CALL (the device camera table past 16 views)."""
    render, native = rm
    c = dict(case(oracle, "C1"))
    c["w"], c["h"] = 8, 8
    c["cams"] = [cam(1), cam(3)] * 65
    g = np.random.default_rng(3).standard_normal((64, 3)).astype(np.float32)
    c["gout"] = np.concatenate([g] * 130)
    got = host(camera_call(render, native, c))
    assert got.shape == (130, 7) and np.isfinite(got).all()
    assert (got[0::2].view(np.uint32) == got[0].view(np.uint32)).all()
    assert (got[1::2].view(np.uint32) == got[1].view(np.uint32)).all()


def test_fp16_colour_scene(rm, oracle):
    render, _ = rm
    c = case(oracle, "C1")
    sc = dict(c["sc"])
    sc["colors"] = sc["colors"].astype(np.float16).astype(np.float32)  # the widened colours
    ref_o, ref_d = rr.ray_grads(c["o"], c["d"], sc, c["k"], c["steps"], c["gout"])
    g_org, g_dir = render.render_diff_backward_rays(dev(c["o"]), dev(c["d"]), scene_dev(render, c["sc"], True),
                                                    c["k"], dev(c["gout"]), c["steps"])
    for what, got, ref in (("g_org", host(g_org), ref_o), ("g_dir", host(g_dir), ref_d)):
        norm, rl2 = errors(got, ref)
        record_margin(f"raygrad_f16_{what}", norm, GRAD_TOL)
        assert norm <= GRAD_TOL and rl2 <= REL_L2["bwd"], (what, norm, rl2)


# ---- 5. autograd surface ---------------------------------------------------------------------------
def scene_leaves(sc):
    return [dev(sc[k]).requires_grad_() for k in ("centers", "colors", "radius", "light_dir", "ambient")]


def test_render_diff_returns_ray_gradients(rm, oracle):
    render, _ = rm
    c = case(oracle, "C1")
    g = dev(c["gout"])
    o, d = dev(c["o"]).requires_grad_(), dev(c["d"]).requires_grad_()
    leaves = scene_leaves(c["sc"])
    out = render.render_diff(o, d, *leaves, c["k"], c["steps"])
    (out * g).sum().backward()
    assert o.grad is not None and d.grad is not None
    scene = scene_dev(render, c["sc"])
    _, t = render.render_diff_forward(o.detach(), d.detach(), scene, c["k"], c["steps"], return_t=True)
    ref_o, ref_d = render.render_diff_backward_rays(o.detach(), d.detach(), scene, c["k"], g, c["steps"], t_march=t)
    assert (bits(o.grad) == bits(ref_o)).all() and (bits(d.grad) == bits(ref_d)).all()
    # the scene gradients are the same bits with and without the ray gradients requested
    leaves2 = scene_leaves(c["sc"])
    (render.render_diff(dev(c["o"]), dev(c["d"]), *leaves2, c["k"], c["steps"]) * g).sum().backward()
    for a, b in zip(leaves, leaves2):
        assert (bits(a.grad) == bits(b.grad)).all()
    # only the origin requires grad: the direction gets none
    o2, d2 = dev(c["o"]).requires_grad_(), dev(c["d"])
    (render.render_diff(o2, d2, *[x.detach() for x in leaves], c["k"], c["steps"]) * g).sum().backward()
    assert (bits(o2.grad) == bits(ref_o)).all() and d2.grad is None


def test_render_diff_cameras_backward_equals_the_low_level_calls(rm, oracle):
    import torch
    render, native = rm
    c = case(oracle, "C9")
    npix = c["w"] * c["h"]
    g = dev(c["gout"][:3 * npix])
    eye = torch.tensor([cm[0] for cm in c["cams"]], dtype=torch.float32, requires_grad=True)
    tgt = torch.tensor([cm[1] for cm in c["cams"]], dtype=torch.float32, requires_grad=True)
    fov = torch.tensor([cm[2] for cm in c["cams"]], dtype=torch.float32, requires_grad=True)
    leaves = scene_leaves(c["sc"])
    out = render.render_diff_cameras(eye, tgt, fov, c["w"], c["h"], *leaves, c["k"], c["steps"])
    assert out.shape == (3 * npix, 3)
    (out * g).sum().backward()
    scene = scene_dev(render, c["sc"])
    fwd, t = render.render_diff_camera(c["cams"], c["w"], c["h"], scene, c["k"], c["steps"], return_t=True)
    assert (bits(out) == bits(fwd)).all()
    gc = host(render.render_diff_backward_cameras(c["cams"], c["w"], c["h"], scene, c["k"], g, c["steps"], t_march=t))
    assert (eye.grad.numpy().view(np.uint32) == gc[:, 0:3].view(np.uint32)).all()
    assert (tgt.grad.numpy().view(np.uint32) == gc[:, 3:6].view(np.uint32)).all()
    assert (fov.grad.numpy().view(np.uint32) == gc[:, 6].view(np.uint32)).all()
    gs = render.render_diff_backward_camera(c["cams"], c["w"], c["h"], scene, c["k"], g, c["steps"], t_march=t)
    for leaf, key in zip(leaves, ("centers", "colors", "radius", "light_dir", "ambient")):
        assert (bits(leaf.grad).reshape(-1) == bits(gs[key]).reshape(-1)).all(), key


# ---- 6. existing behaviour -------------------------------------------------------------------------
def test_scene_only_backward_runs_the_parent_launches(rm, oracle):
    """With only scene inputs requiring grad the autograd path times the same launches as the
    direct forward + parameter backward; asking for the ray gradients adds exactly one."""
    render, _ = rm
    c = case(oracle, "C3")
    g = dev(c["gout"])
    o, d = dev(c["o"]), dev(c["d"])
    ctx = render.context(o.device)
    ctx.timing(True)
    try:
        ctx.collect_timing()
        scene = scene_dev(render, c["sc"])
        _, t = render.render_diff_forward(o, d, scene, c["k"], c["steps"], return_t=True)
        render.render_diff_backward(o, d, scene, c["k"], g, c["steps"], t_march=t)
        _, direct = ctx.collect_timing()
        (render.render_diff(o, d, *scene_leaves(c["sc"]), c["k"], c["steps"]) * g).sum().backward()
        _, scene_only = ctx.collect_timing()
        o2 = dev(c["o"]).requires_grad_()
        (render.render_diff(o2, d, *scene_leaves(c["sc"]), c["k"], c["steps"]) * g).sum().backward()
        _, with_rays = ctx.collect_timing()
    finally:
        ctx.timing(False)
    assert direct >= 2 and scene_only == direct and with_rays == direct + 1, (direct, scene_only, with_rays)


# ---- 7. refinement ---------------------------------------------------------------------------------
def refine(render_fn, steps=30, lr=0.004):
    """Adam on one offset added to eye and target of FINAL1_CAMERA; render_fn(eye [1,3], target
    [1,3]) -> image. Returns (loss_0, loss_end, |offset_0|, |offset_end|); the true pose is offset 0."""
    import torch
    eye0 = torch.tensor([FINAL1_CAMERA[0]], dtype=torch.float64)
    tgt0 = torch.tensor([FINAL1_CAMERA[1]], dtype=torch.float64)
    with torch.no_grad():
        target = render_fn(eye0, tgt0).detach()
    off = torch.tensor([0.06, -0.04, 0.05], dtype=torch.float64, requires_grad=True)
    n0 = float(off.detach().norm())
    opt = torch.optim.Adam([off], lr=lr)
    first = None
    for _ in range(steps):
        opt.zero_grad()
        loss = ((render_fn(eye0 + off, tgt0 + off) - target) ** 2).mean()
        first = float(loss.detach()) if first is None else first
        loss.backward()
        opt.step()
    with torch.no_grad():
        last = float(((render_fn(eye0 + off, tgt0 + off) - target) ** 2).mean())
    return first, last, n0, float(off.detach().norm())


def test_pose_refinement_recovers_a_rigid_shift(rm):
    """scene.json at 48x48, k = 32, 40 steps: 30 Adam iterations at lr 0.004 through
    render_diff_cameras halve the loss and bring the offset to 0.6 of its start. The reference's
    own gradient (torch fp64) reaches 0.13 to 0.22 and 0.27 to 0.34 over three cameras; the same
    loop runs here on the CPU restatement first, so the bound rests on the reference."""
    import torch
    render, _ = rm
    sc = final1_scene()
    w = h = 48
    k, steps = 32.0, 40
    s64 = rr.scene_t(sc)
    fov64 = torch.tensor(float(FINAL1_CAMERA[2]), dtype=torch.float64)

    def cpu_render(eye, tgt):
        o, d = rr.camera_rays_t(w, h, eye[0], tgt[0], fov64)
        return rr._render(o, d, s64, k, steps)

    l0, l1, n0, n1 = refine(cpu_render)
    print(f"reference: loss {l0:.3e} -> {l1:.3e} ({l1 / l0:.3f}), |offset| {n0:.4f} -> {n1:.4f} ({n1 / n0:.3f})")
    assert l1 <= 0.5 * l0 and n1 <= 0.6 * n0, ("the reference itself", l1 / l0, n1 / n0)

    leaves = [dev(sc[key]) for key in ("centers", "colors", "radius", "light_dir", "ambient")]
    fov = torch.tensor([FINAL1_CAMERA[2]], dtype=torch.float32)

    def gpu_render(eye, tgt):
        return render.render_diff_cameras(eye.float(), tgt.float(), fov, w, h, *leaves, k, steps).double()

    g0, g1, m0, m1 = refine(gpu_render)
    print(f"gpu: loss {g0:.3e} -> {g1:.3e} ({g1 / g0:.3f}), |offset| {m0:.4f} -> {m1:.4f} ({m1 / m0:.3f})")
    record_margin("raygrad_refine_loss", g1 / g0, 0.5)
    record_margin("raygrad_refine_offset", m1 / m0, 0.6)
    assert g1 <= 0.5 * g0 and m1 <= 0.6 * m0, (g1 / g0, m1 / m0)
