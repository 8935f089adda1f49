"""The kernels against the references at values of rm_march.normal_eps / color_sharpness /
mask_sharpness other than the reference's 1e-4 / 10 / 15 (tests/constants_ref.py): every entry point
that consumes the three fields, on the general and on the small-scene kernel, in array mode and in
camera mode, against the fp64 oracle with the reference's six-tap normal (and, at normal_eps = 1e-2,
against the oracle's limit normal: include/raymarch.h, rm_march); the ray and camera-pose gradients
against torch autograd of oracle/autodiff_ref.py at the same constants, per ray too; the segments of
the camera gradient's finish kernel; and the library's bit-level promises (early exit, t_march,
skipped blocks, fused calls) where the march policy is not the default's. The bounds are
constants_ref's: max(the suite's bound, 4 x the fp32 reference-order oracle's own error), capped;
tests/test_constants_reference.py shows on the CPU that they pass the fp32 oracle with room and fail
a constant that is ignored, swapped or wrong by 2 %."""
import ctypes

import numpy as np
import pytest

import constants_ref as C
import envelope_ref as E
import raygrad_ref as rr
import test_gpu_envelope as G
from conftest import GRAD_KEYS, GRAD_TOL, REL_ELEM, REL_L2, final1_scene, gpu_available, record_margin

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

dev, host, scene_dev, same_bits = G.dev, G.host, G.scene_dev, G.same_bits
PLAIN = tuple(n for n in C.names() if n not in C.SPLIT_NAMES) + C.LIMIT_NAMES
SMALL = tuple(n for n in PLAIN if n.endswith("-M12"))
POLICY = tuple(f"{s}-M{m}" for s in ("msharp2", "msharp60", "all") for m in (48, 12))  # the bit-level promises
W = E.WIDTH


@pytest.fixture(scope="module")
def rm():
    import torch
    from burn_raymarching_amd import _build
    _build.build_lib()
    from burn_raymarching_amd import native, render
    torch.cuda.init()
    return render, native


_RUNS = {}


def run_gpu(rm, name, camera=False, **env):
    """envelope_ref.run_oracle's keys from the device at the case's constants, plus out_fast (the
    forward without t_march, the only one that may leave the march early) and bwd_t (the backward
    on the forward's saved t_march). Once per (case, mode, environment)."""
    key = (name, camera, tuple(sorted(env.items())))
    if key in _RUNS:
        return _RUNS[key]
    import torch
    render = rm[0]
    c = C.case(name)
    kw = C.consts_kw(c["consts"])
    s = scene_dev(rm, c["scene"])
    k, steps = c["k"], c["steps"]
    g, tg = dev(c["grad_out"]), dev(c["targets"])
    with pytest.MonkeyPatch.context() as mp:
        for var, val in env.items():
            mp.setenv(var, val)
        if camera:
            cams = [c["camera"]]
            out, t = render.render_diff_camera(cams, W, W, s, k, steps, return_t=True, **kw)
            fast = render.render_diff_camera(cams, W, W, s, k, steps, **kw)
            bwd = render.render_diff_backward_camera(cams, W, W, s, k, g, steps, **kw)
            bwd_t = render.render_diff_backward_camera(cams, W, W, s, k, g, steps, t_march=t, **kw)
            tout = torch.empty_like(out)
            loss, train, _ = render.train_step_camera(cams, W, W, tg, s, k, E.PROGRESS, steps, out=tout, **kw)
        else:
            o, d = dev(c["org"]), dev(c["dir"])
            out, t = render.render_diff_forward(o, d, s, k, steps, return_t=True, **kw)
            fast = render.render_diff_forward(o, d, s, k, steps, **kw)
            bwd = render.render_diff_backward(o, d, s, k, g, steps, **kw)
            bwd_t = render.render_diff_backward(o, d, s, k, g, steps, t_march=t, **kw)
            loss, train, tout = render.train_step(o, d, tg, s, k, E.PROGRESS, steps, with_out=True, **kw)
    got = {"out": host(out), "t": host(t), "out_fast": host(fast), "bwd": {q: host(v) for q, v in bwd.items()},
           "bwd_t": {q: host(v) for q, v in bwd_t.items()}, "train_out": host(tout), "loss": float(host(loss)[0]),
           "train": {q: host(v) for q, v in train.items()}}
    _RUNS[key] = got
    return got


def check(got, name, label):
    """Every measure within the case's derived bound, and t_march of the seen rays within T_REL; the
    figures go to the margins record."""
    assert G.all_finite(got), label
    ms, bnd = E.measures(got, C.reference(name)), C.bounds(name)
    for key, v in ms.items():
        record_margin("const_" + "_".join(key), v, bnd[key])
    worst = max(ms, key=lambda q: ms[q] / bnd[q])
    print(f"constants parity {label}: worst {ms[worst] / bnd[worst]:.3f} of bound at {worst} "
          f"({ms[worst]:.3g}, bound {bnd[worst]:.3g})")
    bad = {q: (v, bnd[q]) for q, v in ms.items() if not v <= bnd[q]}
    assert not bad, (label, bad)
    t_err = E.t_rel_error(got["t"], C.reference(name)["t"])[C.seen(name)].max()
    record_margin("const_t_march", t_err, E.T_REL)
    assert t_err <= E.T_REL, (label, "t_march of the seen rays", t_err)


# ---- 1. reference parity ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", PLAIN)
def test_array_mode_matches_reference(rm, name):
    """rm_render_diff, rm_render_diff_backward, rm_train_step and t_march, RM_SMALL at its default. The
    LIMIT cases (normal_eps = 1e-2) are held to the oracle's limit normal, all others to its six taps."""
    got = run_gpu(rm, name)
    check(got, name, f"{name} array")
    assert np.array_equal(got["out"].view(np.uint32), got["out_fast"].view(np.uint32)), "t_march changes the image"
    same_bits({"bwd": got["bwd"]}, {"bwd": got["bwd_t"]}, f"{name} backward on the saved t_march", keys=("bwd",))


@pytest.mark.parametrize("name", PLAIN)
def test_camera_mode_matches_reference(rm, name):
    """rm_render_diff_camera, rm_render_diff_backward_camera, rm_train_step_camera."""
    got = run_gpu(rm, name, camera=True)
    check(got, name, f"{name} camera")
    assert np.array_equal(got["out"].view(np.uint32), got["out_fast"].view(np.uint32)), "t_march changes the image"
    same_bits({"bwd": got["bwd"]}, {"bwd": got["bwd_t"]}, f"{name} backward on the saved t_march", keys=("bwd",))


@pytest.mark.parametrize("name", SMALL)
def test_general_kernel_at_small_m_matches_reference(rm, name):
    """The M = 12 cases on the general kernel (RM_SMALL=0; the default takes the small-scene one)."""
    check(run_gpu(rm, name, RM_SMALL="0"), name, f"{name} array RM_SMALL=0")
    check(run_gpu(rm, name, camera=True, RM_SMALL="0"), name, f"{name} camera RM_SMALL=0")


@pytest.mark.parametrize("split", ["1", "0"])
@pytest.mark.parametrize("name", C.SPLIT_NAMES)
def test_split_march_at_m300(rm, name, split):
    check(run_gpu(rm, name, RM_SPLIT=split), name, f"{name} array RM_SPLIT={split}")
    check(run_gpu(rm, name, camera=True, RM_SPLIT=split), name, f"{name} camera RM_SPLIT={split}")


@pytest.mark.parametrize("m", E.SIZES)
@pytest.mark.parametrize("cset", tuple(C.SETS) + ("limit",))
def test_stages_match_reference(rm, cset, m):
    """rm_debug_intermediates: lighting, mask and mix of the seen rays against render_diff_debug in
    fp64, so that a constant that goes wrong names its stage (normal_eps: lighting; color_sharpness:
    mix; mask_sharpness: mask)."""
    import torch
    render, native = rm
    name = f"{cset}-M{m}"
    c = C.case(name)
    s = scene_dev(rm, c["scene"])
    o, d = dev(c["org"]), dev(c["dir"])
    dbg = torch.full((len(c["org"]), 24), float("nan"), device="cuda")
    march = s.march_for(native.march_params(c["steps"], c["k"], *c["consts"]))
    ctx = render.context()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    ctx.check(ctx._lib.rm_debug_intermediates(ctx.handle, p(o), p(d), len(c["org"]), ctypes.byref(s.c_struct()),
                                              ctypes.byref(march), p(dbg)), "rm_debug_intermediates")
    err, bnd = C.stage_errors(host(dbg), name), C.stage_bounds(name)
    for st, v in err.items():
        record_margin("const_stage_" + st, v, bnd[st])
    print(f"constants stages {name}: " + ", ".join(f"{st} {v:.3g} (bound {bnd[st]:.3g})" for st, v in err.items()))
    assert all(v <= bnd[st] for st, v in err.items()), (name, err, bnd)


# ---- 2. ray and camera-pose gradients --------------------------------------------------------------
def _norm_errors(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return np.abs(a - b).max() / np.abs(b).max(), np.linalg.norm(a - b) / np.linalg.norm(b)


def check_per_ray(label, what, got, f32, ref):
    for floor, err, bound, f32_err, cap_ok in rr.per_ray_check(got, f32, ref, REL_ELEM["bwd"]):
        print(f"{label} {what}: rays >= {floor:g} of the largest: gpu {err:.3e} (bound {bound:.3g}) | torch fp32 {f32_err:.3e}")
        record_margin(f"const_raygrad_per_ray{floor:g}_{what}", err, bound)
        assert cap_ok, (label, what, floor, "torch fp32 breaks the cap", f32_err)
        assert err <= bound, (label, what, f"per ray (|g| >= {floor:g} max)", err, bound, "torch fp32", f32_err)


def check_camera_row(label, got, ref):
    ref_eye, ref_tgt, ref_fov = ref
    e_eye = np.abs(got[0:3] - ref_eye).max() / np.abs(ref_eye).max()
    e_tgt = np.abs(got[3:6] - ref_tgt).max() / np.abs(ref_tgt).max()
    e_fov = abs(got[6] - ref_fov) / abs(ref_fov)
    print(f"{label}: g_eye {e_eye:.3e} g_target {e_tgt:.3e} g_fov {e_fov:.3e}")
    for what, e in (("eye", e_eye), ("target", e_tgt), ("fov", e_fov)):
        record_margin("const_cam_" + what, e, GRAD_TOL)
    assert e_eye <= GRAD_TOL and e_tgt <= GRAD_TOL and e_fov <= GRAD_TOL, (label, e_eye, e_tgt, e_fov)


@pytest.mark.parametrize("m", E.SIZES)
@pytest.mark.parametrize("cset", C.RAYGRAD_SETS)
def test_ray_and_camera_gradients_match_autograd(rm, cset, m):
    """rm_render_diff_backward_rays and rm_render_diff_backward_cameras against torch fp64 autograd of
    autodiff_ref.render_diff at the case's constants: the suite's normwise and relative-L2 bounds
    over the whole array, and the per-ray measure of raygrad_ref."""
    import torch
    render, _ = rm
    name = f"{cset}-M{m}"
    c = C.case(name)
    kw = C.consts_kw(c["consts"])
    args = (c["org"], c["dir"], c["scene"], c["k"], c["steps"], c["grad_out"])
    ref_o, ref_d = rr.ray_grads(*args, **kw)
    f32_o, f32_d = rr.ray_grads(*args, dtype=torch.float32, **kw)
    nz = (np.abs(ref_o).max(1) > 0) | (np.abs(ref_d).max(1) > 0)
    assert nz.sum() >= 30, ("the case proves nothing", int(nz.sum()))
    s = scene_dev(rm, c["scene"])
    g_org, g_dir = render.render_diff_backward_rays(dev(c["org"]), dev(c["dir"]), s, c["k"], dev(c["grad_out"]),
                                                    c["steps"], **kw)
    g_org, g_dir = host(g_org), host(g_dir)
    assert np.isfinite(g_org).all() and np.isfinite(g_dir).all()
    for what, got, f32, ref in (("g_org", g_org, f32_o, ref_o), ("g_dir", g_dir, f32_d, ref_d)):
        norm, rl2 = _norm_errors(got, ref)
        fn, fl = _norm_errors(f32, ref)
        print(f"{name} {what}: gpu normwise {norm:.3e} relL2 {rl2:.3e} | torch fp32 {fn:.3e} {fl:.3e}")
        record_margin(f"const_raygrad_{what}", norm, GRAD_TOL)
        record_margin(f"const_raygrad_relL2_{what}", rl2, REL_L2["bwd"])
        assert norm <= GRAD_TOL, (name, what, "normwise", norm, "torch fp32", fn)
        assert rl2 <= REL_L2["bwd"], (name, what, "relL2", rl2, "torch fp32", fl)
        check_per_ray(name, what, got, f32, ref)
    assert (g_org[~nz] == 0).all() and (g_dir[~nz] == 0).all()
    got = host(render.render_diff_backward_cameras([c["camera"]], W, W, s, c["k"], dev(c["grad_out"]), c["steps"], **kw))
    assert got.shape == (1, 7) and np.isfinite(got).all()
    check_camera_row(f"{name} camera", got[0].astype(np.float64),
                     rr.camera_grads(c["camera"], W, W, c["scene"], c["k"], c["steps"], c["grad_out"], **kw))


# ---- 3. the finish kernel's segments -------------------------------------------------------------------
FINISH_K, FINISH_STEPS = 32.0, 16


def _finish_camera(i):
    import test_gpu_raygrad as T
    return T.cam(i)


@pytest.mark.parametrize("width,height,bpv", [(72, 64, 18), (128, 33, 17), (64, 64, 16)])
def test_camera_gradient_finish_segments(rm, width, height, bpv):
    """rm_raygrad_finish adds a view's partial rows (one per 256-ray block) in 16 segments of
    len = ceil(bpv / 16) rows: bpv = 18 (len 2, nine segments used), 17 (len 2, the last used segment
    holds one row), 16 (len 1, every segment used). scene.json, 16 steps, against camera_grads."""
    render, _ = rm
    assert (width * height + 255) // 256 == bpv
    sc = final1_scene()
    cm = _finish_camera(1)
    g = np.random.default_rng(width + height).standard_normal((width * height, 3)).astype(np.float32)
    got = host(render.render_diff_backward_cameras([cm], width, height, scene_dev(rm, sc), FINISH_K, dev(g), FINISH_STEPS))
    assert got.shape == (1, 7) and np.isfinite(got).all()
    check_camera_row(f"finish {width}x{height}", got[0].astype(np.float64),
                     rr.camera_grads(cm, width, height, sc, FINISH_K, FINISH_STEPS, g))


def test_camera_gradient_of_130_views_against_autograd(rm):
    """130 views at 8x8 (two calls' worth): views 0, 1, 128 and 129 against camera_grads, not only
    against each other."""
    render, _ = rm
    sc = final1_scene()
    cams = [_finish_camera(1), _finish_camera(3)] * 65
    g = np.random.default_rng(3).standard_normal((130, 64, 3)).astype(np.float32)
    got = host(render.render_diff_backward_cameras(cams, 8, 8, scene_dev(rm, sc), FINISH_K, dev(g.reshape(-1, 3)),
                                                   FINISH_STEPS))
    assert got.shape == (130, 7) and np.isfinite(got).all()
    for v in (0, 1, 128, 129):
        check_camera_row(f"130 views, view {v}", got[v].astype(np.float64),
                         rr.camera_grads(cams[v], 8, 8, sc, FINISH_K, FINISH_STEPS, g[v]))


# ---- 4. bit-level promises off the defaults ------------------------------------------------------------
@pytest.mark.parametrize("name", POLICY)
def test_early_exit_changes_no_bit(rm, name):
    """Image, loss, t_march and every gradient with the escaped-ray exit on and off, array mode and
    camera mode, where gone_d is not the default's 6 (45 at mask_sharpness 2, 15 at 6, 6 at 60)."""
    for camera in (False, True):
        a = run_gpu(rm, name, camera=camera, RM_NO_EARLY_EXIT="1")
        b = run_gpu(rm, name, camera=camera, RM_NO_EARLY_EXIT="0")
        same_bits(a, b, f"{name} camera={camera} exit off/on")
        same_bits({"bwd": b["bwd"]}, {"bwd": b["bwd_t"]}, f"{name} camera={camera} saved t", keys=("bwd",))
        assert np.array_equal(b["out"].view(np.uint32), b["out_fast"].view(np.uint32))


@pytest.mark.parametrize("m", E.SIZES)
def test_mask_sharpness_zero_never_arms_the_exit(rm, m):
    """mask_sharpness = 0: no ray is ever gone (mask 0.5 everywhere), so no wave leaves the march, and
    RM_MARCH_NO_EARLY_EXIT changes no bit."""
    render, _ = rm
    name = f"msharp0-M{m}"
    c = C.case(name)
    kw = C.consts_kw(c["consts"])
    s = scene_dev(rm, c["scene"])
    ctx = render.context()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("RM_NO_EARLY_EXIT", "0")
        ctx.stats(True)
        ctx.collect_stats(reset=True)
        render.render_diff_forward(dev(c["org"]), dev(c["dir"]), s, c["k"], c["steps"], **kw)
        render.render_diff_camera([c["camera"]], W, W, s, c["k"], c["steps"], **kw)
        st = ctx.collect_stats(reset=True)
        ctx.stats(False)
    assert st["waves"] > 0 and st["waves_exited"] == 0 and st["blocks_skipped"] == 0, st
    for camera in (False, True):
        same_bits(run_gpu(rm, name, camera=camera, RM_NO_EARLY_EXIT="1"),
                  run_gpu(rm, name, camera=camera, RM_NO_EARLY_EXIT="0"), f"{name} camera={camera} exit off/on")


@pytest.mark.parametrize("m", E.SIZES)
def test_skip_escaped_at_mask_sharpness_two(rm, m, monkeypatch):
    """RM_MARCH_SKIP_ESCAPED in camera mode at mask_sharpness 2 (cull_min_d = 55.4 instead of 50): the
    image bit for bit, the loss and the gradients equal, as tests/test_gpu_escape.py holds them (==).
    The msharp2 scene at 128x128 and 32 steps, where the conservative escape proof passes whole
    tiles beyond 55.4: blocks are skipped (at the case's 32x32 and 12 steps none is). Both legs on the
    general kernel and unsplit (the flag selects it: rm_launch.h, use_small and march_policy)."""
    import torch
    render, _ = rm
    c = C.case(f"msharp2-M{m}")
    kw = C.consts_kw(c["consts"])
    s = scene_dev(rm, c["scene"])
    cams, size, k, steps = [c["camera"]], 128, c["k"], 32
    monkeypatch.setenv("RM_SPLIT", "0")
    monkeypatch.setenv("RM_SMALL", "0")
    monkeypatch.setenv("RM_SKIP_ESCAPED", "0")
    tg = render.render_diff_camera(cams, size, size, scene_dev(rm, E.synthetic(m, 1000)), k, steps, **kw)
    g = torch.randn((size * size, 3), device="cuda", generator=torch.Generator("cuda").manual_seed(0))
    ctx = render.context()

    def run():
        ctx.stats(True)
        ctx.collect_stats(reset=True)
        out = render.render_diff_camera(cams, size, size, s, k, steps, **kw)
        skipped = ctx.collect_stats(reset=True)["blocks_skipped"]
        ctx.stats(False)
        bwd = render.render_diff_backward_camera(cams, size, size, s, k, g, steps, **kw)
        tout = torch.empty_like(out)
        loss, train, _ = render.train_step_camera(cams, size, size, tg, s, k, E.PROGRESS, steps, out=tout, **kw)
        torch.cuda.synchronize()
        return skipped, host(out), host(tout), host(loss), {q: host(v) for q, v in bwd.items()}, \
            {q: host(v) for q, v in train.items()}

    full = run()
    monkeypatch.setenv("RM_SKIP_ESCAPED", "1")
    skip = run()
    assert full[0] == 0 and skip[0] > 0, (full[0], skip[0])
    assert np.array_equal(full[1].view(np.uint32), skip[1].view(np.uint32))
    assert np.array_equal(full[2].view(np.uint32), skip[2].view(np.uint32))
    assert np.array_equal(full[3], skip[3])
    for a, b in ((full[4], skip[4]), (full[5], skip[5])):
        for q in GRAD_KEYS:
            assert np.isfinite(a[q]).all() and np.array_equal(a[q], b[q]), q


@pytest.mark.parametrize("flag", ("RM_FORCE_MAX_SHIFT", "RM_VALU_ONLY"))
@pytest.mark.parametrize("name", POLICY)
def test_march_variants_match_reference(rm, name, flag):
    small = {"RM_SMALL": "0"} if name.endswith("-M12") else {}  # the flags leave the small-scene kernel
    check(run_gpu(rm, name, **{flag: "1"}, **small), name, f"{name} array {flag}")
    check(run_gpu(rm, name, camera=True, **{flag: "1"}, **small), name, f"{name} camera {flag}")


def test_fused_adam_equals_two_calls_at_all(rm):
    """rm_train_step_camera_adam (M = 48) at the `all` constants: bit for bit rm_train_step_camera ->
    rm_optimizer_step, and not the default constants' result."""
    import torch
    from burn_raymarching_amd import model
    render, native = rm
    c = C.case("all-M48")
    sc, cams, tg = c["scene"], [c["camera"]], dev(c["targets"])
    march = native.march_params(c["steps"], c["k"], *c["consts"])

    def run(fused, march):
        mdl = model.SceneModel.from_activated(sc["centers"], sc["colors"], sc["radius"], sc["light_dir"], sc["ambient"])
        opt = model.Adam(mdl, weight_decay=1e-5, with_penalties=True)
        g, loss, pen = torch.zeros(model.packed_size(48), device="cuda"), torch.zeros(1, device="cuda"), \
            torch.zeros(1, device="cuda")
        for i in range(3):
            if fused:
                opt.train_step_camera(cams, W, W, tg, c["k"], 0.3 + 0.1 * i, 0.02, c["steps"], grads_packed=g, loss=loss,
                                      penalty_out=pen, march=march)
            else:
                render.train_step_camera(cams, W, W, tg, mdl.scene(), c["k"], 0.3 + 0.1 * i, c["steps"], grads_packed=g,
                                         loss=loss, march=march)
                opt.step(g, 0.02, penalty_out=pen)
        torch.cuda.synchronize()
        return [x.clone() for x in (mdl.raw, mdl._act, opt.m, opt.v, g, loss, pen)]

    a, b = run(True, march), run(False, march)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all()), i
    dflt = run(True, native.march_params(c["steps"], c["k"]))
    assert not torch.equal(a[4], dflt[4])


def test_train_iteration_equals_three_calls_at_all(rm, oracle, monkeypatch):
    """rm_train_iteration (M = 12, one launch) at the `all` constants: bit for bit rm_sample_batch ->
    rm_train_step -> rm_optimizer_step, and not the default constants' result."""
    import torch
    import test_gpu_small as S
    from burn_raymarching_amd import model
    render, native = rm
    c = C.case("all-M12")
    kw = C.consts_kw(c["consts"])
    rays = [oracle.camera_rays(64, 64, *cm, precision="f32") for cm in model.ring_cameras(4)]
    o = np.concatenate([r[0] for r in rays])
    d = np.concatenate([r[1] for r in rays])
    tg = oracle.render_diff(o.astype(np.float64), d.astype(np.float64), E.synthetic(12, 1000), 24, 32.0, **kw)
    src = [dev(o), dev(d), dev(tg)]
    fg = torch.from_numpy(np.flatnonzero(tg.sum(1) > 0.01).astype(np.int32)).cuda()
    assert fg.numel() > 100
    args = (torch, native, render, model, src, fg, 13107, 3277, c["scene"], 3)
    a = S._iteration(*args, True, monkeypatch, march_kw=kw)
    b = S._iteration(*args, False, monkeypatch, march_kw=kw)
    for it, (xa, xb) in enumerate(zip(a, b)):
        for what, u, v in zip(("raw", "act", "grad", "adam_m", "adam_v", "loss"), xa, xb):
            assert torch.equal(u, v), (it, what, (u - v).abs().max().item())
    assert torch.isfinite(a[-1][0]).all() and a[-1][5][0] > 0
    dflt = S._iteration(*args, True, monkeypatch)
    assert not torch.equal(a[0][2], dflt[0][2])


# ---- 5. nothing written outside the buffers ------------------------------------------------------------
@pytest.mark.parametrize("name", C.names() + C.LIMIT_NAMES)
def test_nothing_written_outside_the_buffers(rm, name):
    """The C ABI calls on slices of one arena filled with GUARD, 64 guard words around each of out,
    t_march, the five gradient buffers, the loss, the ray gradients and the camera gradient: the guard
    words keep their value, and the results are the Python layer's bit for bit."""
    import torch
    render, native = rm
    c = C.case(name)
    m, n = c["M"], len(c["org"])
    sizes = {"out": 3 * n, "t": n, "centers": 3 * m, "colors": 3 * m, "radius": m, "light_dir": 3, "ambient": 1, "loss": 1,
             "g_org": 3 * n, "g_dir": 3 * n, "g_cam": 7}
    off, total = {}, 64
    for key, size in sizes.items():
        off[key] = total
        total += (size + 63) // 64 * 64 + 64
    ctx = render.context()
    s = scene_dev(rm, c["scene"])
    o, d, g, tg = dev(c["org"]), dev(c["dir"]), dev(c["grad_out"]), dev(c["targets"])
    march = s.march_for(native.march_params(c["steps"], c["k"], *c["consts"]))
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    ref = run_gpu(rm, name)

    def arena_call(call, written):
        arena = torch.full((total,), G.GUARD, device="cuda")
        buf = {key: arena[off[key]:off[key] + sizes[key]] for key in sizes}
        cg = native.RmGrads(*(buf[q].data_ptr() for q in GRAD_KEYS))
        call(buf, cg)
        torch.cuda.synchronize()
        used = torch.zeros(total, dtype=torch.bool, device="cuda")
        for key in written:
            used[off[key]:off[key] + sizes[key]] = True
        assert bool((arena[~used] == G.GUARD).all()), f"{name}: a write outside {written}"
        return {key: host(buf[key]).copy() for key in written}

    sc_ref, m_ref = ctypes.byref(s.c_struct()), ctypes.byref(march)
    got = arena_call(lambda b, cg: ctx.check(ctx._lib.rm_render_diff(ctx.handle, p(o), p(d), n, sc_ref, m_ref,
                                                                      p(b["out"]), p(b["t"])), "rm_render_diff"),
                     ("out", "t"))
    assert np.array_equal(got["out"], ref["out"].ravel()) and np.array_equal(got["t"], ref["t"])
    got = arena_call(lambda b, cg: ctx.check(ctx._lib.rm_render_diff_backward(
        ctx.handle, p(o), p(d), n, sc_ref, m_ref, p(g), None, ctypes.byref(cg), 0), "rm_render_diff_backward"), GRAD_KEYS)
    for q in GRAD_KEYS:
        assert np.array_equal(got[q], ref["bwd"][q].ravel()), q

    def train(b, cg):
        b["loss"].zero_()
        ctx.check(ctx._lib.rm_train_step(ctx.handle, p(o), p(d), p(tg), n, float(E.PROGRESS), 1.0 / (3.0 * n), sc_ref,
                                         m_ref, ctypes.byref(cg), p(b["loss"]), p(b["out"]), 0), "rm_train_step")
    got = arena_call(train, GRAD_KEYS + ("loss", "out"))
    assert np.array_equal(got["out"], ref["train_out"].ravel()) and np.float32(got["loss"][0]) == np.float32(ref["loss"])
    for q in GRAD_KEYS:
        assert np.array_equal(got[q], ref["train"][q].ravel()), q
    got = arena_call(lambda b, cg: ctx.check(ctx._lib.rm_render_diff_backward_rays(
        ctx.handle, p(o), p(d), n, sc_ref, m_ref, p(g), None, p(b["g_org"]), p(b["g_dir"]), 0),
        "rm_render_diff_backward_rays"), ("g_org", "g_dir"))
    assert np.isfinite(got["g_org"]).all() and np.isfinite(got["g_dir"]).all()
    got = arena_call(lambda b, cg: ctx.check(ctx._lib.rm_render_diff_backward_cameras(
        ctx.handle, native.cameras([c["camera"]]), 1, W, W, sc_ref, m_ref, p(g), None, p(b["g_cam"]), 0),
        "rm_render_diff_backward_cameras"), ("g_cam",))
    assert np.isfinite(got["g_cam"]).all()


# ---- 6. accepted ranges ---------------------------------------------------------------------------------
RM_ERR_INVALID_ARG = 1  # include/raymarch.h
BAD = [("normal_eps", v) for v in (float("nan"), float("inf"), 0.0, -1e-4)] + \
      [(f, v) for f in ("color_sharpness", "mask_sharpness") for v in (float("nan"), float("inf"), -float("inf"), -1.0)]


def test_constants_out_of_range_are_rejected(rm):
    """check_march: RM_ERR_INVALID_ARG with the field's name in rm_last_error for a non-finite value of
    any of the three constants, normal_eps <= 0 and a negative sharpness, on the forward, the train
    step and the ray-gradient entry points (nothing is launched: the outputs keep their value); zero
    is valid for both sharpnesses."""
    import torch
    render, native = rm
    c = C.case("all-M12")
    n = len(c["org"])
    s = scene_dev(rm, c["scene"])
    o, d, g, tg = dev(c["org"]), dev(c["dir"]), dev(c["grad_out"]), dev(c["targets"])
    ctx = render.context()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    sc_ref = ctypes.byref(s.c_struct())
    out = torch.full((n, 3), G.GUARD, device="cuda")
    loss = torch.zeros(1, device="cuda")
    grads, cg = render._grads_like(s)

    def calls(march):
        m_ref = ctypes.byref(march)
        yield "rm_render_diff", ctx._lib.rm_render_diff(ctx.handle, p(o), p(d), n, sc_ref, m_ref, p(out), None)
        yield "rm_train_step", ctx._lib.rm_train_step(ctx.handle, p(o), p(d), p(tg), n, 0.3, 1.0 / (3.0 * n), sc_ref, m_ref,
                                                      ctypes.byref(cg), p(loss), None, 0)
        yield "rm_render_diff_backward_rays", ctx._lib.rm_render_diff_backward_rays(
            ctx.handle, p(o), p(d), n, sc_ref, m_ref, p(g), None, p(out), None, 0)
        yield "rm_render_diff_camera", ctx._lib.rm_render_diff_camera(ctx.handle, native.cameras([c["camera"]]), 1, W, W,
                                                                      sc_ref, m_ref, p(out), None)

    for field, value in BAD:
        march = native.march_params(c["steps"], c["k"], **{field: value})
        for what, rc in calls(march):
            msg = ctx._lib.rm_last_error(ctx.handle)
            assert rc == RM_ERR_INVALID_ARG and field.encode() in msg, (what, field, value, rc, msg)
    torch.cuda.synchronize()
    assert bool((out == G.GUARD).all())
    for field in ("color_sharpness", "mask_sharpness"):
        march = native.march_params(c["steps"], c["k"], **{field: 0.0})
        for what, rc in calls(march):
            assert rc == native.RM_OK, (what, field, ctx._lib.rm_last_error(ctx.handle))
    with pytest.raises(native.RaymarchError, match="mask_sharpness"):
        render.train_step(o, d, tg, s, c["k"], 0.3, c["steps"], mask_sharpness=-2.0)
