"""The lower-bound escape proof of the unsplit march (bound_proof in rm_ray.h): a
wave whose rays all provably end gone stops before it marches. Exact: forward, backward and the
train step are equal (==) with the exit on and off and stay inside the oracle bounds of
test_gpu_parity.py; the rm_stats counters show which waves the proof took. The general kernel
runs every case unsplit, the proof's scope (RM_SMALL=0: calls at M = 48 would otherwise take the
small-scene kernel; RM_SPLIT=0: calls this small at M = 300 would otherwise take the split march)."""
import ctypes

import numpy as np
import pytest

from conftest import check_grads, gpu_available
from test_gpu_parity import check_fwd

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

S = 32


@pytest.fixture(scope="module")
def mods():
    import torch
    from burn_raymarching_amd import model, native, render
    torch.cuda.init()
    return torch, model, render, native


@pytest.fixture(autouse=True)
def general_kernel(monkeypatch):
    monkeypatch.setenv("RM_SMALL", "0")
    monkeypatch.setenv("RM_SPLIT", "0")


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def _both(monkeypatch, fn):
    monkeypatch.setenv("RM_NO_EARLY_EXIT", "1")
    full = fn()
    monkeypatch.setenv("RM_NO_EARLY_EXIT", "0")
    fast = fn()
    return full, fast


def _stats(render, fn):
    ctx = render.context()
    ctx.stats(True)
    ctx.collect_stats(reset=True)
    fn()
    st = ctx.collect_stats(reset=True)
    ctx.stats(False)
    return st


def _equal(torch, a, b):
    if isinstance(a, dict):
        for key in a:
            assert torch.equal(a[key], b[key]), key
    else:
        assert torch.equal(a, b)


@pytest.fixture(scope="module")
def references(oracle):
    """fp64 oracle results per (w, h, m, k), computed once: rays, image, backward and train step"""
    cache = {}

    def get(model, w, h, m, k):
        key = (w, h, m, k)
        if key not in cache:
            sc = model.synthetic_scene(m, 21)
            cam = model.ring_cameras(10)[3]
            o, d = oracle.camera_rays(w, h, *cam, precision="f32")
            o64, d64 = o.astype(np.float64), d.astype(np.float64)
            g = np.random.default_rng(5).normal(size=o.shape).astype(np.float32)
            tgt = oracle.render_diff(o64, d64, model.synthetic_scene(m, 22), S, 32.0, precision="f64")
            cache[key] = dict(sc=sc, cam=cam, o=o, d=d, g=g, tgt=tgt.astype(np.float32),
                              img=oracle.render_diff(o64, d64, sc, S, k, precision="f64"),
                              bwd=oracle.render_diff_backward(o64, d64, sc, S, k, g.astype(np.float64),
                                                              precision="f64"),
                              train=oracle.train_step(o64, d64, tgt.astype(np.float32).astype(np.float64), sc, S, k, 0.5))
        return cache[key]
    return get


@pytest.mark.parametrize("camera", [True, False], ids=["camera", "array"])
@pytest.mark.parametrize("k", [32.0, 5.0])
@pytest.mark.parametrize("m", [48, 300])  # 48: below kProofMinSpheres = 128, the march as it was; 300: with the proof
@pytest.mark.parametrize("w,h", [(64, 64), (48, 80)])
def test_exit_on_off_equal_and_inside_oracle_bounds(mods, references, monkeypatch, w, h, m, k, camera):
    torch, model, render, _ = mods
    ref = references(model, w, h, m, k)
    sc = model.scene_tensors(ref["sc"], "cuda")
    cams = [ref["cam"]]
    o, d, g, tgt = dev(ref["o"]), dev(ref["d"]), dev(ref["g"]), dev(ref["tgt"])

    def fwd():
        return (render.render_diff_camera(cams, w, h, sc, k, S) if camera
                else render.render_diff_forward(o, d, sc, k, S)).clone()

    def bwd():
        r = (render.render_diff_backward_camera(cams, w, h, sc, k, g, S) if camera
             else render.render_diff_backward(o, d, sc, k, g, S))
        return {key: v.clone() for key, v in r.items()}

    def train():
        if camera:
            out = torch.empty_like(tgt)
            loss, gr, _ = render.train_step_camera(cams, w, h, tgt, sc, k, 0.5, S, out=out)
        else:
            loss, gr, out = render.train_step(o, d, tgt, sc, k, 0.5, S, with_out=True)
        torch.cuda.synchronize()
        return dict(loss=loss.clone(), out=out.clone(), **{key: v.clone() for key, v in gr.items()})

    for fn in (fwd, bwd, train):
        full, fast = _both(monkeypatch, fn)
        _equal(torch, full, fast)
    # backward from the saved t (no march): the same gradients with the exit on and off
    _, t = render.render_diff_forward(o, d, sc, k, S, return_t=True)
    full, fast = _both(monkeypatch, lambda: {key: v.clone() for key, v in
                                             render.render_diff_backward(o, d, sc, k, g, S, t_march=t).items()})
    _equal(torch, full, fast)
    # the exit-on results against the fp64 oracle, bounds of test_gpu_parity.py
    check_fwd(fwd().cpu().numpy(), ref["img"])
    check_grads(bwd(), ref["bwd"])
    out_ref, loss_ref, g_ref = ref["train"]
    tr = train()
    check_fwd(tr["out"].cpu().numpy(), out_ref)
    assert abs(float(tr["loss"].reshape(-1)[0]) - loss_ref) <= 1e-4 * abs(loss_ref) + 1e-3
    check_grads({key: tr[key] for key in g_ref}, g_ref, mode="train")


@pytest.mark.parametrize("m", [48, 128, 300])
def test_ragged_last_block_exit_on_off_equal(mods, references, monkeypatch, m):
    """Array mode with a ray count that leaves lanes past the last ray in the last block and wave.
    M = 128 is the first size at which the proof runs (kProofMinSpheres)."""
    torch, model, render, _ = mods
    ref = references(model, 48, 80, m, 32.0)
    sc = model.scene_tensors(ref["sc"], "cuda")
    n = 48 * 80 - 37
    o, d, tgt = dev(ref["o"][:n]), dev(ref["d"][:n]), dev(ref["tgt"][:n])

    def train():
        loss, gr, out = render.train_step(o, d, tgt, sc, 32.0, 0.5, S, with_out=True)
        torch.cuda.synchronize()
        return dict(loss=loss.clone(), out=out.clone(), **{key: v.clone() for key, v in gr.items()})

    full, fast = _both(monkeypatch, train)
    _equal(torch, full, fast)
    assert _stats(render, train)["waves_exited"] > 0


def _view(oracle, w, h, eye, target, fov):
    return oracle.camera_rays(w, h, np.float32(eye), np.float32(target), fov, precision="f32")


@pytest.mark.parametrize("camera", [True, False], ids=["camera", "array"])
# the proof runs from 128 spheres on: 'away' holds at every size (the march's own receding test), 'beside' needs it
@pytest.mark.parametrize("view,m", [("away", 48), ("away", 300), ("beside", 128), ("beside", 300)])
def test_rays_that_miss_the_scene_run_no_march_step(mods, oracle, monkeypatch, m, camera, view):
    """Every ray misses the scene's soft ball. away: the view looks away from the scene. beside: it
    looks past the scene, the rays approach it first (the receding test of the march itself holds
    only after the closest approach; the bound march proves them before the first step). No wave
    runs a march step: every step of every wave is booked as saved (camera mode: the shared origin
    step too, which no wave runs) and every wave exits. The exit-off run gives the same bits."""
    torch, model, render, _ = mods
    monkeypatch.setenv("RM_NO_EARLY_EXIT", "0")
    sc = model.scene_tensors(model.synthetic_scene(m, 3), "cuda")  # centres within 0.6 of the origin, r <= 0.12
    w, h = 48, 80
    eye = [0.0, 0.5, 2.5]
    cam = (eye, [0.0, 1.0, 5.0], 50.0) if view == "away" else (eye, [2.2, 0.5, 0.0], 20.0)
    o, d = _view(oracle, w, h, *cam)
    tgt = torch.full((w * h, 3), 0.25, device="cuda")

    def train():
        if camera:
            out = torch.empty_like(tgt)
            loss, g, _ = render.train_step_camera([cam], w, h, tgt, sc, 32.0, 0.5, S, out=out)
        else:
            loss, g, out = render.train_step(dev(o), dev(d), tgt, sc, 32.0, 0.5, S, with_out=True)
        torch.cuda.synchronize()
        return loss, g, out

    st = _stats(render, train)
    waves = w * h // 64
    assert st["waves"] == waves
    assert st["waves_exited"] == waves
    assert st["steps_saved"] == waves * S  # executed march steps: waves * S - steps_saved == 0
    loss, g, out = train()
    assert float(out.abs().max()) == 0.0
    for key in ("centers", "colors", "radius"):
        assert float(g[key].abs().max()) == 0.0, key
    monkeypatch.setenv("RM_NO_EARLY_EXIT", "1")
    loss_off, g_off, out_off = train()
    assert torch.equal(loss, loss_off) and torch.equal(out, out_off)
    _equal(torch, g, g_off)


def test_far_origins_in_a_wave_keep_it_marching(mods, oracle, monkeypatch):
    """Array mode, rays of the 'beside' view (every wave provable) with two lanes of every wave moved
    to an origin 300 away, past the magnitude the proof's fp32 margins cover (B <= 256): one
    recedes, one heads for the scene. The guard is a wave vote, so no such wave is taken by the
    proof: no wave exits (each holds a ray that hits the scene, whose output is not 0), the untouched
    control is taken whole, and the train step is equal (==) exit on and off."""
    torch, model, render, _ = mods
    sc = model.scene_tensors(model.synthetic_scene(300, 3), "cuda")
    w, h = 48, 80
    o, d = _view(oracle, w, h, [0.0, 0.5, 2.5], [2.2, 0.5, 0.0], 20.0)
    o, d = o.copy(), d.copy()
    control_o, control_d = dev(o), dev(d)
    for lane, dirn in ((5, 1.0), (40, -1.0)):
        far = np.float32([300.0, 0.5, 2.5])
        o[lane::64] = far
        d[lane::64] = np.float32([1.0, 0.0, 0.0]) if dirn > 0 else -far / np.linalg.norm(far)
    O, D = dev(o), dev(d)
    waves = w * h // 64
    monkeypatch.setenv("RM_NO_EARLY_EXIT", "0")
    st_control = _stats(render, lambda: render.render_diff_forward(control_o, control_d, sc, 32.0, S))
    assert (st_control["waves_exited"], st_control["steps_saved"]) == (waves, waves * S)
    st = _stats(render, lambda: render.render_diff_forward(O, D, sc, 32.0, S))
    # lane 40 of every wave heads for the scene's centre and hits it: no wave may end early, and
    # the rays that pass beside the scene stay exactly 0
    assert st["waves"] == waves and st["waves_exited"] == 0
    assert st["steps_saved"] < waves * S
    out = render.render_diff_forward(O, D, sc, 32.0, S)
    hit = torch.zeros(w * h, dtype=torch.bool, device="cuda")
    hit[40::64] = True
    assert bool((out[hit].abs().amax(1) > 0).all()) and float(out[~hit].abs().max()) == 0.0
    tgt = torch.full((w * h, 3), 0.25, device="cuda")

    def train():
        loss, gr, out = render.train_step(O, D, tgt, sc, 32.0, 0.5, S, with_out=True)
        torch.cuda.synchronize()
        return dict(loss=loss.clone(), out=out.clone(), **{key: v.clone() for key, v in gr.items()})

    full, fast = _both(monkeypatch, train)
    assert all(torch.isfinite(v).all() for v in fast.values())
    _equal(torch, full, fast)


def test_view_from_inside_the_cloud_proves_nothing(mods, oracle, monkeypatch):
    """From inside the cloud no bound step is positive: the counters equal those of the same forward
    with the proof's conditions false (the diagnostics call: exit on, per-ray debug output)."""
    torch, model, render, native = mods
    monkeypatch.setenv("RM_NO_EARLY_EXIT", "0")
    sc = model.scene_tensors(model.synthetic_scene(300, 3), "cuda")
    o, d = _view(oracle, 48, 80, [0.05, 0.0, -0.1], [1.0, 0.3, 0.2], 70.0)
    O, D = dev(o), dev(d)
    st = _stats(render, lambda: render.render_diff_forward(O, D, sc, 32.0, S))

    def debug_call():
        ctx = render.context()
        dbg = torch.zeros((o.shape[0], 24), device="cuda")
        mp = sc.march_for(native.march_params(S, 32.0))
        ctx.check(ctx._lib.rm_debug_intermediates(ctx.handle, ctypes.c_void_p(O.data_ptr()), ctypes.c_void_p(D.data_ptr()),
                                                  o.shape[0], ctypes.byref(sc.c_struct()), ctypes.byref(mp),
                                                  ctypes.c_void_p(dbg.data_ptr())), "rm_debug_intermediates")
        torch.cuda.synchronize()

    st_off = _stats(render, debug_call)
    assert st["waves"] == st_off["waves"] == 48 * 80 // 64
    assert (st["waves_exited"], st["steps_saved"]) == (st_off["waves_exited"], st_off["steps_saved"])
    assert st["steps_saved"] < st["waves"] * S
