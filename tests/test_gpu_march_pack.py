"""Packed march steps of the unsplit general kernel: a ray whose t repeats under
the same shift form takes the D it computed one or two steps back, and only the live rays of a
wave -- not gone, not known -- are summed on the matrix cores, packed into ceil(live / 16) column
blocks. Both are exact: with the exit on and off (RM_MARCH_NO_EARLY_EXIT / env RM_NO_EARLY_EXIT=1:
no ray is known, every block is multiplied) the image, t_march, the loss and every gradient are
equal (==). RM_SPLIT=0 keeps every case on the unsplit kernel (M > 32: the general kernel)."""
import numpy as np
import pytest

from conftest import check_grads, gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

SIZE = 64


@pytest.fixture(scope="module")
def mods():
    import torch
    from burn_raymarching_amd import model, native, render
    torch.cuda.init()
    return torch, model, native, render


def _both(monkeypatch, fn):
    monkeypatch.setenv("RM_SPLIT", "0")
    monkeypatch.setenv("RM_NO_EARLY_EXIT", "1")
    full = fn()
    monkeypatch.setenv("RM_NO_EARLY_EXIT", "0")
    fast = fn()
    return full, fast


def _assert_equal(torch, full, fast):
    for name in full:
        assert torch.isfinite(fast[name]).all(), name
        assert torch.equal(full[name], fast[name]), name


def _camera_step(mods, cams, sc, tgt, k, steps):
    """Image, t_march, loss and the packed gradient of one camera-mode train step."""
    torch, model, native, render = mods
    out = torch.empty_like(tgt)
    gp = torch.zeros(model.packed_size(sc.num_spheres), device="cuda")
    loss, _, _ = render.train_step_camera(cams, SIZE, SIZE, tgt, sc, k, 0.3, steps, out=out, grads_packed=gp)
    _, t = render.render_diff_camera(cams, SIZE, SIZE, sc, k, steps, return_t=True)
    torch.cuda.synchronize()
    return {"out": out, "t_march": t, "loss": loss.clone(), "grads": gp}


def _ray_step(mods, o, d, sc, tgt, k, steps):
    """The same of one array-mode train step (the gradient groups packed in their order)."""
    torch, model, native, render = mods
    loss, g, out = render.train_step(o, d, tgt, sc, k, 0.3, steps, with_out=True)
    _, t = render.render_diff_forward(o, d, sc, k, steps, return_t=True)
    torch.cuda.synchronize()
    gp = torch.cat([g[key].reshape(-1) for key in ("centers", "colors", "radius", "light_dir", "ambient")])
    return {"out": out, "t_march": t, "loss": loss.clone(), "grads": gp}


def _target(mods, cams, m, steps):
    torch, model, native, render = mods
    return render.render_diff_camera(cams, SIZE, SIZE, model.scene_tensors(model.synthetic_scene(m, 4), "cuda"),
                                     32.0, steps)


def _one_sphere_scene(model):
    """One sphere of radius 1 at the origin and 39 small ones inside it."""
    sc = model.synthetic_scene(40, 0)
    sc["centers"][0] = 0.0
    sc["radius"][0] = 1.0
    return sc


# the eye inside the cone the big sphere fills: asin(1 / 1.6) = 38.7 deg > the 33.4 deg of the image corners
ONE_SPHERE_CAM = [([0.0, 0.0, -1.6], [0.0, 0.0, 0.0], 50.0)]


@pytest.mark.parametrize("m", [40, 256])
@pytest.mark.parametrize("k", [32.0, 5.0])
def test_camera_partial_waves(mods, monkeypatch, m, k):
    """Silhouettes cross the 8x8 wave tiles: waves hold live, known and gone rays together."""
    torch, model, native, render = mods
    sc = model.scene_tensors(model.synthetic_scene(m, 0), "cuda")
    cams = model.ring_cameras(10)[:2]
    tgt = _target(mods, cams, m, 32)
    full, fast = _both(monkeypatch, lambda: _camera_step(mods, cams, sc, tgt, k, 32))
    _assert_equal(torch, full, fast)


def test_one_sphere_fills_the_view(mods, monkeypatch):
    """No ray escapes and the rays converge at different steps: 1 to 3 live blocks for many steps."""
    torch, model, native, render = mods
    sc = model.scene_tensors(_one_sphere_scene(model), "cuda")
    tgt = _target(mods, ONE_SPHERE_CAM, 40, 64)
    full, fast = _both(monkeypatch, lambda: _camera_step(mods, ONE_SPHERE_CAM, sc, tgt, 32.0, 64))
    _assert_equal(torch, full, fast)
    assert float(fast["out"].abs().max()) > 0.0


@pytest.fixture(scope="module")
def shuffled_view(mods):
    """The rays of one 64x64 view in a seeded random order, and targets for them."""
    torch, model, native, render = mods
    cam = model.ring_cameras(10)[1]
    o, d = render.create_camera_rays(SIZE, SIZE, *cam)
    perm = torch.from_numpy(np.random.default_rng(5).permutation(SIZE * SIZE)).cuda()
    tgt = _target(mods, [cam], 40, 32)
    return o[perm].contiguous(), d[perm].contiguous(), tgt[perm].contiguous()


@pytest.mark.parametrize("n", [1, 257, 1000])
def test_array_mode_arbitrary_slots(mods, monkeypatch, shuffled_view, n):
    """Live and done lanes interleave, so the slot permutation is arbitrary; invalid lanes and one
    ragged wave."""
    torch, model, native, render = mods
    o, d, tgt = (x[:n].contiguous() for x in shuffled_view)
    sc = model.scene_tensors(model.synthetic_scene(40, 0), "cuda")
    full, fast = _both(monkeypatch, lambda: _ray_step(mods, o, d, sc, tgt, 32.0, 32))
    _assert_equal(torch, full, fast)


def _wave_rays(mods):
    """64 directions of a ring view (an 8x8 grid over the image: hits and misses) from its eye."""
    torch, model, native, render = mods
    cam = model.ring_cameras(10)[2]
    o, d = render.create_camera_rays(SIZE, SIZE, *cam)
    px = torch.arange(4, SIZE, 8, device="cuda")
    idx = (px[:, None] * SIZE + px[None]).reshape(-1)
    return o[idx].contiguous(), d[idx].contiguous()


@pytest.mark.parametrize("k", [32.0, 5.0])
def test_form_change_after_rays_settled(mods, monkeypatch, k):
    """One wave: rays that start 0.3 from the scene's bounding sphere next to rays that start 12
    away along the same directions. The far rays' large steps hold the wave in the fixed form
    while the near rays already repeat; the form moves to unshifted once they arrive."""
    torch, model, native, render = mods
    eye, d = _wave_rays(mods)
    sc_np = model.synthetic_scene(40, 0)
    reach = float((np.linalg.norm(sc_np["centers"], axis=1) + sc_np["radius"]).max())  # about the origin
    near = float(np.linalg.norm(np.asarray(model.ring_cameras(10)[2][0]))) - reach - 0.3
    half = torch.arange(64, device="cuda") % 2 == 0
    start = torch.where(half, torch.tensor(near, device="cuda"), torch.tensor(near - 12.0, device="cuda"))
    o = (eye + d * start[:, None]).contiguous()
    sc = model.scene_tensors(sc_np, "cuda")
    tgt = torch.full_like(o, 0.25)
    full, fast = _both(monkeypatch, lambda: _ray_step(mods, o, d, sc, tgt, k, 48))
    _assert_equal(torch, full, fast)


def test_vector_path_ray(mods, monkeypatch):
    """One ray's origin at |o| = 2e5 in an otherwise near wave: the wave takes the running-max
    vector step (|p|^2 > 1e10), on which no step is memoised."""
    torch, model, native, render = mods
    eye, d = _wave_rays(mods)
    o = eye.clone()
    o[5] = -2e5 * d[5]  # looks at the scene's centre from far out
    sc = model.scene_tensors(model.synthetic_scene(40, 0), "cuda")
    tgt = torch.full_like(o, 0.25)
    full, fast = _both(monkeypatch, lambda: _ray_step(mods, o, d, sc, tgt, 32.0, 32))
    _assert_equal(torch, full, fast)


def test_parity_with_oracle(mods, oracle, monkeypatch):
    torch, model, native, render = mods
    monkeypatch.setenv("RM_SPLIT", "0")
    sc_np = model.synthetic_scene(40, 0)
    cam = model.ring_cameras(10)[0]
    o, d = oracle.camera_rays(SIZE, SIZE, *cam, precision="f32")
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    targets = oracle.render_diff(o64, d64, model.synthetic_scene(40, 4), 32, 32.0, precision="f64")
    tgt = torch.from_numpy(np.ascontiguousarray(targets, np.float32)).cuda()
    loss, g, _ = render.train_step_camera([cam], SIZE, SIZE, tgt, model.scene_tensors(sc_np, "cuda"), 32.0, 0.5, 32)
    _, loss_ref, g_ref = oracle.train_step(o64, d64, targets, sc_np, 32, 32.0, 0.5)
    got = float(loss.cpu().numpy()[0])
    assert abs(got - loss_ref) <= 1e-4 * abs(loss_ref), (got, loss_ref)
    check_grads(g, g_ref, mode="train")


def test_two_calls_same_bits(mods, monkeypatch):
    torch, model, native, render = mods
    monkeypatch.setenv("RM_SPLIT", "0")
    sc = model.scene_tensors(model.synthetic_scene(40, 0), "cuda")
    cams = model.ring_cameras(10)[:2]
    tgt = _target(mods, cams, 40, 32)
    a = _camera_step(mods, cams, sc, tgt, 32.0, 32)
    b = _camera_step(mods, cams, sc, tgt, 32.0, 32)
    _assert_equal(torch, a, b)


def test_skipped_blocks_are_booked(mods, monkeypatch):
    """The one-sphere case's steps_saved exceeds what its waves skip as whole waves -- the shared
    origin step of every wave and the rest of the march of every wave that escaped: column blocks
    were skipped and booked (floor(blocks / 4) steps per wave). No wave escapes here, so the
    whole-wave figure is one step per wave; the steps a wave's cycle exit saves are whole-wave
    steps too, but the counters do not separate them from the booked blocks."""
    torch, model, native, render = mods
    monkeypatch.setenv("RM_SPLIT", "0")
    monkeypatch.setenv("RM_NO_EARLY_EXIT", "0")
    steps = 64
    sc = model.scene_tensors(_one_sphere_scene(model), "cuda")
    tgt = _target(mods, ONE_SPHERE_CAM, 40, steps)
    ctx = render.context()
    ctx.stats(True)
    ctx.collect_stats(reset=True)
    render.train_step_camera(ONE_SPHERE_CAM, SIZE, SIZE, tgt, sc, 32.0, 0.3, steps)
    st = ctx.collect_stats(reset=True)
    ctx.stats(False)
    assert st["waves"] == SIZE * SIZE // 64
    whole_waves = st["waves"] + st["waves_exited"] * (steps - 1)
    print("steps_saved", st["steps_saved"], "whole waves", whole_waves, st)
    assert st["steps_saved"] > whole_waves
    assert st["steps_saved"] <= st["waves"] * steps
