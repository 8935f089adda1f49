"""GPU tests of the viewer's frame render (rm_view, render.view, `rm_train view`) against the fp64
numpy restatement (tests/view_ref.py), at the smallest shapes that can still go wrong: frames ragged
in both tile dimensions, M = 1, odd pair padding (33), several record chunks (300), two blocks of the
record kernel (520), several frames per call and more frames than one launch carries.

Parity. The bound is the project's forward bound: on the pixels where the GPU and
fp64 agree on hit/miss, linear RGB max <= 1e-3 and mean <= 1e-5, depth within 1e-4. A pixel that
disagrees on hit/miss or exceeds the colour bound is excluded (a hit test that falls one iteration
apart) and counted: at most 0.5 % of a frame's pixels. The fp32 run of the restatement itself stays
at zero such pixels (tests/test_view_reference.py). Every figure is printed and recorded
(conftest.record_margin); profiles/r11_view_parity.txt holds a run's figures."""
import math
import os
import subprocess

import numpy as np
import pytest

import view_ref as V
from conftest import GOLDEN, gpu_available, record_margin

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

SCENE_JSON = os.path.join(GOLDEN, "scene.json")
GOLD = V.golden_scene(SCENE_JSON)
ONE = dict(centers=np.array([[0.1, -0.05, 0.0]], np.float32), colors=np.array([[0.8, 0.3, 0.2]], np.float32),
           radius=np.array([0.45], np.float32), light_dir=GOLD["light_dir"], ambient=GOLD["ambient"])
AWAY = ((0.0, 0.0, -2.5), -math.pi / 2, 0.0)              # looks away: every pixel misses
INSIDE = (tuple(float(x) for x in GOLD["centers"][0]), 1.0, 0.2)  # inside sphere 0: hit at t = 0
FAR = ((0.0, 0.0, -6.0), math.pi / 2, 0.0)                # 6 units out: the reference viewer is black here

# (name, scene, width, height, poses): the issue's cases, then M = 1, the 70x45 three-pose call and M = 520
CASES = V.parity_cases(GOLD) + [("one_sphere_40x24", ONE, 40, 24, [V.POSES[0], V.POSES[1]]),
                                ("golden_70x45_special", GOLD, 70, 45, [AWAY, INSIDE, FAR, V.POSES[2]]),
                                # 272 pairs: two blocks of the record kernel (partial headers in the record buffer)
                                ("synth_M520_32x24", V.synthetic_scene(520, 5), 32, 24, [V.POSES[1]])]
RGB_MAX, RGB_MEAN, DEPTH_TOL, EXCLUDED_CAP = 1e-3, 1e-5, 1e-4, 0.005


@pytest.fixture(scope="module")
def rm():
    import torch
    from burn_raymarching_amd import _build
    _build.build_lib()
    from burn_raymarching_amd import native, render
    torch.cuda.init()
    return render, native


def scene_t(sc, half=False):
    import torch
    from burn_raymarching_amd.render import Scene
    t = {k: torch.from_numpy(np.ascontiguousarray(sc[k], np.float32)).cuda() for k in sc}
    return Scene(t["centers"], t["colors"].half() if half else t["colors"], t["radius"], t["light_dir"], t["ambient"])


def cams_of(poses):
    return [V.view_camera(*p) for p in poses]


def all_outputs(render, poses, w, h, sc, **kw):
    rgb, px, dp = render.view(cams_of(poses), w, h, sc, rgba8=True, depth=True, **kw)
    return rgb.cpu().numpy(), px.cpu().numpy(), dp.cpu().numpy()


_REF = {}


def reference(name, scene, w, h, pose):
    key = (name, pose)
    if key not in _REF:
        _REF[key] = V.view(V.view_camera(*pose), w, h, scene)
    return _REF[key]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_parity_against_fp64(rm, case):
    render, _ = rm
    name, scene, w, h, poses = case
    rgb, _, depth = all_outputs(render, poses, w, h, scene_t(scene))
    for f, pose in enumerate(poses):
        ref_rgb, ref_depth = reference(name, scene, w, h, pose)
        fig = V.compare(rgb[f], depth[f], ref_rgb, ref_depth, RGB_MAX)
        excluded = fig["flips"] + fig["over"]
        print(f"view parity {name} pose {f}: {fig}")
        record_margin(f"view_excluded_{name}_{f}", excluded, EXCLUDED_CAP * fig["pixels"])
        record_margin(f"view_rgb_mean_{name}_{f}", fig["rgb_mean"], RGB_MEAN)
        record_margin(f"view_depth_{name}_{f}", fig["depth_max"], DEPTH_TOL)
        assert excluded <= EXCLUDED_CAP * fig["pixels"], (name, f, fig)
        assert fig["rgb_max"] <= RGB_MAX and fig["rgb_mean"] <= RGB_MEAN, (name, f, fig)
        assert fig["depth_max"] <= DEPTH_TOL, (name, f, fig)
        assert fig["miss_exact"], (name, f)
        miss = ~np.isfinite(depth[f])
        assert (depth[f][miss] == np.inf).all() and not np.isnan(rgb[f]).any()


def test_special_poses(rm):
    """Looking away: exact zeros / +inf everywhere. Inside a sphere: every ray hits at t = 0. Six
    units out: the scene is still there (the shifted soft-min)."""
    render, _ = rm
    rgb, px, depth = all_outputs(render, [AWAY, INSIDE, FAR], 70, 45, scene_t(GOLD))
    assert (rgb[0] == 0).all() and (depth[0] == np.inf).all()
    assert (px[0][..., :3] == 0).all() and (px[0][..., 3] == 255).all()
    assert (depth[1] == 0).all() and (rgb[1].sum(-1) > 0).all()
    hit = np.isfinite(depth[2])
    assert hit.any() and 5.0 < depth[2][hit].min() < 6.0 and (rgb[2][hit].sum(-1) > 0).all()


def test_two_calls_give_equal_bits(rm):
    render, _ = rm
    sc = scene_t(V.synthetic_scene(64, 0))
    a = all_outputs(render, [V.POSES[0], V.POSES[4]], 80, 48, sc)
    b = all_outputs(render, [V.POSES[0], V.POSES[4]], 80, 48, sc)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("case", ["golden_70x45_special", "synth_M300_s1", "golden_64x48", "one_sphere_40x24",
                                  "synth_M520_32x24"])
def test_exact_skip_changes_no_bit(rm, case):
    render, native = rm
    name, scene, w, h, poses = next(c for c in CASES if c[0] == case)
    sc = scene_t(scene)
    on = all_outputs(render, poses, w, h, sc)
    off = all_outputs(render, poses, w, h, sc, params=native.view_params(flags=native.RM_MARCH_NO_EARLY_EXIT))
    for x, y in zip(on, off):
        assert x.tobytes() == y.tobytes()
    # and the iteration count the diagnostics flag reports is the specified trace's
    it = render.view(cams_of(poses), w, h, sc, depth=True,
                     params=native.view_params(flags=native.RM_VIEW_COUNT_ITERATIONS))[1].cpu().numpy()
    assert it.min() >= 1 and it.max() <= 100 and (it == np.round(it)).all()
    assert (it[np.isfinite(on[2])] < 100).all()


def test_fp16_colours_equal_fp32_render_of_rounded_colours(rm):
    render, _ = rm
    raw = V.synthetic_scene(33, 2)
    rounded = dict(raw, colors=raw["colors"].astype(np.float16).astype(np.float32))
    a = all_outputs(render, [V.POSES[0], V.POSES[4]], 80, 48, scene_t(raw, half=True))
    b = all_outputs(render, [V.POSES[0], V.POSES[4]], 80, 48, scene_t(rounded))
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_frame_alone_equals_frame_in_batch(rm):
    """Also across launches: 18 frames are more than one launch carries (16)."""
    render, _ = rm
    sc = scene_t(GOLD)
    poses = [V.POSES[i % 4] for i in range(18)]
    poses[17] = FAR
    batch = all_outputs(render, poses, 22, 19, sc)
    for f in (0, 1, 2, 3, 16, 17):
        alone = all_outputs(render, [poses[f]], 22, 19, sc)
        for x, y in zip(batch, alone):
            assert x[f].tobytes() == y[0].tobytes(), f


def test_null_outputs_and_argument_checks(rm):
    import ctypes
    import torch
    render, native = rm
    sc = scene_t(GOLD)
    w, h, poses = 22, 19, [V.POSES[0], V.POSES[2]]
    full = all_outputs(render, poses, w, h, sc)
    ctx = render.context(sc.centers.device)
    cams = native.view_cameras(cams_of(poses))
    p = native.view_params()

    def call(want, frames=2, width=w, height=h, params=p, cams=cams):
        bufs = [torch.zeros((2, h, w, 3), device="cuda"), torch.zeros((2, h, w, 4), device="cuda", dtype=torch.uint8),
                torch.zeros((2, h, w), device="cuda")]
        ptr = [ctypes.c_void_p(b.data_ptr()) if on else None for b, on in zip(bufs, want)]
        rc = ctx._lib.rm_view(ctx.handle, cams, frames, width, height, ctypes.byref(sc.c_struct()),
                              ctypes.byref(params) if params is not None else None, *ptr)
        torch.cuda.synchronize()
        return rc, [b.cpu().numpy() for b in bufs]

    for mask in range(1, 8):
        want = [(mask >> i) & 1 == 1 for i in range(3)]
        rc, got = call(want)
        assert rc == 0, (mask, native.lib().rm_last_error(ctx.handle))
        for on, g, f in zip(want, got, full):
            assert g.tobytes() == f.tobytes() if on else not g.any(), mask
    assert call([True, True, True], params=None)[1][0].tobytes() == full[0].tobytes()  # NULL params: the defaults
    assert call([False, False, False])[0] == 1
    assert b"output" in native.lib().rm_last_error(ctx.handle)
    assert call([True, True, True], frames=0)[0] == 1
    assert call([True, True, True], frames=native.RM_MAX_VIEWS_PER_CALL + 1)[0] == 1
    assert call([True, True, True], width=0)[0] == 1
    assert call([True, True, True], height=0)[0] == 1
    assert call([True, True, True], params=native.view_params(max_steps=0))[0] == 1
    assert call([True, True, True], cams=None)[0] == 1
    assert native.lib().rm_view(None, cams, 2, w, h, ctypes.byref(sc.c_struct()), None, None, None, None) == 1


def test_rgba8_is_the_srgb_encode(rm):
    render, _ = rm
    for name in ("golden_96x64", "synth_M64_s0"):
        _, scene, w, h, poses = next(c for c in CASES if c[0] == name)
        rgb, px, _ = all_outputs(render, poses, w, h, scene_t(scene))
        want = np.round(V.srgb8(rgb))
        err = np.abs(px[..., :3].astype(np.float64) - want).max()
        print(f"view rgba8 {name}: max |byte - round(255 srgb(rgb))| = {err}")
        assert err <= 1.0
        assert (px[..., 3] == 255).all()
        assert (rgb > 0.2).any() and px[..., :3][rgb > 0.2].min() > 100  # display-encoded, not linear bytes


def test_cli_view_writes_the_library_frames(rm, tmp_path):
    render, _ = rm
    from burn_raymarching_amd import _build, host
    exe = _build.build_host()
    out = tmp_path / "one"
    args = [exe, "view", "--scene", SCENE_JSON, "--out", str(out), "--size", "70x45", "--pos", "1.2,0.6,-1.6",
            "--yaw", "126", "--pitch", "-17"]
    subprocess.run(args, check=True, timeout=120)
    assert sorted(os.listdir(out)) == ["frame_0.png"]
    got = host.png_read_rgba(str(out / "frame_0.png"))
    deg = math.pi / 180.0
    pose = host.view_camera((1.2, 0.6, -1.6), float(np.float32(126.0 * deg)), float(np.float32(-17.0 * deg)))
    _, px = render.view([(tuple(pose.pos), tuple(pose.forward), tuple(pose.up))], 70, 45, scene_t(GOLD), rgba8=True)
    assert got.shape == (45, 70, 4) and (got == px[0].cpu().numpy()).all()
    assert (got[..., :3].sum(-1) > 0).sum() > 50  # the scene is in the frame

    orbit = tmp_path / "orbit"
    subprocess.run([exe, "view", "--scene", SCENE_JSON, "--out", str(orbit), "--size", "48x32", "--orbit", "4",
                    "--orbit-radius", "2.0", "--orbit-height", "0.5"], check=True, timeout=120)
    assert sorted(os.listdir(orbit)) == [f"frame_{i}.png" for i in range(4)]
    frames = [host.png_read_rgba(str(orbit / f"frame_{i}.png")) for i in range(4)]
    for fr in frames:
        assert fr.shape == (32, 48, 4) and (fr[..., 3] == 255).all() and (fr[..., :3].sum(-1) > 0).sum() > 20
    assert not (frames[0] == frames[1]).all()
    # pose i stands on the circle looking at the origin: frame 0 is the library's render of it
    ang = -0.5 * math.pi
    pos = tuple(float(np.float32(x)) for x in (2.0 * math.cos(ang), 0.5, 2.0 * math.sin(ang)))
    yaw = math.atan2(-pos[2], -pos[0])
    pitch = math.atan2(-pos[1], math.sqrt(pos[0] * pos[0] + pos[2] * pos[2]))
    pose = host.view_camera(pos, float(np.float32(yaw)), float(np.float32(pitch)))
    _, px = render.view([(tuple(pose.pos), tuple(pose.forward), tuple(pose.up))], 48, 32, scene_t(GOLD), rgba8=True)
    assert (frames[0] == px[0].cpu().numpy()).all()
