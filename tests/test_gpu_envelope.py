"""The kernels against the fp64 oracle outside the envelope of model.synthetic_scene: every case of
tests/envelope_ref.py (scenes that refuse the fixed or the unshifted log-sum-exp by themselves,
both sides of each admission threshold, sphere 0 as the outlier, coincident spheres, eyes inside
the scene / on a centre / inside a sphere, scaled ray directions, a translated scene), through the
Python layer in array mode and in camera mode, on the general and on the small-scene kernel. The
measures and bounds are envelope_ref's: max(the suite's bound, 4 x the fp32 reference-order
oracle's own error at the case), capped; tests/test_envelope_reference.py shows on the CPU that
they pass the fp32 oracle with room and fail an input that is wrong by 2 %."""
import ctypes

import numpy as np
import pytest

import envelope_ref as E
from conftest import GRAD_KEYS, gpu_available, record_margin

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

GUARD = 12345.0
NAMES = E.names()
CAMERA_NAMES = tuple(n for n in NAMES if not n.startswith("dir_scaled"))
SMALL_NAMES = tuple(n for n in NAMES if n.endswith("-M12"))


@pytest.fixture(scope="module")
def rm():
    import torch
    from burn_raymarching_amd import _build
    _build.build_lib()
    from burn_raymarching_amd import native, render
    torch.cuda.init()
    return render, native


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def scene_dev(rm, sc):
    return rm[0].Scene(dev(sc["centers"]), dev(sc["colors"]), dev(sc["radius"]), dev(sc["light_dir"]), dev(sc["ambient"]))


def unit_dirs(name):
    return not name.startswith("dir_scaled")


def exit_env(name):
    """include/raymarch.h, ray_dir: the escape proof is stated for unit directions. The x0.1 rays are
    compared with the oracle with the early exit off only; x0.25 and x0.5 / x2 also with it on."""
    return {"RM_NO_EARLY_EXIT": "1"} if name.startswith("dir_scaled-0.1") else {}


_RUNS = {}


def run_gpu(rm, name, camera=False, **env):
    """The results of run_oracle's keys from the device (numpy), plus out_fast: the forward without
    t_march (the only forward that may leave the march early). Computed once per (case, mode,
    environment); `env` is set for the calls and restored."""
    key = (name, camera, tuple(sorted(env.items())))
    if key in _RUNS:
        return _RUNS[key]
    render = rm[0]
    c = E.case(name)
    s = scene_dev(rm, c["scene"])
    k, steps = c["k"], c["steps"]
    g, tg = dev(c["grad_out"]), dev(c["targets"])
    with pytest.MonkeyPatch.context() as mp:
        for var, val in env.items():
            mp.setenv(var, val)
        if camera:
            cams = [c["camera"]]
            out, t = render.render_diff_camera(cams, E.WIDTH, E.WIDTH, s, k, steps, return_t=True)
            fast = render.render_diff_camera(cams, E.WIDTH, E.WIDTH, s, k, steps)
            bwd = render.render_diff_backward_camera(cams, E.WIDTH, E.WIDTH, s, k, g, steps)
            import torch
            tout = torch.empty_like(out)
            loss, train, _ = render.train_step_camera(cams, E.WIDTH, E.WIDTH, tg, s, k, E.PROGRESS, steps, out=tout)
        else:
            o, d = dev(c["org"]), dev(c["dir"])
            out, t = render.render_diff_forward(o, d, s, k, steps, return_t=True)
            fast = render.render_diff_forward(o, d, s, k, steps)
            bwd = render.render_diff_backward(o, d, s, k, g, steps)
            loss, train, tout = render.train_step(o, d, tg, s, k, E.PROGRESS, steps, with_out=True)
    got = {"out": host(out), "t": host(t), "out_fast": host(fast), "bwd": {q: host(v) for q, v in bwd.items()},
           "train_out": host(tout), "loss": float(host(loss)[0]), "train": {q: host(v) for q, v in train.items()}}
    _RUNS[key] = got
    return got


def all_finite(got):
    return all(np.isfinite(v).all() for key in ("out", "t", "out_fast", "train_out") for v in [got[key]]) and \
        np.isfinite(got["loss"]) and all(np.isfinite(got[m][q]).all() for m in ("bwd", "train") for q in GRAD_KEYS)


def check(got, name, label):
    """Every measure of envelope_ref within the case's bound; the figures go to the margins record."""
    assert all_finite(got), label
    ms, bnd = E.measures(got, E.reference(name)), E.bounds(name)
    for key, v in ms.items():
        record_margin("env_" + "_".join(key), v, bnd[key])
    worst = max(ms, key=lambda q: ms[q] / bnd[q])
    print(f"envelope parity {label}: worst {ms[worst] / bnd[worst]:.3f} of bound at {worst} "
          f"({ms[worst]:.3g}, bound {bnd[worst]:.3g})")
    bad = {q: (v, bnd[q]) for q, v in ms.items() if not v <= bnd[q]}
    assert not bad, (label, bad)


def same_bits(a, b, label, keys=("out", "t", "out_fast", "train_out", "loss", "bwd", "train")):
    for key in keys:
        if key in ("bwd", "train"):
            for q in GRAD_KEYS:
                assert np.array_equal(a[key][q].view(np.uint32), b[key][q].view(np.uint32)), (label, key, q)
        elif key == "loss":
            assert np.float32(a[key]) == np.float32(b[key]), (label, key)
        else:
            assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), (label, key)


@pytest.mark.parametrize("name", NAMES)
def test_array_mode_matches_oracle(rm, name):
    """Forward, backward (normal upstream gradient) and train step, RM_SMALL at its default. Rays
    with scaled directions are outside the documented precondition of the march's shortcuts
    (include/raymarch.h, ray_dir): they are held to the oracle all the same, also with the early
    exit off, but not to the bit-equalities."""
    got = run_gpu(rm, name, **exit_env(name))
    if unit_dirs(name):
        assert np.array_equal(got["out"].view(np.uint32), got["out_fast"].view(np.uint32)), "t_march changes the image"
    else:
        check(run_gpu(rm, name, RM_NO_EARLY_EXIT="1"), name, f"{name} array, exit off")
    check(got, name, f"{name} array")


@pytest.mark.parametrize("name", SMALL_NAMES)
def test_general_kernel_at_small_m_matches_oracle(rm, name):
    """The M = 12 cases on the general kernel (RM_SMALL=0; the default takes the small-scene one)."""
    check(run_gpu(rm, name, RM_SMALL="0", **exit_env(name)), name, f"{name} array RM_SMALL=0")
    if not name.startswith("dir_scaled"):
        check(run_gpu(rm, name, camera=True, RM_SMALL="0"), name, f"{name} camera RM_SMALL=0")


@pytest.mark.parametrize("name", CAMERA_NAMES)
def test_camera_mode_matches_oracle_and_array_mode(rm, name):
    """Camera mode (write_origins, rho_lb, the shared origin step) against the oracle, and its
    forward and t_march bit for bit array mode's on the oracle's fp32 camera.rs rays. A march
    step's log-sum-exp shift is chosen per wave, from the wave's own rays, and the three forms agree
    to rounding only: outside the synthetic envelope the choice differs between waves, so equal
    bits need equal waves. Two comparisons give them: camera mode in row order (RM_ROW_ORDER, the
    order of array mode) in the default 16x16 tiles' place, and the tiles with one shift for every
    wave (RM_FORCE_MAX_SHIFT) on both sides."""
    small = {"RM_SMALL": "0"} if name.endswith("-M12") else {}  # a forced shift leaves the small-scene kernel
    got = run_gpu(rm, name, camera=True)
    check(got, name, f"{name} camera")
    same_bits(run_gpu(rm, name, camera=True, RM_ROW_ORDER="1"), run_gpu(rm, name), f"{name} rows",
              keys=("out", "out_fast", "t"))
    same_bits(run_gpu(rm, name, camera=True, RM_FORCE_MAX_SHIFT="1", **small),
              run_gpu(rm, name, RM_FORCE_MAX_SHIFT="1", **small), f"{name} tiles, one shift", keys=("out", "out_fast", "t"))
    check(run_gpu(rm, name, camera=True, RM_FORCE_MAX_SHIFT="1", **small), name, f"{name} camera, running-max shift")
    # the default tiles against rows: the same bits where the march has one form, else bounded
    arr = run_gpu(rm, name)
    if E.single_form(name):
        same_bits(got, arr, f"{name} tiles, one form", keys=("out", "out_fast", "t"))
    d_out = np.abs(got["out"].astype(np.float64) - arr["out"]).max()
    d_t = np.abs(got["t"].astype(np.float64) - arr["t"]) / np.maximum(1.0, np.abs(arr["t"]))
    t_bnd = np.maximum(E.WAVE_ABS, E.T_AMPLIFY * E.t_sensitivity(name))
    record_margin("env_tiles_rows_out", d_out, E.WAVE_ABS)
    record_margin("env_tiles_rows_t", (d_t / t_bnd).max(), 1.0)
    print(f"envelope tiles/rows {name}: out {d_out:.3g}, t {d_t.max():.3g} ({(d_t / t_bnd).max():.3f} of its bound)")
    assert d_out <= E.WAVE_ABS, (name, d_out)
    assert (d_t <= t_bnd).all(), (name, np.flatnonzero(d_t > t_bnd)[:8], d_t.max())


@pytest.mark.parametrize("name", CAMERA_NAMES)
def test_early_exit_changes_no_bit(rm, name):
    """Image, loss, t_march and every gradient, array mode and camera mode (unit directions: the
    precondition of this guarantee, include/raymarch.h)."""
    a, b = run_gpu(rm, name, RM_NO_EARLY_EXIT="1"), run_gpu(rm, name, RM_NO_EARLY_EXIT="0")
    same_bits(a, b, f"{name} array exit off/on")
    same_bits(b, run_gpu(rm, name), f"{name} array exit default", keys=("out", "loss"))
    same_bits(run_gpu(rm, name, camera=True, RM_NO_EARLY_EXIT="1"),
              run_gpu(rm, name, camera=True, RM_NO_EARLY_EXIT="0"), f"{name} camera exit off/on")


@pytest.mark.parametrize("name", CAMERA_NAMES)
def test_per_ray_origin_changes_no_bit(rm, name):
    """The per-view shared origin step against every ray taking step 0 itself (RM_PER_RAY_ORIGIN)."""
    small = {"RM_SMALL": "0"} if name.endswith("-M12") else {}  # the flag leaves the small-scene kernel
    same_bits(run_gpu(rm, name, camera=True, RM_PER_RAY_ORIGIN="1", **small),
              run_gpu(rm, name, camera=True, RM_PER_RAY_ORIGIN="0", **small), f"{name} camera per-ray origin on/off")


@pytest.mark.parametrize("split", ["1", "0"])
def test_split_march_at_m300(rm, split):
    """trained_like at M = 300 (both shift permissions refused) with the split march forced and off."""
    name = "split-M300"
    check(run_gpu(rm, name, RM_SPLIT=split), name, f"{name} array RM_SPLIT={split}")
    check(run_gpu(rm, name, camera=True, RM_SPLIT=split), name, f"{name} camera RM_SPLIT={split}")


@pytest.mark.parametrize("name", E.t_names())
def test_t_march_contract(rm, name):
    """include/raymarch.h's t_march, as test_gpu_early_exit.py::test_t_march_contract_against_oracle
    states it: the reference's t to 1e-3 where the ray is seen; elsewhere that, or at most the
    reference's with an output of exactly 0, or -- a ray that is neither seen nor proven gone and
    whose t is ill-conditioned -- within envelope_ref.t_bound, the limit the header states."""
    ref = E.reference(name)
    t_ref = np.asarray(ref["t"], np.float64).reshape(-1)
    for camera in (False, True):
        got = run_gpu(rm, name, camera=camera)
        t_gpu = got["t"].astype(np.float64)
        err = E.t_error(t_gpu, name)
        unseen_gone = np.all(got["out"] == 0.0, axis=1) & (t_gpu <= t_ref * (1 + 1e-5) + 1e-4)
        record_margin("env_t_march", err[~unseen_gone].max(), E.T_REL)
        close = err <= E.T_REL
        bounded = (t_gpu <= t_ref * (1 + 1e-5) + 1e-4) & np.all(got["out"] == 0.0, axis=1)
        seen = np.abs(ref["out"]).max(axis=1) > 1e-6
        conditioned = ~seen & (err <= E.t_bound(name))
        record_margin("env_t_march_conditioned", (err / E.t_bound(name))[~unseen_gone].max(), 1.0)
        assert np.all(close | bounded | conditioned), (camera, np.flatnonzero(~(close | bounded | conditioned))[:8])
        assert close.sum() > 0 and np.isfinite(t_gpu).all()
        seen = np.abs(ref["out"]).max(axis=1) > 1e-6
        assert seen.any() and np.all(close[seen]), (camera, np.flatnonzero(seen & ~close)[:8])


@pytest.mark.parametrize("label", E.RENDER_CASES)
@pytest.mark.parametrize("m", E.SIZES)
def test_target_renderer_matches_oracle(rm, label, m):
    """rm_render (renderer.rs, with its own escape distance) against oracle.render in fp64."""
    name = f"{label}-M{m}"
    c = E.case(name)
    sc = c["scene"]
    got = host(rm[0].render(dev(c["org"]), dev(c["dir"]), dev(sc["centers"]), dev(sc["colors"]), dev(sc["radius"])))
    assert np.isfinite(got).all()
    e = np.abs(got.astype(np.float64) - E.render_reference(name))
    bmax, bmean = E.render_bounds(name)
    record_margin("env_render_max", e.max(), bmax)
    record_margin("env_render_mean", e.mean(), bmean)
    assert e.max() <= bmax and e.mean() <= bmean, (e.max(), bmax, e.mean(), bmean)


@pytest.mark.parametrize("name", NAMES)
def test_nothing_written_outside_the_buffers(rm, name):
    """The C ABI calls on slices of one arena filled with GUARD, 64 guard words around each of out,
    t_march, the five gradient buffers and the loss: the guard words keep their value, and the
    results are the Python layer's bit for bit."""
    import torch
    render, native = rm
    c = E.case(name)
    m, n = c["M"], len(c["org"])
    sizes = {"out": 3 * n, "t": n, "centers": 3 * m, "colors": 3 * m, "radius": m, "light_dir": 3, "ambient": 1, "loss": 1}
    off, total = {}, 64
    for key, size in sizes.items():
        off[key] = total
        total += (size + 63) // 64 * 64 + 64
    ctx = render.context()
    s = scene_dev(rm, c["scene"])
    o, d, g, tg = dev(c["org"]), dev(c["dir"]), dev(c["grad_out"]), dev(c["targets"])
    march = s.march_for(native.march_params(c["steps"], c["k"]))
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    ref = run_gpu(rm, name)

    def arena_call(call, written):
        arena = torch.full((total,), GUARD, device="cuda")
        buf = {key: arena[off[key]:off[key] + sizes[key]] for key in sizes}
        cg = native.RmGrads(*(buf[q].data_ptr() for q in GRAD_KEYS))
        call(buf, cg)
        torch.cuda.synchronize()
        used = torch.zeros(total, dtype=torch.bool, device="cuda")
        for key in written:
            used[off[key]:off[key] + sizes[key]] = True
        assert bool((arena[~used] == GUARD).all()), f"{name}: a write outside {written}"
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
