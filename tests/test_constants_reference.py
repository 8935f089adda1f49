"""The constants cases (tests/constants_ref.py) on the CPU: the fp32 reference-order oracle sits within
1/4 of every bound that tests/test_gpu_constants.py applies and no bound breaks its cap; the fp32
oracle at constants that are wrong in one way (a field ignored, two fields swapped, a field x 1.02)
fails the check; the oracle's analytic backward and torch autograd of oracle/autodiff_ref.py agree at
every constant set; and the six-tap normal against its eps -> 0 limit (the form the kernels use):
under a quarter of the forward bounds up to k * normal_eps = 0.032, beyond them at 0.32."""
import numpy as np
import pytest
import torch

import constants_ref as C
import envelope_ref as E
import raygrad_ref as R
from conftest import FINAL1_CAMERA, final1_scene
from oracle import autodiff_ref as ad
from oracle import oracle

NAMES = C.names()
ALL_NAMES = NAMES + C.LIMIT_NAMES


def test_cases_cover_the_issue():
    assert C.SETS == {"eps1e-3": (1e-3, 10.0, 15.0), "eps1e-5": (1e-5, 10.0, 15.0), "csharp3": (1e-4, 3.0, 15.0),
                      "csharp40": (1e-4, 40.0, 15.0), "csharp0": (1e-4, 0.0, 15.0), "msharp2": (1e-4, 10.0, 2.0),
                      "msharp60": (1e-4, 10.0, 60.0), "msharp0": (1e-4, 10.0, 0.0), "all": (1e-3, 25.0, 6.0)}
    for cset in C.SETS:
        assert {f"{cset}-M48", f"{cset}-M12"} <= set(NAMES)
    assert {"all-k5-M48", "all-split-M300", "msharp2-split-M300"} <= set(NAMES)
    for name in ALL_NAMES:
        c = C.case(name)
        assert c["org"].shape == (E.WIDTH * E.WIDTH, 3) and E.WIDTH == 32
        want = C.STEPS_VISIBLE.get(c["set"], 32 if c["M"] in (48, 300) else 40)
        assert c["steps"] == want and c["steps"] <= 40
        assert c["k"] == (5.0 if name == "all-k5-M48" else 32.0)
        if name in NAMES:
            assert c["consts"] == tuple(float(np.float32(v)) for v in C.SETS[c["set"]]) and c["normal"] == "taps"
            assert c["k"] * c["consts"][0] <= C.TAPS_LIMIT_K_EPS * (1 + 1e-6)
    assert all(s <= 12 for s in C.STEPS_VISIBLE.values())
    for name in C.LIMIT_NAMES:
        c = C.case(name)
        assert c["normal"] == "limit" and c["consts"] == tuple(float(np.float32(v)) for v in (1e-2, 10.0, 15.0))
    # msharp2's mask is not 0 on missed rays, msharp0's is 0.5 everywhere
    for name in ("msharp2-M48", "msharp2-M12", "msharp2-split-M300"):  # between the default gone_d = 6 and its 45
        dist = C.debug_reference(name)[:, 9]
        between = (dist > 6.0) & (dist < 45.0)
        assert between.sum() > 50 and (np.abs(C.reference(name)["out"].astype(np.float32)).max(axis=1) > 0)[between].all()
    assert np.allclose(C.debug_reference("msharp0-M48")[:, 10], 0.5, atol=0, rtol=0)


def test_oracle_defaults_are_the_reference_literals():
    """The keywords' defaults give the bits of a call without them (the parent's entry points)."""
    c = E.case("wide-M12")
    for prec, dt in (("f32", np.float32), ("f64", np.float64)):
        o, d = c["org"].astype(dt), c["dir"].astype(dt)
        kw = dict(C.consts_kw(C.DEFAULT), normal="taps", precision=prec)
        a = oracle.render_diff(o, d, c["scene"], c["steps"], c["k"], precision=prec)
        assert np.array_equal(a, oracle.render_diff(o, d, c["scene"], c["steps"], c["k"], **kw))
        out = np.empty_like(a)
        lib = oracle.lib()
        sc = oracle._scene(c["scene"], dt)
        getattr(lib, f"orc_render_diff_{prec}")(len(o), oracle._ptr(o), oracle._ptr(d), *(oracle._ptr(x) for x in sc),
                                                 c["M"], c["steps"], c["k"], oracle._ptr(out), None)
        assert np.array_equal(a.view(np.uint8), out.view(np.uint8))


@pytest.mark.parametrize("name", ALL_NAMES)
def test_float32_oracle_within_a_quarter_of_every_bound(name, capsys):
    ref = C.reference(name)
    for key in ("out", "train_out", "t"):
        assert np.isfinite(ref[key]).all()
    err, bnd = C.fp32_errors(name), C.bounds(name)
    worst = max(err, key=lambda k: err[k] / bnd[k])
    with capsys.disabled():
        print(f"constants fp32 {name:20s} worst {err[worst] / bnd[worst]:.3f} of bound at {worst}: {err[worst]:.3g} "
              f"(bound {bnd[worst]:.3g}, existing {E.existing_bound(worst):.3g})")
    for key, v in err.items():
        assert np.isfinite(v) and v <= bnd[key] / E.MARGIN * (1 + 1e-12), (key, v, bnd[key])
        assert bnd[key] >= E.existing_bound(key)
    assert C.caps_hold(name) == []
    sb = C.stage_bounds(name)
    assert all(E.FWD_MAX <= b <= E.CAP_FACTOR * E.FWD_MAX for b in sb.values()), sb
    assert C.seen(name).sum() >= 30 and (np.abs(ref["out"]).max(axis=1) > 1e-3).sum() >= 30  # rays see the scene
    # t_march of the seen rays: the fp32 oracle within T_REL / MARGIN
    t32 = C.run_oracle(C.case(name), "f32")["t"]
    assert E.t_rel_error(t32, ref["t"])[C.seen(name)].max() <= E.T_REL / E.MARGIN


@pytest.mark.parametrize("name", NAMES)
def test_every_mutant_fails_the_check(name, capsys):
    dist = C.mutant_distances(name)
    cset = C.case(name)["set"]
    with capsys.disabled():
        print(f"constants mutants {name:20s} " + ", ".join(f"{k} {v:.3g}" for k, v in dist.items()))
    want = {f"{f} x1.02" for f in C.FIELDS} | {f"{f} ignored" for f, v, dflt in zip(C.FIELDS, C.SETS[cset], C.DEFAULT)
                                                  if v != dflt}
    if cset == "all":
        want.add("sharpnesses swapped")
        assert len(want) == 7
    assert set(dist) == want
    for mut, v in dist.items():
        other = C.CANNOT_FAIL.get((cset, mut))
        if other is None:
            assert v > 1.0, (mut, v)
        else:  # cannot fail here by construction (1.02 x 0 = 0): the named set catches the same mutant
            assert C.case(name)["consts"][C.FIELDS.index(mut.split(" ")[0])] == 0.0
            for m in (48, 12):
                assert C.mutant_distances(f"{other}-M{m}")[mut] > 1.0


def test_unmutated_float32_oracle_passes_and_a_wrong_one_reports():
    name = "all-M12"
    assert C.failures(C.run_oracle(C.case(name), "f32"), name) == {}
    bad = C.run_oracle(C.case(name), "f32")
    bad["out"] = bad["out"] + np.float32(0.1)
    assert set(C.failures(bad, name)) == {("fwd", "max"), ("fwd", "mean")}


def _torch_params(sc):
    def t(x, shape):
        return torch.tensor(np.asarray(x, np.float64).reshape(shape), requires_grad=True)
    return (t(sc["centers"], (-1, 3)), t(sc["colors"], (-1, 3)), t(sc["radius"], (-1, 1)),
            t(sc["light_dir"], (3,)), t(sc["ambient"], (1,)))


@pytest.mark.parametrize("cset", tuple(C.SETS) + ("all-k5",))
def test_backward_matches_autograd_at_every_constant_set(cset):
    """The two references pin each other off the defaults: the oracle's analytic backward against torch
    fp64 autograd of autodiff_ref.render_diff, test_oracle.py::test_backward_matches_autograd's case
    and tolerance (1e-10 forward, 1e-9 relative per gradient group)."""
    from burn_raymarching_amd.model import ring_cameras, synthetic_scene
    k = 5.0 if cset == "all-k5" else 32.0
    cset = "all" if cset == "all-k5" else cset
    kw = C.consts_kw(C.SETS[cset])
    # the sets whose receding rays stay visible march as few steps here as in their cases: farther out the
    # tap differences sink into fp64's own rounding (4e-10 in the image at msharp0 after 16 steps)
    steps = min(16, C.STEPS_VISIBLE.get(cset, 16))
    sc = synthetic_scene(8, seed=3)
    sc["radius"] = sc["radius"] + 0.04
    o, d = oracle.camera_rays(12, 12, *ring_cameras(6)[2], precision="f64")
    g = np.random.default_rng(7).normal(size=o.shape)
    c, col, r, ld, a = _torch_params(sc)
    out = ad.render_diff(torch.tensor(o), torch.tensor(d), c, col, r, ld, a, k, steps=steps, **kw)
    (out * torch.tensor(g)).sum().backward()
    ref = {"centers": c.grad, "colors": col.grad, "radius": r.grad, "light_dir": ld.grad, "ambient": a.grad}
    fwd = oracle.render_diff(o, d, sc, steps, k, precision="f64", **kw)
    assert np.abs(out.detach().numpy() - fwd).max() < 1e-10
    got = oracle.render_diff_backward(o, d, sc, steps, k, g, precision="f64", **kw)
    for key, v in ref.items():
        v = v.numpy().reshape(-1)
        rel = np.abs(got[key].reshape(-1) - v).max() / max(np.abs(v).max(), 1e-30)
        assert rel < 1e-9, (key, rel)
    if cset in C.RAYGRAD_SETS:  # raygrad_ref passes the constants on: closed form == autograd
        go, gd = R.ray_grads(o, d, sc, k, steps, g, **kw)
        co, cd = R.closed_form_ray_grads(o, d, sc, k, steps, g, **kw)
        assert np.abs(go - co).max() <= 1e-9 * np.abs(go).max() and np.abs(gd - cd).max() <= 1e-9 * np.abs(gd).max()
        do, _ = R.ray_grads(o, d, sc, k, steps, g)
        assert np.abs(go - do).max() > 1e-3 * np.abs(go).max()  # and they change the gradient


def test_limit_normal_is_the_taps_as_eps_goes_to_zero():
    """oracle normal="limit" against the taps in fp64: the raw normal's relative gap falls as (k eps)^2,
    and n = f / sqrt(|f|^2 + 1e-6) is itself proportional to eps once |f| = 2 eps |grad D| sinks under
    1e-3, so n.l's gap falls by 100 to 1000 per decade of eps."""
    c = C.case("limit-M48")
    gaps = [C.taps_limit_gap(c["org"], c["dir"], c["scene"], c["steps"], c["k"], eps)["ndotl"][0]
            for eps in (1e-2, 1e-3, 1e-4)]
    assert gaps[2] < 1e-6 and 50.0 < gaps[0] / gaps[1] < 1000.0 and 50.0 < gaps[1] / gaps[2] < 1000.0, gaps


def test_taps_against_limit(capsys):
    """include/raymarch.h, rm_march.normal_eps: the differentiable modes use f = 2 eps grad D. On the
    M = 48 scene at k = 32 the image of the taps reference differs from the limit's by more than a
    forward bound at eps = 1e-2 (k eps = 0.32) and by less than a quarter of both bounds at eps <= 1e-3
    (k eps <= 0.032, TAPS_LIMIT_K_EPS). The header's table is re-measured here: masked |n.l(taps) -
    n.l(limit)| over 24x24 rays of the final_1 camera on scene.json and on synthetic(48, 3)."""
    for name in ("limit-M48", "eps1e-3-M48", "all-M48"):
        big = C.case_gap(name, 1e-2)["out"]
        assert big[0] > E.FWD_MAX or big[1] > E.FWD_MEAN, (name, big)
        for eps in (1e-3, 1e-4, 1e-5):
            assert eps * 32.0 <= C.TAPS_LIMIT_K_EPS * (1 + 1e-9)
            small = C.case_gap(name, eps)["out"]
            assert small[0] < E.FWD_MAX / 4 and small[1] < E.FWD_MEAN / 4, (name, eps, small)
    o, d = oracle.camera_rays(24, 24, *FINAL1_CAMERA, precision="f64")
    rows = {}
    for label, sc in (("scene.json", final1_scene()), ("synthetic(48, 3)", E.synthetic(48, 3))):
        for k in (32.0, 5.0):
            rows[label, k] = [C.taps_limit_gap(o, d, sc, 40, k, eps)["ndotl"] for eps in C.GAP_EPS]
    with capsys.disabled():
        print("taps against limit, masked |n.l| gap max / mean at eps = " + ", ".join(f"{e:g}" for e in C.GAP_EPS))
        for (label, k), row in rows.items():
            print(f"  {label:18s} k = {k:4.0f}: " + "  ".join(f"{a:.1e} / {b:.1e}" for a, b in row))
    # the header's figures, to a factor of two
    header = {("scene.json", 32.0): (1.8e-5, 2.0e-4, 2.3e-3, 2.1e-2), ("synthetic(48, 3)", 32.0): (2.2e-5, 2.9e-4, 3.7e-3, 2.9e-2)}
    for key, want in header.items():
        for (got, _), w in zip(rows[key][1:], want):
            assert 0.5 * w <= got <= 2.0 * w, (key, got, w)
    for label in ("scene.json", "synthetic(48, 3)"):  # k = 5: far smaller, as (k eps)^2 says
        assert rows[label, 5.0][1][0] < rows[label, 32.0][1][0] / 10 and rows[label, 5.0][3][0] < rows[label, 32.0][3][0] / 50


def test_render_wrappers_take_the_three_constants():
    """render.py: every differentiable wrapper passes the three fields on, defaults the reference's."""
    import inspect

    from burn_raymarching_amd import render
    for fn in (render.render_diff_forward, render.render_diff_backward, render.render_diff_backward_rays,
               render.render_diff_backward_cameras, render.render_diff_camera, render.render_diff_backward_camera,
               render.train_step, render.train_step_camera, render.render_diff, render.render_diff_cameras):
        p = inspect.signature(fn).parameters
        assert [p[f].default for f in C.FIELDS] == list(C.DEFAULT), fn.__name__
        assert all(p[f].kind is inspect.Parameter.KEYWORD_ONLY for f in C.FIELDS), fn.__name__
    for fn in (render._RenderDiffFn.forward, render._RenderDiffCamerasFn.forward):
        assert list(inspect.signature(fn).parameters)[-3:] == list(C.FIELDS)
