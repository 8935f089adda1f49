"""The out-of-envelope parity cases (tests/envelope_ref.py) on the CPU: each case lands on the side
of the shift admission it is meant to exercise, the fp32 reference-order oracle sits within 1/4 of
every bound that tests/test_gpu_envelope.py applies and no bound breaks its cap, and the fp32
oracle on an input that is wrong by a little (envelope_ref.mutants) fails the check. Together: the
bounds pass a correct fp32 computation with room and are not vacuous."""
import numpy as np
import pytest

import envelope_ref as E

NAMES = E.names() + ("split-M300",)


def test_synthetic_restates_model_synthetic_scene():
    from burn_raymarching_amd import model
    for m, seed in ((48, 0), (12, 5)):
        a, b = E.synthetic(m, seed), model.synthetic_scene(m, seed)
        for key in b:
            assert np.array_equal(a[key], b[key]), key
    assert E.ring_camera(3) == model.ring_cameras(7)[3]


def test_cases_cover_the_issue():
    labels = {s[0] for s in E.SPECS}
    assert {"wide", "big_radii", "trained_like-k32", "trained_like-k5", "fixed_edge99", "fixed_edge101", "none_edge29.5",
            "none_edge30.5", "outlier0", "outlier0-swapped", "duplicates", "eye_inside-k32", "eye_inside-k5",
            "eye_on_centre", "eye_in_big_sphere", "dir_scaled-alt", "dir_scaled-0.25", "dir_scaled-0.1"} <= labels
    for name in NAMES:
        c = E.case(name)
        assert c["org"].shape == (E.WIDTH * E.WIDTH, 3) and c["steps"] in (32, 40)
        assert all(np.asarray(v).dtype == np.float32 for v in c["scene"].values())
        assert (c["camera"] is None) == (c["gen"] == "dir_scaled")
    c = E.case("duplicates-M48")["scene"]
    d = np.linalg.norm(c["centers"][24:].astype(np.float64) - c["centers"][:24], axis=1)
    assert (d == 0.0).sum() == 18 and np.allclose(d[d > 0], 1e-3, rtol=1e-3) and d[0] == 0.0
    assert np.array_equal(c["radius"][:24], c["radius"][24:])
    c = E.case("eye_on_centre-M48")
    assert (np.float32(c["camera"][0]) == c["scene"]["centers"]).all(axis=1).any()
    c = E.case("eye_in_big_sphere-M48")
    assert c["scene"]["radius"][1] == 1.0
    assert abs(np.linalg.norm(np.float64(c["camera"][0]) - c["scene"]["centers"][1]) - 0.5) < 1e-6
    ln = np.linalg.norm(E.case("dir_scaled-alt-M48")["dir"].astype(np.float64), axis=1)
    assert np.allclose(ln[0::2], 0.5, atol=1e-6) and np.allclose(ln[1::2], 2.0, atol=1e-6)
    a, b = E.case("outlier0-M48")["scene"], E.case("outlier0-swapped-M48")["scene"]
    assert np.array_equal(a["centers"][0], b["centers"][-1]) and np.array_equal(a["centers"][-1], b["centers"][0])


@pytest.mark.parametrize("name", NAMES)
def test_admission_side(name, capsys):
    """The kernel's formula restated (envelope_ref.admission): which decision the case exercises."""
    c = E.case(name)
    qf, qn, fixed_ok, none_ok = E.admission(c["scene"], c["k"])
    with capsys.disabled():
        print(f"envelope admission {name:28s} kappa (rmax + spread) 1.001 = {qf:7.2f} (fixed_ok {fixed_ok})  "
              f"kappa rmax 1.001 = {qn:6.2f} (none_ok {none_ok})")
    assert (fixed_ok, none_ok) == c["expect_admission"]
    edge = {"fixed_edge99": (qf, 99.0), "fixed_edge101": (qf, 101.0), "none_edge29.5": (qn, 29.5),
            "none_edge30.5": (qn, 30.5), "outlier0": (qf, 99.0)}.get(name.rsplit("-M", 1)[0])
    if edge is not None:
        assert abs(edge[0] - edge[1]) < 0.05, edge
    if name.startswith("outlier0-M"):  # sphere 0 alone sets spread: without it the scene is half as wide
        cen = c["scene"]["centers"].astype(np.float64)
        assert E._spread(cen[1:]) < 0.7 * E._spread(cen)


@pytest.mark.parametrize("name", NAMES)
def test_float32_oracle_within_a_quarter_of_every_bound(name, capsys):
    ref = E.reference(name)
    for key in ("out", "train_out"):
        assert np.isfinite(ref[key]).all()
    err, bnd = E.fp32_errors(name), E.bounds(name)
    worst = max(err, key=lambda k: err[k] / bnd[k])
    with capsys.disabled():
        print(f"envelope fp32 {name:28s} worst {err[worst] / bnd[worst]:.3f} of bound at {worst}: {err[worst]:.3g} "
              f"(bound {bnd[worst]:.3g}, existing {E.existing_bound(worst):.3g})")
    for key, v in err.items():
        assert np.isfinite(v) and v <= bnd[key] / E.MARGIN * (1 + 1e-12), (key, v, bnd[key])
        assert bnd[key] >= E.existing_bound(key)
    assert E.caps_hold(name) == []


@pytest.mark.parametrize("name", NAMES)
def test_every_mutant_fails_the_check(name, capsys):
    dist = E.mutant_distances(name)
    closest = min(dist, key=dist.get)
    with capsys.disabled():
        print(f"envelope mutants {name:28s} closest: {closest} at {dist[closest]:.3g} bounds "
              f"({', '.join(f'{k} {v:.3g}' for k, v in dist.items())})")
    assert {"radius x1.02", "sphere removed", "centre +5e-3", "k x1.02"} <= set(dist)
    if name.startswith("dir_scaled"):
        assert "unit directions" in dist
    assert dist[closest] > 1.0, (closest, dist[closest])


@pytest.mark.parametrize("label", E.RENDER_CASES)
@pytest.mark.parametrize("m", E.SIZES)
def test_render_bounds(label, m):
    """rm_render's cases: the fp32 oracle.render within 1/4 of the bounds, the bounds within the cap."""
    name = f"{label}-M{m}"
    (emax, emean), (bmax, bmean) = E.render_fp32_errors(name), E.render_bounds(name)
    assert emax <= bmax / E.MARGIN and emean <= bmean / E.MARGIN
    assert bmax <= E.CAP_FACTOR * E.FWD_MAX and bmean <= E.CAP_FACTOR * E.FWD_MEAN, (bmax, bmean)
    assert (np.abs(E.render_reference(name)).max(axis=1) > 1e-3).mean() > 0.05  # the rays see the scene


@pytest.mark.parametrize("name", E.t_names())
def test_t_march_cases_are_well_conditioned(name):
    assert E.t_fp32_error(name) <= E.T_REL / E.MARGIN
    ref = E.reference(name)
    assert (np.abs(ref["out"]).max(axis=1) > 1e-6).any()  # some rays are seen


@pytest.mark.parametrize("name", E.t_names())
def test_t_bound_passes_the_float32_oracle_and_keeps_seen_rays_strict(name):
    """The conditioned clause of the t_march check (envelope_ref.t_bound): the fp32 oracle is within
    a quarter of it at every ray, and it widens the bound at few rays only."""
    err = E.t_error(E.run_oracle(E.case(name), "f32")["t"], name)
    assert (err <= E.t_bound(name) / E.MARGIN).all()
    assert (E.t_bound(name) > E.T_REL).mean() <= 0.06


def test_the_grazing_ray_is_in_the_suite():
    """eye_inside-k32-M48, ray 456: at t = 0.33 .. 0.59 for 24 steps, gone to 8.08 in the last four;
    unseen; its t moves 3e-5 under one rounding of the inputs."""
    name = "eye_inside-k32-M48"
    ref = E.reference(name)
    assert 8.0 < ref["t"][456] < 8.2 and np.abs(ref["out"][456]).max() < 1e-30
    assert E.T_REL < E.t_bound(name)[456] < 4.0 * E.T_REL


def test_unmutated_float32_oracle_passes_and_a_wrong_one_reports():
    name = "wide-M12"
    assert E.failures(E.run_oracle(E.case(name), "f32"), name) == {}
    bad = E.run_oracle(E.case(name), "f32")
    bad["out"] = bad["out"] + np.float32(0.1)
    assert set(E.failures(bad, name)) == {("fwd", "max"), ("fwd", "mean")}
    bad["bwd"]["radius"][:] = np.nan
    assert ("bwd", "radius", "norm") in E.failures(bad, name)
