"""Oracle-parity cases outside the envelope of model.synthetic_scene (centres in a ball of 0.6,
radii 0.03-0.12, eyes 2.5 away, unit directions), and the bounds they are checked with. Shared by
tests/test_envelope_reference.py (CPU) and tests/test_gpu_envelope.py. Uses numpy and the CPU
oracle only itself; the existing bounds are imported, not copied (conftest's and
test_gpu_parity's), and importing test_gpu_parity evaluates its skip mark, which imports torch and
asks whether a device is there.

Each case makes one of the march's data-dependent decisions fall the other way than it does on
the synthetic scenes:
  * the log-sum-exp shift admission (rm_ray.h, rm_kernels.hip), restated in admission():
      fixed_ok = kappa (r_max + spread) 1.001 <= 100,   none_ok = kappa r_max 1.001 <= 30,
      kappa = k log2(e), spread = max_j |c_j - c_0|;
  * the clamp-free proofs (all_safe, rho_lb, kSafeRho), which only matter for a ray point within
    ~1e-3 of a sphere centre: eyes inside the scene, inside a sphere, on a centre;
  * the escape proof (write_bound), stated for unit ray directions: scaled directions;
  * coincident spheres (prune_and_split children) and sphere 0 as the outlier that sets spread.

A bound is max(the suite's existing bound for the measure, MARGIN x the error of the fp32
reference-order oracle against the fp64 oracle at that case): the kernels sum in another order
than the reference, so a bound at the reference's own error would test rounding luck. Two caps
keep a derived bound from going vacuous (caps_hold): forward and per-sphere measures at most
CAP_FACTOR x the existing bound, light_dir / ambient normwise at most CAP_GLOBAL. A case that
breaks a cap, or that one of the mutants() passes, is replaced by another seed of its generator
(the seeds of SPECS; test_envelope_reference.py fails until both hold).
"""
import functools
import math

import numpy as np

from conftest import GRAD_KEYS, GRAD_TOL, PER_SPHERE, REL_ELEM, REL_L2, grad_errors
from oracle import oracle
from test_gpu_parity import FWD_MAX, FWD_MEAN

MARGIN = 4.0
CAP_FACTOR = 10.0
CAP_GLOBAL = 0.1
WIDTH = 32
PROGRESS = 0.3
SIZES = (48, 12)  # general kernel / small-scene kernel
LOG2E = 1.44269504
EYE_INSIDE = (0.05, 0.02, -0.03)


def steps_for(m):
    return 32 if m == 48 else 40


# ---- scenes -----------------------------------------------------------------------------------
def synthetic(m, seed, ball=0.6, radius_range=(0.03, 0.12), log_radius=False):
    """model.synthetic_scene restated without torch (same draws in the same order), with the ball
    and the radius law as parameters."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(m, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    rad = ball * rng.random((m, 1)) ** (1.0 / 3.0)
    lo, hi = radius_range
    r = rng.uniform(lo, hi, m)
    if log_radius:
        r = lo * (hi / lo) ** ((r - lo) / (hi - lo))
    return {
        "centers": (v * rad).astype(np.float32),
        "radius": r.astype(np.float32),
        "colors": rng.uniform(0.05, 0.95, (m, 3)).astype(np.float32),
        "light_dir": np.array([-0.5, 0.5, -1.0], np.float32),
        "ambient": np.array([0.2], np.float32),
    }


def ring_camera(i, n=7, radius=2.5, height=0.5, fov=50.0):
    """model.ring_cameras(n)[i]."""
    a = i * (2.0 * math.pi / n)
    return ([radius * math.cos(a), height * radius / 2.5, radius * math.sin(a)], [0.0, 0.0, 0.0], fov)


def admission(scene, k):
    """(fixed quantity, none quantity, fixed_ok, none_ok) by the kernel's formula."""
    c = np.asarray(scene["centers"], np.float64)
    rmax = float(np.asarray(scene["radius"], np.float64).max())
    spread = float(np.sqrt(((c - c[0]) ** 2).sum(axis=1)).max())
    kappa = k * LOG2E
    qf, qn = kappa * (rmax + spread) * 1.001, kappa * rmax * 1.001
    return qf, qn, qf <= 100.0, qn <= 30.0


def _scale_about0(sc, f):
    c = sc["centers"].astype(np.float64)
    sc["centers"] = (c[0] + f * (c - c[0])).astype(np.float32)


def _spread(c):
    c = np.asarray(c, np.float64)
    return float(np.sqrt(((c - c[0]) ** 2).sum(axis=1)).max())


# generator(m, seed, **kw) -> (scene, camera, k)
def gen_wide(m, seed):
    return synthetic(m, seed, ball=1.5, radius_range=(0.075, 0.3)), ring_camera(seed % 7), 32.0


def gen_big_radii(m, seed):
    return synthetic(m, seed, ball=0.5, radius_range=(0.3, 0.8)), ring_camera(seed % 7), 32.0


def gen_trained_like(m, seed, k=32.0):
    sc = synthetic(m, seed, ball=1.2, radius_range=(0.011, 1.2), log_radius=True)
    return sc, ring_camera(seed % 7, radius=3.2), k


def gen_fixed_edge(m, seed, q=99.0):
    sc = synthetic(m, seed)
    kappa = 32.0 * LOG2E
    f = (q / (kappa * 1.001) - float(sc["radius"].max())) / _spread(sc["centers"])
    _scale_about0(sc, f)
    return sc, ring_camera(seed % 7, radius=2.5 * f), 32.0


def gen_none_edge(m, seed, q=29.5):
    sc = synthetic(m, seed)
    rmax = q / (32.0 * LOG2E * 1.001)
    sc["radius"] = (sc["radius"].astype(np.float64) * (rmax / float(sc["radius"].max()))).astype(np.float32)
    return sc, ring_camera(seed % 7), 32.0


def gen_outlier0(m, seed, swap=False, q=99.0):
    """Sphere 0 behind and beside the scene as the camera sees it, as far out as the fixed-shift
    admission allows (bisection on its distance): it alone sets spread."""
    sc = synthetic(m, seed)
    cam = ring_camera(seed % 7, radius=3.0)
    e = np.array(cam[0]) / np.linalg.norm(cam[0])
    side = np.cross(e, [0.0, 1.0, 0.0])
    u = -0.8 * e + 0.6 * side / np.linalg.norm(side)
    target = q / (32.0 * LOG2E * 1.001) - float(sc["radius"].max())
    lo, hi = 0.0, 4.0
    c = sc["centers"].astype(np.float64)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        c[0] = mid * u
        lo, hi = (mid, hi) if _spread(c) < target else (lo, mid)
    c[0] = lo * u
    sc["centers"] = c.astype(np.float32)
    if swap:
        for key in ("centers", "radius", "colors"):
            sc[key][[0, m - 1]] = sc[key][[m - 1, 0]]
    return sc, cam, 32.0


def gen_duplicates(m, seed):
    """m/2 spheres, each twice (sphere j + m/2 = sphere j); every fourth copy 1e-3 away."""
    h = m // 2
    sc = synthetic(h, seed)
    rng = np.random.default_rng(seed + 77)
    off = rng.normal(size=(h, 3))
    off *= 1e-3 / np.linalg.norm(off, axis=1, keepdims=True)
    off[np.arange(h) % 4 != 1] = 0.0
    out = {k: np.concatenate([sc[k], sc[k]]) for k in ("centers", "radius", "colors")}
    out["centers"][h:] = (sc["centers"].astype(np.float64) + off).astype(np.float32)
    out["light_dir"], out["ambient"] = sc["light_dir"], sc["ambient"]
    return out, ring_camera(seed % 7), 32.0


def gen_eye_inside(m, seed, k=32.0):
    e = np.float32(EYE_INSIDE).astype(np.float64)
    return synthetic(m, seed), (list(e), list(e + [1.0, 0.0, 0.0]), 90.0), k


def gen_eye_on_centre(m, seed):
    sc = synthetic(m, seed)
    j = m // 3
    e = sc["centers"][j].astype(np.float64)
    return sc, (list(e), list(e + [1.0, 0.0, 0.0]), 90.0), 32.0


def gen_eye_in_big_sphere(m, seed):
    sc = synthetic(m, seed)
    sc["radius"][1] = 1.0
    c = sc["centers"][1].astype(np.float64)
    e = np.float32(c + [-0.3, 0.0, -0.4]).astype(np.float64)
    return sc, (list(e), list(c), 70.0), 32.0


def gen_dir_scaled(m, seed, scale="alt"):
    return synthetic(m, seed), ring_camera(seed % 7), 32.0


def gen_offset_small(m, seed, shift=(0.5, -0.25, 0.5)):
    sc = synthetic(m, seed)
    s = np.asarray(shift, np.float64)
    sc["centers"] = (sc["centers"].astype(np.float64) + s).astype(np.float32)
    eye, tgt, fov = ring_camera(seed % 7)
    return sc, (list(np.asarray(eye) + s), list(np.asarray(tgt) + s), fov), 32.0


GENERATORS = {
    "wide": gen_wide, "big_radii": gen_big_radii, "trained_like": gen_trained_like, "fixed_edge": gen_fixed_edge,
    "none_edge": gen_none_edge, "outlier0": gen_outlier0, "duplicates": gen_duplicates, "eye_inside": gen_eye_inside,
    "eye_on_centre": gen_eye_on_centre, "eye_in_big_sphere": gen_eye_in_big_sphere, "dir_scaled": gen_dir_scaled,
    "offset_small": gen_offset_small,
}

# (label, generator, kwargs, (fixed_ok, none_ok) the case must show, {M: seed}). A seed other than
# 0 replaced one whose derived bound broke a cap or that a mutant passed (see the module text).
SPECS = (
    ("wide", "wide", {}, (False, True), {48: 1, 12: 1}),
    ("big_radii", "big_radii", {}, (True, False), {48: 0, 12: 0}),
    ("trained_like-k32", "trained_like", {"k": 32.0}, (False, False), {48: 0, 12: 0}),
    ("trained_like-k5", "trained_like", {"k": 5.0}, (True, True), {48: 0, 12: 0}),
    ("fixed_edge99", "fixed_edge", {"q": 99.0}, (True, True), {48: 0, 12: 4}),
    ("fixed_edge101", "fixed_edge", {"q": 101.0}, (False, True), {48: 1, 12: 1}),
    ("none_edge29.5", "none_edge", {"q": 29.5}, (True, True), {48: 1, 12: 1}),
    ("none_edge30.5", "none_edge", {"q": 30.5}, (True, False), {48: 1, 12: 0}),
    ("outlier0", "outlier0", {}, (True, True), {48: 0, 12: 0}),
    ("outlier0-swapped", "outlier0", {"swap": True}, (True, True), {48: 0, 12: 0}),
    ("duplicates", "duplicates", {}, (True, True), {48: 0, 12: 0}),
    # M = 48: ray 456 grazes (t = 0.5 for 24 steps, away in the last four): the case of t_bound()'s
    # conditioned clause. M = 12: seed 1 breaks T_REL / MARGIN (t_fp32_error).
    ("eye_inside-k32", "eye_inside", {"k": 32.0}, (True, True), {48: 1, 12: 5}),
    ("eye_inside-k5", "eye_inside", {"k": 5.0}, (True, True), {48: 0, 12: 0}),
    ("eye_on_centre", "eye_on_centre", {}, (True, True), {48: 0, 12: 4}),
    ("eye_in_big_sphere", "eye_in_big_sphere", {}, (True, False), {48: 10, 12: 5}),
    ("dir_scaled-alt", "dir_scaled", {"scale": "alt"}, (True, True), {48: 0, 12: 0}),
    ("dir_scaled-0.25", "dir_scaled", {"scale": 0.25}, (True, True), {48: 0, 12: 0}),
    ("dir_scaled-0.1", "dir_scaled", {"scale": 0.1}, (True, True), {48: 0, 12: 0}),
    # (1, -0.5, 1) breaks the caps at M = 48 for every seed 0..11 (derived bounds: relative L2 1e-2 to 4e-2
    # against the cap 1e-2, light_dir 0.26 to 2.8 against 0.1): halved, as the caps require
    ("offset_small", "offset_small", {"shift": (0.5, -0.25, 0.5)}, (True, True), {48: 2, 12: 1}),
)
SPLIT_CASE = ("trained_like-k32", 300, 0)  # one M = 300 instance for RM_SPLIT on and off

RENDER_CASES = ("wide", "big_radii", "eye_inside-k32")  # rm_render (renderer.rs) against oracle.render


def build(gen, m, seed, kwargs, steps=None):
    """One case: fp32 inputs (scene, rays, upstream gradient, targets), camera or None."""
    scene, cam, k = GENERATORS[gen](m, seed, **kwargs)
    o, d = oracle.camera_rays(WIDTH, WIDTH, cam[0], cam[1], cam[2], precision="f32")
    if gen == "dir_scaled":
        s = kwargs["scale"]
        f = np.where(np.arange(len(d)) % 2 == 0, 0.5, 2.0) if s == "alt" else np.full(len(d), s)
        d = (d * f[:, None].astype(np.float32)).astype(np.float32)
        cam = None
    if steps is None:  # x2 directions triple a receding ray's distance per step: 40 steps overflow fp32
        steps = 32 if gen == "dir_scaled" else steps_for(m)
    other = GENERATORS[gen](m, seed + 1000, **kwargs)[0]
    targets = oracle.render_diff(o.astype(np.float64), d.astype(np.float64), other, steps, k, precision="f64")
    g = np.random.default_rng(seed + 10).normal(size=o.shape).astype(np.float32)
    return {"gen": gen, "M": m, "seed": seed, "scene": scene, "camera": cam, "k": float(k), "steps": steps,
            "org": o, "dir": d, "grad_out": g, "targets": targets.astype(np.float32)}


def names():
    return tuple(f"{label}-M{m}" for label, _, _, _, seeds in SPECS for m in SIZES if m in seeds)


def _spec(name):
    label, m = name.rsplit("-M", 1)
    return next(s for s in SPECS if s[0] == label), int(m)


@functools.lru_cache(maxsize=None)
def case(name):
    """A case's inputs; the arrays must not be modified."""
    if name == "split-M300":
        label, m, seed = SPLIT_CASE
        spec = next(s for s in SPECS if s[0] == label)
        c = build(spec[1], m, seed, spec[2], steps=32)
    else:
        spec, m = _spec(name)
        c = build(spec[1], m, spec[4][m], spec[2])
    c["name"] = name
    c["expect_admission"] = spec[3]
    return c


# ---- the oracle's three results, measures and bounds ----------------------------------------------
def run_oracle(c, precision, scene=None, k=None, steps=None, rays=None):
    """{out, t, bwd, train_out, loss, train} of the oracle on case c (optionally with a mutated
    scene / k / steps / rays), inputs converted to `precision`."""
    dt = np.float64 if precision == "f64" else np.float32
    o, d = (c["org"], c["dir"]) if rays is None else rays
    o, d = o.astype(dt), d.astype(dt)
    sc = c["scene"] if scene is None else scene
    k = c["k"] if k is None else k
    steps = c["steps"] if steps is None else steps
    out, t = oracle.render_diff(o, d, sc, steps, k, precision=precision, with_t=True)
    bwd = oracle.render_diff_backward(o, d, sc, steps, k, c["grad_out"].astype(dt), precision=precision)
    tout, loss, train = oracle.train_step(o, d, c["targets"].astype(dt), sc, steps, k, PROGRESS, precision=precision)
    return {"out": out, "t": t, "bwd": bwd, "train_out": tout, "loss": loss, "train": train}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The fp64 oracle's results at a case, computed once per process."""
    return run_oracle(case(name), "f64")


def existing_bound(key):
    """The suite's bound for a measure: test_gpu_parity's forward bounds, conftest's gradient ones."""
    if key[0] in ("fwd", "train_out"):
        return FWD_MAX if key[1] == "max" else FWD_MEAN
    if key == ("train", "loss"):
        return 1.0  # in units of 1e-4 |loss| + 1e-3, test_train_step_matches_oracle's bound
    mode, _, what = key
    if what == "norm":
        return GRAD_TOL
    if what == "relL2":
        return REL_L2[mode]
    return dict((f"elem{floor:g}", rel) for floor, rel in REL_ELEM[mode])[what]


def measures(got, ref):
    """{measure: figure} of results `got` (any subset of run_oracle's keys, fp32 or fp64 arrays)
    against the fp64 results `ref`. A non-finite result measures inf."""
    out = {}
    for key in ("out", "train_out"):
        if key in got:
            a = np.asarray(got[key], np.float64)
            e = np.abs(a - ref[key])
            ok = np.isfinite(a).all()
            name = "fwd" if key == "out" else key
            out[name, "max"] = float(e.max()) if ok else math.inf
            out[name, "mean"] = float(e.mean()) if ok else math.inf
    if "loss" in got:
        out["train", "loss"] = abs(float(got["loss"]) - ref["loss"]) / (1e-4 * abs(ref["loss"]) + 1e-3)
    for mode in ("bwd", "train"):
        if mode not in got:
            continue
        for group in GRAD_KEYS:
            a = np.asarray(got[mode][group], np.float64)
            if not np.isfinite(a).all():
                norm, rl2, tiers = math.inf, math.inf, [(f, math.inf) for f, _ in REL_ELEM["bwd"]]
            else:
                norm, rl2, tiers = grad_errors(a, ref[mode][group])
            out[mode, group, "norm"] = float(norm)
            if group in PER_SPHERE:
                out[mode, group, "relL2"] = float(rl2)
                for floor, err in tiers:
                    out[mode, group, f"elem{floor:g}"] = float(err)
    return out


@functools.lru_cache(maxsize=None)
def fp32_errors(name):
    """The fp32 reference-order oracle's figures against the fp64 oracle at a case."""
    return measures(run_oracle(case(name), "f32"), reference(name))


def derive_bounds(errors):
    """The bound rule: {measure: max(existing bound, MARGIN x the fp32 oracle's error)}."""
    return {key: max(existing_bound(key), MARGIN * v) for key, v in errors.items()}


def broken_caps(bnd):
    """The measures of a dict of derived bounds that break a cap."""
    bad = []
    for key, b in bnd.items():
        if len(key) == 3 and key[1] not in PER_SPHERE:
            if b > CAP_GLOBAL:
                bad.append((key, b))
        elif b > CAP_FACTOR * existing_bound(key):
            bad.append((key, b))
    return bad


@functools.lru_cache(maxsize=None)
def bounds(name):
    """{measure: max(existing bound, MARGIN x the fp32 oracle's error)} at a case."""
    return derive_bounds(fp32_errors(name))


def caps_hold(name):
    """The measures whose derived bound breaks a cap (empty: the case is accepted)."""
    return broken_caps(bounds(name))


def ratios(got, name):
    """{measure: figure / bound} of results against a case's reference and bounds."""
    b = bounds(name)
    return {key: (v / b[key]) for key, v in measures(got, reference(name)).items()}


def failures(got, name):
    return {key: r for key, r in ratios(got, name).items() if not r <= 1.0}


# ---- mutants ----------------------------------------------------------------------------------
def lit_sphere(name):
    """The sphere with the largest fp64 colour gradient: one the rays see."""
    return int(np.abs(reference(name)["bwd"]["colors"]).sum(axis=1).argmax())


def mutants(name):
    """{mutant: keyword arguments of run_oracle} -- inputs that are wrong by a little. The fp32
    oracle on each must fail the case's check against the unmutated fp64 reference."""
    c = case(name)
    j = lit_sphere(name)

    def scene_with(key, value):
        sc = {k: np.array(v, copy=True) for k, v in c["scene"].items()}
        sc[key][j] = value
        return sc

    out = {
        "radius x1.02": {"scene": scene_with("radius", c["scene"]["radius"][j] * np.float32(1.02))},
        "sphere removed": {"scene": scene_with("radius", np.float32(-100.0))},
        "centre +5e-3": {"scene": scene_with("centers", c["scene"]["centers"][j] + np.float32([5e-3, 0.0, 0.0]))},
        "k x1.02": {"k": c["k"] * 1.02},
    }
    ref = reference(name)
    o, d = c["org"].astype(np.float64), c["dir"].astype(np.float64)
    less = oracle.render_diff(o, d, c["scene"], c["steps"] - 1, c["k"], precision="f64")
    if np.abs(less - ref["out"]).max() > 2.0 * bounds(name)["fwd", "max"]:  # the rays have not settled
        out["steps - 1"] = {"steps": c["steps"] - 1}
    if c["gen"] == "dir_scaled":
        ln = np.linalg.norm(d, axis=1, keepdims=True)
        out["unit directions"] = {"rays": (c["org"], (d / ln).astype(np.float32))}
    return out


@functools.lru_cache(maxsize=None)
def mutant_distances(name):
    """{mutant: worst figure / bound of the fp32 oracle on the mutated input}; > 1 fails the check."""
    c = case(name)
    return {mut: max(ratios(run_oracle(c, "f32", **kw), name).values()) for mut, kw in mutants(name).items()}


# ---- t_march (include/raymarch.h) ------------------------------------------------------------------
T_REL = 1e-3  # test_gpu_early_exit.py::test_t_march_contract_against_oracle's bound, relative to max(1, |t|)
T_CASES = ("trained_like", "eye_inside")


def t_names():
    return tuple(n for n in names() if n.startswith(T_CASES))


def t_rel_error(t, t_ref):
    """|t - t_ref| / max(1, |t_ref|) per ray."""
    t_ref = np.asarray(t_ref, np.float64).reshape(-1)
    return np.abs(np.asarray(t, np.float64).reshape(-1) - t_ref) / np.maximum(1.0, np.abs(t_ref))


def t_error(t, name):
    """|t - t_ref| / max(1, |t_ref|) per ray against the fp64 march distance."""
    return t_rel_error(t, reference(name)["t"])


T_NOISE = 2.0 ** -24  # relative: one rounding of every input
T_AMPLIFY = 64.0  # see t_bound


@functools.lru_cache(maxsize=None)
def t_sensitivity(name):
    """Per ray, how far the fp64 march distance moves, relative to max(1, |t|), when every input
    (centres, radii, directions) is perturbed by T_NOISE relative Gaussian noise: the largest of
    eight seeded trials. A ray that hovers at a surface and leaves late doubles a perturbation with
    every step it recedes; this measures that amplification without any device."""
    c = case(name)
    o, d = c["org"].astype(np.float64), c["dir"].astype(np.float64)
    rng = np.random.default_rng(12345)
    worst = np.zeros(len(o))
    for _ in range(8):
        sc = {k: np.asarray(v, np.float64) * (1.0 + T_NOISE * rng.standard_normal(np.shape(v)))
              for k, v in c["scene"].items()}
        dn = d * (1.0 + T_NOISE * rng.standard_normal(d.shape))
        _, t = oracle.render_diff(o, dn, sc, c["steps"], c["k"], precision="f64", with_t=True)
        worst = np.maximum(worst, t_error(t, name))
    return worst


def t_bound(name):
    """Per ray bound on a march distance against the fp64 one, or between two fp32 marches that
    round differently: max(T_REL, T_AMPLIFY x t_sensitivity). The second term is the conditioning
    (include/raymarch.h, t_march). Its factor is not a measurement of the device: the reference's
    expansion form q = |p|^2 + |c|^2 - 2 p.c carries an absolute error of ~3 ulp of |p|^2 + |c|^2;
    at a sphere of radius 0.1 in a scene of extent 0.5 that is 1e-7 in q and 5e-7 in sqrt(q), i.e.
    16 roundings of the coordinates per step where t_sensitivity applies one; x MARGIN for another
    summation order. Only unseen rays may use it (the tests keep seen rays to T_REL)."""
    return np.maximum(T_REL, T_AMPLIFY * t_sensitivity(name))


# Camera mode in its default 16 x 16 tiles against array mode (rows) on the same rays: a march step's
# log-sum-exp shift is chosen per wave and the three forms agree to fp32 rounding, so a ray's
# result depends on its wave-mates by that rounding. Bound on out (values in [0, 1]): 32 ulp of 1,
# one per march step at the reference's 32 steps -- each step may round another way, and the mask
# (slope 15 / 4 per unit distance, distances of order 1) passes it on at most about one for one.
# March distances get the same figure relative to max(1, |t|), or their conditioning (t_bound's
# second term) where that is larger.
WAVE_ABS = 32.0 * 2.0 ** -23


def single_form(name):
    """Cases whose march has one shift form for every wave: the small-scene kernel (M = 12 at the
    default RM_SMALL), and scenes that refuse both cheaper forms (running maximum only). There
    camera mode keeps array mode's bits in any ray order."""
    c = case(name)
    _, _, fixed_ok, none_ok = admission(c["scene"], c["k"])
    return c["M"] == 12 or (not fixed_ok and not none_ok)


def t_fp32_error(name):
    """The fp32 oracle's worst t error: a t_march case keeps it within T_REL / MARGIN (a receding
    ray's t doubles its error every step, so a grazing ray that leaves late is ill-conditioned)."""
    return float(t_error(run_oracle(case(name), "f32")["t"], name).max())


# ---- rm_render (renderer.rs, the target renderer) -------------------------------------------------
@functools.lru_cache(maxsize=None)
def render_reference(name):
    c = case(name)
    sc = c["scene"]
    o, d = c["org"].astype(np.float64), c["dir"].astype(np.float64)
    return oracle.render(o, d, sc["centers"], sc["colors"], sc["radius"], precision="f64")


@functools.lru_cache(maxsize=None)
def render_fp32_errors(name):
    """(max, mean) error of the fp32 oracle.render against the fp64 one."""
    c = case(name)
    sc = c["scene"]
    e = np.abs(oracle.render(c["org"], c["dir"], sc["centers"], sc["colors"], sc["radius"], precision="f32")
               - render_reference(name))
    return float(e.max()), float(e.mean())


def render_bounds(name):
    """(max, mean) bounds of rm_render at a case: the same construction and cap as bounds()."""
    emax, emean = render_fp32_errors(name)
    return max(FWD_MAX, MARGIN * emax), max(FWD_MEAN, MARGIN * emean)
