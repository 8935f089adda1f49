"""Oracle-parity cases at values of rm_march.normal_eps / color_sharpness / mask_sharpness other than
the reference's 1e-4 / 10 / 15, and the bounds they are checked with. Shared by
tests/test_constants_reference.py (CPU) and tests/test_gpu_constants.py. The scenes, the camera, the
measures and the bound rule are envelope_ref's (imported, not copied): a bound is max(the suite's
existing bound, MARGIN x the fp32 reference-order oracle's error against the fp64 oracle at the
case), under the same two caps.

The fp64 reference is the oracle with the reference's own six-tap normal (normal="taps") at the
case's constants. The kernels do not evaluate the taps: their differentiable modes use the taps'
limit as eps -> 0, f = 2 eps grad D (include/raymarch.h, rm_march.normal_eps), which deviates from
the taps as (k eps)^2. TAPS_LIMIT_K_EPS is the largest k * normal_eps at which the cases hold the
kernels to the taps reference; the LIMIT_NAMES cases beyond it (eps = 1e-2 at k = 32) hold them to the
oracle's normal="limit" form, and taps_limit_gap() measures the gap between the two forms.

Receding rays: with mask_sharpness 0 (mask 0.5 everywhere) or 2 (mask > 0 out to D = 45) a ray that
has left the scene stays visible while it doubles its distance every step, and fp32 itself loses
the tap differences and the sphere differences far out. Those sets march STEPS_VISIBLE steps (the
largest count <= 12 at which the fp32 oracle alone keeps every derived bound inside the caps).
"""
import functools

import numpy as np

import envelope_ref as E
from oracle import oracle

DEFAULT = (1e-4, 10.0, 15.0)  # scene.rs:91, renderer_diff.rs:74, renderer_diff.rs:88
FIELDS = ("normal_eps", "color_sharpness", "mask_sharpness")

# name -> (normal_eps, color_sharpness, mask_sharpness)
SETS = {
    "eps1e-3": (1e-3, 10.0, 15.0),
    "eps1e-5": (1e-5, 10.0, 15.0),
    "csharp3": (1e-4, 3.0, 15.0),
    "csharp40": (1e-4, 40.0, 15.0),
    "csharp0": (1e-4, 0.0, 15.0),   # uniform colour weights
    "msharp2": (1e-4, 10.0, 2.0),   # gone_d = 45: the image is not 0 on missed rays
    "msharp60": (1e-4, 10.0, 60.0),
    "msharp0": (1e-4, 10.0, 0.0),   # mask 0.5 everywhere, every ray seeded, the exit never armed
    "all": (1e-3, 25.0, 6.0),       # the only set in which a swap of two fields shows
}
TAPS_LIMIT_K_EPS = 0.032  # k * normal_eps up to which the kernels are held to the taps reference
LIMIT_EPS = 1e-2          # beyond it: the limit-normal contract, k = 32

# the sets whose receding rays stay visible: steps instead of envelope_ref.steps_for (module text).
# msharp0 at 12 steps: no seed of 0..15 keeps the M = 12 bounds inside the caps (two do at M = 48); at 10
# steps seeds 4, 5, 11 and 12 do at both sizes (ring cameras 4 and 5).
STEPS_VISIBLE = {"msharp0": 10, "msharp2": 12}

# (label, set, {M: seed}, extra): extra = k. A seed other than 0 replaced one whose derived bound
# broke a cap or that a mutant passed (test_constants_reference.py fails until both hold):
#   eps1e-5   the fp32 taps at 1e-5 are noisy (tap difference 2e-5 against 1e-7 of rounding in D), and
#             light_dir's gradient is a cancelling sum over rays: seeds 0..2 at M = 48 and seed 0 at
#             M = 12 break CAP_GLOBAL on it; seed 0 at M = 12 also passes the normal_eps x 1.02 mutant
#   msharp2   seed 0 at M = 12 breaks CAP_GLOBAL on light_dir
#   msharp0   see STEPS_VISIBLE
_SEEDS = {"eps1e-5": {48: 3, 12: 1}, "msharp2": {48: 0, 12: 1}, "msharp0": {48: 5, 12: 5}}
SPECS = tuple((name, name, _SEEDS.get(name, {48: 0, 12: 0}), {}) for name in SETS) + (
    ("all-k5", "all", {48: 0}, {"k": 5.0}),
    ("all-split", "all", {300: 0}, {}),
    ("msharp2-split", "msharp2", {300: 0}, {}),
)
SPLIT_NAMES = ("all-split-M300", "msharp2-split-M300")
LIMIT_NAMES = ("limit-M48", "limit-M12")
RAYGRAD_SETS = ("eps1e-3", "csharp3", "msharp2", "all")


def consts_kw(consts):
    return dict(zip(FIELDS, consts))


def names():
    return tuple(f"{label}-M{m}" for label, _, seeds, _ in SPECS for m in seeds)


def set_of(name):
    """The constant set's name of a case."""
    if name in LIMIT_NAMES:
        return "limit"
    label = name.rsplit("-M", 1)[0]
    return next(s[1] for s in SPECS if s[0] == label)


@functools.lru_cache(maxsize=None)
def case(name):
    """A case's inputs (envelope_ref.build's keys plus consts and normal); not to be modified."""
    label, m = name.rsplit("-M", 1)
    m = int(m)
    if name in LIMIT_NAMES:
        cset, consts, seed, extra, normal = "limit", (LIMIT_EPS,) + DEFAULT[1:], 0, {}, "limit"
    else:
        _, cset, seeds, extra = next(s for s in SPECS if s[0] == label)
        consts, seed, normal = SETS[cset], seeds[m], "taps"
    scene = E.synthetic(m, seed)
    cam = E.ring_camera(seed % 7)
    k = float(extra.get("k", 32.0))
    steps = STEPS_VISIBLE.get(cset, 32 if m == 300 else E.steps_for(m))
    o, d = oracle.camera_rays(E.WIDTH, E.WIDTH, cam[0], cam[1], cam[2], precision="f32")
    targets = oracle.render_diff(o.astype(np.float64), d.astype(np.float64), E.synthetic(m, seed + 1000), steps, k,
                                 precision="f64", normal=normal, **consts_kw(consts))
    g = np.random.default_rng(seed + 10).normal(size=o.shape).astype(np.float32)
    return {"name": name, "set": cset, "M": m, "seed": seed, "scene": scene, "camera": cam, "k": k, "steps": steps,
            "consts": tuple(float(np.float32(v)) for v in consts), "normal": normal, "org": o, "dir": d, "grad_out": g,
            "targets": targets.astype(np.float32)}


# ---- the oracle's results, measures and bounds ----------------------------------------------------
def run_oracle(c, precision, consts=None, normal=None):
    """envelope_ref.run_oracle's keys on case c at its constants (or `consts` / `normal`)."""
    dt = np.float64 if precision == "f64" else np.float32
    o, d = c["org"].astype(dt), c["dir"].astype(dt)
    kw = dict(consts_kw(c["consts"] if consts is None else consts), normal=c["normal"] if normal is None else normal,
              precision=precision)
    sc, steps, k = c["scene"], c["steps"], c["k"]
    out, t = oracle.render_diff(o, d, sc, steps, k, with_t=True, **kw)
    bwd = oracle.render_diff_backward(o, d, sc, steps, k, c["grad_out"].astype(dt), **kw)
    tout, loss, train = oracle.train_step(o, d, c["targets"].astype(dt), sc, steps, k, E.PROGRESS, **kw)
    return {"out": out, "t": t, "bwd": bwd, "train_out": tout, "loss": loss, "train": train}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The fp64 oracle's results at a case (taps normal; limit normal for LIMIT_NAMES)."""
    return run_oracle(case(name), "f64")


@functools.lru_cache(maxsize=None)
def fp32_errors(name):
    return E.measures(run_oracle(case(name), "f32"), reference(name))


@functools.lru_cache(maxsize=None)
def bounds(name):
    return E.derive_bounds(fp32_errors(name))


def caps_hold(name):
    return E.broken_caps(bounds(name))


def ratios(got, name):
    b = bounds(name)
    return {key: v / b[key] for key, v in E.measures(got, reference(name)).items()}


def failures(got, name):
    return {key: r for key, r in ratios(got, name).items() if not r <= 1.0}


def seen(name):
    """The rays the fp64 reference sees (mask above 1e-3): the rays of the t_march and the stage checks."""
    return debug_reference(name)[:, 10] > 1e-3


def _debug(c, precision):
    dt = np.float64 if precision == "f64" else np.float32
    return oracle.render_diff_debug(c["org"].astype(dt), c["dir"].astype(dt), c["scene"], c["steps"], c["k"],
                                    precision=precision, normal=c["normal"], **consts_kw(c["consts"]))


@functools.lru_cache(maxsize=None)
def debug_reference(name):
    """render_diff_debug in fp64 at a case: [N,24] in the layout of rm_debug_intermediates."""
    return _debug(case(name), "f64")


STAGES = {"lighting": slice(5, 6), "mix": slice(6, 9), "mask": slice(10, 11)}


def stage_errors(dbg, name):
    """{stage: max |dbg - fp64| over the seen rays} of a [N,24] intermediates array."""
    ref, rows = debug_reference(name), seen(name)
    a = np.asarray(dbg, np.float64)
    return {st: (float(np.abs(a[rows, cols] - ref[rows, cols]).max()) if np.isfinite(a[rows, cols]).all() else np.inf)
            for st, cols in STAGES.items()}


@functools.lru_cache(maxsize=None)
def stage_bounds(name):
    """The bound rule on the stages (values of order 1, like the image): max(FWD_MAX, MARGIN x fp32)."""
    err = stage_errors(_debug(case(name), "f32"), name)
    return {st: max(E.FWD_MAX, E.MARGIN * v) for st, v in err.items()}


# ---- mutants ----------------------------------------------------------------------------------
def mutants(name):
    """{mutant: constants} -- the case's constants wrong in one way: a field ignored (its default in
    its place, where that differs), colour and mask sharpness swapped (`all`), a field x 1.02. The
    fp32 oracle on each must fail the case's check against the unmutated fp64 reference, except
    the ones CANNOT_FAIL names."""
    cs = case(name)["consts"]
    out = {}
    for i, field in enumerate(FIELDS):
        if cs[i] != float(np.float32(DEFAULT[i])):
            out[f"{field} ignored"] = cs[:i] + (DEFAULT[i],) + cs[i + 1:]
        out[f"{field} x1.02"] = cs[:i] + (cs[i] * 1.02,) + cs[i + 1:]
    if case(name)["set"] == "all":
        out["sharpnesses swapped"] = (cs[0], cs[2], cs[1])
    return out


# A x 1.02 mutant that cannot fail a set by construction, and the set that catches the same mutant.
CANNOT_FAIL = {
    ("csharp0", "color_sharpness x1.02"): "csharp3",  # 1.02 x 0 = 0: the mutant is the case itself
    ("msharp0", "mask_sharpness x1.02"): "msharp2",
}


@functools.lru_cache(maxsize=None)
def mutant_distances(name):
    """{mutant: worst figure / bound of the fp32 oracle at the mutated constants}; > 1 fails the check."""
    c = case(name)
    return {mut: max(ratios(run_oracle(c, "f32", consts=cs), name).values()) for mut, cs in mutants(name).items()}


# ---- the six taps against their limit -----------------------------------------------------------------
GAP_EPS = (1e-4, 1e-3, 3e-3, 1e-2, 3e-2)


def taps_limit_gap(o, d, scene, steps, k, eps, csharp=DEFAULT[1], msharp=DEFAULT[2]):
    """The fp64 oracle with the six taps against the oracle with their limit at normal_eps = eps on
    the same rays: {"ndotl": (max, mean) of mask |n.l(taps) - n.l(limit)|, "out": (max, mean) of
    |out(taps) - out(limit)|}."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    kw = dict(consts_kw((eps, csharp, msharp)), precision="f64")
    a = oracle.render_diff_debug(o, d, scene, steps, k, normal="taps", **kw)
    b = oracle.render_diff_debug(o, d, scene, steps, k, normal="limit", **kw)
    ndl = a[:, 10] * np.abs(a[:, 11] - b[:, 11])
    img = np.abs(a[:, 6:9] * a[:, 5:6] * a[:, 10:11] - b[:, 6:9] * b[:, 5:6] * b[:, 10:11])
    return {"ndotl": (float(ndl.max()), float(ndl.mean())), "out": (float(img.max()), float(img.mean()))}


def case_gap(name, eps):
    c = case(name)
    return taps_limit_gap(c["org"], c["dir"], c["scene"], c["steps"], c["k"], eps, *c["consts"][1:])
