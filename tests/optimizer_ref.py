"""Reference of one optimizer step (rm_optimizer_step: activation chain rule, the compute_loss
penalties of training.rs:38-82, coupled weight decay, Burn's Adam), its cases, error measures and
bounds. Shared by tests/test_optimizer_reference.py (CPU) and tests/test_gpu_optimizer.py.

reference_step is torch autograd of sum(activate(raw) * gact) + compute_loss(raw, 0, 0) -- both
from oracle/autodiff_ref.py -- then + wd raw, then Adam as model.Adam documents it:

  m' = b1 m + (1 - b1) g,  v' = b2 v + (1 - b2) g^2,
  raw' = raw - lr (m' / (1 - b1^t)) / (sqrt(v' / (1 - b2^t)) + eps)

The hyper-parameters b1 = 0.9, b2 = 0.999, eps = 1e-5, lr and wd are fp32 values in Burn and in
the kernel, so like every other input they are rounded to fp32 once and then used in the run's
dtype (1 - f32(0.999) differs from 0.001 by 1.3e-5 relative: an input, not an error). float64 is
the anchor; float32 gives the error of the same program in the kernels' precision, which is what
the bounds below are set from. `mutate` scales one term or switches one Adam variant (MUTANTS): the
CPU test uses it to show that every bound separates the right step from each wrong one.
"""
import functools
import math

import numpy as np
import torch

from oracle import autodiff_ref as ad

LR = 0.05
WD = 1e-5
SIZES = (1, 2, 9, 64, 65, 256, 257, 300, 1100)
WARM_STEPS = (2, 10, 700)  # 700: a stage of the reference loop
CHAIN_SIZES = (9, 300)
CHAIN_STEPS = 4


def f32(x):
    return float(np.float32(x))


def group_slices(m):
    return {"centers": slice(0, 3 * m), "colors": slice(3 * m, 6 * m), "radius": slice(6 * m, 7 * m),
            "light_ambient": slice(7 * m, 7 * m + 4)}


def _split(x, m):
    return {"centers": x[:3 * m].reshape(m, 3), "colors": x[3 * m:6 * m].reshape(m, 3),
            "radius": x[6 * m:7 * m].reshape(m, 1), "light_dir": x[7 * m:7 * m + 3], "ambient": x[7 * m + 3:]}


def _flat(d):
    return torch.cat([d[k].reshape(-1) for k in ("centers", "colors", "radius", "light_dir", "ambient")])


def penalty_terms(raw):
    """The four penalties of autodiff_ref.compute_loss (the radius one in its two parts), each with
    its weight: restated only so that a mutant can add (scale - 1) * term to compute_loss."""
    centers = raw["centers"]
    radii = torch.log(1.0 + torch.exp(raw["radius"]))
    m = centers.shape[0]
    reach = (centers.pow(2).sum(dim=1, keepdim=True) + 1e-6).sqrt() + radii
    c_sq = centers.pow(2).sum(dim=1, keepdim=True)
    dist = (c_sq + c_sq.t() - (centers @ centers.t()) * 2.0).clamp_min(1e-6).sqrt()
    return {
        "radius_l1": radii.abs().mean() * 0.002,
        "radius_large": torch.where(radii > 1.0, radii.pow(2), torch.zeros_like(radii)).mean() * 0.04,
        "center_l2": centers.pow(2).mean() * 0.05,
        "reach": torch.where(reach > 1.2, (reach - 1.2).pow(2), torch.zeros_like(reach)).mean() * 5.0,
        "repulsion": (dist + torch.eye(m, dtype=centers.dtype) * 100.0 + 1e-6).pow(-1.0).mean() * 0.00001,
    }


# name -> mutate argument of reference_step. Penalty terms and chain factors are scaled, the
# weight decay is scaled, "adam" names a variant of the update.
MUTANTS = {
    "repulsion x0": {"repulsion": 0.0}, "repulsion x-1": {"repulsion": -1.0}, "repulsion x2": {"repulsion": 2.0},
    "radius L1 x0": {"radius_l1": 0.0}, "radius L1 x2": {"radius_l1": 2.0},
    "large radius x0": {"radius_large": 0.0}, "large radius x2": {"radius_large": 2.0},
    "centre L2 x0": {"center_l2": 0.0},
    "reach x0": {"reach": 0.0}, "reach x1.5": {"reach": 1.5},
    "colour chain x2": {"chain_colors": 2.0}, "ambient chain x3": {"chain_ambient": 3.0},
    "radius chain x2": {"chain_radius": 2.0},
    "weight decay x0": {"wd": 0.0}, "weight decay x2": {"wd": 2.0},
    "eps 1e-8": {"adam": "eps_1e-8"}, "eps inside the root": {"adam": "eps_in_root"},
    "no bias correction": {"adam": "no_bias"}, "bias correction with step-1": {"adam": "bias_prev_step"},
    "decoupled decay": {"adam": "decoupled"}, "beta2 0.99": {"adam": "beta2_0.99"},
}
PENALTY_KEYS = ("radius_l1", "radius_large", "center_l2", "reach", "repulsion")


def _scale_grad(v, k):
    """v with its gradient scaled by k (the value is unchanged)."""
    return v.detach() + (v - v.detach()) * k


def reference_step(raw, m1, m2, gact, step, lr=LR, weight_decay=WD, with_penalties=True, dtype=torch.float64,
                   mutate=None):
    """One optimizer step on packed arrays (7M+4). Returns a dict of float64 arrays: raw, m1, m2
    (updated), act = activate(raw'), gv (the total gradient, weight decay included) and the float
    penalty (0 without penalties)."""
    mutate = dict(mutate or {})
    variant = mutate.pop("adam", None)
    n = len(raw)
    m = (n - 4) // 7
    t = lambda a: torch.tensor(np.asarray(a, np.float64)).to(dtype)  # noqa: E731
    x = t(raw).requires_grad_(True)
    p = _split(x, m)
    if "chain_radius" in mutate:  # the radius penalties go through the same sigmoid factor
        p["radius"] = _scale_grad(p["radius"], mutate["chain_radius"])
    a = ad.activate(p)
    for key in ("colors", "ambient"):
        if "chain_" + key in mutate:
            a[key] = _scale_grad(a[key], mutate["chain_" + key])
    obj = (_flat(a) * t(gact)).sum()
    penalty = 0.0
    if with_penalties:
        zero = torch.zeros((1, 3), dtype=dtype)
        pen = ad.compute_loss(p, zero, zero, 0.0)
        if any(k in mutate for k in PENALTY_KEYS):
            terms = penalty_terms(p)
            for k in PENALTY_KEYS:
                if k in mutate:
                    pen = pen + terms[k] * (mutate[k] - 1.0)
        penalty = float(pen.detach())
        obj = obj + pen
    obj.backward()
    xd = x.detach()
    wd = f32(weight_decay) * mutate.get("wd", 1.0)
    lr = f32(lr)
    b1, b2, eps = f32(0.9), f32(0.999), f32(1e-5)
    if variant == "beta2_0.99":
        b2 = f32(0.99)
    if variant == "eps_1e-8":
        eps = f32(1e-8)
    gv = x.grad if variant == "decoupled" else x.grad + wd * xd
    mm = b1 * t(m1) + (1.0 - b1) * gv
    vv = b2 * t(m2) + (1.0 - b2) * gv * gv
    tb = step - 1 if variant == "bias_prev_step" else step
    one = torch.ones((), dtype=dtype)
    c1 = one - torch.tensor(b1, dtype=dtype) ** tb
    c2 = one - torch.tensor(b2, dtype=dtype) ** tb
    if variant == "no_bias":
        c1 = c2 = one
    mh, vh = mm / c1, vv / c2
    upd = mh / (vh + eps).sqrt() if variant == "eps_in_root" else mh / (vh.sqrt() + eps)
    xn = xd - lr * upd
    if variant == "decoupled":
        xn = xn - lr * wd * xd
    act = _flat(ad.activate(_split(xn, m)))
    d = lambda v: v.detach().to(torch.float64).numpy()  # noqa: E731
    return {"raw": d(xn), "m1": d(mm), "m2": d(vv), "act": d(act), "gv": d(gv), "penalty": penalty}


def activate64(raw):
    raw = np.asarray(raw, np.float64)
    m = (len(raw) - 4) // 7
    return _flat(ad.activate(_split(torch.tensor(raw), m))).numpy()


# ---- error measures -------------------------------------------------------------------------
def rel_measure(a, b):
    """max_i |a_i - b_i| / (|b_i| + 1e-3 max |b|); inf for a non-finite a, or a != 0 where b is all 0."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    if not np.isfinite(a).all():
        return math.inf
    top = np.abs(b).max()
    if top == 0.0:
        return 0.0 if not a.any() else math.inf
    return float((np.abs(a - b) / (np.abs(b) + 1e-3 * top)).max())


def measures(got, ref, case):
    """{(measure, group): figure} of a step's results `got` (dict with raw, m1, m2, act, penalty;
    float32 or float64 arrays) against the fp64 reference `ref` of the same inputs `case`."""
    out = {}
    raw0 = np.asarray(case["raw"], np.float64)
    lr = f32(case["lr"])
    zero_moments = not np.any(case["m1"]) and not np.any(case["m2"])
    g = {k: np.asarray(got[k], np.float64) for k in ("raw", "m1", "m2", "act")}
    act64 = activate64(g["raw"]) if np.isfinite(g["raw"]).all() else np.full_like(g["raw"], np.nan)
    for name, sl in group_slices(case["M"]).items():
        if zero_moments:  # m1' = (1 - b1) gv: the device's total gradient
            out["grad", name] = rel_measure(g["m1"][sl] / (1.0 - f32(0.9)), ref["gv"][sl])
        else:
            out["m1", name] = rel_measure(g["m1"][sl], ref["m1"][sl])
        out["m2", name] = rel_measure(g["m2"][sl], ref["m2"][sl])
        du = np.abs((g["raw"][sl] - raw0[sl]) - (ref["raw"][sl] - raw0[sl])) / lr
        out["update", name] = float(du.max()) if np.isfinite(du).all() else math.inf
        da = np.abs(g["act"][sl] - act64[sl])
        out["act", name] = float(da.max()) if np.isfinite(da).all() else math.inf
    p, q = float(got["penalty"]), float(ref["penalty"])
    out["penalty", "all"] = abs(p - q) / abs(q) if q != 0.0 else (0.0 if p == 0.0 else math.inf)
    return out


# ---- bounds ---------------------------------------------------------------------------------
# Each bound is 8 times the worst figure of the float32 run of reference_step over all cases()
# and chains (the figure beside it, measured on the CPU), rounded up to 1, 2 or 5: the fp32
# reference-order error with headroom for the kernel's v_rcp / v_rsq / expf / logf (about 1 ulp
# each) and its other summation order of the repulsion row. Not taken from a GPU run.
# tests/test_optimizer_reference.py keeps the fp32 run within 1/8 of every bound and every entry of
# MUTANTS at least 4 bounds away in some case.
#  * grad / m1 / m2 (rel_measure): the worst elements are sums that cancel (g fac against the
#    penalties, the repulsion row's q = |a|^2 + |b|^2 - 2 a.b at close pairs).
#  * update (max |d raw' - d raw'_ref| / lr, absolute; the update itself is O(1)): the rounding of
#    raw' = raw - lr u, ulp(20) / 2 / lr = 1.9e-5 at the saturated parameters; elements whose
#    gradient is near Adam's eps, where du = dg eps / (|g| + eps)^2; and the colours with raw = +20,
#    whose chain factor c (1 - c) = 2e-9 is 0 in fp32 (sigmoid rounds to 1) -- without weight decay
#    their whole update, 3.3e-4, is lost in fp32.
#  * act: against activate64 of the run's own raw'. Centres and light are copies: exact.
BOUNDS = {
    "grad": {"centers": 5e-5, "colors": 1e-5, "radius": 5e-5, "light_ambient": 2e-6},  # 5.7e-6 1.1e-6 3.3e-6 1.4e-7
    "m1": {"centers": 2e-5, "colors": 5e-5, "radius": 5e-5, "light_ambient": 5e-6},  # 2.3e-6 4.6e-6 4.2e-6 5.4e-7
    "m2": {"centers": 1e-5, "colors": 5e-5, "radius": 1e-5, "light_ambient": 5e-6},  # 6.7e-7 5.0e-6 6.7e-7 3.1e-7
    "update": {"centers": 2e-4, "colors": 5e-3, "radius": 1e-3, "light_ambient": 5e-5},  # 2.2e-5 3.3e-4 1.0e-4 4.8e-6
    "act": {"centers": 0.0, "colors": 1e-6, "radius": 5e-6, "light_ambient": 2e-7},  # 0 8.2e-8 5.0e-7 1.6e-8
    "penalty": 5e-6,  # 3.0e-7
}


def bound(measure, group):
    b = BOUNDS[measure]
    return b[group] if isinstance(b, dict) else b


# ---- cases ----------------------------------------------------------------------------------
def scene(m, seed, ambient=-1.4):
    """Packed raw parameters (fp32 values): centres N(0, 0.5), raw colours N(0, 1), raw radius
    1.5 N(0, 1) with radius[0] = 2 (softplus > 1); from 9 spheres on also saturated raw colours and
    radii (-20, 0, +20 on spheres 1, 2, 3), a coincident pair (2, 4: q = 0, clamped and gated), a
    pair with q = 2^-16 (5, 6: above the clamp, it dominates their repulsion rows) and a pair with
    q = 2^-22 (7, 8: below the clamp, counted in the value, gated in the gradient). Those squares
    and products are exact in fp32, so both sides of the q >= 1e-6 gate are deterministic."""
    rng = np.random.default_rng(seed)
    c = rng.normal(scale=0.5, size=(m, 3))
    col = rng.normal(size=(m, 3))
    r = 1.5 * rng.normal(size=m)
    r[0] = 2.0
    if m >= 9:
        for s, v in ((1, -20.0), (2, 0.0), (3, 20.0)):
            col[s] = v
            r[s] = v
        c = c.astype(np.float32).astype(np.float64)
        c[4] = c[2]
        c[5] = (0.25, 0.0, 0.0)
        c[6] = (0.25 + 2.0 ** -8, 0.0, 0.0)
        c[7] = (-0.25, 0.0, 0.0)
        c[8] = (-0.25 - 2.0 ** -11, 0.0, 0.0)
    out = np.concatenate([c.ravel(), col.ravel(), r, [0.2, 1.0, -0.3], [ambient]])
    return out.astype(np.float32)


def mixed_gradient(n, rng):
    """N(0,1) * 10^U(-4,1) per element, every fifth element zero."""
    g = rng.normal(size=n) * 10.0 ** rng.uniform(-4.0, 1.0, size=n)
    g[::5] = 0.0
    return g.astype(np.float32)


def _case(name, m, raw, gact, m1=None, m2=None, step=1, wd=WD, pen=1):
    n = 7 * m + 4
    z = np.zeros(n, np.float32)
    return {"name": name, "M": m, "raw": raw, "gact": gact, "m1": z if m1 is None else m1,
            "m2": z.copy() if m2 is None else m2, "step": step, "lr": LR, "wd": wd, "pen": pen}


SEED = 7  # changed until no sphere sits near a branch threshold (check_thresholds)


@functools.lru_cache(maxsize=None)
def cases():
    """The single-step cases, in a fixed order; arrays are fp32 and must not be modified."""
    out = []
    for m in SIZES:
        n = 7 * m + 4
        rng = np.random.default_rng(1000 * SEED + m)
        raw = scene(m, 100 * SEED + m)
        gmix = mixed_gradient(n, rng)
        out.append(_case(f"zero_g-M{m}", m, raw, np.zeros(n, np.float32)))
        out.append(_case(f"mixed_g-M{m}", m, raw, gmix))
        w1 = (0.1 * rng.normal(size=n)).astype(np.float32)
        w2 = (w1.astype(np.float64) ** 2).astype(np.float32)  # the same draw: |m1| / sqrt(m2) = 1, as in a real run
        for step in WARM_STEPS:
            out.append(_case(f"warm{step}-M{m}", m, raw, gmix, w1, w2, step))
        if m in CHAIN_SIZES:  # flag coverage
            for pen, wd in ((0, 0.0), (0, WD), (1, 0.0)):
                out.append(_case(f"mixed_g-M{m}-pen{pen}-wd{wd:g}", m, raw, gmix, wd=wd, pen=pen))
                out.append(_case(f"warm10-M{m}-pen{pen}-wd{wd:g}", m, raw, gmix, w1, w2, 10, wd=wd, pen=pen))
        if m == 9:  # a saturated ambient
            out.append(_case("mixed_g-M9-ambient-20", m, scene(m, 100 * SEED + m, ambient=-20.0), gmix))
    return tuple(out)


def case(name):
    return next(c for c in cases() if c["name"] == name)


def chain(m):
    """(raw, [gact of step 1..CHAIN_STEPS]): a run from zero moments with a fresh gradient each
    step. The reference is restarted from the device's state before every step, so each step is a
    one-step comparison (elements with gv ~ 0 would make two free-running trajectories diverge)."""
    rng = np.random.default_rng(2000 * SEED + m)
    return scene(m, 100 * SEED + m), [mixed_gradient(7 * m + 4, rng) for _ in range(CHAIN_STEPS)]


def chain_case(m, k, raw, m1, m2):
    """Step k (1-based) of chain(m) from the state (raw, m1, m2) the previous step left."""
    f = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    return _case(f"chain-M{m}-step{k}", m, f(raw), chain(m)[1][k - 1], f(m1), f(m2), k)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The fp64 reference of a single-step case, computed once per process."""
    return run(case(name))


def run(c, dtype=torch.float64, mutate=None):
    return reference_step(c["raw"], c["m1"], c["m2"], c["gact"], c["step"], c["lr"], c["wd"], bool(c["pen"]),
                          dtype=dtype, mutate=mutate)


def check_thresholds(raw, margin=1e-4):
    """The condition on a case's inputs: in fp64 no sphere within `margin` of a branch threshold
    (reach = 1.2, softplus radius = 1), no pair's squared distance near the 1e-6 clamp."""
    raw = np.asarray(raw, np.float64)
    m = (len(raw) - 4) // 7
    c = raw[:3 * m].reshape(m, 3)
    rs = np.log1p(np.exp(raw[6 * m:7 * m]))
    reach = np.sqrt((c * c).sum(axis=1) + 1e-6) + rs
    q = ((c[:, None, :] - c[None, :, :]) ** 2).sum(axis=2)
    return bool((np.abs(reach - 1.2) > margin).all() and (np.abs(rs - 1.0) > margin).all()
                and not ((q > 5e-7) & (q < 2e-6)).any())
