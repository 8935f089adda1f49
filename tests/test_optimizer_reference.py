"""The optimizer-step reference (tests/optimizer_ref.py) on the CPU: its inputs meet the
branch-threshold condition, its float32 run stays within 1/8 of every bound the GPU test applies,
and every mutant -- a penalty term, a chain factor or the weight decay scaled, an Adam variant --
lies at least 4 bounds away from it in some case. Together: the bounds of
tests/test_gpu_optimizer.py pass a correct fp32 step with room and fail each of these wrong ones."""
import math

import numpy as np
import pytest
import torch

import optimizer_ref as R

MUTANT_SIZES = (1, 9, 65, 300)  # both kernel paths; the other sizes add run time, not separation


def chain_steps(dtype):
    """The chains with a float32 (or float64) run of the reference standing in for the device:
    yields (case, result) per step, each step restarted from the previous result rounded to fp32."""
    for m in R.CHAIN_SIZES:
        raw, _ = R.chain(m)
        m1 = m2 = np.zeros_like(raw)
        for k in range(1, R.CHAIN_STEPS + 1):
            c = R.chain_case(m, k, raw, m1, m2)
            got = R.run(c, dtype=dtype)
            yield c, got
            raw, m1, m2 = got["raw"], got["m1"], got["m2"]


def test_inputs_avoid_branch_thresholds():
    for c in R.cases():
        assert R.check_thresholds(c["raw"]), c["name"]
    for c, _ in chain_steps(torch.float32):
        assert R.check_thresholds(c["raw"]), c["name"]


def test_cases_cover_the_issue():
    names = {c["name"] for c in R.cases()}
    for m in R.SIZES:
        assert {f"zero_g-M{m}", f"mixed_g-M{m}"} | {f"warm{s}-M{m}" for s in R.WARM_STEPS} <= names
    for c in R.cases():
        assert all(np.asarray(c[k]).dtype == np.float32 for k in ("raw", "gact", "m1", "m2"))
        if c["name"].startswith("mixed_g"):
            assert not c["gact"][::5].any() and np.count_nonzero(c["gact"]) >= len(c["gact"]) * 3 // 5
    c = R.case("zero_g-M9")["raw"].astype(np.float64)
    cen = c[:27].reshape(9, 3)
    q = lambda a, b: float(((cen[a] - cen[b]) ** 2).sum())  # noqa: E731
    assert q(2, 4) == 0.0 and q(5, 6) == 2.0 ** -16 and q(7, 8) == 2.0 ** -22
    assert list(c[54 + 1:54 + 4]) == [-20.0, 0.0, 20.0] and c[54] == 2.0
    assert R.case("mixed_g-M9-ambient-20")["raw"][-1] == -20.0


def test_float32_reference_within_an_eighth_of_every_bound(capsys):
    worst = {}
    runs = [(c, R.run(c, dtype=torch.float32), R.reference(c["name"])) for c in R.cases()]
    runs += [(c, got, R.run(c)) for c, got in chain_steps(torch.float32)]
    for c, got, ref in runs:
        for key, v in R.measures(got, ref, c).items():
            if v >= worst.get(key, (-1.0, ""))[0]:
                worst[key] = (v, c["name"])
    with capsys.disabled():
        for key in sorted(worst):
            v, name = worst[key]
            print(f"optimizer fp32 {key[0]:8s}{key[1]:14s} {v:.3g} (bound {R.bound(*key):g}) at {name}")
    for key, (v, name) in worst.items():
        assert v <= R.bound(*key) / 8.0, (key, v, R.bound(*key), name)


@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_mutant_is_at_least_four_bounds_away(mutant, capsys):
    best = (0.0, None, None)
    for c in R.cases():
        if c["M"] not in MUTANT_SIZES or (c["M"] < 2 and "repulsion" in mutant):
            continue
        ref = R.reference(c["name"])
        for key, v in R.measures(R.run(c, mutate=R.MUTANTS[mutant]), ref, c).items():
            b = R.bound(*key)
            if key[0] == "act" or b == 0.0:  # a mutant's activations are those of its own raw'
                continue
            if v / b > best[0]:
                best = (v / b, key, c["name"])
    with capsys.disabled():
        print(f"optimizer mutant {mutant:28s} {best[0]:.3g} bounds: {best[1]} at {best[2]}")
    assert best[0] >= 4.0, best


def test_adam_variants_are_separated_by_a_finite_figure():
    """`bias correction with step-1` divides by zero at step 1; it must also fail where it is finite."""
    for mutant in ("bias correction with step-1", "no bias correction", "beta2 0.99"):
        ratios = []
        for name in ("warm2-M9", "warm10-M9", "warm700-M9"):
            c = R.case(name)
            ms = R.measures(R.run(c, mutate=R.MUTANTS[mutant]), R.reference(name), c)
            ratios.append(max(v / R.bound(*k) for k, v in ms.items() if k[0] in ("update", "m2")))
        assert all(math.isfinite(r) for r in ratios) and max(ratios) >= 4.0, (mutant, ratios)


def test_reference_equals_the_closed_form_update():
    """reference_step against a hand calculation at M = 1 without penalties: gv = g fac + wd raw."""
    c = R.case("warm10-M1")
    got = R.reference_step(c["raw"], c["m1"], c["m2"], c["gact"], 10, with_penalties=False)
    x, g, m1, m2 = (c[k].astype(np.float64) for k in ("raw", "gact", "m1", "m2"))
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))  # noqa: E731
    fac = np.array([1, 1, 1, *(sig(x[3:6]) * (1 - sig(x[3:6]))), sig(x[6]), 1, 1, 1, sig(x[10]) * (1 - sig(x[10]))])
    gv = g * fac + R.f32(R.WD) * x
    b1, b2 = R.f32(0.9), R.f32(0.999)
    mm = b1 * m1 + (1 - b1) * gv
    vv = b2 * m2 + (1 - b2) * gv * gv
    xn = x - R.f32(R.LR) * (mm / (1 - b1 ** 10)) / (np.sqrt(vv / (1 - b2 ** 10)) + R.f32(1e-5))
    np.testing.assert_allclose(got["gv"], gv, rtol=1e-13, atol=0)
    np.testing.assert_allclose(got["raw"], xn, rtol=1e-13, atol=0)
    np.testing.assert_allclose(got["m2"], vv, rtol=1e-13, atol=0)
