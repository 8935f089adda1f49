"""CPU tests of the restatement behind the view-dependent colour's GPU tests (tests/sh_ref.py): it is
render_diff when the coefficients are zero, the header's analytic backward is its autograd, the committed
parity cases keep clear of the clamp's kink, and a degree-1 fit explains a view-dependent target that
colours alone cannot."""
import numpy as np
import pytest
import torch

import sh_ref as R
from oracle import autodiff_ref as A


def test_zero_coefficients_are_render_diff_bit_for_bit():
    """sh = 0 (and no coefficients at all): autodiff_ref.render_diff's fp64 output, torch.equal."""
    for name in ("m3_d1", "m33_d2"):
        c = R.case(name)
        o, d, par = R.tensors(c, torch.float64)
        ref = A.render_diff(o, d, par["centers"], par["colors"], par["radius"], par["light_dir"], par["ambient"], c["k"],
                            c["steps"], **R.CONSTS)
        for sh in (torch.zeros_like(par["sh"]), par["sh"][:, :0, :]):
            out = R.render_t(o, d, par["centers"], par["colors"], sh, par["radius"], par["light_dir"], par["ambient"],
                             c["k"], c["steps"], **R.CONSTS)
            assert torch.equal(out, ref), name
        assert not torch.equal(R.render_t(o, d, par["centers"], par["colors"], par["sh"], par["radius"], par["light_dir"],
                                          par["ambient"], c["k"], c["steps"], **R.CONSTS), ref)


def scaled(c):
    """The case with every other direction 1.25 long: Y must come from d / |d|."""
    d = np.array(c["dir"])
    d[1::2] *= np.float32(1.25)
    return dict(c, dir=d)


@pytest.mark.parametrize("name", ["m3_d1", "m3_d2", "m33_d2", "m48_d1"])
def test_analytic_formulas_are_the_restatements_autograd(name):
    """The header's formulas equal fp64 autograd of the restatement to 1e-9 relative, on unit and on scaled
    directions."""
    for c in (R.case(name), scaled(R.case(name))):
        n = 300
        ref = R.run(c, torch.float64, n, c["grad_out"])
        got = R.analytic(c, c["grad_out"], n)
        for q in ("out",) + R.GRADS:
            e = R.rel_err(got[q], ref[q])
            print(f"sh analytic vs autograd {name} {q}: {e:.3e}")
            assert e <= 1e-9, (name, q, e)


@pytest.mark.parametrize("name", ["m33_d2", "m48_d1"])
def test_planted_faults_break_the_analytic_formulas(name):
    """Each switch of sh_ref.analytic moves the gradients it touches off the autograd by far more than the
    1e-9 the formulas are held to (scenes where the clamp is exercised, directions that are not all unit)."""
    c = scaled(R.case(name))
    ref = R.run(c, torch.float64, 300, c["grad_out"])
    band = 1 if c["degree"] == 1 else 5
    for fault, hit in (({"no_indicator": True}, ("colors", "sh")), ({"unnormalised": True}, ("sh", "out")),
                       ({"flip_band": band}, ("sh", "out")), ({"col_in_delta": True}, ("centers", "radius"))):
        bad = R.analytic(c, c["grad_out"], 300, **fault)
        worst = {q: R.rel_err(bad[q], ref[q]) for q in hit}
        print(f"sh analytic fault {name} {fault}: {worst}")
        assert all(v > 1e-6 for v in worst.values()), (name, fault, worst)


@pytest.mark.parametrize("name", sorted(R.PARITY_CASES))
def test_kink_condition_holds_for_the_committed_cases(name):
    """A condition on the inputs, not a tolerance: no (ray, sphere, channel) of a GPU parity case has
    |col + sh . Y| < 1e-5 with w_j mu >= 1e-4 in the fp64 restatement, so fp32 and fp64 make the same clamp
    decisions wherever they matter. The clamp is exercised all the same."""
    c = R.PARITY_CASES[name]()
    near, clamped = R.kinks(c)
    print(f"sh kinks {name}: {near} near the clamp, {100 * clamped:.1f} % of the weighted triples clamped")
    assert near == 0, (name, near)
    if c["scene"]["centers"].shape[0] >= 33 and np.any(c["sh"]):
        assert clamped > 0.05, (name, clamped)


def test_fit_demonstration():
    """Colours and degree-1 coefficients fitted to a view-dependent target end below colours alone (fp64
    restatement, Adam; no fixed threshold)."""
    c, target = R.fit_problem()
    like = torch.zeros((), dtype=torch.float64)
    both = R.fit_run(R.fit_restatement(), c, target, True, like)
    alone = R.fit_run(R.fit_restatement(), c, target, False, like)
    print(f"sh fit: colours and sh {both:.3e}, colours alone {alone:.3e}")
    assert both < alone, (both, alone)
