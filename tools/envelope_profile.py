#!/usr/bin/env python3
"""The out-of-envelope parity record (profiles/rNN_envelope_parity.txt): per case of
tests/envelope_ref.py the shift admission side and the closest mutant, per measure the fp32
reference-order oracle's error against fp64 (recomputed here on the CPU), the bound, and the GPU's
worst error with its ratio to the bound, taken from the margins record that a `pytest -m gpu` session
writes (tests/conftest.py, pytest_sessionfinish).

    python3 tools/envelope_profile.py <parity_margins.json> <profiles/rNN_envelope_parity.txt>

Everything in the output file from the line NOTES on (hand-written findings) is kept.
"""
import collections
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import envelope_ref as E  # noqa: E402

NOTES = "# ==== notes (kept when this file is regenerated) ===="


def main(margins, dest):
    d = json.load(open(margins))
    gpu = collections.defaultdict(float)
    for m in d["cases"]:
        if not m["quantity"].startswith("env_") or "test_gpu_envelope" not in m["test"]:
            continue
        mm = re.search(r"\[(.*)\]", m["test"])
        name = mm.group(1) if mm else "?"
        if "test_split_march" in m["test"]:
            name = "split-M300"
        if "test_target_renderer" in m["test"]:
            mval, label = name.split("-", 1)
            name = f"{label}-M{mval}"
        gpu[name, m["quantity"]] = max(gpu[name, m["quantity"]], m["err"])

    out = []
    w = out.append
    w("# Oracle parity outside the synthetic-scene envelope: tests/envelope_ref.py's cases (32 x 32 rays).")
    w("# Per case: the shift admission quantities (kernel formula restated) and the closest mutant in bounds")
    w("# (fp32 oracle on the mutated input against the unmutated fp64 reference; > 1 fails the check).")
    w("# Per measure: the fp32 reference-order oracle's error against fp64 (CPU), the bound =")
    w("# max(existing bound, 4 x that error), the GPU's worst error over the tests of the case (array and")
    w("# camera mode, RM_SMALL default and 0, exit on and off, running-max shift) and its ratio to the bound.")
    w("# GPU figures: one MI355X, pytest -m gpu, the margins record (conftest.record_margin) of the full-suite run.")
    worst = (0.0, None, None)
    for name in E.names() + ("split-M300",):
        c = E.case(name)
        qf, qn, fo, no = E.admission(c["scene"], c["k"])
        md = E.mutant_distances(name)
        cl = min(md, key=md.get)
        w("")
        w(f"{name}: M {c['M']} steps {c['steps']} k {c['k']:g} seed {c['seed']}; kappa (rmax + spread) 1.001 = {qf:.2f} "
          f"fixed_ok {fo}; kappa rmax 1.001 = {qn:.2f} none_ok {no}; closest mutant {cl} at {md[cl]:.3g} bounds "
          f"(of {', '.join(md)})")
        err, bnd = E.fp32_errors(name), E.bounds(name)
        for key in err:
            q = "env_" + "_".join(key)
            g = gpu.get((name, q))
            r = g / bnd[key] if g is not None else None
            if r is not None and r > worst[0]:
                worst = (r, name, key)
            w(f"  {'/'.join(key):28s} fp32 {err[key]:9.3g}  bound {bnd[key]:9.3g} (existing {E.existing_bound(key):g})  "
              + (f"gpu {g:9.3g}  ratio {r:.3f}" if g is not None else "gpu -"))
        if name in E.t_names():
            g = gpu.get((name, "env_t_march"))
            w(f"  {'t_march':28s} fp32 {E.t_fp32_error(name):9.3g}  bound {E.T_REL:9.3g} (the contract's)  gpu {g:9.3g}  ratio {g / E.T_REL:.3f}")
        label = name.rsplit("-M", 1)[0]
        if label in E.RENDER_CASES:
            (emax, emean), (bmax, bmean) = E.render_fp32_errors(name), E.render_bounds(name)
            for what, e, b, ex in (("max", emax, bmax, E.FWD_MAX), ("mean", emean, bmean, E.FWD_MEAN)):
                g = gpu.get((name, "env_render_" + what))
                w(f"  {'rm_render/' + what:28s} fp32 {e:9.3g}  bound {b:9.3g} (existing {ex:g})  gpu {g:9.3g}  ratio {g / b:.3f}")
    w("")
    w(f"# worst GPU ratio: {worst[0]:.3f} at {worst[1]} {'/'.join(worst[2])}")
    for q, label in (("env_tiles_rows_out", "camera tiles against array rows, out"),
                     ("env_tiles_rows_t", "camera tiles against array rows, t (of its per-ray bound)"),
                     ("env_t_march_conditioned", "t_march of rays not proven gone (of t_bound)")):
        vals = [(v, n) for (n, qq), v in gpu.items() if qq == q]
        if vals:
            v, n = max(vals)
            w(f"# worst {label}: {v:.3g} at {n}" + (f" (bound {E.WAVE_ABS:.3g})" if q.endswith("out") else ""))
    notes = ""
    if os.path.exists(dest):
        old = open(dest).read()
        if NOTES in old:
            notes = old[old.index(NOTES):]
    with open(dest, "w") as f:
        f.write("\n".join(out) + "\n" + notes)
    print(f"worst GPU ratio {worst[0]:.3f} at {worst[1]} {'/'.join(worst[2])}; {len(out)} lines")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
