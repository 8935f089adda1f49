#!/usr/bin/env python3
"""The constants parity record (profiles/rNN_constants_parity.txt): per case of tests/constants_ref.py
(values of rm_march.normal_eps / color_sharpness / mask_sharpness other than 1e-4 / 10 / 15) the
constants, the closest mutant, per measure the fp32 reference-order oracle's error against fp64
(recomputed here on the CPU), the bound, and the GPU's worst error with its ratio to the bound,
taken from the margins record that a `pytest -m gpu` session writes (tests/conftest.py,
pytest_sessionfinish). Then the stage, ray-gradient and camera-gradient figures, and the six taps
against their limit (include/raymarch.h, rm_march).

    python3 tools/constants_profile.py <parity_margins.json> <profiles/rNN_constants_parity.txt>

Everything in the output file from the line NOTES on (hand-written findings) is kept.
"""
import collections
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import constants_ref as C  # noqa: E402
import envelope_ref as E  # noqa: E402

NOTES = "# ==== notes (kept when this file is regenerated) ===="


def case_of(test_id, names):
    """The case name inside a parametrised test id: 'all-split-M300-1', 'msharp2-M48-RM_VALU_ONLY',
    'eps1e-3-48' (set and size as two parameters)."""
    hit = [n for n in names if test_id == n or test_id.startswith(n + "-")]
    if hit:
        return max(hit, key=len)
    m = re.match(r"^(.*)-(48|12)$", test_id)
    return f"{m.group(1)}-M{m.group(2)}" if m else test_id


def main(margins, dest):
    d = json.load(open(margins))
    names = C.names() + C.LIMIT_NAMES
    gpu = collections.defaultdict(float)
    for m in d["cases"]:
        if "test_gpu_constants" not in m["test"]:
            continue
        mm = re.search(r"\[(.*)\]", m["test"])
        name = case_of(mm.group(1), names) if mm else m["test"].rsplit("::", 1)[-1]
        gpu[name, m["quantity"]] = max(gpu[name, m["quantity"]], m["err"])

    out = []
    w = out.append
    w("# Oracle parity off the reference's shading constants: tests/constants_ref.py's cases (32 x 32 rays).")
    w("# Per case: normal_eps / color_sharpness / mask_sharpness and the closest mutant in bounds (fp32 oracle")
    w("# at the mutated constants against the unmutated fp64 reference; > 1 fails the check; 0.25 = a x 1.02")
    w("# of a constant that is 0, caught at the set CANNOT_FAIL names). Per measure: the fp32 reference-order")
    w("# oracle's error against fp64 (CPU), the bound = max(existing bound, 4 x that error), the GPU's worst")
    w("# error over the tests of the case (array and camera mode, RM_SMALL default and 0, RM_SPLIT 1 and 0,")
    w("# running-max shift, vector-unit march) and its ratio to the bound. The reference is the oracle's")
    w("# six-tap normal; for limit-M48 / limit-M12 (normal_eps = 1e-2) its limit normal.")
    w("# GPU figures: one MI355X, pytest -m gpu, the margins record (conftest.record_margin).")
    worst = (0.0, None, None)
    for name in names:
        c = C.case(name)
        w("")
        head = (f"{name}: M {c['M']} steps {c['steps']} k {c['k']:g} seed {c['seed']} normal {c['normal']}; "
                f"eps {c['consts'][0]:.3g} csharp {c['consts'][1]:g} msharp {c['consts'][2]:g}")
        if name not in C.LIMIT_NAMES:
            md = C.mutant_distances(name)
            cl = min(md, key=md.get)
            head += f"; closest mutant {cl} at {md[cl]:.3g} bounds (of {', '.join(md)})"
        w(head)
        err, bnd = C.fp32_errors(name), C.bounds(name)
        for key in err:
            g = gpu.get((name, "const_" + "_".join(key)))
            r = g / bnd[key] if g is not None else None
            if r is not None and r > worst[0]:
                worst = (r, name, "/".join(key))
            w(f"  {'/'.join(key):28s} fp32 {err[key]:9.3g}  bound {bnd[key]:9.3g} (existing {E.existing_bound(key):g})  "
              + (f"gpu {g:9.3g}  ratio {r:.3f}" if g is not None else "gpu -"))
        g = gpu.get((name, "const_t_march"))
        t32 = float(E.t_rel_error(C.run_oracle(c, "f32")["t"], C.reference(name)["t"])[C.seen(name)].max())
        w(f"  {'t_march (seen rays)':28s} fp32 {t32:9.3g}  bound {E.T_REL:9.3g} (the contract's)  "
          + (f"gpu {g:9.3g}  ratio {g / E.T_REL:.3f}" if g is not None else "gpu -"))
        if g is not None and g / E.T_REL > worst[0]:
            worst = (g / E.T_REL, name, "t_march")
        sb, s32 = C.stage_bounds(name), C.stage_errors(C._debug(c, "f32"), name)
        for st in C.STAGES:
            g = gpu.get((name, "const_stage_" + st))
            if g is not None:
                w(f"  {'stage/' + st:28s} fp32 {s32[st]:9.3g}  bound {sb[st]:9.3g} (existing {E.FWD_MAX:g})  gpu {g:9.3g}  "
                  f"ratio {g / sb[st]:.3f}")
                if g / sb[st] > worst[0]:
                    worst = (g / sb[st], name, "stage/" + st)
        for q in sorted({qq for (n, qq) in gpu if n == name and qq.startswith(("const_raygrad", "const_cam"))}):
            w(f"  {q[6:]:28s} gpu {gpu[name, q]:9.3g}")
    w("")
    w("# camera-pose gradients of the finish kernel's segment cases and the 130-view call (bound 3e-3):")
    for (n, q), v in sorted(gpu.items()):
        if n not in names and q.startswith("const_cam"):
            w(f"  {n:40s} {q[6:]:12s} gpu {v:9.3g}  ratio {v / 3e-3:.3f}")
    w("")
    w(f"# worst GPU ratio: {worst[0]:.3f} at {worst[1]} {worst[2]}")
    w("")
    w("# the six taps against their limit (the kernels' normal), fp64, |out(taps) - out(limit)| max / mean")
    w("# on the M = 48 cases at k = 32; the forward bounds are 1e-3 / 1e-5:")
    for name in ("limit-M48", "eps1e-3-M48", "all-M48"):
        w(f"  {name:14s} " + "  ".join(f"eps {eps:g}: {a:.1e} / {b:.1e}" for eps in C.GAP_EPS
                                       for a, b in [C.case_gap(name, eps)["out"]]))
    notes = ""
    if os.path.exists(dest):
        old = open(dest).read()
        if NOTES in old:
            notes = old[old.index(NOTES):]
    with open(dest, "w") as f:
        f.write("\n".join(out) + "\n" + notes)
    print(f"worst GPU ratio {worst[0]:.3f} at {worst[1]} {worst[2]}; {len(out)} lines")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
