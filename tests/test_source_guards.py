"""CPU guards on the kernel sources for the bit-level pins of DESIGN.md §5.3.

The reference loop's trajectory (tests/test_gpu_trajectory.py) once changed with edits meant to be
bit-identical because the light-direction gradient was compiled with FP contraction on, so its
fusion followed the surrounding code (profiles/r07a_r06ao_cause.txt). These tests keep the helpers
that feed the trajectory -- the light-direction unit vector and gradient, the activation, the
repulsion rows and the optimizer's two halves -- compiled with contraction off, and keep every
light-direction gradient (the general kernel's reductions and the small kernel's final block)
going through the one helper. A GPU run is still what pins the bits (test_gpu_trajectory.py);
these catch the source change that would move them before it reaches the GPU.
"""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "burn_raymarching_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _body(src, signature):
    """The text of the function whose definition starts with `signature`, up to its closing brace."""
    i = src.index(signature)
    j = src.index("{", i)
    depth = 0
    for k in range(j, len(src)):
        if src[k] == "{":
            depth += 1
        elif src[k] == "}":
            depth -= 1
            if depth == 0:
                return src[j:k + 1]
    raise AssertionError(f"unbalanced braces after {signature}")


@pytest.mark.parametrize("signature", [
    "__device__ __forceinline__ float light_unit(",
    "__device__ __forceinline__ float light_grad(",
    "__device__ __forceinline__ float activate_elem(",
    "__device__ __forceinline__ void repulsion_row(",
    "__device__ __forceinline__ ElemPre optimizer_pre(",
    "__device__ __forceinline__ void optimizer_apply(",
])
def test_trajectory_helpers_compile_without_contraction(signature):
    # the helpers live in rm_kernels.hip and in the headers it includes (one translation unit)
    body = _body(_src("rm_kernels.hip") + _src("rm_reduce.h"), signature)
    first = body.split("\n", 2)[1].strip()
    assert first == "#pragma clang fp contract(off)", f"{signature} must open with contraction off"


def _proof_constants():
    """{name: (type, value)} of the `constexpr <type> k... = <expr>;` lines of csrc/rm_proof.h, where <expr> is a
    literal or a sum or product of literals and names defined above it. The values are what the compiler gets: a
    float's literal is rounded to float32 (sums and products of floats are not formed in the header)."""
    import numpy as np
    number = r"\d+\.?\d*(?:[eE][-+]?\d+)?|\.\d+(?:[eE][-+]?\d+)?"
    out = {}
    for ctype, name, expr in re.findall(r"^constexpr\s+(int|float|double)\s+(k\w+)\s*=\s*([^;]+);", _src("rm_proof.h"), re.M):
        tokens = re.findall(rf"\s*(k\w+|(?:{number})f?|[-+*()])", expr)
        assert "".join(tokens) == re.sub(r"\s+", "", expr), f"{name}: not a sum or product of literals and names: {expr}"
        terms = [str(out[t][1]) if t in out else t.rstrip("f") for t in tokens]
        value = eval("".join(terms), {"__builtins__": {}})  # numbers, + - * and parentheses only (the assert above)
        if ctype == "float":
            assert len(tokens) == 1, f"{name}: a float is a literal here"
            value = float(np.float32(value))
        out[name] = (ctype, int(value) if ctype == "int" else value)
    return out


def test_cpu_model_has_the_headers_margins():
    """tests/escape_ref.py restates the escape proof under rm_proof.h's names (kTileConeRel -> TILE_CONE_REL): every
    constant of the header is a module-level name of the model with the same value -- the lattice's size, margin and
    give-up step, every allowance of the ledger, the derived figures -- and the model's float32 uses see the
    float32 the kernels see."""
    import numpy as np
    import escape_ref
    consts = _proof_constants()
    wanted = {"kProofMinSpheres", "kLatticeN", "kLatticeMargin", "kProofMinStep", "kMarchAbs", "kBoundStepAbs", "kRadiusRel",
              "kEscapeRel", "kProofRel", "kProofMaxMagnitude", "kLatticeHalfDiag", "kLatticeCellRel", "kLatticeKernelAbs",
              "kTileRootRel", "kTileLatticeRel", "kTileRoundAbs", "kTileConeRel", "kTileConeAbs", "kTileRecedeRel", "kBallAbs",
              "kTileLatticeAbs", "kProofDistUp"}
    assert wanted <= set(consts), wanted - set(consts)
    for name, (ctype, value) in consts.items():
        mirror = re.sub(r"(?<=[a-z0-9])(?=[A-Z])", "_", name[1:]).upper()
        assert hasattr(escape_ref, mirror), f"{name}: tests/escape_ref.py has no {mirror}"
        got = getattr(escape_ref, mirror)
        if ctype == "float":  # the model's literal, as the kernel's fp32 has it
            got = float(np.float32(got))
        assert got == value and isinstance(got, int) == (ctype == "int"), (name, value, mirror, got)
    # the derived figures are what their parts say, in the safe direction (the header's static_asserts)
    assert consts["kBallAbs"][1] == consts["kMarchAbs"][1] + consts["kBoundStepAbs"][1] == 2e-3
    assert consts["kTileLatticeAbs"][1] == 3.1e-3
    assert consts["kProofDistUp"][1] * (1.0 - consts["kProofRel"][1]) >= 1.0


def test_light_direction_gradient_has_one_definition():
    """Every light-direction gradient is light_grad's: no kernel forms (r - ln proj) / len itself."""
    for name in ("rm_kernels.hip", "rm_reduce.h", "rm_small.h"):
        src = _src(name)
        # the Jacobian of l / |l| written out anywhere but in light_grad
        body = _body(src, "__device__ __forceinline__ float light_grad(") if "float light_grad(" in src else ""
        rest = src.replace(body, "")
        assert not re.search(r"-\s*\w+\s*\*\s*proj\s*\)\s*/", rest), name
    assert "light_grad(" in _src("rm_small.h")
