"""rm_optimizer_step[_f16] against the fp64 reference of tests/optimizer_ref.py, on both kernel
paths: rm_optimizer_small (one block, M <= 64) and rm_penalty_pairs + rm_optimizer_kernel
(RM_OPT_SMALL=0, and every M > 64). Every case of optimizer_ref.cases() and both chains; the
measures and bounds are optimizer_ref's (set from the reference's own float32 error on the CPU,
tests/test_optimizer_reference.py, which also shows that each bound fails a step with one term
wrong). Around each call: act_out equals rm_scene_activate of the updated parameters bit for bit,
the gradient is left as it was, and nothing is written outside the buffers that were passed."""
import ctypes

import numpy as np
import pytest

import optimizer_ref as R
from conftest import gpu_available, record_margin

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

GUARD = 12345.0
SMALL_MAX_M = 64  # kOptSmallMaxM: up to here RM_OPT_SMALL chooses the path


@pytest.fixture(scope="module")
def rm():
    import torch
    from burn_raymarching_amd import _build
    _build.build_lib()
    from burn_raymarching_amd import render
    torch.cuda.init()
    return render.context()


def paths(m):
    return ("1", "0") if m <= SMALL_MAX_M else ("1",)


def gpu_step(ctx, c, *, f16=False, with_penalty_out=True):
    """One rm_optimizer_step[_f16] call on case c's inputs. The buffers are slices of one arena
    filled with GUARD, 64 guard words before and after each: returns the results as numpy arrays
    after checking the guard words, the gradient and act_out == rm_scene_activate(raw')."""
    import torch
    m = c["M"]
    n = 7 * m + 4
    slot = (n + 63) // 64 * 64 + 64
    names = ("raw", "m1", "m2", "act", "gact", "act2", "penalty")
    arena = torch.full((64 + slot * len(names),), GUARD, device="cuda")
    used = torch.zeros(arena.numel(), dtype=torch.bool, device="cuda")
    buf = {}
    for k, name in enumerate(names):
        size = 1 if name == "penalty" else n
        buf[name] = arena[64 + k * slot:64 + k * slot + size]
        if name != "penalty" or with_penalty_out:
            used[64 + k * slot:64 + k * slot + size] = True
    for name in ("raw", "m1", "m2", "gact"):
        buf[name].copy_(torch.from_numpy(c[name]))
    colh = torch.full((3 * m + 64,), GUARD, dtype=torch.float16, device="cuda") if f16 else None
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    args = [ctx.handle, p(buf["raw"]), p(buf["gact"]), p(buf["m1"]), p(buf["m2"]), m, c["step"], float(c["lr"]),
            float(c["wd"]), int(c["pen"]), p(buf["penalty"]) if with_penalty_out else None, p(buf["act"])]
    if f16:
        ctx.check(ctx._lib.rm_optimizer_step_f16(*args, p(colh)), "rm_optimizer_step_f16")
    else:
        ctx.check(ctx._lib.rm_optimizer_step(*args), "rm_optimizer_step")
    ctx.check(ctx._lib.rm_scene_activate(ctx.handle, p(buf["raw"]), m, p(buf["act2"])), "rm_scene_activate")
    torch.cuda.synchronize()
    assert bool((arena[~used] == GUARD).all()), "a write outside the buffers passed (or to a NULL loss_penalty)"
    out = {k: v.cpu().numpy().copy() for k, v in buf.items()}
    assert np.array_equal(out["gact"], c["gact"]), "the gradient was modified"
    assert np.array_equal(out["act"].view(np.uint32), out["act2"].view(np.uint32)), "act_out != rm_scene_activate(raw')"
    out["penalty"] = float(out["penalty"][0]) if with_penalty_out else None
    if f16:
        h = colh.cpu().numpy()
        assert (h[3 * m:] == np.float16(GUARD)).all()
        out["colh"] = h[:3 * m]
    return out


def check(got, ref, c, label):
    ms = R.measures(got, ref, c)
    worst = {}
    for (measure, group), v in ms.items():
        b = R.bound(measure, group)
        record_margin(f"opt_{measure}_{group}", v, b)
        r = v / b if b > 0 else (0.0 if v == 0 else float("inf"))
        if r >= worst.get(measure, (-1.0,))[0]:
            worst[measure] = (r, group, v)
    print(f"optimizer parity {label}: " + ", ".join(f"{k} {v[2]:.3g} ({v[1]}, {v[0]:.2f} of bound)"
                                                    for k, v in sorted(worst.items())))
    for (measure, group), v in ms.items():
        assert v <= R.bound(measure, group), (label, measure, group, v, R.bound(measure, group))


SINGLE = [(c["name"], path) for c in R.cases() for path in paths(c["M"])]


@pytest.mark.parametrize("name,path", SINGLE, ids=[f"{n}-small{p}" for n, p in SINGLE])
def test_step_matches_reference(rm, monkeypatch, name, path):
    monkeypatch.setenv("RM_OPT_SMALL", path)
    c = R.case(name)
    check(gpu_step(rm, c), R.reference(name), c, f"{name} RM_OPT_SMALL={path}")


CHAINS = [(m, path) for m in R.CHAIN_SIZES for path in paths(m)]


@pytest.mark.parametrize("m,path", CHAINS, ids=[f"M{m}-small{p}" for m, p in CHAINS])
def test_chain_matches_reference_step_by_step(rm, monkeypatch, m, path):
    """Four steps with a fresh gradient each; the reference restarts from the device's state."""
    monkeypatch.setenv("RM_OPT_SMALL", path)
    raw, _ = R.chain(m)
    m1 = m2 = np.zeros_like(raw)
    for k in range(1, R.CHAIN_STEPS + 1):
        c = R.chain_case(m, k, raw, m1, m2)
        assert R.check_thresholds(c["raw"]), "a sphere drifted onto a branch threshold: change optimizer_ref.SEED"
        got = gpu_step(rm, c)
        check(got, R.run(c), c, f"{c['name']} RM_OPT_SMALL={path}")
        raw, m1, m2 = got["raw"], got["m1"], got["m2"]


F16 = [(f"{kind}-M{m}", path) for m in R.CHAIN_SIZES for kind in ("zero_g", "warm10") for path in paths(m)]


@pytest.mark.parametrize("name,path", F16, ids=[f"{n}-small{p}" for n, p in F16])
def test_f16_call_equals_fp32_call(rm, monkeypatch, name, path):
    """rm_optimizer_step_f16: the fp32 call's masters, moments, activations and penalty bit for bit,
    and the updated colours as half(act colours), rounded to nearest even."""
    monkeypatch.setenv("RM_OPT_SMALL", path)
    c = R.case(name)
    m = c["M"]
    a = gpu_step(rm, c)
    b = gpu_step(rm, c, f16=True)
    for k in ("raw", "m1", "m2", "act"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert np.float32(a["penalty"]) == np.float32(b["penalty"])
    assert np.array_equal(b["colh"].view(np.uint16), a["act"][3 * m:6 * m].astype(np.float16).view(np.uint16))
    check(b, R.reference(name), c, f"{name} f16 RM_OPT_SMALL={path}")


@pytest.mark.parametrize("m,path", CHAINS, ids=[f"M{m}-small{p}" for m, p in CHAINS])
def test_null_loss_penalty_writes_no_penalty(rm, monkeypatch, m, path):
    """loss_penalty == NULL: the same step, and the word a penalty would have gone to keeps its
    guard value (gpu_step checks it with every other word outside the buffers passed)."""
    monkeypatch.setenv("RM_OPT_SMALL", path)
    c = R.case(f"warm2-M{m}")
    a = gpu_step(rm, c)
    b = gpu_step(rm, c, with_penalty_out=False)
    for k in ("raw", "m1", "m2", "act"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
