"""GPU tests of the image-space loss (rm_image_loss through ctypes, render.image_loss, render.image_metrics)
against the fp64 restatement (tests/ssim_ref.py).

Parity bounds. Nothing is fixed by hand (ssim_ref.bounds): per element of ssim_map, and of grad_out relative to
the case's largest gradient magnitude, 8 times the largest error of the restatement's float32 run (in the kernels'
horizontal-then-vertical order) against its fp64 run over the whole case set. The scalars are means of such
elements and are held to the same per-element bounds scaled by their weights: view_stats / pixel count to the
bounds of W|x - y|, (x - y)^2 and S, the loss to l1_weight x the first plus ssim_weight x the last. Figures are
printed and recorded (conftest.record_margin).

Measured on an MI355X (worst error over bound across the file): see DESIGN.md 5.2."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import ssim_ref as R
from conftest import GOLDEN, check_grads, gpu_available, record_margin

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

GUARD = 64
SENT = 1234.5
OUTPUTS = ("loss", "view_stats", "ssim_map", "grad")


@pytest.fixture(scope="module")
def rm():
    from burn_raymarching_amd import _build
    _build.build_lib()
    from burn_raymarching_amd import native, render
    torch.cuda.init()
    return render, native


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Outputs:
    """The four outputs of one call, each in its own buffer between GUARD sentinel words; NaN where requested."""

    def __init__(self, shape, want):
        v = shape[0]
        shapes = {"loss": (1,), "view_stats": (v, 3), "ssim_map": tuple(shape), "grad": tuple(shape)}
        self.buf, self.out, self.want = {}, {}, tuple(want)
        for k in OUTPUTS:
            size = int(np.prod(shapes[k]))
            b = torch.full((size + 2 * GUARD,), SENT, device="cuda")
            o = b[GUARD:GUARD + size].view(shapes[k])
            if k in self.want:
                o.fill_(float("nan"))
            self.buf[k], self.out[k] = b, o

    def ptr(self, k):
        return ptr(self.out[k]) if k in self.want else None

    def guards_intact(self):
        ok = True
        for k, b in self.buf.items():
            if k in self.want:
                ok = ok and bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + self.out[k].numel():] == SENT).all())
            else:
                ok = ok and bool((b == SENT).all())
        return ok

    def untouched(self):
        """Nothing was written at all: the guards, and NaN in every requested output."""
        return self.guards_intact() and all(bool(torch.isnan(self.out[k]).all()) for k in self.want)

    def host(self):
        return {k: self.out[k].cpu().numpy() for k in self.want}


def call(rm, x, y, want=OUTPUTS, *, inv_count=None, width=None, height=None, views=None, alias_grad=False, **fields):
    """rm_image_loss through ctypes on device tensors x, y [V, H, W, 3]. Returns (rc, Outputs, error text)."""
    render, native = rm
    v, h, w, _ = x.shape
    o = Outputs(x.shape, want)
    p = native.image_loss_params(**fields)
    ctx = render.context()
    rc = ctx._lib.rm_image_loss(ctx.handle, ptr(x), ptr(y), v if views is None else views, w if width is None else width,
                                h if height is None else height, 1.0 / x.numel() if inv_count is None else inv_count,
                                ctypes.byref(p), o.ptr("loss"), o.ptr("view_stats"), o.ptr("ssim_map"),
                                ptr(x) if alias_grad else o.ptr("grad"))
    torch.cuda.synchronize()
    return rc, o, ctx._lib.rm_last_error(ctx.handle).decode()


def check(tag, got, ref, lw, sw):
    """got against the fp64 run under the measured bounds."""
    b, _ = R.bounds()
    n = ref["ssim_map"][0].size  # elements of a view
    gmax = max(float(np.abs(ref["grad"]).max()), 1e-300)
    pairs = [("ssim_map", R.max_err(got["ssim_map"], ref["ssim_map"]), b["ssim_map"]),
             ("grad", R.max_err(got["grad"], ref["grad"]) / gmax, b["grad_rel"]),
             ("loss", R.max_err(got["loss"], ref["loss"]), lw * b["l1_elems"] + sw * b["ssim_map"]),
             ("stats_l1", R.max_err(got["view_stats"][:, 0], ref["view_stats"][:, 0]) / n, b["l1_elems"]),
             ("stats_sq", R.max_err(got["view_stats"][:, 1], ref["view_stats"][:, 1]) / n, b["sq_elems"]),
             ("stats_ssim", R.max_err(got["view_stats"][:, 2], ref["view_stats"][:, 2]) / n, b["ssim_map"])]
    bad = []
    for q, e, bound in pairs:
        print(f"loss parity {tag} {q}: gpu {e:.3e} bound {bound:.3e}")
        record_margin(f"loss_{q}", e, bound)
        if not e <= bound:
            bad.append((q, e, bound))
    assert all(np.isfinite(np.asarray(got[k])).all() for k in OUTPUTS)
    assert not bad, (tag, bad)


# ---- 1. parity ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("plain", [False, True])
@pytest.mark.parametrize("progress", R.PROGRESS)
@pytest.mark.parametrize("weights", R.WEIGHTS)
@pytest.mark.parametrize("case", R.CASES)
def test_parity_against_fp64(rm, case, weights, progress, plain):
    native = rm[1]
    x, y = R.images(*case)
    lw, sw = weights
    rc, o, err = call(rm, dev(x), dev(y), l1_weight=lw, ssim_weight=sw, progress=progress,
                      flags=native.RM_LOSS_PLAIN_L1 if plain else 0)
    assert rc == 0 and o.guards_intact(), err
    ref = R.run(x, y, torch.float64, l1_weight=lw, ssim_weight=sw, progress=progress, plain=plain)
    check(f"{case}_{lw}/{sw}_p{progress}_{'plain' if plain else 'w'}", o.host(), ref, lw, sw)


# ---- 2. the L1 seed's bits ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.CASES)
def test_l1_gradient_bit_for_bit(rm, case):
    """Weights (1, 0): grad_out is (W * sign(x - y)) * inv_count in float32, with a pixel at x == y and, where the
    image has room, a target sum exactly at the 0.01 threshold."""
    x, y = (a.copy() for a in R.images(*case))
    x[0, case[1] // 2, case[2] // 2] = y[0, case[1] // 2, case[2] // 2]
    if case[2] > 2:
        y[-1, 0, 0] = np.float32([0.0025, 0.0025, 0.005])
        y[-1, 0, 1] = np.float32([0.0025, 0.0025, 0.0051])
    for progress in R.PROGRESS:
        inv = float(np.float32(1.0 / x.size))
        rc, o, err = call(rm, dev(x), dev(y), ("grad", "loss"), inv_count=inv, l1_weight=1.0, ssim_weight=0.0,
                          progress=progress)
        assert rc == 0 and o.guards_intact(), err
        want = R.l1_grad_f32(x, y, progress, inv_count=inv)
        assert o.host()["grad"].tobytes() == want.tobytes(), (case, progress)
        assert np.all(o.host()["grad"][0, case[1] // 2, case[2] // 2] == 0.0)


# ---- 3. view isolation -------------------------------------------------------------------------------

def test_views_are_isolated(rm):
    x, y = (a.copy() for a in R.images(3, 19, 23))
    rc, a, err = call(rm, dev(x), dev(y))
    assert rc == 0, err
    x2, y2 = x.copy(), y.copy()
    rng = np.random.default_rng(5)
    x2[1], y2[1] = rng.uniform(0, 1, x[1].shape), rng.uniform(0, 1, y[1].shape)
    rc, b, err = call(rm, dev(x2), dev(y2))
    assert rc == 0, err
    ha, hb = a.host(), b.host()
    for k in ("ssim_map", "grad", "view_stats"):
        for v in (0, 2):
            assert ha[k][v].tobytes() == hb[k][v].tobytes(), (k, v)
        assert ha[k][1].tobytes() != hb[k][1].tobytes(), k


# ---- 4. nullable outputs -----------------------------------------------------------------------------

SUBSETS = [("loss",), ("view_stats",), ("ssim_map",), ("grad",), ("loss", "grad"), ("view_stats", "ssim_map"),
           ("loss", "view_stats", "ssim_map")]


@pytest.mark.parametrize("weights", [(0.8, 0.2), (1.0, 0.0)])
def test_nullable_outputs(rm, weights):
    """Every subset: guards intact, an unrequested buffer untouched, and each output's bits those of the call with
    every output -- the metrics-only calls (grad_out NULL) included."""
    x, y = (dev(a) for a in R.images(2, 33, 17))
    lw, sw = weights
    rc, full, err = call(rm, x, y, l1_weight=lw, ssim_weight=sw)
    assert rc == 0 and full.guards_intact(), err
    ref = full.host()
    for want in SUBSETS:
        rc, o, err = call(rm, x, y, want, l1_weight=lw, ssim_weight=sw)
        assert rc == 0 and o.guards_intact(), (want, err)
        for k, val in o.host().items():
            assert np.isfinite(val).all() and val.tobytes() == ref[k].tobytes(), (want, k)


# ---- 5. determinism and scratch reuse ----------------------------------------------------------------

def test_two_calls_and_scratch_reuse_give_the_same_bits(rm):
    x, y = (dev(a) for a in R.images(3, 19, 23))
    rc, a, err = call(rm, x, y)
    assert rc == 0, err
    rc, b, _ = call(rm, x, y)
    big = [dev(t) for t in R.images(1, 48, 40)]
    rc2, _, _ = call(rm, big[0] * 1e3, big[1] * 1e3)  # a larger shape leaves other values in the scratch
    rc3, c, _ = call(rm, x, y)
    assert rc == 0 and rc2 == 0 and rc3 == 0
    for k, val in a.host().items():
        assert val.tobytes() == b.host()[k].tobytes() == c.host()[k].tobytes(), k


# ---- 6. invalid arguments ----------------------------------------------------------------------------

@pytest.mark.parametrize("name, kw, word", [
    ("width", {"width": 0}, "width"),
    ("height", {"height": -1}, "height"),
    ("views", {"views": 0}, "num_views"),
    ("l1_weight", {"l1_weight": -0.5}, "l1_weight"),
    ("ssim_weight", {"ssim_weight": float("nan")}, "ssim_weight"),
    ("c1", {"c1": float("inf")}, "c1"),
    ("c2", {"c2": 0.0}, "c2"),
    ("flags", {"flags": 2}, "flags"),
    ("no_output", {"want": ()}, "no output"),
    ("alias", {"alias_grad": True}, "grad_out aliases"),
])
def test_invalid_arguments_touch_nothing(rm, name, kw, word):
    x, y = (dev(a) for a in R.images(2, 5, 7))
    x0 = x.clone()
    kw = dict(kw)
    want = kw.pop("want", OUTPUTS)
    rc, o, err = call(rm, x, y, want, **kw)
    assert rc == 1 and word in err, (name, rc, err)
    assert o.untouched() and torch.equal(x, x0)
    rc, o, err = call(rm, x, y)  # the context still works
    assert rc == 0 and o.guards_intact(), err


# ---- 7. identical images -----------------------------------------------------------------------------

def test_identical_images(rm):
    render, _ = rm
    b, _ = R.bounds()
    _, y = R.images(3, 19, 23)
    t = dev(y)
    rc, o, err = call(rm, t, t.clone(), l1_weight=1.0, ssim_weight=0.0)
    assert rc == 0, err
    assert np.all(o.host()["grad"] == 0.0) and o.host()["loss"][0] == 0.0
    rc, o, err = call(rm, t, t.clone())
    h = o.host()
    e_map, e_grad = np.abs(h["ssim_map"] - 1.0).max(), np.abs(h["grad"]).max()
    # the gradient's scale here is the case's largest gradient against its own render
    gmax = np.abs(R.run(*R.images(3, 19, 23), torch.float64)["grad"]).max()
    print(f"loss identical images: |S - 1| {e_map:.3e} (bound {b['ssim_map']:.3e}), |grad| / gmax {e_grad / gmax:.3e} "
          f"(bound {b['grad_rel']:.3e})")
    record_margin("loss_identical_map", e_map, b["ssim_map"])
    record_margin("loss_identical_grad", e_grad / gmax, b["grad_rel"])
    assert e_map <= b["ssim_map"] and e_grad / gmax <= b["grad_rel"]
    m = render.image_metrics(t, t.clone(), 23, 19)
    assert bool(torch.isinf(m["psnr"]).all()) and bool((m["psnr"] > 0).all()) and bool((m["l1"] == 0).all())
    assert float((m["ssim"] - 1.0).abs().max()) <= b["ssim_map"]


# ---- 8. golden metrics -------------------------------------------------------------------------------

def test_golden_metrics(rm):
    render, _ = rm
    b, _ = R.bounds()
    rec = json.load(open(os.path.join(GOLDEN, "ssim_targets.json")))
    x, y = R.golden_pair()
    m = render.image_metrics(dev(x).reshape(-1, 3), dev(y).reshape(-1, 3), 256, 256)
    got = {k: float(v.cpu()[0]) for k, v in m.items()}
    mse = 10.0 ** (-rec["psnr"] / 10.0)
    # PSNR through its mean squared error: d psnr = 10 / ln 10 * d mse / mse
    bound = {"ssim": b["ssim_map"], "l1": b["l1_elems"], "psnr": 10.0 / np.log(10.0) * b["sq_elems"] / mse + 1e-5}
    for k in ("psnr", "ssim", "l1"):
        e = abs(got[k] - rec[k])
        print(f"loss golden {k}: gpu {got[k]:.9g} recorded {rec[k]:.9g} err {e:.3e} bound {bound[k]:.3e}")
        record_margin(f"loss_golden_{k}", e, bound[k])
        assert e <= bound[k], (k, got[k], rec[k])


# ---- 9. through the render ---------------------------------------------------------------------------

W_R, V_R, K_R, S_R = 32, 2, 32.0, 32


def _render_problem():
    from burn_raymarching_amd import model, render
    cams = model.ring_cameras(V_R)
    eye = torch.tensor([c[0] for c in cams], dtype=torch.float32)
    tgt = torch.tensor([c[1] for c in cams], dtype=torch.float32)
    fov = torch.tensor([c[2] for c in cams], dtype=torch.float32)
    target = render.render_diff_camera(cams, W_R, W_R, model.scene_tensors(model.synthetic_scene(8, 1)), K_R, S_R)
    sc = model.synthetic_scene(8, 0)
    par = {k: dev(sc[k]).requires_grad_(True) for k in ("centers", "colors", "radius", "light_dir", "ambient")}
    return (eye, tgt, fov), target, par


def _render(cam, par):
    from burn_raymarching_amd import render
    return render.render_diff_cameras(cam[0], cam[1], cam[2], W_R, W_R, par["centers"], par["colors"], par["radius"],
                                      par["light_dir"], par["ambient"], K_R, S_R)


def test_scene_gradients_through_the_render(rm):
    """render.image_loss(render.render_diff_cameras(...)).backward(): the scene gradients against the same render
    autograd driven by the fp64 restatement's loss gradient."""
    render, _ = rm
    cam, target, par = _render_problem()
    out = _render(cam, par)
    loss = render.image_loss(out, target, W_R, W_R)
    loss.backward()
    got = {k: v.grad.clone() for k, v in par.items()}
    x = out.detach().cpu().numpy().reshape(V_R, W_R, W_R, 3)
    y = target.cpu().numpy().reshape(V_R, W_R, W_R, 3)
    ref = R.run(x, y, torch.float64)
    assert abs(float(loss.detach()) - float(ref["loss"])) <= 0.8 * R.bounds()[0]["l1_elems"] + 0.2 * R.bounds()[0]["ssim_map"]
    for v in par.values():
        v.grad = None
    _render(cam, par).backward(dev(ref["grad"]).reshape(-1, 3))
    want = {k: v.grad.double().cpu().numpy() for k, v in par.items()}
    check_grads(got, want, mode="bwd")
    assert all(np.abs(w).max() > 0 for w in want.values())


def test_adam_steps_lower_the_loss(rm):
    """25 Adam steps (torch, lr 0.01) on centres, colours and radii end below where they start. The run is
    deterministic; recorded on an MI355X: 0.049990 before the first step, 0.039036 after the last."""
    render, _ = rm
    cam, target, par = _render_problem()
    train = [par[k] for k in ("centers", "colors", "radius")]
    opt = torch.optim.Adam(train, lr=0.01)
    losses = []
    for _ in range(25):
        opt.zero_grad()
        loss = render.image_loss(_render(cam, par), target, W_R, W_R)
        loss.backward()
        opt.step()
        with torch.no_grad():
            par["colors"].clamp_(0.0, 1.0)
            par["radius"].clamp_(min=0.02)
        losses.append(float(loss.detach()))
    last = float(render.image_loss(_render(cam, par), target, W_R, W_R).detach())
    print(f"loss fit: first {losses[0]:.6f} after 25 steps {last:.6f}")
    assert np.isfinite(losses).all() and last < losses[0], (losses[0], last)
