"""GPU tests of the distance field's backward (rm_sdf_query_backward, render.sdf_query_backward /
sdf_field) against torch autograd of the fp64 restatement (tests/sdf_grad_ref.py), on the scenes and the
point pool of tests/test_gpu_sdf.py.

Parity bounds. Nothing is fixed by hand: per scene, seed set and output the bound is 8 times the max
error of the restatement's float32 run against fp64 over the scene's whole pool of 1000 points (the point
gradient separately over the near points and the six points 1e3 units away), and holds for every point
count N, whose points and seeds are the pool's first N. Figures are printed and recorded
(conftest.record_margin); profiles/r22_sdf_grad_parity.txt holds a run's.

Additivity (tests/additivity_ref.py): a call on one block's 256 points alone returns that block's partial
record bit for bit, so the full call is held to the fp32 summation bound of its own terms, no tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import additivity_ref as AD
import sdf_grad_ref as R
from conftest import gpu_available, record_margin
from test_gpu_sdf import CSHARP, K, err, pool

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

GUARD = 64
SENT = 1234.5  # the guard words' and the light buffers' value
SCENE_KEYS = ("centers", "colors", "radius")
ALL = SCENE_KEYS + ("points",)


@pytest.fixture(scope="module")
def rm():
    from burn_raymarching_amd import _build
    _build.build_lib()
    from burn_raymarching_amd import native, render
    torch.cuda.init()
    return render, native


def dev(x, dtype=np.float32):
    return torch.from_numpy(np.array(x, dtype)).cuda()  # a copy: the pool's arrays are read-only


def bits(t):
    return t.detach().cpu().numpy().tobytes()


def scene_dev(sc, half=False):
    t = {k: dev(sc[k]) for k in SCENE_KEYS}
    if half:
        t["colors"] = t["colors"].half()
    return t


class Outputs:
    """The outputs of one C call, each inside its own buffer with GUARD sentinel words on both sides, and
    the light_dir / ambient buffers the call must never write."""

    def __init__(self, m, n, want, fill=float("nan"), prior=None):
        shapes = {"centers": (m, 3), "colors": (m, 3), "radius": (m,), "points": (n, 3)}
        self.buf, self.out = {}, {}
        for k in want:
            size = int(np.prod(shapes[k]))
            b = torch.full((size + 2 * GUARD,), SENT, device="cuda")
            v = b[GUARD:GUARD + size].view(shapes[k])
            if prior is not None:
                v.copy_(prior[k])
            else:
                v.fill_(fill)
            self.buf[k], self.out[k] = b, v
        self.light = torch.full((3 + 1 + 2 * GUARD,), SENT, device="cuda")

    def ptr(self, k):
        return ctypes.c_void_p(self.out[k].data_ptr()) if k in self.out else None

    def guards_intact(self):
        ok = bool((self.light == SENT).all())
        for k, b in self.buf.items():
            ok = ok and bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + self.out[k].numel():] == SENT).all())
        return ok

    def host(self):
        return {k: v.cpu().numpy() for k, v in self.out.items()}


def c_call(rm, pts, sct, gD, gC, want=ALL, accumulate=0, prior=None, num=None, params=None, grads_null=False):
    """rm_sdf_query_backward through ctypes. pts / gD / gC: device tensors (seeds may be None). Returns
    (rc, Outputs)."""
    render, native = rm
    n = pts.shape[0]
    m = sct["centers"].shape[0]
    o = Outputs(m, n, want, prior=prior)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    cs = native.RmScene(sct["centers"].data_ptr(), sct["colors"].data_ptr(), sct["radius"].data_ptr(), None, None, m)
    half = sct["colors"].dtype == torch.float16
    par = params if params is not None else native.sdf_params(smooth_k=K, color_sharpness=CSHARP,
                                                             flags=native.RM_MARCH_COLOR_F16 if half else 0)
    g = native.RmGrads(o.ptr("centers"), o.ptr("colors"), o.ptr("radius"), ctypes.c_void_p(o.light.data_ptr() + 4 * GUARD),
                       ctypes.c_void_p(o.light.data_ptr() + 4 * (GUARD + 3)))
    ctx = render.context(pts.device)
    rc = ctx._lib.rm_sdf_query_backward(ctx.handle, p(pts), n if num is None else num, ctypes.byref(cs), ctypes.byref(par),
                                        p(gD), p(gC), None if grads_null else ctypes.byref(g), o.ptr("points"),
                                        accumulate)
    torch.cuda.synchronize()
    return rc, o


_BOUNDS = {}


def case(name, seeds, half=False):
    """(scene, points, far, (gD, gC) float32 for the whole pool, bounds) of a scene and seed set."""
    key = (name, seeds, half)
    if key not in _BOUNDS:
        sc, pts, far, _, _ = pool(name)
        if half:
            sc = dict(sc, colors=sc["colors"].astype(np.float16).astype(np.float32))
        gD, gC = R.seed_sets(len(pts))[seeds]
        b, _ = R.bounds(pts, far, sc, K, CSHARP, gD, gC)
        _BOUNDS[key] = (sc, pts, far, gD, gC, b)
    return _BOUNDS[key]


def check_parity(tag, got, sc, pts, far, gD, gC, bound, n):
    ref = R.autograd(pts[:n], sc, K, CSHARP, None if gD is None else gD[:n], None if gC is None else gC[:n])
    e = R.errors(got, ref, far[:n])
    bad = []
    for q, v in e.items():
        print(f"sdf grad parity {tag} N={n} {q}: gpu {v:.3e} bound {bound[q]:.3e}")
        record_margin(f"sdf_grad_{q}_{tag}_{n}", v, bound[q])
        if not v <= bound[q]:
            bad.append((q, v, bound[q]))
    assert all(np.isfinite(x).all() for x in got.values())
    assert not bad, (tag, n, bad)


@pytest.mark.parametrize("n", [1, 65, 256, 257, 1000])
@pytest.mark.parametrize("name", ["golden", "one", "m33", "m300", "m520"])
def test_parity_against_fp64_autograd(rm, name, n):
    for seeds in R.SEEDS:
        sc, pts, far, gD, gC, bound = case(name, seeds)
        rc, o = c_call(rm, dev(pts[:n]), scene_dev(sc), None if gD is None else dev(gD[:n]),
                       None if gC is None else dev(gC[:n]))
        assert rc == 0 and o.guards_intact()
        check_parity(f"{name}_{seeds}", o.host(), sc, pts, far, gD, gC, bound, n)


def test_clamp_mask_off_the_centre(rm):
    """The pool's centre point has e = 0 exactly, where the clamp's mask changes nothing. Here point 9 of
    the m33 pool sits 5e-4 from the centre of sphere 0 (q = 2.5e-7 < 1e-6, e != 0): its term must drop out
    of dL/dc_0 and of its own point gradient, under bounds taken over the changed pool
    (tests/test_sdf_grad_reference.py: ignoring the mask misses them by 160 bounds and more)."""
    sc, pts, far, _, _ = pool("m33")
    pts = pts.copy()
    pts[9] = sc["centers"][0] + np.array([5e-4, 0.0, 0.0], np.float32)
    gD, gC = R.seed_sets(len(pts))["both"]
    bound, _ = R.bounds(pts, far, sc, K, CSHARP, gD, gC)
    n = 65
    rc, o = c_call(rm, dev(pts[:n]), scene_dev(sc), dev(gD[:n]), dev(gC[:n]))
    assert rc == 0
    check_parity("m33_both_under_clamp", o.host(), sc, pts, far, gD, gC, bound, n)


def test_fp16_colours(rm):
    """Half colours: parity against the restatement on the rounded colours, the bits of the fp32 call on
    the rounded colours, and an fp32 colour gradient (Outputs allocates float32)."""
    n = 257
    sc, pts, far, gD, gC, bound = case("m33", "both", half=True)
    args = (dev(pts[:n]),), (dev(gD[:n]), dev(gC[:n]))
    rc, h = c_call(rm, *args[0], scene_dev(sc, half=True), *args[1])
    assert rc == 0 and h.guards_intact()
    check_parity("m33_both_f16", h.host(), sc, pts, far, gD, gC, bound, n)
    rc, f = c_call(rm, *args[0], scene_dev(sc), *args[1])
    raw = pool("m33")[0]
    rc2, base = c_call(rm, *args[0], scene_dev(raw), *args[1])
    assert rc == 0 and rc2 == 0
    assert all(bits(h.out[k]) == bits(f.out[k]) for k in ALL)
    assert bits(h.out["centers"]) != bits(base.out["centers"])


# ---- additivity ----------------------------------------------------------------------------------

def packed(o):
    return np.concatenate([o.out[k].cpu().numpy().astype(np.float64).reshape(-1) for k in SCENE_KEYS])


def blocks_problem(m, nblocks, seed, zero_blocks=()):
    from burn_raymarching_amd import model
    sc = model.synthetic_scene(m, seed)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    n = nblocks * 256
    pts = torch.rand((n, 3), device="cuda", generator=gen) * 2 - 1
    gD = torch.randn((n,), device="cuda", generator=gen)
    gC = torch.randn((n, 3), device="cuda", generator=gen)
    for b in zero_blocks:
        gD[b * 256:(b + 1) * 256] = 0
        gC[b * 256:(b + 1) * 256] = 0
    return scene_dev(sc), pts, gD, gC


def poison(rm, sct, pts):
    """A call on the same context with every point live and seeds of 2^40: whatever it leaves in the
    workspace must not reach the next call's result."""
    big = float(2 ** 40)
    rc, _ = c_call(rm, pts, sct, torch.full((pts.shape[0],), big, device="cuda"),
                   torch.full((pts.shape[0], 3), -big, device="cuda"))
    assert rc == 0


def additivity(rm, sct, pts, gD, gC, live_blocks, tag):
    poison(rm, sct, pts)
    rc, full = c_call(rm, pts, sct, gD, gC)
    assert rc == 0 and full.guards_intact()
    rows = []
    for b in live_blocks:
        s = slice(b * 256, (b + 1) * 256)
        rc, r = c_call(rm, pts[s], sct, gD[s], gC[s], want=SCENE_KEYS)
        assert rc == 0
        rows.append(packed(r))
    ok, ratio, nz = AD.measure(packed(full), np.stack(rows))
    print(f"sdf grad additivity {tag}: worst err / bound {ratio:.3f} over {nz} non-zero rows")
    record_margin(f"sdf_grad_additivity_{tag}", ratio, 1.0)
    assert ok, (tag, ratio, nz)
    return full


@pytest.mark.parametrize("nblocks", [2, 3, 129])
def test_additivity(rm, monkeypatch, nblocks):
    monkeypatch.delenv("RM_MAX_BLOCKS_PER_LAUNCH", raising=False)
    sct, pts, gD, gC = blocks_problem(33, nblocks, 40 + nblocks)
    additivity(rm, sct, pts[:nblocks * 256 - 100], gD[:nblocks * 256 - 100], gC[:nblocks * 256 - 100], range(nblocks),
               f"m33_{nblocks}_blocks")


def test_additivity_sub_launches(rm, monkeypatch):
    """RM_MAX_BLOCKS_PER_LAUNCH=2: seven blocks in four launches, the later ones accumulating. The chain
    of launches is itself a sum of the launches' results; the same bits at accumulate = 0 as one launch's
    additivity bound allows (measured against the rows), and grad_points the bits of the single launch."""
    sct, pts, gD, gC = blocks_problem(300, 7, 47)
    monkeypatch.delenv("RM_MAX_BLOCKS_PER_LAUNCH", raising=False)
    rc, one = c_call(rm, pts, sct, gD, gC)
    assert rc == 0
    monkeypatch.setenv("RM_MAX_BLOCKS_PER_LAUNCH", "2")
    split = additivity(rm, sct, pts, gD, gC, range(7), "m300_7_blocks_by_2")
    assert bits(split.out["points"]) == bits(one.out["points"])


def test_additivity_large_launch(rm, monkeypatch):
    """32,769 blocks at M = 1: more than kReduceSegs * 256 rows, the reduction's large-launch branch (192
    segments of 171 rows). One block in each segment is live, the first and the last block among them; the
    others have zero seeds, so their rows are exact zeros and the live blocks' rows are all the terms."""
    monkeypatch.delenv("RM_MAX_BLOCKS_PER_LAUNCH", raising=False)
    nblocks = 32769
    segs, seg_len = AD.seg_layout(nblocks)
    assert segs == 192 and seg_len == 171
    live = sorted({0, nblocks - 1} | {s * seg_len + (37 * s) % seg_len for s in range(segs) if s * seg_len < nblocks - 1})
    live = [b for b in live if b < nblocks]
    from burn_raymarching_amd import model
    sct = scene_dev(model.synthetic_scene(1, 9))
    gen = torch.Generator(device="cuda").manual_seed(5)
    n = nblocks * 256
    pts = torch.rand((n, 3), device="cuda", generator=gen) * 2 - 1
    gD = torch.zeros((n,), device="cuda")
    gC = torch.zeros((n, 3), device="cuda")
    for b in live:
        gD[b * 256:(b + 1) * 256] = torch.randn((256,), device="cuda", generator=gen)
        gC[b * 256:(b + 1) * 256] = torch.randn((256, 3), device="cuda", generator=gen)
    full = additivity(rm, sct, pts, gD, gC, live, "m1_32769_blocks")
    gp = full.out["points"].view(nblocks, 256, 3)
    dead = torch.ones(nblocks, dtype=torch.bool, device="cuda")
    dead[torch.tensor(live, device="cuda")] = False
    assert not gp[dead].any() and gp[~dead].any()


def test_zero_seed_blocks(rm, monkeypatch):
    """Blocks whose seeds are all zero, first, middle and last: their rows are exact zeros, and the call
    has the bits of the call on the live blocks alone (the block boundaries coincide)."""
    monkeypatch.delenv("RM_MAX_BLOCKS_PER_LAUNCH", raising=False)
    sct, pts, gD, gC = blocks_problem(33, 5, 51, zero_blocks=(0, 2, 4))
    full = additivity(rm, sct, pts, gD, gC, range(5), "m33_5_blocks_3_dead")
    for b in (0, 2, 4):
        s = slice(b * 256, (b + 1) * 256)
        rc, r = c_call(rm, pts[s], sct, gD[s], gC[s])
        assert rc == 0 and not any(v.any() for v in r.out.values())
        assert not full.out["points"][s].any()
    keep = torch.cat([torch.arange(256, 512), torch.arange(768, 1024)]).cuda()
    rc, only = c_call(rm, pts[keep].contiguous(), sct, gD[keep].contiguous(), gC[keep].contiguous())
    assert rc == 0
    assert all(bits(full.out[k]) == bits(only.out[k]) for k in SCENE_KEYS)
    assert bits(full.out["points"][keep]) == bits(only.out["points"])
    # zero seeds inside a live block: exact zeros for those points, and the sums of the others alone
    gD2, gC2 = gD.clone(), gC.clone()
    gD2[300:400] = 0
    gC2[300:400] = 0
    rc, part = c_call(rm, pts, sct, gD2, gC2)
    assert rc == 0 and not part.out["points"][300:400].any() and part.out["points"][256:300].any()


# ---- bit-level pins ------------------------------------------------------------------------------

def test_bit_level_pins(rm, monkeypatch):
    monkeypatch.delenv("RM_MAX_BLOCKS_PER_LAUNCH", raising=False)
    n = 1000
    sc, pts, far, gD, gC, _ = case("m300", "both")
    sct, p, d, c = scene_dev(sc), dev(pts[:n]), dev(gD[:n]), dev(gC[:n])
    rc, full = c_call(rm, p, sct, d, c)  # outputs pre-filled with NaN
    assert rc == 0 and full.guards_intact()
    assert all(torch.isfinite(v).all() for v in full.out.values())
    rc, again = c_call(rm, p, sct, d, c)
    assert rc == 0 and all(bits(full.out[k]) == bits(again.out[k]) for k in ALL)
    # each output alone, and the pairs with the point gradient, have the bits of the full call
    for want in [(k,) for k in ALL] + [("centers", "points"), ("colors", "radius")]:
        rc, part = c_call(rm, p, sct, d, c, want=want)
        assert rc == 0 and part.guards_intact(), want
        assert all(bits(part.out[k]) == bits(full.out[k]) for k in want), want
    # accumulate = 1 on a random prior: float32(G0 + G)
    rng = np.random.default_rng(3)
    prior = {k: dev(rng.normal(size=tuple(v.shape))) for k, v in full.out.items()}
    rc, acc = c_call(rm, p, sct, d, c, accumulate=1, prior=prior)
    assert rc == 0 and acc.guards_intact()
    for k in ALL:
        want = prior[k].cpu().numpy() + full.out[k].cpu().numpy()  # one float32 addition
        assert want.dtype == np.float32 and acc.out[k].cpu().numpy().tobytes() == want.tobytes(), k


@pytest.mark.parametrize("name", ["golden", "m300"])
def test_point_gradient_is_the_querys_grad(rm, name):
    """gD = 1 and no colour seed: grad_points is grad D, within test_gpu_sdf.py's grad bound of
    rm_sdf_query's own grad output (and of the fp64 restatement)."""
    render, _ = rm
    sc, pts, far, ref64, ref32 = pool(name)
    n = 1000
    p = dev(pts[:n])
    rc, o = c_call(rm, p, scene_dev(sc), torch.ones(n, device="cuda"), None, want=("points",))
    assert rc == 0
    t = {k: dev(sc[k]) for k in sc}
    scene = render.Scene(t["centers"], t["colors"], t["radius"], t["light_dir"], t["ambient"])
    g = render.sdf_query(p, scene, K, color_sharpness=CSHARP, color=False)[1].cpu().numpy()
    got = o.out["points"].cpu().numpy()
    for group, mask in (("near", ~far), ("far", far)):
        bound = 8.0 * err(ref32[1], ref64[1], mask)
        e_q, e_64 = err(got, g, mask), err(got, ref64[1], mask)
        print(f"sdf grad points vs query grad {name} {group}: {e_q:.3e}, vs fp64 {e_64:.3e}, bound {bound:.3e}")
        record_margin(f"sdf_grad_points_vs_query_{group}_{name}", e_q, bound)
        assert e_q <= bound and e_64 <= bound, (name, group, e_q, e_64, bound)


# ---- call behaviour ------------------------------------------------------------------------------

def test_call_behaviour(rm):
    render, native = rm
    sc, pts, far, gD, gC, _ = case("m33", "both")
    n = 257
    sct, p, d, c = scene_dev(sc), dev(pts[:n]), dev(gD[:n]), dev(gC[:n])
    ctx = render.context(p.device)

    def refused(res, word=None):
        rc, o = res
        msg = ctx._lib.rm_last_error(ctx.handle).decode()
        assert rc == 1 and msg and (word is None or word in msg), (rc, msg)  # RM_ERR_INVALID_ARG with a message
        assert o.guards_intact() and all(torch.isnan(v).all() for v in o.out.values())  # nothing was launched

    refused(c_call(rm, p, sct, None, None), "grad_dist")
    refused(c_call(rm, p, sct, d, c, want=()), "output")
    refused(c_call(rm, p, sct, d, c, want=(), grads_null=True), "output")
    refused(c_call(rm, p, sct, d, c, params=native.sdf_params(smooth_k=0.0)), "smooth_k")
    refused(c_call(rm, p, sct, d, c, params=native.sdf_params(color_sharpness=-1.0)), "color_sharpness")
    refused(c_call(rm, p, sct, d, c, params=native.sdf_params(flags=native.RM_MARCH_SPLIT)), "flags")
    refused(c_call(rm, p, sct, d, c, num=-1), "num_points")
    # grads NULL with grad_points, and the reverse, are calls
    rc, o = c_call(rm, p, sct, d, c, want=("points",), grads_null=True)
    assert rc == 0 and torch.isfinite(o.out["points"]).all()
    # N = 0: zeros to grads at accumulate = 0, nothing at accumulate = 1; grad_points has no element
    rc, o = c_call(rm, p, sct, d, c, num=0)
    assert rc == 0 and o.guards_intact()
    assert all(not o.out[k].any() for k in SCENE_KEYS) and torch.isnan(o.out["points"]).all()
    rc, o = c_call(rm, p, sct, d, c, num=0, accumulate=1)
    assert rc == 0 and all(torch.isnan(v).all() for v in o.out.values())
    with pytest.raises(native.RaymarchError, match="RM_ERR_INVALID_ARG"):
        render.sdf_query_backward(p, sct["centers"], sct["colors"], sct["radius"], 0.0, grad_dist=d)


def test_prepared_optimizer_state_is_dropped(rm, oracle, monkeypatch):
    """As tests/test_gpu_small.py's test_prepared_step_dropped_by_another_call, with this entry point as the
    other call: after it, rm_optimizer_step computes on the changed parameters (the result of
    RM_OPT_PREPARE=0), not with the factors prepared on the old ones."""
    from burn_raymarching_amd import model
    render, native = rm
    m, nu, nf = 7, 6000, 2000
    rays = [oracle.camera_rays(48, 48, *cam, precision="f32") for cam in model.ring_cameras(2)]
    o = dev(np.concatenate([r[0] for r in rays]))
    d = dev(np.concatenate([r[1] for r in rays]))
    tg = dev(np.random.default_rng(5).uniform(size=(o.shape[0], 3)))
    fg = torch.arange(0, o.shape[0], 2, dtype=torch.int32, device="cuda")
    sc = model.synthetic_scene(m, 123, radius_range=(0.08, 0.3))
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    pts, gD = dev(pool("m33")[1][:64]), torch.ones(64, device="cuda")
    res = []
    for prepare in ("1", "0"):
        monkeypatch.setenv("RM_OPT_PREPARE", prepare)
        ctx = render.context()
        sm = model.SceneModel.from_activated(sc["centers"], sc["colors"], sc["radius"], sc["light_dir"], sc["ambient"])
        raw = sm.raw.clone()
        act = sm.activated_packed().clone()
        npk = model.packed_size(m)
        grad = torch.zeros(npk, device="cuda")
        mom = [torch.zeros(npk, device="cuda") for _ in range(2)]
        loss = torch.zeros(2, device="cuda")
        s = native.RmScene()
        ctx._lib.rm_scene_from_packed(p(act), m, ctypes.byref(s))
        g = native.RmGrads()
        ctx._lib.rm_grads_from_packed(p(grad), m, ctypes.byref(g))
        march = native.march_params(40, 20.0)
        ctx.check(ctx._lib.rm_train_step_sampled_prepared(ctx.handle, p(o), p(d), p(tg), o.shape[0], p(fg), fg.numel(),
                                                          nu, nf, 3, 1, 1, 0.5, 1.0 / (3 * (nu + nf)), ctypes.byref(s),
                                                          ctypes.byref(march), ctypes.byref(g), p(loss), p(raw), 1, 1,
                                                          ctypes.c_void_p(loss.data_ptr() + 4)),
                  "rm_train_step_sampled_prepared")
        torch.cuda.synchronize()
        raw.add_(0.25)  # a host-side change of the parameters between the calls
        gp = torch.empty((64, 3), device="cuda")
        ctx.check(ctx._lib.rm_sdf_query_backward(ctx.handle, p(pts), 64, ctypes.byref(s), None, p(gD), None, None, p(gp), 0),
                  "rm_sdf_query_backward")
        ctx.check(ctx._lib.rm_optimizer_step(ctx.handle, p(raw), p(grad), p(mom[0]), p(mom[1]), m, 1, 0.01, 1e-5, 1,
                                             ctypes.c_void_p(loss.data_ptr() + 4), p(act)), "rm_optimizer_step")
        torch.cuda.synchronize()
        res.append([x.clone() for x in (raw, act, mom[0], mom[1], loss)])
    for name, u, v in zip(("raw", "act", "adam_m", "adam_v", "loss"), *res):
        assert torch.equal(u, v), (name, (u - v).abs().max().item())


# ---- torch ---------------------------------------------------------------------------------------

def test_sdf_field_autograd(rm, monkeypatch):
    render, _ = rm
    n = 257
    sc, pts, far, gD, gC, _ = case("m33", "both")
    sct, d, c = scene_dev(sc), dev(gD[:n]), dev(gC[:n])
    p = dev(pts[:n])
    rc, ref = c_call(rm, p, sct, d, c)
    assert rc == 0
    leaf = {k: sct[k].clone().requires_grad_(True) for k in SCENE_KEYS}
    pl = p.clone().requires_grad_(True)
    dist, col = render.sdf_field(pl, leaf["centers"], leaf["colors"], leaf["radius"], K, color_sharpness=CSHARP)
    # the forward is sdf_query's, bit for bit
    t = {k: dev(sc[k]) for k in sc}
    qd, qc = render.sdf_query(p, render.Scene(t["centers"], t["colors"], t["radius"], t["light_dir"], t["ambient"]), K,
                              color_sharpness=CSHARP, grad=False)
    assert bits(dist) == bits(qd) and bits(col) == bits(qc)
    torch.autograd.backward([dist, col], [d, c])
    assert bits(pl.grad) == bits(ref.out["points"])
    assert all(bits(leaf[k].grad) == bits(ref.out[k]) for k in SCENE_KEYS)
    # only the inputs that require grad, only from the seeds that exist: the distance alone, two leaves
    rc, ref_d = c_call(rm, p, sct, d, None, want=("centers", "points"))
    assert rc == 0
    cl, pl2 = sct["centers"].clone().requires_grad_(True), p.clone().requires_grad_(True)
    dist2, _ = render.sdf_field(pl2, cl, sct["colors"], sct["radius"], K, color_sharpness=CSHARP)
    calls = []
    inner = render.sdf_query_backward

    def spy(*a, **kw):
        calls.append(kw)
        return inner(*a, **kw)

    monkeypatch.setattr(render, "sdf_query_backward", spy)
    g_p, g_c = torch.autograd.grad(dist2, (pl2, cl), d)
    monkeypatch.setattr(render, "sdf_query_backward", inner)
    assert bits(g_p) == bits(ref_d.out["points"]) and bits(g_c) == bits(ref_d.out["centers"])
    assert len(calls) == 1 and sorted(calls[0]["want"]) == ["centers", "points"] and calls[0]["grad_color"] is None
    # half colours: the fp16 path, an fp32 gradient cast to half
    rc, ref_h = c_call(rm, p, scene_dev(sc, half=True), d, c, want=("colors",))
    assert rc == 0
    ch = sct["colors"].half().requires_grad_(True)
    dh, colh = render.sdf_field(p, sct["centers"], ch, sct["radius"], K, color_sharpness=CSHARP)
    torch.autograd.backward([dh, colh], [d, c])
    assert ch.grad.dtype == torch.float16 and bits(ch.grad) == bits(ref_h.out["colors"].half())
    # no double backward
    d3, _ = render.sdf_field(pl2, cl, sct["colors"], sct["radius"], K, color_sharpness=CSHARP)
    (g1,) = torch.autograd.grad(d3.sum(), pl2, create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()


def test_fit_demonstration(rm):
    """Three spheres fitted to samples of a target's surface through render.sdf_field and torch's Adam:
    200 steps end at or below 0.05 of the initial loss (twice the bar the restatement itself is held to in
    tests/test_sdf_grad_reference.py; fp32 trajectories are not bit-comparable)."""
    render, _ = rm
    pts, tcol, start = R.fit_problem()
    first, last = R.fit_run(lambda x, c, col, r: render.sdf_field(x, c, col, r, R.FIT_K, color_sharpness=R.FIT_CS),
                            dev(pts), dev(tcol), start)
    print(f"fit through render.sdf_field: loss {first:.5f} -> {last:.5f} ({last / first:.4f} of the start)")
    record_margin("sdf_field_fit", last / first, 0.05)
    assert last <= 0.05 * first, (first, last)
