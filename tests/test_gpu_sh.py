"""GPU tests of the view-dependent sphere colour (rm_render_diff_sh, rm_render_diff_sh_backward, their camera
forms and render.render_diff_sh) against torch autograd of the fp64 restatement (tests/sh_ref.py).

Parity bounds. Nothing is fixed by hand: per case, for out and for each of the six gradient groups, the bound
is 8 times the max error of the restatement's float32 run against its fp64 run over the case's 576 rays, and
holds for every ray count N (the first N rays and seeds). Figures are printed and recorded
(conftest.record_margin).

Additivity (tests/additivity_ref.py): a call on one block's 256 rays alone returns that block's partial record
bit for bit, so the full call is held to the fp32 summation bound of its own terms, no tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import additivity_ref as AD
import sh_ref as R
from conftest import gpu_available, record_margin

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

GUARD = 64
SENT = 1234.5
SCENE_KEYS = ("centers", "colors", "radius", "light_dir", "ambient")
ALL = SCENE_KEYS + ("sh",)


@pytest.fixture(scope="module")
def rm():
    from burn_raymarching_amd import _build
    _build.build_lib()
    from burn_raymarching_amd import native, render
    torch.cuda.init()
    return render, native


def dev(x, dtype=np.float32):
    return torch.from_numpy(np.array(x, dtype)).cuda()


def bits(t):
    return t.detach().cpu().numpy().tobytes()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def scene_of(rm, c, half=False):
    render, _ = rm
    sc = c["scene"]
    col = dev(sc["colors"])
    return render.Scene(dev(sc["centers"]), col.half() if half else col, dev(sc["radius"]), dev(sc["light_dir"]),
                        dev(sc["ambient"]))


def march_of(rm, c, scene, flags=0):
    _, native = rm
    return scene.march_for(native.march_params(c["steps"], c["k"], R.CONSTS["normal_eps"], R.CONSTS["color_sharpness"],
                                               R.CONSTS["mask_sharpness"], skip_escaped=False, flags=flags))


class Outputs:
    """The outputs of one backward call, each inside its own buffer with GUARD sentinel words on both sides."""

    def __init__(self, m, nb, want, prior=None):
        shapes = {"centers": (m, 3), "colors": (m, 3), "radius": (m,), "light_dir": (3,), "ambient": (1,), "sh": (m, nb, 3)}
        self.buf, self.out = {}, {}
        for k in ALL:
            size = int(np.prod(shapes[k]))
            b = torch.full((size + 2 * GUARD,), SENT, device="cuda")
            v = b[GUARD:GUARD + size].view(shapes[k])
            if k in want:
                if prior is not None:
                    v.copy_(prior[k])
                else:
                    v.fill_(float("nan"))
            self.buf[k], self.out[k] = b, v
        self.want = tuple(want)

    def ptr(self, k):
        return ctypes.c_void_p(self.out[k].data_ptr()) if k in self.want else None

    def guards_intact(self):
        """The guard words of every buffer, and the whole buffer of an output that was not requested."""
        ok = True
        for k, b in self.buf.items():
            if k in self.want:
                ok = ok and bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + self.out[k].numel():] == SENT).all())
            else:
                ok = ok and bool((b == SENT).all())
        return ok

    def host(self):
        return {k: self.out[k].cpu().numpy() for k in self.want}


def backward(rm, c, n, want=ALL, accumulate=0, prior=None, t=None, rays=None, gout=None, half=False, flags=0, degree=None,
             sh=None, cams=None, width=None, num=None, grads_null=False):
    """rm_render_diff_sh_backward (cams: its camera form) through ctypes on the case's first n rays (rays /
    gout: other device tensors). Returns (rc, Outputs)."""
    render, native = rm
    scene = scene_of(rm, c, half)
    m = scene.num_spheres
    sh_t = dev(c["sh"]) if sh is None else sh
    deg = c["degree"] if degree is None else degree
    o = Outputs(m, c["sh"].shape[1], want, prior)
    g = native.RmGrads(*[o.ptr(k) for k in SCENE_KEYS])
    march = march_of(rm, c, scene, flags)
    ctx = render.context()
    go = dev(c["grad_out"][:n]) if gout is None else gout
    cs = scene.c_struct()
    if cams is not None:
        rc = ctx._lib.rm_render_diff_sh_backward_camera(ctx.handle, native.cameras(cams), len(cams), width, width,
                                                        ctypes.byref(cs), ptr(sh_t), deg, ctypes.byref(march), ptr(go),
                                                        ptr(t), None if grads_null else ctypes.byref(g), o.ptr("sh"),
                                                        accumulate)
    else:
        ro, rd = (dev(c["org"][:n]), dev(c["dir"][:n])) if rays is None else rays
        rc = ctx._lib.rm_render_diff_sh_backward(ctx.handle, ptr(ro), ptr(rd), n if num is None else num, ctypes.byref(cs),
                                                 ptr(sh_t), deg, ctypes.byref(march), ptr(go), ptr(t),
                                                 None if grads_null else ctypes.byref(g), o.ptr("sh"), accumulate)
    torch.cuda.synchronize()
    return rc, o


def forward(rm, c, n, half=False, flags=0, return_t=True):
    render, _ = rm
    return render.render_diff_sh_forward(dev(c["org"][:n]), dev(c["dir"][:n]), scene_of(rm, c, half), dev(c["sh"]), c["k"],
                                         c["steps"], return_t=return_t, flags=flags, **R.CONSTS)


def check(tag, got, ref, bound, keys):
    bad = []
    for q in keys:
        e = R.max_err(got[q], ref[q])
        print(f"sh parity {tag} {q}: gpu {e:.3e} bound {bound[q]:.3e}")
        record_margin(f"sh_{q}_{tag}", e, bound[q])
        if not e <= bound[q]:
            bad.append((q, e, bound[q]))
    assert all(np.isfinite(np.asarray(got[q])).all() for q in keys)
    assert not bad, (tag, bad)


# ---- 1. parity ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", R.COUNTS)
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_parity_against_fp64_autograd(rm, name, n):
    c = R.case(name)
    bound, ref = R.bounds(c), R.reference(c, n)
    out, t = forward(rm, c, n)
    rc, o = backward(rm, c, n, t=t)
    assert rc == 0 and o.guards_intact()
    got = dict(o.host(), out=out.cpu().numpy())
    check(f"{name}_{n}", got, ref, bound, ("out",) + ALL)


# ---- 2. zero coefficients ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["m33_d2", "m48_d1"])
def test_zero_coefficients_against_the_oracle(rm, oracle, name):
    """sh = 0: out and the five scene gradients against the existing fp64 oracle path (no SH anywhere in it),
    under the bounds the convention gives this case; grad_sh is non-zero all the same and meets its bound."""
    c = R.case(name, zero_sh=True)
    n = 576
    bound = R.bounds(c)
    out, t = forward(rm, c, n)
    rc, o = backward(rm, c, n, t=t)
    assert rc == 0 and o.guards_intact()
    ref = oracle.render_diff_backward(c["org"], c["dir"], c["scene"], c["steps"], c["k"], c["grad_out"], "f64", **R.CONSTS)
    ref["out"] = oracle.render_diff(c["org"], c["dir"], c["scene"], c["steps"], c["k"], "f64", **R.CONSTS)
    ref["ambient"] = np.asarray(ref["ambient"]).reshape(-1)
    got = dict(o.host(), out=out.cpu().numpy())
    check(f"{name}_zero_sh_oracle", got, ref, bound, ("out",) + SCENE_KEYS)
    check(f"{name}_zero_sh", got, R.reference(c, n), bound, ("sh",))
    assert np.abs(got["sh"]).max() > 100 * bound["sh"]


# ---- 3. degree 0 -------------------------------------------------------------------------------------

def test_degree_zero_is_the_existing_entry_point(rm):
    render, native = rm
    c = R.case("m33_d2")
    n = 576
    scene = scene_of(rm, c)
    o, d, go = dev(c["org"]), dev(c["dir"]), dev(c["grad_out"])
    base_out, base_t = render.render_diff_forward(o, d, scene, c["k"], c["steps"], return_t=True, **R.CONSTS)
    base_g = render.render_diff_backward(o, d, scene, c["k"], go, c["steps"], t_march=base_t, **R.CONSTS)
    ctx = render.context()
    march = march_of(rm, c, scene)
    out, t = torch.empty((n, 3), device="cuda"), torch.empty((n,), device="cuda")
    cs = scene.c_struct()
    # sh is ignored at degree 0: a buffer of NaN would show in the bits if any of it were read
    poison = torch.full((scene.num_spheres, 8, 3), float("nan"), device="cuda")
    rc = ctx._lib.rm_render_diff_sh(ctx.handle, ptr(o), ptr(d), n, ctypes.byref(cs), ptr(poison), 0, ctypes.byref(march),
                                    ptr(out), ptr(t))
    assert rc == 0 and bits(out) == bits(base_out) and bits(t) == bits(base_t)
    rc, got = backward(rm, c, n, t=t, degree=0, sh=poison)
    assert rc == 0 and got.guards_intact()
    assert all(bits(got.out[k]) == bits(base_g[k]) for k in SCENE_KEYS)
    assert torch.isnan(got.out["sh"]).all()  # untouched: as Outputs filled it
    # out-of-range degrees and a missing coefficient array are refused, and name the field
    for deg, sh, word in ((3, dev(c["sh"]), "sh_degree"), (-1, dev(c["sh"]), "sh_degree")):
        rc, bad = backward(rm, c, n, t=t, degree=deg, sh=sh)
        assert rc == 1 and word in ctx._lib.rm_last_error(ctx.handle).decode()
        assert all(torch.isnan(bad.out[k]).all() for k in ALL) and bad.guards_intact()
    rc = ctx._lib.rm_render_diff_sh(ctx.handle, ptr(o), ptr(d), n, ctypes.byref(cs), None, 2, ctypes.byref(march), ptr(out),
                                    ptr(t))
    assert rc == 1 and "sh is NULL" in ctx._lib.rm_last_error(ctx.handle).decode()
    rc, bad = backward(rm, c, n, t=t, want=())
    assert rc == 1 and "output" in ctx._lib.rm_last_error(ctx.handle).decode()
    rc, only_sh = backward(rm, c, n, t=t, want=("sh",), grads_null=True)
    assert rc == 0 and torch.isfinite(only_sh.out["sh"]).all() and only_sh.guards_intact()
    # N = 0: zeros at accumulate = 0, nothing at accumulate = 1
    rc, z = backward(rm, c, n, t=t, num=0)
    assert rc == 0 and z.guards_intact() and all(not z.out[k].any() for k in ALL)
    rc, z = backward(rm, c, n, t=t, num=0, accumulate=1)
    assert rc == 0 and all(torch.isnan(z.out[k]).all() for k in ALL)


# ---- 4. camera mode ----------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [32, 24])
def test_camera_mode(rm, width):
    """Camera mode at 32 x 32 (16 x 16 tiles) and 24 x 24 (rows): with RM_MARCH_ROW_ORDER out has array mode's
    bits on create_camera_rays' rays, and the gradients meet the parity bounds in both orders."""
    render, native = rm
    cam = R.CAMERA
    c = R.camera_case(width)
    bound, ref = R.bounds(c), R.reference(c)
    scene, sh = scene_of(rm, c), dev(c["sh"])
    arr_out, _ = forward(rm, c, None)
    for flags in (native.RM_MARCH_ROW_ORDER, 0):
        out, t = render.render_diff_sh_camera([cam], width, width, scene, sh, c["k"], c["steps"], return_t=True, flags=flags,
                                              **R.CONSTS)
        if flags:
            assert bits(out) == bits(arr_out)
        rc, got = backward(rm, c, None, t=t, cams=[cam], width=width, flags=flags)
        assert rc == 0 and got.guards_intact()
        check(f"m48_d1_cam{width}_flags{flags}", dict(got.host(), out=out.cpu().numpy()), ref, bound, ("out",) + ALL)


# ---- 5. saved t against the replayed march -----------------------------------------------------------

@pytest.mark.parametrize("name", ["m3_d2", "m300_d1"])
def test_saved_t_has_the_replayed_marchs_bits(rm, name):
    c = R.case(name)
    n = 576
    out, t = forward(rm, c, n)
    assert bits(forward(rm, c, n, return_t=False)) == bits(out)
    rc, saved = backward(rm, c, n, t=t)
    rc2, replayed = backward(rm, c, n)
    assert rc == 0 and rc2 == 0
    assert all(bits(saved.out[k]) == bits(replayed.out[k]) for k in ALL)


# ---- 6. additivity and sub-launches ------------------------------------------------------------------

def packed(o):
    """The outputs that are sums of the blocks' rows. light_dir is not one: it is light_grad's projection of the
    summed light terms, which travel in the same eight scalars of the record as ambient's."""
    return np.concatenate([o.out[k].cpu().numpy().astype(np.float64).reshape(-1) for k in ALL if k != "light_dir"])


def blocks_problem(c, nblocks, seed, zero_blocks=()):
    """nblocks x 256 rays aimed at the scene's ball from eyes on a sphere of 2.5, and seeds from N(0, 1)."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    n = nblocks * 256
    eye = torch.randn((n, 3), device="cuda", generator=gen)
    eye = 2.5 * eye / eye.norm(dim=1, keepdim=True)
    aim = (torch.rand((n, 3), device="cuda", generator=gen) - 0.5) * 0.8
    d = aim - eye
    d = d / d.norm(dim=1, keepdim=True)
    g = torch.randn((n, 3), device="cuda", generator=gen)
    for b in zero_blocks:
        g[b * 256:(b + 1) * 256] = 0
    return eye.contiguous(), d.contiguous(), g


def additivity(rm, c, o, d, g, blocks, tag):
    n = o.shape[0]
    big = torch.full_like(g, float(2 ** 40))  # poison: whatever this leaves in the workspace must not be read
    assert backward(rm, c, n, rays=(o, d), gout=big)[0] == 0
    rc, full = backward(rm, c, n, rays=(o, d), gout=g)
    assert rc == 0 and full.guards_intact()
    rows = []
    for b in blocks:
        s = slice(b * 256, min((b + 1) * 256, n))
        rc, r = backward(rm, c, s.stop - s.start, rays=(o[s].contiguous(), d[s].contiguous()), gout=g[s].contiguous())
        assert rc == 0
        rows.append(packed(r))
    ok, ratio, nz = AD.measure(packed(full), np.stack(rows))
    print(f"sh additivity {tag}: worst err / bound {ratio:.3f} over {nz} non-zero rows")
    record_margin(f"sh_additivity_{tag}", ratio, 1.0)
    assert ok, (tag, ratio, nz)
    return full


def test_additivity(rm, monkeypatch):
    monkeypatch.delenv("RM_MAX_BLOCKS_PER_LAUNCH", raising=False)
    c = R.case("m33_d2")
    o, d, g = blocks_problem(c, 3, 41)
    additivity(rm, c, o[:668], d[:668], g[:668], range(3), "m33_d2_3_blocks")


def test_additivity_sub_launches_and_accumulate(rm, monkeypatch):
    """RM_MAX_BLOCKS_PER_LAUNCH=2: seven blocks in four launches, the later ones accumulating into the first's
    result; then accumulate = 1 on a random prior: float32(G0 + G), one addition."""
    c = R.case("m300_d1")
    o, d, g = blocks_problem(c, 7, 47)
    monkeypatch.setenv("RM_MAX_BLOCKS_PER_LAUNCH", "2")
    full = additivity(rm, c, o, d, g, range(7), "m300_d1_7_blocks_by_2")
    monkeypatch.delenv("RM_MAX_BLOCKS_PER_LAUNCH", raising=False)
    rc, one = backward(rm, c, o.shape[0], rays=(o, d), gout=g)
    assert rc == 0
    rng = np.random.default_rng(3)
    prior = {k: dev(rng.normal(size=tuple(v.shape))) for k, v in one.out.items()}
    rc, acc = backward(rm, c, o.shape[0], rays=(o, d), gout=g, accumulate=1, prior=prior)
    assert rc == 0 and acc.guards_intact()
    for k in ALL:
        want = prior[k].cpu().numpy() + one.out[k].cpu().numpy()
        assert want.dtype == np.float32 and acc.out[k].cpu().numpy().tobytes() == want.tobytes(), k
    assert np.isfinite(packed(full)).all()


# ---- 7. / 8. bit-level repeatability, guard words, zero seeds ----------------------------------------

def test_bit_level_pins(rm, monkeypatch):
    monkeypatch.delenv("RM_MAX_BLOCKS_PER_LAUNCH", raising=False)
    c = R.case("m520_d2")
    n = 576
    _, t = forward(rm, c, n)
    rc, full = backward(rm, c, n, t=t)  # outputs pre-filled with NaN
    assert rc == 0 and full.guards_intact() and all(torch.isfinite(v).all() for v in full.out.values())
    rc, again = backward(rm, c, n, t=t)
    assert rc == 0 and all(bits(full.out[k]) == bits(again.out[k]) for k in ALL)
    # each output alone, and two pairs, have the full call's bits; what is not requested is not written
    # (light_dir and ambient among them: Outputs.guards_intact checks their whole buffers)
    for want in [(k,) for k in ALL] + [("centers", "sh"), ("light_dir", "colors")]:
        rc, part = backward(rm, c, n, t=t, want=want)
        assert rc == 0 and part.guards_intact(), want
        assert all(bits(part.out[k]) == bits(full.out[k]) for k in want), want


def test_zero_seed_rays_and_blocks(rm, monkeypatch):
    """A block of zero-seed rays writes exact zeros and adds exact zeros; so do zero seeds inside a live block."""
    monkeypatch.delenv("RM_MAX_BLOCKS_PER_LAUNCH", raising=False)
    c = R.case("m33_d2")
    o, d, g = blocks_problem(c, 5, 51, zero_blocks=(0, 2, 4))
    full = additivity(rm, c, o, d, g, range(5), "m33_d2_5_blocks_3_dead")
    for b in (0, 2, 4):
        s = slice(b * 256, (b + 1) * 256)
        rc, r = backward(rm, c, 256, rays=(o[s].contiguous(), d[s].contiguous()), gout=g[s].contiguous())
        assert rc == 0 and r.guards_intact() and not any(v.any() for v in r.out.values())
    keep = torch.cat([torch.arange(256, 512), torch.arange(768, 1024)]).cuda()
    rc, only = backward(rm, c, 512, rays=(o[keep].contiguous(), d[keep].contiguous()), gout=g[keep].contiguous())
    assert rc == 0 and all(bits(full.out[k]) == bits(only.out[k]) for k in ALL)
    # escaped rays (aimed away from the scene) are zero-seed rays whatever grad_out is
    rc, away = backward(rm, c, 256, rays=(o[:256].contiguous(), (-d[:256]).contiguous()), gout=torch.ones_like(g[:256]))
    assert rc == 0 and not any(v.any() for v in away.out.values())


# ---- 9. fp16 colours ---------------------------------------------------------------------------------

def test_fp16_colours(rm):
    """RM_MARCH_COLOR_F16 at M = 48: parity against the restatement on the rounded colours, and the bits of the
    fp32 call on the rounded colours; sh and every gradient stay fp32."""
    c0, c = R.case("m48_d1"), R.f16_case()
    n = 576
    bound, ref = R.bounds(c), R.reference(c, n)
    out_h, t_h = forward(rm, c, n, half=True)
    rc, h = backward(rm, c, n, t=t_h, half=True)
    assert rc == 0 and h.guards_intact()
    check("m48_d1_f16", dict(h.host(), out=out_h.cpu().numpy()), ref, bound, ("out",) + ALL)
    out_f, t_f = forward(rm, c, n)
    rc, f = backward(rm, c, n, t=t_f)
    assert rc == 0 and bits(out_h) == bits(out_f) and all(bits(h.out[k]) == bits(f.out[k]) for k in ALL)
    out_raw, _ = forward(rm, c0, n)
    assert bits(out_raw) != bits(out_h)


# ---- 10. the autograd function -----------------------------------------------------------------------

def test_render_diff_sh_autograd(rm):
    render, _ = rm
    c = R.case("m33_d2")
    n = 576
    sc = c["scene"]
    out_raw, t = forward(rm, c, n)
    rc, ref = backward(rm, c, n, t=t)
    assert rc == 0
    leaf = {k: dev(sc[k]).requires_grad_(True) for k in SCENE_KEYS}
    sh = dev(c["sh"]).requires_grad_(True)
    o, d, go = dev(c["org"]), dev(c["dir"]), dev(c["grad_out"])
    out = render.render_diff_sh(o, d, leaf["centers"], leaf["colors"], sh, leaf["radius"], leaf["light_dir"],
                                leaf["ambient"], c["k"], c["steps"], **R.CONSTS)
    assert bits(out) == bits(out_raw)
    out.backward(go)
    assert bits(sh.grad) == bits(ref.out["sh"])
    assert all(bits(leaf[k].grad) == bits(ref.out[k]) for k in SCENE_KEYS)
    # only the inputs that require grad are computed: sh alone
    sh2 = dev(c["sh"]).requires_grad_(True)
    out2 = render.render_diff_sh(o, d, dev(sc["centers"]), dev(sc["colors"]), sh2, dev(sc["radius"]), dev(sc["light_dir"]),
                                 dev(sc["ambient"]), c["k"], c["steps"], **R.CONSTS)
    (g2,) = torch.autograd.grad(out2, sh2, go)
    assert bits(g2) == bits(ref.out["sh"])
    # no coefficients: render_diff itself
    base = render.render_diff(o, d, dev(sc["centers"]), dev(sc["colors"]), dev(sc["radius"]), dev(sc["light_dir"]),
                              dev(sc["ambient"]), c["k"], c["steps"], **R.CONSTS)
    none = render.render_diff_sh(o, d, dev(sc["centers"]), dev(sc["colors"]), sh[:, :0, :].detach(), dev(sc["radius"]),
                                 dev(sc["light_dir"]), dev(sc["ambient"]), c["k"], c["steps"], **R.CONSTS)
    assert bits(none) == bits(base)
    # rays that require grad: an error, not silent zeros
    with pytest.raises(ValueError, match="ray gradients are not available with SH"):
        render.render_diff_sh(o.clone().requires_grad_(True), d, dev(sc["centers"]), dev(sc["colors"]), sh, dev(sc["radius"]),
                              dev(sc["light_dir"]), dev(sc["ambient"]), c["k"], c["steps"], **R.CONSTS)


def test_fit_demonstration(rm):
    """The fit of tests/test_sh_reference.py through render.render_diff_sh in fp32: colours and degree-1
    coefficients end below colours alone."""
    render, _ = rm
    c, target = R.fit_problem()

    def fn(o, d, cen, col, sh, r, ld, amb):
        return render.render_diff_sh(o, d, cen, col, sh, r, ld, amb, R.K, R.FIT_STEPS, **R.CONSTS)

    like = torch.zeros((), device="cuda")
    both = R.fit_run(fn, c, target, True, like)
    alone = R.fit_run(fn, c, target, False, like)
    print(f"sh fit through render.render_diff_sh: colours and sh {both:.3e}, colours alone {alone:.3e}")
    record_margin("sh_fit", both, alone)
    assert both < alone, (both, alone)
