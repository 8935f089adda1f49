"""GPU tests of the torch autograd layer's contract: the five torch.autograd.Functions of render.py
(render_diff, render_diff_cameras, render_diff_sh, sdf_field, image_loss) called the way an optimisation loop
written in torch calls them -- slices of one packed parameter buffer, non-leaf activated tensors, in-place
updates between a forward and a later backward, retain_graph, create_graph, side streams, [M,1] / [1,3] / 0-d
shapes.

Every assertion is bitwise or an expected exception; the file adds no tolerance. The reference of each Function
is the same Function on contiguous float32 leaves of the canonical shapes (`plain`), computed once: that call is
what tests/test_gpu_raygrad.py (section 5), test_gpu_sh.py, test_gpu_sdf_grad.py, test_gpu_loss.py and
test_gpu_context_families.py hold to the low-level calls and those to their fp64 restatements. The inputs are
theirs: C1 (6 spheres, the small-scene kernel) and C3 (64 spheres, the general kernel) of test_gpu_raygrad at
576 rays, two of C9's views at 20 x 24, sh_ref's m3_d1 and m33_d2 at 576 rays, the first 257 points of
test_gpu_sdf's m33 pool with sdf_grad_ref's seeds, ssim_ref.images(2, 24, 40): ragged last blocks and a ragged
loss tile. The layouts are tests/autograd_layouts.py's, each held to its claim by tests/test_autograd_layouts.py."""
import functools
import gc

import numpy as np
import pytest
import torch

import autograd_layouts as L
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

SCENE = ("centers", "colors", "radius", "light_dir", "ambient")
NAMES = ("render_diff_small", "render_diff_general", "render_diff_cameras", "render_diff_sh_d1", "render_diff_sh_d2",
         "sdf_field", "image_loss")
INPLACE = "modified by an inplace operation"


@pytest.fixture(scope="module")
def rm():
    from burn_raymarching_amd import _build
    _build.build_lib()
    from burn_raymarching_amd import render
    torch.cuda.init()
    return render


class Spec:
    """One Function at one case. arrays: its tensor arguments in call order (float32 numpy, canonical shapes);
    call(render, t) -> the tuple of its outputs; seeds: one upstream gradient per output; diff: the arguments
    that take a gradient; host: arguments that live on the host; by_value: arguments the layer reads at forward
    time and never again."""

    def __init__(self, name, arrays, call, seeds, diff, host=(), by_value=()):
        self.name, self.arrays, self.call, self.seeds = name, arrays, call, tuple(seeds)
        self.diff, self.host, self.by_value = tuple(diff), tuple(host), tuple(by_value)
        self.scene = tuple(k for k in SCENE if k in arrays)

    def __repr__(self):
        return self.name


def _f32(a):
    return np.array(a, np.float32)


def _raygrad_spec(name, case, views=None):
    import test_gpu_raygrad as RG
    from oracle import oracle as orc
    orc.build()
    make, k, steps, w, h, cams = RG.CASES[case]
    cams = [RG.cam(i) for i in (cams if views is None else cams[:views])]
    sc = make()
    scene = {key: _f32(sc[key]).reshape((-1, 3) if key in ("centers", "colors") else (-1,)) for key in SCENE}
    rng = np.random.default_rng(sum(map(ord, name)))
    if views is None:
        rays = [orc.camera_rays(w, h, *c, precision="f32") for c in cams]
        arrays = {"ray_org": _f32(np.concatenate([r[0] for r in rays])), "ray_dir": _f32(np.concatenate([r[1] for r in rays]))}
        arrays.update(scene)
        n = arrays["ray_org"].shape[0]

        def call(render, t):
            return (render.render_diff(t["ray_org"], t["ray_dir"], *(t[key] for key in SCENE), k, steps),)
        return Spec(name, arrays, call, [_f32(rng.standard_normal((n, 3)))], tuple(arrays))
    arrays = {"eye": _f32([c[0] for c in cams]), "target": _f32([c[1] for c in cams]), "fov_deg": _f32([c[2] for c in cams])}
    arrays.update(scene)

    def call(render, t):
        return (render.render_diff_cameras(t["eye"], t["target"], t["fov_deg"], w, h, *(t[key] for key in SCENE), k, steps),)
    cam_args = ("eye", "target", "fov_deg")
    return Spec(name, arrays, call, [_f32(rng.standard_normal((len(cams) * w * h, 3)))], tuple(arrays), host=cam_args,
                by_value=cam_args)


def _sh_spec(name, case):
    import sh_ref as R
    c = R.case(case)
    sc = c["scene"]
    arrays = {"ray_org": _f32(c["org"]), "ray_dir": _f32(c["dir"]), "centers": _f32(sc["centers"]), "colors": _f32(sc["colors"]),
              "sh": _f32(c["sh"]), "radius": _f32(sc["radius"]).reshape(-1), "light_dir": _f32(sc["light_dir"]).reshape(3),
              "ambient": _f32(sc["ambient"]).reshape(1)}

    def call(render, t):
        return (render.render_diff_sh(t["ray_org"], t["ray_dir"], t["centers"], t["colors"], t["sh"], t["radius"],
                                      t["light_dir"], t["ambient"], c["k"], c["steps"], **R.CONSTS),)
    return Spec(name, arrays, call, [_f32(c["grad_out"])], ("centers", "colors", "sh", "radius", "light_dir", "ambient"))


def _sdf_spec(name):
    import sdf_grad_ref as G
    from test_gpu_sdf import CSHARP, K, pool
    n = 257
    sc, pts, _, _, _ = pool("m33")
    gD, gC = G.seed_sets(len(pts))["both"]
    arrays = {"points": _f32(pts[:n]), "centers": _f32(sc["centers"]), "colors": _f32(sc["colors"]),
              "radius": _f32(sc["radius"]).reshape(-1)}

    def call(render, t):
        return tuple(render.sdf_field(t["points"], t["centers"], t["colors"], t["radius"], K, color_sharpness=CSHARP))
    return Spec(name, arrays, call, [_f32(gD[:n]), _f32(gC[:n])], tuple(arrays))


def _loss_spec(name):
    import ssim_ref as S
    v, h, w = 2, 24, 40
    x, y = S.images(v, h, w)

    def call(render, t):
        return (render.image_loss(t["out"], t["target"], w, h),)
    return Spec(name, {"out": _f32(x), "target": _f32(y)}, call, [_f32(0.75)], ("out",), by_value=("out", "target"))


@functools.lru_cache(maxsize=None)
def spec(name):
    s = {"render_diff_small": lambda: _raygrad_spec(name, "C1"), "render_diff_general": lambda: _raygrad_spec(name, "C3"),
         "render_diff_cameras": lambda: _raygrad_spec(name, "C9", views=2),
         "render_diff_sh_d1": lambda: _sh_spec(name, "m3_d1"), "render_diff_sh_d2": lambda: _sh_spec(name, "m33_d2"),
         "sdf_field": lambda: _sdf_spec(name), "image_loss": lambda: _loss_spec(name)}[name]()
    n = max(a.shape[0] if a.ndim else 1 for a in s.arrays.values())
    assert n <= 576 or name == "image_loss", (name, n)  # at most 576 rays or points; two views of at most 40 x 24
    return s


def tensors(s, arrays=None):
    """Fresh contiguous tensors of the spec's arguments: on the device, but for the host arguments."""
    return {k: torch.from_numpy(_f32(a)) if k in s.host else torch.from_numpy(_f32(a)).cuda()
            for k, a in (arrays or s.arrays).items()}


def seed_tensors(s, seeds=None):
    return [torch.from_numpy(_f32(g)).cuda() for g in (seeds or s.seeds)]


def leaves_of(s, tens, need=None):
    """The tensors as the Function's inputs: detached (the storage and the strides stay), the ones named in
    `need` (default: every differentiable argument) leaves that require grad."""
    need = s.diff if need is None else need
    return {k: t.detach().requires_grad_() if k in need else t.detach() for k, t in tens.items()}


def run(render, s, tens, seeds, need=None):
    lv = leaves_of(s, tens, need)
    outs = s.call(render, lv)
    torch.autograd.backward(outs, seeds)
    return outs, lv


_REF = {}


def reference(render, s, tag="base", arrays=None, seeds=None, need=None):
    """(outputs, {argument: gradient}) of the Function on plain leaves, computed once per (spec, tag, need)."""
    need = s.diff if need is None else tuple(need)
    key = (s.name, tag, need)
    if key not in _REF:
        outs, lv = run(render, s, tensors(s, arrays), seed_tensors(s, seeds), need)
        _REF[key] = ([o.detach().clone() for o in outs], {k: lv[k].grad.detach().clone() for k in need})
    return _REF[key]


def check(s, outs, lv, ref, what, need=None):
    """The outputs and every gradient have the reference's bits, and each gradient its input's shape."""
    for i, (o, r) in enumerate(zip(outs, ref[0])):
        assert L.same_bits(o, r), (s.name, what, "output", i)
    for k in (s.diff if need is None else need):
        g = lv[k].grad
        assert g is not None, (s.name, what, k, "no gradient")
        assert tuple(g.shape) == tuple(lv[k].shape), (s.name, what, k, tuple(g.shape), tuple(lv[k].shape))
        assert L.same_bits(g.reshape(ref[1][k].shape), ref[1][k]), (s.name, what, "gradient of", k)


# ---- the reference itself ------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_reference_run_is_alive_and_repeatable(rm, name):
    """Finite, non-zero outputs and gradients (equal bits of zeros would prove nothing), the same bits twice."""
    s = spec(name)
    ref = reference(rm, s)
    for t in ref[0] + list(ref[1].values()):
        assert torch.isfinite(t).all() and t.abs().max() > 0, name
    outs, lv = run(rm, s, tensors(s), seed_tensors(s))
    check(s, outs, lv, ref, "second plain run")


# ---- layouts -------------------------------------------------------------------------------------

SINGLE = ("col_slice", "transposed", "row_stride", "offset1", "expanded")


def _variants(s, arg, layout):
    """(tag, arrays, seeds) of the runs of one argument in one layout. `expanded` needs values that allow it:
    every sphere of one colour, and the grad_out of ones that .sum() hands back."""
    if layout != "expanded":
        return [("base", None, None)]
    if arg == "colors":
        arrays = dict(s.arrays, colors=np.repeat(s.arrays["colors"][:1], s.arrays["colors"].shape[0], 0))
        return [("one_colour", arrays, None)]
    if arg == "grad_out":
        return [("ones", None, [np.ones_like(g) for g in s.seeds])]
    return []


@pytest.mark.parametrize("layout", SINGLE)
@pytest.mark.parametrize("name", NAMES)
def test_every_argument_in_each_layout(rm, name, layout):
    """One argument at a time (and the upstream gradients, through torch.autograd.backward) in the layout, the
    others plain: the plain run's bits, gradients in the inputs' shapes."""
    s = spec(name)
    ran = []
    for arg in list(s.arrays) + ["grad_out"]:
        for tag, arrays, seeds in _variants(s, arg, layout):
            ref = reference(rm, s, tag, arrays, seeds)
            tens, sd = tensors(s, arrays), seed_tensors(s, seeds)
            if arg == "grad_out" and layout == "expanded":
                lv = leaves_of(s, tens)
                outs = s.call(rm, lv)
                sum(o.sum() for o in outs).backward()  # torch's own expanded ones
            else:
                if arg == "grad_out":
                    made = [getattr(L, layout)(g) for g in sd]
                    if all(m is None for m in made):
                        continue
                    assert all(m is None or L.claim_holds(layout, m) for m in made)
                    sd = [g if m is None else m for g, m in zip(sd, made)]
                else:
                    made = getattr(L, layout)(tens[arg])
                    if made is None:
                        continue
                    assert L.claim_holds(layout, made) and L.same_bits(made, tens[arg]), (arg, layout)
                    tens[arg] = made
                outs, lv = run(rm, s, tens, sd)
            check(s, outs, lv, ref, (arg, layout))
            ran.append(arg)
    if layout == "expanded":
        assert ran == [a for a in ("colors", "grad_out") if a == "grad_out" or a in s.arrays], ran
    elif layout == "transposed":
        assert ran or name == "image_loss", ran  # the loss has no 2-D argument
    else:
        # every argument of more than one row (ambient has one), and grad_out (the loss's is 0-d: offset1 only)
        assert len(ran) >= len(s.arrays) - 1 and ("grad_out" in ran or name == "image_loss"), ran


@pytest.mark.parametrize("name", [n for n in NAMES if n != "image_loss"])
def test_scene_as_views_of_one_packed_vector(rm, name):
    """The `packed` layout: every scene tensor a view into one flat vector, all at once."""
    s = spec(name)
    tens = tensors(s)
    flat, views = L.packed({k: tens[k] for k in s.scene})
    assert all(L.claim_holds("packed", v) for v in views.values())
    tens.update(views)
    outs, lv = run(rm, s, tens, seed_tensors(s))
    check(s, outs, lv, reference(rm, s), "packed")
    assert not torch.isnan(flat[1:]).any() and torch.isnan(flat[0])


def _activate(flat, m, names):
    """model.SceneModel's activation (scene.rs:41-45) in torch, on views of the packed raw vector `flat`
    (one leading word, then model.pack's order)."""
    at, act = 1, {}
    for k in names:
        size = {"centers": 3 * m, "colors": 3 * m, "radius": m, "light_dir": 3, "ambient": 1}[k]
        raw = flat[at:at + size]
        at += size
        if k in ("centers", "colors"):
            raw = raw.view(m, 3)
        act[k] = {"centers": lambda r: r, "light_dir": lambda r: r, "colors": torch.sigmoid, "ambient": torch.sigmoid,
                  "radius": lambda r: torch.nn.functional.softplus(r) + 0.01}[k](raw)
    return act


@pytest.mark.parametrize("name", [n for n in NAMES if n != "image_loss"])
def test_packed_raw_parameters_through_the_activation(rm, name):
    """raw (one leaf) -> the model's activation in torch -> the Function -> (out * g).sum(): the centres and the
    light direction reach the Function as views of the leaf, the rest as non-leaf tensors. The activated
    parameters' gradients are the plain run's, and the raw gradient is torch's own backward of the activation
    from those."""
    from burn_raymarching_amd import model
    s = spec(name)
    a = s.arrays
    m = a["centers"].shape[0]
    raw_np = {"centers": a["centers"], "colors": model.logit(a["colors"]),
              "radius": model.softplus_inv(a["radius"].astype(np.float64) - 0.01)}
    if "light_dir" in a:
        raw_np.update(light_dir=a["light_dir"], ambient=model.logit(a["ambient"]))
    flat0 = torch.cat([torch.zeros(1)] + [torch.from_numpy(_f32(raw_np[k]).reshape(-1)) for k in s.scene]).cuda()

    flat = flat0.clone().requires_grad_()
    act = _activate(flat, m, s.scene)
    for v in act.values():
        assert not v.is_leaf
        v.retain_grad()
    assert act["centers"].storage_offset() == 1 and act["centers"].data_ptr() % 8 == 4
    tens = tensors(s)
    sd = seed_tensors(s)
    outs = s.call(rm, dict(tens, **act))
    sum((o * g).sum() for o, g in zip(outs, sd)).backward()

    plain = dict(s.arrays, **{k: v.detach().cpu().numpy() for k, v in act.items()})
    ref = reference(rm, s, "activated", plain, None, need=s.scene)
    for i, (o, r) in enumerate(zip(outs, ref[0])):
        assert L.same_bits(o, r), (name, "output", i)
    for k in s.scene:
        assert L.same_bits(act[k].grad, ref[1][k]), (name, "activated gradient", k)
    flat2 = flat0.clone().requires_grad_()
    act2 = _activate(flat2, m, s.scene)
    torch.autograd.backward([act2[k] for k in s.scene], [ref[1][k] for k in s.scene])
    assert flat.grad.abs().max() > 0 and L.same_bits(flat.grad, flat2.grad), name


# ---- shapes --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n in NAMES if n != "image_loss"])
def test_accepted_shapes_and_refused_ones(rm, name):
    s = spec(name)
    ref = reference(rm, s)
    for arg in ("radius", "ambient", "light_dir", "centers", "colors"):
        if arg not in s.arrays:
            continue
        base = tensors(s)[arg]
        for label, t in L.shapes(arg, base):
            tens = tensors(s)
            tens[arg] = t
            outs, lv = run(rm, s, tens, seed_tensors(s))
            check(s, outs, lv, ref, (arg, label))  # forward, backward, and the gradient in the input's shape
        for t in L.wrong_shapes(arg, base):
            tens = tensors(s)
            tens[arg] = t
            with pytest.raises(ValueError, match=rf"\b{arg}\b"):
                s.call(rm, leaves_of(s, tens))


# ---- argument errors -----------------------------------------------------------------------------

def _short(x):
    """x with one column (or, 1-D and 0-d, one element) too few or too many."""
    if x.dim() >= 2:
        return x[..., :2].contiguous()
    return torch.cat([x.reshape(-1), x.reshape(-1)[:1]])


@pytest.mark.parametrize("name", NAMES)
def test_argument_errors(rm, name):
    """Every tensor argument: float64 -> TypeError, a host tensor -> ValueError (but the camera tensors), a wrong
    shape -> ValueError; each message names the argument and each error leaves the forward call."""
    s = spec(name)
    table = []
    for arg in s.arrays:
        table.append((arg, "float64", TypeError, lambda t: t.double()))
        if arg not in s.host:
            table.append((arg, "host", ValueError, lambda t: t.cpu()))
        table.append((arg, "shape", ValueError, _short))
    assert len(table) == 3 * len(s.arrays) - len(s.host)
    for arg, what, exc, change in table:
        tens = tensors(s)
        tens[arg] = change(tens[arg])
        with pytest.raises(exc, match=rf"\b{arg}\b"):
            s.call(rm, leaves_of(s, tens))
        # nothing ran: a call with the arguments put right still has the reference's bits
    outs, lv = run(rm, s, tensors(s), seed_tensors(s))
    check(s, outs, lv, reference(rm, s), "after the refused calls")


def test_camera_tensors_on_the_device(rm):
    """The camera tensors may live on either side; their gradients come back where they live."""
    s = spec("render_diff_cameras")
    tens = {k: t.cuda() for k, t in tensors(s).items()}
    outs, lv = run(rm, s, tens, seed_tensors(s))
    assert all(lv[k].grad.is_cuda for k in s.host)
    check(s, outs, lv, reference(rm, s), "camera tensors on the device")


# ---- in-place changes between forward and backward -----------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_inplace_change_between_forward_and_backward(rm, name):
    """A contiguous float32 tensor the backward reads is the caller's own (no copy): changing it in place after
    the forward must raise torch's error. A tensor the layer had to copy, or takes by value, gives the
    gradients of the forward-time values."""
    s = spec(name)
    ref = reference(rm, s)
    for arg in s.arrays:
        lv = leaves_of(s, tensors(s))
        outs = s.call(rm, lv)
        with torch.no_grad():
            lv[arg].add_(0.25)  # what optimizer.step() or p.clamp_() does
        if arg in s.by_value:
            torch.autograd.backward(outs, seed_tensors(s))
            check(s, [], lv, ref, (arg, "by value"))
            continue
        with pytest.raises(RuntimeError, match=INPLACE):
            torch.autograd.backward(outs, seed_tensors(s))
        tens = tensors(s)
        made = L.col_slice(tens[arg])
        if made is None:  # one row: no non-contiguous form
            continue
        tens[arg] = made
        lv = leaves_of(s, tens)
        outs = s.call(rm, lv)
        with torch.no_grad():
            lv[arg].add_(0.25)
        torch.autograd.backward(outs, seed_tensors(s))
        check(s, [], lv, ref, (arg, "copied"))


@pytest.mark.parametrize("name", ["render_diff_small", "render_diff_cameras", "render_diff_sh_d2"])
def test_inplace_change_of_an_alternative_shape(rm, name):
    """radius [M,1], light_dir [1,3] and a 0-d ambient are flattened as views, not copies: they raise too."""
    s = spec(name)
    for arg in ("radius", "light_dir", "ambient"):
        tens = tensors(s)
        tens[arg] = list(L.shapes(arg, tens[arg]))[1][1]
        lv = leaves_of(s, tens)
        outs = s.call(rm, lv)
        with torch.no_grad():
            lv[arg].mul_(1.5)
        with pytest.raises(RuntimeError, match=INPLACE):
            torch.autograd.backward(outs, seed_tensors(s))


@pytest.mark.parametrize("name", [n for n in NAMES if n != "image_loss"])
def test_an_update_between_two_graphs_of_the_same_leaves(rm, name):
    """Two forwards from the same leaves, backward of the first, an in-place SGD step, backward of the second:
    the second graph was recorded on the old parameters and must say so."""
    s = spec(name)
    lv = leaves_of(s, tensors(s))
    first, second = s.call(rm, lv), s.call(rm, lv)
    torch.autograd.backward(first, seed_tensors(s))
    check(s, first, lv, reference(rm, s), "the first graph")
    with torch.no_grad():
        for k in s.diff:
            lv[k].sub_(1e-3 * lv[k].grad)
    with pytest.raises(RuntimeError, match=INPLACE):
        torch.autograd.backward(second, seed_tensors(s))


# ---- requires_grad subsets -----------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_requires_grad_subsets(rm, name):
    s = spec(name)
    ref = reference(rm, s)  # all inputs
    for arg in s.diff:
        outs, lv = run(rm, s, tensors(s), seed_tensors(s), need=(arg,))
        check(s, outs, lv, ref, ("alone", arg), need=(arg,))
        assert all(lv[k].grad is None for k in lv if k != arg), arg
    lv = leaves_of(s, tensors(s), need=())
    outs = s.call(rm, lv)
    assert all(o.grad_fn is None and not o.requires_grad for o in outs)
    check(s, outs, lv, ref, "no input requires grad", need=())
    lv = leaves_of(s, tensors(s))
    with torch.no_grad():
        outs = s.call(rm, lv)
    assert all(o.grad_fn is None and not o.requires_grad for o in outs)
    check(s, outs, lv, ref, "under no_grad", need=())


# ---- repeated and double backward ----------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_repeated_backward(rm, name):
    s = spec(name)
    ref = reference(rm, s)
    lv = leaves_of(s, tensors(s))
    outs = s.call(rm, lv)
    sd = seed_tensors(s)
    torch.autograd.backward(outs, sd, retain_graph=True)
    torch.autograd.backward(outs, sd, retain_graph=True)
    for k in s.diff:
        assert L.same_bits(lv[k].grad, ref[1][k] * 2.0), (name, k)  # g + g, exactly
    torch.autograd.backward(outs, sd)
    with pytest.raises(RuntimeError, match="backward through the graph a second time"):
        torch.autograd.backward(outs, sd)


@pytest.mark.parametrize("name", NAMES)
def test_double_backward_raises(rm, name):
    """The layer is first order only. The loss is quadratic in the outputs, so that the incoming gradient carries a
    graph (tests/test_autograd_layouts.py: torch arms a once-differentiable backward's error only then)."""
    s = spec(name)
    lv = leaves_of(s, tensors(s))
    outs = s.call(rm, lv)
    loss = sum((o * o * g).sum() for o, g in zip(outs, seed_tensors(s)))
    xs = [lv[k] for k in s.diff]
    gs = torch.autograd.grad(loss, xs, create_graph=True)
    assert all(g.requires_grad for g in gs)
    total = sum(g.sum().to("cuda") for g in gs) + sum(x.sum().to("cuda") for x in xs)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        total.backward()


# ---- streams -------------------------------------------------------------------------------------

@pytest.mark.parametrize("backward_on", ["side", "default"])
@pytest.mark.parametrize("name", NAMES)
def test_side_stream(rm, name, backward_on):
    """Forward and backward inside torch.cuda.stream(side), and forward on the side stream with backward called
    from the default stream: the reference's bits after a synchronize."""
    s = spec(name)
    ref = reference(rm, s)
    lv, sd = leaves_of(s, tensors(s)), seed_tensors(s)
    side = torch.cuda.Stream()
    key = (torch.cuda.current_device(), side.cuda_stream)
    rm._ctx_cache.pop(key, None)  # torch hands streams out of a pool: a context an earlier test left there
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(side):
            outs = s.call(rm, lv)
            if backward_on == "side":
                torch.autograd.backward(outs, sd)
        if backward_on == "default":
            torch.autograd.backward(outs, sd)
        torch.cuda.synchronize()
        check(s, outs, lv, ref, ("stream", backward_on))
    finally:
        torch.cuda.synchronize()
        rm._ctx_cache.pop(key, None)


# ---- lifetime ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_nothing_outlives_the_graph(rm, name):
    s = spec(name)
    lv, sd = leaves_of(s, tensors(s)), seed_tensors(s)
    xs = [lv[k] for k in s.diff]

    def once():
        outs = s.call(rm, lv)
        held = torch.cuda.memory_allocated()
        loss = sum((o * g).sum() for o, g in zip(outs, sd))
        gs = torch.autograd.grad(loss, xs)
        del outs, loss, gs
        return held

    once()  # warm-up
    gc.collect()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    held = once()
    gc.collect()
    torch.cuda.synchronize()
    assert held > before  # the outputs and what the graph saved were counted
    assert torch.cuda.memory_allocated() == before, (name, torch.cuda.memory_allocated() - before)


# ---- the low-level calls: float arrays need 4-byte alignment only ---------------------------------

def _both_alignments(call, arrays):
    """call(tensors) on aligned tensors and on offset1 views of them (data_ptr % 8 == 4): equal bits."""
    aligned = {k: torch.from_numpy(_f32(a)).cuda() for k, a in arrays.items()}
    odd = {k: L.offset1(t) for k, t in aligned.items()}
    assert all(t.data_ptr() % 8 == 0 for t in aligned.values()) and all(L.claim_holds("offset1", t) for t in odd.values())
    a, b = call(aligned), call(odd)
    assert len(a) == len(b) and len(a) > 0
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.isfinite(x).all() and L.same_bits(x, y), i


@pytest.mark.parametrize("name", ["render_diff_small", "render_diff_general"])
def test_low_level_render_calls_at_4_byte_alignment(rm, name):
    s = spec(name)
    k, steps = {"render_diff_small": (32.0, 40), "render_diff_general": (32.0, 32)}[name]
    _, t = rm.render_diff_forward(*(tensors(s)[key] for key in ("ray_org", "ray_dir")),
                                  rm.Scene(*(tensors(s)[key] for key in SCENE)), k, steps, return_t=True)

    def call(x):
        scene = rm.Scene(*(x[key] for key in SCENE))
        out, tm = rm.render_diff_forward(x["ray_org"], x["ray_dir"], scene, k, steps, return_t=True)
        g = rm.render_diff_backward(x["ray_org"], x["ray_dir"], scene, k, x["grad_out"], steps, t_march=x["t"])
        return [out, tm] + [g[key] for key in SCENE]
    _both_alignments(call, dict(s.arrays, grad_out=s.seeds[0], t=t.cpu().numpy()))


def test_low_level_sh_backward_at_4_byte_alignment(rm):
    import sh_ref as R
    s = spec("render_diff_sh_d2")
    c = R.case("m33_d2")
    x0 = tensors(s)
    _, t = rm.render_diff_sh_forward(x0["ray_org"], x0["ray_dir"], rm.Scene(*(x0[key] for key in SCENE)), x0["sh"], c["k"],
                                     c["steps"], return_t=True, **R.CONSTS)

    def call(x):
        scene = rm.Scene(*(x[key] for key in SCENE))
        g = rm.render_diff_sh_backward(x["ray_org"], x["ray_dir"], scene, x["sh"], c["k"], x["grad_out"], c["steps"],
                                       t_march=x["t"], **R.CONSTS)
        return [g[key] for key in SCENE + ("sh",)]
    _both_alignments(call, dict(s.arrays, grad_out=s.seeds[0], t=t.cpu().numpy()))


def test_low_level_sdf_backward_at_4_byte_alignment(rm):
    from test_gpu_sdf import CSHARP, K
    s = spec("sdf_field")

    def call(x):
        g = rm.sdf_query_backward(x["points"], x["centers"], x["colors"], x["radius"], K, color_sharpness=CSHARP,
                                  grad_dist=x["gD"], grad_color=x["gC"])
        return [g[key] for key in ("centers", "colors", "radius", "points")]
    _both_alignments(call, dict(s.arrays, gD=s.seeds[0], gC=s.seeds[1]))


def test_low_level_image_loss_at_4_byte_alignment(rm):
    s = spec("image_loss")

    def call(x):
        r = rm.image_loss_call(x["out"], x["target"], 40, 24, loss=True, view_stats=True, ssim_map=True, grad=True)
        return [r[key] for key in ("loss", "view_stats", "ssim_map", "grad")]
    _both_alignments(call, s.arrays)


def test_backward_camera_view_limit_names_its_constant(rm):
    """render_diff_backward_camera takes RM_MAX_VIEWS_PER_CALL views a call and says so (the autograd Function
    splits longer lists itself); refused before anything is read."""
    from burn_raymarching_amd import native
    cams = [([0.0, 0.0, -2.5], [0.0, 0.0, 0.0], 50.0)] * (native.RM_MAX_VIEWS_PER_CALL + 1)
    with pytest.raises(ValueError, match=rf"RM_MAX_VIEWS_PER_CALL = {native.RM_MAX_VIEWS_PER_CALL}\b"):
        rm.render_diff_backward_camera(cams, 2, 2, None, 32.0, None)
