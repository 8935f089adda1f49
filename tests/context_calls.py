"""Calls of every family of entry points on one rm_context: TEST INFRASTRUCTURE ONLY (plain helpers, imported
by tests/test_gpu_context_reuse.py and tests/test_gpu_context_families.py).

A node is a zero-argument closure over inputs made once; it returns the list of its call's output tensors. A
node resets its own mutable inputs (raw parameters, moments, gradient buffers) before each call, sets the
environment switches its path needs around its own call (the library reads them once per call) and restores
them. The project's contract is that a call's outputs are a function of its arguments alone, so a node's
outputs on a context other calls have used equal, bit for bit, its outputs on a context nobody has used.

Shapes are the smallest that take the named path, taken where possible from the cases the family's own parity
file pins against its fp64 restatement or the oracle; a node of another shape carries a `restate` check of its
fresh-context outputs against that restatement under that file's own bounds. `evidence` asserts from the
library's diagnostics that the node ran the path it is named for."""
import contextlib
import ctypes
import os

import numpy as np

K = 32.0
LAST = 15  # the last cost class (kOrderClasses - 1)
FWD_MAX, FWD_MEAN = 1e-3, 1e-5  # the forward bound against fp64 (tests/test_gpu_parity.py's)


@contextlib.contextmanager
def fresh_context(torch, render):
    """Run under a new stream whose rm_context no call has used. torch hands its streams out of a
    pool, so a context an earlier test left under the same stream handle is dropped first."""
    s = torch.cuda.Stream()
    key = (torch.cuda.current_device(), s.cuda_stream)
    render._ctx_cache.pop(key, None)
    torch.cuda.synchronize()  # the inputs were made on another stream
    try:
        with torch.cuda.stream(s):
            yield s, render.context()
            torch.cuda.synchronize()
    finally:
        render._ctx_cache.pop(key, None)  # rm_destroy


def _run(call):
    return [t.clone() for t in call()]


def _same(got, ref, what):
    """Bit for bit (float32 tensors, compared as their words)."""
    import torch
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert torch.equal(g.view(torch.int32), r.view(torch.int32)), (what, i)


def strided_rays(render, model, n, size=72):
    """n rays spread over one size x size view of the ring."""
    o, d = render.create_camera_rays(size, size, *model.ring_cameras(3)[1])
    step = (size * size) // n
    return o[::step][:n].contiguous(), d[::step][:n].contiguous()


def weights(torch, n, seed):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3)).astype(np.float32)).cuda()


@contextlib.contextmanager
def switches(env):
    """The environment switches of one call, restored afterwards."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def words_equal(got, ref):
    """A device bool: every output of `got` has the words of `ref` (no synchronisation)."""
    import torch
    assert len(got) == len(ref)
    ok = [(g.view(torch.int32) == r.view(torch.int32)).all() for g, r in zip(got, ref)]
    return torch.stack(ok).all()


def dev(x, dtype=np.float32):
    import torch
    return torch.from_numpy(np.array(x, dtype)).cuda()  # a copy: the cases' arrays are read-only


def host(t):
    return t.detach().float().cpu().numpy()


class Node:
    """name; call() -> [tensors]; evidence(info): asserts the path from the diagnostics of one run on a fresh
    context (info: stats, order counts and next set, the last class's lists, the tile-proof bytes, the outputs);
    restate(ref): the fresh-context outputs against the family's restatement, for a shape no parity file pins."""

    def __init__(self, name, call, evidence=None, restate=None):
        self.name, self.call, self.evidence, self.restate = name, call, evidence, restate

    def __call__(self):
        return self.call()

    def __repr__(self):
        return self.name


def oracle():
    from oracle import oracle as orc
    orc.build()
    return orc


# ---- the per-ray families -----------------------------------------------------------------------------------

def per_ray(blocks=None, waves=None, seeded=True):
    """Evidence of a per-ray launch: blocks, waves and (for a backward or train call of the general kernel)
    seeded rays are positive; `blocks` / `waves` pin the launch's size, hence its kernel and rays per block."""
    def check(info):
        st = info["stats"]
        assert st["blocks"] > 0 and st["waves"] > 0, st
        if blocks is not None:
            assert st["blocks"] == blocks, (st, blocks)
        if waves is not None:
            assert st["waves"] == waves, (st, waves)
        if seeded:
            assert st["seeded_rays"] > 0, st
    return check


def bwd_node(torch, render, model, name, n, m, seed, blocks, waves):
    """rm_render_diff_backward over ray arrays at tests/test_gpu_context_reuse.py's sizes. The upstream gradient
    is one-signed and the scene seed chosen so that the fp64 oracle can be the yardstick: with signed weights
    light_dir's gradient cancels across the rays, and the oracle's own fp32 run misses conftest.check_grads'
    bound on it at most seeds of the 5,000-ray shape (3.6 bounds at seed 3); as built, the fp32 oracle sits at
    0.24 (300 rays) and 0.07 (5,000 rays) of the bounds."""
    sc_np = model.synthetic_scene(m, seed)
    sc = model.scene_tensors(sc_np)
    o, d = strided_rays(render, model, n)
    go = weights(torch, n, n).abs()

    def restate(ref):
        from conftest import check_grads
        g_ref = oracle().render_diff_backward(host(o).astype(np.float64), host(d).astype(np.float64), sc_np, 8, K,
                                              host(go).astype(np.float64))
        check_grads(dict(zip(("centers", "colors", "radius", "light_dir", "ambient"), ref)), g_ref, mode="bwd")
    return Node(name, lambda: list(render.render_diff_backward(o, d, sc, K, go, 8).values()),
                per_ray(blocks, waves), restate)


def multi_tile_node(torch, render, model):
    """tests/test_gpu_parity.py::test_multi_tile_spheres' backward: 1,100 spheres (three blocks of the record
    kernel, the per-sweep restaging), the 256 rays of a 16x16 view, 8 steps: eight 32-ray groups of the split march."""
    orc = oracle()
    sc = model.scene_tensors(model.synthetic_scene(1100, 21, radius_range=(0.01, 0.04)))
    o, d = orc.camera_rays(16, 16, *model.ring_cameras(7)[1], precision="f32")
    o, d = dev(o), dev(d)
    g = dev(np.random.default_rng(0).normal(size=(256, 3)))
    return Node("a_m1100", lambda: list(render.render_diff_backward(o, d, sc, K, g, 8).values()), per_ray(8, 8))


def tilted(cams, y):
    """The cameras looking at (0, y, 0): the scene sits below the image centre."""
    return [(eye, [0.0, y, 0.0], fov) for eye, _, fov in cams]


class TrainCamera:
    """rm_train_step_camera of `m` spheres over `cams` at w x h into a packed gradient + loss buffer the node
    zeroes before each call. The target is the render of another seed's scene."""

    def __init__(self, torch, render, model, m, cams, w, h, steps, *, seed=11, half=False, progress=0.25,
                 radius_range=(0.03, 0.12), env=None):
        self.torch, self.render, self.model = torch, render, model
        self.m, self.cams, self.w, self.h, self.steps, self.progress = m, list(cams), w, h, steps, progress
        self.env = dict(env or {})
        self.sc_np = model.synthetic_scene(m, seed, radius_range=radius_range)
        if half:
            self.sc_np["colors"] = self.sc_np["colors"].astype(np.float16).astype(np.float32)
        sc = model.scene_tensors(self.sc_np)
        self.sc = render.Scene(sc.centers, sc.colors.half() if half else sc.colors, sc.radius, sc.light_dir, sc.ambient)
        tsc = model.scene_tensors(model.synthetic_scene(m, seed + 1, radius_range=radius_range))
        self.tg = render.render_diff_camera(self.cams, w, h, tsc, K, steps).view(-1, 3).contiguous()
        self.buf = torch.zeros(model.packed_size(m) + 1, device="cuda")

    def __call__(self):
        self.buf.zero_()
        with switches(self.env):
            self.render.train_step_camera(self.cams, self.w, self.h, self.tg, self.sc, K, self.progress, self.steps,
                                          grads_packed=self.buf[:-1], loss=self.buf[-1:])
        return [self.buf]

    def restate(self, ref):
        """The fresh-context gradient and loss against the fp64 oracle on the same rays, as the train step's
        definition: forward, compute_loss's L1 seed (training.rs:17-34), backward. The seed's signs are taken from
        the kernel's own `out` -- held to the oracle's render under tests/test_gpu_parity.py's forward bound -- and
        the gradient is held to the oracle's backward of that seed under conftest.check_grads' backward bounds; in
        fp64 this composition is the oracle's train step to 1e-15. The oracle's own fp32 train step, with its own
        signs, misses check_grads' train-step bounds by factors of 10 to 700 at one seed in eight of these shapes
        (sign(out - target) flips on a pixel that matters), so its fp64 train step cannot be the yardstick here;
        with the signs shared, the fp32 oracle sits at 0.16 to 0.37 of the backward bounds at the seeds used."""
        orc = oracle()
        rays = [orc.camera_rays(self.w, self.h, *c, precision="f32") for c in self.cams]
        o = np.concatenate([r[0] for r in rays]).astype(np.float64)
        d = np.concatenate([r[1] for r in rays]).astype(np.float64)
        out_t = self.torch.full_like(self.tg, float("nan"))
        buf = self.torch.zeros_like(self.buf)
        with switches(self.env):  # the same call once more, with its image
            self.render.train_step_camera(self.cams, self.w, self.h, self.tg, self.sc, K, self.progress, self.steps,
                                          grads_packed=buf[:-1], loss=buf[-1:], out=out_t)
        assert self.torch.equal(buf.view(self.torch.int32), ref[0].view(self.torch.int32))
        got = host(ref[0])
        shared_sign_check(f"M={self.m} {len(self.cams)}x{self.w}x{self.h}", o, d, host(self.tg), self.sc_np, self.steps, K,
                          self.progress, host(out_t), self.model.unpack(got[:-1], self.m), got[-1])


def shared_sign_check(tag, o, d, tg, sc_np, steps, k, progress, out, grads, loss):
    """A train step's image, loss and gradient against the fp64 oracle: `out` under the forward bound, the loss
    against sum W |out - tg|, the gradient against the oracle's backward of the L1 seed W sign(out - tg) / (3 N)
    formed from this `out`, under conftest.check_grads' backward bounds (TrainCamera.restate says why)."""
    from conftest import check_grads
    orc = oracle()
    o, d, tg, out = (np.asarray(x, np.float64) for x in (o, d, tg, out))
    e = np.abs(out - orc.render_diff(o, d, sc_np, steps, k, precision="f64"))
    weight = np.where(tg.sum(1, keepdims=True) > 0.01, 10.0, 1.0 + 4.0 * progress)
    g_ref = orc.render_diff_backward(o, d, sc_np, steps, k, weight * np.sign(out - tg) / (3.0 * o.shape[0]))
    loss_ref = float((weight * np.abs(out - tg)).sum())
    print(f"train-step node {tag}: out max {e.max():.3e} mean {e.mean():.3e}, loss {loss:.6e} oracle {loss_ref:.6e}")
    assert e.max() <= FWD_MAX and e.mean() <= FWD_MEAN, (e.max(), e.mean())
    assert abs(loss - loss_ref) <= 1e-4 * abs(loss_ref) + 1e-3, (loss, loss_ref)
    check_grads(grads, g_ref, mode="bwd")


def cost_ordered(blocks, shards=False, tile_proof=False):
    """Evidence of a keyed (cost-ordered) launch: it appended its `blocks` blocks to the lists of its set;
    shards: the last class is not empty and went to its own lists; tile_proof: the pre-pass judged its waves."""
    base = per_ray(blocks, 4 * blocks)

    def check(info):
        base(info)
        counts, nxt = info["order"]
        mine = counts[(nxt + 2) % 3]
        assert sum(mine) == blocks, (counts, nxt)
        lists = info["shards"][(nxt + 2) % 3]
        assert sum(lists) == mine[LAST], (lists, mine)
        if shards:  # two last-class blocks or more: their launch positions differ, and so do their lists
            assert mine[LAST] >= 2 and sum(1 for n in lists if n) >= 2, (lists, mine)
        else:
            assert lists[1:] == [0] * (len(lists) - 1), lists
        assert (len(info["tile_proof"]) > 0) == tile_proof, len(info["tile_proof"])
    return check


def not_ordered(blocks, waves):
    base = per_ray(blocks, waves)

    def check(info):
        base(info)
        assert sum(sum(c) for c in info["order"][0]) == 0, info["order"]  # no keyed launch on this context
    return check


def train_nodes(torch, render, model):
    ring2 = model.ring_cameras(2)
    wide = [(eye, tgt, 90.0) for eye, tgt, _ in tilted(ring2, 1.2)]  # the scene inside the two lower tiles
    nodes = []
    # b. the small-scene kernel: 9 spheres, two lanes per ray (128 rays a block)
    b = TrainCamera(torch, render, model, 9, ring2, 32, 32, 24, seed=49, radius_range=(0.08, 0.3))
    nodes.append(Node("b_small_m9", b, per_ray(16, 64, seeded=False), b.restate))
    # c. the general kernel with the soft-ball proof: 16x16 tiles (block order, cost order) and rows
    c = TrainCamera(torch, render, model, 128, wide, 32, 32, 32)
    nodes.append(Node("c_m128_tiled", c, cost_ordered(8), c.restate))
    cr = TrainCamera(torch, render, model, 128, ring2, 24, 40, 32, seed=12)
    nodes.append(Node("c_m128_rows", cr, not_ordered(8, 32), cr.restate))
    # d. c with the lattice, the tile proof and the sharded last class forced
    d = TrainCamera(torch, render, model, 128, wide, 32, 32, 32, env={"RM_PROOF_LATTICE": "1", "RM_ORDER_SHARDS": "1"})
    nodes.append(Node("d_m128_lattice_shards", d, cost_ordered(8, shards=True, tile_proof=True), d.restate))
    # e. the split march with a continuation at step 32 (tests/test_gpu_context_reuse.py's shape): 32-ray groups
    e = TrainCamera(torch, render, model, 256, ring2, 32, 32, 64, seed=0)
    nodes.append(Node("e_m256_split_cont", e, per_ray(64, 64), e.restate))
    # f. more than 16 views: the context's device camera table, then 17 other views
    f1 = TrainCamera(torch, render, model, 48, model.ring_cameras(17), 16, 16, 16, seed=4)
    nodes.append(Node("f_17_views", f1, per_ray(17, 68), f1.restate))
    f2 = TrainCamera(torch, render, model, 48, model.ring_cameras(17, radius=2.2, height=0.8, offset=3), 16, 16, 16, seed=4)
    nodes.append(Node("f_17_other_views", f2, per_ray(17, 68), f2.restate))
    # n. c on an fp16-colour scene
    n = TrainCamera(torch, render, model, 128, wide, 32, 32, 32, half=True)
    nodes.append(Node("n_m128_f16_colours", n, cost_ordered(8), n.restate))
    return nodes


# ---- ray and pose gradients (tests/test_gpu_raygrad.py's cases) ----------------------------------------------

def raygrad_call(torch, render, model, n):
    """rm_render_diff_backward_rays without a saved t (the forward replays the march into the
    ray-gradient workspace), 12 spheres."""
    sc = model.scene_tensors(model.synthetic_scene(12, 5, radius_range=(0.08, 0.3)))
    o, d = strided_rays(render, model, n)
    go = weights(torch, n, 7 + n)
    return lambda: list(render.render_diff_backward_rays(o, d, sc, K, go, 16))


def raygrad_nodes(torch, render, model):
    import test_gpu_raygrad as T
    orc = oracle()

    def inputs(name):
        make, k, steps, w, h, cams = T.CASES[name]
        rays = [orc.camera_rays(w, h, *T.cam(i), precision="f32") for i in cams]
        o, d = np.concatenate([r[0] for r in rays]), np.concatenate([r[1] for r in rays])
        if name in ("C8", "C10"):
            o, d = np.concatenate([o, o[100:101]]), np.concatenate([d, d[100:101]])
        gout = np.random.default_rng(sum(map(ord, name))).standard_normal(o.shape).astype(np.float32)
        return T.scene_dev(render, make()), k, steps, w, h, [T.cam(i) for i in cams], dev(o), dev(d), dev(gout)

    nodes = []
    for name in ("C3", "C10"):  # 64 spheres and 576 rays; 520 spheres (two record blocks) and 257 rays
        sc, k, steps, w, h, cams, o, d, g = inputs(name)
        nodes.append(Node(f"g_rays_{name}", lambda o=o, d=d, sc=sc, k=k, g=g, steps=steps:
                          list(render.render_diff_backward_rays(o, d, sc, k, g, steps)), per_ray(seeded=False)))
    for name in ("C9", "C7"):  # three views of 6 spheres; one view of 300 spheres
        sc, k, steps, w, h, cams, o, d, g = inputs(name)
        g = g[:len(cams) * w * h].contiguous()
        nodes.append(Node(f"g_cameras_{name}", lambda cams=cams, w=w, h=h, sc=sc, k=k, g=g, steps=steps:
                          [render.render_diff_backward_cameras(cams, w, h, sc, k, g, steps)], per_ray(seeded=False)))
    return nodes


# ---- SH colour (tests/sh_ref.py's cases) --------------------------------------------------------------------

SH_KEYS = ("centers", "colors", "radius", "light_dir", "ambient", "sh")


def sh_nodes(torch, render, model):
    import sh_ref as R
    nodes = []
    for name in ("m33_d2", "m300_d1"):
        c = R.case(name)
        s = c["scene"]
        sc = render.Scene(dev(s["centers"]), dev(s["colors"]), dev(s["radius"]), dev(s["light_dir"]), dev(s["ambient"]))
        sh, g = dev(c["sh"]), dev(c["grad_out"])

        def call(sc=sc, sh=sh, g=g, c=c):
            out = render.render_diff_sh_backward_camera([R.CAMERA], R.WIDTH, R.WIDTH, sc, sh, c["k"], g, c["steps"],
                                                        want=SH_KEYS, **R.CONSTS)
            return [out[k] for k in SH_KEYS]

        def restate(ref, c=c, name=name):
            """The camera form's gradients against fp64 autograd of the restatement on the same rays, under the
            case's own bounds (tests/test_gpu_sh.py::test_camera_mode does the same for m48_d1)."""
            bound, r64 = R.bounds(c), R.reference(c)
            for q, t in zip(SH_KEYS, ref):
                e = R.max_err(host(t), r64[q])
                print(f"sh node {name} {q}: gpu {e:.3e} bound {bound[q]:.3e}")
                assert e <= bound[q], (name, q, e, bound[q])
        nodes.append(Node(f"h_sh_backward_camera_{name}", call, per_ray(seeded=False), restate))
    c = R.case("m33_d2")
    s = c["scene"]
    sc = render.Scene(dev(s["centers"]), dev(s["colors"]), dev(s["radius"]), dev(s["light_dir"]), dev(s["ambient"]))
    o, d, sh = dev(c["org"]), dev(c["dir"]), dev(c["sh"])
    nodes.append(Node("h_sh_forward_m33_d2", lambda: list(render.render_diff_sh_forward(
        o, d, sc, sh, c["k"], c["steps"], return_t=True, **R.CONSTS)), per_ray(3, 12, seeded=False)))
    return nodes


# ---- the distance field (tests/test_gpu_sdf.py's pool, tests/sdf_grad_ref.py's seeds) -------------------------

def sdf_nodes(torch, render, model):
    import sdf_grad_ref as G
    import sdf_ref as S
    import test_gpu_sdf as T
    n = 257
    lattice = ((-0.8, -0.4, -0.2), 0.1, (17, 9, 5))
    nodes = []

    def calls(sc_np, pts_np, gD_np, gC_np):
        sc = T.scene_t(sc_np)
        pts, gD, gC = dev(pts_np), dev(gD_np), dev(gC_np)
        query = lambda: list(render.sdf_query(pts, sc, T.K, color_sharpness=T.CSHARP))  # noqa: E731
        back = lambda: list(render.sdf_query_backward(pts, sc.centers, sc.colors, sc.radius, T.K,  # noqa: E731
                                                      color_sharpness=T.CSHARP, grad_dist=gD, grad_color=gC).values())
        grid = lambda: list(render.sdf_grid(*lattice, sc, T.K, color_sharpness=T.CSHARP, color=True))  # noqa: E731
        return sc, query, back, grid

    # 300 spheres: the pool's first 257 points and the "both" seeds, and test_grid_equals_query_bit_for_bit's lattice
    sc_np, pool, _, _, _ = T.pool("m300")
    gD, gC = G.seed_sets(len(pool))["both"]
    _, query, back, grid = calls(sc_np, pool[:n], gD[:n], gC[:n])
    nodes += [Node("i_sdf_query_m300", query), Node("i_sdf_backward_m300", back), Node("i_sdf_grid_m300", grid)]

    # 9 spheres: no parity file has them; one node of the three calls, each held to its restatement
    sc9 = model.synthetic_scene(9, 3, radius_range=(0.08, 0.3))
    pts9 = np.random.default_rng(9).uniform(-1, 1, (n, 3)).astype(np.float32)
    gD9, gC9 = G.seed_sets(n)["both"]
    sct9, query9, back9, grid9 = calls(sc9, pts9, gD9, gC9)

    def restate(ref):
        """sdf_query against the fp64 field and sdf_query_backward against its fp64 autograd, under 8 times the
        restatement's own fp32 error over these points (the two files' convention); sdf_grid against sdf_query
        at the lattice's points, bit for bit."""
        r64, r32 = S.field(pts9, sc9, T.K, T.CSHARP, torch.float64), S.field(pts9, sc9, T.K, T.CSHARP, torch.float32)
        for what, t, a, b in zip(("dist", "grad", "color"), ref[:3], r64, r32):
            e, bound = G.max_err(host(t), a), 8.0 * G.max_err(b, a)
            print(f"sdf node m9 {what}: gpu {e:.3e} bound {bound:.3e}")
            assert e <= bound, (what, e, bound)
        far = np.zeros(n, bool)
        bound, g64 = G.bounds(pts9, far, sc9, T.K, T.CSHARP, gD9, gC9)
        got = dict(zip(("centers", "colors", "radius", "points"), (host(t) for t in ref[3:7])))
        for q, e in G.errors(got, g64, far).items():
            print(f"sdf node m9 backward {q}: gpu {e:.3e} bound {bound[q]:.3e}")
            assert e <= bound[q], (q, e, bound[q])
        pts = torch.from_numpy(S.lattice(*lattice).reshape(-1, 3)).cuda()
        qd, qc = render.sdf_query(pts, sct9, T.K, color_sharpness=T.CSHARP, grad=False)
        assert torch.equal(ref[7].reshape(-1), qd) and torch.equal(ref[8].reshape(-1, 3), qc)
    nodes.append(Node("i_sdf_all_m9", lambda: query9() + back9() + grid9(), restate=restate))
    return nodes


# ---- the viewer, the image loss --------------------------------------------------------------------------------

def view_nodes(torch, render, model):
    import test_gpu_view as T
    nodes = []
    for case in ("synth_M520_32x24", "one_sphere_40x24"):
        _, scene, w, h, poses = next(c for c in T.CASES if c[0] == case)
        sc, cams = T.scene_t(scene), T.cams_of(poses)
        nodes.append(Node(f"j_view_{case}", lambda cams=cams, w=w, h=h, sc=sc:
                          list(render.view(cams, w, h, sc, rgba8=True, depth=True))))
    return nodes


def loss_nodes(torch, render, model):
    import ssim_ref as R
    nodes = []
    for case in ((2, 33, 17), (1, 48, 40)):
        x, y = (dev(a) for a in R.images(*case))
        _, h, w = case
        nodes.append(Node("k_image_loss_%dx%dx%d" % case, lambda x=x, y=y, w=w, h=h: list(render.image_loss_call(
            x, y, w, h, loss=True, view_stats=True, ssim_map=True, grad=True).values())))
    return nodes


# ---- the sampled iteration and the fused-Adam step -------------------------------------------------------------

class Iteration:
    """One rm_train_iteration (step 1, penalties on) of a 9-sphere model on a batch of n rays drawn
    from two 64x64 views; every call starts from the same state, in buffers it keeps."""

    def __init__(self, torch, render, model, native, n, m=9):
        self.torch, self.render, self.native, self.m = torch, render, native, m
        cams = model.ring_cameras(2)
        rays = [render.create_camera_rays(64, 64, *c) for c in cams]
        self.o = torch.cat([r[0] for r in rays]).contiguous()
        self.d = torch.cat([r[1] for r in rays]).contiguous()
        tsc = model.scene_tensors(model.synthetic_scene(6, 2, radius_range=(0.08, 0.3)))
        self.t = render.render_diff_forward(self.o, self.d, tsc, 32.0, 24).contiguous()
        self.fg = torch.nonzero(self.t.sum(1) > 0.01).flatten().to(torch.int32).contiguous()
        assert self.fg.numel() > 0
        self.nf = n // 5
        self.nu = n - self.nf
        sc = model.synthetic_scene(m, 49, radius_range=(0.08, 0.3))
        sm = model.SceneModel.from_activated(sc["centers"], sc["colors"], sc["radius"], sc["light_dir"], sc["ambient"])
        self.init = (sm.raw.clone(), sm.activated_packed().clone())
        npk = model.packed_size(m)
        self.raw, self.act = self.init[0].clone(), self.init[1].clone()
        self.rest = [torch.zeros(npk, device="cuda") for _ in range(3)] + [torch.zeros(2, device="cuda")]
        torch.cuda.synchronize()

    def __call__(self):
        self.raw.copy_(self.init[0])
        self.act.copy_(self.init[1])
        for t in self.rest:
            t.zero_()
        grad, m1, m2, loss = self.rest
        ctx = self.render.context()
        p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
        n = self.nu + self.nf
        march = self.native.march_params(40, 16.0)
        ctx.check(ctx._lib.rm_train_iteration(ctx.handle, p(self.o), p(self.d), p(self.t), self.o.shape[0], p(self.fg),
                                              self.fg.numel(), self.nu, self.nf, 11, 1, 1, 0.5, 1.0 / (3 * n),
                                              ctypes.byref(march), p(self.act), p(grad), p(self.raw), p(m1), p(m2),
                                              self.m, 1, 0.01, 1e-5, 1, p(loss), ctypes.c_void_p(loss.data_ptr() + 4)),
                  "rm_train_iteration")
        return [self.raw, self.act, grad, m1, m2, loss]


def iteration_nodes(torch, render, model, native):
    def node(name, n, fused, blocks):
        it = Iteration(torch, render, model, native, n)

        def call():
            with switches({"RM_FUSED_ITER": "1" if fused else "0"}):
                return it()

        def evidence(info):
            per_ray(blocks, 4 * blocks, seeded=False)(info)
            assert not info["torch"].equal(info["ref"][0], it.init[0])  # the optimizer moved the parameters
        def restate(ref):
            """rm_train_iteration is rm_sample_batch -> rm_train_step -> rm_optimizer_step (train.rs:169-198;
            tests/test_gpu_small.py pins the equality at other ray counts): the three calls made here give the
            node's bits, the train step on the drawn batch meets the fp64 oracle (shared_sign_check), and
            rm_optimizer_step at 9 spheres is what tests/test_gpu_optimizer.py holds to its fp64 reference."""
            p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
            ctx = render.context()
            nb = it.nu + it.nf
            b = [torch.empty((nb, 3), device="cuda") for _ in range(3)]
            ctx.check(ctx._lib.rm_sample_batch(ctx.handle, p(it.o), p(it.d), p(it.t), it.o.shape[0], p(it.fg), it.fg.numel(),
                                               it.nu, it.nf, 11, 1, 1, p(b[0]), p(b[1]), p(b[2]), None), "rm_sample_batch")
            act0 = model.unpack(it.init[1], it.m)
            sc = render.Scene(*(act0[k].clone() for k in ("centers", "colors", "radius", "light_dir", "ambient")))
            with switches({"RM_FUSED_ITER": "0"}):
                loss, g, out = render.train_step(b[0], b[1], b[2], sc, 16.0, 0.5, 40, inv_count=1.0 / (3 * nb),
                                                 with_out=True)
            grad = torch.cat([g[k].reshape(-1) for k in ("centers", "colors", "radius", "light_dir", "ambient")])
            _same([grad, loss], [ref[2], ref[5][:1]], f"{name}: the train step on the drawn batch")
            raw, m1, m2, pen = it.init[0].clone(), torch.zeros_like(grad), torch.zeros_like(grad), torch.zeros(1, device="cuda")
            act = torch.empty_like(raw)
            ctx.check(ctx._lib.rm_optimizer_step(ctx.handle, p(raw), p(grad), p(m1), p(m2), it.m, 1, 0.01, 1e-5, 1, p(pen),
                                                 p(act)), "rm_optimizer_step")
            _same([raw, act, m1, m2, pen], [ref[0], ref[1], ref[3], ref[4], ref[5][1:]], f"{name}: the optimizer step")
            sc_np = {k: host(v) for k, v in act0.items()}
            shared_sign_check(name, host(b[0]), host(b[1]), host(b[2]), sc_np, 40, 16.0, 0.5, host(out),
                              {k: host(v) for k, v in g.items()}, float(loss.item()))
        return Node(name, call, evidence, restate)
    # two lanes per ray: 128 rays a block
    return [node("l_iteration_fused", 512, True, 4), node("l_iteration_three_calls", 512, False, 4),
            node("l_iteration_three_calls_4096", 4096, False, 32)]


def adam_node(torch, render, model):
    """rm_train_step_camera_adam at tests/test_gpu_fused_adam.py's scene and march (64 spheres, 64x64 views of the
    ring of ten, 32 steps, the first step's progress 0.3) on two views: the optimizer inside the gradient reduction."""
    m, w = 64, 64
    cams = model.ring_cameras(10)[:2]
    tg = render.render_diff_camera(cams, w, w, model.scene_tensors(model.synthetic_scene(m, 4)), K, 32)
    sc = model.synthetic_scene(m, 3)
    mdl = model.SceneModel.from_activated(sc["centers"], sc["colors"], sc["radius"], sc["light_dir"], sc["ambient"])
    opt = model.Adam(mdl, weight_decay=1e-5, with_penalties=True)
    raw0 = mdl.raw.clone()
    g, loss, pen = torch.zeros(model.packed_size(m), device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")

    def call():
        mdl.raw.copy_(raw0)
        mdl.invalidate()  # rm_scene_activate is part of the node
        for t in (opt.m, opt.v, g, loss, pen):
            t.zero_()
        opt.t = 0
        with switches({"RM_FUSED_ADAM": "1"}):
            opt.train_step_camera(cams, w, w, tg, K, 0.3, 0.02, 32, grads_packed=g, loss=loss, penalty_out=pen)
        return [mdl.raw, mdl._act, opt.m, opt.v, g, loss, pen]

    def evidence(info):
        cost_ordered(32)(info)
        # adam_done: the call made no optimizer launch of its own, and the parameters and moments moved
        assert not info["torch"].equal(info["ref"][0], raw0) and info["ref"][2].abs().max() > 0

    def restate(ref):
        """The fused call is rm_train_step_camera -> rm_optimizer_step (tests/test_gpu_fused_adam.py pins the
        equality on three views): the two calls made here give the node's bits, and their train step meets the
        fp64 oracle (shared_sign_check); rm_optimizer_step at 64 spheres is tests/test_gpu_optimizer.py's."""
        mdl.raw.copy_(raw0)
        mdl.invalidate()
        sc = mdl.scene()
        sc_np = {k: host(v) for k, v in model.unpack(mdl._act, m).items()}
        g2, l2, p2, out = torch.zeros_like(g), torch.zeros_like(loss), torch.zeros_like(pen), torch.full_like(tg, float("nan"))
        render.train_step_camera(cams, w, w, tg, sc, K, 0.3, 32, grads_packed=g2, loss=l2, out=out)
        _same([g2, l2], [ref[4], ref[5]], "m_fused_adam_m64: the train step alone")
        opt2 = model.Adam(mdl, weight_decay=1e-5, with_penalties=True)
        opt2.step(g2, 0.02, penalty_out=p2)
        _same([mdl.raw, mdl._act, opt2.m, opt2.v, p2], [ref[0], ref[1], ref[2], ref[3], ref[6]],
              "m_fused_adam_m64: the optimizer step alone")
        orc = oracle()
        rays = [orc.camera_rays(w, w, *c, precision="f32") for c in cams]
        shared_sign_check("m_fused_adam_m64", np.concatenate([r[0] for r in rays]), np.concatenate([r[1] for r in rays]),
                          host(tg), sc_np, 32, K, 0.3, host(out), model.unpack(host(g2), m), float(l2.item()))
    return Node("m_fused_adam_m64", call, evidence, restate)


_CATALOGUE = None


def catalogue(torch, render, model, native):
    """The nodes, in catalogue order; built once (on torch's default stream) and left unchanged."""
    global _CATALOGUE
    if _CATALOGUE is None:
        nodes = [bwd_node(torch, render, model, "a_bwd_300_rays_m40", 300, 40, 3, 2, 8),
                 # the automatic split march: 157 groups of 32 rays, one wave each
                 bwd_node(torch, render, model, "a_bwd_5000_rays_m300", 5000, 300, 10, 157, 157),
                 multi_tile_node(torch, render, model)]
        nodes += train_nodes(torch, render, model)
        nodes += raygrad_nodes(torch, render, model)
        nodes += sh_nodes(torch, render, model)
        nodes += sdf_nodes(torch, render, model)
        nodes += view_nodes(torch, render, model)
        nodes += loss_nodes(torch, render, model)
        nodes += iteration_nodes(torch, render, model, native)
        nodes.append(adam_node(torch, render, model))
        assert [n.name for n in nodes] == NAMES, [n.name for n in nodes]
        torch.cuda.synchronize()
        _CATALOGUE = nodes
    return _CATALOGUE


NAMES = ["a_bwd_300_rays_m40", "a_bwd_5000_rays_m300", "a_m1100", "b_small_m9", "c_m128_tiled", "c_m128_rows",
         "d_m128_lattice_shards", "e_m256_split_cont", "f_17_views", "f_17_other_views", "n_m128_f16_colours",
         "g_rays_C3", "g_rays_C10", "g_cameras_C9", "g_cameras_C7", "h_sh_backward_camera_m33_d2",
         "h_sh_backward_camera_m300_d1", "h_sh_forward_m33_d2", "i_sdf_query_m300", "i_sdf_backward_m300",
         "i_sdf_grid_m300", "i_sdf_all_m9", "j_view_synth_M520_32x24", "j_view_one_sphere_40x24",
         "k_image_loss_2x33x17", "k_image_loss_1x48x40", "l_iteration_fused", "l_iteration_three_calls",
         "l_iteration_three_calls_4096", "m_fused_adam_m64"]


def diagnostics(torch, render, node):
    """One run of the node on a fresh context with the work counters on: what `evidence` reads. Not
    bit-compared (the counters add stores to the kernels)."""
    with fresh_context(torch, render) as (_, ctx):
        ctx.stats(True)
        try:
            ref = _run(node)
            torch.cuda.synchronize()
            stats = ctx.collect_stats(reset=True)
        finally:
            ctx.stats(False)
        return {"torch": torch, "ref": ref, "stats": stats, "order": ctx.order_counts(),
                "shards": ctx.order_shard_counts(), "tile_proof": ctx.tile_proof()}


__all__ = ["fresh_context", "_run", "_same", "strided_rays", "weights", "Iteration", "raygrad_call", "catalogue",
           "NAMES", "Node", "diagnostics", "words_equal", "switches"]
