"""One rm_context across calls of different sizes: its device buffers (the workspace, the record
buffer, the split continuation's state, the ray-gradient workspace, the drawn batch) grow when a
later call needs more, and nothing of an earlier call may leak into a later one. Each test runs a
small call, a large call and the small call again on one context and compares every result bit for
bit with the same call on a fresh context; the last test pre-allocates with rm_reserve and then
captures the calls in a hipGraph, which tolerates no allocation.

A fresh context is the one of a new torch stream (render.context() keys on the stream)."""
import contextlib
import ctypes

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]


@pytest.fixture(scope="module")
def rm():
    import torch
    from burn_raymarching_amd import _build
    _build.build_lib()
    from burn_raymarching_amd import model, native, render
    torch.cuda.init()
    return torch, render, model, native


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


def check_reuse(torch, render, small, large):
    """small, large, small on one context, each against the same call on a fresh context."""
    ref = {}
    for name, call in (("small", small), ("large", large)):
        with fresh_context(torch, render):
            ref[name] = _run(call)
    with fresh_context(torch, render):
        got = [(name, _run(call)) for name, call in (("small", small), ("large", large), ("small", small))]
    for i, (name, res) in enumerate(got):
        _same(res, ref[name], f"call {i} ({name})")
    for res in ref.values():  # the calls did something
        assert all(torch.isfinite(t).all() for t in res) and any(t.abs().max() > 0 for t in res)
    return ref


def strided_rays(render, model, n, size=72):
    """n rays spread over one size x size view of the ring."""
    o, d = render.create_camera_rays(size, size, *model.ring_cameras(3)[1])
    step = (size * size) // n
    return o[::step][:n].contiguous(), d[::step][:n].contiguous()


def weights(torch, n, seed):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3)).astype(np.float32)).cuda()


def test_workspace_and_records_grow(rm):
    """rm_render_diff_backward over ray arrays: 300 rays / 40 spheres (256-ray blocks), then 5,000
    rays / 300 spheres (the automatic split march: 157 blocks of 32 rays, a larger workspace and
    record buffer), then the first call again."""
    torch, render, model, native = rm

    def bwd(n, m):
        sc = model.scene_tensors(model.synthetic_scene(m, 3))
        o, d = strided_rays(render, model, n)
        go = weights(torch, n, n)
        return lambda: list(render.render_diff_backward(o, d, sc, 32.0, go, 8).values())
    check_reuse(torch, render, bwd(300, 40), bwd(5000, 300))


def test_continuation_buffer_grows(rm):
    """rm_train_step_camera of 256 spheres and 64 march steps -- the split march with a
    continuation at step 32 -- over 2 views of 32x32, then 4 views of 48x48, then the first again."""
    torch, render, model, native = rm
    m, steps = 256, 64
    sc = model.scene_tensors(model.synthetic_scene(m, 0))
    target = model.scene_tensors(model.synthetic_scene(m, 1))

    def train(views, w):
        cams = model.ring_cameras(views)
        tg = render.render_diff_camera(cams, w, w, target, 32.0, steps).view(-1, 3).contiguous()

        def call():
            buf = torch.zeros(model.packed_size(m) + 1, device="cuda")
            render.train_step_camera(cams, w, w, tg, sc, 32.0, 0.25, steps, grads_packed=buf[:-1], loss=buf[-1:])
            return [buf]
        return call
    check_reuse(torch, render, train(2, 32), train(4, 48))


def raygrad_call(torch, render, model, n):
    """rm_render_diff_backward_rays without a saved t (the forward replays the march into the
    ray-gradient workspace), 12 spheres."""
    sc = model.scene_tensors(model.synthetic_scene(12, 5, radius_range=(0.08, 0.3)))
    o, d = strided_rays(render, model, n)
    go = weights(torch, n, 7 + n)
    return lambda: list(render.render_diff_backward_rays(o, d, sc, 32.0, go, 16))


def test_raygrad_workspace_grows(rm):
    torch, render, model, native = rm
    check_reuse(torch, render, raygrad_call(torch, render, model, 256), raygrad_call(torch, render, model, 4096))


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


def test_batch_buffer_grows(rm, monkeypatch):
    """rm_train_iteration as its three separate steps (RM_FUSED_ITER=0: the batch is drawn into the
    context's buffer): 512 rays drawn, then 4,096, then 512 again."""
    torch, render, model, native = rm
    monkeypatch.setenv("RM_FUSED_ITER", "0")
    check_reuse(torch, render, Iteration(torch, render, model, native, 512), Iteration(torch, render, model, native, 4096))


def test_reserve_then_capture(rm, monkeypatch):
    """After rm_reserve(4096 rays, 64 spheres) nothing grows: the 4,096-ray ray-gradient call and
    the 4,096-ray unfused iteration give the un-reserved results, and after one eager run each is
    captured in a hipGraph (no allocation may happen there) and replays to the same bits."""
    torch, render, model, native = rm
    monkeypatch.setenv("RM_FUSED_ITER", "0")
    calls = {"raygrad": raygrad_call(torch, render, model, 4096),
             "iteration": Iteration(torch, render, model, native, 4096)}
    ref = {}
    for name, call in calls.items():
        with fresh_context(torch, render):
            ref[name] = _run(call)
    with fresh_context(torch, render) as (s, ctx):
        ctx.check(ctx._lib.rm_reserve(ctx.handle, 4096, 64), "rm_reserve")
        for name, call in calls.items():
            _same(_run(call), ref[name], f"{name} after rm_reserve")  # the eager warm-up
        torch.cuda.synchronize()
        for name, call in calls.items():
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                out = call()
            g.replay()
            torch.cuda.synchronize()
            _same([t.clone() for t in out], ref[name], f"{name} replayed")
