"""One rm_context across calls of different sizes: its device buffers (the workspace, the record
buffer, the split continuation's state, the ray-gradient workspace, the drawn batch) grow when a
later call needs more, and nothing of an earlier call may leak into a later one. Each test runs a
small call, a large call and the small call again on one context and compares every result bit for
bit with the same call on a fresh context; the last test pre-allocates with rm_reserve and then
captures the calls in a hipGraph, which tolerates no allocation.

A fresh context is the one of a new torch stream (render.context() keys on the stream)."""
import pytest

from conftest import gpu_available
from context_calls import Iteration, _run, _same, fresh_context, raygrad_call, strided_rays, weights

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]


@pytest.fixture(scope="module")
def rm():
    import torch
    from burn_raymarching_amd import _build
    _build.build_lib()
    from burn_raymarching_amd import model, native, render
    torch.cuda.init()
    return torch, render, model, native


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


def test_raygrad_workspace_grows(rm):
    torch, render, model, native = rm
    check_reuse(torch, render, raygrad_call(torch, render, model, 256), raygrad_call(torch, render, model, 4096))


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
