"""Torch-facing mirror of the reference's render interface, executed by the HIP kernels.

Names and argument meaning follow the reference:
  * ``render_diff(ray_org, ray_dir, centers, colors, radius, light_dir, ambient, smooth_k)``
    -- renderer_diff.rs:6-15, differentiable through ``torch.autograd`` (the gradient
    is the analytic burn-autodiff backward computed by rm_render_diff_backward);
  * ``render_diff_camera(cams, width, height, ...)`` -- the same with rays generated
    in-kernel as create_camera_rays (camera.rs:30-90) would;
  * ``render_diff_cameras(eye, target, fov_deg, width, height, ...)`` -- the same as an autograd
    function over the camera tensors too (pose refinement; rm_render_diff_backward_cameras), and
    ``render_diff_backward_rays`` / ``render_diff_backward_cameras`` -- the ray / pose gradients;
  * ``render_diff_sh(ray_org, ray_dir, centers, colors, sh, radius, ...)`` -- render_diff with a
    view-dependent colour per sphere, spherical harmonics of degree 1 or 2 over the base colour
    (rm_render_diff_sh / rm_render_diff_sh_backward; ``render_diff_sh_forward`` / ``_backward`` and
    their ``_camera`` forms are the calls themselves);
  * ``image_loss(out, target, width, height)`` -- weighted L1 + D-SSIM on whole rendered views as an
    autograd scalar over ``out``, and ``image_metrics`` -- PSNR / SSIM / L1 per view (rm_image_loss;
    ``image_loss_call`` is the call itself);
  * ``train_step(...)`` -- forward + compute_loss reconstruction seed + backward fused;
  * ``create_camera_rays(width, height, eye, target, fov_deg)`` -- host ray
    generation (camera.rs:30-90, a host loop in the reference too);
  * ``view(cams, width, height, scene)`` / ``view_camera(pos, yaw, pitch)`` -- the reference
    viewer's frames (viewer.rs + shader.wgsl), headless: rm_view, not differentiable;
  * ``sdf_query(points, scene)`` / ``sdf_grid(origin, spacing, shape, scene)`` -- the scene's
    distance field (scene.rs:60-79), its gradient and blended colour at points of the caller's
    choosing or on a lattice: rm_sdf_query / rm_sdf_grid;
  * ``sdf_field(points, centers, colors, radius)`` -- the field's distance and colour as an
    autograd function over the points and the scene (rm_sdf_query_backward; ``sdf_query_backward``
    is the call itself).

Tensors are torch CUDA (HIP) tensors, fp32, ``[N, 3]``; torch provides device memory
and the stream only. Shapes are checked on the host before any launch.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import native
from .native import RmGrads, RmScene

_ctx_cache: dict = {}


def context(device=None) -> native.Context:
    """Per-(device, stream) rm_context, bound to torch's current stream."""
    dev = torch.cuda.current_device() if device is None else (device.index if isinstance(device, torch.device)
                                                              else int(device))
    stream = torch.cuda.current_stream(dev).cuda_stream
    key = (dev, stream)
    ctx = _ctx_cache.get(key)
    if ctx is None:
        ctx = native.Context(dev, stream)
        _ctx_cache[key] = ctx
    return ctx


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _f32(t, shape, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor")
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device (HIP) tensor: the render path has no CPU implementation")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    t = t.contiguous()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


class Scene:
    """Activated scene parameters (scene.rs:41-45) as device tensors + the rm_scene view."""

    def __init__(self, centers, colors, radius, light_dir, ambient):
        m = centers.shape[0]
        self.centers = _f32(centers, (m, 3), "centers")
        # fp16 colour / fp32 SDF (BASELINE configs[4]): half colours select RM_MARCH_COLOR_F16
        self.color_f16 = isinstance(colors, torch.Tensor) and colors.dtype == torch.float16
        if self.color_f16:
            if not colors.is_cuda or tuple(colors.shape) != (m, 3):
                raise ValueError("fp16 colors must be a [M,3] device tensor")
            self.colors = colors.contiguous()
        else:
            self.colors = _f32(colors, (m, 3), "colors")
        self.radius = _f32(radius.reshape(-1), (m,), "radius")
        self.light_dir = _f32(light_dir.reshape(-1), (3,), "light_dir")
        self.ambient = _f32(ambient.reshape(-1), (1,), "ambient")
        self.num_spheres = m

    @property
    def march_flags(self) -> int:
        return native.RM_MARCH_COLOR_F16 if self.color_f16 else 0

    def march_for(self, march) -> native.RmMarch:
        """A copy of `march` whose RM_MARCH_COLOR_F16 bit matches this scene's colour dtype (the
        caller's struct is never modified: a march shared between an fp16-colour and an fp32
        scene must not carry the bit from one call into the next)."""
        m = native.RmMarch.from_buffer_copy(march)
        m.flags = (m.flags & ~native.RM_MARCH_COLOR_F16) | self.march_flags
        return m

    def c_struct(self) -> RmScene:
        return RmScene(self.centers.data_ptr(), self.colors.data_ptr(), self.radius.data_ptr(),
                       self.light_dir.data_ptr(), self.ambient.data_ptr(), self.num_spheres)


def _grads_like(scene: Scene):
    dev = scene.centers.device
    m = scene.num_spheres
    g = {"centers": torch.empty((m, 3), device=dev), "colors": torch.empty((m, 3), device=dev),
         "radius": torch.empty((m,), device=dev), "light_dir": torch.empty((3,), device=dev),
         "ambient": torch.empty((1,), device=dev)}
    cg = RmGrads(g["centers"].data_ptr(), g["colors"].data_ptr(), g["radius"].data_ptr(),
                 g["light_dir"].data_ptr(), g["ambient"].data_ptr())
    return g, cg


def render_diff_forward(ray_org, ray_dir, scene: Scene, smooth_k, steps=40, *, normal_eps=1e-4,
                        color_sharpness=10.0, mask_sharpness=15.0, return_t=False):
    n = ray_org.shape[0]
    ray_org = _f32(ray_org, (n, 3), "ray_org")
    ray_dir = _f32(ray_dir, (n, 3), "ray_dir")
    out = torch.empty((n, 3), device=ray_org.device)
    t = torch.empty((n,), device=ray_org.device) if return_t else None
    ctx = context(ray_org.device)
    march = native.march_params(steps, smooth_k, normal_eps, color_sharpness, mask_sharpness)
    march = scene.march_for(march)
    ctx.check(ctx._lib.rm_render_diff(ctx.handle, _ptr(ray_org), _ptr(ray_dir), n, ctypes.byref(scene.c_struct()),
                                      ctypes.byref(march), _ptr(out), _ptr(t)), "rm_render_diff")
    return (out, t) if return_t else out


def render_diff_backward(ray_org, ray_dir, scene: Scene, smooth_k, grad_out, steps=40, *, t_march=None,
                         normal_eps=1e-4, color_sharpness=10.0, mask_sharpness=15.0):
    """Gradients of sum(out * grad_out) w.r.t. the activated params (light_dir raw)."""
    n = ray_org.shape[0]
    ray_org = _f32(ray_org, (n, 3), "ray_org")
    ray_dir = _f32(ray_dir, (n, 3), "ray_dir")
    grad_out = _f32(grad_out, (n, 3), "grad_out")
    if t_march is not None:
        t_march = _f32(t_march, (n,), "t_march")
    g, cg = _grads_like(scene)
    ctx = context(ray_org.device)
    march = native.march_params(steps, smooth_k, normal_eps, color_sharpness, mask_sharpness)
    march = scene.march_for(march)
    ctx.check(ctx._lib.rm_render_diff_backward(ctx.handle, _ptr(ray_org), _ptr(ray_dir), n,
                                               ctypes.byref(scene.c_struct()), ctypes.byref(march), _ptr(grad_out),
                                               _ptr(t_march), ctypes.byref(cg), 0), "rm_render_diff_backward")
    return g


def render_diff_backward_rays(ray_org, ray_dir, scene: Scene, smooth_k, grad_out, steps=40, *, t_march=None,
                              want_org=True, want_dir=True, grad_org=None, grad_dir=None, accumulate=False,
                              normal_eps=1e-4, color_sharpness=10.0, mask_sharpness=15.0, flags=0):
    """(dL/d ray_org, dL/d ray_dir) of sum(out * grad_out), [N,3] each (None where not wanted).

    This is the gradient of the reference's graph (renderer_diff.rs:6-91) with respect to its
    first two arguments: the march distance t and the normal are detached there, so with
    p_a = o + d t, t_f = t + D(p_a), p_f = o + d t_f the result is g_o = g_p + g_pa and
    g_d = t_f g_p + t g_pa (g_p = dL/dp_f, g_pa = (g_p . d) grad D(p_a)). It is what burn-autodiff
    returns for these inputs, not the derivative of the image through the march. grad_org /
    grad_dir: existing [N,3] tensors to write (or, with accumulate, add) into."""
    n = ray_org.shape[0]
    ray_org = _f32(ray_org, (n, 3), "ray_org")
    ray_dir = _f32(ray_dir, (n, 3), "ray_dir")
    grad_out = _f32(grad_out, (n, 3), "grad_out")
    if t_march is not None:
        t_march = _f32(t_march, (n,), "t_march")
    for name, g in (("grad_org", grad_org), ("grad_dir", grad_dir)):
        if g is not None and (_f32(g, (n, 3), name).data_ptr() != g.data_ptr()):
            raise ValueError(f"{name} must be contiguous")
    if accumulate and ((want_org and grad_org is None) or (want_dir and grad_dir is None)):
        raise ValueError("accumulate needs the tensors to add into")
    go = (grad_org if grad_org is not None else torch.empty((n, 3), device=ray_org.device)) if want_org else None
    gd = (grad_dir if grad_dir is not None else torch.empty((n, 3), device=ray_org.device)) if want_dir else None
    ctx = context(ray_org.device)
    march = native.march_params(steps, smooth_k, normal_eps, color_sharpness, mask_sharpness, flags=flags)
    march = scene.march_for(march)
    ctx.check(ctx._lib.rm_render_diff_backward_rays(ctx.handle, _ptr(ray_org), _ptr(ray_dir), n,
                                                    ctypes.byref(scene.c_struct()), ctypes.byref(march),
                                                    _ptr(grad_out), _ptr(t_march), _ptr(go), _ptr(gd),
                                                    1 if accumulate else 0), "rm_render_diff_backward_rays")
    return go, gd


def render_diff_backward_cameras(cams, width, height, scene: Scene, smooth_k, grad_out, steps=40, *, t_march=None,
                                 grad_cams=None, accumulate=False, normal_eps=1e-4, color_sharpness=10.0,
                                 mask_sharpness=15.0, flags=0):
    """dL/d(eye, target, fov_deg) per view of sum(out * grad_out): a [V,7] tensor laid out as
    rm_camera (eye 0:3, target 3:6, fov_deg 6). Any number of views (chunks of 128 per call).

    The ray gradients of render_diff_backward_rays chained through create_camera_rays
    (camera.rs:41-79): the reference graph's gradient (march detached, normal detached), not the
    derivative of the image. It follows finite differences of the image for a rigid shift of the
    camera (eye and target moved together; cosines of 0.89 to 0.99 were measured), but need not
    for eye moved alone against a fixed target, where the translation and rotation parts nearly
    cancel (one of three measured cases gave a cosine of -0.93)."""
    cams = list(cams)
    v = len(cams)
    if v == 0:
        raise ValueError("at least one camera is required")
    npix = width * height
    grad_out = _f32(grad_out, (v * npix, 3), "grad_out")
    if t_march is not None:
        t_march = _f32(t_march, (v * npix,), "t_march")
    dev = scene.centers.device
    if grad_cams is None:
        if accumulate:
            raise ValueError("accumulate needs the tensor to add into")
        grad_cams = torch.empty((v, 7), device=dev)
    elif _f32(grad_cams, (v, 7), "grad_cams").data_ptr() != grad_cams.data_ptr():
        raise ValueError("grad_cams must be contiguous")
    ctx = context(dev)
    march = native.march_params(steps, smooth_k, normal_eps, color_sharpness, mask_sharpness, flags=flags)
    march = scene.march_for(march)
    for i in range(0, v, native.RM_MAX_VIEWS_PER_CALL):
        chunk = cams[i:i + native.RM_MAX_VIEWS_PER_CALL]
        lo, hi = i * npix, (i + len(chunk)) * npix
        tt = t_march[lo:hi] if t_march is not None else None
        ctx.check(ctx._lib.rm_render_diff_backward_cameras(ctx.handle, native.cameras(chunk), len(chunk), width, height,
                                                           ctypes.byref(scene.c_struct()), ctypes.byref(march),
                                                           _ptr(grad_out[lo:hi]), _ptr(tt),
                                                           _ptr(grad_cams[i:i + len(chunk)]), 1 if accumulate else 0),
                  "rm_render_diff_backward_cameras")
    return grad_cams


def _check_shape(t, name, accepted):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor")
    if tuple(t.shape) not in accepted:
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected " + " or ".join(str(a) for a in accepted))


def _check_param_shapes(centers, radius, light_dir=None, ambient=None):
    """The shapes the autograd functions take for the per-scene parameters, checked before autograd sees
    anything (Scene itself flattens whatever has the right number of elements): radius [M] or [M, 1],
    light_dir [3] or [1, 3], ambient [1] or 0-d. Their gradients come back in the shape passed."""
    m = centers.shape[0] if isinstance(centers, torch.Tensor) and centers.dim() else 0
    _check_shape(centers, "centers", ((m, 3),))
    _check_shape(radius, "radius", ((m,), (m, 1)))
    if light_dir is not None:
        _check_shape(light_dir, "light_dir", ((3,), (1, 3)))
        _check_shape(ambient, "ambient", ((1,), ()))


def _rays(ray_org, ray_dir):
    """The rays as the kernels read them: contiguous float32 [N, 3] (the caller's own tensors where they
    already are, copies otherwise)."""
    n = ray_org.shape[0] if isinstance(ray_org, torch.Tensor) and ray_org.dim() else 0
    return _f32(ray_org, (n, 3), "ray_org"), _f32(ray_dir, (n, 3), "ray_dir")


def _scene_tensors(scene: Scene):
    """What an autograd Function saves of its scene: the five tensors the kernels read. Saved through
    save_for_backward they carry the version of the caller's parameters wherever they alias them, so an
    in-place update between forward and backward raises instead of differentiating the new values."""
    return scene.centers, scene.colors, scene.radius, scene.light_dir, scene.ambient


def _scene_grads(g, shapes):
    """(centers, colors, radius, light_dir, ambient) gradients of the dict g (None where absent), the last
    three in the shapes the caller passed (radius [M] or [M, 1], light_dir [3] or [1, 3], ambient [1] or 0-d)."""
    gr, gl, ga = g.get("radius"), g.get("light_dir"), g.get("ambient")
    return (g.get("centers"), g.get("colors"), gr.reshape(shapes[0]) if gr is not None else None,
            gl.reshape(shapes[1]) if gl is not None else None, ga.reshape(shapes[2]) if ga is not None else None)


class _RenderDiffFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ray_org, ray_dir, centers, colors, radius, light_dir, ambient, smooth_k, steps, normal_eps,
                color_sharpness, mask_sharpness):
        scene = Scene(centers.detach(), colors.detach(), radius.detach(), light_dir.detach(), ambient.detach())
        ray_org, ray_dir = _rays(ray_org.detach(), ray_dir.detach())
        ctx.consts = {"normal_eps": normal_eps, "color_sharpness": color_sharpness, "mask_sharpness": mask_sharpness}
        out, t = render_diff_forward(ray_org, ray_dir, scene, smooth_k, steps, return_t=True, **ctx.consts)
        ctx.save_for_backward(ray_org, ray_dir, t, *_scene_tensors(scene))
        ctx.smooth_k = smooth_k
        ctx.steps = steps
        ctx.shapes = (radius.shape, light_dir.shape, ambient.shape)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        ray_org, ray_dir, t, *saved = ctx.saved_tensors
        scene = Scene(*saved)
        grad_out = grad_out.contiguous().float()
        need = ctx.needs_input_grad
        g_org = g_dir = None
        if need[0] or need[1]:
            g_org, g_dir = render_diff_backward_rays(ray_org, ray_dir, scene, ctx.smooth_k, grad_out, ctx.steps,
                                                     t_march=t, want_org=need[0], want_dir=need[1], **ctx.consts)
        if not any(need[2:7]):  # only the rays are differentiated: the parameter backward does not run
            return (g_org, g_dir) + (None,) * 10
        g = render_diff_backward(ray_org, ray_dir, scene, ctx.smooth_k, grad_out, ctx.steps, t_march=t, **ctx.consts)
        return (g_org, g_dir) + _scene_grads(g, ctx.shapes) + (None,) * 5


def render_diff(ray_org, ray_dir, centers, colors, radius, light_dir, ambient, smooth_k, steps=40, *,
                normal_eps=1e-4, color_sharpness=10.0, mask_sharpness=15.0):
    """renderer_diff.rs:6-91 on the GPU. Differentiable w.r.t. centers, colors, radius, light_dir,
    ambient and, when they require grad, ray_org / ray_dir (see render_diff_backward_rays: the
    reference graph's gradient -- march detached, normal detached -- not the derivative of the
    image). A caller who differentiates only the scene runs the parameter backward alone.

    First order only. The backward reads the caller's own tensors wherever they were contiguous float32 (no
    copy is made), so an in-place change of one of them between forward and backward raises torch's "modified by
    an inplace operation" error. radius [M] or [M, 1], light_dir [3] or [1, 3], ambient [1] or 0-d."""
    _check_param_shapes(centers, radius, light_dir, ambient)
    return _RenderDiffFn.apply(ray_org, ray_dir, centers, colors, radius, light_dir, ambient, float(smooth_k),
                               int(steps), float(normal_eps), float(color_sharpness), float(mask_sharpness))


class _RenderDiffCamerasFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eye, target, fov_deg, width, height, centers, colors, radius, light_dir, ambient, smooth_k,
                steps, normal_eps, color_sharpness, mask_sharpness):
        scene = Scene(centers.detach(), colors.detach(), radius.detach(), light_dir.detach(), ambient.detach())
        e, tg, f = eye.detach().cpu().tolist(), target.detach().cpu().tolist(), fov_deg.detach().cpu().tolist()
        cams = [(e[i], tg[i], f[i]) for i in range(len(f))]
        ctx.consts = {"normal_eps": normal_eps, "color_sharpness": color_sharpness, "mask_sharpness": mask_sharpness}
        out, t = render_diff_camera(cams, width, height, scene, smooth_k, steps, return_t=True, **ctx.consts)
        ctx.save_for_backward(t, *_scene_tensors(scene))
        ctx.cams = cams
        ctx.size = (width, height)
        ctx.smooth_k = smooth_k
        ctx.steps = steps
        ctx.shapes = (radius.shape, light_dir.shape, ambient.shape)
        ctx.cam_meta = (eye.device, eye.dtype, target.device, target.dtype, fov_deg.device, fov_deg.dtype,
                        fov_deg.shape)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        t, *saved = ctx.saved_tensors
        scene = Scene(*saved)
        grad_out = grad_out.contiguous().float()
        need = ctx.needs_input_grad
        w, h = ctx.size
        g_eye = g_tgt = g_fov = None
        if need[0] or need[1] or need[2]:
            gc = render_diff_backward_cameras(ctx.cams, w, h, scene, ctx.smooth_k, grad_out, ctx.steps, t_march=t,
                                              **ctx.consts)
            ed, et, td, tt, fd, ft, fs = ctx.cam_meta
            g_eye = gc[:, 0:3].to(device=ed, dtype=et) if need[0] else None
            g_tgt = gc[:, 3:6].to(device=td, dtype=tt) if need[1] else None
            g_fov = gc[:, 6].reshape(fs).to(device=fd, dtype=ft) if need[2] else None
        gs = (None,) * 5
        if any(need[5:10]):
            g = None
            v, npix = len(ctx.cams), w * h
            for i in range(0, v, native.RM_MAX_VIEWS_PER_CALL):  # the parameter backward takes 128 views a call
                j = min(i + native.RM_MAX_VIEWS_PER_CALL, v)
                gi = render_diff_backward_camera(ctx.cams[i:j], w, h, scene, ctx.smooth_k,
                                                 grad_out[i * npix:j * npix], ctx.steps, t_march=t[i * npix:j * npix],
                                                 **ctx.consts)
                g = gi if g is None else {k: g[k] + gi[k] for k in g}
            gs = _scene_grads(g, ctx.shapes)
        return (g_eye, g_tgt, g_fov, None, None) + gs + (None,) * 5


def render_diff_cameras(eye, target, fov_deg, width, height, centers, colors, radius, light_dir, ambient, smooth_k,
                        steps=40, *, normal_eps=1e-4, color_sharpness=10.0, mask_sharpness=15.0):
    """render_diff over the rays of create_camera_rays (camera.rs:30-90) for V cameras, differentiable
    w.r.t. the camera tensors eye [V,3], target [V,3], fov_deg [V] and the scene: out [V*H*W, 3].

    The camera tensors may live on the host or the device (the poses go to the kernels by value;
    their gradients come back on the tensors' own device). The gradient is the reference graph's
    (march detached, normal detached) chained through create_camera_rays, not the derivative of
    the image: it follows finite differences for a rigid shift of the camera (eye and target moved
    together; measured cosines 0.89 to 0.99) and so serves pose refinement of that kind, but it need
    not for eye moved alone against a fixed target, where the translation and rotation parts
    nearly cancel (one of three measured cases gave a cosine of -0.93). First order only; the scene tensors
    are held as render_diff holds them, the camera tensors are read at forward time."""
    _check_param_shapes(centers, radius, light_dir, ambient)
    v = eye.shape[0] if isinstance(eye, torch.Tensor) and eye.dim() else 0
    for name, t, shape in (("eye", eye, (v, 3)), ("target", target, (v, 3)), ("fov_deg", fov_deg, (v,))):
        _check_shape(t, name, (shape,))
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
    return _RenderDiffCamerasFn.apply(eye, target, fov_deg, int(width), int(height), centers, colors, radius,
                                      light_dir, ambient, float(smooth_k), int(steps), float(normal_eps),
                                      float(color_sharpness), float(mask_sharpness))


def render_diff_camera(cams, width, height, scene: Scene, smooth_k, steps=40, *, normal_eps=1e-4,
                       color_sharpness=10.0, mask_sharpness=15.0, return_t=False):
    """Forward in camera mode: out [V*H*W, 3] for the given cameras (rays made in-kernel)."""
    cams = list(cams)
    v = len(cams)
    if v == 0:
        raise ValueError("at least one camera is required")
    dev = scene.centers.device
    out = torch.empty((v * height * width, 3), device=dev)
    t = torch.empty((v * height * width,), device=dev) if return_t else None
    ctx = context(dev)
    march = native.march_params(steps, smooth_k, normal_eps, color_sharpness, mask_sharpness)
    march = scene.march_for(march)
    for i in range(0, v, native.RM_MAX_VIEWS_PER_CALL):
        chunk = cams[i:i + native.RM_MAX_VIEWS_PER_CALL]
        off = i * height * width
        o = out[off:off + len(chunk) * height * width]
        tt = t[off:off + len(chunk) * height * width] if t is not None else None
        ctx.check(ctx._lib.rm_render_diff_camera(ctx.handle, native.cameras(chunk), len(chunk), width, height,
                                                 ctypes.byref(scene.c_struct()), ctypes.byref(march), _ptr(o),
                                                 _ptr(tt)), "rm_render_diff_camera")
    return (out, t) if return_t else out


def render_diff_backward_camera(cams, width, height, scene: Scene, smooth_k, grad_out, steps=40, *, t_march=None,
                                normal_eps=1e-4, color_sharpness=10.0, mask_sharpness=15.0):
    cams = list(cams)
    if len(cams) > native.RM_MAX_VIEWS_PER_CALL:
        raise ValueError(f"at most RM_MAX_VIEWS_PER_CALL = {native.RM_MAX_VIEWS_PER_CALL} views per backward call")
    n = len(cams) * width * height
    grad_out = _f32(grad_out, (n, 3), "grad_out")
    if t_march is not None:
        t_march = _f32(t_march, (n,), "t_march")
    g, cg = _grads_like(scene)
    ctx = context(scene.centers.device)
    march = native.march_params(steps, smooth_k, normal_eps, color_sharpness, mask_sharpness)
    march = scene.march_for(march)
    ctx.check(ctx._lib.rm_render_diff_backward_camera(ctx.handle, native.cameras(cams), len(cams), width, height,
                                                      ctypes.byref(scene.c_struct()), ctypes.byref(march),
                                                      _ptr(grad_out), _ptr(t_march), ctypes.byref(cg), 0),
              "rm_render_diff_backward_camera")
    return g


# ---- view-dependent sphere colour: spherical harmonics (rm_render_diff_sh) ---------------------
SH_BANDS = {0: 0, 3: 1, 8: 2}  # coefficients per sphere and channel -> degree


def _sh_coeffs(sh, m):
    """(contiguous float32 [M, B, 3] tensor, degree) of the coefficients; B must be 0, 3 or 8."""
    if not isinstance(sh, torch.Tensor) or sh.dim() != 3 or sh.shape[0] != m or sh.shape[2] != 3:
        raise ValueError(f"sh must be a [M, B, 3] tensor with M = {m}")
    if sh.shape[1] not in SH_BANDS:
        raise ValueError(f"sh has {sh.shape[1]} coefficients per sphere and channel: 0, 3 (degree 1) or 8 (degree 2)")
    if sh.shape[1] == 0:
        return None, 0
    return _f32(sh, (m, sh.shape[1], 3), "sh"), SH_BANDS[sh.shape[1]]


def _sh_march(scene, smooth_k, steps, normal_eps, color_sharpness, mask_sharpness, flags):
    return scene.march_for(native.march_params(steps, smooth_k, normal_eps, color_sharpness, mask_sharpness, flags=flags))


def _sh_outputs(scene, sh, want):
    """Output tensors and the (rm_grads, grad_sh) arguments for the gradients named in `want`."""
    dev, m = scene.centers.device, scene.num_spheres
    shapes = {"centers": (m, 3), "colors": (m, 3), "radius": (m,), "light_dir": (3,), "ambient": (1,)}
    if sh is not None:
        shapes["sh"] = tuple(sh.shape)
    unknown = [k for k in want if k not in shapes]
    if unknown:
        raise ValueError(f"unknown gradient {unknown[0]!r}")
    g = {k: torch.empty(shapes[k], device=dev) for k in want}
    cg = RmGrads(*[g[k].data_ptr() if k in g else None for k in ("centers", "colors", "radius", "light_dir", "ambient")])
    return g, cg, _ptr(g.get("sh"))


SH_GRADS = ("centers", "colors", "radius", "light_dir", "ambient", "sh")


def render_diff_sh_forward(ray_org, ray_dir, scene: Scene, sh, smooth_k, steps=40, *, normal_eps=1e-4,
                           color_sharpness=10.0, mask_sharpness=15.0, return_t=False, flags=0):
    """rm_render_diff_sh: render_diff with the albedo max(col_j + sum_b sh[j][b] Y_b(d / |d|), 0) per sphere
    and ray (sh: [M, B, 3], B = 3 or 8; B = 0 is render_diff itself). out [N, 3], and t_march [N] if asked."""
    n = ray_org.shape[0]
    ray_org = _f32(ray_org, (n, 3), "ray_org")
    ray_dir = _f32(ray_dir, (n, 3), "ray_dir")
    sh, deg = _sh_coeffs(sh, scene.num_spheres)
    out = torch.empty((n, 3), device=ray_org.device)
    t = torch.empty((n,), device=ray_org.device) if return_t else None
    ctx = context(ray_org.device)
    march = _sh_march(scene, smooth_k, steps, normal_eps, color_sharpness, mask_sharpness, flags)
    ctx.check(ctx._lib.rm_render_diff_sh(ctx.handle, _ptr(ray_org), _ptr(ray_dir), n, ctypes.byref(scene.c_struct()),
                                         _ptr(sh), deg, ctypes.byref(march), _ptr(out), _ptr(t)), "rm_render_diff_sh")
    return (out, t) if return_t else out


def render_diff_sh_backward(ray_org, ray_dir, scene: Scene, sh, smooth_k, grad_out, steps=40, *, t_march=None,
                            want=SH_GRADS, normal_eps=1e-4, color_sharpness=10.0, mask_sharpness=15.0, flags=0):
    """rm_render_diff_sh_backward: the gradients of sum(out * grad_out) named in `want` (centers, colors,
    radius, light_dir, ambient, sh), as a dict of float32 tensors. Deterministic: two calls give the same bits."""
    n = ray_org.shape[0]
    ray_org = _f32(ray_org, (n, 3), "ray_org")
    ray_dir = _f32(ray_dir, (n, 3), "ray_dir")
    grad_out = _f32(grad_out, (n, 3), "grad_out")
    if t_march is not None:
        t_march = _f32(t_march, (n,), "t_march")
    sh, deg = _sh_coeffs(sh, scene.num_spheres)
    g, cg, gsh = _sh_outputs(scene, sh, want)
    ctx = context(ray_org.device)
    march = _sh_march(scene, smooth_k, steps, normal_eps, color_sharpness, mask_sharpness, flags)
    ctx.check(ctx._lib.rm_render_diff_sh_backward(ctx.handle, _ptr(ray_org), _ptr(ray_dir), n,
                                                  ctypes.byref(scene.c_struct()), _ptr(sh), deg, ctypes.byref(march),
                                                  _ptr(grad_out), _ptr(t_march), ctypes.byref(cg), gsh, 0),
              "rm_render_diff_sh_backward")
    return g


def render_diff_sh_camera(cams, width, height, scene: Scene, sh, smooth_k, steps=40, *, normal_eps=1e-4,
                          color_sharpness=10.0, mask_sharpness=15.0, return_t=False, flags=0):
    """rm_render_diff_sh_camera: render_diff_sh_forward over in-kernel camera rays, out [V*H*W, 3] (up to
    128 views a call)."""
    cams = list(cams)
    if not 1 <= len(cams) <= native.RM_MAX_VIEWS_PER_CALL:
        raise ValueError(f"1..{native.RM_MAX_VIEWS_PER_CALL} views per call")
    n = len(cams) * width * height
    dev = scene.centers.device
    sh, deg = _sh_coeffs(sh, scene.num_spheres)
    out = torch.empty((n, 3), device=dev)
    t = torch.empty((n,), device=dev) if return_t else None
    ctx = context(dev)
    march = _sh_march(scene, smooth_k, steps, normal_eps, color_sharpness, mask_sharpness, flags)
    ctx.check(ctx._lib.rm_render_diff_sh_camera(ctx.handle, native.cameras(cams), len(cams), width, height,
                                                ctypes.byref(scene.c_struct()), _ptr(sh), deg, ctypes.byref(march),
                                                _ptr(out), _ptr(t)), "rm_render_diff_sh_camera")
    return (out, t) if return_t else out


def render_diff_sh_backward_camera(cams, width, height, scene: Scene, sh, smooth_k, grad_out, steps=40, *, t_march=None,
                                   want=SH_GRADS, normal_eps=1e-4, color_sharpness=10.0, mask_sharpness=15.0, flags=0):
    """rm_render_diff_sh_backward_camera: render_diff_sh_backward over in-kernel camera rays."""
    cams = list(cams)
    if not 1 <= len(cams) <= native.RM_MAX_VIEWS_PER_CALL:
        raise ValueError(f"1..{native.RM_MAX_VIEWS_PER_CALL} views per call")
    n = len(cams) * width * height
    grad_out = _f32(grad_out, (n, 3), "grad_out")
    if t_march is not None:
        t_march = _f32(t_march, (n,), "t_march")
    sh, deg = _sh_coeffs(sh, scene.num_spheres)
    g, cg, gsh = _sh_outputs(scene, sh, want)
    ctx = context(scene.centers.device)
    march = _sh_march(scene, smooth_k, steps, normal_eps, color_sharpness, mask_sharpness, flags)
    ctx.check(ctx._lib.rm_render_diff_sh_backward_camera(ctx.handle, native.cameras(cams), len(cams), width, height,
                                                         ctypes.byref(scene.c_struct()), _ptr(sh), deg,
                                                         ctypes.byref(march), _ptr(grad_out), _ptr(t_march),
                                                         ctypes.byref(cg), gsh, 0),
              "rm_render_diff_sh_backward_camera")
    return g


class _RenderDiffShFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ray_org, ray_dir, centers, colors, sh, radius, light_dir, ambient, smooth_k, steps, normal_eps,
                color_sharpness, mask_sharpness):
        scene = Scene(centers.detach(), colors.detach(), radius.detach(), light_dir.detach(), ambient.detach())
        ctx.consts = {"normal_eps": normal_eps, "color_sharpness": color_sharpness, "mask_sharpness": mask_sharpness}
        ray_org, ray_dir = _rays(ray_org.detach(), ray_dir.detach())
        shd = sh.detach()
        if shd.shape[1]:
            shd = _f32(shd, (scene.num_spheres, shd.shape[1], 3), "sh")
        out, t = render_diff_sh_forward(ray_org, ray_dir, scene, shd, smooth_k, steps, return_t=True, **ctx.consts)
        ctx.save_for_backward(ray_org, ray_dir, t, shd, *_scene_tensors(scene))
        ctx.smooth_k = smooth_k
        ctx.steps = steps
        ctx.shapes = (radius.shape, light_dir.shape, ambient.shape)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        ray_org, ray_dir, t, sh, *saved = ctx.saved_tensors
        scene = Scene(*saved)
        need = ctx.needs_input_grad
        names = ("centers", "colors", "sh", "radius", "light_dir", "ambient")
        want = [k for k, w in zip(names, need[2:8]) if w and not (k == "sh" and sh.shape[1] == 0)]
        g = {}
        if want:
            g = render_diff_sh_backward(ray_org, ray_dir, scene, sh, ctx.smooth_k, grad_out.contiguous().float(),
                                        ctx.steps, t_march=t, want=want, **ctx.consts)
        if need[4] and sh.shape[1] == 0:
            g["sh"] = torch.zeros_like(sh)
        gs = _scene_grads(g, ctx.shapes)
        return (None, None, gs[0], gs[1], g.get("sh"), gs[2], gs[3], gs[4], None, None, None, None, None)


def render_diff_sh(ray_org, ray_dir, centers, colors, sh, radius, light_dir, ambient, smooth_k, steps=40, *,
                   normal_eps=1e-4, color_sharpness=10.0, mask_sharpness=15.0):
    """render_diff with view-dependent sphere colour: each sphere's albedo on a ray of direction d is
    max(colors_j + sum_b sh[j][b] Y_b(d / |d|), 0), Y the real spherical harmonics of degree 1 (sh [M, 3, 3])
    or 2 (sh [M, 8, 3]) with 3D Gaussian splatting's constants and signs; sh [M, 0, 3] is render_diff.
    Differentiable w.r.t. centers, colors, sh, radius, light_dir and ambient (rm_render_diff_sh_backward, from
    the forward's saved march t; only the gradients whose inputs require grad are computed). The rays are
    not: Y's dependence on the direction is not differentiated, so rays that require grad raise."""
    if not isinstance(sh, torch.Tensor) or sh.dim() != 3 or sh.shape[1] not in SH_BANDS:
        got = tuple(sh.shape) if isinstance(sh, torch.Tensor) else type(sh).__name__
        raise ValueError(f"sh must be [M, B, 3] with B = 0, 3 (degree 1) or 8 (degree 2), got {got}")
    if any(isinstance(r, torch.Tensor) and r.requires_grad for r in (ray_org, ray_dir)):
        raise ValueError("ray gradients are not available with SH: render_diff_sh does not differentiate ray_org / "
                         "ray_dir (detach them, or use render_diff for the ray and pose gradients)")
    _check_param_shapes(centers, radius, light_dir, ambient)
    return _RenderDiffShFn.apply(ray_org, ray_dir, centers, colors, sh, radius, light_dir, ambient, float(smooth_k),
                                 int(steps), float(normal_eps), float(color_sharpness), float(mask_sharpness))


# ---- image-space loss: weighted L1 + D-SSIM on whole views (rm_image_loss) ----------------------

def _loss_images(out, target, width, height):
    """out and target as contiguous [V, H, W, 3] float32 views of one device; every check runs on the host
    before anything reaches the device. Returns (out, target, V)."""
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError(f"width and height must be >= 1, got {width} x {height}")
    imgs = []
    for name, t in (("out", out), ("target", target)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
        if t.dim() not in (2, 4) or t.shape[-1] != 3:
            raise ValueError(f"{name} must be [V*H*W, 3] or [V, H, W, 3] with 3 channels, got {tuple(t.shape)}")
        if t.dim() == 4 and tuple(t.shape[1:3]) != (height, width):
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected [V, {height}, {width}, 3]")
        pixels = t.numel() // 3
        if pixels == 0 or pixels % (width * height) != 0:
            raise ValueError(f"{name} holds {pixels} pixels, not a positive multiple of "
                             f"width * height = {width * height} (V*H*W)")
        imgs.append(t)
    if imgs[0].numel() != imgs[1].numel():
        raise ValueError(f"out holds {imgs[0].numel() // 3} pixels and target {imgs[1].numel() // 3}")
    if imgs[0].device != imgs[1].device:
        raise ValueError(f"out is on {imgs[0].device} and target on {imgs[1].device}")
    if not imgs[0].is_cuda:
        raise ValueError("out and target must be device (HIP) tensors: the loss has no CPU implementation")
    v = imgs[0].numel() // (3 * width * height)
    return imgs[0].contiguous().view(v, height, width, 3), imgs[1].contiguous().view(v, height, width, 3), v


def image_loss_call(out, target, width, height, *, l1_weight=0.8, ssim_weight=0.2, progress=0.0, plain_l1=False,
                    inv_count=None, c1=1e-4, c2=9e-4, loss=True, view_stats=False, ssim_map=False, grad=False):
    """One rm_image_loss call: a dict of the requested outputs ("loss" [1], "view_stats" [V, 3],
    "ssim_map" and "grad" [V, H, W, 3])."""
    x, y, v = _loss_images(out, target, width, height)
    if inv_count is None:
        inv_count = 1.0 / x.numel()
    dev = x.device
    res = {}
    if loss:
        res["loss"] = torch.empty((1,), device=dev)
    if view_stats:
        res["view_stats"] = torch.empty((v, 3), device=dev)
    if ssim_map:
        res["ssim_map"] = torch.empty_like(x)
    if grad:
        res["grad"] = torch.empty_like(x)
    params = native.image_loss_params(l1_weight=float(l1_weight), ssim_weight=float(ssim_weight),
                                      progress=float(progress), c1=float(c1), c2=float(c2),
                                      flags=native.RM_LOSS_PLAIN_L1 if plain_l1 else 0)
    ctx = context(dev)
    ctx.check(ctx._lib.rm_image_loss(ctx.handle, _ptr(x), _ptr(y), v, int(width), int(height), float(inv_count),
                                     ctypes.byref(params), _ptr(res.get("loss")), _ptr(res.get("view_stats")),
                                     _ptr(res.get("ssim_map")), _ptr(res.get("grad"))), "rm_image_loss")
    return res


class _ImageLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out, target, width, height, kw):
        need = out.requires_grad
        res = image_loss_call(out.detach(), target.detach(), width, height, grad=need, **kw)
        ctx.shape = out.shape
        if need:
            ctx.save_for_backward(res["grad"])
        return res["loss"].reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        (g,) = ctx.saved_tensors
        return (g * grad_loss).reshape(ctx.shape), None, None, None, None


def image_loss(out, target, width, height, *, l1_weight=0.8, ssim_weight=0.2, progress=0.0, plain_l1=False,
               inv_count=None):
    """The image-space loss of 3D Gaussian splatting on whole views, as a scalar differentiable w.r.t. `out`:
    inv_count (l1_weight sum W |out - target| + ssim_weight sum (1 - SSIM)), SSIM with the 11 x 11 Gaussian
    window of sigma 1.5 and zero padding, W compute_loss's weight (10 on the target's foreground, 1 + 4 progress
    elsewhere; plain_l1: 1). out and target: [V*H*W, 3] or [V, H, W, 3] float32 device tensors in the layout of
    render_diff_camera / render_diff_cameras / render_diff_sh; inv_count defaults to 1 / (3 V H W), the mean.
    One rm_image_loss call computes the loss and, when out requires grad, the gradient that backward returns
    times the incoming scalar; target gets none."""
    if isinstance(target, torch.Tensor) and target.requires_grad:
        target = target.detach()
    kw = {"l1_weight": float(l1_weight), "ssim_weight": float(ssim_weight), "progress": float(progress),
          "plain_l1": bool(plain_l1), "inv_count": inv_count}
    _loss_images(out, target, width, height)  # the checks, before autograd sees anything
    return _ImageLossFn.apply(out, target, int(width), int(height), kw)


def image_metrics(out, target, width, height):
    """Per-view image quality on the device: {"psnr": [V], "ssim": [V], "l1": [V]}. PSNR is
    -10 log10(mean (out - target)^2) for peak 1 (inf for identical images), SSIM the mean of the SSIM map, l1 the
    mean |out - target|; formed from rm_image_loss's per-view sums (no gradient kernel runs)."""
    st = image_loss_call(out, target, width, height, plain_l1=True, loss=False, view_stats=True)["view_stats"]
    n = 3.0 * int(width) * int(height)
    return {"psnr": -10.0 * torch.log10(st[:, 1] / n), "ssim": st[:, 2] / n, "l1": st[:, 0] / n}


def train_step(ray_org, ray_dir, targets, scene: Scene, smooth_k, progress, steps=40, *, inv_count=None,
               with_out=False, normal_eps=1e-4, color_sharpness=10.0, mask_sharpness=15.0):
    """Fused forward + training.rs:17-34 seed + backward over rays. Returns (loss_sum, grads, out)."""
    n = ray_org.shape[0]
    ray_org = _f32(ray_org, (n, 3), "ray_org")
    ray_dir = _f32(ray_dir, (n, 3), "ray_dir")
    targets = _f32(targets, (n, 3), "targets")
    if inv_count is None:
        inv_count = 1.0 / (3.0 * n)
    g, cg = _grads_like(scene)
    loss = torch.zeros((1,), device=ray_org.device)
    out = torch.empty((n, 3), device=ray_org.device) if with_out else None
    ctx = context(ray_org.device)
    march = native.march_params(steps, smooth_k, normal_eps, color_sharpness, mask_sharpness)
    march = scene.march_for(march)
    ctx.check(ctx._lib.rm_train_step(ctx.handle, _ptr(ray_org), _ptr(ray_dir), _ptr(targets), n, float(progress),
                                     float(inv_count), ctypes.byref(scene.c_struct()), ctypes.byref(march),
                                     ctypes.byref(cg), _ptr(loss), _ptr(out), 0), "rm_train_step")
    return loss, g, out


def train_step_camera(cams, width, height, targets, scene: Scene, smooth_k, progress, steps=40, *, inv_count=None,
                      grads_packed=None, loss=None, out=None, accumulate=False, march=None, ctx=None,
                      normal_eps=1e-4, color_sharpness=10.0, mask_sharpness=15.0):
    """Camera-mode fused train step. If grads_packed ((7M+4) device tensor) is given the
    gradients go there in the packed layout; otherwise a dict is returned. ctx: the rm_context
    to run on (default: the one of torch's current stream). A given `march` carries its own three
    constants; the keywords apply when it is built here."""
    cams = list(cams)
    if not 1 <= len(cams) <= native.RM_MAX_VIEWS_PER_CALL:
        raise ValueError(f"1..{native.RM_MAX_VIEWS_PER_CALL} views per call")
    n = len(cams) * width * height
    targets = _f32(targets, (n, 3), "targets")
    if inv_count is None:
        inv_count = 1.0 / (3.0 * n)
    if ctx is None:
        ctx = context(scene.centers.device)
    if grads_packed is not None:
        cg = RmGrads()
        ctx._lib.rm_grads_from_packed(_ptr(grads_packed), scene.num_spheres, ctypes.byref(cg))
        g = grads_packed
    else:
        g, cg = _grads_like(scene)
    if loss is None:
        loss = torch.zeros((1,), device=scene.centers.device)
    if march is None:
        march = native.march_params(steps, smooth_k, normal_eps, color_sharpness, mask_sharpness)
    march = scene.march_for(march)
    ctx.check(ctx._lib.rm_train_step_camera(ctx.handle, native.cameras(cams), len(cams), width, height, _ptr(targets),
                                            float(progress), float(inv_count), ctypes.byref(scene.c_struct()),
                                            ctypes.byref(march), ctypes.byref(cg), _ptr(loss), _ptr(out),
                                            1 if accumulate else 0), "rm_train_step_camera")
    return loss, g, out


def create_camera_rays(width, height, eye, target, fov_deg, device="cuda"):
    """camera.rs:30-90 (host loop in f32, like the reference), uploaded as [W*H, 3] tensors."""
    f32 = np.float32
    eye = np.asarray(eye, f32)
    target = np.asarray(target, f32)

    def normalize(v):
        ln = f32(np.sqrt(f32(v[0] * v[0] + v[1] * v[1]) + f32(v[2] * v[2])))
        return np.zeros(3, f32) if ln == 0 else (v / ln).astype(f32)

    fwd = normalize((target - eye).astype(f32))
    up_w = np.array([0, 1, 0], f32)
    right = normalize(np.cross(fwd, up_w).astype(f32))
    up = np.cross(right, fwd).astype(f32)
    aspect = f32(width) / f32(height)
    theta = f32(fov_deg) * (f32(math.pi) / f32(180.0)) / f32(2.0)
    half_h = f32(np.tan(theta))
    half_w = f32(aspect * half_h)
    xs = np.arange(width, dtype=f32)
    ys = np.arange(height, dtype=f32)
    u = (xs / f32(width)) * f32(2) - f32(1)
    v = -((ys / f32(height)) * f32(2) - f32(1))
    rs = (u * half_w)[None, :, None]
    us = (v * half_h)[:, None, None]
    d = (right[None, None, :] * rs + up[None, None, :] * us) + fwd[None, None, :]
    ln = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])[..., None]
    d = (d / ln).astype(f32).reshape(-1, 3)
    o = np.broadcast_to(eye, d.shape).copy()
    return torch.from_numpy(o).to(device), torch.from_numpy(d).to(device)


def render(ray_org, ray_dir, centers, colors, radius):
    """renderer.rs:4-80 (the non-differentiable target renderer of generate.rs) on the GPU."""
    n = ray_org.shape[0]
    m = centers.shape[0]
    ray_org = _f32(ray_org, (n, 3), "ray_org")
    ray_dir = _f32(ray_dir, (n, 3), "ray_dir")
    centers = _f32(centers, (m, 3), "centers")
    colors = _f32(colors, (m, 3), "colors")
    radius = _f32(radius.reshape(-1), (m,), "radius")
    out = torch.empty((n, 3), device=ray_org.device)
    ctx = context(ray_org.device)
    ctx.check(ctx._lib.rm_render(ctx.handle, _ptr(ray_org), _ptr(ray_dir), n, _ptr(centers), _ptr(colors),
                                 _ptr(radius), m, _ptr(out)), "rm_render")
    return out


def render_camera(cams, width, height, centers, colors, radius):
    """renderer.rs:4-80 with in-kernel camera rays: out [V*H*W, 3] (generate.rs:88-104)."""
    cams = list(cams)
    if not 1 <= len(cams) <= native.RM_MAX_VIEWS_PER_CALL:
        raise ValueError(f"1..{native.RM_MAX_VIEWS_PER_CALL} views per call")
    m = centers.shape[0]
    centers = _f32(centers, (m, 3), "centers")
    colors = _f32(colors, (m, 3), "colors")
    radius = _f32(radius.reshape(-1), (m,), "radius")
    out = torch.empty((len(cams) * width * height, 3), device=centers.device)
    ctx = context(centers.device)
    ctx.check(ctx._lib.rm_render_camera(ctx.handle, native.cameras(cams), len(cams), width, height, _ptr(centers),
                                        _ptr(colors), _ptr(radius), m, _ptr(out)), "rm_render_camera")
    return out


# ---- the reference viewer, headless (src/bin/viewer.rs + shader.wgsl; rm_view) -----------------
VIEW_START = ((0.0, 0.0, -2.5), math.pi / 2.0, 0.0)  # the viewer's first pose: pos, yaw, pitch


def view_camera(pos, yaw, pitch):
    """The viewer's camera (viewer.rs:65-86) as (pos, forward, up): forward = (cos yaw cos pitch,
    sin pitch, sin yaw cos pitch) normalised, right = normalize(forward x Y), up = normalize(right x
    forward); angles in radians. ``view_camera(*VIEW_START)`` is where the viewer starts."""
    f = np.array([math.cos(yaw) * math.cos(pitch), math.sin(pitch), math.sin(yaw) * math.cos(pitch)], np.float64)
    f /= np.linalg.norm(f)
    r = np.cross(f, np.array([0.0, 1.0, 0.0]))
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    u /= np.linalg.norm(u)
    return (tuple(float(np.float32(x)) for x in pos), tuple(float(np.float32(x)) for x in f),
            tuple(float(np.float32(x)) for x in u))


def view(cams, width, height, scene: Scene, *, params=None, rgba8=False, depth=False):
    """The reference viewer's frames of `scene` from the poses `cams` ((pos, forward, up) each, see
    view_camera): sphere trace with a per-ray hit exit, four-tap tetrahedral normal, normalised
    exp(-10 d) colour, no mask (shader.wgsl:43-128) -- not the training render. `scene` is drawn as
    given (the viewer draws scene.json's radii without the training activation's +0.01). Returns
    the linear RGB frames [F, H, W, 3] (float32), then, if asked for, the display-encoded RGBA8
    frames [F, H, W, 4] (uint8: piecewise sRGB, alpha 255) and the hit depth [F, H, W] (+inf for a
    miss). `params`: native.view_params(...). No autograd: the viewer is not differentiable."""
    cams = list(cams)
    f = len(cams)
    if f == 0:
        raise ValueError("at least one camera is required")
    dev = scene.centers.device
    p = native.RmViewParams.from_buffer_copy(params) if params is not None else native.view_params()
    p.flags = (p.flags & ~native.RM_MARCH_COLOR_F16) | scene.march_flags
    rgb = torch.empty((f, height, width, 3), device=dev)
    px = torch.empty((f, height, width, 4), device=dev, dtype=torch.uint8) if rgba8 else None
    dp = torch.empty((f, height, width), device=dev) if depth else None
    ctx = context(dev)
    for i in range(0, f, native.RM_MAX_VIEWS_PER_CALL):
        chunk = cams[i:i + native.RM_MAX_VIEWS_PER_CALL]
        j = i + len(chunk)
        ctx.check(ctx._lib.rm_view(ctx.handle, native.view_cameras(chunk), len(chunk), width, height,
                                   ctypes.byref(scene.c_struct()), ctypes.byref(p), _ptr(rgb[i:j]),
                                   _ptr(px[i:j]) if px is not None else None,
                                   _ptr(dp[i:j]) if dp is not None else None), "rm_view")
    out = (rgb,) + ((px,) if rgba8 else ()) + ((dp,) if depth else ())
    return out[0] if len(out) == 1 else out


def sdf_query(points, scene: Scene, smooth_k=32.0, *, color_sharpness=10.0, grad=True, color=True):
    """The scene's distance field at `points` [N, 3] (rm_sdf_query): the soft-min distance D [N] of
    scene.rs:60-79, then, if asked for, its gradient [N, 3] (sum_j softmax(-k d)_j (p - c_j) / rho_j,
    no term from a sphere whose centre the point sits on) and the blended colour [N, 3]
    (softmax(-color_sharpness d) over the spheres' colours, renderer_diff.rs:64-80). `scene` is used
    as given: add the training activation's 0.01 to scene.json's radii for the surface training
    fitted. No autograd: sdf_field is the differentiable form of dist and color."""
    n = points.shape[0]
    points = _f32(points, (n, 3), "points")
    dev = points.device
    dist = torch.empty((n,), device=dev)
    g = torch.empty((n, 3), device=dev) if grad else None
    col = torch.empty((n, 3), device=dev) if color else None
    p = native.sdf_params(smooth_k=float(smooth_k), color_sharpness=float(color_sharpness), flags=scene.march_flags)
    ctx = context(dev)
    ctx.check(ctx._lib.rm_sdf_query(ctx.handle, _ptr(points), n, ctypes.byref(scene.c_struct()), ctypes.byref(p),
                                    _ptr(dist), _ptr(g), _ptr(col)), "rm_sdf_query")
    out = (dist,) + ((g,) if grad else ()) + ((col,) if color else ())
    return out[0] if len(out) == 1 else out


def _field_scene(centers, colors, radius):
    """rm_scene of a distance-field call: no light (the field does not read it). Returns the struct
    and the tensors it points into, which the caller keeps alive until the call is made."""
    m = centers.shape[0]
    centers = _f32(centers, (m, 3), "centers")
    half = colors.dtype == torch.float16
    if half:
        if not colors.is_cuda or tuple(colors.shape) != (m, 3):
            raise ValueError("fp16 colors must be a [M,3] device tensor")
        colors = colors.contiguous()
    else:
        colors = _f32(colors, (m, 3), "colors")
    radius = _f32(radius.reshape(-1), (m,), "radius")
    cs = RmScene(centers.data_ptr(), colors.data_ptr(), radius.data_ptr(), None, None, m)
    return cs, (centers, colors, radius), native.RM_MARCH_COLOR_F16 if half else 0


def sdf_query_backward(points, centers, colors, radius, smooth_k=32.0, *, color_sharpness=10.0, grad_dist=None,
                       grad_color=None, want=("centers", "colors", "radius", "points")):
    """The backward of the field's dist and color (rm_sdf_query_backward, one call): for upstream
    gradients grad_dist [N] and / or grad_color [N, 3], the gradients named in `want` as a dict of
    float32 tensors (centers [M, 3], colors [M, 3], radius [M], points [N, 3]). Half `colors` select
    the fp16 path; their gradient is float32 all the same. Deterministic: two calls give the same
    bits."""
    n = points.shape[0]
    points = _f32(points, (n, 3), "points")
    dev = points.device
    cs, keep, flags = _field_scene(centers, colors, radius)
    m = cs.num_spheres
    gd = _f32(grad_dist.reshape(-1), (n,), "grad_dist") if grad_dist is not None else None
    gc = _f32(grad_color, (n, 3), "grad_color") if grad_color is not None else None
    shapes = {"centers": (m, 3), "colors": (m, 3), "radius": (m,), "points": (n, 3)}
    unknown = [k for k in want if k not in shapes]
    if unknown:
        raise ValueError(f"unknown gradient {unknown[0]!r}")
    out = {k: torch.empty(shapes[k], device=dev) for k in want}
    g = RmGrads(*[out[k].data_ptr() if k in out else None for k in ("centers", "colors", "radius")], None, None)
    p = native.sdf_params(smooth_k=float(smooth_k), color_sharpness=float(color_sharpness), flags=flags)
    ctx = context(dev)
    ctx.check(ctx._lib.rm_sdf_query_backward(ctx.handle, _ptr(points), n, ctypes.byref(cs), ctypes.byref(p), _ptr(gd),
                                             _ptr(gc), ctypes.byref(g), _ptr(out.get("points")), 0),
              "rm_sdf_query_backward")
    del keep
    return out


class _SdfFieldFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, centers, colors, radius, smooth_k, color_sharpness):
        n = points.shape[0]
        pts = _f32(points.detach(), (n, 3), "points")
        cs, keep, flags = _field_scene(centers.detach(), colors.detach(), radius.detach())
        dist = torch.empty((n,), device=pts.device)
        col = torch.empty((n, 3), device=pts.device)
        p = native.sdf_params(smooth_k=smooth_k, color_sharpness=color_sharpness, flags=flags)
        c = context(pts.device)
        c.check(c._lib.rm_sdf_query(c.handle, _ptr(pts), n, ctypes.byref(cs), ctypes.byref(p), _ptr(dist), None,
                                    _ptr(col)), "rm_sdf_query")
        ctx.save_for_backward(pts, *keep)
        ctx.consts = (smooth_k, color_sharpness)
        ctx.shapes = (points.shape, radius.shape)
        ctx.set_materialize_grads(False)
        return dist, col

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_dist, grad_color):
        pts, centers, colors, radius = ctx.saved_tensors
        need = ctx.needs_input_grad
        want = [k for k, w in zip(("points", "centers", "colors", "radius"), need[:4]) if w]
        if not want or (grad_dist is None and grad_color is None):
            return (None,) * 6
        g = sdf_query_backward(pts, centers, colors, radius, ctx.consts[0], color_sharpness=ctx.consts[1],
                               grad_dist=grad_dist.contiguous().float() if grad_dist is not None else None,
                               grad_color=grad_color.contiguous().float() if grad_color is not None else None, want=want)
        gcol = g.get("colors")
        if gcol is not None and colors.dtype == torch.float16:
            gcol = gcol.half()
        gr = g.get("radius")
        return (g["points"].reshape(ctx.shapes[0]) if "points" in g else None, g.get("centers"), gcol,
                gr.reshape(ctx.shapes[1]) if gr is not None else None, None, None)


def sdf_field(points, centers, colors, radius, smooth_k=32.0, *, color_sharpness=10.0):
    """The distance field as a differentiable function: (dist [N], color [N, 3]) of sdf_query at
    `points` [N, 3] for the scene (centers [M, 3], colors [M, 3], radius [M]), with gradients for all
    four through torch.autograd -- supervision in 3-D: fitting the spheres to a point cloud, pulling
    the surface onto depth samples or coloured points, field regularisers, moving query points. The
    forward is rm_sdf_query; the backward is one rm_sdf_query_backward call that computes only the
    gradients whose inputs require grad, from the outputs that received one. Half-precision `colors`
    select the fp16 path and receive their float32 gradient cast to half. First order only (no
    gradient through sdf_query's grad output, no double backward)."""
    _check_param_shapes(centers, radius)
    return _SdfFieldFn.apply(points, centers, colors, radius, float(smooth_k), float(color_sharpness))


def sdf_grid(origin, spacing, shape, scene: Scene, smooth_k=32.0, *, color_sharpness=10.0, color=False):
    """The distance field on a lattice (rm_sdf_grid): shape = (nx, ny, nz) points at origin +
    float32(i) * spacing per axis, formed in the kernel in fp32 with exactly those two roundings.
    Returns D as [nz, ny, nx] (x fastest) and, with color=True, the blended colour [nz, ny, nx, 3]."""
    nx, ny, nz = (int(v) for v in shape)
    dev = scene.centers.device
    dist = torch.empty((nz, ny, nx), device=dev)
    col = torch.empty((nz, ny, nx, 3), device=dev) if color else None
    org = (ctypes.c_float * 3)(*[float(v) for v in origin])
    p = native.sdf_params(smooth_k=float(smooth_k), color_sharpness=float(color_sharpness), flags=scene.march_flags)
    ctx = context(dev)
    ctx.check(ctx._lib.rm_sdf_grid(ctx.handle, ctypes.byref(org), float(spacing), nx, ny, nz,
                                   ctypes.byref(scene.c_struct()), ctypes.byref(p), _ptr(dist), _ptr(col)),
              "rm_sdf_grid")
    return (dist, col) if color else dist
