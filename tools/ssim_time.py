#!/usr/bin/env python3
"""Time of the image-space loss (rm_image_loss: weighted L1 + D-SSIM, its gradient, the per-view sums) next to
a dense torch formulation of the same loss and to the fused train step, on the same GPU in the same run. One JSON
line per step: device events around each call after warm-up, median and min / max of the repetitions, and for the
loss calls the image-sized arrays they move and the bytes per second that makes.

  v10    10 ring views of 512 x 512
  v80    80 ring views of 512 x 512 (the benchmark's view count)

The rendered image is rm_render_diff_camera of model.synthetic_scene(256, 0) at 32 march steps, the target the
same views of model.synthetic_scene(256, 1). Per shape:
  copy              out.clone(): one array read, one written -- the copy bandwidth the fractions refer to
  loss_all          rm_image_loss with every output (loss, view_stats, ssim_map, grad_out): 12 arrays
                    (stats kernel: x, y in, S, A, B, C out; gradient kernel: A, B, C, x, y in, grad out)
  loss_grad         loss and grad_out, what render.image_loss runs in training: 11 arrays
  metrics           view_stats alone, what render.image_metrics runs: 2 arrays, no gradient kernel
  l1_grad           weights (1, 0), grad_out alone: the gradient kernel without its convolutions, 3 arrays
  torch_dense       the same loss in torch: five grouped 11 x 11 conv2d over the 3 V planes in fp32, forward and
                    backward by autograd, in chunks of views that keep the intermediates within a few GB
  train_step        rm_train_step_camera on the rendered scene at 32 march steps: the step the loss is a share of

    python3 tools/ssim_time.py                 # both shapes, each in a child process under `timeout`
    python3 tools/ssim_time.py --shape v10
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, STEPS, SPHERES, WIDTH = 32.0, 32, 256, 512
SHAPES = {"v10": 10, "v80": 80}
SHAPE_LIMIT = 300  # seconds per shape
TORCH_CHUNK = 10   # views per chunk of the dense formulation


def torch_loss(x, y, l1_weight, ssim_weight, inv_count, window):
    """The loss as a user would write it in torch: x, y [V, H, W, 3]."""
    import torch
    import torch.nn.functional as F
    v, h, w, _ = x.shape
    px, py = (t.permute(0, 3, 1, 2).reshape(1, 3 * v, h, w) for t in (x, y))
    wt = window.expand(3 * v, 1, 11, 11)
    blur = lambda a: F.conv2d(a, wt, padding=5, groups=3 * v)
    mx, my = blur(px), blur(py)
    sx, sy, sxy = blur(px * px) - mx * mx, blur(py * py) - my * my, blur(px * py) - mx * my
    s = (2 * mx * my + 1e-4) * (2 * sxy + 9e-4) / ((mx * mx + my * my + 1e-4) * (sx + sy + 9e-4))
    wl = torch.where(y.sum(3, keepdim=True) > 0.01, 10.0, 1.0)
    return inv_count * (l1_weight * (wl * (x - y).abs()).sum() + ssim_weight * (1 - s).sum())


def timed(name, fn, extra, arrays=None, array_bytes=None, reps=10):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    rec = dict(extra, step=name, reps=reps, median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4),
               max_ms=round(max(ms), 4))
    if arrays is not None:
        rec["arrays"] = arrays
        rec["gb_per_s"] = round(arrays * array_bytes / (statistics.median(ms) * 1e-3) / 1e9, 1)
    print(json.dumps(rec), flush=True)
    return statistics.median(ms)


def run_shape(shape):
    import torch
    from burn_raymarching_amd import model, render
    views = SHAPES[shape]
    cams = model.ring_cameras(views)
    scene = model.scene_tensors(model.synthetic_scene(SPHERES, 0))
    x = render.render_diff_camera(cams, WIDTH, WIDTH, scene, K, STEPS)
    y = render.render_diff_camera(cams, WIDTH, WIDTH, model.scene_tensors(model.synthetic_scene(SPHERES, 1)), K, STEPS)
    nbytes = x.numel() * 4
    extra = {"shape": shape, "views": views, "width": WIDTH, "array_mb": round(nbytes / 1e6, 1)}
    call = lambda **kw: render.image_loss_call(x, y, WIDTH, WIDTH, **kw)

    t_copy = timed("copy", lambda: x.clone(), extra, 2, nbytes)
    t_all = timed("loss_all", lambda: call(loss=True, view_stats=True, ssim_map=True, grad=True), extra, 12, nbytes)
    t_grad = timed("loss_grad", lambda: call(loss=True, grad=True), extra, 11, nbytes)
    timed("metrics", lambda: call(loss=False, view_stats=True), extra, 2, nbytes)
    timed("l1_grad", lambda: call(loss=False, grad=True, l1_weight=1.0, ssim_weight=0.0), extra, 3, nbytes)

    g = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-g * g / 4.5)
    g = (g / g.sum()).float().cuda()
    window = (g[:, None] * g[None, :]).reshape(1, 1, 11, 11)
    x4, y4 = x.view(views, WIDTH, WIDTH, 3), y.view(views, WIDTH, WIDTH, 3)
    inv = 1.0 / x.numel()

    def torch_fn():
        for i in range(0, views, TORCH_CHUNK):
            xi = x4[i:i + TORCH_CHUNK].clone().requires_grad_(True)
            torch_loss(xi, y4[i:i + TORCH_CHUNK], 0.8, 0.2, inv, window).backward()

    t_torch = timed("torch_dense", torch_fn, dict(extra, chunk_views=TORCH_CHUNK), reps=5)
    t_step = timed("train_step", lambda: render.train_step_camera(cams, WIDTH, WIDTH, y, scene, K, 0.0, STEPS), extra)
    copy_bw = 2 * nbytes / (t_copy * 1e-3)
    print(json.dumps(dict(extra, step="summary", torch_over_loss_all=round(t_torch / t_all, 2),
                          torch_over_loss_grad=round(t_torch / t_grad, 2),
                          loss_grad_share_of_train_step=round(t_grad / t_step, 4),
                          copy_gb_per_s=round(copy_bw / 1e9, 1),
                          loss_all_fraction_of_copy_bw=round(12 * nbytes / (t_all * 1e-3) / copy_bw, 3),
                          loss_grad_fraction_of_copy_bw=round(11 * nbytes / (t_grad * 1e-3) / copy_bw, 3))), flush=True)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--shape":
        run_shape(sys.argv[2])
        return 0
    for name in SHAPES:  # a fresh process per shape, each under its own limit; stop at the first failure
        rc = subprocess.run(["timeout", "-k", "10", str(SHAPE_LIMIT), sys.executable, os.path.abspath(__file__), "--shape",
                             name]).returncode
        if rc != 0:
            print(json.dumps({"shape": name, "failed": rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
