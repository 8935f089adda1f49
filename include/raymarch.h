/*
 * raymarch.h -- C ABI of libraymarch_hip.so, the MI355X (gfx950) differentiable
 * SDF-sphere raymarcher.
 *
 * This boundary replaces the reference's hot path, the per-ray differentiable
 * render of kokutoupan/burn_raymarching:
 *
 *   render_diff<B: Backend>(ray_org [N,3], ray_dir [N,3], centers [M,3], colors [M,3],
 *                           radius [M,1], light_dir [3], ambient [1], smooth_k: f32)
 *       -> Tensor<B,2> [N,3]                              (src/renderer_diff.rs:6-15)
 *
 * called from SceneModel::forward (src/model/scene.rs:35-57) by the training step
 * (src/bin/train.rs:182) and the preview (src/bin/train.rs:355), together with its
 * gradient, which the reference gets from burn-autodiff via loss.backward()
 * (src/bin/train.rs:189-190). The reference has no FFI for this path; a Rust host
 * would bind these entry points with `extern "C"`.
 *
 * Conventions
 *  - Every tensor argument is a caller-owned DEVICE pointer to fp32, row-major, AoS
 *    [n][3] exactly like the reference's tensors. Camera descriptors are host structs.
 *  - Scene parameters are the ACTIVATED values render_diff receives
 *    (scene.rs:41-45): colors = sigmoid(raw), radius = softplus(raw)+0.01,
 *    ambient = sigmoid(raw), light_dir raw (normalised inside, renderer_diff.rs:49-50).
 *    rm_scene_activate() produces them from the raw Param tensors.
 *  - Every call is asynchronous on the context's stream; the caller synchronises.
 *  - Return value: RM_OK (0) or an RM_ERR_* code; rm_last_error() has the text.
 *    Invalid arguments never launch work. A context is not thread-safe; use one
 *    context per host thread / stream.
 *  - Results are deterministic: every cross-ray sum is reduced in a fixed order.
 */
#ifndef RAYMARCH_H_
#define RAYMARCH_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RM_OK 0
#define RM_ERR_INVALID_ARG 1
#define RM_ERR_HIP 2
#define RM_ERR_OOM 3
#define RM_ERR_UNSUPPORTED 4

/* Limits of this build. */
#define RM_MAX_VIEWS_PER_CALL 128    /* camera descriptors per rm_*_camera call */
#define RM_MAX_SPHERES 65536

typedef struct rm_context rm_context;

/* Activated scene parameters (device pointers), scene.rs:9-16 after scene.rs:41-45. */
typedef struct rm_scene {
  const float* centers;   /* [M,3]                                      */
  const float* colors;    /* [M,3] sigmoid(raw colors)                   */
  const float* radius;    /* [M]   softplus(raw radius) + 0.01           */
  const float* light_dir; /* [3]   raw light direction                   */
  const float* ambient;   /* [1]   sigmoid(raw ambient)                  */
  int32_t num_spheres;    /* M >= 1                                      */
} rm_scene;

/* March / shading constants. rm_march_default() fills the reference's values.
 *
 * Accepted ranges (anything else: RM_ERR_INVALID_ARG, rm_last_error names the field):
 *   normal_eps       finite and > 0
 *   color_sharpness  finite and >= 0 (0: uniform colour weights). The colour sums are shifted by the
 *                    smallest sphere distance on the premise that no exponent is positive. A value
 *                    below 1e-12 acts as 1e-12 (weights of 1 to fp32 rounding; the internal padding
 *                    spheres, 1e15 away, must still underflow to weight 0).
 *   mask_sharpness   finite and >= 0. The escape distances of the march (beyond which the mask is
 *                    exactly 0 in fp32) assume a mask that vanishes outward; at 0 the mask is 0.5
 *                    everywhere, every ray carries gradient and the escaped-ray exit is never armed.
 *
 * normal_eps and the normal. The reference takes the normal from six taps D(p +- eps e_a)
 * (scene.rs:81-128): f_a = D(p + eps e_a) - D(p - eps e_a), n = f / sqrt(|f|^2 + 1e-6). The
 * differentiable modes (rm_render_diff*, rm_train_step* and the ray / camera gradients) do not
 * evaluate the taps: they use their limit as eps -> 0, f = 2 eps grad D, with grad D = sum_j
 * beta_j (p - c_j) / rho_j, beta = softmax(-k delta), no term from a sphere under the clamp of
 * scene.rs:72. normal_eps therefore still sets the length of n (|f| = 2 eps |grad D| against the
 * 1e-6 under the root: |n| is about 0.2 at 1e-4), but not its curvature terms: the limit deviates
 * from the taps by a relative amount that grows as (k eps)^2 (the taps' third-order term; D bends
 * on the scale 1 / k where spheres blend). At the reference's 1e-4 that is below fp32 rounding. The suite holds the kernels to the reference's taps (fp64) up to
 * k * normal_eps = 0.032, where the image differs between the two forms by less than a quarter of the
 * forward bounds (1e-3 max, 1e-5 mean); at k * normal_eps = 0.32 it differs by more than the bounds,
 * and there the suite holds the kernels to the limit form instead (tests/constants_ref.py).
 * Masked |n.l(taps) - n.l(limit)| in fp64, max / mean over 24x24 rays of the final_1 camera, k = 32
 * (tests/test_constants_reference.py re-measures it; at k = 5 the figures are 40 to 200 times smaller):
 *   normal_eps         1e-4           1e-3           3e-3           1e-2           3e-2
 *   scene.json         4e-8 / 8e-10   1.8e-5 / 3e-7  2.0e-4 / 3e-6  2.3e-3 / 3e-5  2.1e-2 / 3e-4
 *   synthetic(48, 3)   2e-7 / 2e-9    2.2e-5 / 6e-7  2.9e-4 / 5e-6  3.7e-3 / 6e-5  2.9e-2 / 5e-4 */
typedef struct rm_march {
  int32_t steps;          /* fixed march steps, renderer_diff.rs:22 (40)             */
  float smooth_k;         /* soft-min sharpness k, sdf.rs:30 (train 5->32, preview 32) */
  float normal_eps;       /* finite-difference normal step, scene.rs:91 (1e-4); see above */
  float color_sharpness;  /* softmax(-c * dist) colour blend, renderer_diff.rs:74 (10) */
  float mask_sharpness;   /* sigmoid(-c * D) silhouette, renderer_diff.rs:88 (15)     */
  int32_t flags;          /* RM_MARCH_* bits (default 0)                              */
} rm_march;

/* Skip the per-sphere work of ray blocks that provably escape the scene: every ray of the
 * block ends its march past the scene's bounding sphere at a distance where the silhouette
 * mask is exactly 0 in f32, so out = 0 and all its gradient terms are 0 -- the values the full
 * computation produces. The proof is a conservative f64 march of a bounding-sphere lower bound
 * in a pre-pass kernel (escapes() in rm_kernels.hip); camera mode then renders 16x16 pixel
 * tiles per block. Pays for compact scenes seen in camera mode (previews, target generation);
 * off by default because the pre-pass and the uneven block costs lose when few blocks escape.
 * Ignored when t_march or debug outputs are requested. */
#define RM_MARCH_SKIP_ESCAPED 1
/* Camera mode: launch rays in row order instead of 16x16 pixel tiles per 256-ray block (8x8
 * per wave; the default when width and height are multiples of 16). Changes the summation order
 * of the gradients and which rays share a wave. A march step's log-sum-exp shift (unshifted,
 * fixed or running maximum, equal to fp32 rounding) is chosen per wave from its own rays: where
 * the scene lets the choice differ between waves (r_max + spread beyond the admission bounds of
 * the cheaper forms, eyes inside the scene) the image and t_march move by that rounding too
 * (2e-6 measured); on scenes that admit one form everywhere they keep their bits. In row order
 * camera mode gives array mode's bits on the same rays. */
#define RM_MARCH_ROW_ORDER 2
/* Disable the escaped-ray early exit: by default a wave stops marching once all its rays
 * recede from the scene's bounding sphere at a distance where the silhouette mask is exactly
 * 0 in fp32 (their outputs and gradient terms are then exactly 0, as the full computation
 * gives). Set for A/B timing; t_march and debug outputs disable it automatically (rays that
 * provably escape still step by the escape bound, see t_march below). */
#define RM_MARCH_NO_EARLY_EXIT 4
/* Camera mode with 16x16 tiles and whole views per launch: dispatch the ray blocks in launch
 * order instead of centre-out (tiles nearest the image centre first, views interleaved, so the
 * blocks that march every step start first and the cheap border blocks fill the tail). The
 * dispatch order changes no result bit: gradient partials are indexed by tile. A/B timing. */
#define RM_MARCH_NATURAL_ORDER 8
/* Run the march's sphere sums on the vector units only. By default the squared distances of
 * the unshifted / fixed-shift march steps come from bf16 matrix-core products of exact
 * three-part splits of the fp32 operands (equal to the fp32 expansion form to rounding) and
 * the vector units do only sqrt, exp2 and the accumulate. A/B timing. */
#define RM_MARCH_VALU_ONLY 16
/* Camera mode: every ray of a view starts at the eye, so by default the first march step's
 * soft-min D(eye) is evaluated once per view (in the per-call record kernel, by the march's own
 * code path for that step) and shared by all rays of the view -- bit-identical results, one
 * march step fewer per ray. This flag makes every ray evaluate it itself. A/B timing. */
#define RM_MARCH_PER_RAY_ORIGIN 32
/* Train / backward calls over the same views (one launch): by default the ray blocks are
 * dispatched grouped by the cost they had in the previous such call (march steps their waves
 * ran, plus the post-march work of live waves), dearest first; this flag keeps the static
 * centre-out order. Results are identical either way. A/B timing. */
#define RM_MARCH_STATIC_ORDER 64
/* Testing: every march step takes the running-maximum log-sum-exp shift (the vector path that
 * follows the reference's exact max, sdf.rs:36-37) instead of the provably safe unshifted /
 * fixed-shift forms; implies RM_MARCH_PER_RAY_ORIGIN. Results agree to fp32 rounding. */
#define RM_MARCH_FORCE_MAX_SHIFT 128
/* fp16 colour / fp32 SDF (BASELINE configs[4]): rm_scene.colors points to IEEE binary16
 * [M,3] activated colours instead of fp32. The per-call record kernel widens them exactly;
 * the colour blend, the SDF, the march and every gradient stay fp32 (grads->colors is fp32,
 * the master gradient). See rm_optimizer_step_f16 for the optimizer side. */
#define RM_MARCH_COLOR_F16 256
/* Split march: a ray block takes 32 rays (half an 8x8 pixel quadrant in camera mode) held by all
 * four waves of the block; every march step each wave sums a quarter of the spheres on the
 * matrix cores and the quarters are added in a fixed order, so the waves march in lockstep;
 * the post-march sweeps are split the same way, and the backward shares the sphere groups out
 * over the four waves. A ray that marches every step then spreads over four SIMDs: for launches that fill
 * the GPU a few times (BASELINE configs[4]), where a few rays march all steps while the rest
 * leave early. Taken automatically from 256 spheres for launches of at most 262,144 rays and
 * from 512 spheres for at most 1,048,576 rays; this flag forces it, RM_MARCH_NO_SPLIT forbids
 * it. Results agree to fp32 rounding (the sphere sums are added in another order). */
#define RM_MARCH_SPLIT 512
#define RM_MARCH_NO_SPLIT 1024

/* Pinhole LookAt camera, camera.rs:30-37. Rays are generated in-kernel exactly as
 * create_camera_rays (camera.rs:41-87): rows y then x, u = x/W*2-1, v = -(y/H*2-1). */
typedef struct rm_camera {
  float eye[3];
  float target[3];
  float fov_deg;
} rm_camera;

/* Gradient outputs (device pointers) w.r.t. the ACTIVATED parameters, except
 * light_dir which is w.r.t. the raw light direction (the normalisation is inside
 * render_diff). Any pointer may be NULL to skip that output. */
typedef struct rm_grads {
  float* centers;    /* [M,3] */
  float* colors;     /* [M,3] */
  float* radius;     /* [M]   */
  float* light_dir;  /* [3]   */
  float* ambient;    /* [1]   */
} rm_grads;

/* ---- context --------------------------------------------------------------- */
/* "burn_raymarching_amd <version> (gfx950) src <hash>": <hash> = the first 16 hex digits of the
 * sha256 of the kernel sources the library was built from (burn_raymarching_amd/_build.py). */
const char* rm_version(void);
/* stream: a hipStream_t (NULL = the null stream). */
int rm_create(int32_t device, void* stream, rm_context** out_ctx);
int rm_set_stream(rm_context* ctx, void* stream);
void rm_destroy(rm_context* ctx);
const char* rm_last_error(const rm_context* ctx);
void rm_march_default(rm_march* m);
/* Pre-size the workspace for backward/train calls of up to max_rays rays and
 * max_spheres spheres, and allocate the context's small per-call buffers (reduction arrival
 * counters, the fused iteration's optimizer hand-off), so later calls never allocate (needed
 * for hipGraph capture; keeps first-call allocations out of a timed loop). */
int rm_reserve(rm_context* ctx, int64_t max_rays, int32_t max_spheres);

/* ---- forward: renderer_diff.rs:6-91 --------------------------------------- */
/* out [N,3] receives render_diff(ray_org, ray_dir, scene..., smooth_k).
 * ray_dir (every array-mode call): taken as given, p = ray_org + ray_dir t as in the reference,
 * and nothing is rejected. The march's shortcuts, though, are proven for unit directions, |d|^2
 * within 1 +- 4e-6 (what normalising in fp32 gives; camera mode's rays are unit by
 * construction): the escape bound ("every step is at least |p - c| - R' long") and the
 * clamp-free proof ("the next point is |D| away"). Unit directions are the precondition of the
 * bit-level guarantees below (the same bits with the early exit on and off, with t_march and
 * without). With other directions the results still follow the reference within the suite's
 * bounds where measured (x0.25, x0.5 / x2 alternating; x0.1 with RM_MARCH_NO_EARLY_EXIT), but
 *   - a ray shorter than unit can be taken for escaped while its mask is not yet exactly 0: a
 *     wave of such rays returns exact zeros where the reference has tiny values (at |d| = 0.02,
 *     48 spheres and 32 steps the reference's image is <= 3e-8 and its sphere gradients reach
 *     1e-5), and the exit on and off differ in the last bits of out (8.8e-17 measured at
 *     |d| = 0.25);
 *   - a ray longer than unit can pass the clamp-free proof at a point within 1e-3 of a sphere
 *     centre, where the reference clamps q at 1e-6.
 * A caller with scaled directions normalises them and scales t.
 * t_march (nullable) [N] receives the detached march distance t after `steps`
 * steps (renderer_diff.rs:20-26), which rm_render_diff_backward can reuse. For a ray that
 * provably escapes the scene -- receding from its bounding sphere so far that the silhouette
 * mask, out and every gradient term are exactly 0 in fp32 -- the march continues with steps
 * of that escape bound (|p - c| - R - ln(M)/k, never longer than the soft-min step), so its
 * t_march is at most the reference's t and already past the distance where the mask is 0;
 * every other ray's t_march is the reference march to fp32 rounding. Either t gives the same
 * out and gradients. "To fp32 rounding" is per step: a receding ray's next step is as long as
 * its distance from the scene, so it doubles whatever error it carries with every step. For a
 * ray the image sees, t_march is within 1e-3 of the reference's, relative to max(1, t). A ray
 * that hovers at a surface for most of the march and leaves in the last few steps -- unseen, not
 * yet proven escaped -- has an ill-conditioned t: the reference's own fp64 t moves by 3e-5 under
 * one rounding of the inputs at such a ray, and the kernels' three log-sum-exp shift forms, equal
 * to rounding per step, end 1.9e-4 (running maximum), 7e-4 (vector units) and 1.2e-3 (default)
 * from the fp64 t there. For those rays the bound is 64 times that sensitivity
 * (tests/envelope_ref.py, t_bound); out and every gradient are unaffected (the mask is 0). */
int rm_render_diff(rm_context* ctx, const float* ray_org, const float* ray_dir, int64_t num_rays,
                   const rm_scene* scene, const rm_march* march, float* out, float* t_march);
/* Camera mode: rays of `num_views` cameras at width x height generated in-kernel;
 * out is [num_views*height*width, 3] in view, row, column order. */
int rm_render_diff_camera(rm_context* ctx, const rm_camera* cams, int32_t num_views, int32_t width,
                          int32_t height, const rm_scene* scene, const rm_march* march, float* out,
                          float* t_march);

/* ---- backward: the burn-autodiff gradient of render_diff ------------------ */
/* grad_out [N,3] = dL/d(out). t_march (nullable) = the forward's saved march t;
 * when given the march is not replayed. accumulate != 0 adds into the grads. */
int rm_render_diff_backward(rm_context* ctx, const float* ray_org, const float* ray_dir, int64_t num_rays,
                            const rm_scene* scene, const rm_march* march, const float* grad_out,
                            const float* t_march, const rm_grads* grads, int32_t accumulate);
int rm_render_diff_backward_camera(rm_context* ctx, const rm_camera* cams, int32_t num_views, int32_t width,
                                   int32_t height, const rm_scene* scene, const rm_march* march,
                                   const float* grad_out, const float* t_march, const rm_grads* grads,
                                   int32_t accumulate);

/* ---- backward w.r.t. the rays and the camera poses ------------------------- */
/* The gradient of the reference's graph with respect to render_diff's first two arguments
 * (renderer_diff.rs:6-15; the march t and the normal are detached, :25 and :41-46): with
 * p_a = o + d t, t_f = t + D(p_a), p_f = o + d t_f, g_p = dL/dp_f and g_pa = (g_p . d) grad D(p_a),
 *   dL/do = g_p + g_pa,   dL/dd = t_f g_p + t g_pa.
 * It is the reference autodiff's gradient, not the derivative of the image through the march.
 * Rays whose backward seeds are zero (every escaped ray) get exact zeros. One dedicated kernel
 * (one ray per lane), no floating-point atomics; when t_march is NULL the forward replays the
 * march first. RM_MARCH_COLOR_F16 is honoured; the march-path A/B flags apply to that replay only. */
/* dL/d(ray_org), dL/d(ray_dir) of render_diff for grad_out = dL/d(out): [N,3] each, either NULL
 * to skip it; accumulate != 0 adds. t_march as in rm_render_diff_backward. */
int rm_render_diff_backward_rays(rm_context* ctx, const float* ray_org, const float* ray_dir, int64_t num_rays,
                                 const rm_scene* scene, const rm_march* march, const float* grad_out,
                                 const float* t_march, float* grad_org, float* grad_dir, int32_t accumulate);
/* dL/d(eye, target, fov_deg) per view: grad_cams is DEVICE memory, num_views records laid out as
 * rm_camera (7 floats). The ray gradients chained through create_camera_rays (camera.rs:41-79);
 * math::normalize of a zero vector has a zero Jacobian here, so the result is finite. */
int rm_render_diff_backward_cameras(rm_context* ctx, const rm_camera* cams, int32_t num_views, int32_t width,
                                    int32_t height, const rm_scene* scene, const rm_march* march,
                                    const float* grad_out, const float* t_march, rm_camera* grad_cams,
                                    int32_t accumulate);

/* ---- view-dependent sphere colour: spherical harmonics --------------------- */
/* render_diff with a colour per sphere AND ray direction. B = (sh_degree + 1)^2 - 1 (3 or 8); sh is
 * DEVICE memory, fp32 [M, B, 3], sh[(j*B + b)*3 + c]; degree 0 is scene->colors. For a ray of
 * direction d, u = d / |d| (a zero direction gives Y = 0) and, with the real SH constants and signs of
 * 3D Gaussian splatting,
 *   C1 = 0.4886025119029199
 *   Y_1..3 = -C1 u.y,  C1 u.z,  -C1 u.x
 *   C2 = {1.0925484305920792, -1.0925484305920792, 0.31539156525252005,
 *         -1.0925484305920792, 0.5462742152960396}
 *   Y_4..8 = C2[0] xy,  C2[1] yz,  C2[2] (2zz - xx - yy),  C2[3] xz,  C2[4] (xx - yy)
 * the albedo of sphere j on that ray is a_jc = max(col_jc + sum_b sh[j][b][c] Y_b(u), 0) -- the clamp
 * per sphere and per channel -- and everything else is render_diff (renderer_diff.rs:6-91) with the
 * colours replaced by a, t and the normal detached:
 *   mix_c = sum_j w_j a_jc,  w = softmax(-color_sharpness delta),   out = mix L mu.
 * With g = dL/dout, gm = g L mu and mg = gm . mix the backward returns
 *   dL/dcol_jc = w_j gm_c [a_jc > 0],   dL/dsh[j][b][c] = w_j gm_c Y_b [a_jc > 0],
 * the colour term of dL/ddelta_j is -color_sharpness w_j (gm . a_j - mg), and the mask, reconnect,
 * light and ambient terms are rm_render_diff_backward's with this mix. Y depends on the ray
 * direction; that dependence is not differentiated (there is no ray or pose gradient with SH).
 * sh_degree == 0: sh and grad_sh are ignored and the call IS the existing entry point, bit for bit.
 * sh_degree outside 0..RM_SH_MAX_DEGREE, or sh NULL with sh_degree > 0: RM_ERR_INVALID_ARG.
 * The march is the existing kernels' (every march flag applies to it); out comes from a shade
 * kernel of its own that starts from the march's t. t_march: a nullable output of the forward, a
 * nullable input of the backward (NULL: the march is replayed). RM_MARCH_COLOR_F16 is honoured for
 * scene->colors; sh and grad_sh are always fp32.
 * Backward: grads is nullable, as is each of its members and grad_sh ([M, B, 3], DEVICE); at least
 * one output is required. accumulate as in rm_render_diff_backward: without it every element of
 * every requested output is overwritten (num_rays == 0: with zeros). Rays whose backward seeds are
 * zero (every escaped ray) add exact zeros. No floating-point atomics: two calls give the same
 * bits, and an output's bits do not depend on which other outputs are requested. */
#define RM_SH_MAX_DEGREE 2
int rm_render_diff_sh(rm_context* ctx, const float* ray_org, const float* ray_dir, int64_t num_rays,
                      const rm_scene* scene, const float* sh, int32_t sh_degree, const rm_march* march,
                      float* out, float* t_march);
int rm_render_diff_sh_camera(rm_context* ctx, const rm_camera* cams, int32_t num_views, int32_t width,
                             int32_t height, const rm_scene* scene, const float* sh, int32_t sh_degree,
                             const rm_march* march, float* out, float* t_march);
int rm_render_diff_sh_backward(rm_context* ctx, const float* ray_org, const float* ray_dir, int64_t num_rays,
                               const rm_scene* scene, const float* sh, int32_t sh_degree, const rm_march* march,
                               const float* grad_out, const float* t_march, const rm_grads* grads,
                               float* grad_sh, int32_t accumulate);
int rm_render_diff_sh_backward_camera(rm_context* ctx, const rm_camera* cams, int32_t num_views, int32_t width,
                                      int32_t height, const rm_scene* scene, const float* sh, int32_t sh_degree,
                                      const rm_march* march, const float* grad_out, const float* t_march,
                                      const rm_grads* grads, float* grad_sh, int32_t accumulate);

/* ---- fused train step: forward + compute_loss seed + backward ------------- */
/* The reconstruction term of compute_loss (training.rs:17-34): for each ray,
 * W = 10 where sum(target) > 0.01 else 1 + 4*progress, loss += sum_c |out-target|*W,
 * g = W*sign(out-target)*inv_count (inv_count = 1/(3*N_global) gives the mean).
 * loss_sum (device, 1 float) receives sum |out-target|*W (multiply by inv_count
 * for the mean), added to its current value when accumulate != 0. out (nullable)
 * receives the forward image. targets are linear RGB [N,3]. */
int rm_train_step(rm_context* ctx, const float* ray_org, const float* ray_dir, const float* targets,
                  int64_t num_rays, float progress, float inv_count, const rm_scene* scene,
                  const rm_march* march, const rm_grads* grads, float* loss_sum, float* out,
                  int32_t accumulate);
int rm_train_step_camera(rm_context* ctx, const rm_camera* cams, int32_t num_views, int32_t width,
                         int32_t height, const float* targets, float progress, float inv_count,
                         const rm_scene* scene, const rm_march* march, const rm_grads* grads,
                         float* loss_sum, float* out, int32_t accumulate);

/* ---- image-space loss: weighted L1 + D-SSIM over whole views --------------- */
/* The loss of 3D Gaussian splatting, (1 - lambda) L1 + lambda (1 - SSIM), on rendered views, with its
 * gradient and the sums behind PSNR / SSIM / L1. x = out is the rendered image and y = targets the
 * target, both DEVICE fp32 [V, H, W, 3] in the layout rm_render_diff_camera writes: pixel (v, row, col)
 * at ((v*H + row)*W + col)*3 + c.
 *   window    w(i, j) = g(i) g(j), g the 11-tap Gaussian of sigma 1.5 normalised to sum 1 (separable)
 *   padding   pixels outside an image are zeros (conv2d(padding = 5)); every view and every channel is
 *             its own image, nothing is read across a view boundary
 *   per pixel and channel, with F(a) = sum w a over the window:
 *     mux = F(x), muy = F(y), sx = F(x^2) - mux^2, sy = F(y^2) - muy^2, sxy = F(xy) - mux muy
 *     S = (2 mux muy + c1)(2 sxy + c2) / ((mux^2 + muy^2 + c1)(sx + sy + c2))
 *   L1 term   W |x - y|, W compute_loss's weight of the TARGET pixel exactly as the train step forms it:
 *             (t0 + t1 + t2) > 0.01f ? 10 : fmaf(progress, 4, 1); with RM_LOSS_PLAIN_L1, W = 1. sign(0) = 0.
 *   loss = inv_count * (l1_weight * sum W|x - y| + ssim_weight * sum (1 - S)), the sums over every pixel
 *   and channel of the call. inv_count = 1 / (3 V H W) gives the mean; a caller that splits a step over
 *   calls or ranks passes the global count and the losses (and gradients) add: rm_train_step's convention.
 *   grad_out = d loss / d x with y held constant:
 *     L1 part    W * sign(x - y) * s, s = l1_weight * inv_count formed once on the host in float (for
 *                l1_weight = 1 bit for bit the seed rm_train_step forms)
 *     SSIM part  with B = dS/dsx, C = dS/dsxy, A = dS/dmux - 2 mux B - muy C:
 *                d(sum S)/dx_p = sum_q w(q - p) (A_q + 2 x_p B_q + y_p C_q), scaled by -ssim_weight * inv_count.
 * Outputs, all DEVICE and nullable, at least one required: loss (1 float); view_stats [V][3] = per view
 * sum W|x - y|, sum (x - y)^2, sum S; ssim_map [V, H, W, 3] = S; grad_out [V, H, W, 3], overwritten.
 * grad_out NULL: the gradient kernel does not run (the metrics path). num_views, width, height >= 1: no
 * view cap and no multiple-of-16 rule. The weights are finite and >= 0, c1 and c2 finite and > 0, flags
 * RM_LOSS_* only; grad_out and ssim_map must not overlap out, targets or each other. Anything else:
 * RM_ERR_INVALID_ARG with the field named in rm_last_error, before any launch. params NULL: the defaults.
 * The per-view sums are the fp64 sum of the tiles' partial sums in tile order, rounded once to float, and
 * the loss the fp64 sum of those over the views: no floating-point atomics, two calls give the same bits,
 * and an output's bits do not depend on which other outputs are requested. Scratch (three image-sized
 * arrays when a gradient with ssim_weight > 0 is asked for) is the context's: the first call of a shape
 * grows it, later calls allocate nothing and never synchronise. */
#define RM_LOSS_PLAIN_L1 1
typedef struct rm_image_loss_params {
  float l1_weight;    /* 0.8 */
  float ssim_weight;  /* 0.2 */
  float progress;     /* compute_loss's background weight 1 + 4 progress (0) */
  float c1, c2;       /* 1e-4, 9e-4 */
  int32_t flags;      /* RM_LOSS_* */
} rm_image_loss_params;
void rm_image_loss_default(rm_image_loss_params* p);   /* 0.8, 0.2, 0, 1e-4, 9e-4, 0 */
int rm_image_loss(rm_context* ctx, const float* out, const float* targets, int32_t num_views, int32_t width,
                  int32_t height, float inv_count, const rm_image_loss_params* params, float* loss,
                  float* view_stats, float* ssim_map, float* grad_out);

/* ---- non-differentiable target renderer: renderer.rs:4-80 (used by generate.rs) ---- */
/* 40 march steps at k = 32, detached normal, fixed light (-0.5, 0.5, -1)/|.|, lighting =
 * diffuse + 0.1, colour = sum(col exp(-10 d)) / (sum(exp(-10 d)) + 1e-5), mask = exp(-10 D^2).
 * centers/colors/radius are device pointers ([M,3], [M,3], [M]); out [N,3]. */
int rm_render(rm_context* ctx, const float* ray_org, const float* ray_dir, int64_t num_rays,
              const float* centers, const float* colors, const float* radius, int32_t num_spheres, float* out);
int rm_render_camera(rm_context* ctx, const rm_camera* cams, int32_t num_views, int32_t width, int32_t height,
                     const float* centers, const float* colors, const float* radius, int32_t num_spheres,
                     float* out);

/* ---- the reference viewer, headless: src/bin/viewer.rs + src/bin/shader.wgsl ---------------- */
/* How a user looks at the scene.json that training wrote, as frames instead of a window. The
 * viewer's math is not the training render's: a sphere trace with a per-ray exit at a hit
 * threshold (t = 0; up to max_steps times: d = D(pos + t rd); d < hit_eps is a hit, else t > t_max
 * is a miss, else t += d), the four-tap tetrahedral normal at normal_eps, the normalised
 * exp(-color_sharpness d) colour with its absolute 1e-5, Lambert + ambient, and no silhouette mask:
 * a miss is exactly 0. Pixel (i, j) of a frame, row 0 at the top, looks along
 * normalize(ux uu + uy vv + focal ww) with ux = (2 (i + .5) / W - 1) W / H, uy = 1 - 2 (j + .5) / H,
 * ww = normalize(forward), uu = normalize(ww x up), vv = normalize(uu x ww) (shader.wgsl:104-112).
 * Two stated differences from the reference: the soft-min is a shifted
 * log-sum-exp, so it keeps rendering where the shader's unshifted fp32 fold underflows to log(0)
 * (every sphere farther than about 2.7 units) and the reference goes black; and a tap sum of exactly
 * zero gives a zero diffuse term, not NaN. Not differentiable. */
typedef struct rm_view_camera {
  float pos[3];
  float forward[3];
  float up[3];
} rm_view_camera;
typedef struct rm_view_params {
  int32_t max_steps;      /* trace iterations, shader.wgsl MAX_STEPS (100)              */
  float smooth_k;         /* soft-min sharpness (32)                                    */
  float hit_eps;          /* hit threshold on D (1e-3)                                  */
  float t_max;            /* a ray past this t is a miss (20)                           */
  float normal_eps;       /* tetrahedral tap distance (1e-3)                            */
  float color_sharpness;  /* exp(-c d) colour weights (10)                              */
  float focal;            /* image plane distance (1.5)                                 */
  int32_t flags;          /* RM_MARCH_COLOR_F16, RM_MARCH_NO_EARLY_EXIT, RM_VIEW_* bits  */
} rm_view_params;
/* Diagnostics: out_depth receives the number of soft-min evaluations the ray's trace made (as a
 * float, 0 for no ray) instead of its depth; the exact skips are off, so it is the count of the
 * trace as specified. */
#define RM_VIEW_COUNT_ITERATIONS 65536
void rm_view_params_default(rm_view_params* params);   /* 100, 32, 1e-3, 20, 1e-3, 10, 1.5, 0 */
/* Renders num_frames (1 .. RM_MAX_VIEWS_PER_CALL) frames of width x height from the poses cams
 * (HOST memory, like rm_camera). scene is used as given: scene.json stores the radii without the
 * +0.01 of the training activation and the reference viewer draws them so; whether to add it is
 * the caller's business. Outputs (device pointers, any may be NULL but not all three):
 *   out_rgb   [F,H,W,3] linear float RGB;
 *   (float arrays, here and in every other call of this header, inputs and outputs alike, need the
 *   4-byte alignment of a float and no more: the kernels read and write the caller's arrays one
 *   word at a time, so a view that starts an odd number of floats into an allocation is as good
 *   as the allocation; tests/test_gpu_autograd_contract.py pins the bits for the float32 inputs)
 *   out_rgba8 [F,H,W,4] (4-byte aligned) the bytes the viewer's sRGB surface shows: the piecewise
 *             sRGB encode (12.92 c below 0.0031308, else 1.055 c^(1/2.4) - 0.055) rounded to
 *             nearest, alpha 255 -- not the gamma-1/2.2 truncation of the training PNGs (util.rs);
 *   out_depth [F,H,W] t at the hit, +inf for a miss.
 * Rays that provably cannot hit (their line stays outside the scene's bounding sphere grown by
 * hit_eps + ln(M)/k and a rounding margin, or they recede beyond it) end as misses without further
 * marching; RM_MARCH_NO_EARLY_EXIT in flags turns that off: the same bits either way. params NULL =
 * the defaults. Two identical calls give identical bits. */
int rm_view(rm_context* ctx, const rm_view_camera* cams, int32_t num_frames, int32_t width, int32_t height,
            const rm_scene* scene, const rm_view_params* params, float* out_rgb, uint8_t* out_rgba8,
            float* out_depth);

/* ---- the scene's distance field at points of the caller's choosing: scene.rs:60-79 --------- */
/* What every kernel here evaluates, as a query: for a point p, with d_j = sqrt(max(|p - c_j|^2,
 * 1e-6)) - r_j,
 *   dist   D(p) = softmin_k(d), the log-sum-exp shifted by its maximum with the reference's
 *          clamp_min(sum, 1e-8) (sdf.rs:30-44); finite however far p lies from the scene;
 *   grad   grad D(p) = sum_j beta_j (p - c_j) / rho_j, beta = softmax(-k d); a sphere with
 *          |p - c_j|^2 < 1e-6 contributes no term (the zero Jacobian of clamp_min: what autograd of
 *          the reference's graph gives);
 *   color  sum_j w_j col_j, w = softmax(-color_sharpness d), the blend of renderer_diff.rs:64-80.
 * |p - c_j|^2 comes from p - c_j in direct form; the reference's expansion form differs in rounding.
 * scene is used as given (light_dir and ambient are not read and may be NULL); whether the radii
 * carry the +0.01 of the training activation is the caller's business. flags takes
 * RM_MARCH_COLOR_F16 only. One dedicated kernel, one point per lane, no atomics: two identical
 * calls give identical bits, and an output has the same bits whichever others are requested. */
typedef struct rm_sdf_params {
  float smooth_k;         /* soft-min sharpness k (32): finite and > 0                  */
  float color_sharpness;  /* softmax(-c d) colour blend (10): finite and >= 0           */
  int32_t flags;          /* RM_MARCH_COLOR_F16 or 0                                    */
} rm_sdf_params;
void rm_sdf_params_default(rm_sdf_params* params);   /* 32, 10, 0 */
/* points [N,3] (device). Outputs (device pointers, any may be NULL but not all three): dist [N],
 * grad [N,3], color [N,3]. num_points == 0 returns RM_OK without a launch. params NULL = the
 * defaults. */
int rm_sdf_query(rm_context* ctx, const float* points, int64_t num_points, const rm_scene* scene,
                 const rm_sdf_params* params, float* dist, float* grad, float* color);
/* The backward of rm_sdf_query's dist and color (not of its grad: no second order). For upstream
 * gradients gD = grad_dist [N] and gC = grad_color [N,3] (device; either may be NULL, not both), with
 * e_j = p - c_j, q_j = |e_j|^2, rho_j = sqrt(max(q_j, 1e-6)), beta = softmax(-k d), w =
 * softmax(-color_sharpness d) and C = sum_j w_j col_j as above, per point
 *   a_j = gD beta_j - color_sharpness w_j (gC . (col_j - C)),
 *   u_j = e_j / rho_j if q_j >= 1e-6, else 0 (the zero Jacobian of clamp_min, as in grad above),
 *   dL/dc_j += -a_j u_j,  dL/dr_j += -a_j,  dL/dcol_j += w_j gC,  dL/dp_i = sum_j a_j u_j.
 * The clamp_min(sum, 1e-8) of the shifted log-sum-exp is never active (the nearest sphere's term is
 * 1) and has no branch in the gradient. Outputs: grads (nullable; its centers / colors / radius, any
 * of them NULL to skip it; light_dir and ambient are never written: the field does not depend on
 * them) and grad_points [N,3] (nullable); at least one output must be requested. accumulate != 0
 * adds into the outputs; otherwise every element of every requested output is overwritten, all M
 * rows of grads included. num_points == 0 with accumulate == 0 writes zeros to grads and returns
 * without a per-point launch. params as in rm_sdf_query; with RM_MARCH_COLOR_F16 the scene's colours
 * are read as binary16 and grads->colors stays float32. No floating-point atomics: every sum over
 * the points is taken in a fixed order, two identical calls give identical bits, and an output's bits
 * do not depend on which other outputs are requested. A point whose seeds are all zero contributes
 * exact zeros. Calls of more points than one launch takes are split as the ray calls are. Scratch
 * (one partial record of 8 M + 8 floats per 256 points of a launch, at most 256 MB of them, plus the
 * reduction's segment sums) is the context's workspace, grown on demand: the first call may allocate. */
int rm_sdf_query_backward(rm_context* ctx, const float* points, int64_t num_points, const rm_scene* scene,
                          const rm_sdf_params* params, const float* grad_dist, const float* grad_color,
                          const rm_grads* grads, float* grad_points, int32_t accumulate);
/* rm_sdf_query on the lattice p = origin + (float)i * spacing per axis (formed in the kernel in fp32
 * with these two roundings, no fused multiply-add, so a host reproduces the points bit for bit; no
 * point array): origin is HOST memory, spacing > 0, nx, ny, nz >= 1. dist [nz,ny,nx] and color
 * [nz,ny,nx,3] (either NULL, not both), x fastest: index (iz ny + iy) nx + ix. Bit for bit
 * rm_sdf_query at those points. */
int rm_sdf_grid(rm_context* ctx, const float origin[3], float spacing, int32_t nx, int32_t ny, int32_t nz,
                const rm_scene* scene, const rm_sdf_params* params, float* dist, float* color);

/* ---- batch gather: SceneDataset::sample_batch, dataset.rs:75-79 ---------------- */
/* out_*[i] = src[indices[i]] for the ray origin, direction and target arrays ([num_src,3]
 * each; any output may be NULL to skip it). indices is a device int32 [num_rays]; an index
 * outside [0, num_src) gives a zero row. */
int rm_gather_rays(rm_context* ctx, const float* ray_org, const float* ray_dir, const float* targets,
                   int64_t num_src, const int32_t* indices, int64_t num_rays, float* out_org, float* out_dir,
                   float* out_targets);

/* ---- batch sampler on the device: SceneDataset::sample_batch, dataset.rs:47-82 ------------- */
/* Draws n_uniform pixel indices uniformly from [0, num_src), then n_fg more uniformly from the
 * foreground list fg_indices[0, num_fg) (device int32; dataset.rs:54-73 -- the counts come from
 * the caller, see rmh_dataset_sample_count), and gathers those rows of ray_org / ray_dir /
 * targets ([num_src,3] device arrays) into out_* ([n_uniform+n_fg,3]; any NULL to skip it);
 * indices_out (nullable, int32) receives the drawn indices. The generator is counter-based (row
 * i of call (seed, stream, counter) is a splitmix64 draw of those four numbers), so a batch is
 * reproducible and independent of the launch; the reference's draws (rand::rng()) are unseeded,
 * so batches match it in distribution. One kernel: no host sampling, no host-to-device copy. */
int rm_sample_batch(rm_context* ctx, const float* ray_org, const float* ray_dir, const float* targets, int64_t num_src,
                    const int32_t* fg_indices, int64_t num_fg, int64_t n_uniform, int64_t n_fg, uint64_t seed,
                    uint64_t stream, uint64_t counter, float* out_org, float* out_dir, float* out_targets,
                    int32_t* indices_out);

/* ---- hipGraph capture of a training step ----------------------------------- */
/* A step's calls (train step, optimizer) can be captured once in a hipGraph
 * (hipStreamBeginCapture on the context's stream ... hipStreamEndCapture, hipGraphInstantiate)
 * and replayed with hipGraphLaunch. What changes from one step to the next lives on the device:
 *  - the per-step scalars: while an rm_step_scalars record is bound to the context
 *    (rm_bind_step_scalars), rm_train_step[_camera] take progress = min(index / total, 1) in fp32
 *    (train.rs:171-172) instead of their `progress` argument, and rm_optimizer_step[_f16] take
 *    Adam's step from `step` instead of their argument and then advance the record on the device
 *    (step += 1, index += 1) -- the optimizer ends a training step;
 *  - the cost-ordered dispatch rotates its list sets on the device by itself.
 * rm_reserve before the capture keeps every call allocation-free; kernel timing (rm_timing_enable)
 * and rm_train_iteration's one-launch form are not for capture (with a bound record,
 * rm_train_iteration runs its three calls). dev = NULL unbinds; the record is the caller's device
 * memory and must outlive the binding. */
typedef struct rm_step_scalars {
  int32_t step;     /* Adam's step of the next optimizer call (counts from 1) */
  int32_t index;    /* the global step of the next train call ... */
  int32_t total;    /* ... out of total: progress = index / total */
  int32_t reserved;
} rm_step_scalars;
int rm_bind_step_scalars(rm_context* ctx, rm_step_scalars* dev);

/* ---- diagnostics ------------------------------------------------------------ */
/* Per-ray forward intermediates dbg [N][24] = {t, t_final, n.x, n.y, n.z, lighting,
 * mix.r, mix.g, mix.b, D_final, mask, n.l, min delta, Zw, Zb, 0, D(+x), D(-x), D(+y),
 * D(-y), D(+z), D(-z), 0, 0} (renderer_diff.rs
 * stages) for parity debugging against the oracle. Not on the hot path. */
int rm_debug_intermediates(rm_context* ctx, const float* ray_org, const float* ray_dir, int64_t num_rays,
                           const rm_scene* scene, const rm_march* march, float* dbg);

/* Cost-ordered dispatch state (tests): copies the 3 x classes per-class block counts of the
 * three list sets (see RM_MARCH_STATIC_ORDER) into counts[0 .. 3*classes) after synchronising
 * the stream; *classes = the build's class count, *next_set = the set the next keyed launch
 * appends to (it reads set (next_set + 2) % 3, whose total equals the launch's block count
 * when the cost order is used and differs when the launch falls back to the static order).
 * Environment RM_DEBUG_SKIP_ORDER_CLEAR=1 makes a launch leave the next set's counts
 * uncleared (the state a failed launch in the rotation leaves), for the recovery test.
 * The last class's count is the sum of its lists (large launches append it to several; env
 * RM_ORDER_SHARDS=1 / 0: at any size / never). With capacity >= 3*classes + 3*RM_ORDER_SHARDS the
 * lists' own counts follow: counts[3*classes + set*RM_ORDER_SHARDS + list]. */
#define RM_ORDER_SHARDS 4
int rm_debug_order_counts(rm_context* ctx, int32_t* counts, int32_t capacity, int32_t* classes, int32_t* next_set);

/* The tile proof of the escape lattice (tests): after synchronising the stream, copies the bytes the last
 * per-ray launch of a camera call with the lattice read -- one per wave (64 rays; wave w & 3 of ray block
 * w >> 2, an 8x8 pixel quadrant of a 16x16 tile), 1 where the pre-pass proved every ray of the wave gone, 0
 * where it did not -- into host[0 .. min(capacity, waves)); *n_waves = the bytes copied. Only the context's
 * LAST per-ray launch is seen: 0 bytes when that launch took no tile proof (no lattice, row order, a launch
 * below the tile proof's size), and of a call split over several launches the last launch's waves alone. */
int rm_debug_tile_proof(rm_context* ctx, uint8_t* host, int64_t capacity, int64_t* n_waves);

/* Stream stall (tests of a caller's watchdog, e.g. rmh_collective.wait): enqueues on the context's
 * stream one wave that spins until rm_debug_stall_release(ctx) or until max_ms (1 .. 600000) have
 * passed, whichever comes first -- it always ends by itself. rm_destroy releases a pending one. */
int rm_debug_stall(rm_context* ctx, int32_t max_ms);
int rm_debug_stall_release(rm_context* ctx);

/* ---- kernel timing (benchmark instrumentation) ------------------------------ */
/* rm_timing_enable(ctx, 1): every later render / backward / train call records a
 * hipEvent pair around each launch of its main per-ray kernel on the context's
 * stream. rm_timing_collect synchronises those events and returns the summed kernel
 * time in milliseconds and the number of launches (reset != 0 clears the record). */
int rm_timing_enable(rm_context* ctx, int32_t enable);
int rm_timing_collect(rm_context* ctx, double* total_ms, int64_t* launches, int32_t reset);

/* ---- work statistics -------------------------------------------------------- */
/* rm_stats_enable(ctx, 1): count, for every later per-ray launch, the ray blocks (256 rays)
 * launched, those skipped whole by RM_MARCH_SKIP_ESCAPED, and the waves (64 rays) that left
 * the march early because all their rays escaped, with the march steps they saved, and the rays
 * the backward modes' two gradient sweeps ran for (the rays with non-zero seeds: a ray whose
 * seeds are 0 contributes exact zeros and is not swept; the general kernel counts them, the
 * small kernel (M <= 32) reports 0).
 * rm_stats_collect synchronises the stream; reset != 0 clears the counters. */
typedef struct rm_stats {
  int64_t blocks;          /* ray blocks launched */
  int64_t blocks_skipped;  /* blocks skipped by RM_MARCH_SKIP_ESCAPED */
  int64_t waves;           /* waves launched (4 per block) */
  int64_t waves_exited;    /* waves that stopped marching early (all rays escaped) */
  int64_t steps_saved;     /* march steps those waves did not run */
  int64_t seeded_rays;     /* rays the first backward sweep (at p) ran for */
  int64_t seeded_rays_a;   /* rays the second backward sweep (at p_approx) ran for */
} rm_stats;
int rm_stats_enable(rm_context* ctx, int32_t enable);
int rm_stats_collect(rm_context* ctx, rm_stats* out, int32_t reset);

/* ---- model helpers: SceneModel activations, compute_loss penalties, Adam ---- */
/* Packed parameter layout used by the helpers (raw Param tensors or their grads):
 *   [centers 3M | colors 3M | radius M | light_dir 3 | ambient 1]  (7M+4 floats)
 * rm_scene_activate writes the activated values in the same packed layout
 * (scene.rs:41-45) so an rm_scene can point into it (see rm_scene_from_packed). */
int rm_scene_activate(rm_context* ctx, const float* raw_packed, int32_t num_spheres, float* act_packed);
void rm_scene_from_packed(const float* act_packed, int32_t num_spheres, rm_scene* out_scene);
void rm_grads_from_packed(float* grad_packed, int32_t num_spheres, rm_grads* out_grads);

/* Optimizer step on the raw packed params (train.rs:161-198): the activated-space
 * gradient (packed, e.g. all-reduced across ranks) is chained through scene.rs:41-45,
 * the compute_loss parameter penalties (training.rs:38-82) are added when
 * with_penalties != 0, then Burn's Adam (beta1 0.9, beta2 0.999, eps 1e-5) with
 * coupled L2 weight decay `weight_decay` updates raw_packed in place. adam_m and
 * adam_v are (7M+4)-float device buffers (zero them when re-initialising the
 * optimizer, train.rs:160-163); step counts from 1. loss_penalty (nullable, device
 * float) receives the penalty value at the pre-step parameters. act_out (nullable)
 * receives the activated packed parameters of the UPDATED model (what
 * rm_scene_activate would return), so the next render needs no separate launch. */
int rm_optimizer_step(rm_context* ctx, float* raw_packed, const float* grad_act_packed, float* adam_m,
                      float* adam_v, int32_t num_spheres, int32_t step, float lr, float weight_decay,
                      int32_t with_penalties, float* loss_penalty, float* act_out);

/* rm_optimizer_step for fp16-colour models (RM_MARCH_COLOR_F16, BASELINE configs[4]): the
 * same update (fp32 master parameters, moments and gradient), and colors_f16_out (nullable,
 * device, [M,3] IEEE binary16) receives the updated activated colours rounded to nearest --
 * the colour tensor of the next fp16-colour render. */
int rm_optimizer_step_f16(rm_context* ctx, float* raw_packed, const float* grad_act_packed, float* adam_m,
                          float* adam_v, int32_t num_spheres, int32_t step, float lr, float weight_decay,
                          int32_t with_penalties, float* loss_penalty, float* act_out, uint16_t* colors_f16_out);

/* One single-process training step on whole views (train.rs:182-198: model.forward, compute_loss,
 * loss.backward(), optim.step), replacing rm_train_step_camera -> rm_optimizer_step[_f16] with the
 * same arguments and the same results bit for bit:
 *   1. the render of act_packed (activated packed parameters; with RM_MARCH_COLOR_F16 in
 *      march->flags the colours come from colors_f16_out), the loss seed and the backward into
 *      grad_packed ((7M+4) floats, overwritten) and loss_sum (1 float, overwritten), as
 *      rm_train_step_camera with progress and inv_count;
 *   2. the optimizer step on raw_packed / adam_m / adam_v (step, lr, weight_decay,
 *      with_penalties, loss_penalty nullable) writing the updated activated parameters to
 *      act_packed (and, fp16-colour models, their rounded colours to colors_f16_out), as
 *      rm_optimizer_step_f16 with act_out = act_packed.
 * Models of up to 64 spheres run the optimizer inside the call's gradient reduction, in the block
 * that completes the gradient (env RM_FUSED_ADAM=0 turns this off): one launch fewer per step.
 * Otherwise -- more spheres, the small-scene kernel, more than one ray sub-launch -- the two calls
 * run as such. Bound step scalars (rm_bind_step_scalars) apply as to the two calls. Not for
 * data-parallel training: the gradient is consumed before it could be all-reduced. */
int rm_train_step_camera_adam(rm_context* ctx, const rm_camera* cams, int32_t num_views, int32_t width,
                              int32_t height, const float* targets, float progress, float inv_count,
                              const rm_march* march, float* act_packed, float* grad_packed, float* raw_packed,
                              float* adam_m, float* adam_v, int32_t num_spheres, int32_t step, float lr,
                              float weight_decay, int32_t with_penalties, float* loss_sum, float* loss_penalty,
                              uint16_t* colors_f16_out);

/* One step of the reference training loop (train.rs:169-198) for one process, replacing the
 * sequence rm_sample_batch -> rm_train_step -> rm_optimizer_step with the same arguments and
 * the same results bit for bit:
 *   1. the batch: rows drawn from the dataset arrays ray_org / ray_dir / targets ([num_src,3])
 *      as rm_sample_batch draws them (n_uniform + n_fg rows; seed, stream, counter);
 *   2. the render of the scene act_packed (activated packed parameters), the loss seed and the
 *      backward into grad_packed ((7M+4) floats, overwritten) and loss_sum (1 float, overwritten),
 *      as rm_train_step with progress, inv_count and march;
 *   3. the optimizer step on raw_packed / adam_m / adam_v (step, lr, weight_decay,
 *      with_penalties, loss_penalty nullable) writing the updated activated parameters back into
 *      act_packed, as rm_optimizer_step with act_out = act_packed.
 * Models of up to 32 spheres and batches of up to 16,384 rays run as ONE launch (the small-scene
 * kernel draws and gathers its rays, an extra block of the launch runs the optimizer's
 * gradient-independent part beside the ray blocks and the last block applies the update; env
 * RM_FUSED_ITER=0 turns this off); other sizes run the three calls. fp32 colour models only.
 * Not for data-parallel training: the gradient is consumed before it could be all-reduced. */
/* The data-parallel rank's step before its all-reduce (train.rs:179-190 on the rank's share of
 * the batch), replacing the sequence rm_sample_batch -> rm_train_step with the same arguments and
 * the same results bit for bit: the rows drawn from the dataset arrays as rm_sample_batch draws
 * them (n_uniform + n_fg rows; seed, stream, counter), then the render of `scene`, the loss seed
 * and the backward into `grads` and loss_sum (overwritten), as rm_train_step with progress,
 * inv_count and march (accumulate 0, no per-ray output). The gradient is left for the caller's
 * all-reduce and rm_optimizer_step[_f16]. Models of up to 32 spheres and batches of up to 16,384
 * rays run as ONE launch (the small-scene kernel draws and gathers its rays and its last block
 * completes the gradient; env RM_FUSED_ITER=0 turns this off); other sizes run the two calls. */
int rm_train_step_sampled(rm_context* ctx, const float* ray_org, const float* ray_dir, const float* targets,
                          int64_t num_src, const int32_t* fg_indices, int64_t num_fg, int64_t n_uniform,
                          int64_t n_fg, uint64_t seed, uint64_t stream, uint64_t counter, float progress,
                          float inv_count, const rm_scene* scene, const rm_march* march, const rm_grads* grads,
                          float* loss_sum);

/* rm_train_step_sampled, and in the same launch the gradient-independent part of the optimizer
 * step that follows the all-reduce (penalties incl. the repulsion rows, the chain-rule factors,
 * Adam's bias corrections; loss_penalty (nullable) written here) on raw_packed / step /
 * with_penalties: the next rm_optimizer_step on this context with the same raw_packed,
 * num_spheres, step, with_penalties and loss_penalty then runs the update only -- the same bits
 * as without the preparation. The contents of raw_packed (and of the buffers the gradient comes
 * from) must not change between the two calls except through the caller's all-reduce of the
 * gradient: the library cannot see a host copy into raw_packed or a parameter broadcast, and the
 * update would use the factors prepared on the old values. Any other call of this library on the
 * context in between (every render, train, sampling, gather and activation entry point) drops the
 * preparation, as do different arguments: the optimizer step then computes everything itself. Models of
 * up to 32 spheres and batches of up to 16,384 rays (the one-launch case); otherwise it is
 * rm_train_step_sampled. Not with bound step scalars (rm_bind_step_scalars). */
int rm_train_step_sampled_prepared(rm_context* ctx, const float* ray_org, const float* ray_dir, const float* targets,
                                   int64_t num_src, const int32_t* fg_indices, int64_t num_fg, int64_t n_uniform,
                                   int64_t n_fg, uint64_t seed, uint64_t stream, uint64_t counter, float progress,
                                   float inv_count, const rm_scene* scene, const rm_march* march,
                                   const rm_grads* grads, float* loss_sum, const float* raw_packed, int32_t step,
                                   int32_t with_penalties, float* loss_penalty);

int rm_train_iteration(rm_context* ctx, const float* ray_org, const float* ray_dir, const float* targets,
                       int64_t num_src, const int32_t* fg_indices, int64_t num_fg, int64_t n_uniform, int64_t n_fg,
                       uint64_t seed, uint64_t stream, uint64_t counter, float progress, float inv_count,
                       const rm_march* march, float* act_packed, float* grad_packed, float* raw_packed,
                       float* adam_m, float* adam_v, int32_t num_spheres, int32_t step, float lr,
                       float weight_decay, int32_t with_penalties, float* loss_sum, float* loss_penalty);

#ifdef __cplusplus
}
#endif

#endif /* RAYMARCH_H_ */
