// rm_launch.h -- launch orchestration behind the C ABI: what a call is (Geometry, Call,
// RayGradCall), its checks and its KArgs, and the launch sequences of the general kernel (run),
// the small-scene kernel (run_small), the ray-gradient kernel (run_raygrad), the viewer's frame
// render (run_view), the distance-field query (run_sdf), its backward (run_sdf_grad), the view-dependent
// colour's forward and backward (run_sh_forward, run_sh_backward), the image-space loss (run_image_loss) and the
// gradient reduction. Host code only;
// included by rm_kernels.hip after rm_context.h.
#pragma once

namespace {

using namespace rm;

int pad_spheres(int M) { return (M + kSphereAlign - 1) / kSphereAlign * kSphereAlign; }
// column blocks of the reduction at the largest scene (RM_MAX_SPHERES): its arrival counters
constexpr int kRedArrivals = (RM_MAX_SPHERES * 8 + 8 + 255) / 256 * kRedArrStride;

// Ray blocks per per-ray launch: kMaxBlocksPerLaunch, or less with the environment variable
// RM_MAX_BLOCKS_PER_LAUNCH (tests use it to exercise the sub-launch split at small sizes).
long long max_blocks_per_launch() {
  const char* e = std::getenv("RM_MAX_BLOCKS_PER_LAUNCH");
  const long long v = e ? std::atoll(e) : 0;
  return (v >= 1 && v <= kMaxBlocksPerLaunch) ? v : kMaxBlocksPerLaunch;
}

long long rec_floats(int Mpad) { return (long long)Mpad * 8 + 8; }

// March steps after which a split launch hands the blocks still marching to a continuation
// launch: env RM_SPLIT_CONT_STEPS (0 = one launch), else max(32, 3 S / 8) for S >= 64 march steps
// (measured, tools/gpu_env_ab.sh: at 4096 spheres S = 128 step 48 gave -20 %, S = 64 step 32 -8 %;
// at S = 32 any step was slower).
int split_cont_steps(int steps) {
  if (const char* e = std::getenv("RM_SPLIT_CONT_STEPS")) return std::max(0, std::atoi(e));
  return steps >= 64 ? std::max(32, 3 * steps / 8) : 0;
}
// The second continuation (a third launch) from S >= 128: at 3S/4 the blocks still marching are
// dealt out again over the CUs (C5 / C5g with 32-ray groups, three rounds on one box: +2.5 % /
// +3.5 % at 96 of 128 steps, profiles/r06_ab.txt r06r). 0 = none; env RM_SPLIT_CONT2_STEPS.
int split_cont2_steps(int steps) {
  if (const char* e = std::getenv("RM_SPLIT_CONT2_STEPS")) return std::max(0, std::atoi(e));
  return steps >= 128 ? 3 * steps / 4 : 0;
}
// The continuation steps of a split launch, increasing, each < steps: caps[0..n), caps[n] = 0.
// Env RM_SPLIT_CONT_LIST="48,80,112" replaces the rule (up to kMaxCont steps).
constexpr int kMaxCont = 4;
int split_cont_caps(int steps, int (&caps)[kMaxCont + 1]) {
  int n = 0;
  if (const char* e = std::getenv("RM_SPLIT_CONT_LIST")) {
    for (const char* q = e; *q && n < kMaxCont;) {
      const int v = std::atoi(q);
      if (v > 0 && v < steps && (n == 0 || v > caps[n - 1])) caps[n++] = v;
      while (*q && *q != ',') ++q;
      if (*q == ',') ++q;
    }
  } else if (steps >= 128 && !std::getenv("RM_SPLIT_CONT_STEPS") && !std::getenv("RM_SPLIT_CONT2_STEPS")) {
    // ray mode: a continuation costs only the rays still marching, so defer earlier and more
    // often -- 3S/16, 3S/8, 3S/4 (C5g, one box: 24 / 48 / 96 of 128 steps 42.3 Mrays/s against 39.8
    // with 48 / 96 and 40.1 with 32 / 96; 16 / 32 / 64 / 96 42.3; C5 within 1 %, profiles/r07g)
    caps[n++] = 3 * steps / 16;
    caps[n++] = 3 * steps / 8;
    caps[n++] = 3 * steps / 4;
  } else {
    const int c0 = split_cont_steps(steps), c1 = split_cont2_steps(steps);
    if (c0 > 0 && c0 < steps) {
      caps[n++] = c0;
      if (c1 > c0 && c1 < steps) caps[n++] = c1;
    }
  }
  for (int i = n; i <= kMaxCont; ++i) caps[i] = 0;
  return n;
}

size_t ws_need(long long max_rays, int M, int rays_per_block = kBlock) {
  const int Mpad = pad_spheres(M);
  long long blocks = (max_rays + rays_per_block - 1) / rays_per_block;
  blocks = std::min<long long>(blocks, kMaxBlocksPerLaunch);
  const long long rec = rec_floats(Mpad);
  return (size_t)(blocks * rec + (long long)reduce_segs(blocks) * rec + 4096) * sizeof(float);
}

// Workspace of the ray-gradient calls (rm_render_diff_backward_rays / _cameras): the replayed
// march's t for every ray, then one partial row per 256-ray block of every view.
size_t rg_need(long long rays) {
  const long long rows = (rays + kBlock - 1) / kBlock + RM_MAX_VIEWS_PER_CALL;
  return (size_t)(rays + rows * kRgCols + 64) * sizeof(float);
}

// The mode ladder, once: f(std::integral_constant<int, MODE>) for the call's mode.
template <class F>
void with_mode(int mode, F&& f) {
  switch (mode) {
    case kFwd: f(std::integral_constant<int, kFwd>{}); break;
    case kBwd: f(std::integral_constant<int, kBwd>{}); break;
    case kTrain: f(std::integral_constant<int, kTrain>{}); break;
    default: f(std::integral_constant<int, kRender>{}); break;
  }
}

// ---- what a call is --------------------------------------------------------------------------

// The rays of a call -- ray arrays, or cameras whose rays the kernel forms -- and its scene.
struct Geometry {
  bool cam = false;
  const float* org = nullptr;
  const float* dir = nullptr;
  long long n = 0;
  const rm_camera* cams = nullptr;
  int views = 0, W = 0, H = 0;
  const rm_scene* scene = nullptr;
  const rm_march* march = nullptr;
  long long rays() const { return cam ? (long long)views * W * H : n; }
};

Geometry ray_geometry(const float* org, const float* dir, long long n, const rm_scene* scene, const rm_march* march) {
  Geometry g;
  g.org = org;
  g.dir = dir;
  g.n = n;
  g.scene = scene;
  g.march = march;
  return g;
}

Geometry camera_geometry(const rm_camera* cams, int views, int W, int H, const rm_scene* scene, const rm_march* march) {
  Geometry g;
  g.cam = true;
  g.cams = cams;
  g.views = views;
  g.W = W;
  g.H = H;
  g.scene = scene;
  g.march = march;
  return g;
}

struct Call : Geometry {
  int mode;  // Mode
  float* out = nullptr;
  float* t_out = nullptr;
  const float* t_in = nullptr;
  const float* gout = nullptr;
  const float* targets = nullptr;
  float progress = 0.0f, inv_count = 0.0f;
  float* dbg = nullptr;
  const rm_grads* grads = nullptr;
  float* loss_sum = nullptr;
  int accumulate = 0;
  // rm_train_iteration: org / dir / targets are the dataset arrays the kernel draws the batch
  // from, and the optimizer runs in the same launch (rm_small_kernel<kTrain, MB, true>)
  const SmallArgs* fused = nullptr;
  // rm_train_step_camera_adam: the optimizer step on the packed gradient (grads->centers), run by
  // the gradient reduction's last block where it can (rm_context::adam_done says whether it did)
  struct Adam {
    float *raw, *m1, *m2, *act_out, *loss_penalty;
    _Float16* col_h;
    int step, with_pen;
    float lr, wd;
  };
  const Adam* adam = nullptr;
  Call(int mode_, const Geometry& g) : Geometry(g), mode(mode_) {}
  bool has_bwd() const { return mode == kBwd || mode == kTrain; }
};

Call ray_call(int mode, const float* org, const float* dir, long long n, const rm_scene* scene, const rm_march* march) {
  return Call(mode, ray_geometry(org, dir, n, scene, march));
}

Call camera_call(int mode, const rm_camera* cams, int views, int W, int H, const rm_scene* scene,
                 const rm_march* march) {
  return Call(mode, camera_geometry(cams, views, W, H, scene, march));
}

// the training part of a kTrain call
void set_training(Call& c, const float* targets, float progress, float inv_count, const rm_grads* grads,
                  float* loss_sum, int accumulate) {
  c.targets = targets;
  c.progress = progress;
  c.inv_count = inv_count;
  c.grads = grads;
  c.loss_sum = loss_sum;
  c.accumulate = accumulate;
}

struct RayGradCall : Geometry {
  const float* gout = nullptr;
  const float* t_in = nullptr;
  float* g_org = nullptr;
  float* g_dir = nullptr;
  rm_camera* grad_cams = nullptr;
  int accumulate = 0;
  explicit RayGradCall(const Geometry& g) : Geometry(g) {}
};

// ---- call setup shared by run and run_raygrad ------------------------------------------------

int check_scene(rm_context* ctx, const rm_scene* s, bool need_light) {
  if (!s) return fail(ctx, RM_ERR_INVALID_ARG, "scene is NULL");
  if (s->num_spheres < 1 || s->num_spheres > RM_MAX_SPHERES)
    return fail(ctx, RM_ERR_INVALID_ARG, "num_spheres %d out of [1, %d]", s->num_spheres, RM_MAX_SPHERES);
  if (!s->centers || !s->colors || !s->radius || (need_light && (!s->light_dir || !s->ambient)))
    return fail(ctx, RM_ERR_INVALID_ARG, "scene has a NULL parameter pointer");
  return RM_OK;
}

int check_march(rm_context* ctx, const rm_march* m) {
  if (!m) return fail(ctx, RM_ERR_INVALID_ARG, "march is NULL");
  if (m->steps < 0 || m->steps > 100000) return fail(ctx, RM_ERR_INVALID_ARG, "steps %d out of range", m->steps);
  if (!(m->smooth_k > 0.0f) || !std::isfinite(m->smooth_k))
    return fail(ctx, RM_ERR_INVALID_ARG, "smooth_k must be finite and > 0 (got %g)", (double)m->smooth_k);
  if (!(m->normal_eps > 0.0f) || !std::isfinite(m->normal_eps))
    return fail(ctx, RM_ERR_INVALID_ARG, "normal_eps must be finite and > 0 (got %g)", (double)m->normal_eps);
  // the colour sums are shifted by the smallest sphere distance on the premise that no exponent
  // (-csharp (d_j - d_min)) is positive; gone_d / cull_min_d assume a mask that vanishes outward
  if (!(m->color_sharpness >= 0.0f) || !std::isfinite(m->color_sharpness))
    return fail(ctx, RM_ERR_INVALID_ARG, "color_sharpness must be finite and >= 0 (got %g)",
                (double)m->color_sharpness);
  if (!(m->mask_sharpness >= 0.0f) || !std::isfinite(m->mask_sharpness))
    return fail(ctx, RM_ERR_INVALID_ARG, "mask_sharpness must be finite and >= 0 (got %g)",
                (double)m->mask_sharpness);
  return RM_OK;
}

// the scene, the march settings and the cameras or ray arrays of a call
int check_geometry(rm_context* ctx, const Geometry& g, bool need_light) {
  int rc;
  if ((rc = check_scene(ctx, g.scene, need_light)) != RM_OK) return rc;
  if ((rc = check_march(ctx, g.march)) != RM_OK) return rc;
  if (g.cam) {
    if (!g.cams) return fail(ctx, RM_ERR_INVALID_ARG, "cams is NULL");
    if (g.views < 1 || g.views > RM_MAX_VIEWS_PER_CALL)
      return fail(ctx, RM_ERR_INVALID_ARG, "num_views %d out of [1, %d]", g.views, RM_MAX_VIEWS_PER_CALL);
    if (g.W < 1 || g.H < 1 || (long long)g.W * g.H > (1LL << 28))
      return fail(ctx, RM_ERR_INVALID_ARG, "bad image size %dx%d", g.W, g.H);
  } else {
    if (g.n < 0) return fail(ctx, RM_ERR_INVALID_ARG, "num_rays %lld < 0", g.n);
    if (g.n > 0 && (!g.org || !g.dir)) return fail(ctx, RM_ERR_INVALID_ARG, "ray_org/ray_dir is NULL");
  }
  return RM_OK;
}

constexpr float kMinColorSharpness = 1e-12f;

// The scene and march part of a call's KArgs.
void fill_scene_args(const Geometry& g, KArgs& a) {
  a.centers = g.scene->centers;
  if ((g.march->flags & RM_MARCH_COLOR_F16) != 0) {
    a.colors = nullptr;
    a.colors_h = reinterpret_cast<const _Float16*>(g.scene->colors);
  } else {
    a.colors = g.scene->colors;
  }
  a.radius = g.scene->radius;
  a.light_dir = g.scene->light_dir;
  a.ambient = g.scene->ambient;
  a.M = g.scene->num_spheres;
  a.Mpad = pad_spheres(a.M);
  a.steps = g.march->steps;
  a.k = g.march->smooth_k;
  a.eps = g.march->normal_eps;
  // color_sharpness 0 (uniform colour weights) and values next to it: the padding spheres sit at
  // distance ~1e15 (kPadCenter) and leave the colour sums only through 2^(-c log2(e) 1e15) = 0, and
  // the sweeps start from dmin = inf, where (dn - dmin) * 0 is NaN. A sharpness below 1e-12 is
  // raised to it: the real spheres, a few units apart, keep weights 2^(-1e-11) = 1 exactly in fp32,
  // the padding spheres get 2^(-1443) = 0, and the colour term of the gradients is 1e-12 x a finite
  // sum where the exact one is 0.
  a.csharp = std::max(g.march->color_sharpness, kMinColorSharpness);
  a.msharp = g.march->mask_sharpness;
  a.lse_slack = (float)(std::log((double)a.M) / (double)a.k * (1.0 + 1e-6)) + 1e-7f;
  a.rec = rec_floats(a.Mpad);
}

// camera.rs:40-52 on the host, in f32 like the reference.
int make_basis(rm_context* ctx, const rm_camera& c, int W, int H, CamBasis& b) {
  auto normalize = [](const float v[3], float out[3]) {
    const float len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (len == 0.0f) {
      out[0] = out[1] = out[2] = 0.0f;
    } else {
      out[0] = v[0] / len;
      out[1] = v[1] / len;
      out[2] = v[2] / len;
    }
  };
  auto cross = [](const float a[3], const float bb[3], float out[3]) {
    out[0] = a[1] * bb[2] - a[2] * bb[1];
    out[1] = a[2] * bb[0] - a[0] * bb[2];
    out[2] = a[0] * bb[1] - a[1] * bb[0];
  };
  const float up_w[3] = {0.0f, 1.0f, 0.0f};
  const float fr[3] = {c.target[0] - c.eye[0], c.target[1] - c.eye[1], c.target[2] - c.eye[2]};
  float rr[3];
  normalize(fr, b.fwd);
  cross(b.fwd, up_w, rr);
  normalize(rr, b.right);
  cross(b.right, b.fwd, b.up);
  const float aspect = (float)W / (float)H;
  const float rads_per_deg = 3.14159265358979323846f / 180.0f;
  const float theta = c.fov_deg * rads_per_deg / 2.0f;
  b.half_h = std::tan(theta);
  b.half_w = aspect * b.half_h;
  for (int i = 0; i < 3; ++i) b.eye[i] = c.eye[i];
  if (!std::isfinite(b.half_h) || !(c.fov_deg > 0.0f && c.fov_deg < 180.0f))
    return fail(ctx, RM_ERR_INVALID_ARG, "camera fov_deg %g out of (0, 180)", (double)c.fov_deg);
  return RM_OK;
}

// Camera bases of a call with more than kInlineCams views: built on the host (make_basis), staged
// in one of kCamRing pinned slots and copied to the context's device table on its stream (the
// copy is ordered after the previous call's kernels, so one device table serves every call; a
// pinned slot is rewritten only after its previous copy has run).
int upload_cams(rm_context* ctx, const Geometry& c, KArgs& a) {
  int rc;
  if ((rc = ctx->cams_dev.ensure(ctx, sizeof(CamBasis) * RM_MAX_VIEWS_PER_CALL, "camera table")) != RM_OK) return rc;
  if (!ctx->cams_pin) {
    if (hipHostMalloc(&ctx->cams_pin, sizeof(CamBasis) * RM_MAX_VIEWS_PER_CALL * kCamRing) != hipSuccess)
      return fail(ctx, RM_ERR_OOM, "camera staging");
    for (hipEvent_t& e : ctx->cam_ev) RM_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  CamBasis* table = ctx->cams_dev.as<CamBasis>();
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  RM_HIP(ctx, hipStreamIsCapturing(ctx->stream, &cap));
  if (cap != hipStreamCaptureStatusNone) {
    // under hipGraph capture nothing may wait or stage: the call must find its views in the device
    // table already -- an eager call with the same views on this context uploaded them -- and the
    // replays read that table (the caller keeps it: no call with other views on this context)
    std::vector<CamBasis> want(c.views);
    for (int v = 0; v < c.views; ++v)
      if ((rc = make_basis(ctx, c.cams[v], c.W, c.H, want[v])) != RM_OK) return rc;
    if (ctx->cams_shadow.size() != want.size() ||
        std::memcmp(ctx->cams_shadow.data(), want.data(), sizeof(CamBasis) * want.size()) != 0)
      return fail(ctx, RM_ERR_UNSUPPORTED,
                  "a captured call of %d views reads the context's camera table: run the same call once before "
                  "the capture", c.views);
    a.cams_dev = table;
    return RM_OK;
  }
  const int slot = ctx->cam_slot;
  ctx->cam_slot = (slot + 1) % kCamRing;
  RM_HIP(ctx, hipEventSynchronize(ctx->cam_ev[slot]));
  CamBasis* pin = ctx->cams_pin + (size_t)slot * RM_MAX_VIEWS_PER_CALL;
  for (int v = 0; v < c.views; ++v)
    if ((rc = make_basis(ctx, c.cams[v], c.W, c.H, pin[v])) != RM_OK) return rc;
  RM_HIP(ctx, hipMemcpyAsync(table, pin, sizeof(CamBasis) * c.views, hipMemcpyHostToDevice, ctx->stream));
  RM_HIP(ctx, hipEventRecord(ctx->cam_ev[slot], ctx->stream));
  ctx->cams_shadow.assign(pin, pin + c.views);
  a.cams_dev = table;
  return RM_OK;
}

// The rays of a call's KArgs: the ray arrays, or the camera bases (inline up to kInlineCams views,
// else the context's device table), the image size and the pixel tiling.
int fill_camera_args(rm_context* ctx, const Geometry& g, KArgs& a) {
  a.org = g.org;
  a.dir = g.dir;
  if (!g.cam) return RM_OK;
  int rc;
  a.cams_dev = nullptr;
  if (g.views <= kInlineCams) {
    for (int v = 0; v < g.views; ++v)
      if ((rc = make_basis(ctx, g.cams[v], g.W, g.H, a.cams[v])) != RM_OK) return rc;
  } else if ((rc = upload_cams(ctx, g, a)) != RM_OK) {
    return rc;
  }
  a.width = g.W;
  a.height = g.H;
  a.num_views = g.views;
  // Compact 16x16 tiles per block (8x8 per wave): more waves whose rays all miss the scene
  // leave the march early (68 % vs 62 % of waves at the metric view, +3-4 %).
  a.tiling = (g.W % 16 == 0 && g.H % 16 == 0 && (g.march->flags & RM_MARCH_ROW_ORDER) == 0) ? 2 : 0;
  return RM_OK;
}

// Sphere records of this call (rm_prep_kernel; fp16 colours are widened there): read by every
// sweep through scalar loads. origin (camera mode): also the per-view first march step at the
// eye, shared by every ray of the view (rm_origin_kernel); a.origin is set before the record
// kernels, which take the whole KArgs.
int prepare_records(rm_context* ctx, KArgs& a, bool origin) {
  const RecLayout lay(a.Mpad);
  const int nprep = lay.nprep();
  int rc;
  if ((rc = ctx->rec.ensure(ctx, lay.bytes(), "record buffer")) != RM_OK) return rc;
  char* rec = ctx->rec.as<char>();
  a.origin = origin ? RecLayout::at<float>(rec, lay.origin(RecTail::kD0)) : nullptr;
  hipLaunchKernelGGL(rm_prep_kernel, dim3(nprep), dim3(256), 0, ctx->stream, a, (float4*)rec);
  RM_HIP(ctx, hipGetLastError());
  if (nprep > 1) {
    hipLaunchKernelGGL(rm_prep_finish, dim3(1), dim3(256), 0, ctx->stream, a, RecLayout::at<float>(rec, lay.header()),
                       RecLayout::at<float>(rec, lay.esc()), nprep);
    RM_HIP(ctx, hipGetLastError());
  }
  if (origin) {
    if (a.split)
      hipLaunchKernelGGL(rm_origin_kernel<true>, dim3(a.num_views), dim3(64 * kSplitWaves), 0, ctx->stream, a,
                         (const float4*)rec, nprep);
    else
      hipLaunchKernelGGL(rm_origin_kernel<false>, dim3(a.num_views), dim3(64), 0, ctx->stream, a, (const float4*)rec,
                         nprep);
    RM_HIP(ctx, hipGetLastError());
  }
  a.rec_buf = (const float4*)rec;
  return RM_OK;
}

// ---- the escape proof ------------------------------------------------------------------------
// The host's side of the escape proof (rm_proof.h; bound_proof in rm_ray.h, rm_tile_proof_kernel in rm_sdf.h):
// which tier a call runs (proof_tier, once per call), its two context buffers (ensure_proof_buffers), the
// call's lattice (prepare_records_and_lattice) and the tile proof of a launch (tile_proof_policy, tile_proof).
// On the call's stream, in this order: records, origin step, lattice fill; then per launch the tile proof and
// the per-ray launch that reads it.
constexpr size_t kLatticeCells = (size_t)kLatticeN * kLatticeN * kLatticeN;
// The escape lattice costs a call one rm_lattice_kernel launch (kLatticeN^3 M evaluations, about 24 us at
// 256 spheres) whatever its size, and saves in proportion to its rays. Measured on the bench scene, 512x512
// views of 256 spheres, lattice against soft ball alone (profiles/r19_escape_lattice_ab.txt): 80 views
// +12.7 %, 10 views +10 %, 4 views +4.5 %, 2 views -1 % (inside the noise), 1 view -5 %, a 256x256 view
// -11 %. Camera calls below kLatticeMinRays rays (4 views of 512x512) keep the soft ball alone.
constexpr long long kLatticeMinRays = 1048576;
// The tile proof needs the 16x16 tiling -- in rows order a wave's 64 rays are no pixel rectangle and have no
// narrow cone -- and a launch large enough to pay for it: one lane per tile, each a chain of up to `steps`
// dependent bound steps of about 0.4 us, it takes 26 us at 10 views of 512x512 and 32 steps however few tiles
// there are, and 42 us at 80 views. Measured against the per-ray lookup (profiles/r20_tile_proof_ab.txt): 80
// views +3.8 %, 10 views a tie at 32 steps and -0.6 to -0.9 % at 64 steps. Launches below kTileProofMinRays
// rays (20 views of 512x512) keep the per-ray lookup.
constexpr long long kTileProofMinRays = 5242880;

// What a call runs of the proof: KArgs::proof, and whether env RM_PROOF_LATTICE=1 asked for the lattice.
struct ProofTier {
  enum { kNone = 0, kBall = 1, kLattice = 2 };
  int tier;
  bool forced;  // the lattice at any call size, and the tile proof at any launch size
};
// The proof at all: the unsplit training kernels with the exit on (hence no per-ray t and no debug output),
// from kProofMinSpheres spheres on. With the call's escape lattice: camera calls of at least kLatticeMinRays
// rays; env RM_PROOF_LATTICE=0 never, =1 at any size (read once per call, as RM_SPLIT). Other calls keep the
// soft ball alone.
ProofTier proof_tier(bool early_exit, bool split, int mode, int Mpad, bool cam, long long rays) {
  if (!early_exit || split || mode == kRender || Mpad < kProofMinSpheres) return {ProofTier::kNone, false};
  if (!cam) return {ProofTier::kBall, false};
  const char* e = std::getenv("RM_PROOF_LATTICE");
  const bool never = e && e[0] == '0', forced = e && e[0] == '1';
  if (never || !(rays >= kLatticeMinRays || forced)) return {ProofTier::kBall, false};
  return {ProofTier::kLattice, forced};
}

// The lattice (kLatticeN^3 floats) and the tile-proof bytes (one per wave of the largest launch) of a context.
int ensure_proof_buffers(rm_context* ctx) {
  int rc;
  if ((rc = ctx->lattice.ensure(ctx, sizeof(float) * kLatticeCells, "escape lattice")) != RM_OK) return rc;
  return ctx->tile_proof.ensure(ctx, (size_t)kMaxBlocksPerLaunch * kWaves, "tile proof");
}

// The call's escape lattice (KArgs::lattice; rm_tile_proof_kernel or bound_proof reads it): the soft-min at the
// kLatticeN^3 cell centres the record kernel laid out, by the distance-only lattice sweep of
// rm_sdf_grid. Once per call, after the record kernels and before the per-ray launches, on the call's
// stream: the scene changes with every optimizer step, so nothing of it is kept across calls.
int fill_lattice(rm_context* ctx, const KArgs& a) {
  SdfArgs s;
  std::memset(&s, 0, sizeof s);
  s.rec_buf = a.rec_buf;
  s.Mpad = a.Mpad;
  s.kappa = a.k * kLog2e;
  s.n = (long long)kLatticeCells;
  s.nx = kLatticeN;
  s.ny = kLatticeN;
  s.dist = const_cast<float*>(a.lattice);
  s.geom = RecLayout::at<const float>(a.rec_buf, RecLayout(a.Mpad).lattice());
  static_assert(kLatticeCells % kBlock == 0 && kLatticeCells / kBlock <= kMaxBlocksPerLaunch, "one launch");
  hipLaunchKernelGGL(rm_lattice_kernel, dim3((unsigned)(kLatticeCells / kBlock)), dim3(kBlock), 0, ctx->stream, s);
  RM_HIP(ctx, hipGetLastError());
  return RM_OK;
}

// The records of a call (prepare_records) and, at the lattice tier, its lattice. KArgs::lattice is bound before
// the record kernel, which lays the lattice out only for a call that has one (write_bound); the fill follows.
int prepare_records_and_lattice(rm_context* ctx, KArgs& a, bool origin, const ProofTier& proof) {
  int rc;
  if (proof.tier == ProofTier::kLattice) {
    if ((rc = ensure_proof_buffers(ctx)) != RM_OK) return rc;
    a.lattice = ctx->lattice.as<float>();
  }
  if ((rc = prepare_records(ctx, a, origin)) != RM_OK) return rc;
  return a.lattice != nullptr ? fill_lattice(ctx, a) : RM_OK;
}

// Where a launch of a call with the lattice reads it: in the tile proof before the launch (true) or per ray
// inside bound_proof (false; rm_ray.h): tiled launches of at least kTileProofMinRays rays (the measurements
// above), or of any size when the call's lattice was forced. Either way the same waves' results: what a proof
// tries changes none.
bool tile_proof_policy(const KArgs& a, const ProofTier& proof, long long nr) {
  return proof.tier == ProofTier::kLattice && a.tiling == 2 && (nr >= kTileProofMinRays || proof.forced);
}

// Whether a cost-ordered launch of nb blocks shards its last cost class over kOrderShards lists (the high half
// of KArgs::order_views, order_append): from kOrderShardMinBlocks blocks on (20 views of 512x512, the tile proof's
// threshold); env RM_ORDER_SHARDS=0 never, =1 at any size (read once per call). Measured against one list
// (profiles/r27_order_shards.txt): 80 views +0.6 to +0.8 %, 10 views a tie either way; a launch below the threshold
// appends to one list and looks its position up in the first kOrderClasses lists alone, as before the shards.
constexpr long long kOrderShardMinBlocks = 20480;
int order_shard_policy(long long nb) {
  const char* e = std::getenv("RM_ORDER_SHARDS");
  const bool never = e && e[0] == '0', forced = e && e[0] == '1';
  return !never && (nb >= kOrderShardMinBlocks || forced) ? kOrderShards - 1 : 0;
}

// The tile proof of one per-ray launch of nb blocks and nr rays (KArgs::tile_proof; rm_tile_proof_kernel), where
// the policy takes it: a byte per wave of the launch, written on the call's stream after the lattice and the
// origin kernel and before the per-ray launch, which reads it. Nothing of it is kept: every launch writes all
// of its bytes, inside a captured graph as outside, and a launch without the tile proof leaves none
// (rm_debug_tile_proof).
int tile_proof(rm_context* ctx, KArgs& a, const ProofTier& proof, long long nb, long long nr) {
  a.tile_proof = nullptr;
  ctx->tile_proof_n = 0;
  if (nb <= 0 || !tile_proof_policy(a, proof, nr)) return RM_OK;
  unsigned char* taken = ctx->tile_proof.as<unsigned char>();  // ensure_proof_buffers, with the call's lattice
  const long long n_tiles = nb * kWaves;
  hipLaunchKernelGGL(rm_tile_proof_kernel, dim3((unsigned)((n_tiles + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream,
                     a, taken, n_tiles);
  RM_HIP(ctx, hipGetLastError());
  ctx->tile_proof_n = n_tiles;
  a.tile_proof = taken;
  return RM_OK;
}

// ---- the gradient reduction ------------------------------------------------------------------

FinalArgs final_args(const Call& c, bool first) {
  const rm_grads* gp = c.grads;
  FinalArgs fa{};
  fa.light_dir = c.scene->light_dir;
  fa.gc = gp->centers;
  fa.gcol = gp->colors;
  fa.gr = gp->radius;
  fa.gld = gp->light_dir;
  fa.gamb = gp->ambient;
  fa.loss_sum = c.mode == kTrain ? c.loss_sum : nullptr;
  fa.accumulate = first ? c.accumulate : 1;
  fa.oturn = nullptr;
  return fa;
}

// The fixed-order cross-block reduction of a launch's nb partial records (a.partials) and the
// gradient scatter into the caller's layout (rm_reduce_partials + rm_finalize_grads).
int reduce_and_finalize(rm_context* ctx, const Call& c, const KArgs& a, long long nb, bool first, bool only = false) {
  FinalArgs fa = final_args(c, first);
  fa.oturn = const_cast<int*>(a.oturn);  // a keyed launch: its reduction advances the turn
  const int nblocks = (int)nb;
  const int ncols = a.Mpad * 8 + 8;
  float* S = a.partials + (long long)std::max<long long>(nb, 1) * a.rec;
  const int segs = reduce_segs(nblocks);  // every segment is written (empty ones as 0)
  const int seg_len = (nblocks + segs - 1) / segs;
  // pass 1 compacts a segment's rows in one 256-entry list (rm_reduce_partials)
  if (seg_len > 256) return fail(ctx, RM_ERR_INVALID_ARG, "%d ray blocks in one launch", nblocks);
  const int xblocks = (ncols + 255) / 256;
  int rc;
  // pass 2 in the same launch (the last-arriving segment block of each column block) unless
  // RM_REDUCE_FUSED=0 (then rm_finalize_grads: the same bits)
  const bool fused = !env_is("RM_REDUCE_FUSED", '0');
  if (fused && (rc = ctx->red_arrivals.ensure(ctx, sizeof(unsigned) * kRedArrivals, "reduction counters", true)) != RM_OK)
    return rc;
  // rm_train_step_camera_adam: the optimizer in the reduction's last block (one launch, the only
  // one of the call, M <= kOptSmallMaxM, the fused reduction)
  if (c.adam != nullptr && only && fused && a.M <= kOptSmallMaxM && !env_is("RM_OPT_SMALL", '0') &&
      !env_is("RM_FUSED_ADAM", '0')) {
    if ((rc = ctx->opt_arrival.ensure(ctx, 128, "optimizer counter", true)) != RM_OK) return rc;
    fa.raw = c.adam->raw;
    fa.m1 = c.adam->m1;
    fa.m2 = c.adam->m2;
    fa.act_out = c.adam->act_out;
    fa.loss_penalty = c.adam->loss_penalty;
    fa.col_h = c.adam->col_h;
    fa.sdev = ctx->sdev;
    fa.opt_arrival = ctx->opt_arrival.as<unsigned>();
    fa.step = c.adam->step;
    fa.with_pen = c.adam->with_pen;
    fa.lr = c.adam->lr;
    fa.wd = c.adam->wd;
    ctx->adam_done = true;
  }
  hipLaunchKernelGGL(rm_reduce_partials, dim3((unsigned)xblocks, (unsigned)segs), dim3(256), 0, ctx->stream, a.partials,
                     a.rec, a.M, a.Mpad, nblocks, seg_len, S, fa, fused ? ctx->red_arrivals.as<unsigned>() : nullptr);
  RM_HIP(ctx, hipGetLastError());
  if (!fused) {
    hipLaunchKernelGGL(rm_finalize_grads, dim3((unsigned)((ncols + 63) / 64)), dim3(256), 0, ctx->stream, S, segs, a.M,
                       a.Mpad, final_args(c, first));
    RM_HIP(ctx, hipGetLastError());
  }
  return RM_OK;
}

// Per-launch timing events (rm_timing_enable): the next pair of the context's pool.
int next_events(rm_context* ctx, hipEvent_t& ev0, hipEvent_t& ev1) {
  ev0 = ev1 = nullptr;
  if (!ctx->timing) return RM_OK;
  if (ctx->events_used == ctx->events.size()) {
    std::pair<hipEvent_t, hipEvent_t> pr;
    RM_HIP(ctx, hipEventCreate(&pr.first));
    RM_HIP(ctx, hipEventCreate(&pr.second));
    ctx->events.push_back(pr);
  }
  ev0 = ctx->events[ctx->events_used].first;
  ev1 = ctx->events[ctx->events_used].second;
  ++ctx->events_used;
  return RM_OK;
}

#ifdef RM_BLOCK_TRACE
// measurement build: the per-wave records of the launch about to run, `waves` of them
int bind_block_trace(rm_context* ctx, KArgs& a, long long waves) {
  int rc = ctx->btrace.ensure(ctx, sizeof(unsigned long long) * kTraceWords * kWaves * (size_t)kMaxBlocksPerLaunch,
                              "block trace");
  if (rc != RM_OK) return rc;
  a.btrace = ctx->btrace.as<unsigned long long>();
  ctx->btrace_waves = waves;
  return RM_OK;
}
#endif

// ---- the small-scene kernel ------------------------------------------------------------------

// Small scenes (M <= kSmallMaxM): rm_small_kernel. Taken by default for ray-array calls (the
// reference training loop's random batches, train.rs:169-199) and for camera calls of up to
// kSmallCamMaxRays rays (64x64 / 16 steps: 13.5 vs 56 us, 256x256 / 40 steps: 25 vs 84 us;
// tools/small_batch_sweep.py -- larger camera calls keep the general kernel's exact early exits);
// env RM_SMALL=1 takes it for every eligible call, RM_SMALL=0 never. Not for the renderer.rs
// mode, the diagnostics or the flags that select the general kernel's march paths for testing.
constexpr long long kSmallCamMaxRays = 1LL << 20;
bool use_small(const Call& c, int M, long long n) {
  if (M > kSmallMaxM || n <= 0 || c.mode == kRender || c.dbg) return false;
  if ((c.march->flags & (RM_MARCH_VALU_ONLY | RM_MARCH_FORCE_MAX_SHIFT | RM_MARCH_SPLIT | RM_MARCH_PER_RAY_ORIGIN |
                         RM_MARCH_SKIP_ESCAPED)) != 0)
    return false;
  const char* e = std::getenv("RM_SMALL");
  if (e && e[0] == '0') return false;
  if (e && e[0] == '1') return true;
  return !c.cam || n <= kSmallCamMaxRays;
}

// rm_small_kernel for M spheres: the bucket of M rounded up to a multiple of 4
template <int MODE, bool FUSED = false, int LPR = 1>
void launch_small_m(int M, dim3 grid, hipStream_t st, const KArgs& a, const SmallArgs& sa, hipEvent_t ev0,
                    hipEvent_t ev1) {
  const dim3 blk(kBlock);
  switch ((M + 3) / 4) {
#define RM_SMALL_CASE(C, MB) \
  case C: hipExtLaunchKernelGGL((rm_small_kernel<MODE, MB, FUSED, LPR>), grid, blk, 0, st, ev0, ev1, 0u, a, sa); break;
    RM_SMALL_CASE(1, 4)
    RM_SMALL_CASE(2, 8)
    RM_SMALL_CASE(3, 12)
    RM_SMALL_CASE(4, 16)
    RM_SMALL_CASE(5, 20)
    RM_SMALL_CASE(6, 24)
    RM_SMALL_CASE(7, 28)
#undef RM_SMALL_CASE
    default: hipExtLaunchKernelGGL((rm_small_kernel<MODE, 32, FUSED, LPR>), grid, blk, 0, st, ev0, ev1, 0u, a, sa); break;
  }
}

// Lanes per ray of a small-kernel call: train steps of up to 32,768 rays split each ray's march
// over two lanes (rm_small.h, LPR; 16,384 rays: 18.6 vs 19.7 us, 4,096: 15.9 vs 19.2; from
// 65,536 rays the SIMDs are full and one lane per ray is faster, 25.6 vs 28.7). Env
// RM_SMALL_LPR=1 / 2 forces one or two.
int small_lpr(const Call& c, long long n) {
  if (c.mode != kTrain || env_is("RM_SMALL_LPR", '1')) return 1;
  return env_is("RM_SMALL_LPR", '2') || n <= 32768 ? 2 : 1;
}

int run_small(rm_context* ctx, const Call& c, KArgs& a, long long n) {
  const bool has_bwd = c.has_bwd();
  const int lpr = small_lpr(c, n), rpb = kBlock / lpr;
  int rc;
  if (has_bwd && (rc = ctx->ws.ensure(ctx, ws_need(n, a.M, rpb), "workspace")) != RM_OK) return rc;
  if ((rc = ctx->arrivals.ensure(ctx, 64, "arrival counter", true)) != RM_OK) return rc;
  long long done = 0;
  bool first = true;
  while (done < n) {
    const long long nb = std::min<long long>((n - done + rpb - 1) / rpb, max_blocks_per_launch());
    const long long nr = std::min<long long>(n - done, nb * rpb);
    a.ray_begin = done;
    a.n_rays = nr;
    a.partials = ctx->ws.as<float>();
#ifdef RM_BLOCK_TRACE
    if ((rc = bind_block_trace(ctx, a, (nb + (c.fused && c.fused->adam ? 1 : 0)) * kWaves)) != RM_OK) return rc;
    RM_HIP(ctx, hipMemsetAsync(a.btrace, 0, sizeof(unsigned long long) * kTraceWords * kWaves * (size_t)(nb + 1), ctx->stream));
#endif
    SmallArgs sa;
    std::memset(&sa, 0, sizeof sa);
    if (c.fused) sa = *c.fused;
    if (has_bwd) sa.fin = final_args(c, first);
    sa.arrivals = ctx->arrivals.as<unsigned>();
    sa.final_in_kernel = has_bwd && nb <= kSmallFinalMaxBlocks ? 1 : 0;
    if (c.fused && (!sa.final_in_kernel || nr != n))  // rm_train_iteration / _step_sampled checked this
      return fail(ctx, RM_ERR_INVALID_ARG, "fused iteration needs one launch of <= %d blocks", kSmallFinalMaxBlocks);
    const bool extra = c.fused && sa.adam;  // the launch's extra (optimizer) block
    if (ctx->stats_dev) {
      ctx->stats_blocks += nb;
      ctx->stats_waves += nb * kWaves;
    }
    if (extra) {  // the extra block's optimizer part (rm_small.h)
      if ((rc = ctx->opt_pre.ensure(ctx, sizeof(float) * (4 * kOptPreStride + 2), "optimizer hand-off")) != RM_OK)
        return rc;
      sa.opt_pre = ctx->opt_pre.as<float>();
      ctx->opt_prepared = false;  // a preparing call records its arguments after the launch
    }
    hipEvent_t ev0, ev1;
    if ((rc = next_events(ctx, ev0, ev1)) != RM_OK) return rc;
    const dim3 grid((unsigned)(nb + (extra ? 1 : 0)));
    if (c.fused && lpr == 2) launch_small_m<kTrain, true, 2>(a.M, grid, ctx->stream, a, sa, ev0, ev1);
    else if (c.fused) launch_small_m<kTrain, true>(a.M, grid, ctx->stream, a, sa, ev0, ev1);
    else if (c.mode == kFwd) launch_small_m<kFwd>(a.M, grid, ctx->stream, a, sa, ev0, ev1);
    else if (c.mode == kBwd) launch_small_m<kBwd>(a.M, grid, ctx->stream, a, sa, ev0, ev1);
    else if (lpr == 2) launch_small_m<kTrain, false, 2>(a.M, grid, ctx->stream, a, sa, ev0, ev1);
    else launch_small_m<kTrain>(a.M, grid, ctx->stream, a, sa, ev0, ev1);
    RM_HIP(ctx, hipGetLastError());
    if (has_bwd && !sa.final_in_kernel && (rc = reduce_and_finalize(ctx, c, a, nb, first)) != RM_OK) return rc;
    done += nr;
    first = false;
  }
  return RM_OK;
}

// ---- the general kernel ----------------------------------------------------------------------

template <int MODE>
void launch_escape(bool cam, dim3 grid, hipStream_t st, const KArgs& a, int* flags) {
  if (cam)
    hipLaunchKernelGGL((rm_escape_kernel<MODE, true>), grid, dim3(kBlock), 0, st, a, flags);
  else
    hipLaunchKernelGGL((rm_escape_kernel<MODE, false>), grid, dim3(kBlock), 0, st, a, flags);
}

// Launches the per-ray kernel; false for a combination that is not built: the renderer.rs mode
// never takes the split march (march_policy).
template <int MODE>
bool launch_ray(bool cam, bool split, dim3 grid, size_t lds, hipStream_t st, const KArgs& a, hipEvent_t ev0,
                hipEvent_t ev1) {
  // With timing on, the start/stop timestamps come from the kernel's own dispatch packet
  // (hipExtLaunchKernel): no extra barrier packets or cache flushes around the launch.
  const dim3 blk(split ? 64 * kSplitWaves : kBlock);
  const uint32_t sh = (uint32_t)lds;
  if (split) {
    if constexpr (MODE == kRender) {
      return false;
    } else {
      if (cam) hipExtLaunchKernelGGL((rm_ray_kernel<MODE, true, true>), grid, blk, sh, st, ev0, ev1, 0u, a);
      else hipExtLaunchKernelGGL((rm_ray_kernel<MODE, false, true>), grid, blk, sh, st, ev0, ev1, 0u, a);
    }
  } else {
    if constexpr (MODE != kRender) {
      if (a.proof) {
        if (cam) hipExtLaunchKernelGGL((rm_ray_kernel<MODE, true, false, true>), grid, blk, sh, st, ev0, ev1, 0u, a);
        else hipExtLaunchKernelGGL((rm_ray_kernel<MODE, false, false, true>), grid, blk, sh, st, ev0, ev1, 0u, a);
        return true;
      }
    }
    if (cam) hipExtLaunchKernelGGL((rm_ray_kernel<MODE, true, false>), grid, blk, sh, st, ev0, ev1, 0u, a);
    else hipExtLaunchKernelGGL((rm_ray_kernel<MODE, false, false>), grid, blk, sh, st, ev0, ev1, 0u, a);
  }
  return true;
}

// The call's outputs and inputs against its mode.
int check_call(rm_context* ctx, const Call& c, long long n) {
  if ((c.mode == kFwd || c.mode == kRender) && n > 0 && !c.out && !c.t_out && !c.dbg) return fail(ctx, RM_ERR_INVALID_ARG, "no output requested");
  if (c.mode == kBwd && n > 0 && !c.gout) return fail(ctx, RM_ERR_INVALID_ARG, "grad_out is NULL");
  if (c.mode == kTrain && n > 0 && !c.targets) return fail(ctx, RM_ERR_INVALID_ARG, "targets is NULL");
  if (c.has_bwd() && !c.grads) return fail(ctx, RM_ERR_INVALID_ARG, "grads is NULL");
  return RM_OK;
}

// How the call marches, into KArgs: the split march, the escape pre-pass, the early exit, the escape proof's
// tier (also handed back: `proof`) and the flags that select march paths. Returns whether the call takes the
// split march.
bool march_policy(const Call& c, long long n, KArgs& a, ProofTier& proof) {
  const int M = a.M;
  // Escape skipping needs the mask to be exactly 0 at the certified distance: sigmoid(-msharp D)
  // once msharp log2(e) D > 128 overflows exp2 (use 160), exp(-10 D^2) in kRender long before 50.
  const bool mask_vanishes = c.mode == kRender || a.msharp > 0.0f;
  // Split march (RM_MARCH_SPLIT): forced by the flag or env RM_SPLIT=1, automatic by sphere count
  // and rays per launch (kSplitMinSpheres / kSplitMaxRays, kSplitMinSpheresWide / ...Wide); never with
  // RM_MARCH_NO_SPLIT / env RM_SPLIT=0, in the renderer.rs mode or with the escape pre-pass.
  bool split = false;
  if (c.mode != kRender && (c.march->flags & RM_MARCH_SKIP_ESCAPED) == 0) {
    const char* e = std::getenv("RM_SPLIT");
    if ((c.march->flags & RM_MARCH_SPLIT) != 0 || (e && e[0] == '1')) split = true;
    else if ((c.march->flags & RM_MARCH_NO_SPLIT) == 0 && !(e && e[0] == '0'))
      split = (M >= kSplitMinSpheres && n <= kSplitMaxRays) || (M >= kSplitMinSpheresWide && n <= kSplitMaxRaysWide);
  }
  // every split launch runs in ray mode (the scene-uniform shift, per-ray retirement and the
  // ray-level continuation: the split kernels are compiled for it, see KArgs::cont_cap)
  a.split = split ? 1 : 0;
  a.cull = ((c.march->flags & RM_MARCH_SKIP_ESCAPED) != 0 && mask_vanishes && !c.t_out && !c.dbg && !split) ? 1 : 0;
  a.cull_min_d = c.mode == kRender ? 50.0f : std::max(50.0f, 160.0f / (a.msharp * 1.44269504f));
  // Escaped-ray early exit: the mask must be exactly 0 at distance gone_d -- exp2 of
  // msharp log2(e) D overflows at 128 (use 130; the reference's sigmoid(-15 D) is 0 from 5.92);
  // exp(-10 D^2) underflows long before 6.
  // Gone rays (the march) in every mode but the diagnostics; the exit itself not when the march t
  // of every ray is requested (t_out) or with RM_MARCH_NO_EARLY_EXIT.
  a.gone_d = 0.0f;
  if (!c.dbg) {
    if (c.mode == kRender) a.gone_d = 6.0f;
    else if (a.msharp > 0.0f) a.gone_d = std::max(6.0f, 130.0f / (a.msharp * 1.44269504f));
  }
  a.early_exit = a.gone_d > 0.0f && (c.march->flags & RM_MARCH_NO_EARLY_EXIT) == 0 && !c.t_out ? 1 : 0;
  proof = proof_tier(a.early_exit != 0, split, c.mode, a.Mpad, c.cam, n);
  a.proof = proof.tier;
  a.mfma = (c.march->flags & RM_MARCH_VALU_ONLY) == 0;
  a.shift_max = (c.march->flags & RM_MARCH_FORCE_MAX_SHIFT) != 0;
  if (c.mode == kRender) {  // renderer.rs:27-32, normalised in f32 on the host like the reference
    const float lv[3] = {-0.5f, 0.5f, -1.0f};
    const float len = std::sqrt(lv[0] * lv[0] + lv[1] * lv[1] + lv[2] * lv[2]);
    for (int i = 0; i < 3; ++i) a.light_fixed[i] = lv[i] / len;
  }
  return split;
}

// Centre-out dispatch order of the ray blocks of a view's tx x ty 16x16 tiles (ray_block): by
// distance of the block's pixel-centre from the image centre, ties by block index. A block is a
// whole tile (256-ray blocks) or one of its four 8x8 quadrants (64-ray blocks: the split march), in
// the pixel order of setup_ray. Built once per tiling (tx, ty, sub) and context, each in a table of its own
// that nothing rewrites (BlockOrder): calls of different image sizes or block sizes alternate on one context
// without a launch in flight, or a captured one, ever reading another tiling's order.
int ensure_block_order(rm_context* ctx, int tx, int ty, int sub, const int** table) {
  for (const BlockOrder& o : ctx->block_orders)
    if (o.tx == tx && o.ty == ty && o.sub == sub) {
      *table = o.table.as<int>();
      return RM_OK;
    }
  // sub = ray blocks per 16x16 tile: 1 (256-ray blocks), 4 (8x8 quadrants: 64-ray split blocks),
  // 8 (8x4 halves of the quadrants: 32-ray split blocks) or 16 (8x2 quarters: 16-ray split blocks)
  std::vector<int> ord((size_t)tx * ty * sub);
  for (size_t i = 0; i < ord.size(); ++i) ord[i] = (int)i;
  auto key = [&](int i) {  // twice the pixel offset of the block centre from the image centre
    const int tile = i / sub, q = i % sub;
    const int per_quad = sub / 4, quad = sub == 1 ? 0 : q / per_quad, part = sub == 1 ? 0 : q % per_quad;
    const long long rows = sub == 1 ? 16 : 8 / per_quad;  // pixel rows of one block inside its quadrant
    const long long ox = sub == 1 ? 16 : 16 * (quad & 1) + 8,
                    oy = sub == 1 ? 16 : 16 * (quad >> 1) + 2 * rows * part + rows;
    const long long dx = 32LL * (tile % tx) + ox - 16LL * tx, dy = 32LL * (tile / tx) + oy - 16LL * ty;
    return dx * dx + dy * dy;
  };
  std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return key(x) < key(y); });
  // a new table: no launch knows its address yet, so nothing is drained. Not under capture (an allocation
  // and a copy): a captured call finds the table an eager call of its tiling made.
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  RM_HIP(ctx, hipStreamIsCapturing(ctx->stream, &cap));
  if (cap != hipStreamCaptureStatusNone)
    return fail(ctx, RM_ERR_UNSUPPORTED,
                "a captured call of %d x %d tiles needs the context's block order: run the same call once before "
                "the capture", tx, ty);
  ctx->block_orders.emplace_back();
  BlockOrder& o = ctx->block_orders.back();
  int rc;
  if ((rc = o.table.ensure(ctx, sizeof(int) * ord.size(), "block order")) != RM_OK) {
    ctx->block_orders.pop_back();
    return rc;
  }
  const hipError_t e = hipMemcpy(o.table.p, ord.data(), sizeof(int) * ord.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    ctx->block_orders.pop_back();
    return fail(ctx, RM_ERR_HIP, "block order upload: %s", hipGetErrorString(e));
  }
  o.tx = tx;
  o.ty = ty;
  o.sub = sub;
  *table = o.table.as<int>();
  return RM_OK;
}

// One launch of a call: ray blocks [done / rpb, +nb) of blocks_left still to run, nr rays.
struct Launch {
  long long done, nb, nr, blocks_left;
  int rpb;  // rays per block
};

// the centre-out block order of a launch of whole views
int bind_block_order(rm_context* ctx, const Call& c, const Launch& l, KArgs& a) {
  a.block_order = nullptr;
  const long long npix = (long long)c.W * c.H;
  if (!(c.cam && a.tiling == 2 && l.nb > 1 && l.done % npix == 0 && l.nr % npix == 0 && l.nr == l.nb * l.rpb &&
        (c.march->flags & RM_MARCH_NATURAL_ORDER) == 0))
    return RM_OK;
  int rc;
  const int* table = nullptr;
  if ((rc = ensure_block_order(ctx, c.W / 16, c.H / 16, 256 / l.rpb, &table)) != RM_OK) return rc;
  a.block_order = table;
  a.order_views = (int)(l.nr / npix);
  a.order_tiles = (int)(npix / l.rpb);
  return RM_OK;
}

// cost-ordered dispatch from the previous launch over the same views (single-launch calls)
int bind_cost_order(rm_context* ctx, const Call& c, const Launch& l, KArgs& a) {
  a.olist_r = nullptr;
  a.ocnt_r = nullptr;
  a.olist_w = nullptr;
  a.ocnt_w = nullptr;
  a.ocnt_z = nullptr;
  a.oturn = nullptr;
  a.order_views &= 0xFFFF;
  if (!c.has_bwd()) return RM_OK;
  unsigned long long key = 0;
  if (a.block_order != nullptr && l.nb == l.blocks_left && l.done == 0 && (c.march->flags & RM_MARCH_STATIC_ORDER) == 0) {
    key = ((unsigned long long)c.W << 48) ^ ((unsigned long long)c.H << 32) ^ ((unsigned long long)c.views << 24) ^
          ((unsigned long long)a.Mpad << 1) ^ 1ull ^ ((unsigned long long)(a.split != 0) << 2);
    const int shard_mask = order_shard_policy(l.nb);
    a.order_views |= shard_mask << 16;
    key ^= (unsigned long long)(shard_mask != 0) << 3;  // lists appended sharded are read sharded
    int rc;
    if ((rc = ctx->olist.ensure(ctx, sizeof(int) * 3 * kOrderLists * kMaxBlocksPerLaunch, "cost-order lists")) != RM_OK) return rc;
    // the three sets' counts, then the turn word, kOrderCntStride ints apart
    if ((rc = ctx->ocnt.ensure(ctx, sizeof(int) * 4 * kOrderCntStride, "cost-order counts", true)) != RM_OK) return rc;
    int* olist = ctx->olist.as<int>();
    int* ocnt = ctx->ocnt.as<int>();
    ctx->oturn = ocnt + 3 * kOrderCntStride;
    // three list sets in rotation: the previous launch's (read), this launch's (appended;
    // cleared by the previous launch) and the next launch's (cleared by this one); which is which
    // the kernel reads from the device turn word, advanced by this call's reduction (order_sets)
    if (ctx->cost_valid && ctx->cost_key == key) {
      a.olist_r = olist;
      a.ocnt_r = ocnt;
    }
    a.olist_w = olist;
    a.ocnt_w = ocnt;
    a.ocnt_z = env_is("RM_DEBUG_SKIP_ORDER_CLEAR", '1') ? nullptr : ocnt;  // recovery test (rm_debug_order_counts)
    a.oturn = ctx->oturn;
  }
  ctx->cost_valid = key != 0;
  ctx->cost_key = key;
  return RM_OK;
}

// The per-ray launch of nb blocks and, for a split march, its continuations.
// Split continuation (bwd / train launches with the early exit; KArgs::cont_cap): the groups
// whose rays still march at step caps[0] stop there and list themselves and those rays;
// continuation launches at increasing steps (split_cont_caps) march the listed rays packed
// into full blocks -- spread evenly over the CUs, where the first launch placed the groups by
// a cost order that only partly predicts which of them march every step -- and a resume
// launch finishes the listed groups. Bit-identical to one launch (tests/test_gpu_split.py).
int launch_with_continuations(rm_context* ctx, const Call& c, KArgs& a, long long nb) {
  int rc;
  const bool split = a.split != 0;
  const size_t lds = lds_bytes();
  const dim3 grid((unsigned)nb);
  hipEvent_t ev0, ev1;
  if ((rc = next_events(ctx, ev0, ev1)) != RM_OK) return rc;
  int caps[kMaxCont + 1];
  const int ncaps = split_cont_caps(a.steps, caps);
  const bool cont = split && c.has_bwd() && a.early_exit && ncaps > 0 && a.steps >= 2 * caps[0];
  int* glist = nullptr;  // the deferred groups and their count
  int* gcount = nullptr;
  int* rlists[2] = {nullptr, nullptr};
  int* rcounts[2] = {nullptr, nullptr};
  if (cont) {
    const long long rays = nb * kSplitRays;
    // the rays' and groups' saved states (ContState); the group list and its count; two ray lists
    // of up to `rays` entries and their counts
    const size_t need = ContState::floats(rays, nb) * sizeof(float) + (size_t)(nb + 8 + 16) * sizeof(int) +
                        (size_t)(2 * rays + 16) * sizeof(int);
    if ((rc = ctx->cont_buf.ensure(ctx, need, "continuation buffer")) != RM_OK) return rc;
    float* state = ctx->cont_buf.as<float>();
    glist = reinterpret_cast<int*>(state + ContState::floats(rays, nb));
    gcount = glist + nb;
    rcounts[0] = gcount + 8;  // the three counts 32 bytes apart
    rcounts[1] = rcounts[0] + 8;
    rlists[0] = rcounts[1] + 8;
    rlists[1] = rlists[0] + rays;
    a.cont_state = state;
    a.cont_rays = rays;
    a.cont_list_w = glist;
    a.cont_count_w = gcount;
    a.cont_cap = caps[0];
    a.cont_resume = 0;
    a.ray_list_w = rlists[0];  // the first launch appends the marching rays to ray list 0
    a.ray_count_w = rcounts[0];
    RM_HIP(ctx, hipMemsetAsync(gcount, 0, (8 + 16) * sizeof(int), ctx->stream));  // the three counts
  }
  // one per-ray launch of this call's mode and march (the continuation and resume launches below
  // run the same kernel)
  auto launch = [&](const KArgs& b, hipEvent_t e0, hipEvent_t e1) {
    bool built = true;
    with_mode(c.mode, [&](auto m) { built = launch_ray<decltype(m)::value>(c.cam, split, grid, lds, ctx->stream, b, e0, e1); });
    if (!built) return fail(ctx, RM_ERR_UNSUPPORTED, "the split march is not built for mode %d", c.mode);
    RM_HIP(ctx, hipGetLastError());
    return (int)RM_OK;
  };
  if ((rc = launch(a, ev0, ev1)) != RM_OK || !cont) return rc;
  auto launch_cont_mode = [&](const KArgs& b) {
    hipEvent_t e0, e1;
    const int rc2 = next_events(ctx, e0, e1);
    return rc2 != RM_OK ? rc2 : launch(b, e0, e1);
  };
  // continuation k marches the rays of ray list k % 2 (deferring at the next cap into
  // list (k + 1) % 2, whose count is cleared first: continuation k - 1 read it), then one resume
  // launch runs the deferred groups' post-march forward and backward from their final states
  for (int ph = 0; ph < ncaps; ++ph) {
    KArgs b = a;
    b.ray_cont = 1;
    b.cont_resume = caps[ph];
    b.cont_cap = caps[ph + 1];
    b.ray_list = rlists[ph & 1];
    b.ray_count = rcounts[ph & 1];
    b.ray_list_w = rlists[(ph + 1) & 1];
    b.ray_count_w = rcounts[(ph + 1) & 1];
    if (b.cont_cap > 0) RM_HIP(ctx, hipMemsetAsync(b.ray_count_w, 0, sizeof(int), ctx->stream));
    b.cont_list_w = nullptr;
    b.cont_count_w = nullptr;
    b.ocnt_z = nullptr;
    b.olist_r = nullptr;
    b.ocnt_r = nullptr;
    b.ocnt_w = nullptr;  // no groups of its own: the resume launch appends them
    b.olist_w = nullptr;
    if ((rc = launch_cont_mode(b)) != RM_OK) return rc;
  }
  KArgs b = a;
  b.cont_resume = a.steps;
  b.cont_cap = 0;
  b.cont_list = glist;
  b.cont_count = gcount;
  b.cont_list_w = nullptr;
  b.cont_count_w = nullptr;
  b.ray_list_w = nullptr;
  b.ray_count_w = nullptr;
  b.ocnt_z = nullptr;
  b.olist_r = nullptr;
  b.ocnt_r = nullptr;
  return launch_cont_mode(b);
}

int run(rm_context* ctx, const Call& c) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  // a prepared optimizer step is for the rm_optimizer_step right after its own sampled step: any
  // other call in between may change the parameters it was prepared on (sampled_step sets it again)
  ctx->opt_prepared = false;
  int rc;
  KArgs a;
  std::memset(&a, 0, sizeof a);
  if ((rc = check_geometry(ctx, c, c.mode != kRender)) != RM_OK) return rc;
  if ((rc = fill_camera_args(ctx, c, a)) != RM_OK) return rc;
  const long long n = c.rays();
  if ((rc = check_call(ctx, c, n)) != RM_OK) return rc;
  const bool has_bwd = c.has_bwd();

  fill_scene_args(c, a);
  a.out = c.out;
  a.t_out = c.t_out;
  a.t_in = c.t_in;
  a.gout = c.gout;
  a.targets = c.targets;
  a.progress = c.progress;
  a.inv_count = c.inv_count;
  a.sdev = ctx->sdev;
  a.dbg = c.dbg;
  ProofTier proof;
  const bool split = march_policy(c, n, a, proof);
  if (use_small(c, a.M, n)) return run_small(ctx, c, a, n);
  if (c.fused) return fail(ctx, RM_ERR_INVALID_ARG, "fused iteration outside the small kernel");
  const bool origin = c.cam && (c.march->flags & (RM_MARCH_PER_RAY_ORIGIN | RM_MARCH_FORCE_MAX_SHIFT)) == 0;
  if (n > 0 && (rc = prepare_records_and_lattice(ctx, a, origin, proof)) != RM_OK) return rc;

  const int rpb = split ? kSplitRays : kBlock;  // rays per block
  if (has_bwd && (rc = ctx->ws.ensure(ctx, ws_need(std::max<long long>(n, 1), a.M, rpb), "workspace")) != RM_OK)
    return rc;
  if (n == 0 && !has_bwd) return RM_OK;  // nothing to render; backward/train still define their outputs
  long long done = 0;
  do {
    Launch l;
    l.done = done;
    l.rpb = rpb;
    l.blocks_left = (n - done + rpb - 1) / rpb;
    l.nb = std::min<long long>(l.blocks_left, max_blocks_per_launch());
    l.nr = std::min<long long>(n - done, l.nb * rpb);
    a.ray_begin = done;
    a.n_rays = l.nr;
    a.partials = ctx->ws.as<float>();
    a.stats = ctx->stats_dev.as<unsigned long long>();
    if (ctx->stats_dev) {
      ctx->stats_blocks += l.nb;
      ctx->stats_waves += l.nb * (split ? 1 : kWaves);
    }
    if ((rc = bind_block_order(ctx, c, l, a)) != RM_OK) return rc;
    if ((rc = bind_cost_order(ctx, c, l, a)) != RM_OK) return rc;
    a.esc_flags = nullptr;
    if (l.nb > 0 && a.cull) {  // the escape pre-pass
      if ((rc = ctx->esc_flags.ensure(ctx, sizeof(int) * kMaxBlocksPerLaunch, "escape flags")) != RM_OK) return rc;
      int* flags = ctx->esc_flags.as<int>();
      with_mode(c.mode, [&](auto m) {
        launch_escape<decltype(m)::value>(c.cam, dim3((unsigned)l.nb), ctx->stream, a, flags);
      });
      RM_HIP(ctx, hipGetLastError());
      a.esc_flags = flags;
    }
    if ((rc = tile_proof(ctx, a, proof, l.nb, l.nr)) != RM_OK) return rc;
    if (l.nb > 0) {
#ifdef RM_BLOCK_TRACE
      if ((rc = bind_block_trace(ctx, a, l.nb * kWaves)) != RM_OK) return rc;
#endif
      if ((rc = launch_with_continuations(ctx, c, a, l.nb)) != RM_OK) return rc;
    }
    const bool first = done == 0;
    if (has_bwd && (rc = reduce_and_finalize(ctx, c, a, l.nb, first, first && l.nb == l.blocks_left)) != RM_OK) return rc;
    done += l.nr;
  } while (done < n);
  return RM_OK;
}

// ---- ray and camera-pose gradients (rm_raygrad.h) --------------------------------------------

int run_raygrad(rm_context* ctx, const RayGradCall& c) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  int rc;
  if ((rc = check_geometry(ctx, c, true)) != RM_OK) return rc;
  if (c.cam && !c.grad_cams) return fail(ctx, RM_ERR_INVALID_ARG, "grad_cams is NULL");
  if (!c.cam && !c.g_org && !c.g_dir) return fail(ctx, RM_ERR_INVALID_ARG, "grad_org and grad_dir are both NULL");
  const long long n = c.rays();
  if (n > 0 && !c.gout) return fail(ctx, RM_ERR_INVALID_ARG, "grad_out is NULL");
  if (n == 0) return RM_OK;
  const long long bpv = c.cam ? ((long long)c.W * c.H + kBlock - 1) / kBlock : 0;
  if ((rc = ctx->rg_ws.ensure(ctx, rg_need(n), "ray-gradient workspace")) != RM_OK) return rc;
  float* rg_ws = ctx->rg_ws.as<float>();

  // no saved t: the existing forward replays the march into the workspace (escaped rays' t carries
  // the documented guarantee); the gradient kernel itself never marches
  const float* t_in = c.t_in;
  if (!t_in) {
    Call f(kFwd, c);
    f.t_out = rg_ws;
    if ((rc = run(ctx, f)) != RM_OK) return rc;
    t_in = rg_ws;
  }
  ctx->opt_prepared = false;

  // the march fields of KArgs stay zero: the kernel starts from t_in
  KArgs a;
  std::memset(&a, 0, sizeof a);
  fill_scene_args(c, a);
  a.gout = c.gout;
  a.t_in = t_in;
  if ((rc = fill_camera_args(ctx, c, a)) != RM_OK) return rc;
  if ((rc = prepare_records(ctx, a, false)) != RM_OK) return rc;
  RayGradArgs r{};
  r.g_org = c.g_org;
  r.g_dir = c.g_dir;
  r.accumulate = c.accumulate ? 1 : 0;
  hipEvent_t ev0, ev1;
  if (c.cam) {
    RayGradCams tail;
    std::memset(&tail, 0, sizeof tail);
    for (int v = 0; v < c.views; ++v) tail.c[v] = c.cams[v];
    // the partial rows follow the t of all n rays (the replayed march may live there)
    r.partial = rg_ws + n;
    if ((rc = next_events(ctx, ev0, ev1)) != RM_OK) return rc;
    hipExtLaunchKernelGGL((rm_raygrad_kernel<true>), dim3((unsigned)bpv, (unsigned)c.views), dim3(kBlock), 0,
                          ctx->stream, ev0, ev1, 0u, a, r);
    RM_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(rm_raygrad_finish, dim3((unsigned)c.views), dim3(256), 0, ctx->stream, r.partial, (int)bpv, tail,
                       reinterpret_cast<float*>(c.grad_cams), r.accumulate);
    RM_HIP(ctx, hipGetLastError());
    return RM_OK;
  }
  for (long long done = 0; done < n;) {
    const long long nb = std::min<long long>((n - done + kBlock - 1) / kBlock, max_blocks_per_launch());
    const long long nr = std::min<long long>(n - done, nb * kBlock);
    a.ray_begin = done;
    a.n_rays = nr;
    if ((rc = next_events(ctx, ev0, ev1)) != RM_OK) return rc;
    hipExtLaunchKernelGGL((rm_raygrad_kernel<false>), dim3((unsigned)nb), dim3(kBlock), 0, ctx->stream, ev0, ev1, 0u,
                          a, r);
    RM_HIP(ctx, hipGetLastError());
    done += nr;
  }
  return RM_OK;
}

// The records of a scene-only call (run_view, run_sdf). The record kernel takes the scene and k through a march
// description, m (of its flags only the colour format counts): checks both, then if `launch` fills a and runs it.
int scene_records(rm_context* ctx, const rm_scene* scene, bool need_light, rm_march m, bool launch, KArgs& a) {
  int rc;
  m.mask_sharpness = 0.0f;
  m.flags &= RM_MARCH_COLOR_F16;
  const Geometry g = ray_geometry(nullptr, nullptr, 0, scene, &m);
  if ((rc = check_scene(ctx, scene, need_light)) != RM_OK) return rc;
  if ((rc = check_march(ctx, &m)) != RM_OK) return rc;
  std::memset(&a, 0, sizeof a);
  if (!launch) return RM_OK;
  fill_scene_args(g, a);
  return prepare_records(ctx, a, false);
}

// ---- the viewer's frame render (rm_view.h) ---------------------------------------------------

// viewer.rs:65-86 / shader.wgsl:108-110 in f32: ro and the basis ww, uu = ww x up, vv = uu x ww
void make_view_cam(const rm_view_camera& c, ViewCam& b) {
  auto normalize = [](const float v[3], float out[3]) {
    const float len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    for (int k = 0; k < 3; ++k) out[k] = v[k] / len;
  };
  auto cross = [](const float a[3], const float bb[3], float out[3]) {
    out[0] = a[1] * bb[2] - a[2] * bb[1];
    out[1] = a[2] * bb[0] - a[0] * bb[2];
    out[2] = a[0] * bb[1] - a[1] * bb[0];
  };
  float x[3];
  normalize(c.forward, b.ww);
  cross(b.ww, c.up, x);
  normalize(x, b.uu);
  cross(b.uu, b.ww, x);
  normalize(x, b.vv);
  for (int k = 0; k < 3; ++k) b.pos[k] = c.pos[k];
}

int run_view(rm_context* ctx, const rm_view_camera* cams, int frames, int W, int H, const rm_scene* scene,
             const rm_view_params& vp, float* out_rgb, uint8_t* out_rgba8, float* out_depth) {
  ctx->opt_prepared = false;
  int rc;
  rm_march m;
  rm_march_default(&m);
  m.steps = vp.max_steps;
  m.smooth_k = vp.smooth_k;
  m.normal_eps = vp.normal_eps;
  m.color_sharpness = vp.color_sharpness;
  m.flags = vp.flags;
  KArgs a;
  if ((rc = scene_records(ctx, scene, true, m, true, a)) != RM_OK) return rc;

  ViewArgs v;
  std::memset(&v, 0, sizeof v);
  v.rec_buf = a.rec_buf;
  v.Mpad = a.Mpad;
  v.width = W;
  v.height = H;
  v.tiles_x = (W + 15) / 16;
  v.max_steps = vp.max_steps;
  v.kappa = vp.smooth_k * kLog2e;
  v.hit_eps = vp.hit_eps;
  v.t_max = vp.t_max;
  v.normal_eps = vp.normal_eps;
  v.c10l = vp.color_sharpness * kLog2e;
  v.focal = vp.focal;
  v.count_iters = (vp.flags & RM_VIEW_COUNT_ITERATIONS) != 0;
  // the exact skips need every step to advance the ray (d >= hit_eps > 0), see rm_view.h
  // (the bounding radius R is in the record header on the device: the kernel adds it)
  const bool exits = (vp.flags & RM_MARCH_NO_EARLY_EXIT) == 0 && !v.count_iters && vp.hit_eps > 0.0f;
  v.skip_add = exits ? vp.hit_eps + a.lse_slack + 1e-3f : 0.0f;
  v.light_dir = scene->light_dir;
  v.ambient = scene->ambient;
  v.out_rgb = out_rgb;
  v.out_rgba8 = out_rgba8;
  v.out_depth = out_depth;
  const unsigned tiles = (unsigned)v.tiles_x * (unsigned)((H + 15) / 16);
  for (int f0 = 0; f0 < frames; f0 += kViewInline) {
    const int nf = std::min(kViewInline, frames - f0);
    for (int f = 0; f < nf; ++f) make_view_cam(cams[f0 + f], v.cams[f]);
    v.frame0 = f0;
    hipEvent_t ev0, ev1;
    if ((rc = next_events(ctx, ev0, ev1)) != RM_OK) return rc;
    hipExtLaunchKernelGGL(rm_view_kernel, dim3(tiles, (unsigned)nf), dim3(kBlock), 0, ctx->stream, ev0, ev1, 0u, v);
    RM_HIP(ctx, hipGetLastError());
  }
  return RM_OK;
}

// ---- the distance-field query (rm_sdf.h) -----------------------------------------------------

// The points of an rm_sdf_query (points, n) or the lattice of an rm_sdf_grid (grid: origin, spacing,
// nx, ny; n = nx ny nz). All the scratch it takes is the record buffer (rm_reserve covers it).
int run_sdf(rm_context* ctx, bool grid, const float* points, long long n, const float* origin, float spacing, int nx,
            int ny, const rm_scene* scene, const rm_sdf_params& sp, float* dist, float* grad, float* color) {
  ctx->opt_prepared = false;
  int rc;
  rm_march m;
  rm_march_default(&m);
  m.smooth_k = sp.smooth_k;
  m.color_sharpness = sp.color_sharpness;
  m.flags = sp.flags;
  KArgs a;
  if ((rc = scene_records(ctx, scene, false, m, n != 0, a)) != RM_OK) return rc;
  if (n == 0) return RM_OK;

  SdfArgs s;
  std::memset(&s, 0, sizeof s);
  s.rec_buf = a.rec_buf;
  s.Mpad = a.Mpad;
  s.kappa = sp.smooth_k * kLog2e;
  s.c10l = a.csharp * kLog2e;
  s.points = points;
  s.n = n;
  s.nx = nx;
  s.ny = ny;
  if (grid)
    for (int k = 0; k < 3; ++k) s.origin[k] = origin[k];
  s.spacing = spacing;
  s.dist = dist;
  s.grad = grad;
  s.color = color;
  const bool full = grad != nullptr || color != nullptr;
  for (long long done = 0; done < n;) {
    const long long nb = std::min<long long>((n - done + kBlock - 1) / kBlock, max_blocks_per_launch());
    s.begin = done;
    hipEvent_t ev0, ev1;
    if ((rc = next_events(ctx, ev0, ev1)) != RM_OK) return rc;
    const dim3 gr((unsigned)nb), blk(kBlock);
    if (grid && full) hipExtLaunchKernelGGL((rm_sdf_kernel<true, true>), gr, blk, 0, ctx->stream, ev0, ev1, 0u, s);
    else if (grid) hipExtLaunchKernelGGL((rm_sdf_kernel<true, false>), gr, blk, 0, ctx->stream, ev0, ev1, 0u, s);
    else if (full) hipExtLaunchKernelGGL((rm_sdf_kernel<false, true>), gr, blk, 0, ctx->stream, ev0, ev1, 0u, s);
    else hipExtLaunchKernelGGL((rm_sdf_kernel<false, false>), gr, blk, 0, ctx->stream, ev0, ev1, 0u, s);
    RM_HIP(ctx, hipGetLastError());
    done += nb * kBlock;
  }
  return RM_OK;
}

// ---- the distance field's backward (rm_sdf_grad_kernel, rm_sdf.h) ---------------------------------

// Blocks of 256 points per launch: the sub-launch limit, and no more than keep the per-sphere part of
// the launch's partial records within kSdfGradScratch bytes of the workspace (a record is 128 KB at
// 4096 spheres: 2048 blocks).
constexpr size_t kSdfGradScratch = (size_t)256 << 20;
long long sdf_grad_blocks_per_launch(int Mpad) {
  const long long fit = (long long)(kSdfGradScratch / (sizeof(float) * 8 * (size_t)Mpad));
  return std::max<long long>(1, std::min<long long>(fit, max_blocks_per_launch()));
}

// rm_sdf_query_backward. want: the scene gradient's members to write (light_dir and ambient NULL), or
// NULL for the point gradient alone. The partial records and the reduction's segment sums live in the
// context's workspace, as the ray kernels' do; rm_reduce_partials and the finalize run unchanged on them.
int run_sdf_grad(rm_context* ctx, const float* points, long long n, const rm_scene* scene, const rm_sdf_params& sp,
                 const float* g_dist, const float* g_color, const rm_grads* want, float* g_points, int accumulate) {
  ctx->opt_prepared = false;
  int rc;
  rm_march m;
  rm_march_default(&m);
  m.smooth_k = sp.smooth_k;
  m.color_sharpness = sp.color_sharpness;
  m.flags = sp.flags;
  KArgs a;
  if ((rc = scene_records(ctx, scene, false, m, n != 0, a)) != RM_OK) return rc;
  if (n == 0 && (want == nullptr || accumulate)) return RM_OK;
  m.mask_sharpness = 0.0f;
  m.flags &= RM_MARCH_COLOR_F16;
  Call c(kBwd, ray_geometry(nullptr, nullptr, 0, scene, &m));
  if (n == 0) fill_scene_args(c, a);  // no records: the reduction needs M and the record size only
  c.grads = want;
  c.accumulate = accumulate;
  const long long per = sdf_grad_blocks_per_launch(a.Mpad);
  if (want != nullptr) {
    const long long nbmax = std::max<long long>(1, std::min<long long>((n + kBlock - 1) / kBlock, per));
    const size_t need = (size_t)(nbmax * a.rec + (long long)reduce_segs(nbmax) * a.rec + 4096) * sizeof(float);
    if ((rc = ctx->ws.ensure(ctx, need, "workspace")) != RM_OK) return rc;
    a.partials = ctx->ws.as<float>();
  }
  if (n == 0) return reduce_and_finalize(ctx, c, a, 0, true);  // every requested element: zero

  SdfGradArgs s;
  std::memset(&s, 0, sizeof s);
  s.rec_buf = a.rec_buf;
  s.Mpad = a.Mpad;
  s.kappa = sp.smooth_k * kLog2e;
  s.c10l = a.csharp * kLog2e;
  s.cs = a.csharp;
  s.points = points;
  s.n = n;
  s.g_dist = g_dist;
  s.g_color = g_color;
  s.g_points = g_points;
  s.accumulate = accumulate ? 1 : 0;
  s.partials = a.partials;
  s.rec = a.rec;
  for (long long done = 0; done < n;) {
    const long long nb = std::min<long long>((n - done + kBlock - 1) / kBlock, per);
    s.begin = done;
    hipEvent_t ev0, ev1;
    if ((rc = next_events(ctx, ev0, ev1)) != RM_OK) return rc;
    hipExtLaunchKernelGGL(rm_sdf_grad_kernel, dim3((unsigned)nb), dim3(kBlock), 0, ctx->stream, ev0, ev1, 0u, s);
    RM_HIP(ctx, hipGetLastError());
    if (want != nullptr && (rc = reduce_and_finalize(ctx, c, a, nb, done == 0)) != RM_OK) return rc;
    done += nb * kBlock;
  }
  return RM_OK;
}

// ---- view-dependent colour (rm_sh.h) ---------------------------------------------------------

// rm_render_diff_sh[_camera] and their backward: the rays and the scene, the coefficients (degree 1 or 2:
// degree 0 is the existing entry point and never gets here) and the outputs of either direction.
struct ShCall : Geometry {
  const float* sh = nullptr;
  int degree = 0;
  float* out = nullptr;    // forward
  float* t_out = nullptr;  // forward, nullable
  const float* gout = nullptr;  // backward
  const float* t_in = nullptr;  // backward, nullable: the existing forward replays the march
  rm_grads want{};              // backward: the scene gradient's members to write
  float* grad_sh = nullptr;     // backward, nullable
  int accumulate = 0;
  explicit ShCall(const Geometry& g) : Geometry(g) {}
  int cols() const { return 3 * ((degree + 1) * (degree + 1) - 1); }  // 3B
};

// The march of an SH call: the existing forward (every kernel path and march flag) writes t for all rays.
int sh_march(rm_context* ctx, const ShCall& c, float* t) {
  Call f(kFwd, c);
  f.t_out = t;
  return run(ctx, f);
}

// The KArgs of the SH kernels (the march fields stay zero: they start from t_in), the call's records and its
// packed coefficients.
int sh_prepare(rm_context* ctx, const ShCall& c, KArgs& a, ShArgs& s) {
  int rc;
  std::memset(&a, 0, sizeof a);
  std::memset(&s, 0, sizeof s);
  fill_scene_args(c, a);
  if ((rc = fill_camera_args(ctx, c, a)) != RM_OK) return rc;
  if ((rc = prepare_records(ctx, a, false)) != RM_OK) return rc;
  const int np = a.Mpad / 2, cols = c.cols();
  if ((rc = ctx->sh_rec.ensure(ctx, sizeof(float2) * (size_t)np * cols, "coefficient records")) != RM_OK) return rc;
  hipLaunchKernelGGL(rm_sh_pack_kernel, dim3((unsigned)((np * cols + 255) / 256)), dim3(256), 0, ctx->stream, c.sh, a.M, np,
                     cols, ctx->sh_rec.as<float2>());
  RM_HIP(ctx, hipGetLastError());
  s.shp = ctx->sh_rec.as<const f2v>();
  return RM_OK;
}

int run_sh_forward(rm_context* ctx, const ShCall& c) {
  ctx->opt_prepared = false;
  int rc;
  if ((rc = check_geometry(ctx, c, true)) != RM_OK) return rc;
  const long long n = c.rays();
  if (n > 0 && !c.out && !c.t_out) return fail(ctx, RM_ERR_INVALID_ARG, "no output requested");
  if (n == 0) return RM_OK;
  float* t = c.t_out;
  if (!t) {
    if ((rc = ctx->rg_ws.ensure(ctx, rg_need(n), "ray-gradient workspace")) != RM_OK) return rc;
    t = ctx->rg_ws.as<float>();
  }
  if ((rc = sh_march(ctx, c, t)) != RM_OK || !c.out) return rc;
  KArgs a;
  ShArgs s;
  if ((rc = sh_prepare(ctx, c, a, s)) != RM_OK) return rc;
  a.t_in = t;
  a.out = c.out;
  for (long long done = 0; done < n;) {
    const long long nb = std::min<long long>((n - done + kBlock - 1) / kBlock, max_blocks_per_launch());
    a.ray_begin = done;
    a.n_rays = std::min<long long>(n - done, nb * kBlock);
    hipEvent_t ev0, ev1;
    if ((rc = next_events(ctx, ev0, ev1)) != RM_OK) return rc;
    const dim3 gr((unsigned)nb), blk(kBlock);
    if (c.cam && c.degree == 1) hipExtLaunchKernelGGL((rm_sh_shade_kernel<true, 3>), gr, blk, 0, ctx->stream, ev0, ev1, 0u, a, s);
    else if (c.cam) hipExtLaunchKernelGGL((rm_sh_shade_kernel<true, 8>), gr, blk, 0, ctx->stream, ev0, ev1, 0u, a, s);
    else if (c.degree == 1) hipExtLaunchKernelGGL((rm_sh_shade_kernel<false, 3>), gr, blk, 0, ctx->stream, ev0, ev1, 0u, a, s);
    else hipExtLaunchKernelGGL((rm_sh_shade_kernel<false, 8>), gr, blk, 0, ctx->stream, ev0, ev1, 0u, a, s);
    RM_HIP(ctx, hipGetLastError());
    done += nb * kBlock;
  }
  return RM_OK;
}

// Blocks of 256 rays per backward launch: the sub-launch limit, and no more than keep the per-sphere part of
// the launch's partial records (8 + 3B floats a sphere) within kSdfGradScratch bytes of the workspace.
long long sh_grad_blocks_per_launch(int Mpad, int cols) {
  const long long fit = (long long)(kSdfGradScratch / (sizeof(float) * (size_t)(8 + cols) * (size_t)Mpad));
  return std::max<long long>(1, std::min<long long>(fit, max_blocks_per_launch()));
}

// The coefficient gradient of a launch of nb blocks: rm_sh_reduce_partials + rm_sh_finalize on its records.
int sh_reduce(rm_context* ctx, const KArgs& a, const ShArgs& s, int cols, long long nb, float* S, float* grad_sh,
              int accumulate) {
  const int stride = a.Mpad * cols, seg_len = (int)((nb + kShSegs - 1) / kShSegs);
  hipLaunchKernelGGL(rm_sh_reduce_partials, dim3((unsigned)((stride + 255) / 256), (unsigned)kShSegs), dim3(256), 0,
                     ctx->stream, s.gsh_part, stride, a.partials + (long long)a.Mpad * 8 + 7, a.rec, (int)nb, seg_len, S);
  RM_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(rm_sh_finalize, dim3((unsigned)((a.M * cols + 255) / 256)), dim3(256), 0, ctx->stream, S, stride,
                     a.M * cols, grad_sh, accumulate);
  RM_HIP(ctx, hipGetLastError());
  return RM_OK;
}

int run_sh_backward(rm_context* ctx, const ShCall& c) {
  ctx->opt_prepared = false;
  int rc;
  if ((rc = check_geometry(ctx, c, true)) != RM_OK) return rc;
  const bool scene_grad = c.want.centers || c.want.colors || c.want.radius || c.want.light_dir || c.want.ambient;
  if (!scene_grad && !c.grad_sh) return fail(ctx, RM_ERR_INVALID_ARG, "no output requested");
  const long long n = c.rays();
  if (n > 0 && !c.gout) return fail(ctx, RM_ERR_INVALID_ARG, "grad_out is NULL");
  if (n == 0 && c.accumulate) return RM_OK;
  const float* t_in = c.t_in;
  if (n > 0 && !t_in) {  // no saved t: the existing forward replays the march into the workspace
    if ((rc = ctx->rg_ws.ensure(ctx, rg_need(n), "ray-gradient workspace")) != RM_OK) return rc;
    if ((rc = sh_march(ctx, c, ctx->rg_ws.as<float>())) != RM_OK) return rc;
    t_in = ctx->rg_ws.as<float>();
  }
  KArgs a;
  ShArgs s;
  if (n > 0) {
    if ((rc = sh_prepare(ctx, c, a, s)) != RM_OK) return rc;
  } else {  // no records: the reductions need M and the record sizes only
    std::memset(&a, 0, sizeof a);
    std::memset(&s, 0, sizeof s);
    fill_scene_args(c, a);
  }
  a.gout = c.gout;
  a.t_in = t_in;
  // the workspace: main partial records | their segment sums | coefficient records | their segment sums
  const int cols = c.cols();
  const long long per = sh_grad_blocks_per_launch(a.Mpad, cols);
  const long long nbmax = std::max<long long>(1, std::min<long long>((n + kBlock - 1) / kBlock, per));
  const long long main_floats = nbmax * a.rec + (long long)reduce_segs(nbmax) * a.rec + 4096;
  const long long rec_sh = (long long)a.Mpad * cols;
  if ((rc = ctx->ws.ensure(ctx, (size_t)(main_floats + (nbmax + kShSegs) * rec_sh) * sizeof(float), "workspace")) != RM_OK)
    return rc;
  a.partials = ctx->ws.as<float>();
  s.gsh_part = a.partials + main_floats;
  float* S_sh = s.gsh_part + nbmax * rec_sh;
  Call red(kBwd, c);  // the main record's reduction: the per-ray kernels', unchanged
  red.grads = &c.want;
  red.accumulate = c.accumulate;
  if (n == 0) {  // every requested element: zero
    if (scene_grad && (rc = reduce_and_finalize(ctx, red, a, 0, true)) != RM_OK) return rc;
    return c.grad_sh ? sh_reduce(ctx, a, s, cols, 0, S_sh, c.grad_sh, 0) : RM_OK;
  }
  for (long long done = 0; done < n;) {
    const long long nb = std::min<long long>((n - done + kBlock - 1) / kBlock, per);
    a.ray_begin = done;
    a.n_rays = std::min<long long>(n - done, nb * kBlock);
    hipEvent_t ev0, ev1;
    if ((rc = next_events(ctx, ev0, ev1)) != RM_OK) return rc;
    const dim3 gr((unsigned)nb), blk(kBlock);
    if (c.cam && c.degree == 1) hipExtLaunchKernelGGL((rm_sh_grad_kernel<true, 3>), gr, blk, 0, ctx->stream, ev0, ev1, 0u, a, s);
    else if (c.cam) hipExtLaunchKernelGGL((rm_sh_grad_kernel<true, 8>), gr, blk, 0, ctx->stream, ev0, ev1, 0u, a, s);
    else if (c.degree == 1) hipExtLaunchKernelGGL((rm_sh_grad_kernel<false, 3>), gr, blk, 0, ctx->stream, ev0, ev1, 0u, a, s);
    else hipExtLaunchKernelGGL((rm_sh_grad_kernel<false, 8>), gr, blk, 0, ctx->stream, ev0, ev1, 0u, a, s);
    RM_HIP(ctx, hipGetLastError());
    const bool first = done == 0;
    if (scene_grad && (rc = reduce_and_finalize(ctx, red, a, nb, first)) != RM_OK) return rc;
    if (c.grad_sh && (rc = sh_reduce(ctx, a, s, cols, nb, S_sh, c.grad_sh, first ? c.accumulate : 1)) != RM_OK) return rc;
    done += nb * kBlock;
  }
  return RM_OK;
}

// ---- the image-space loss (rm_loss.h) --------------------------------------------------------

// [b, b + n) floats against [a, a + n)
bool loss_overlap(const float* a, const float* b, long long n) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b, bytes = (uintptr_t)n * sizeof(float);
  return a && b && pa < pb + bytes && pb < pa + bytes;
}

int run_image_loss(rm_context* ctx, const float* out, const float* targets, int num_views, int width, int height,
                   float inv_count, const rm_image_loss_params* params, float* loss, float* view_stats, float* ssim_map,
                   float* grad_out) {
  ctx->opt_prepared = false;
  rm_image_loss_params p;
  rm_image_loss_default(&p);
  if (params) p = *params;
  if (!out) return fail(ctx, RM_ERR_INVALID_ARG, "out is NULL");
  if (!targets) return fail(ctx, RM_ERR_INVALID_ARG, "targets is NULL");
  if (num_views < 1) return fail(ctx, RM_ERR_INVALID_ARG, "num_views %d < 1", num_views);
  if (width < 1) return fail(ctx, RM_ERR_INVALID_ARG, "width %d < 1", width);
  if (height < 1) return fail(ctx, RM_ERR_INVALID_ARG, "height %d < 1", height);
  if (!std::isfinite(inv_count)) return fail(ctx, RM_ERR_INVALID_ARG, "inv_count is not finite");
  if (!(std::isfinite(p.l1_weight) && p.l1_weight >= 0.0f))
    return fail(ctx, RM_ERR_INVALID_ARG, "l1_weight %g: finite and >= 0 required", (double)p.l1_weight);
  if (!(std::isfinite(p.ssim_weight) && p.ssim_weight >= 0.0f))
    return fail(ctx, RM_ERR_INVALID_ARG, "ssim_weight %g: finite and >= 0 required", (double)p.ssim_weight);
  if (!std::isfinite(p.progress)) return fail(ctx, RM_ERR_INVALID_ARG, "progress is not finite");
  if (!(std::isfinite(p.c1) && p.c1 > 0.0f)) return fail(ctx, RM_ERR_INVALID_ARG, "c1 %g: finite and > 0 required", (double)p.c1);
  if (!(std::isfinite(p.c2) && p.c2 > 0.0f)) return fail(ctx, RM_ERR_INVALID_ARG, "c2 %g: finite and > 0 required", (double)p.c2);
  if ((p.flags & ~RM_LOSS_PLAIN_L1) != 0) return fail(ctx, RM_ERR_INVALID_ARG, "flags 0x%x: RM_LOSS_PLAIN_L1 only", p.flags);
  if (!loss && !view_stats && !ssim_map && !grad_out) return fail(ctx, RM_ERR_INVALID_ARG, "no output requested");
  const long long n = 3LL * num_views * height * width;  // floats of an image array
  if (loss_overlap(out, grad_out, n) || loss_overlap(targets, grad_out, n))
    return fail(ctx, RM_ERR_INVALID_ARG, "grad_out aliases out or targets");
  if (loss_overlap(out, ssim_map, n) || loss_overlap(targets, ssim_map, n))
    return fail(ctx, RM_ERR_INVALID_ARG, "ssim_map aliases out or targets");
  if (loss_overlap(grad_out, ssim_map, n)) return fail(ctx, RM_ERR_INVALID_ARG, "ssim_map aliases grad_out");

  LossArgs a;
  std::memset(&a, 0, sizeof a);
  a.x = out;
  a.y = targets;
  a.H = height;
  a.W = width;
  a.tiles_x = (width + kLossTW - 1) / kLossTW;
  a.tiles_y = (height + kLossTH - 1) / kLossTH;
  const long long tpv = (long long)a.tiles_x * a.tiles_y, nblocks = tpv * num_views;
  if (nblocks > INT32_MAX) return fail(ctx, RM_ERR_INVALID_ARG, "num_views x width x height: %lld tiles exceed one launch", nblocks);
  a.c1 = p.c1;
  a.c2 = p.c2;
  a.progress = p.progress;
  a.plain_l1 = (p.flags & RM_LOSS_PLAIN_L1) ? 1 : 0;
  a.l1_scale = p.l1_weight * inv_count;
  a.ssim_scale = -p.ssim_weight * inv_count;
  const bool ssim_grad = grad_out && a.ssim_scale != 0.0f;
  const bool stats = loss || view_stats || ssim_map || ssim_grad;

  // the context's scratch: per-view sums (double) | tile partial records | A | B | C
  const size_t sums_bytes = ((sizeof(double) * 3 * (size_t)num_views + 15) / 16) * 16;
  const size_t part_bytes = sizeof(float) * kLossPart * (size_t)nblocks;
  const size_t need = sums_bytes + part_bytes + (ssim_grad ? 3 * sizeof(float) * (size_t)n : 0);
  int rc;
  if ((rc = ctx->loss_ws.ensure(ctx, need, "image-loss scratch")) != RM_OK) return rc;
  char* base = ctx->loss_ws.as<char>();
  double* vsum = reinterpret_cast<double*>(base);
  a.partials = reinterpret_cast<float*>(base + sums_bytes);
  if (ssim_grad) {
    a.A = reinterpret_cast<float*>(base + sums_bytes + part_bytes);
    a.B = a.A + n;
    a.C = a.B + n;
  }
  a.S = ssim_map;
  a.grad = grad_out;
  const dim3 grid((unsigned)nblocks), blk(kLossThreads);
  if (stats) {
    hipLaunchKernelGGL(rm_loss_stats_kernel, grid, blk, 0, ctx->stream, a);
    RM_HIP(ctx, hipGetLastError());
  }
  if (loss || view_stats) {
    hipLaunchKernelGGL(rm_loss_view_sums, dim3((unsigned)num_views), dim3(64), 0, ctx->stream, a.partials, (int)tpv, vsum,
                       view_stats);
    RM_HIP(ctx, hipGetLastError());
  }
  if (loss) {
    hipLaunchKernelGGL(rm_loss_total, dim3(1), dim3(64), 0, ctx->stream, vsum, num_views, (double)n, p.l1_weight,
                       p.ssim_weight, inv_count, loss);
    RM_HIP(ctx, hipGetLastError());
  }
  if (grad_out) {
    hipLaunchKernelGGL(rm_loss_grad_kernel, grid, blk, 0, ctx->stream, a);
    RM_HIP(ctx, hipGetLastError());
  }
  return RM_OK;
}

}  // namespace
