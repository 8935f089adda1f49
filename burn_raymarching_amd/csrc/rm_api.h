// rm_api.h -- the C ABI of include/raymarch.h: each entry point checks what is particular to it,
// describes the call (ray_call / camera_call) and hands it to rm_launch.h. Host code only;
// included last by rm_kernels.hip.
#pragma once

namespace {

// the sampler's per-call key: (seed, stream, counter) mixed on the host
unsigned long long sample_key(uint64_t seed, uint64_t stream, uint64_t counter) {
  auto mix = [](unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  };
  return mix(mix(mix(seed) ^ stream) ^ counter);
}

// the dataset and the draw of a launch that samples its own batch (rm_small_kernel<.., FUSED>)
SmallArgs sampling_args(const float* ray_org, const float* ray_dir, const float* targets, int64_t num_src,
                        const int32_t* fg_indices, int64_t num_fg, int64_t n_uniform, uint64_t seed, uint64_t stream,
                        uint64_t counter) {
  SmallArgs fz;
  std::memset(&fz, 0, sizeof fz);
  fz.src_org = ray_org;
  fz.src_dir = ray_dir;
  fz.src_tgt = targets;
  fz.fg = fg_indices;
  fz.num_src = num_src;
  fz.num_fg = num_fg;
  fz.n_uniform = n_uniform;
  fz.key = sample_key(seed, stream, counter);
  return fz;
}

// rm_sample_batch into the context's batch buffer, then rm_train_step on it: the separate-call
// form of the sampled step (rm_train_iteration's and rm_train_step_sampled's other sizes)
int sample_then_train(rm_context* ctx, const float* ray_org, const float* ray_dir, const float* targets,
                      int64_t num_src, const int32_t* fg_indices, int64_t num_fg, int64_t n_uniform, int64_t n_fg,
                      uint64_t seed, uint64_t stream, uint64_t counter, float progress, float inv_count,
                      const rm_scene* sc, const rm_march* march, const rm_grads* gr, float* loss_sum) {
  const long long n = n_uniform + n_fg;
  int rc;
  if (n > 0 && (rc = ctx->batch.ensure(ctx, sizeof(float) * 9 * (size_t)n, "batch buffer")) != RM_OK) return rc;
  float* bo = ctx->batch.as<float>();
  float* bd = bo ? bo + 3 * n : nullptr;
  float* bt = bo ? bo + 6 * n : nullptr;
  if (n > 0 && (rc = rm_sample_batch(ctx, ray_org, ray_dir, targets, num_src, fg_indices, num_fg, n_uniform, n_fg, seed,
                                     stream, counter, bo, bd, bt, nullptr)) != RM_OK)
    return rc;
  return rm_train_step(ctx, bo, bd, bt, n, progress, inv_count, sc, march, gr, loss_sum, nullptr, 0);
}

// the sampled step's validation (rm_train_iteration and rm_train_step_sampled)
int check_sampling(rm_context* ctx, const float* ray_org, const float* ray_dir, const float* targets,
                   int64_t num_src, const int32_t* fg_indices, int64_t num_fg, int64_t n_uniform, int64_t n_fg) {
  if (!ray_org || !ray_dir || !targets) return fail(ctx, RM_ERR_INVALID_ARG, "NULL dataset array");
  if (num_src < 1 || num_src > INT32_MAX || n_uniform < 0 || n_fg < 0 || num_fg < 0)
    return fail(ctx, RM_ERR_INVALID_ARG, "bad sampling sizes");
  if (n_fg > 0 && (num_fg == 0 || !fg_indices)) return fail(ctx, RM_ERR_INVALID_ARG, "n_fg > 0 needs foreground indices");
  return RM_OK;
}

// one launch of the small-scene kernel with its in-kernel final reduction for this call
bool sampled_one_launch(const Call& c, int M, long long n) {
  const int rpb = kBlock / small_lpr(c, n);
  return use_small(c, M, n) && (n + rpb - 1) / rpb <= kSmallFinalMaxBlocks &&
         (n + rpb - 1) / rpb <= max_blocks_per_launch() && !env_is("RM_FUSED_ITER", '0');
}

// rm_train_step_sampled[_prepared]; raw_packed != nullptr: prepare the next optimizer step
int sampled_step(rm_context* ctx, const float* ray_org, const float* ray_dir, const float* targets, int64_t num_src,
                 const int32_t* fg_indices, int64_t num_fg, int64_t n_uniform, int64_t n_fg, uint64_t seed,
                 uint64_t stream, uint64_t counter, float progress, float inv_count, const rm_scene* scene,
                 const rm_march* march, const rm_grads* grads, float* loss_sum, const float* raw_packed, int32_t step,
                 int32_t with_penalties, float* loss_penalty) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  ctx->opt_prepared = false;  // a preparation is for the optimizer call right after its own step
  int rc;
  if ((rc = check_sampling(ctx, ray_org, ray_dir, targets, num_src, fg_indices, num_fg, n_uniform, n_fg)) != RM_OK)
    return rc;
  if (!scene || !march || !grads) return fail(ctx, RM_ERR_INVALID_ARG, "NULL scene / march / grads");
  if (scene->num_spheres < 1 || scene->num_spheres > RM_MAX_SPHERES) return fail(ctx, RM_ERR_INVALID_ARG, "bad num_spheres");
  const long long n = n_uniform + n_fg;
  Call c = ray_call(kTrain, ray_org, ray_dir, n, scene, march);
  set_training(c, targets, progress, inv_count, grads, loss_sum, 0);
  // one launch: the small kernel draws its rays and reduces the gradient in its last block
  if (n > 0 && sampled_one_launch(c, scene->num_spheres, n) && ctx->sdev == nullptr) {
    SmallArgs fz = sampling_args(ray_org, ray_dir, targets, num_src, fg_indices, num_fg, n_uniform, seed, stream, counter);
    const int M = scene->num_spheres;
    const bool prep = raw_packed != nullptr && M <= kOptSmallMaxM && !env_is("RM_OPT_SMALL", '0') &&
                      !env_is("RM_OPT_PREPARE", '0');
    fz.adam = prep ? 2 : 0;
    if (prep) {  // the extra block: opt_small_pre of rm_optimizer_small on these parameters
      fz.raw = const_cast<float*>(raw_packed);
      fz.m1 = fz.m2 = const_cast<float*>(raw_packed);  // loaded with the parameters, not used
      fz.step = step;
      fz.with_pen = with_penalties ? 1 : 0;
      fz.loss_penalty = loss_penalty;
    }
    c.fused = &fz;
    rc = run(ctx, c);
    if (rc == RM_OK && prep) {
      ctx->opt_prepared = true;
      ctx->prep_raw = raw_packed;
      ctx->prep_loss_penalty = loss_penalty;
      ctx->prep_M = M;
      ctx->prep_step = step;
      ctx->prep_pen = with_penalties ? 1 : 0;
    }
    return rc;
  }
  return sample_then_train(ctx, ray_org, ray_dir, targets, num_src, fg_indices, num_fg, n_uniform, n_fg, seed, stream,
                           counter, progress, inv_count, scene, march, grads, loss_sum);
}

// the parameters of rm_sdf_query / rm_sdf_grid (NULL: the defaults) and their flags
int check_sdf_params(rm_context* ctx, const rm_sdf_params* params, rm_sdf_params& sp) {
  rm_sdf_params_default(&sp);
  if (params) sp = *params;
  if ((sp.flags & ~RM_MARCH_COLOR_F16) != 0)
    return fail(ctx, RM_ERR_INVALID_ARG, "flags 0x%x: the distance-field calls take RM_MARCH_COLOR_F16 only", sp.flags);
  return RM_OK;
}

// the coefficients of the rm_render_diff_sh calls
int check_sh(rm_context* ctx, const float* sh, int32_t sh_degree) {
  if (sh_degree < 0 || sh_degree > RM_SH_MAX_DEGREE)
    return fail(ctx, RM_ERR_INVALID_ARG, "sh_degree %d out of [0, %d]", sh_degree, RM_SH_MAX_DEGREE);
  if (sh_degree > 0 && !sh) return fail(ctx, RM_ERR_INVALID_ARG, "sh is NULL with sh_degree %d", sh_degree);
  return RM_OK;
}

ShCall sh_forward_call(const Geometry& g, const float* sh, int degree, float* out, float* t_march) {
  ShCall c(g);
  c.sh = sh;
  c.degree = degree;
  c.out = out;
  c.t_out = t_march;
  return c;
}

ShCall sh_backward_call(const Geometry& g, const float* sh, int degree, const float* grad_out, const float* t_march,
                        const rm_grads* grads, float* grad_sh, int accumulate) {
  ShCall c(g);
  c.sh = sh;
  c.degree = degree;
  c.gout = grad_out;
  c.t_in = t_march;
  if (grads) c.want = *grads;
  c.grad_sh = grad_sh;
  c.accumulate = accumulate;
  return c;
}

}  // namespace

extern "C" {

#ifndef RM_SOURCE_SHA
#define RM_SOURCE_SHA "unknown"  // _build.py passes the sha256 of the kernel sources
#endif
const char* rm_version(void) { return "burn_raymarching_amd 0.1.0 (gfx950) src " RM_SOURCE_SHA; }

int rm_create(int32_t device, void* stream, rm_context** out_ctx) {
  if (!out_ctx) return RM_ERR_INVALID_ARG;
  *out_ctx = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return RM_ERR_HIP;
  if (hipSetDevice(device) != hipSuccess) return RM_ERR_HIP;
  rm_context* ctx = new rm_context();
  ctx->device = device;
  ctx->stream = static_cast<hipStream_t>(stream);
  *out_ctx = ctx;
  return RM_OK;
}

int rm_bind_step_scalars(rm_context* ctx, rm_step_scalars* dev) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  ctx->sdev = dev;
  return RM_OK;
}

int rm_set_stream(rm_context* ctx, void* stream) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  ctx->stream = static_cast<hipStream_t>(stream);
  return RM_OK;
}

int rm_timing_enable(rm_context* ctx, int32_t enable) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  ctx->timing = enable != 0;
  // pre-create a pool so event creation stays out of timed regions
  while (ctx->timing && ctx->events.size() < 256) {
    std::pair<hipEvent_t, hipEvent_t> pr;
    RM_HIP(ctx, hipEventCreate(&pr.first));
    RM_HIP(ctx, hipEventCreate(&pr.second));
    ctx->events.push_back(pr);
  }
  return RM_OK;
}

int rm_timing_collect(rm_context* ctx, double* total_ms, int64_t* launches, int32_t reset) {
  if (!ctx || !total_ms || !launches) return RM_ERR_INVALID_ARG;
  double acc = 0.0;
  for (size_t i = 0; i < ctx->events_used; ++i) {
    RM_HIP(ctx, hipEventSynchronize(ctx->events[i].second));
    float ms = 0.0f;
    RM_HIP(ctx, hipEventElapsedTime(&ms, ctx->events[i].first, ctx->events[i].second));
    acc += ms;
  }
  *total_ms = acc;
  *launches = (int64_t)ctx->events_used;
  if (reset) ctx->events_used = 0;
  return RM_OK;
}

int rm_debug_order_counts(rm_context* ctx, int32_t* counts, int32_t capacity, int32_t* classes, int32_t* next_set) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  constexpr int kCls = kOrderClasses;
  if (classes) *classes = kCls;
  if (counts && capacity < 3 * kCls) return fail(ctx, RM_ERR_INVALID_ARG, "counts needs %d entries", 3 * kCls);
  RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  std::vector<int> host(4 * kOrderCntStride, 0);  // the sets' counts and the device turn word
  if (ctx->ocnt) RM_HIP(ctx, hipMemcpy(host.data(), ctx->ocnt.p, sizeof(int) * host.size(), hipMemcpyDeviceToHost));
  if (next_set) *next_set = host[3 * kOrderCntStride];
  if (counts)
    for (int st = 0; st < 3; ++st)
      for (int l = 0; l < kOrderLists; ++l) {  // the last class: the sum of its per-XCD lists
        const int c = std::min(l, kCls - 1);
        counts[st * kCls + c] = (l > c ? counts[st * kCls + c] : 0) + host[st * kOrderCntStride + l * kOrderClsStride];
        if (l >= kCls - 1 && capacity >= 3 * kCls + 3 * kOrderShards)  // the last class's lists one by one
          counts[3 * kCls + st * kOrderShards + (l - (kCls - 1))] = host[st * kOrderCntStride + l * kOrderClsStride];
      }
  return RM_OK;
}

#ifdef RM_BLOCK_TRACE
// Measurement build only (not in include/raymarch.h): the per-wave records of the last per-ray
// launch, 4 x u64 per wave in launch order (see rm_ray_kernel). Synchronises the stream.
int rm_debug_block_trace(rm_context* ctx, unsigned long long* host, int64_t cap_waves, int64_t* n_waves) {
  if (!ctx || !host || !n_waves) return RM_ERR_INVALID_ARG;
  RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const long long n = std::min<long long>(ctx->btrace_waves, cap_waves);
  *n_waves = n;
  if (n > 0) RM_HIP(ctx, hipMemcpy(host, ctx->btrace.p, sizeof(unsigned long long) * kTraceWords * n, hipMemcpyDeviceToHost));
  return RM_OK;
}
#endif

int rm_debug_tile_proof(rm_context* ctx, uint8_t* host, int64_t capacity, int64_t* n_waves) {
  if (!ctx || !host || !n_waves || capacity < 0) return RM_ERR_INVALID_ARG;
  RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const long long n = ctx->tile_proof ? std::min<long long>(ctx->tile_proof_n, capacity) : 0;
  *n_waves = n;
  if (n > 0) RM_HIP(ctx, hipMemcpy(host, ctx->tile_proof.p, (size_t)n, hipMemcpyDeviceToHost));
  return RM_OK;
}

int rm_debug_stall(rm_context* ctx, int32_t max_ms) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  if (max_ms < 1 || max_ms > 600000) return fail(ctx, RM_ERR_INVALID_ARG, "max_ms %d out of [1, 600000]", max_ms);
  if (!ctx->stall_flag)
    RM_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&ctx->stall_flag), 64, hipHostMallocMapped | hipHostMallocCoherent));
  __atomic_store_n(ctx->stall_flag, 0, __ATOMIC_RELEASE);
  int* dflag = nullptr;
  RM_HIP(ctx, hipHostGetDevicePointer(reinterpret_cast<void**>(&dflag), ctx->stall_flag, 0));
  hipLaunchKernelGGL(rm::rm_stall_kernel, dim3(1), dim3(64), 0, ctx->stream, dflag,
                     (unsigned long long)max_ms * 100000ull);  // s_memrealtime: 100 MHz
  RM_HIP(ctx, hipGetLastError());
  return RM_OK;
}

int rm_debug_stall_release(rm_context* ctx) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  if (ctx->stall_flag) __atomic_store_n(ctx->stall_flag, 1, __ATOMIC_RELEASE);
  return RM_OK;
}

int rm_stats_enable(rm_context* ctx, int32_t enable) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  if (enable && !ctx->stats_dev) {
    int rc = ctx->stats_dev.ensure(ctx, kStatsWords * sizeof(unsigned long long), "work counters", true);
    if (rc != RM_OK) return rc;
    ctx->stats_blocks = 0;
    ctx->stats_waves = 0;
  } else if (!enable && ctx->stats_dev) {
    RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stats_dev.release();
  }
  return RM_OK;
}

int rm_stats_collect(rm_context* ctx, rm_stats* out, int32_t reset) {
  if (!ctx || !out) return RM_ERR_INVALID_ARG;
  if (!ctx->stats_dev) return fail(ctx, RM_ERR_INVALID_ARG, "stats are not enabled");
  unsigned long long v[kStatsWords];
  RM_HIP(ctx, hipMemcpyAsync(v, ctx->stats_dev.p, sizeof v, hipMemcpyDeviceToHost, ctx->stream));
  RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  out->blocks = ctx->stats_blocks;
  out->blocks_skipped = (int64_t)v[0];
  out->waves = ctx->stats_waves;
  out->waves_exited = (int64_t)v[1];
  out->steps_saved = (int64_t)v[2];
  out->seeded_rays = (int64_t)v[4];
  out->seeded_rays_a = (int64_t)v[5];
  if (reset) {
    RM_HIP(ctx, hipMemsetAsync(ctx->stats_dev.p, 0, sizeof v, ctx->stream));
    ctx->stats_blocks = 0;
    ctx->stats_waves = 0;
  }
  return RM_OK;
}

void rm_destroy(rm_context* ctx) {
  if (!ctx) return;
  // a pending stall ends before its flag goes away
  if (ctx->stall_flag) __atomic_store_n(ctx->stall_flag, 1, __ATOMIC_RELEASE);
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->stall_flag) (void)hipHostFree(ctx->stall_flag);
  if (ctx->cams_pin) (void)hipHostFree(ctx->cams_pin);
  for (hipEvent_t& e : ctx->cam_ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& pr : ctx->events) {
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  delete ctx;  // every DevBuf frees its buffer
}

const char* rm_last_error(const rm_context* ctx) { return ctx ? ctx->err.c_str() : "NULL context"; }

void rm_march_default(rm_march* m) {
  if (!m) return;
  m->steps = 40;             // renderer_diff.rs:22
  m->smooth_k = 32.0f;       // train.rs:131 MAX_SMOOTH / preview train.rs:355
  m->normal_eps = 1e-4f;     // scene.rs:91
  m->color_sharpness = 10.0f; // renderer_diff.rs:74
  m->mask_sharpness = 15.0f;  // renderer_diff.rs:88
  m->flags = 0;
}

int rm_reserve(rm_context* ctx, int64_t max_rays, int32_t max_spheres) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  if (max_rays < 0 || max_spheres < 1 || max_spheres > RM_MAX_SPHERES)
    return fail(ctx, RM_ERR_INVALID_ARG, "bad reserve sizes");
  const int64_t rays = std::max<int64_t>(max_rays, 1);
  int rc;
  // the small buffers the calls otherwise allocate on first use: the arrival counters of the
  // in-kernel reductions (zeroed) and the fused iteration's optimizer hand-off
  if ((rc = ctx->arrivals.ensure(ctx, 64, "arrival counter", true)) != RM_OK) return rc;
  if ((rc = ctx->red_arrivals.ensure(ctx, sizeof(unsigned) * kRedArrivals, "reduction counters", true)) != RM_OK) return rc;
  if ((rc = ctx->opt_arrival.ensure(ctx, 128, "optimizer counter", true)) != RM_OK) return rc;
  if ((rc = ctx->opt_pre.ensure(ctx, sizeof(float) * (4 * kOptPreStride + 2), "optimizer hand-off")) != RM_OK) return rc;
  if ((rc = ctx->rg_ws.ensure(ctx, rg_need(rays), "ray-gradient workspace")) != RM_OK) return rc;
  {  // the sphere records: all the scratch rm_view takes
    if ((rc = ctx->rec.ensure(ctx, RecLayout(pad_spheres(max_spheres)).bytes(), "record buffer")) != RM_OK) return rc;
  }
  if (rays >= kLatticeMinRays && pad_spheres(max_spheres) >= kProofMinSpheres && (rc = ensure_proof_buffers(ctx)) != RM_OK)
    return rc;
  return ctx->ws.ensure(ctx, ws_need(rays, max_spheres), "workspace");
}

int rm_render_diff(rm_context* ctx, const float* ray_org, const float* ray_dir, int64_t num_rays,
                   const rm_scene* scene, const rm_march* march, float* out, float* t_march) {
  Call c = ray_call(kFwd, ray_org, ray_dir, num_rays, scene, march);
  c.out = out;
  c.t_out = t_march;
  return run(ctx, c);
}

int rm_render_diff_camera(rm_context* ctx, const rm_camera* cams, int32_t num_views, int32_t width, int32_t height,
                          const rm_scene* scene, const rm_march* march, float* out, float* t_march) {
  Call c = camera_call(kFwd, cams, num_views, width, height, scene, march);
  c.out = out;
  c.t_out = t_march;
  return run(ctx, c);
}

int rm_render_diff_backward(rm_context* ctx, const float* ray_org, const float* ray_dir, int64_t num_rays,
                            const rm_scene* scene, const rm_march* march, const float* grad_out,
                            const float* t_march, const rm_grads* grads, int32_t accumulate) {
  Call c = ray_call(kBwd, ray_org, ray_dir, num_rays, scene, march);
  c.gout = grad_out;
  c.t_in = t_march;
  c.grads = grads;
  c.accumulate = accumulate;
  return run(ctx, c);
}

int rm_render_diff_backward_camera(rm_context* ctx, const rm_camera* cams, int32_t num_views, int32_t width,
                                   int32_t height, const rm_scene* scene, const rm_march* march,
                                   const float* grad_out, const float* t_march, const rm_grads* grads,
                                   int32_t accumulate) {
  Call c = camera_call(kBwd, cams, num_views, width, height, scene, march);
  c.gout = grad_out;
  c.t_in = t_march;
  c.grads = grads;
  c.accumulate = accumulate;
  return run(ctx, c);
}

int rm_train_step(rm_context* ctx, const float* ray_org, const float* ray_dir, const float* targets,
                  int64_t num_rays, float progress, float inv_count, const rm_scene* scene, const rm_march* march,
                  const rm_grads* grads, float* loss_sum, float* out, int32_t accumulate) {
  Call c = ray_call(kTrain, ray_org, ray_dir, num_rays, scene, march);
  set_training(c, targets, progress, inv_count, grads, loss_sum, accumulate);
  c.out = out;
  return run(ctx, c);
}

int rm_train_step_camera(rm_context* ctx, const rm_camera* cams, int32_t num_views, int32_t width, int32_t height,
                         const float* targets, float progress, float inv_count, const rm_scene* scene,
                         const rm_march* march, const rm_grads* grads, float* loss_sum, float* out,
                         int32_t accumulate) {
  Call c = camera_call(kTrain, cams, num_views, width, height, scene, march);
  set_training(c, targets, progress, inv_count, grads, loss_sum, accumulate);
  c.out = out;
  return run(ctx, c);
}

int rm_render(rm_context* ctx, const float* ray_org, const float* ray_dir, int64_t num_rays, const float* centers,
              const float* colors, const float* radius, int32_t num_spheres, float* out) {
  rm_scene sc{centers, colors, radius, nullptr, nullptr, num_spheres};
  rm_march m;
  rm_march_default(&m);  // 40 steps, k = 32, eps 1e-4, exp(-10 d) (renderer.rs:17-19, :52)
  Call c = ray_call(kRender, ray_org, ray_dir, num_rays, &sc, &m);
  c.out = out;
  return run(ctx, c);
}

int rm_render_camera(rm_context* ctx, const rm_camera* cams, int32_t num_views, int32_t width, int32_t height,
                     const float* centers, const float* colors, const float* radius, int32_t num_spheres,
                     float* out) {
  rm_scene sc{centers, colors, radius, nullptr, nullptr, num_spheres};
  rm_march m;
  rm_march_default(&m);
  Call c = camera_call(kRender, cams, num_views, width, height, &sc, &m);
  c.out = out;
  return run(ctx, c);
}

int rm_debug_intermediates(rm_context* ctx, const float* ray_org, const float* ray_dir, int64_t num_rays,
                           const rm_scene* scene, const rm_march* march, float* dbg) {
  if (!dbg) return fail(ctx, RM_ERR_INVALID_ARG, "dbg is NULL");
  Call c = ray_call(kFwd, ray_org, ray_dir, num_rays, scene, march);
  c.dbg = dbg;
  return run(ctx, c);
}

int rm_scene_activate(rm_context* ctx, const float* raw_packed, int32_t num_spheres, float* act_packed) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  ctx->opt_prepared = false;  // the parameters may have changed since a prepared step (see run)
  if (!raw_packed || !act_packed) return fail(ctx, RM_ERR_INVALID_ARG, "NULL packed buffer");
  if (num_spheres < 1 || num_spheres > RM_MAX_SPHERES) return fail(ctx, RM_ERR_INVALID_ARG, "bad num_spheres");
  const int n = 7 * num_spheres + 4;
  hipLaunchKernelGGL(rm::rm_activate_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, raw_packed,
                     num_spheres, act_packed);
  RM_HIP(ctx, hipGetLastError());
  return RM_OK;
}

int rm_gather_rays(rm_context* ctx, const float* ray_org, const float* ray_dir, const float* targets,
                   int64_t num_src, const int32_t* indices, int64_t num_rays, float* out_org, float* out_dir,
                   float* out_targets) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  ctx->opt_prepared = false;
  if (num_rays < 0 || num_src < 0) return fail(ctx, RM_ERR_INVALID_ARG, "negative size");
  if (num_rays == 0) return RM_OK;
  if (!indices) return fail(ctx, RM_ERR_INVALID_ARG, "indices is NULL");
  if ((out_org && !ray_org) || (out_dir && !ray_dir) || (out_targets && !targets))
    return fail(ctx, RM_ERR_INVALID_ARG, "an output is requested without its source array");
  if (!out_org && !out_dir && !out_targets) return fail(ctx, RM_ERR_INVALID_ARG, "no output requested");
  const long long nel = 3 * (long long)num_rays;
  hipLaunchKernelGGL(rm::rm_gather_kernel, dim3((unsigned)((nel + 255) / 256)), dim3(256), 0, ctx->stream, ray_org,
                     ray_dir, targets, (long long)num_src, indices, (long long)num_rays, out_org, out_dir,
                     out_targets);
  RM_HIP(ctx, hipGetLastError());
  return RM_OK;
}

int rm_sample_batch(rm_context* ctx, const float* ray_org, const float* ray_dir, const float* targets, int64_t num_src,
                    const int32_t* fg_indices, int64_t num_fg, int64_t n_uniform, int64_t n_fg, uint64_t seed,
                    uint64_t stream, uint64_t counter, float* out_org, float* out_dir, float* out_targets,
                    int32_t* indices_out) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  ctx->opt_prepared = false;
  if (num_src < 0 || num_fg < 0 || n_uniform < 0 || n_fg < 0) return fail(ctx, RM_ERR_INVALID_ARG, "negative size");
  const long long n = n_uniform + n_fg;
  if (n == 0) return RM_OK;
  if (num_src == 0 || num_src > INT32_MAX) return fail(ctx, RM_ERR_INVALID_ARG, "num_src %lld out of [1, 2^31)", (long long)num_src);
  if (n_fg > 0 && (num_fg == 0 || !fg_indices)) return fail(ctx, RM_ERR_INVALID_ARG, "n_fg > 0 needs foreground indices");
  if ((out_org && !ray_org) || (out_dir && !ray_dir) || (out_targets && !targets))
    return fail(ctx, RM_ERR_INVALID_ARG, "an output is requested without its source array");
  if (!out_org && !out_dir && !out_targets && !indices_out) return fail(ctx, RM_ERR_INVALID_ARG, "no output requested");
  const unsigned long long key = sample_key(seed, stream, counter);
  hipLaunchKernelGGL(rm::rm_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ray_org, ray_dir,
                     targets, (long long)num_src, fg_indices, (long long)num_fg, (long long)n_uniform, n, key, out_org,
                     out_dir, out_targets, indices_out);
  RM_HIP(ctx, hipGetLastError());
  return RM_OK;
}

void rm_scene_from_packed(const float* act, int32_t M, rm_scene* s) {
  if (!s) return;
  s->centers = act;
  s->colors = act + 3 * M;
  s->radius = act + 6 * M;
  s->light_dir = act + 7 * M;
  s->ambient = act + 7 * M + 3;
  s->num_spheres = M;
}

void rm_grads_from_packed(float* g, int32_t M, rm_grads* o) {
  if (!o) return;
  o->centers = g;
  o->colors = g + 3 * M;
  o->radius = g + 6 * M;
  o->light_dir = g + 7 * M;
  o->ambient = g + 7 * M + 3;
}

int rm_optimizer_step_f16(rm_context* ctx, float* raw_packed, const float* grad_act_packed, float* adam_m,
                          float* adam_v, int32_t num_spheres, int32_t step, float lr, float weight_decay,
                          int32_t with_penalties, float* loss_penalty, float* act_out, uint16_t* colors_f16_out) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  if (!raw_packed || !grad_act_packed || !adam_m || !adam_v)
    return fail(ctx, RM_ERR_INVALID_ARG, "NULL optimizer buffer");
  if (num_spheres < 1 || num_spheres > RM_MAX_SPHERES) return fail(ctx, RM_ERR_INVALID_ARG, "bad num_spheres");
  if (step < 1 && !ctx->sdev) return fail(ctx, RM_ERR_INVALID_ARG, "step counts from 1");
  const int M = num_spheres;
  const int n = 7 * M + 4;
  const int nb = (n + 255) / 256;
  const bool prepared = ctx->opt_prepared && ctx->prep_raw == raw_packed && ctx->prep_M == M &&
                        ctx->prep_step == step && ctx->prep_pen == (with_penalties ? 1 : 0) &&
                        ctx->prep_loss_penalty == loss_penalty && !ctx->sdev;
  ctx->opt_prepared = false;
  if (prepared) {  // the gradient-independent part ran in the sampled launch (rm_train_step_sampled_prepared)
    hipLaunchKernelGGL(rm::rm_optimizer_post_small, dim3(1), dim3(256), 0, ctx->stream, raw_packed, grad_act_packed,
                       adam_m, adam_v, M, lr, weight_decay, act_out, reinterpret_cast<_Float16*>(colors_f16_out),
                       ctx->opt_pre.as<const float>());
    RM_HIP(ctx, hipGetLastError());
    return RM_OK;
  }
  if (M <= rm::kOptSmallMaxM && !env_is("RM_OPT_SMALL", '0')) {  // one block: snapshot, repulsion rows, update
    hipLaunchKernelGGL(rm::rm_optimizer_small, dim3(1), dim3(256), 0, ctx->stream, raw_packed, grad_act_packed, adam_m,
                       adam_v, M, step, lr, weight_decay, with_penalties ? 1 : 0, loss_penalty, act_out,
                       reinterpret_cast<_Float16*>(colors_f16_out), ctx->sdev);
    RM_HIP(ctx, hipGetLastError());
    return RM_OK;
  }
  // workspace: snapshot of the pre-step params | repulsion rows [M][4] | penalty partials
  const size_t need = ((size_t)n + 4 * (size_t)M + (size_t)nb + 64) * sizeof(float);
  int rc = ctx->ws.ensure(ctx, need, "workspace");
  if (rc != RM_OK) return rc;
  float* snap = ctx->ws.as<float>();
  float* pair = snap + n;
  float* parts = loss_penalty ? pair + 4 * M : nullptr;
  hipLaunchKernelGGL(rm::rm_penalty_pairs, dim3(M), dim3(256), 0, ctx->stream, raw_packed, M,
                     with_penalties ? 1 : 0, snap, pair);
  RM_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(rm::rm_optimizer_kernel, dim3(nb), dim3(256), 0, ctx->stream, snap, raw_packed,
                     grad_act_packed, adam_m, adam_v, pair, M, step, lr, weight_decay, with_penalties ? 1 : 0, parts,
                     act_out, reinterpret_cast<_Float16*>(colors_f16_out), ctx->sdev);
  RM_HIP(ctx, hipGetLastError());
  if (ctx->sdev) {
    hipLaunchKernelGGL(rm::rm_step_advance, dim3(1), dim3(64), 0, ctx->stream, ctx->sdev);
    RM_HIP(ctx, hipGetLastError());
  }
  if (loss_penalty) {
    hipLaunchKernelGGL(rm::rm_sum_small, dim3(1), dim3(64), 0, ctx->stream, parts, nb, loss_penalty);
    RM_HIP(ctx, hipGetLastError());
  }
  return RM_OK;
}

int rm_optimizer_step(rm_context* ctx, float* raw_packed, const float* grad_act_packed, float* adam_m,
                      float* adam_v, int32_t num_spheres, int32_t step, float lr, float weight_decay,
                      int32_t with_penalties, float* loss_penalty, float* act_out) {
  return rm_optimizer_step_f16(ctx, raw_packed, grad_act_packed, adam_m, adam_v, num_spheres, step, lr, weight_decay,
                               with_penalties, loss_penalty, act_out, nullptr);
}

int rm_train_step_camera_adam(rm_context* ctx, const rm_camera* cams, int32_t num_views, int32_t width,
                              int32_t height, const float* targets, float progress, float inv_count,
                              const rm_march* march, float* act_packed, float* grad_packed, float* raw_packed,
                              float* adam_m, float* adam_v, int32_t num_spheres, int32_t step, float lr,
                              float weight_decay, int32_t with_penalties, float* loss_sum, float* loss_penalty,
                              uint16_t* colors_f16_out) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  ctx->opt_prepared = false;
  if (!act_packed || !grad_packed || !raw_packed || !adam_m || !adam_v || !march)
    return fail(ctx, RM_ERR_INVALID_ARG, "NULL model buffer");
  if (num_spheres < 1 || num_spheres > RM_MAX_SPHERES) return fail(ctx, RM_ERR_INVALID_ARG, "bad num_spheres");
  const bool f16 = (march->flags & RM_MARCH_COLOR_F16) != 0;
  if (f16 != (colors_f16_out != nullptr))
    return fail(ctx, RM_ERR_INVALID_ARG, "colors_f16_out goes with RM_MARCH_COLOR_F16 (and only with it)");
  if (step < 1 && !ctx->sdev) return fail(ctx, RM_ERR_INVALID_ARG, "step counts from 1");
  const int M = num_spheres;
  rm_scene sc;
  rm_scene_from_packed(act_packed, M, &sc);
  if (f16) sc.colors = reinterpret_cast<const float*>(colors_f16_out);  // the fp16 colours the step renders
  rm_grads gr;
  rm_grads_from_packed(grad_packed, M, &gr);
  Call c = camera_call(kTrain, cams, num_views, width, height, &sc, march);
  set_training(c, targets, progress, inv_count, &gr, loss_sum, 0);
  const Call::Adam ad{raw_packed, adam_m, adam_v, act_packed, loss_penalty, reinterpret_cast<_Float16*>(colors_f16_out),
                      step, with_penalties ? 1 : 0, lr, weight_decay};
  c.adam = &ad;
  ctx->adam_done = false;
  int rc = run(ctx, c);
  const bool done = ctx->adam_done;
  ctx->adam_done = false;
  if (rc != RM_OK || done) return rc;
  // not fused (more than 64 spheres, the small-scene kernel, sub-launches): the optimizer call
  return rm_optimizer_step_f16(ctx, raw_packed, grad_packed, adam_m, adam_v, M, step, lr, weight_decay,
                               with_penalties, loss_penalty, act_packed, colors_f16_out);
}

int rm_train_step_sampled(rm_context* ctx, const float* ray_org, const float* ray_dir, const float* targets,
                          int64_t num_src, const int32_t* fg_indices, int64_t num_fg, int64_t n_uniform,
                          int64_t n_fg, uint64_t seed, uint64_t stream, uint64_t counter, float progress,
                          float inv_count, const rm_scene* scene, const rm_march* march, const rm_grads* grads,
                          float* loss_sum) {
  return sampled_step(ctx, ray_org, ray_dir, targets, num_src, fg_indices, num_fg, n_uniform, n_fg, seed, stream,
                      counter, progress, inv_count, scene, march, grads, loss_sum, nullptr, 0, 0, nullptr);
}

int rm_train_step_sampled_prepared(rm_context* ctx, const float* ray_org, const float* ray_dir, const float* targets,
                                   int64_t num_src, const int32_t* fg_indices, int64_t num_fg, int64_t n_uniform,
                                   int64_t n_fg, uint64_t seed, uint64_t stream, uint64_t counter, float progress,
                                   float inv_count, const rm_scene* scene, const rm_march* march,
                                   const rm_grads* grads, float* loss_sum, const float* raw_packed, int32_t step,
                                   int32_t with_penalties, float* loss_penalty) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  if (!raw_packed) return fail(ctx, RM_ERR_INVALID_ARG, "NULL raw parameters");
  if (step < 1) return fail(ctx, RM_ERR_INVALID_ARG, "step counts from 1");
  if (ctx->sdev) return fail(ctx, RM_ERR_INVALID_ARG, "prepared steps do not take bound step scalars");
  return sampled_step(ctx, ray_org, ray_dir, targets, num_src, fg_indices, num_fg, n_uniform, n_fg, seed, stream,
                      counter, progress, inv_count, scene, march, grads, loss_sum, raw_packed, step, with_penalties,
                      loss_penalty);
}

int rm_train_iteration(rm_context* ctx, const float* ray_org, const float* ray_dir, const float* targets,
                       int64_t num_src, const int32_t* fg_indices, int64_t num_fg, int64_t n_uniform, int64_t n_fg,
                       uint64_t seed, uint64_t stream, uint64_t counter, float progress, float inv_count,
                       const rm_march* march, float* act_packed, float* grad_packed, float* raw_packed,
                       float* adam_m, float* adam_v, int32_t num_spheres, int32_t step, float lr,
                       float weight_decay, int32_t with_penalties, float* loss_sum, float* loss_penalty) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  ctx->opt_prepared = false;
  int rc;
  if ((rc = check_sampling(ctx, ray_org, ray_dir, targets, num_src, fg_indices, num_fg, n_uniform, n_fg)) != RM_OK)
    return rc;
  if (!act_packed || !grad_packed || !raw_packed || !adam_m || !adam_v || !march)
    return fail(ctx, RM_ERR_INVALID_ARG, "NULL model buffer");
  if (num_spheres < 1 || num_spheres > RM_MAX_SPHERES) return fail(ctx, RM_ERR_INVALID_ARG, "bad num_spheres");
  if ((march->flags & RM_MARCH_COLOR_F16) != 0)
    return fail(ctx, RM_ERR_INVALID_ARG, "rm_train_iteration trains fp32 colour models");
  if (step < 1 && !ctx->sdev) return fail(ctx, RM_ERR_INVALID_ARG, "step counts from 1");
  const int M = num_spheres;
  const long long n = n_uniform + n_fg;
  rm_scene sc;
  rm_scene_from_packed(act_packed, M, &sc);
  rm_grads gr;
  rm_grads_from_packed(grad_packed, M, &gr);
  Call c = ray_call(kTrain, ray_org, ray_dir, n, &sc, march);
  set_training(c, targets, progress, inv_count, &gr, loss_sum, 0);
  // one launch: the small kernel with its in-kernel final reduction (RM_FUSED_ITER=0: three calls)
  const bool fused = sampled_one_launch(c, M, n) && M <= kOptSmallMaxM && ctx->sdev == nullptr;
  if (fused) {
    SmallArgs fz = sampling_args(ray_org, ray_dir, targets, num_src, fg_indices, num_fg, n_uniform, seed, stream, counter);
    fz.raw = raw_packed;
    fz.m1 = adam_m;
    fz.m2 = adam_v;
    fz.step = step;
    fz.with_pen = with_penalties ? 1 : 0;
    fz.lr = lr;
    fz.wd = weight_decay;
    fz.loss_penalty = loss_penalty;
    fz.act_out = act_packed;
    fz.adam = 1;
    c.fused = &fz;
    return run(ctx, c);
  }
  // the same three steps as separate calls: draw + gather, train step, optimizer
  if ((rc = sample_then_train(ctx, ray_org, ray_dir, targets, num_src, fg_indices, num_fg, n_uniform, n_fg, seed,
                              stream, counter, progress, inv_count, &sc, march, &gr, loss_sum)) != RM_OK)
    return rc;
  return rm_optimizer_step(ctx, raw_packed, grad_packed, adam_m, adam_v, M, step, lr, weight_decay, with_penalties,
                           loss_penalty, act_packed);
}

int rm_render_diff_backward_rays(rm_context* ctx, const float* ray_org, const float* ray_dir, int64_t num_rays,
                                 const rm_scene* scene, const rm_march* march, const float* grad_out,
                                 const float* t_march, float* grad_org, float* grad_dir, int32_t accumulate) {
  RayGradCall c(ray_geometry(ray_org, ray_dir, num_rays, scene, march));
  c.gout = grad_out;
  c.t_in = t_march;
  c.g_org = grad_org;
  c.g_dir = grad_dir;
  c.accumulate = accumulate;
  return run_raygrad(ctx, c);
}

int rm_render_diff_backward_cameras(rm_context* ctx, const rm_camera* cams, int32_t num_views, int32_t width,
                                    int32_t height, const rm_scene* scene, const rm_march* march,
                                    const float* grad_out, const float* t_march, rm_camera* grad_cams,
                                    int32_t accumulate) {
  RayGradCall c(camera_geometry(cams, num_views, width, height, scene, march));
  c.gout = grad_out;
  c.t_in = t_march;
  c.grad_cams = grad_cams;
  c.accumulate = accumulate;
  return run_raygrad(ctx, c);
}

int rm_render_diff_sh(rm_context* ctx, const float* ray_org, const float* ray_dir, int64_t num_rays,
                      const rm_scene* scene, const float* sh, int32_t sh_degree, const rm_march* march, float* out,
                      float* t_march) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  int rc;
  if ((rc = check_sh(ctx, sh, sh_degree)) != RM_OK) return rc;
  if (sh_degree == 0) return rm_render_diff(ctx, ray_org, ray_dir, num_rays, scene, march, out, t_march);
  return run_sh_forward(ctx, sh_forward_call(ray_geometry(ray_org, ray_dir, num_rays, scene, march), sh, sh_degree, out, t_march));
}

int rm_render_diff_sh_camera(rm_context* ctx, const rm_camera* cams, int32_t num_views, int32_t width, int32_t height,
                             const rm_scene* scene, const float* sh, int32_t sh_degree, const rm_march* march,
                             float* out, float* t_march) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  int rc;
  if ((rc = check_sh(ctx, sh, sh_degree)) != RM_OK) return rc;
  if (sh_degree == 0) return rm_render_diff_camera(ctx, cams, num_views, width, height, scene, march, out, t_march);
  return run_sh_forward(ctx, sh_forward_call(camera_geometry(cams, num_views, width, height, scene, march), sh, sh_degree, out,
                                             t_march));
}

int rm_render_diff_sh_backward(rm_context* ctx, const float* ray_org, const float* ray_dir, int64_t num_rays,
                               const rm_scene* scene, const float* sh, int32_t sh_degree, const rm_march* march,
                               const float* grad_out, const float* t_march, const rm_grads* grads, float* grad_sh,
                               int32_t accumulate) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  int rc;
  if ((rc = check_sh(ctx, sh, sh_degree)) != RM_OK) return rc;
  if (sh_degree == 0)
    return rm_render_diff_backward(ctx, ray_org, ray_dir, num_rays, scene, march, grad_out, t_march, grads, accumulate);
  return run_sh_backward(ctx, sh_backward_call(ray_geometry(ray_org, ray_dir, num_rays, scene, march), sh, sh_degree, grad_out,
                                               t_march, grads, grad_sh, accumulate));
}

int rm_render_diff_sh_backward_camera(rm_context* ctx, const rm_camera* cams, int32_t num_views, int32_t width,
                                      int32_t height, const rm_scene* scene, const float* sh, int32_t sh_degree,
                                      const rm_march* march, const float* grad_out, const float* t_march,
                                      const rm_grads* grads, float* grad_sh, int32_t accumulate) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  int rc;
  if ((rc = check_sh(ctx, sh, sh_degree)) != RM_OK) return rc;
  if (sh_degree == 0)
    return rm_render_diff_backward_camera(ctx, cams, num_views, width, height, scene, march, grad_out, t_march, grads,
                                          accumulate);
  return run_sh_backward(ctx, sh_backward_call(camera_geometry(cams, num_views, width, height, scene, march), sh, sh_degree,
                                               grad_out, t_march, grads, grad_sh, accumulate));
}

void rm_image_loss_default(rm_image_loss_params* p) {
  if (!p) return;
  p->l1_weight = 0.8f;    // 3D Gaussian splatting's lambda = 0.2
  p->ssim_weight = 0.2f;
  p->progress = 0.0f;
  p->c1 = 1e-4f;          // 0.01^2
  p->c2 = 9e-4f;          // 0.03^2
  p->flags = 0;
}

int rm_image_loss(rm_context* ctx, const float* out, const float* targets, int32_t num_views, int32_t width,
                  int32_t height, float inv_count, const rm_image_loss_params* params, float* loss, float* view_stats,
                  float* ssim_map, float* grad_out) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  return run_image_loss(ctx, out, targets, num_views, width, height, inv_count, params, loss, view_stats, ssim_map,
                        grad_out);
}

void rm_view_params_default(rm_view_params* p) {
  if (!p) return;
  p->max_steps = 100;          // shader.wgsl MAX_STEPS
  p->smooth_k = 32.0f;         // viewer.rs smooth_k
  p->hit_eps = 1e-3f;          // shader.wgsl: d < 0.001
  p->t_max = 20.0f;            // shader.wgsl: t > 20.0
  p->normal_eps = 1e-3f;       // shader.wgsl calc_normal
  p->color_sharpness = 10.0f;  // shader.wgsl: exp(-10 d)
  p->focal = 1.5f;             // shader.wgsl: 1.5 * ww
  p->flags = 0;
}

int rm_view(rm_context* ctx, const rm_view_camera* cams, int32_t num_frames, int32_t width, int32_t height,
            const rm_scene* scene, const rm_view_params* params, float* out_rgb, uint8_t* out_rgba8,
            float* out_depth) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  rm_view_params vp;
  rm_view_params_default(&vp);
  if (params) vp = *params;
  if (!cams) return fail(ctx, RM_ERR_INVALID_ARG, "cams is NULL");
  if (num_frames < 1 || num_frames > RM_MAX_VIEWS_PER_CALL)
    return fail(ctx, RM_ERR_INVALID_ARG, "num_frames %d out of [1, %d]", num_frames, RM_MAX_VIEWS_PER_CALL);
  if (width < 1 || height < 1 || (long long)width * height > (1LL << 28))
    return fail(ctx, RM_ERR_INVALID_ARG, "bad frame size %dx%d", width, height);
  if (vp.max_steps < 1) return fail(ctx, RM_ERR_INVALID_ARG, "max_steps %d < 1", vp.max_steps);
  if (!out_rgb && !out_rgba8 && !out_depth) return fail(ctx, RM_ERR_INVALID_ARG, "no output requested");
  if ((reinterpret_cast<uintptr_t>(out_rgba8) & 3) != 0) return fail(ctx, RM_ERR_INVALID_ARG, "out_rgba8 is not 4-byte aligned");
  if (!std::isfinite(vp.focal) || !std::isfinite(vp.hit_eps) || !std::isfinite(vp.color_sharpness))
    return fail(ctx, RM_ERR_INVALID_ARG, "focal, hit_eps and color_sharpness must be finite");
  return run_view(ctx, cams, num_frames, width, height, scene, vp, out_rgb, out_rgba8, out_depth);
}

void rm_sdf_params_default(rm_sdf_params* p) {
  if (!p) return;
  p->smooth_k = 32.0f;         // train.rs:131 MAX_SMOOTH, the k of the previews and the viewer
  p->color_sharpness = 10.0f;  // renderer_diff.rs:74
  p->flags = 0;
}

int rm_sdf_query(rm_context* ctx, const float* points, int64_t num_points, const rm_scene* scene,
                 const rm_sdf_params* params, float* dist, float* grad, float* color) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  rm_sdf_params sp;
  int rc;
  if ((rc = check_sdf_params(ctx, params, sp)) != RM_OK) return rc;
  if (num_points < 0) return fail(ctx, RM_ERR_INVALID_ARG, "num_points %lld < 0", (long long)num_points);
  if (!dist && !grad && !color) return fail(ctx, RM_ERR_INVALID_ARG, "no output requested");
  if (num_points > 0 && !points) return fail(ctx, RM_ERR_INVALID_ARG, "points is NULL");
  return run_sdf(ctx, false, points, num_points, nullptr, 0.0f, 0, 0, scene, sp, dist, grad, color);
}

int rm_sdf_query_backward(rm_context* ctx, const float* points, int64_t num_points, const rm_scene* scene,
                          const rm_sdf_params* params, const float* grad_dist, const float* grad_color,
                          const rm_grads* grads, float* grad_points, int32_t accumulate) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  rm_sdf_params sp;
  int rc;
  if ((rc = check_sdf_params(ctx, params, sp)) != RM_OK) return rc;
  if (num_points < 0) return fail(ctx, RM_ERR_INVALID_ARG, "num_points %lld < 0", (long long)num_points);
  if (!grad_dist && !grad_color) return fail(ctx, RM_ERR_INVALID_ARG, "grad_dist and grad_color are both NULL");
  // the field does not depend on the light: those two members are never written
  rm_grads want{};
  if (grads) {
    want.centers = grads->centers;
    want.colors = grads->colors;
    want.radius = grads->radius;
  }
  const bool scene_grad = want.centers || want.colors || want.radius;
  if (!scene_grad && !grad_points) return fail(ctx, RM_ERR_INVALID_ARG, "no output requested");
  if (num_points > 0 && !points) return fail(ctx, RM_ERR_INVALID_ARG, "points is NULL");
  return run_sdf_grad(ctx, points, num_points, scene, sp, grad_dist, grad_color, scene_grad ? &want : nullptr,
                      grad_points, accumulate);
}

int rm_sdf_grid(rm_context* ctx, const float origin[3], float spacing, int32_t nx, int32_t ny, int32_t nz,
                const rm_scene* scene, const rm_sdf_params* params, float* dist, float* color) {
  if (!ctx) return RM_ERR_INVALID_ARG;
  rm_sdf_params sp;
  int rc;
  if ((rc = check_sdf_params(ctx, params, sp)) != RM_OK) return rc;
  if (!origin || !std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2]))
    return fail(ctx, RM_ERR_INVALID_ARG, "origin must be three finite floats");
  if (!(spacing > 0.0f) || !std::isfinite(spacing))
    return fail(ctx, RM_ERR_INVALID_ARG, "spacing must be finite and > 0 (got %g)", (double)spacing);
  if (nx < 1 || ny < 1 || nz < 1 || (long long)nx * ny > (1LL << 34) / nz)
    return fail(ctx, RM_ERR_INVALID_ARG, "bad grid extents %dx%dx%d", nx, ny, nz);
  if (!dist && !color) return fail(ctx, RM_ERR_INVALID_ARG, "no output requested");
  return run_sdf(ctx, true, nullptr, (long long)nx * ny * nz, origin, spacing, nx, ny, scene, sp, dist, nullptr, color);
}

}  // extern "C"
