// librm_host.so, part 3: the GPU-driving programs of the reference, over the C ABI of
// libraymarch_hip.so: the multi-stage training driver (train.rs:23-330), the preview
// (train.rs:335-366) and the target generator (generate.rs:20-112).
#include <hip/hip_runtime_api.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>

#include "raymarch.h"
#include "rmh_common.hpp"

using namespace rmh;

namespace {

#define RMCHK(ctx, call)                                                                        \
  do {                                                                                          \
    int r_ = (call);                                                                            \
    if (r_ != RM_OK) return fail(RMH_ERR_GPU, "%s: %s", #call, rm_last_error(ctx));             \
  } while (0)

// A rank that leaves rmh_train with an error releases its side of the collectives
// (rmh_collective.abort: the RCCL one aborts its communicator). The other ranks learn of it through
// their own watchdog (rmh_collective.wait at every synchronisation point of the driver) or from
// the launcher, which ends the remaining ranks when one fails.
struct AbortOnError {
  const rmh_collective* comm = nullptr;
  bool done = false;
  ~AbortOnError() {
    if (!done && comm && comm->world > 1 && comm->abort) comm->abort(comm->state);
  }
};

// One rm_context + stream for a driver call.
struct Gpu {
  hipStream_t stream = nullptr;
  rm_context* ctx = nullptr;
  ~Gpu() {
    if (ctx) rm_destroy(ctx);
    if (stream) (void)hipStreamDestroy(stream);
  }
  int open(int device) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    if (rm_create(device, stream, &ctx) != RM_OK) return fail(RMH_ERR_GPU, "rm_create(device %d) failed", device);
    return RMH_OK;
  }
};

// Training steps a rank enqueues ahead of the GPU when it runs with collectives (rmh_train).
constexpr int32_t kStepsInFlight = 32;

// Waits for the driver's stream: through the collective's watchdog when collectives may be in
// flight (a dead peer then ends in an error instead of a hang), else hipStreamSynchronize.
int sync_stream(const Gpu& g, const rmh_collective* comm) {
  if (comm && comm->wait) {
    const int rc = comm->wait(comm->state, g.stream);
    if (rc != RMH_OK) {
      const std::string why = rmh_last_error();
      return fail(rc, "waiting for the stream: %s", why.c_str());
    }
    return RMH_OK;
  }
  HIPCHK(hipStreamSynchronize(g.stream));
  return RMH_OK;
}

bool file_exists(const std::string& p) {
  FILE* f = std::fopen(p.c_str(), "rb");
  if (!f) return false;
  std::fclose(f);
  return true;
}

// cameras.json names files relative to the reference's working directory ("data/target_0.png");
// try that, then relative to the json's directory, then the bare file name next to the json.
std::string resolve_image(const std::string& json_path, const std::string& file) {
  if (file_exists(file)) return file;
  const std::string dir = dirname_of(json_path);
  const std::string a = join_path(dir, file);
  if (file_exists(a)) return a;
  const size_t s = file.rfind('/');
  return join_path(dir, s == std::string::npos ? file : file.substr(s + 1));
}

void camera_struct(rm_camera& c, const float eye[3], const float target[3], float fov) {
  for (int k = 0; k < 3; ++k) {
    c.eye[k] = eye[k];
    c.target[k] = target[k];
  }
  c.fov_deg = fov;
}

// One camera's render_diff image as a file: the whole image in one camera-mode launch (the
// reference chunks 4096 rays only to save VRAM), copied to the host, waited for and saved.
int render_to_file(Gpu& g, const rm_scene& sc, const rm_march& m, const rm_camera& cam, int32_t W, int32_t H,
                   const char* path) {
  DevBuf out;
  HIPCHK(out.alloc(sizeof(float) * 3 * (size_t)W * H));
  RMCHK(g.ctx, rm_render_diff_camera(g.ctx, &cam, 1, W, H, &sc, &m, out.f(), nullptr));
  std::vector<float> host(3 * (size_t)W * H);
  HIPCHK(hipMemcpyAsync(host.data(), out.p, out.bytes, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  return rmh_image_save(path, host.data(), W, H);
}

// train.rs:210-262: centers raw, colours sigmoid, radii softplus (no +0.01), light raw,
// ambient sigmoid.
int export_scene(const std::vector<float>& raw, int32_t M, const std::string& path) {
  std::vector<float> col(3 * (size_t)M), rad(M);
  for (int32_t i = 0; i < 3 * M; ++i) col[i] = sigmoid_f32(raw[3 * M + i]);
  for (int32_t i = 0; i < M; ++i) rad[i] = softplus_f32(raw[6 * M + i]);
  const float amb = sigmoid_f32(raw[7 * M + 3]);
  return rmh_scene_save(path.c_str(), M, raw.data(), col.data(), rad.data(), raw.data() + 7 * M, &amb);
}

// scene.json for rmh_preview / rmh_view as the activated packed buffer [centers | colours | radii +
// offset | light | ambient] on the device of `g`, which opens once the file has parsed. `act` is
// the caller's: the asynchronous upload reads it.
int load_scene(const char* scene_json, float radius_offset, int32_t device, Gpu& g, std::vector<float>& act,
               DevBuf& d_act, rm_scene* sc) {
  int32_t M = 0;
  float *c = nullptr, *col = nullptr, *r = nullptr, ld[3], amb = 0.0f;
  int rc = rmh_scene_load(scene_json, &M, &c, &col, &r, ld, &amb);
  if (rc) return rc;
  std::unique_ptr<float, void (*)(void*)> g1(c, std::free), g2(col, std::free), g3(r, std::free);
  if (M < 1) return fail(RMH_ERR_FORMAT, "%s has no sphere", scene_json);
  act.resize(7 * (size_t)M + 4);
  std::memcpy(act.data(), c, sizeof(float) * 3 * M);
  std::memcpy(act.data() + 3 * M, col, sizeof(float) * 3 * M);
  for (int32_t i = 0; i < M; ++i) act[6 * M + i] = r[i] + radius_offset;  // viewer.rs draws the stored radii
  std::memcpy(act.data() + 7 * M, ld, sizeof ld);
  act[7 * M + 3] = amb;
  if ((rc = g.open(device)) != RMH_OK) return rc;
  HIPCHK(d_act.alloc(sizeof(float) * act.size()));
  HIPCHK(hipMemcpyAsync(d_act.p, act.data(), d_act.bytes, hipMemcpyHostToDevice, g.stream));
  rm_scene_from_packed(d_act.f(), M, sc);
  return RMH_OK;
}

// ---- rmh_train's phases, in the order of train.rs ----

bool leads(const rmh_collective* comm) { return !comm || comm->rank == 0; }  // logs, previews and scene.json

// rank q's share of the batch (B/P rays per rank, the remainder spread)
int32_t batch_share(const rmh_train_config* cfg, int32_t world, int32_t q) {
  return cfg->batch / world + (q < cfg->batch % world ? 1 : 0);
}

// The training set (train.rs:62-96). The host arrays stay: the asynchronous uploads read them.
struct TrainSet {
  std::vector<float> h_org, h_dir, h_tgt;
  std::unique_ptr<rmh_dataset, void (*)(rmh_dataset*)> ds{nullptr, rmh_dataset_destroy};
  DevBuf d_org, d_dir, d_tgt, d_fg;  // d_fg: the foreground list of the dataset, for the device sampler
  int64_t P = 0, n_fg_list = 0;
  // Opens `g` once the files have loaded.
  int load(const rmh_train_config* cfg, Gpu& g, bool verbose) {
    const int32_t W = cfg->width, H = cfg->height;
    rmh_camera_entry* cams = nullptr;
    int32_t ncam = 0;
    int rc = rmh_cameras_load(cfg->cameras_json, &cams, &ncam);
    if (rc) return rc;
    std::unique_ptr<rmh_camera_entry, void (*)(void*)> cams_guard(cams, std::free);
    if (ncam < 1) return fail(RMH_ERR_FORMAT, "%s holds no camera", cfg->cameras_json);
    const int64_t per_view = (int64_t)W * H;
    P = per_view * ncam;
    h_org.resize(3 * P), h_dir.resize(3 * P), h_tgt.resize(3 * P);
    for (int32_t v = 0; v < ncam; ++v) {
      rmh_camera_rays(W, H, cams[v].origin, cams[v].target, cams[v].fov, h_org.data() + 3 * per_view * v,
                      h_dir.data() + 3 * per_view * v);
      const std::string img = resolve_image(cfg->cameras_json, cams[v].file);
      int32_t iw = 0, ih = 0;
      float* lin = nullptr;
      if ((rc = rmh_image_load(img.c_str(), &iw, &ih, &lin)) != RMH_OK) return rc;
      std::unique_ptr<float, void (*)(void*)> lin_guard(lin, std::free);
      if (iw != W || ih != H) return fail(RMH_ERR_FORMAT, "%s is %dx%d, expected %dx%d", img.c_str(), iw, ih, W, H);
      std::memcpy(h_tgt.data() + 3 * per_view * v, lin, sizeof(float) * 3 * per_view);
    }
    rmh_dataset* ds_raw = nullptr;
    if ((rc = rmh_dataset_create(h_tgt.data(), P, &ds_raw)) != RMH_OK) return rc;
    ds.reset(ds_raw);
    int64_t nfg = 0, nbg = 0;
    rmh_dataset_counts(ds.get(), &nfg, &nbg);
    if (verbose) {
      std::printf("Total training pixels: %lld\n", (long long)P);
      std::printf("Foreground pixels: %lld, Background pixels: %lld\n", (long long)nfg, (long long)nbg);
    }
    if ((rc = g.open(cfg->device)) != RMH_OK) return rc;
    HIPCHK(d_org.alloc(sizeof(float) * 3 * P));
    HIPCHK(d_dir.alloc(sizeof(float) * 3 * P));
    HIPCHK(d_tgt.alloc(sizeof(float) * 3 * P));
    HIPCHK(hipMemcpyAsync(d_org.p, h_org.data(), d_org.bytes, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(d_dir.p, h_dir.data(), d_dir.bytes, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(d_tgt.p, h_tgt.data(), d_tgt.bytes, hipMemcpyHostToDevice, g.stream));
    const int32_t* h_fg = nullptr;  // owned by ds
    rmh_dataset_fg(ds.get(), &h_fg, &n_fg_list);
    HIPCHK(d_fg.alloc(sizeof(int32_t) * (size_t)std::max<int64_t>(n_fg_list, 1)));
    if (n_fg_list > 0)
      HIPCHK(hipMemcpyAsync(d_fg.p, h_fg, sizeof(int32_t) * n_fg_list, hipMemcpyHostToDevice, g.stream));
    return RMH_OK;
  }
};

// The schedule arithmetic of one step, as plain numbers: no allocation, no output.
struct StepPlan {
  float global_step, progress;  // float, as train.rs has them; the sampler's counter is (uint64_t)global_step
  float smooth_k, uniform_ratio, inv_count;
  int64_t n_uni, n_boost, n_global;  // this rank's draw; every rank's draws together
  double lr;
  bool last, read_loss;
};

StepPlan plan_step(const rmh_train_config* cfg, const rmh_dataset* ds, int32_t stage, int32_t step, int32_t world,
                   int32_t rank, double base_lr) {
  StepPlan p{};
  p.global_step = (float)(stage * cfg->steps_per_stage + step);
  p.progress = p.global_step / (float)(cfg->stages * cfg->steps_per_stage);
  p.smooth_k = 5.0f + (cfg->max_smooth - 5.0f) * p.progress;  // train.rs:174
  p.uniform_ratio = 0.8f - 0.4f * p.progress;                  // train.rs:176
  // the count rule of sample_batch (dataset.rs:47-82) on every rank's share: the global ray count
  // of this step and this rank's own draw (the device draws and gathers)
  for (int32_t q = 0; q < world; ++q) {
    int64_t qu = 0, qf = 0;
    rmh_dataset_sample_count(ds, batch_share(cfg, world, q), p.uniform_ratio, &qu, &qf);
    p.n_global += qu + qf;
    if (q == rank) p.n_uni = qu, p.n_boost = qf;
  }
  // model.forward + compute_loss + backward (train.rs:182-190), mean over the n*3 elements
  p.inv_count = 1.0f / (3.0f * (float)p.n_global);
  p.lr = step > cfg->steps_per_stage / 2 ? base_lr * 0.2 : base_lr;  // train.rs:193-197
  p.last = stage == cfg->stages - 1 && step == cfg->steps_per_stage;
  p.read_loss = (cfg->log_every > 0 && rank == 0 && step % cfg->log_every == 0) || p.last;
  return p;
}

// One generation's device state, freed when the stage's scope ends: after the stage's last wait.
struct Stage {
  int32_t M = 0;
  size_t np = 0;  // 7 M + 4
  // d_grad: [packed gradient (np) | loss sum | penalty]: the first np + 1 floats are the one all-reduce
  DevBuf d_raw, d_act, d_grad, d_m, d_v, d_col_h;
  float* d_loss = nullptr;     // d_grad + np
  std::vector<_Float16> half;  // fp16-colour models: the activated colours the renders read (d_col_h), on the host
  rm_scene sc;
  rm_grads gr;
  rm_march march;
  std::vector<float> init_centers;
  // Leaves uploads on the stream that read `raw`: the caller waits before it changes `raw`.
  int begin(Gpu& g, const std::vector<float>& raw, int32_t M_, bool f16, int32_t B, int32_t march_steps) {
    M = M_;
    np = 7 * (size_t)M + 4;
    HIPCHK(d_raw.alloc(sizeof(float) * np));
    HIPCHK(d_act.alloc(sizeof(float) * np));
    HIPCHK(d_grad.alloc(sizeof(float) * (np + 2)));
    d_loss = d_grad.f() + np;
    HIPCHK(d_m.alloc(sizeof(float) * np));
    HIPCHK(d_v.alloc(sizeof(float) * np));
    HIPCHK(hipMemcpyAsync(d_raw.p, raw.data(), sizeof(float) * np, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemsetAsync(d_m.p, 0, d_m.bytes, g.stream));  // Adam re-created per stage (train.rs:160)
    HIPCHK(hipMemsetAsync(d_v.p, 0, d_v.bytes, g.stream));
    RMCHK(g.ctx, rm_scene_activate(g.ctx, d_raw.f(), M, d_act.f()));
    rm_scene_from_packed(d_act.f(), M, &sc);
    rm_grads_from_packed(d_grad.f(), M, &gr);
    rm_march_default(&march);
    march.steps = march_steps;
    if (f16) {
      std::vector<float> col(3 * (size_t)M);
      half = std::vector<_Float16>(col.size());
      HIPCHK(hipMemcpyAsync(col.data(), d_act.f() + 3 * M, sizeof(float) * col.size(), hipMemcpyDeviceToHost,
                            g.stream));
      HIPCHK(hipStreamSynchronize(g.stream));
      // round to nearest even, as torch's .half() and the optimizer's colors_f16_out do
      for (size_t i = 0; i < col.size(); ++i) half[i] = (_Float16)col[i];
      HIPCHK(d_col_h.alloc(sizeof(_Float16) * half.size()));
      HIPCHK(hipMemcpyAsync(d_col_h.p, half.data(), d_col_h.bytes, hipMemcpyHostToDevice, g.stream));
      sc.colors = (const float*)d_col_h.p;
      march.flags |= RM_MARCH_COLOR_F16;
    }
    RMCHK(g.ctx, rm_reserve(g.ctx, B, M));
    init_centers = std::vector<float>(raw.begin(), raw.begin() + 3 * M);
    return RMH_OK;
  }
};

// One step on the stream. The penalty share of the loss costs a summation launch: its pointer is
// passed only on the steps that read the loss.
int train_step(Gpu& g, const rmh_train_config* cfg, const rmh_collective* comm, const TrainSet& ts, Stage& st,
               const StepPlan& p, int32_t stage, int32_t step) {
  // batches: rank-distinct streams of the device sampler, one counter value per step
  const uint64_t sample_stream = 1 + 1000 * (uint64_t)(comm ? comm->rank : 0);
  float* penalty = p.read_loss ? st.d_loss + 1 : nullptr;
  st.march.smooth_k = p.smooth_k;
  if (!comm && !cfg->color_f16) {
    // one process, no collective: draw + render + backward + optimizer in one call (one launch for
    // the small models of the schedule)
    RMCHK(g.ctx, rm_train_iteration(g.ctx, ts.d_org.f(), ts.d_dir.f(), ts.d_tgt.f(), ts.P, ts.d_fg.i(), ts.n_fg_list,
                                    p.n_uni, p.n_boost, cfg->seed, sample_stream, (uint64_t)p.global_step, p.progress,
                                    p.inv_count, &st.march, st.d_act.f(), st.d_grad.f(), st.d_raw.f(), st.d_m.f(),
                                    st.d_v.f(), st.M, step, (float)p.lr, cfg->weight_decay, 1, st.d_loss, penalty));
    return RMH_OK;
  }
  // draw + render + backward (one launch for the small models, whose extra block also runs the
  // optimizer's gradient-independent part), then the all-reduce, then the update
  RMCHK(g.ctx, rm_train_step_sampled_prepared(g.ctx, ts.d_org.f(), ts.d_dir.f(), ts.d_tgt.f(), ts.P, ts.d_fg.i(),
                                              ts.n_fg_list, p.n_uni, p.n_boost, cfg->seed, sample_stream,
                                              (uint64_t)p.global_step, p.progress, p.inv_count, &st.sc, &st.march,
                                              &st.gr, st.d_loss, st.d_raw.f(), step, 1, penalty));
  if (comm) {
    const int rc = comm->all_reduce_sum(comm->state, st.d_grad.f(), (int64_t)st.np + 1, g.stream);
    if (rc != RMH_OK)
      return fail(rc, "all-reduce of the gradient (stage %d, step %d): %s", stage, step, rmh_last_error());
  }
  if (cfg->color_f16)
    RMCHK(g.ctx, rm_optimizer_step_f16(g.ctx, st.d_raw.f(), st.d_grad.f(), st.d_m.f(), st.d_v.f(), st.M, step,
                                       (float)p.lr, cfg->weight_decay, 1, penalty, st.d_act.f(),
                                       (uint16_t*)st.d_col_h.p));
  else
    RMCHK(g.ctx, rm_optimizer_step(g.ctx, st.d_raw.f(), st.d_grad.f(), st.d_m.f(), st.d_v.f(), st.M, step,
                                   (float)p.lr, cfg->weight_decay, 1, penalty, st.d_act.f()));
  return RMH_OK;
}

// The loss of a reporting step: into page-locked memory on the stream, one wait under the
// watchdog, then rank 0's log line (log_bits: with the two sums' bits, for diagnosis).
int report_loss(Gpu& g, const rmh_train_config* cfg, const rmh_collective* comm, const Stage& st, const StepPlan& p,
                int32_t step, const PinnedBuf& h_loss, bool log_bits, float* loss) {
  HIPCHK(hipMemcpyAsync(h_loss.p, st.d_loss, 2 * sizeof(float), hipMemcpyDeviceToHost, g.stream));
  if (const int rc = sync_stream(g, comm); rc != RMH_OK) return rc;
  const float* s = h_loss.f();
  *loss = s[0] * p.inv_count + s[1];  // training.rs:34 + penalties
  if (leads(comm) && cfg->log_every > 0 && step % cfg->log_every == 0) {
    std::printf("  Step %d | Loss: %.5f | k: %.1f", step, *loss, p.smooth_k);
    if (log_bits) {
      uint32_t b[2];
      std::memcpy(b, s, sizeof b);
      std::printf(" | bits %08x %08x", b[0], b[1]);
    }
    std::printf("\n");
  }
  return RMH_OK;
}

// The end of a stage (train.rs:206-290), entered when the host has issued the stage's steps: the
// last wait and the timing, the trained parameters into `raw` and to on_generation, rank 0's files.
int end_stage(Gpu& g, const rmh_train_config* cfg, const rmh_collective* comm, const Stage& st, int32_t stage,
              std::chrono::steady_clock::time_point t0, bool stage_times, std::vector<float>& raw, double* seconds) {
  const auto t_enq = std::chrono::steady_clock::now();
  int rc = sync_stream(g, comm);
  if (rc != RMH_OK) return rc;
  const auto t_end = std::chrono::steady_clock::now();
  *seconds += std::chrono::duration<double>(t_end - t0).count();
  if (stage_times)  // measurement: host issue vs drain
    std::fprintf(stderr, "stage %d: issued in %.3f ms, drained %.3f ms later\n", stage + 1,
                 1e3 * std::chrono::duration<double>(t_enq - t0).count(),
                 1e3 * std::chrono::duration<double>(t_end - t_enq).count());
  HIPCHK(hipMemcpy(raw.data(), st.d_raw.p, sizeof(float) * st.np, hipMemcpyDeviceToHost));
  if (cfg->on_generation) cfg->on_generation(cfg->user, stage, st.M, raw.data());
  const std::string out_dir = cfg->out_dir ? cfg->out_dir : "";
  if (!leads(comm) || out_dir.empty()) return RMH_OK;
  const bool final = stage == cfg->stages - 1;
  if (final) {
    if ((rc = export_scene(raw, st.M, join_path(out_dir, "scene.json"))) != RMH_OK) return rc;
    if (cfg->log_every > 0) std::printf("  => Saved to scene.json (N = %d)\n", st.M);
  }
  if (!cfg->previews) return RMH_OK;
  const std::string name = final ? "steps/final_1.png" : "steps/stage_" + std::to_string(stage) + ".png";
  // save_tiled_preview (train.rs:335-366): render_diff at k = 32 of the scene view and march the
  // stage trained with (an fp16-colour model previews with its fp16 colours)
  rm_march m = st.march;
  m.smooth_k = 32.0f;
  rm_camera cam;
  const float eye[3] = {0.0f, 0.0f, -2.5f}, tgt[3] = {0.0f, 0.0f, 0.0f};  // train.rs:37-44
  camera_struct(cam, eye, tgt, 50.0f);
  return render_to_file(g, st.sc, m, cam, cfg->width, cfg->height, join_path(out_dir, name).c_str());
}

// The next generation (prune & split, train.rs:300-328): `raw` and `M` become the next stage's.
// Rank 0 decides it (rng is consumed there only). With a collective it reaches every rank in two
// broadcasts on the stream, each followed by a wait under the watchdog:
//   1. one float, the size M'. It is exact (M' <= 2 M <= 2^17) and doubles as the status word:
//      -1 says that rank 0 failed in prune_and_split.
//   2. the 7 M' + 4 raw parameters.
// Rank 0 returns its own error only after broadcast 1 has told the others. One rank with a
// collective takes the same path as many (the RCCL path is the same). The size checks come last.
int next_generation(Gpu& g, const rmh_train_config* cfg, const rmh_collective* comm, const Stage& st, int32_t stage,
                    rmh_rng* rng, std::vector<float>& raw, int32_t* M) {
  // the growth knobs: 0 (a zeroed struct) = the reference's value, < 0 = no such condition
  // (rmh_prune_and_split_ex takes 0 for that) -- ADVICE r04: a zeroed config is the reference rule
  const float split_scale = cfg->split_scale == 0.0f ? 1.0f : std::max(cfg->split_scale, 0.0f);
  const float split_move = cfg->split_move == 0.0f ? 0.05f : std::max(cfg->split_move, 0.0f);
  std::vector<float> next(14 * (size_t)st.M + 4);
  int32_t nextM = 0;
  int rc, split_rc = RMH_OK;
  if (leads(comm))
    split_rc = rmh_prune_and_split_ex(raw.data(), st.M, st.init_centers.data(), stage, cfg->stages, split_scale,
                                      split_move, cfg->max_spheres, rng, next.data(), &nextM);
  if (split_rc != RMH_OK && !comm) return split_rc;
  if (comm) {
    DevBuf d_next;
    HIPCHK(d_next.alloc(sizeof(float) * next.size()));
    float fm = split_rc == RMH_OK ? (float)nextM : -1.0f;
    HIPCHK(hipMemcpyAsync(d_next.p, &fm, sizeof fm, hipMemcpyHostToDevice, g.stream));
    if ((rc = comm->broadcast(comm->state, d_next.f(), 1, 0, g.stream)) != RMH_OK)
      return fail(rc, "broadcast of the next size: %s", rmh_last_error());
    if ((rc = sync_stream(g, comm)) != RMH_OK) return rc;
    HIPCHK(hipMemcpy(&fm, d_next.p, sizeof fm, hipMemcpyDeviceToHost));
    nextM = (int32_t)fm;
    if (split_rc != RMH_OK) return split_rc;
    if (nextM < 0) return fail(RMH_ERR_GPU, "rank 0 failed in prune_and_split (stage %d)", stage);
    if (nextM < 1 || 7 * (size_t)nextM + 4 > next.size()) return fail(RMH_ERR_GPU, "broadcast size %d", nextM);
    const size_t nn = 7 * (size_t)nextM + 4;
    if (leads(comm))
      HIPCHK(hipMemcpyAsync(d_next.p, next.data(), sizeof(float) * nn, hipMemcpyHostToDevice, g.stream));
    if ((rc = comm->broadcast(comm->state, d_next.f(), (int64_t)nn, 0, g.stream)) != RMH_OK)
      return fail(rc, "broadcast of the next generation: %s", rmh_last_error());
    if ((rc = sync_stream(g, comm)) != RMH_OK) return rc;
    HIPCHK(hipMemcpy(next.data(), d_next.p, sizeof(float) * nn, hipMemcpyDeviceToHost));
  }
  if (nextM > RM_MAX_SPHERES) return fail(RMH_ERR_INVALID_ARG, "model grew past RM_MAX_SPHERES");
  next.resize(7 * (size_t)nextM + 4);
  raw.swap(next);
  *M = nextM;
  return RMH_OK;
}

}  // namespace

extern "C" {

void rmh_train_config_default(rmh_train_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof *c);
  c->cameras_json = "data/cameras.json";
  c->out_dir = ".";
  c->width = 256;
  c->height = 256;
  c->stages = 5;
  c->steps_per_stage = 700;
  c->batch = 16384;
  c->march_steps = 40;
  c->max_smooth = 32.0f;
  c->base_lr = 0.05f;
  c->weight_decay = 1e-5f;
  c->log_every = 100;
  c->previews = 1;
  c->seed = 0;
  c->device = 0;
  c->split_scale = 1.0f;   // training.rs:185
  c->split_move = 0.05f;   // training.rs:188
}

int rmh_train(const rmh_train_config* cfg, rmh_train_result* result, float* raw_out, int32_t raw_capacity) {
  if (!cfg || !cfg->cameras_json) return fail(RMH_ERR_INVALID_ARG, "NULL config");
  if (cfg->width < 1 || cfg->height < 1 || cfg->stages < 1 || cfg->steps_per_stage < 1 || cfg->batch < 1 ||
      cfg->march_steps < 1 || std::isnan(cfg->split_scale) || std::isnan(cfg->split_move) || cfg->max_spheres < 0)
    return fail(RMH_ERR_INVALID_ARG, "bad training configuration");
  const rmh_collective* comm = cfg->comm;
  const int32_t world = comm ? comm->world : 1, rank = comm ? comm->rank : 0;
  if (world < 1 || rank < 0 || rank >= world || (world > 1 && (!comm->all_reduce_sum || !comm->broadcast)))
    return fail(RMH_ERR_INVALID_ARG, "bad collective (rank %d of %d)", rank, world);
  if (cfg->batch < world) return fail(RMH_ERR_INVALID_ARG, "batch %d < %d ranks", cfg->batch, world);
  AbortOnError abort_guard{comm};  // from here on every error return releases this rank's side
  const bool verbose = cfg->log_every > 0 && rank == 0;
  const char *e_bits = std::getenv("RMH_LOG_BITS"), *e_times = std::getenv("RMH_STAGE_TIMES");
  const bool log_bits = e_bits && e_bits[0] == '1', stage_times = e_times && e_times[0] == '1';

  Gpu g;  // before the device buffers, which go first
  TrainSet ts;
  int rc = ts.load(cfg, g, verbose);
  if (rc != RMH_OK) return rc;
  rmh_rng rng_split;  // consumed on rank 0 only
  rmh_rng_seed(&rng_split, cfg->seed, 2);
  int32_t M = 7;  // initial model (train.rs:100-126)
  std::vector<float> raw(7 * M + 4);
  rmh_initial_model(raw.data());
  rmh_train_result res{};
  PinnedBuf h_loss;  // the loss sum and penalty read back on reporting steps
  HIPCHK(h_loss.alloc(2 * sizeof(float)));
  if (verbose) std::printf("Start Multi-Stage Optimization...\n");

  for (int32_t stage = 0; stage < cfg->stages; ++stage) {
    if (verbose) std::printf("=== Stage %d/%d (N = %d) ===\n", stage + 1, cfg->stages, M);
    Stage st;
    rc = st.begin(g, raw, M, cfg->color_f16 != 0, batch_share(cfg, world, rank), cfg->march_steps);
    if (rc != RMH_OK || (rc = sync_stream(g, comm)) != RMH_OK) return rc;  // set-up ends here: the steps are timed
    const double base_lr = (double)cfg->base_lr * std::pow(0.6, stage);  // train.rs:166
    const auto t0 = std::chrono::steady_clock::now();
    for (int32_t step = 1; step <= cfg->steps_per_stage; ++step) {
      const StepPlan plan = plan_step(cfg, ts.ds.get(), stage, step, world, rank, base_lr);
      if ((rc = train_step(g, cfg, comm, ts, st, plan, stage, step)) != RMH_OK) return rc;
      ++res.steps;
      // With collectives every rank drains its stream under the watchdog every kStepsInFlight
      // steps, not only where rank 0 reads the loss: a rank whose peer stopped then meets the
      // watchdog within kStepsInFlight steps instead of blocking inside a launch or ncclAllReduce
      // once the HIP queue fills, and the watchdog's timeout measures at most that many steps of
      // queued work, not a whole stage's backlog.
      if (comm && world > 1 && !plan.read_loss && step % kStepsInFlight == 0 && (rc = sync_stream(g, comm)) != RMH_OK)
        return rc;
      if (plan.read_loss &&
          (rc = report_loss(g, cfg, comm, st, plan, step, h_loss, log_bits, &res.final_loss)) != RMH_OK)
        return rc;
    }
    if ((rc = end_stage(g, cfg, comm, st, stage, t0, stage_times, raw, &res.seconds)) != RMH_OK) return rc;
    if (stage == cfg->stages - 1) break;
    if ((rc = next_generation(g, cfg, comm, st, stage, &rng_split, raw, &M)) != RMH_OK) return rc;
    if (verbose) std::printf("  => Pruning & Splitting complete. Next N = %d\n", M);
  }

  if (raw_out) {
    if (raw_capacity < 7 * M + 4) return fail(RMH_ERR_INVALID_ARG, "raw_out holds %d floats, need %d", raw_capacity,
                                              7 * M + 4);
    std::memcpy(raw_out, raw.data(), sizeof(float) * (7 * (size_t)M + 4));
  }
  abort_guard.done = true;
  res.num_spheres = M;
  res.step_ms = res.steps ? 1e3 * res.seconds / res.steps : 0.0;
  if (result) *result = res;
  return RMH_OK;
}

int rmh_preview(const char* scene_json, const char* png_path, int32_t W, int32_t H, const float eye[3],
                const float target[3], float fov_deg, float radius_offset, int32_t device) {
  if (!scene_json || !png_path || !eye || !target || W < 1 || H < 1) return fail(RMH_ERR_INVALID_ARG, "bad arguments");
  Gpu g;
  std::vector<float> act;
  DevBuf d_act;
  rm_scene sc;
  const int rc = load_scene(scene_json, radius_offset, device, g, act, d_act, &sc);
  if (rc) return rc;
  rm_march m;
  rm_march_default(&m);  // S = 40, k = 32 (train.rs:355)
  rm_camera cam;
  camera_struct(cam, eye, target, fov_deg);
  return render_to_file(g, sc, m, cam, W, H, png_path);
}

void rmh_view_camera(const float pos[3], float yaw, float pitch, rmh_view_pose* out) {
  if (!pos || !out) return;
  // viewer.rs:65-86 in f64, rounded once (cos(pi/2) must not leak 6e-17 into a unit vector's f32)
  auto normalize = [](double v[3]) {
    const double len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    for (int k = 0; k < 3; ++k) v[k] /= len;
  };
  double f[3] = {std::cos((double)yaw) * std::cos((double)pitch), std::sin((double)pitch),
                 std::sin((double)yaw) * std::cos((double)pitch)};
  normalize(f);
  double r[3] = {-f[2], 0.0, f[0]};  // forward x (0, 1, 0)
  normalize(r);
  double u[3] = {r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]};
  normalize(u);
  for (int k = 0; k < 3; ++k) {
    out->pos[k] = pos[k];
    out->forward[k] = (float)f[k];
    out->up[k] = (float)u[k];
  }
}

int rmh_view(const char* scene_json, const char* out_pattern, int32_t W, int32_t H, const rmh_view_pose* cams,
             int32_t count, float radius_offset, int32_t device) {
  static_assert(sizeof(rmh_view_pose) == sizeof(rm_view_camera), "rmh_view_pose is rm_view_camera");
  if (!scene_json || !out_pattern || !cams || W < 1 || H < 1 || count < 1)
    return fail(RMH_ERR_INVALID_ARG, "bad arguments");
  Gpu g;
  std::vector<float> act;
  DevBuf d_act, out;
  rm_scene sc;
  int rc = load_scene(scene_json, radius_offset, device, g, act, d_act, &sc);
  if (rc) return rc;
  const size_t per_frame = 4 * (size_t)W * H;
  const int32_t chunk_max = std::min<int32_t>(count, RM_MAX_VIEWS_PER_CALL);
  HIPCHK(out.alloc(per_frame * chunk_max));
  std::vector<uint8_t> host(per_frame * chunk_max);
  const std::string pat = out_pattern;
  const bool has_index = pat.find("%d") != std::string::npos;
  for (int32_t f0 = 0; f0 < count; f0 += chunk_max) {
    const int32_t nf = std::min(chunk_max, count - f0);
    RMCHK(g.ctx, rm_view(g.ctx, reinterpret_cast<const rm_view_camera*>(cams + f0), nf, W, H, &sc, nullptr, nullptr,
                         (uint8_t*)out.p, nullptr));
    HIPCHK(hipMemcpyAsync(host.data(), out.p, per_frame * nf, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    for (int32_t f = 0; f < nf; ++f) {
      std::string path = pat;
      const std::string idx = std::to_string(f0 + f);
      if (has_index) {
        path.replace(path.find("%d"), 2, idx);
      } else if (count > 1) {
        const size_t dot = path.rfind('.'), slash = path.rfind('/');
        const size_t at = (dot == std::string::npos || (slash != std::string::npos && dot < slash)) ? path.size() : dot;
        path.insert(at, "_" + idx);
      }
      if ((rc = rmh_png_write_rgba(path.c_str(), host.data() + per_frame * f, W, H)) != RMH_OK) return rc;
    }
  }
  return RMH_OK;
}

void rmh_mesh_config_default(rmh_mesh_config* c) {
  if (!c) return;
  c->res = 128;
  c->margin = 0.05f;
  c->smooth_k = 32.0f;      // train.rs:131 MAX_SMOOTH, the k of the previews and the viewer
  c->radius_offset = 0.01f;  // scene.rs:43: the surface training fitted, as rmh_preview
  c->refine = 2;
  c->device = 0;
}

int rmh_mesh_extract(const char* scene_json, const rmh_mesh_config* config, rmh_mesh** out) {
  if (!out) return fail(RMH_ERR_INVALID_ARG, "out is NULL");
  *out = nullptr;
  if (!scene_json) return fail(RMH_ERR_INVALID_ARG, "scene_json is NULL");
  rmh_mesh_config cfg;
  rmh_mesh_config_default(&cfg);
  if (config) cfg = *config;
  if (cfg.res < 1 || cfg.res > 2048) return fail(RMH_ERR_INVALID_ARG, "res %d out of [1, 2048]", cfg.res);
  if (!(cfg.margin >= 0.0f) || !std::isfinite(cfg.margin) || !(cfg.smooth_k > 0.0f) || !std::isfinite(cfg.smooth_k) ||
      !std::isfinite(cfg.radius_offset) || cfg.refine < 0 || cfg.refine > 64)
    return fail(RMH_ERR_INVALID_ARG, "bad mesh configuration");
  using clock = std::chrono::steady_clock;
  auto ms_since = [](clock::time_point t0) { return std::chrono::duration<double, std::milli>(clock::now() - t0).count(); };
  Gpu g;
  std::vector<float> act;
  DevBuf d_act, d_grid, d_v, d_out;
  rm_scene sc;
  int rc = load_scene(scene_json, cfg.radius_offset, cfg.device, g, act, d_act, &sc);
  if (rc) return rc;
  const int32_t M = sc.num_spheres;

  // the axis-aligned box of c_j +- (r_j + margin), cubic cells of (longest extent / res)
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int32_t j = 0; j < M; ++j) {
    const float reach = act[6 * M + j] + cfg.margin;
    for (int k = 0; k < 3; ++k) {
      lo[k] = std::min(lo[k], act[3 * j + k] - reach);
      hi[k] = std::max(hi[k], act[3 * j + k] + reach);
    }
  }
  const float longest = std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2]));
  if (!(longest > 0.0f) || !std::isfinite(longest)) return fail(RMH_ERR_FORMAT, "%s has no finite, non-empty box", scene_json);
  const float spacing = longest / (float)cfg.res;
  int32_t n[3];
  for (int k = 0; k < 3; ++k)  // lattice points: the cells that cover the extent, at least one
    n[k] = std::max(1, (int32_t)std::ceil((double)(hi[k] - lo[k]) / (double)spacing)) + 1;
  const size_t cells = (size_t)n[0] * n[1] * n[2];

  rm_sdf_params sp;
  rm_sdf_params_default(&sp);
  sp.smooth_k = cfg.smooth_k;
  HIPCHK(d_grid.alloc(sizeof(float) * cells));
  HIPCHK(hipStreamSynchronize(g.stream));  // the scene upload: not part of the grid's time
  auto t0 = clock::now();
  RMCHK(g.ctx, rm_sdf_grid(g.ctx, lo, spacing, n[0], n[1], n[2], &sc, &sp, d_grid.f(), nullptr));
  HIPCHK(hipStreamSynchronize(g.stream));
  const double ms_grid = ms_since(t0);
  t0 = clock::now();
  std::vector<float> grid(cells);
  HIPCHK(hipMemcpyAsync(grid.data(), d_grid.p, sizeof(float) * cells, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  const double ms_copy = ms_since(t0);
  t0 = clock::now();
  rmh_mesh* raw = nullptr;
  if ((rc = rmh_mesh_from_grid(grid.data(), n[0], n[1], n[2], lo, spacing, &raw)) != RMH_OK) return rc;
  std::unique_ptr<rmh_mesh, void (*)(rmh_mesh*)> mesh(raw, rmh_mesh_free);
  const double ms_extract = ms_since(t0);
  t0 = clock::now();

  const size_t V = mesh->vertices.size() / 3;
  if (V > 0) {
    // Newton projections onto D = 0, then the normals and colours at the final vertices
    HIPCHK(d_v.alloc(sizeof(float) * 3 * V));
    HIPCHK(d_out.alloc(sizeof(float) * 7 * V));  // dist [V] | grad [V][3] | color [V][3]
    float *d_dist = d_out.f(), *d_grad = d_dist + V, *d_col = d_grad + 3 * V;
    std::vector<float> h(7 * V);
    for (int32_t it = 0; it <= cfg.refine; ++it) {
      const bool last = it == cfg.refine;
      HIPCHK(hipMemcpyAsync(d_v.p, mesh->vertices.data(), sizeof(float) * 3 * V, hipMemcpyHostToDevice, g.stream));
      RMCHK(g.ctx, rm_sdf_query(g.ctx, d_v.f(), (int64_t)V, &sc, &sp, last ? nullptr : d_dist, d_grad, last ? d_col : nullptr));
      HIPCHK(hipMemcpyAsync(h.data(), d_out.p, sizeof(float) * 7 * V, hipMemcpyDeviceToHost, g.stream));
      HIPCHK(hipStreamSynchronize(g.stream));
      const float* gr = h.data() + V;
      if (!last) {
        for (size_t v = 0; v < V; ++v) {
          const float gx = gr[3 * v], gy = gr[3 * v + 1], gz = gr[3 * v + 2];
          const float g2 = gx * gx + gy * gy + gz * gz;
          if (!(g2 >= 1e-12f)) continue;
          const float step = h[v] / g2;
          mesh->vertices[3 * v] -= step * gx;
          mesh->vertices[3 * v + 1] -= step * gy;
          mesh->vertices[3 * v + 2] -= step * gz;
        }
      } else {
        mesh->normals.assign(3 * V, 0.0f);
        mesh->colors.assign(h.begin() + 4 * V, h.end());
        for (size_t v = 0; v < V; ++v) {
          const double gx = gr[3 * v], gy = gr[3 * v + 1], gz = gr[3 * v + 2];
          const double len = std::sqrt(gx * gx + gy * gy + gz * gz);
          if (!(len > 0.0)) continue;
          mesh->normals[3 * v] = (float)(gx / len);
          mesh->normals[3 * v + 1] = (float)(gy / len);
          mesh->normals[3 * v + 2] = (float)(gz / len);
        }
      }
    }
  }
  mesh->ms[0] = ms_grid;
  mesh->ms[1] = ms_copy;
  mesh->ms[2] = ms_extract;
  mesh->ms[3] = ms_since(t0);
  *out = mesh.release();
  return RMH_OK;
}

int rmh_generate(const char* out_dir, const char* prefix, int32_t W, int32_t H, int32_t device) {
  if (!out_dir || W < 1 || H < 1) return fail(RMH_ERR_INVALID_ARG, "bad arguments");
  const std::string pre = prefix ? prefix : "";
  // generate.rs:29-40: the three-sphere "dango"
  const float centers[9] = {-0.3f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.3f, 0.0f, 0.0f};
  const float colors[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  const float radii[3] = {0.2f, 0.15f, 0.2f};
  // generate.rs:44-86: 8 views around at y = 0.5, one from the top, one from below
  std::vector<rmh_camera_entry> cams;
  const int num_h = 8;
  const float radius = 2.5f, fov = 50.0f;
  auto add = [&](float x, float y, float z) {
    rmh_camera_entry e;
    std::memset(&e, 0, sizeof e);
    std::snprintf(e.file, sizeof e.file, "%starget_%zu.png", pre.c_str(), cams.size());
    e.origin[0] = x;
    e.origin[1] = y;
    e.origin[2] = z;
    e.fov = fov;
    cams.push_back(e);
  };
  for (int i = 0; i < num_h; ++i) {
    const float angle = (float)i * (2.0f * (float)M_PI / (float)num_h);
    add(radius * std::cos(angle), 0.5f, radius * std::sin(angle));
  }
  add(0.0f, 2.5f, -0.001f);
  add(0.0f, -1.5f, -2.0f);
  const int V = (int)cams.size();
  Gpu g;
  int rc;
  if ((rc = g.open(device)) != RMH_OK) return rc;
  DevBuf d_c, d_col, d_r, out;
  HIPCHK(d_c.alloc(sizeof centers));
  HIPCHK(d_col.alloc(sizeof colors));
  HIPCHK(d_r.alloc(sizeof radii));
  HIPCHK(hipMemcpyAsync(d_c.p, centers, sizeof centers, hipMemcpyHostToDevice, g.stream));
  HIPCHK(hipMemcpyAsync(d_col.p, colors, sizeof colors, hipMemcpyHostToDevice, g.stream));
  HIPCHK(hipMemcpyAsync(d_r.p, radii, sizeof radii, hipMemcpyHostToDevice, g.stream));
  std::vector<rm_camera> rc_cams(V);
  for (int v = 0; v < V; ++v) camera_struct(rc_cams[v], cams[v].origin, cams[v].target, cams[v].fov);
  const size_t per_view = 3 * (size_t)W * H;
  HIPCHK(out.alloc(sizeof(float) * per_view * V));
  RMCHK(g.ctx, rm_render_camera(g.ctx, rc_cams.data(), V, W, H, d_c.f(), d_col.f(), d_r.f(), 3, out.f()));
  std::vector<float> host(per_view * V);
  HIPCHK(hipMemcpyAsync(host.data(), out.p, out.bytes, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  const std::string dir = out_dir;
  for (int v = 0; v < V; ++v) {
    char name[64];
    std::snprintf(name, sizeof name, "target_%d.png", v);
    if ((rc = rmh_image_save(join_path(dir, name).c_str(), host.data() + per_view * v, W, H)) != RMH_OK) return rc;
  }
  return rmh_cameras_save(join_path(dir, "cameras.json").c_str(), cams.data(), V);
}

}  // extern "C"
