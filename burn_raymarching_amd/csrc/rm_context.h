// rm_context.h -- the host side's state: the context behind the C ABI, the one owner of its device
// buffers (DevBuf), and the error plumbing (fail, RM_HIP). Included by rm_kernels.hip after the
// kernels (one translation unit); rm_launch.h and rm_api.h follow.
#pragma once

struct rm_context;

namespace {

int fail(rm_context* ctx, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));

// A grow-only device buffer. ensure() is the library's only device allocation; a buffer is freed
// when it has to grow, by release() and with its context.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  // At least `bytes` of device memory. Never shrinks; with enough capacity no HIP call at all. To
  // grow, the context's stream is drained first (launches in flight may read the old buffer), then
  // the old buffer is freed and the new one allocated -- its contents are not kept. zero: one
  // hipMemsetAsync of the whole buffer on the stream, at allocation only (the arrival counters,
  // which the kernels leave zero between launches). On failure the buffer is empty: RM_ERR_OOM.
  int ensure(rm_context* ctx, size_t bytes, const char* what, bool zero = false);
  void release() {  // the caller has drained the stream
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
  explicit operator bool() const { return p != nullptr; }
};

constexpr int kCamRing = 32;  // calls of > kInlineCams views in flight before the host waits for a slot

// The centre-out block order of one tiling (ensure_block_order): written once, when the context first meets
// a tiled call of tx x ty tiles and `sub` blocks a tile, and never rewritten or freed before the context, so a
// launch that holds its address -- in flight, or captured in a hipGraph -- reads its own order whatever other
// tilings later calls bring.
struct BlockOrder {
  int tx = 0, ty = 0, sub = 0;
  DevBuf table;  // tx * ty * sub ints
};

}  // namespace

struct rm_context {
  int device = 0;
  hipStream_t stream = nullptr;
  rm_step_scalars* sdev = nullptr;  // device step scalars (rm_bind_step_scalars), nullable
  std::string err;
  bool timing = false;  // record hipEvents around every per-ray kernel launch
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
  size_t events_used = 0;
  DevBuf ws;            // partials | segment sums | small scratch
  DevBuf rg_ws;         // ray-gradient calls: march t [rays] | per-view partial rows (rm_raygrad_kernel)
  DevBuf rec;           // sphere records of the current call (rm_prep_kernel)
  DevBuf sh_rec;        // rm_render_diff_sh: the call's coefficients per sphere pair (rm_sh_pack_kernel)
  DevBuf loss_ws;       // rm_image_loss: per-view fp64 sums | tile partial records | the A, B, C maps (rm_loss.h)
  DevBuf batch;         // rm_train_iteration's unfused path: the drawn batch (9 floats/ray)
  DevBuf cont_buf;      // split continuation: saved march state | list | count
  DevBuf stats_dev;     // work counters (rm_stats_enable), kStatsWords words
  DevBuf esc_flags;     // per-block escape flags, kMaxBlocksPerLaunch ints
  DevBuf lattice;       // the current call's escape lattice, kLatticeN^3 floats (rm_lattice_kernel)
  DevBuf tile_proof;    // the current launch's tile-proof bytes, one per wave (rm_tile_proof_kernel)
  long long tile_proof_n = 0;  // bytes the last launch with the tile proof wrote (rm_debug_tile_proof)
  DevBuf arrivals;      // rm_small_kernel's arrival counter (zero between launches)
  DevBuf red_arrivals;  // rm_reduce_partials' per-column-block arrival counters
  DevBuf opt_arrival;   // rm_train_step_camera_adam: the reduction's column-block counter
  DevBuf opt_pre;       // rm_train_iteration: the optimizer part of the launch's extra block
  std::list<BlockOrder> block_orders;  // centre-out tile orders, one per tiling the context has met
  DevBuf olist;         // cost-ordered dispatch: 3 x [list][kMaxBlocksPerLaunch] block lists (kOrderLists)
  DevBuf ocnt;          // 3 x [list] list lengths (zeroed one launch ahead), then the turn word
  DevBuf cams_dev;      // camera bases of calls with > kInlineCams views (device)
  rm::CamBasis* cams_pin = nullptr;       // their pinned host staging, kCamRing slots
  hipEvent_t cam_ev[kCamRing] = {};       // slot k's copy has run
  int cam_slot = 0;
  std::vector<rm::CamBasis> cams_shadow;  // what the device table holds (the last upload)
  // rm_train_step_sampled_prepared: opt_pre holds the next rm_optimizer_step's gradient-independent
  // part for these arguments (consumed by that call, cleared by any other use of opt_pre)
  bool opt_prepared = false;
  const float* prep_raw = nullptr;
  float* prep_loss_penalty = nullptr;
  int prep_M = 0, prep_step = 0, prep_pen = 0;
  bool adam_done = false;      // the last call's optimizer ran inside its reduction
  long long stats_blocks = 0;  // ray blocks launched while stats are on
  long long stats_waves = 0;   // their ray waves (a split block holds one)
  int* stall_flag = nullptr;        // rm_debug_stall: host-mapped release flag (host pointer)
  int* oturn = nullptr;             // device word in ocnt: the list set the next keyed launch appends to
  unsigned long long cost_key = 0;  // geometry of the last keyed launch (its lists order the next)
  bool cost_valid = false;
#ifdef RM_BLOCK_TRACE
  DevBuf btrace;  // measurement build: per-wave records of the last launch
  long long btrace_waves = 0;
#endif
};

namespace {

int fail(rm_context* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (ctx) ctx->err = buf;
  return code;
}

#define RM_HIP(ctx, call)                                                                        \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess) return fail(ctx, RM_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
  } while (0)

int DevBuf::ensure(rm_context* ctx, size_t bytes, const char* what, bool zero) {
  if (cap >= bytes) return RM_OK;
  if (p) {
    RM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    RM_HIP(ctx, hipFree(p));
    p = nullptr;
    cap = 0;
  }
  const hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) {
    p = nullptr;
    return fail(ctx, RM_ERR_OOM, "%s (%zu B) allocation failed: %s", what, bytes, hipGetErrorString(e));
  }
  cap = bytes;
  if (zero) RM_HIP(ctx, hipMemsetAsync(p, 0, bytes, ctx->stream));
  return RM_OK;
}

bool env_is(const char* name, char v) {
  const char* e = std::getenv(name);
  return e && e[0] == v;
}

}  // namespace
