// rm_kernels.hip -- MI355X (gfx950) kernels of the differentiable SDF-sphere raymarcher
// and the C ABI declared in include/raymarch.h.
//
// Hot path replaced: render_diff (renderer_diff.rs:6-91) and its burn-autodiff
// backward (train.rs:189-190). One thread owns one ray for the whole pipeline:
//
//   in-kernel camera ray (camera.rs:58-78), 16x16 pixel tiles per block, centre-out dispatch
//   S fixed soft-min march steps          (renderer_diff.rs:20-26, scene.rs:60-79, sdf.rs:30-44)
//     squared distances on the matrix cores (bf16 three-way splits, lse_mfma), sqrt/exp2 on
//     the vector units; waves whose rays provably escape leave early (exact)
//   gradient reconnect sweep at p_approx  (renderer_diff.rs:28-39)
//   detached normal: one soft-min gradient sweep, the eps -> 0 limit of the six central
//     differences of scene.rs:81-128 (renderer.rs mode: the six taps)
//   Lambert + ambient                     (renderer_diff.rs:48-62)
//   softmax colour blend + mask soft-min  (renderer_diff.rs:64-90), one shared sweep
//   [train] weighted-L1 seed              (training.rs:17-34)
//   [bwd]   analytic backward: sweep at p_final, then at p_approx
//
// Sphere records are built once per call (rm_prep_kernel) and read through the constant
// address space into SGPRs (vector sweeps, two spheres per packed instruction) or as bf16
// MFMA fragments (march). The soft-min log-sum-exp runs in base 2 on v_exp_f32/v_log_f32 with
// the cheapest provably safe shift. Per-sphere gradients are summed over the 64 rays of a
// wave with a transposing permlane/DPP reduction, over the live waves in LDS, and over
// workgroups in a fixed order by rm_reduce_partials (deterministic; no floating-point
// atomics). DESIGN.md §4 has the details and the measurements.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdarg>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/raymarch.h"
#include "rm_device.h"

#ifndef RM_ORDER_CLASSES
#define RM_ORDER_CLASSES 16  // cost classes of the cost-ordered dispatch (order_append)
#endif
// ints between the three list sets' class counts and before the turn word: each on cache lines of
// its own (every block of a launch reads the turn and the previous set's counts while the blocks'
// appends hit the current set's counts with atomics; sharing a 128-byte line made every launch
// that appended to the set next to the turn word 50 % slower at C2: tools/order_probe.py)
#ifndef RM_ORDER_CLS_STRIDE
// ints between a set's class counts: each class on a 128-byte line of its own, as the reduction's
// arrival counters below (both: C2cj 4348-4404 vs 4305-4315 Mrays/s with neither, the metric
// equal; tools/gpu_ab.sh, profiles/r05e_ab.txt)
#define RM_ORDER_CLS_STRIDE 32
#endif
#ifndef RM_ORDER_CNT_STRIDE
#define RM_ORDER_CNT_STRIDE (RM_ORDER_CLASSES * RM_ORDER_CLS_STRIDE > 64 ? RM_ORDER_CLASSES * RM_ORDER_CLS_STRIDE : 64)
#endif
static_assert(RM_ORDER_CNT_STRIDE >= RM_ORDER_CLASSES * RM_ORDER_CLS_STRIDE && RM_ORDER_CNT_STRIDE % 32 == 0,
              "128-byte lines per set");
#ifndef RM_RED_ARR_STRIDE
#define RM_RED_ARR_STRIDE 32  // unsigneds between rm_reduce_partials' arrival counters: a 128-byte line each
#endif

namespace rm {

// kRender: the non-differentiable target renderer of renderer.rs:4-80 (generate.rs)
enum Mode { kFwd = 0, kBwd = 1, kTrain = 2, kRender = 3 };

// bounds the partial-gradient workspace per launch: 16 views of 512x512
// 128 views of 512 x 512 in one launch (per-launch ramp-down and the per-call record, origin
// and reduction launches amortised over all the views of a step)
constexpr int kMaxBlocksPerLaunch = 131072 * (256 / kBlock);
// camera bases carried in the kernel arguments; calls with more views read a device table
constexpr int kInlineCams = 16;
// automatic split march (RM_MARCH_SPLIT): from kSplitMinSpheres spheres for launches of at most
// kSplitMaxRays rays (about one fill of the GPU: 1024 resident 256-ray blocks), from
// kSplitMinSpheresWide for launches of at most kSplitMaxRaysWide (four fills) -- measured
// (tools/gpu_split_sweep.sh): split wins at 1 view from 256 spheres and at 4 views of 512x512
// from 512, loses at 10 views of 256 spheres and at 4 views of 1024x1024
constexpr int kSplitMinSpheres = 256;
constexpr int kSplitMinSpheresWide = 512;
constexpr long long kSplitMaxRaysWide = 1048576;
#ifndef RM_SPLIT_WAVES
#define RM_SPLIT_WAVES 4
#endif
#ifndef RM_SPLIT_MIN_WAVES
#define RM_SPLIT_MIN_WAVES 3  // register budget of the split kernels (waves per SIMD): 3 = 168 VGPRs, no
                              // spills (4: 128 VGPRs, 4-12 VGPR spills, 20 B/lane scratch; C5 equal either way)
#endif
#ifndef RM_CONT_MIN_WAVES
#define RM_CONT_MIN_WAVES RM_SPLIT_MIN_WAVES  // register budget of the split continuation kernel
#endif
constexpr int kSplitWaves = RM_SPLIT_WAVES;  // waves per ray group of the split march (2 or 4)
static_assert(kSplitWaves == 2 || kSplitWaves == 4, "split blocks have 2 or 4 waves");
#ifndef RM_SPLIT_RAYS
#define RM_SPLIT_RAYS 32  // (same box, the work-unit backward: C5 +3.5 %, C5g +5 % against 64)
#endif
// Rays per split block (64, 32 or 16). Below 64 every wave of the block holds each of its rays
// 64 / kSplitRays times (lane l and l + kSplitRays carry the same ray, bit for bit) and the
// march's matrix-core tiles run kSplitRays / 16 column blocks instead of 4: a march step of a
// block costs its waves kSplitRays / 64 of the 64-ray step, so heavy rays hold their SIMDs for
// shorter and the blocks that march to the end are smaller work units (configs[4]).
constexpr int kSplitRays = RM_SPLIT_RAYS;
static_assert(kSplitRays == 64 || kSplitRays == 32 || kSplitRays == 16, "split blocks hold 64, 32 or 16 rays");
constexpr int kSplitCB = kSplitRays / 16;  // column blocks of 16 rays in the split march's tiles
constexpr long long kSplitMaxRays = 262144;
#ifndef RM_REDUCE_SEGS
#define RM_REDUCE_SEGS 128
#endif
constexpr int kReduceSegs = RM_REDUCE_SEGS;  // block segments of the reduction (128: 12.6 + 6.9 us at 10 views vs 20.3 + 4.9 with 64)

struct KArgs {
  // rays: array mode (org/dir) or camera mode (cams)
  const float* org;
  const float* dir;
  long long ray_begin;  // first ray of this launch
  long long n_rays;     // rays in this launch
  int width, height, num_views;
  int tiling;  // camera mode pixel order: 2 = 16x16 tile per block (8x8 per wave), 0 = rows
  int cull;    // skip blocks whose rays provably escape the scene (RM_MARCH_SKIP_ESCAPED)
  float cull_min_d;  // scene distance at which the silhouette mask is exactly 0
  float lse_slack;  // ln(M) / k (rounded up): the hard min exceeds the soft-min by at most this
  unsigned long long* stats;  // nullable: [0] += 1 per escaped (skipped) block, [1] exited waves,
                              // [2] march steps saved, [3] unused (zero), [4] / [5] rays the two
                              // backward sweeps run for (non-zero seeds)
  float gone_d;               // > 0: rays that provably escape past this distance are `gone` (see the march)
  int early_exit;             // waves whose rays are all gone stop marching
  int split;                  // split march (RM_MARCH_SPLIT): 64 rays per block, a quarter of the spheres per wave
  int mfma;                   // march sums on the matrix cores (lse_mfma) instead of lse_weighted
  int shift_max;              // RM_MARCH_FORCE_MAX_SHIFT: every march step takes the running-max shift
  const int* esc_flags;       // nullable: per-block escape flags of this launch (rm_escape_kernel)
  const int* block_order;     // nullable: heavy-first dispatch order of the tiles of a view (ray_block)
  int order_views, order_tiles;
  // cost-ordered dispatch: [class][kMaxBlocksPerLaunch] block lists + [class] counts of the
  // previous launch (read, nullable), of this launch (appended, nullable) and the counts to clear
  // for the next launch (nullable)
  const int* olist_r;
  const int* ocnt_r;
  int* olist_w;
  int* ocnt_w;
  int* ocnt_z;
  // nullable: the device word naming the list set this launch appends to (0..2); with it the five
  // pointers above point to set 0 and the launch picks its sets from the word (read: the set
  // before, clear: the set after), and the call's reduction advances the word -- the rotation
  // lives on the device, so a launch captured in a hipGraph keeps rotating when replayed
  const int* oturn;
  CamBasis cams[kInlineCams];  // views <= kInlineCams
  const CamBasis* cams_dev;    // more views: the bases in device memory (cams unused), else NULL
  // activated scene
  const float* centers;
  const float* colors;
  const _Float16* colors_h;  // RM_MARCH_COLOR_F16: the colours as IEEE half [M,3] (colors is then NULL)
  const float* radius;
  const float* light_dir;
  const float* ambient;
  int M, Mpad;
  const float4* rec_buf;  // sphere records of this call (rm_prep_kernel), see Lds
  float* origin;  // camera mode, nullable: per view, the first march step's D at the eye (write_origins)
  // march / shading
  int steps;
  float k, eps, csharp, msharp;
  // io
  float* out;
  float* t_out;
  const float* t_in;
  const float* gout;
  const float* targets;
  float progress, inv_count;
  const rm_step_scalars* sdev;  // nullable (rm_bind_step_scalars): progress = index / total from here
  float light_fixed[3];  // kRender: renderer.rs:27-32 light, normalised on the host in f32
  float* dbg;       // optional per-ray intermediates [n][16] (diagnostics; see rm_debug_intermediates)
  float* partials;  // [gridDim.x][rec], rec = Mpad*8 + 8
  long long rec;
  // Continuation of a split launch (split_cont_caps, see run()). The split kernels march in ray
  // mode: every march step takes the scene-uniform fixed shift (the running maximum where the
  // scene does not admit it), so a ray's step is a function of its own state alone. A ray whose t
  // repeats with period 2 retires with its final t by itself (the wave-level cycle exit
  // generalised), and at a continuation cap the still-marching RAYS, not their groups, go on:
  //  * first launch (cont_cap > 0, cont_resume = 0): a group whose rays still march at step
  //    cont_cap saves every ray's state, appends itself to cont_list_w (*cont_count_w entries, in
  //    arrival order) and its marching rays to ray_list_w (*ray_count_w entries), and ends;
  //  * ray_cont launches (cont_resume = the cap before): a block marches kSplitRays listed rays
  //    (ray_list[0..*ray_count), of any groups) from cont_resume to its own cont_cap, where it
  //    lists the rays still marching again, or to the end, and writes their states back;
  //  * resume launch (cont_resume = steps, ray_cont = 0): block b runs the post-march forward and
  //    the backward of group cont_list[b], b < *cont_count, from the saved final states.
  // The grouping of rays changes no bit (tests/test_gpu_split.py).
  // cont_state: eight per-ray rows of cont_rays floats -- 0 t, 1 lb, 2 D_prev, 3 / 4 t one and two
  // steps back, 5 the ray's code (0 marching, 1 gone, 2 retired), 6 rho_lb, 7 the ray's own choice
  // history (as int bits) -- then, from float 8 cont_rays, two words per group: the group's choice
  // history and its steps saved (as int bits).
  int cont_cap, cont_resume;
  float* cont_state;
  const int* cont_list;
  const int* cont_count;
  int* cont_list_w;
  int* cont_count_w;
  long long cont_rays;
  int ray_cont;
  const int* ray_list;
  const int* ray_count;
  int* ray_list_w;
  int* ray_count_w;
#ifdef RM_BLOCK_TRACE
  unsigned long long* btrace;  // measurement build: per-wave timing records (rm_ray_kernel)
#endif
};
#ifdef RM_BLOCK_TRACE
constexpr int kTraceWords = 12;
// measurement build: word w of this wave's record (lane 0 writes)
__device__ __forceinline__ void trace_word(const KArgs& a, int w, unsigned long long v) {
  if (a.btrace != nullptr && (threadIdx.x & 63) == 0)
    a.btrace[kTraceWords * ((unsigned long long)blockIdx.x * kWaves + (threadIdx.x >> 6)) + w] = v;
}
#define RM_TRACE(w, v) trace_word(a, (w), (v))
#else
#define RM_TRACE(w, v) ((void)0)
#endif

// ---- sphere records: pair-interleaved, in global memory, read through scalar loads ----------
// rm_prep_kernel writes them once per call. Pair i holds spheres (2i, 2i+1) so every sweep runs
// two spheres per v_pk_* instruction:
//   P0 = {-2cx0, -2cx1, -2cy0, -2cy1}   P1 = {-2cz0, -2cz1, |c0|^2, |c1|^2}
//   P2 = {k r0, k r1, r0, r1}           P3 = {red0, red1, green0, green1}   P4 = {blue0, blue1}
//   S0, S1 = P0, P1 scaled by k^2       W  = {2^(k r0), 2^(k r1), 2^(k (r0 - r_first)), 2^(k (r1 - r_first))}
// (k = smooth_k log2 e). Every lane of a wave reads the same record at the same time, so the
// kernel reads them through the constant address space: s_load into SGPRs that feed the
// packed VALU ops as scalar operands -- no LDS staging, no LDS broadcast traffic, and no limit
// on M (the records stream through the scalar cache / L2).
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(4))) f4v* cf4_ptr;
typedef const __attribute__((address_space(4))) f2v* cf2_ptr;
typedef const __attribute__((address_space(4))) float* cf1_ptr;

// Header after the records: {r_min, r_max, max |c_j - c_0|, 0, c_x, c_y, c_z, R} of the real
// spheres ((c, R): bounding sphere, scene_bound), followed by one partial header per
// rm_prep_kernel block when that kernel ran on more than one block.
constexpr int kRecHeader = 8;

// Then, 16-byte aligned, the matrix-core tiles of the march (lse_mfma): per row block of 16
// spheres 64 lanes x 16 B of A fragments, then per row block 32 floats {w(16), w_fixed(16)}.
__host__ __device__ inline size_t tiles_offset(int npairs, int nprep) {
  return ((size_t)npairs * (7 * 16 + 8) + (size_t)(nprep + 1) * kRecHeader * sizeof(float) + 15) & ~(size_t)15;
}
// Then the escape thresholds of the march: kEscTab floats (see write_bound).
constexpr int kEscTab = 64;
constexpr int kStatsWords = 6;  // rm_stats device counters (KArgs::stats)
__host__ __device__ inline size_t esc_offset(int npairs, int nprep) {
  const size_t nrb = (size_t)npairs / 8;
  return tiles_offset(npairs, nprep) + nrb * 64 * 16 + nrb * 32 * sizeof(float);
}
// Then the per-view origin steps of camera mode (write_origins): RM_MAX_VIEWS_PER_CALL floats,
// then per view a lower bound on the eye's distance to the nearest sphere centre (the march's
// clamp-free proof, rho_lb in rm_ray_kernel): RM_MAX_VIEWS_PER_CALL floats.
__host__ __device__ inline size_t origin_offset(int npairs, int nprep) {
  return esc_offset(npairs, nprep) + kEscTab * sizeof(float);
}
__host__ __device__ inline size_t rec_bytes(int npairs, int nprep) {
  return origin_offset(npairs, nprep) + 2 * RM_MAX_VIEWS_PER_CALL * sizeof(float);
}

struct Lds {  // the sphere records (global, scalar-loaded) plus the kernel's LDS scratch
  cf4_ptr P0, P1, P2, P3, S0, S1, W;
  cf2_ptr P4;
  const uint4* At;  // lse_mfma sphere fragments (global)
  const float* Wt;  // lse_mfma weights (global)
  float* slots;  // LDS: the backward's ray images and shares; lse_mfma's ray exchange in the march
  float* misc;   // small LDS scratch
  __device__ __forceinline__ static float4 v4(f4v v) { return make_float4(v.x, v.y, v.z, v.w); }
  __device__ __forceinline__ float4 p0(int i) const { return v4(P0[i]); }
  __device__ __forceinline__ float4 p1(int i) const { return v4(P1[i]); }
  __device__ __forceinline__ float4 p2(int i) const { return v4(P2[i]); }
  __device__ __forceinline__ float4 p3(int i) const { return v4(P3[i]); }
  __device__ __forceinline__ float2 p4(int i) const {
    const f2v v = P4[i];
    return make_float2(v.x, v.y);
  }
  __device__ __forceinline__ float2 kr(int i) const {
    const f4v v = P2[i];
    return make_float2(v.x, v.y);
  }
  // the same records from pair `off` on (a split block's quarter of the vector sweeps)
  __device__ __forceinline__ Lds from_pair(int off) const {
    Lds q = *this;
    q.P0 += off;
    q.P1 += off;
    q.P2 += off;
    q.P3 += off;
    q.S0 += off;
    q.S1 += off;
    q.W += off;
    q.P4 += off;
    return q;
  }
};

// LDS: the backward's ray images and g_t shares, or (during the march) lse_mfma's per-wave ray
// exchange (64 x (16 + 16 + 4) B per wave); then 256 B of misc scratch.
// The backward (one sphere per lane) uses 15 x 64 ray-data floats (field-major) per wave
// and kWaves x 64 g_t shares per wave (19.3 KB). The LDS of a block decides how many blocks a CU
// holds once waves leave the march early (their registers free up, the block's LDS stays until its
// last wave ends): 19.3 KB -> 8 blocks per CU (24.3 KB -> 6, 32.3 KB -> 4).
constexpr int kBwdFields = 15;  // ray-image fields of the transposed backward
constexpr size_t kSlotBwdT = ((size_t)kWaves * 64 * kBwdFields + (size_t)kWaves * kWaves * 64) * sizeof(float);
constexpr size_t kSlotBytes = kSlotBwdT;
static_assert((size_t)kWaves * 64 * 36 <= kSlotBytes, "the march's ray exchange fits the slots");
__host__ __device__ constexpr size_t lds_bytes() { return kSlotBytes + 256; }
// the split march's two combine buffers (kWaves x 64 floats each) after the march exchange
constexpr int kSplitCombOff = kWaves * 64 * 9;  // floats: xa, xb (64 uint4 per wave each), xs
static_assert((kSplitCombOff + 2 * kWaves * 64) * sizeof(float) <= kSlotBytes, "split combine buffers fit the slots");

// three-value block reduction (min, max, max) for the record header (blockDim.x / 64 <= 16 waves)
__device__ __forceinline__ void header_reduce(float& rmin, float& rmax, float& spread, float* dst) {
  __shared__ float red[3][16];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    rmin = fminf(rmin, __shfl_xor(rmin, off));
    rmax = fmaxf(rmax, __shfl_xor(rmax, off));
    spread = fmaxf(spread, __shfl_xor(spread, off));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wave] = rmin;
    red[1][wave] = rmax;
    red[2][wave] = spread;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w2 = 1; w2 < (int)(blockDim.x >> 6); ++w2) {
      red[0][0] = fminf(red[0][0], red[0][w2]);
      red[1][0] = fmaxf(red[1][0], red[1][w2]);
      red[2][0] = fmaxf(red[2][0], red[2][w2]);
    }
    dst[0] = red[0][0];
    dst[1] = red[1][0];
    dst[2] = red[2][0];
    dst[3] = 0.0f;
  }
}

// Bounding sphere of the scene, block-wide: c0 = centre of the centres' bounding box,
// R >= |c_j - c0| + r_j for every sphere (rounded up). scratch: >= 8 floats of LDS per wave of
// the block.
__device__ __forceinline__ void scene_bound(const KArgs& a, float* scratch, int tid, float c0[3], float& R) {
  const int lane = tid & 63, wave = tid >> 6, nt = (int)blockDim.x, nw = nt >> 6;
  float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int j = tid; j < a.M; j += nt)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float c = a.centers[3 * j + k];
      v[k] = fminf(v[k], c);
      v[3 + k] = fmaxf(v[3 + k], c);
    }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v[k] = fminf(v[k], __shfl_xor(v[k], off));
      v[3 + k] = fmaxf(v[3 + k], __shfl_xor(v[3 + k], off));
    }
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < 6; ++k) scratch[8 * wave + k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float lo = scratch[k], hi = scratch[3 + k];
    for (int w = 1; w < nw; ++w) {
      lo = fminf(lo, scratch[8 * w + k]);
      hi = fmaxf(hi, scratch[8 * w + 3 + k]);
    }
    c0[k] = 0.5f * (lo + hi);
  }
  float r = 0.0f;
  for (int j = tid; j < a.M; j += nt) {
    const float dx = a.centers[3 * j] - c0[0], dy = a.centers[3 * j + 1] - c0[1], dz = a.centers[3 * j + 2] - c0[2];
    r = fmaxf(r, fsqrt(dx * dx + dy * dy + dz * dz) + a.radius[j]);  // 1 ulp: inside the round-up below
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) r = fmaxf(r, __shfl_xor(r, off));
  __syncthreads();  // everyone has read the box
  if (lane == 0) scratch[8 * wave] = r;
  __syncthreads();
  R = scratch[0];
  for (int w = 1; w < nw; ++w) R = fmaxf(R, scratch[8 * w]);
  R = R * (1.0f + 1e-5f) + 1e-6f;  // cover the f32 rounding of |c - c0| + r
  __syncthreads();  // scratch is reused by the caller
}

// ---- matrix-core march fragments (see lse_mfma) ----------------------------------------------
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// exact three-part bf16 split of x (bit patterns in the low 16 bits)
__device__ __forceinline__ void split3(float x, unsigned& h1, unsigned& h2, unsigned& h3) {
  const unsigned a = __float_as_uint(x) & 0xFFFF0000u;
  const float r1 = x - __uint_as_float(a);
  const unsigned b = __float_as_uint(r1) & 0xFFFF0000u;
  const float r2 = r1 - __uint_as_float(b);
  const unsigned c = __float_as_uint(r2) & 0xFFFF0000u;
  h1 = a >> 16;
  h2 = b >> 16;
  h3 = c >> 16;
}
__device__ __forceinline__ unsigned pack2(unsigned lo16, unsigned hi16) { return lo16 | (hi16 << 16); }
constexpr unsigned kBf16One = 0x3F80u;

// sphere-side fragment: K slice g (8 bf16) of sphere j (rm_prep_kernel)
__device__ __forceinline__ uint4 mfma_a_slice(const KArgs& a, int j, int g) {
  const float kappa = a.k * kLog2e, k2 = kappa * kappa;
  float cx, cy, cz;
  if (j < a.M) {
    cx = a.centers[3 * j];
    cy = a.centers[3 * j + 1];
    cz = a.centers[3 * j + 2];
  } else {  // padding sphere (see rm_prep_kernel)
    cx = kPadCenter;
    cy = cz = 0.0f;
  }
  unsigned x[3], y[3], z[3], C[3];
  split3(-2.0f * k2 * cx, x[0], x[1], x[2]);
  split3(-2.0f * k2 * cy, y[0], y[1], y[2]);
  split3(-2.0f * k2 * cz, z[0], z[1], z[2]);
  split3(k2 * (cx * cx + cy * cy + cz * cz), C[0], C[1], C[2]);
  if (g < 2)
    return make_uint4(pack2(x[g], x[g]), pack2(x[g], y[g]), pack2(y[g], y[g]), pack2(z[g], z[g]));
  if (g == 2) return make_uint4(pack2(x[2], x[2]), pack2(0u, y[2]), pack2(y[2], 0u), pack2(z[2], z[2]));
  return make_uint4(pack2(z[0], z[1]), pack2(kBf16One, kBf16One), pack2(kBf16One, C[0]), pack2(C[1], C[2]));
}
// Element e of the tile array: v_mfma_f32_16x16x32_bf16 -- row block rb = e / 64 of 16 spheres,
// lane l = e % 64 holds sphere 16 rb + (l & 15), slice l >> 4.
__device__ __forceinline__ uint4 mfma_a_frag(const KArgs& a, int e) {
  const int l = e & 63;
  return mfma_a_slice(a, 16 * (e >> 6) + (l & 15), l >> 4);
}
// Sphere of weight slot e (per 16 spheres 32 slots: 16 unshifted | 16 fixed-shift weights in sphere
// order)
__device__ __forceinline__ int mfma_w_sphere(int e) { return 16 * (e >> 5) + (e & 15); }
__device__ __forceinline__ bool mfma_w_fixed(int e) { return (e & 16) != 0; }

// hdr[4..7] = the bounding sphere (c, R) of scene_bound, for the march's escape test, and its
// distance thresholds T(n), n < kEscTab: a receding ray at distance d from c with n march steps
// left ends them at distance >= gone_d + R' from c if (1 - 1e-5) d >= T(n). Every step is at
// least g = d - R' long (R' = R + ln(M)/k + 1e-3: the soft-min is >= the hard min - ln(M)/k,
// 1e-3 covers the fp32 march) and keeps the ray receding, so one step takes d to at least
// F(d) = (1 - 1e-5) sqrt(d^2 + (d - R')^2); T(0) = gone_d + R' and T(n) = F^-1(T(n - 1)) =
// (R' + sqrt(2 y^2 - R'^2)) / 2 with y = T(n - 1) / (1 - 1e-5), rounded up. For n >= kEscTab the
// march uses T(kEscTab - 1) >= T(n).
__device__ void write_bound(const KArgs& a, float* hdr, float* esc) {
  __shared__ float scratch[8 * 16];
  float c[3], R;
  scene_bound(a, scratch, threadIdx.x, c, R);
  if (threadIdx.x == 0) {
    hdr[4] = c[0];
    hdr[5] = c[1];
    hdr[6] = c[2];
    hdr[7] = R;
  }
  if (threadIdx.x < kEscTab) {
    // f32 with a 1e-5 relative + 1e-6 absolute round-up per iteration (the f32 rounding of one
    // iteration is a few 1e-7): every T(n) stays above the exact inverse iterate. (R' rounded up
    // is conservative too: F^-1 grows with R' for y > R', which holds along the table.)
    float tv = INFINITY;
    if (a.gone_d > 0.0f) {
      const float rp = (R + a.lse_slack + 1e-3f) * (1.0f + 1e-6f);
      const float inv_shrink = 1.0000101f;  // y = T / (1 - 1e-5) <= T inv_shrink
      float T = (a.gone_d + rp) * (1.0f + 1e-6f);
      // four dependent instructions per step (v_sqrt_f32: 1 ulp, inside the round-up)
      const float two_c2 = 2.0f * inv_shrink * inv_shrink * (1.0f + 1e-6f), nrp2 = -rp * rp,
                  half_up = 0.5f * (1.0f + 1e-5f);
      // the march reads T(n) for n <= a.steps only: entries past it repeat T(a.steps) (>= T(n)),
      // which shortens the longest dependent chain at S < kEscTab
      const int nmax = min((int)threadIdx.x, a.steps);
      for (int n = 1; n <= nmax; ++n) T = fmaf(rp + fsqrt(fmaf(two_c2 * T, T, nrp2)), half_up, 1e-6f);
      tv = T * (1.0f + 1e-6f);
    }
    esc[threadIdx.x] = tv;
  }
}

// Records of the call (see Lds), one thread per sphere pair. Each block reduces its pairs'
// {r_min, r_max, spread} into the header (one block) or its partial (several blocks, then
// rm_prep_finish); the final header also gets the scene's bounding sphere (scene_bound).
constexpr int kPrepStageMax = 512;  // one-block prep: parameters staged in LDS up to this M

template <bool PAR>
__device__ void write_origins(const KArgs& a, const float4& S00, const float4& S10, float rmax, float spread,
                              const uint4* At, const float* Wt, float* orig, unsigned char* xch, int v);

__global__ __launch_bounds__(256) void rm_prep_kernel(const KArgs a0, float4* __restrict__ rec) {
  // One-block case: stage the parameters in LDS once (one load round instead of one per phase:
  // records, MFMA tiles, header, bounding sphere); the phases below read them through `a`.
  __shared__ float stage[7 * kPrepStageMax];
  const int nt = (int)blockDim.x;
  KArgs a = a0;
  if (gridDim.x == 1 && a0.M <= kPrepStageMax) {
    const int M = a0.M;
    for (int e = threadIdx.x; e < 3 * M; e += nt) {
      stage[e] = a0.centers[e];
      stage[3 * M + e] = a0.colors_h != nullptr ? (float)a0.colors_h[e] : a0.colors[e];
    }
    for (int e = threadIdx.x; e < M; e += nt) stage[6 * M + e] = a0.radius[e];
    __syncthreads();
    a.centers = stage;
    a.colors = stage + 3 * M;
    a.colors_h = nullptr;
    a.radius = stage + 6 * M;
  }
  const int np = a.Mpad / 2;
  float4* P0 = rec;
  float4* P1 = P0 + np;
  float4* P2 = P1 + np;
  float4* P3 = P2 + np;
  float4* S0 = P3 + np;
  float4* S1 = S0 + np;
  float4* W = S1 + np;
  float2* P4 = reinterpret_cast<float2*>(W + np);
  float* hdr = reinterpret_cast<float*>(P4 + np);
  const float kappa = a.k * kLog2e, k2 = kappa * kappa;
  const float kr_first = kappa * a.radius[0];
  const float c0x = a.centers[0], c0y = a.centers[1], c0z = a.centers[2];
  float rmin = INFINITY, rmax = 0.0f, spread = 0.0f;
  const int ip = blockIdx.x * nt + threadIdx.x;
  if (ip < np) {
    float gx[2], gy[2], gz[2], cc[2], kr[2], rr[2], cr[2], cg[2], cb[2], w[2], wf[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = 2 * ip + h;
      if (j < a.M) {
        const float cx = a.centers[3 * j], cy = a.centers[3 * j + 1], cz = a.centers[3 * j + 2];
        const float r = a.radius[j];
        gx[h] = -2.0f * cx;
        gy[h] = -2.0f * cy;
        gz[h] = -2.0f * cz;
        cc[h] = cx * cx + cy * cy + cz * cz;
        kr[h] = kappa * r;
        rr[h] = r;
        if (a.colors_h != nullptr) {  // fp16 colours: widened exactly, blended in fp32
          cr[h] = (float)a.colors_h[3 * j];
          cg[h] = (float)a.colors_h[3 * j + 1];
          cb[h] = (float)a.colors_h[3 * j + 2];
        } else {
          cr[h] = a.colors[3 * j];
          cg[h] = a.colors[3 * j + 1];
          cb[h] = a.colors[3 * j + 2];
        }
        w[h] = fexp2(kr[h]);
        wf[h] = fexp2(kr[h] - kr_first);
        rmin = fminf(rmin, r);
        rmax = fmaxf(rmax, r);
        const float ex = cx - c0x, ey = cy - c0y, ez = cz - c0z;
        spread = fmaxf(spread, sqrtf(ex * ex + ey * ey + ez * ez));
      } else {
        // padding sphere at c = (kPadCenter, 0, 0): the expansion form (|c|^2) and the direct
        // form of the normal taps (p - c) both see distance ~1e15, so every exp() of its terms
        // underflows to exactly 0 (its weights are 0) and all of its gradient terms are 0.
        gx[h] = -2.0f * kPadCenter;
        gy[h] = gz[h] = 0.0f;
        cc[h] = kPadCenter * kPadCenter;
        kr[h] = rr[h] = cr[h] = cg[h] = cb[h] = w[h] = wf[h] = 0.0f;
      }
    }
    P0[ip] = make_float4(gx[0], gx[1], gy[0], gy[1]);
    P1[ip] = make_float4(gz[0], gz[1], cc[0], cc[1]);
    P2[ip] = make_float4(kr[0], kr[1], rr[0], rr[1]);
    P3[ip] = make_float4(cr[0], cr[1], cg[0], cg[1]);
    P4[ip] = make_float2(cb[0], cb[1]);
    S0[ip] = make_float4(k2 * gx[0], k2 * gx[1], k2 * gy[0], k2 * gy[1]);
    S1[ip] = make_float4(k2 * gz[0], k2 * gz[1], k2 * cc[0], k2 * cc[1]);
    W[ip] = make_float4(w[0], w[1], wf[0], wf[1]);
  }
  // matrix-core tiles of the march (lse_mfma)
  const int nrb = np / 8;
  char* tiles = reinterpret_cast<char*>(rec) + tiles_offset(np, gridDim.x);
  uint4* At = reinterpret_cast<uint4*>(tiles);
  float* Wt = reinterpret_cast<float*>(At + (size_t)nrb * 64);
  for (int e = blockIdx.x * nt + threadIdx.x; e < nrb * 64; e += gridDim.x * nt) At[e] = mfma_a_frag(a, e);
  for (int e = blockIdx.x * nt + threadIdx.x; e < nrb * 32; e += gridDim.x * nt) {
    const int j = mfma_w_sphere(e);
    const float krj = j < a.M ? kappa * a.radius[j] : 0.0f;
    Wt[e] = j >= a.M ? 0.0f : (mfma_w_fixed(e) ? fexp2(krj - kr_first) : fexp2(krj));
  }
  header_reduce(rmin, rmax, spread, gridDim.x == 1 ? hdr : hdr + (size_t)(1 + blockIdx.x) * kRecHeader);
  if (gridDim.x == 1) write_bound(a, hdr, reinterpret_cast<float*>(reinterpret_cast<char*>(rec) + esc_offset(np, 1)));
}

__global__ __launch_bounds__(256) void rm_prep_finish(const KArgs a, float* __restrict__ hdr, float* __restrict__ esc,
                                                      int nprep) {
  float rmin = INFINITY, rmax = 0.0f, spread = 0.0f;
  for (int b = threadIdx.x; b < nprep; b += 256) {
    const float* h = hdr + (size_t)(1 + b) * kRecHeader;
    rmin = fminf(rmin, h[0]);
    rmax = fmaxf(rmax, h[1]);
    spread = fmaxf(spread, h[2]);
  }
  header_reduce(rmin, rmax, spread, hdr);
  write_bound(a, hdr, esc);
}

// The per-view origin steps (write_origins), one 64-thread block (one wave) per view, after the
// records are complete: the views run on separate CUs side by side.
// A split launch's origin step runs its four quarters on four waves of the block (the split
// march's own combine: the same bits).
constexpr int kOriginXch = 64 * 36;  // bytes of march exchange per wave
template <bool SPLIT>
__global__ __launch_bounds__(SPLIT ? 64 * kSplitWaves : 64) void rm_origin_kernel(const KArgs a,
                                                                                 const float4* __restrict__ rec,
                                                                                 int nprep) {
  __shared__ __attribute__((aligned(16))) unsigned char xch[SPLIT ? kSplitWaves * kOriginXch + kSplitWaves * 64 * 4
                                                                  : kOriginXch];
  const int np = a.Mpad / 2;
  const uint4* At = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(rec) + tiles_offset(np, nprep));
  const float* Wt = reinterpret_cast<const float*>(At + (size_t)(np / 8) * 64);
  const float* hdr = reinterpret_cast<const float*>(reinterpret_cast<const float2*>(rec + 7 * (size_t)np) + np);
  write_origins<SPLIT>(a, rec[4 * np], rec[5 * np], hdr[1], hdr[2], At, Wt, a.origin, xch, blockIdx.x);
}

// ---- packed helpers --------------------------------------------------------------------------
__device__ __forceinline__ f2 sp(float x) { return f2{x, x}; }
__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 sqrt2(f2 q) { return f2{fsqrt(q.x), fsqrt(q.y)}; }
__device__ __forceinline__ f2 exp2v(f2 x) { return f2{fexp2(x.x), fexp2(x.y)}; }
__device__ __forceinline__ f2 rcp2(f2 x) { return f2{frcp(x.x), frcp(x.y)}; }
__device__ __forceinline__ f2 rsq2(f2 x) { return f2{frsq(x.x), frsq(x.y)}; }
// max(q, qmin) for qmin > 0 as one integer max on the bit patterns (non-negative floats order
// like their bits, negative ones have negative bit patterns): fmaxf in the kernels' IEEE mode
// costs a canonicalising v_max before the v_max. Equal to fmaxf for every non-NaN q.
__device__ __forceinline__ float qclamp(float q, float qmin) {
  return __int_as_float(max(__float_as_int(q), __float_as_int(qmin)));
}
__device__ __forceinline__ f2 clamp_q(f2 q) { return f2{qclamp(q.x, 1e-6f), qclamp(q.y, 1e-6f)}; }
__device__ __forceinline__ f2 lo(const float4& v) { return f2{v.x, v.y}; }
__device__ __forceinline__ f2 hi(const float4& v) { return f2{v.z, v.w}; }

// q = |p|^2 + |c|^2 - 2 p.c for a sphere pair (expansion form, scene.rs:66-71). Every sweep that
// must reproduce another sweep's distances bit for bit uses this one expression.
__device__ __forceinline__ f2 qpair(const f2& PX, const f2& PY, const f2& PZ, const f2& PP, const float4& A,
                                    const float4& B) {
  return fma2(PZ, lo(B), fma2(PY, hi(A), fma2(PX, lo(A), PP + hi(B))));
}
__device__ __forceinline__ float psq(const float p[3]) { return fmaf(p[2], p[2], fmaf(p[1], p[1], p[0] * p[0])); }

// The light direction ld / |ld| (renderer_diff.rs:49-50) and the Jacobian of that normalisation
// applied to summed per-ray terms r: component k of (r - ldn (ldn . r)) / |ld|. Contraction off in
// both: every kernel (general and small, forward and final blocks) forms them with the same fp32
// operations whatever code surrounds the call, so their bits cannot follow unrelated edits.
__device__ __forceinline__ float light_unit(const float* light_dir, float (&ln)[3]) {
#pragma clang fp contract(off)
  const float l0 = light_dir[0], l1 = light_dir[1], l2 = light_dir[2];
  const float len = sqrtf(l0 * l0 + l1 * l1 + l2 * l2);
  ln[0] = l0 / len;
  ln[1] = l1 / len;
  ln[2] = l2 / len;
  return len;
}
__device__ __forceinline__ float light_grad(const float (&r)[3], const float* light_dir, int k) {
#pragma clang fp contract(off)
  float ln[3];
  const float len = light_unit(light_dir, ln);
  const float proj = ln[0] * r[0] + ln[1] * r[1] + ln[2] * r[2];
  const float rk = k == 0 ? r[0] : (k == 1 ? r[1] : r[2]), lk = k == 0 ? ln[0] : (k == 1 ? ln[1] : ln[2]);
  return (rk - lk * proj) / len;
}

// A wave's 64 spheres' 8 record columns (lane = sphere, v[7] = 0) stored as two contiguous 1 KB
// runs: store h covers spheres 32 h .. 32 h + 31, lane l writing half (l & 1) of sphere
// 32 h + (l >> 1) (two half-line stores per lane would touch every line twice). Every lane of
// the wave calls it; nsph = the group's spheres below Mpad.
__device__ __forceinline__ void store_group_cols(float* rec_grp, const float (&v)[8], int lane, int nsph) {
  const int s = lane >> 1, hf = lane & 1;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    float o[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float lo = __shfl(v[c], 32 * h + s), hi = __shfl(v[4 + c], 32 * h + s);
      o[c] = hf ? hi : lo;
    }
    const int sph = 32 * h + s;
    if (sph < nsph) reinterpret_cast<float4*>(rec_grp)[2 * sph + hf] = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// ---- forward sweeps -----------------------------------------------------------------
// Base-2 log-sum-exp of v_j = kappa*(r_j - rho_j) over a tile (sdf.rs:36-40), running max m and
// shifted sum s carried across tiles; chunks of 16 spheres, one rescale exp per chunk.
// CLAMP=false drops max(q, 1e-6): only used when the caller proved every rho_j >= kSafeRho.
// Shift of the exponents: kShiftMax = chunked running max (always safe); kShiftFixed = m set
// once from the first sphere (safe when kappa * (r_max + max |c_j - c_0|) <= 100 and the point
// is near enough that fp32 rounding of rho stays small, so every exponent lies within +-100 of
// it); kShiftNone = m = 0 (safe when the hard maximum is known to lie in [-100, 100]). All three
// give the same log-sum-exp up to fp32 rounding.
enum LseShift { kShiftMax = 0, kShiftFixed = 1, kShiftNone = 2 };

template <bool CLAMP, int SHIFT>
__device__ __forceinline__ void lse_point(const float p[3], const Lds& L, int npairs, float nkappa, float& m,
                                          float& s) {
  const f2 PX = sp(p[0]), PY = sp(p[1]), PZ = sp(p[2]), PP = sp(psq(p)), NK = sp(nkappa);
  for (int i0 = 0; i0 < npairs; i0 += 8) {
    f2 v[8];
#pragma unroll
    for (int ii = 0; ii < 8; ++ii) {
      const float4 A = L.p0(i0 + ii), B = L.p1(i0 + ii);
      const float2 K = L.kr(i0 + ii);
      f2 q = qpair(PX, PY, PZ, PP, A, B);
      if constexpr (CLAMP) q = clamp_q(q);
      v[ii] = fma2(q * rsq2(q), NK, f2{K.x, K.y});  // rho = q rsq(q), as backward sweep 2
    }
    if constexpr (SHIFT != kShiftMax) {
      if constexpr (SHIFT == kShiftFixed) {
        if (m == -INFINITY) m = v[0].x;
      }
      const f2 MN = sp(m);
      f2 acc = f2{s, 0.0f};
#pragma unroll
      for (int ii = 0; ii < 8; ++ii) acc += exp2v(SHIFT == kShiftNone ? v[ii] : v[ii] - MN);
      s = acc.x + acc.y;
      continue;
    }
    float cm = fmaxf(v[0].x, v[0].y);
#pragma unroll
    for (int ii = 1; ii < 8; ++ii) cm = fmaxf(cm, fmaxf(v[ii].x, v[ii].y));
    const float mn = fmaxf(m, cm);
    const f2 MN = sp(mn);
    f2 acc = f2{s * fexp2(m - mn), 0.0f};
#pragma unroll
    for (int ii = 0; ii < 8; ++ii) acc += exp2v(v[ii] - MN);
    s = acc.x + acc.y;
    m = mn;
  }
}

// ---- the march's log-sum-exp on the matrix cores ---------------------------------------------
// q'_jn = k^2 |p_n - c_j|^2 for 16 spheres x 16 rays is one v_mfma_f32_16x16x32_bf16: every f32
// operand is split exactly into three bf16 parts (x = x1 + x2 + x3, truncation: each part keeps
// the next 8 significant bits), and the K = 32 products are the 30 split-part products that
// matter (a3 x3 is below 2^-30 of a x), all exact in fp32:
//   K slice 0: A = [a1x a1x a1x a1y a1y a1y a1z a1z]   B = Sa = [x1 x2 x3 y1 y2 y3 z1 z2]
//   K slice 1: A = [a2x a2x a2x a2y a2y a2y a2z a2z]   B = Sa
//   K slice 2: A = [a3x a3x 0   a3y a3y 0   a3z a3z]   B = Sa
//   K slice 3: A = [a1z a2z 1 1 1 C1 C2 C3]             B = Sb = [z3 z3 P1 P2 P3 1 1 1]
// with a = -2 k^2 c, C = k^2 |c|^2 (sphere side, rm_prep_kernel) and P = k^2 |p|^2 (ray side):
// sum = k^2 (|p|^2 - 2 p.c + |c|^2), the expansion form of scene.rs:66-71. The lanes then run
// only sqrt, exp2 and the weighted accumulate (lse_weighted's four packed ops per sphere pair
// go to the matrix pipe). Lane (n, g) = (l & 15, l >> 4) holds rays 16cb + n of the wave and
// spheres 16rb + 4g + v; the rays' Sa / Sb / shift go through a per-wave LDS exchange.
// Sum over the spheres of w_j 2^(-rho'_j) (FIXED = false; w = 2^(k r)) or w_j 2^(sh - rho'_j)
// (FIXED; w = 2^(k (r - r_0)), sh = the ray's own shift) for the lane's own ray -- the same sum
// as lse_weighted up to fp32 rounding. xa / xb / xs: this wave's LDS exchange (64 uint4, 64
// uint4, 64 floats).
// NCB < 4 (the split march's smaller ray groups, kSplitRays): the wave's lanes hold 16 NCB rays,
// lane l the ray of lane l mod 16 NCB; only the first NCB column blocks are multiplied and summed,
// and the reduction takes the missing blocks as copies of the present ones. A ray's sum is the
// same chain of the same terms as with NCB = 4 (the same bits; IEEE addition is commutative).
// PACK (the unsplit march's packed step, lse_mfma_packed): only the lanes with `live` set need
// their sum. Live lane l writes its ray into column `slot` = its rank among the live lanes, so
// the live rays fill the first NCB = ceil(live / 16) column blocks and only those are multiplied;
// the missing blocks add 0 to the reduction, which leaves lane s with the total of column s, and a
// live lane fetches its own from lane `slot`. The other lanes write nothing (the columns past the
// last live one hold stale fragments; a column touches no other column) and get no meaningful sum.
template <bool CLAMP, bool FIXED, int NCB = 4, bool PACK = false>
__device__ __forceinline__ float lse_mfma(const float p[3], float k2, float sh, const uint4* __restrict__ At,
                                          const float* __restrict__ Wt, int nrb, uint4* xa, uint4* xb, float* xs,
                                          int lane, int slot = 0, bool live = true) {
  // no fp contraction: the record kernel's origin step (write_origins) runs this code in another
  // kernel and must reproduce it bit for bit
#pragma clang fp contract(off)
  static_assert(PACK ? NCB >= 1 && NCB <= 3 : NCB == 1 || NCB == 2 || NCB == 4, "column blocks per wave");
  {  // the lane's own ray: Sa, Sb and the shift into the exchange
    unsigned x[3], y[3], z[3], P[3];
    split3(p[0], x[0], x[1], x[2]);
    split3(p[1], y[0], y[1], y[2]);
    split3(p[2], z[0], z[1], z[2]);
    split3(k2 * psq(p), P[0], P[1], P[2]);
    const int col = PACK ? slot : lane;
    if (!PACK || live) {
      xa[col] = make_uint4(pack2(x[0], x[1]), pack2(x[2], y[0]), pack2(y[1], y[2]), pack2(z[0], z[1]));
      xb[col] = make_uint4(pack2(z[2], z[2]), pack2(P[0], P[1]), pack2(P[2], kBf16One), pack2(kBf16One, kBf16One));
      if constexpr (FIXED) xs[col] = sh;
    }
  }
  __builtin_amdgcn_wave_barrier();
  const int n = lane & 15, g = lane >> 4;
  const uint4* src = g < 3 ? xa : xb;
  bf16x8 B[NCB];
  float S[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
    B[cb] = __builtin_bit_cast(bf16x8, src[16 * cb + n]);
    S[cb] = FIXED ? xs[16 * cb + n] : 0.0f;
  }
  const float QMIN = k2 * 1e-6f;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  if (nrb == 0) {  // an empty quarter of a split block
    __builtin_amdgcn_wave_barrier();
    return 0.0f;
  }
  // buffer loads: the row block's byte offset in a scalar register, the lane's offset fixed in a
  // vector register, no per-load 64-bit address arithmetic on the vector units (against global
  // loads the unsplit march +3 %, the split march +2 % once its quarter bounds are scalar)
  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)At, (short)0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw =
      __builtin_amdgcn_make_buffer_rsrc((void*)(Wt + (FIXED ? 16 : 0)), (short)0, 0x7fffffff, 0x00020000);
  const int va = lane * 16, vw = g * 16;
  auto load_a = [&](int rb) {
    return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(ra, va, rb * 1024, 0));
  };
  auto load_w = [&](int rb) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rw, vw, rb * 128, 0));
  };
  auto tile = [&](const bf16x8& A, f32x4 (&D)[NCB]) {
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) D[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, B[cb], zero, 0, 0, 0);
  };
  f2 acc2[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) acc2[cb] = sp(0.0f);
  auto consume = [&](const f32x4 (&D)[NCB], const float4& w) {
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      float q[4] = {D[cb].x, D[cb].y, D[cb].z, D[cb].w};
      const float wv[4] = {w.x, w.y, w.z, w.w};
      float rho[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        if constexpr (CLAMP) q[v] = qclamp(q[v], QMIN);
        rho[v] = fsqrt(q[v]);
      }
#pragma unroll
      for (int v = 0; v < 4; v += 2) {
        // FIXED: the shifted exponents two at a time (v_pk_add_f32: the same bits as two v_sub_f32)
        const f2 x = FIXED ? sp(S[cb]) - f2{rho[v], rho[v + 1]} : f2{-rho[v], -rho[v + 1]};
        acc2[cb] = fma2(f2{wv[v], wv[v + 1]}, f2{fexp2(x.x), fexp2(x.y)}, acc2[cb]);
      }
    }
  };
  // one tile at a time (registers: the march must not spill at 128 VGPRs); the fragments of the
  // next row block load while the lanes work on this one (nrb is even: Mpad % 32 == 0)
  f32x4 D[NCB];
  bf16x8 A = load_a(0);
  float4 w = load_w(0);
  for (int rb = 0; rb < nrb; rb += 2) {
    tile(A, D);
    const bf16x8 A1 = load_a(rb + 1);
    const float4 w1 = load_w(rb + 1);
    __builtin_amdgcn_sched_barrier(0);  // keep the loads a tile ahead of their use
    consume(D, w);
    __builtin_amdgcn_sched_barrier(0);
    tile(A1, D);
    const int rn = min(rb + 2, nrb - 1);
    A = load_a(rn);
    w = load_w(rn);
    __builtin_amdgcn_sched_barrier(0);
    consume(D, w1);
    __builtin_amdgcn_sched_barrier(0);
  }
  // partial sums of ray 16cb + n sit in the four lane groups: one transposing reduction (two
  // v_permlane32_swap and one v_permlane16_swap, no LDS) leaves lane (n, g) with the total of
  // its own ray 16g + n: rows 0/2 keep the column blocks 0/2 summed over lane bit 5, rows 1/3
  // the blocks 1/3, then each row adds its bit-4 partner
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) acc[cb] = acc2[cb].x + acc2[cb].y;
  // NCB < 4: column block cb + NCB is a copy of block cb (the lanes' rays repeat every 16 NCB);
  // PACK: the blocks not multiplied add 0
#pragma unroll
  for (int cb = NCB; cb < 4; ++cb) acc[cb] = PACK ? 0.0f : acc[cb - NCB];
  const float own = swap16_sum(swap32_sum(acc[0], acc[2]), swap32_sum(acc[1], acc[3]));
  __builtin_amdgcn_wave_barrier();  // the exchange is rewritten by the next step
  if constexpr (PACK) return u2f(__builtin_amdgcn_ds_bpermute(slot << 2, f2u(own)));  // column `slot`'s total
  return own;
}

// The unsplit march's step on the matrix cores for the `live` lanes only (bm = their ballot): the
// live rays packed into ncb = ceil(popc(bm) / 16) column blocks (lse_mfma, PACK), one loop per
// block count chosen by a scalar switch. More than 48 live rays need all four blocks: the wave
// runs the unpacked step, every lane in its own column (no rank, no fetch; the lanes that are not
// live get their sum as well). ncb == 0: no tile at all. A ray's sum does not depend on its
// column, so a live lane gets the bits of the unpacked step.
template <bool CLAMP, bool FIXED>
__device__ __forceinline__ float lse_mfma_packed(const float p[3], float k2, float sh, const uint4* __restrict__ At,
                                                 const float* __restrict__ Wt, int nrb, uint4* xa, uint4* xb,
                                                 float* xs, int lane, unsigned long long bm, bool live) {
  const int ncb = (__popcll(bm) + 15) >> 4;
  if (ncb == 4) return lse_mfma<CLAMP, FIXED, 4>(p, k2, sh, At, Wt, nrb, xa, xb, xs, lane);
  if (ncb == 0) return 0.0f;
  const int slot = __builtin_amdgcn_mbcnt_hi((unsigned)(bm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bm, 0u));
  if (ncb == 1) return lse_mfma<CLAMP, FIXED, 1, true>(p, k2, sh, At, Wt, nrb, xa, xb, xs, lane, slot, live);
  if (ncb == 2) return lse_mfma<CLAMP, FIXED, 2, true>(p, k2, sh, At, Wt, nrb, xa, xb, xs, lane, slot, live);
  return lse_mfma<CLAMP, FIXED, 3, true>(p, k2, sh, At, Wt, nrb, xa, xb, xs, lane, slot, live);
}

// Split march (RM_MARCH_SPLIT): the kSplitWaves waves of a block hold the same 64 rays; wave w
// sums the row blocks [part_rb(w), part_rb(w + 1)) (even bounds: lse_mfma runs pairs) and the
// partial sums are added in wave order, so every wave gets the same total. comb: 64 floats per
// wave of LDS.
__device__ __forceinline__ int part_rb(int nrb, int w) { return ((nrb * w) / kSplitWaves) & ~1; }
__device__ __forceinline__ float split_combine(float part, float* comb, int wave, int lane) {
  comb[wave * 64 + lane] = part;
  __syncthreads();
  float s = comb[lane];
#pragma unroll
  for (int w = 1; w < kSplitWaves; ++w) s += comb[w * 64 + lane];
  return s;
}
// A march step's soft-min D at p on the matrix cores without a shift (soft_min_march's
// unshifted step; shared with write_origins like march_d_fixed). comb != nullptr: a split
// block's wave, At / Wt / nrb its quarter (split_combine).
// PACK: the unsplit march's packed step (lse_mfma_packed) for the lanes with `live` set.
template <bool CLAMP, int NCB = 4, bool PACK = false>
__device__ __forceinline__ float march_d_none(const float p[3], float kappa, float inv_kappa,
                                              const uint4* __restrict__ At, const float* __restrict__ Wt, int nrb,
                                              uint4* xa, uint4* xb, float* xs, int lane, float* comb = nullptr,
                                              int wave = 0, unsigned long long bm = 0, bool live = true) {
#pragma clang fp contract(off)
  float s;
  if constexpr (PACK)
    s = lse_mfma_packed<CLAMP, false>(p, kappa * kappa, 0.0f, At, Wt, nrb, xa, xb, xs, lane, bm, live);
  else
    s = lse_mfma<CLAMP, false, NCB>(p, kappa * kappa, 0.0f, At, Wt, nrb, xa, xb, xs, lane);
  if (comb != nullptr) s = split_combine(s, comb, wave, lane);
  return -flog2(fmaxf(s, 1e-30f)) * inv_kappa;
}

// rho'_0 = k |p - c_0| (k = smooth_k log2 e) of sphere 0 from its records S00 / S1[0] = S10: the
// fixed shift of the march, and (rho'_0 - k r_0 >= k d_min) the unshifted form's admission test.
__device__ __forceinline__ float fixed_shift(const float p[3], float k2, const float4& S00, const float4& S10) {
#pragma clang fp contract(off)
  const float q0 = fmaf(p[2], S10.x, fmaf(p[1], S00.z, fmaf(p[0], S00.x, fmaf(k2, psq(p), S10.z))));
  return fsqrt(qclamp(q0, k2 * 1e-6f));
}

// A march step's soft-min D at p on the matrix cores with the fixed shift sh = rho'_0 (sphere 0;
// S00 / S10 = its records S0[0] / S1[0]) -- soft_min_march's fixed-shift step, shared with the
// per-view origin step (write_origins) so that both give the same bits.
template <bool CLAMP, int NCB = 4, bool PACK = false>
__device__ __forceinline__ float march_d_fixed(const float p[3], float kappa, float inv_kappa, float kr_first,
                                               const float4& S00, const float4& S10, const uint4* __restrict__ At,
                                               const float* __restrict__ Wt, int nrb, uint4* xa, uint4* xb,
                                               float* xs, int lane, float* comb = nullptr, int wave = 0,
                                               unsigned long long bm = 0, bool live = true) {
#pragma clang fp contract(off)
  const float k2 = kappa * kappa;
  const float sh = fixed_shift(p, k2, S00, S10);
  float s;
  if constexpr (PACK)
    s = lse_mfma_packed<CLAMP, true>(p, k2, sh, At, Wt, nrb, xa, xb, xs, lane, bm, live);
  else
    s = lse_mfma<CLAMP, true, NCB>(p, k2, sh, At, Wt, nrb, xa, xb, xs, lane);
  if (comb != nullptr) s = split_combine(s, comb, wave, lane);
  const float m = kr_first - sh;
  return -(flog2(fmaxf(s, 1e-30f)) + m) * inv_kappa;
}

// Camera mode: every ray of view v starts its march at the eye (camera.rs:83-85), so the first
// step's soft-min D(eye) is one number per view. Evaluated here once per view (one wave each) by
// the march's own code path for that step -- none = false (no previous step), the clamped
// sweep (no distance bound yet), fixed shift on the matrix cores -- it stands in for the step of
// every ray bit for bit (rm_ray_kernel). NaN where the first step would take another path
// (vector-only march, or the fixed shift not provably safe): those rays march it themselves.
// rec / hdr: this call's complete records and header; At / Wt: its march tiles; xch: 64 x 36 B
// of LDS. One wave computes view v.
template <bool PAR>
__device__ void write_origins(const KArgs& a, const float4& S00, const float4& S10, float rmax, float spread,
                              const uint4* At, const float* Wt, float* orig, unsigned char* xch, int v) {
  const int lane = threadIdx.x & 63;
  const int np = a.Mpad / 2;
  const float kappa = a.k * kLog2e, inv_kappa = 1.0f / kappa;
  const bool shift_fixed_ok = kappa * (rmax + spread) * 1.001f <= 100.0f;
  const bool shift_none_ok = kappa * rmax * 1.001f <= 30.0f;
  const float kr_first = kappa * a.radius[0];
  // PAR (a split launch, a block of kSplitWaves waves): wave w sums quarter w, combined in wave
  // order (split_combine) -- the split march's own sum; else one wave sums every row block
  const int wave = PAR ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;
  uint4* xa = reinterpret_cast<uint4*>(xch + wave * kOriginXch);
  uint4* xb = xa + 64;
  float* xs = reinterpret_cast<float*>(xa) + 64 * 8;
  float* comb = PAR ? reinterpret_cast<float*>(xch + kSplitWaves * kOriginXch) : nullptr;
  const int nrb = np / 8;
  const uint4* Aq = At;
  const float* Wq = Wt;
  int nq = nrb;
  if constexpr (PAR) {
    const int r0 = part_rb(nrb, wave);
    nq = part_rb(nrb, wave + 1) - r0;
    Aq += (size_t)r0 * 64;
    Wq += (size_t)r0 * 32;
  }
  {
    const CamBasis& cb = a.cams_dev != nullptr ? a.cams_dev[v] : a.cams[v];
    const float p[3] = {cb.eye[0], cb.eye[1], cb.eye[2]};
    float D = __builtin_nanf("");
    // the first step's choice in soft_min_march: unshifted when sphere 0 proves it safe, else
    // the fixed shift (else the vector path: not shared); block-uniform
    const bool none = a.mfma && shift_none_ok && fixed_shift(p, kappa * kappa, S00, S10) - kr_first <= 90.0f;
    // (a split launch's first step adds the four quarters' sums: the same here)
    if (none)
      D = march_d_none<true>(p, kappa, inv_kappa, Aq, Wq, nq, xa, xb, xs, lane, comb, wave);
    else if (a.mfma && shift_fixed_ok && psq(p) <= 1e10f)
      D = march_d_fixed<true>(p, kappa, inv_kappa, kr_first, S00, S10, Aq, Wq, nq, xa, xb, xs, lane, comb, wave);
    if (lane == 0 && wave == 0) orig[v] = D;
    // the eye's distance to the nearest sphere centre (direct form), rounded down by a relative
    // 1e-6 and 1e-6 (1 + |eye|) against the fp32 rounding of the eye and of the centres' offsets
    float m2 = INFINITY;
    for (int j = (int)threadIdx.x; j < a.M; j += (int)blockDim.x) {
      const float dx = p[0] - a.centers[3 * j], dy = p[1] - a.centers[3 * j + 1], dz = p[2] - a.centers[3 * j + 2];
      m2 = fminf(m2, fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m2 = fminf(m2, __shfl_xor(m2, off));
    if constexpr (PAR) {
      __shared__ float wmin[kSplitWaves];
      if (lane == 0) wmin[wave] = m2;
      __syncthreads();
#pragma unroll
      for (int w = 0; w < kSplitWaves; ++w) m2 = fminf(m2, wmin[w]);
    }
    if (lane == 0 && wave == 0)
      orig[RM_MAX_VIEWS_PER_CALL + v] =
          sqrtf(m2) * (1.0f - 1e-6f) - 1e-6f * (1.0f + fabsf(p[0]) + fabsf(p[1]) + fabsf(p[2]));
  }
}

// The march's log-sum-exp in weighted form: rho' = sqrt(k^2 q) = k rho straight from the scaled
// geometry, term = 2^(k r_j) 2^(-rho'_j) (FIXED = false: shift 0) or 2^(k (r_j - r_0))
// 2^(rho'_0 - rho'_j) (FIXED: shift v_0 = k r_0 - rho'_0) -- one packed fma per sphere pair
// instead of the fma + subtract + add of lse_point. Returns the sum; *sh receives rho'_0.
template <bool CLAMP, bool FIXED>
__device__ __forceinline__ float lse_weighted(const float p[3], const Lds& L, int npairs, float k2, float& sh) {
  const f2 PX = sp(p[0]), PY = sp(p[1]), PZ = sp(p[2]), PP = sp(k2 * psq(p)), QMIN = sp(k2 * 1e-6f);
  f2 acc[2] = {sp(0.0f), sp(0.0f)}, SH = sp(0.0f);  // two chains keep the fma latency hidden
  for (int i0 = 0; i0 < npairs; i0 += 8) {
#pragma unroll
    for (int ii = 0; ii < 8; ++ii) {
      const float4 A = Lds::v4(L.S0[i0 + ii]), B = Lds::v4(L.S1[i0 + ii]), Wt = Lds::v4(L.W[i0 + ii]);
      f2 q = qpair(PX, PY, PZ, PP, A, B);
      if constexpr (CLAMP) q = f2{qclamp(q.x, QMIN.x), qclamp(q.y, QMIN.y)};
      const f2 rho = sqrt2(q);
      if constexpr (FIXED) {
        if (i0 == 0 && ii == 0) SH = sp(rho.x);
        acc[ii & 1] = fma2(hi(Wt), exp2v(SH - rho), acc[ii & 1]);
      } else {
        acc[ii & 1] = fma2(lo(Wt), exp2v(-rho), acc[ii & 1]);
      }
    }
  }
  sh = SH.x;
  const f2 t = acc[0] + acc[1];
  return t.x + t.y;
}

// The six normal taps p +- eps*e_a (scene.rs:93-111) in one pass over the spheres. q at a tap
// is formed from e = p - c in direct form, |e +- eps e_a|^2 = |e|^2 + eps^2 +- 2 eps e_a, which
// keeps the fp32 error of the finite difference ~10x below the reference's expansion form.
template <bool CLAMP>
__device__ __forceinline__ void lse_taps(const float p[3], const Lds& L, int npairs, float nkappa, float two_eps,
                                         float eps2, float (&m)[6], float (&s)[6]) {
  const f2 PX = sp(p[0]), PY = sp(p[1]), PZ = sp(p[2]), NK = sp(nkappa), HALF = sp(0.5f), E2 = sp(eps2),
           TE = sp(two_eps), NTE = sp(-two_eps);
  for (int i0 = 0; i0 < npairs; i0 += 4) {
    f2 v[6][4];
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
      const float4 A = L.p0(i0 + ii), B = L.p1(i0 + ii);
      const float2 K = L.kr(i0 + ii);
      const f2 ex = fma2(HALF, lo(A), PX), ey = fma2(HALF, hi(A), PY), ez = fma2(HALF, lo(B), PZ);
      const f2 Q = fma2(ez, ez, fma2(ey, ey, fma2(ex, ex, E2)));
      f2 q[6] = {fma2(ex, TE, Q), fma2(ex, NTE, Q), fma2(ey, TE, Q), fma2(ey, NTE, Q), fma2(ez, TE, Q),
                 fma2(ez, NTE, Q)};
#pragma unroll
      for (int t = 0; t < 6; ++t) {
        if constexpr (CLAMP) q[t] = clamp_q(q[t]);
        v[t][ii] = fma2(sqrt2(q[t]), NK, f2{K.x, K.y});
      }
    }
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      float cm = fmaxf(v[t][0].x, v[t][0].y);
#pragma unroll
      for (int ii = 1; ii < 4; ++ii) cm = fmaxf(cm, fmaxf(v[t][ii].x, v[t][ii].y));
      const float mn = fmaxf(m[t], cm);
      const f2 MN = sp(mn);
      f2 acc = f2{s[t] * fexp2(m[t] - mn), 0.0f};
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) acc += exp2v(v[t][ii] - MN);
      s[t] = acc.x + acc.y;
      m[t] = mn;
    }
  }
}

// The six taps in weighted form (no shift, see lse_weighted): e' = k (p - c) from the unscaled
// records, q'_tap = |e'|^2 + (k eps)^2 +- 2 (k eps) e'_a = k^2 q_tap, term = 2^(k r) 2^(-sqrt(q')),
// one packed fma per tap and pair instead of fma + subtract + add + running max.
template <bool CLAMP>
__device__ __forceinline__ void lse_taps_w(const float p[3], const Lds& L, int npairs, float kappa, float eps,
                                           float (&s)[6]) {
  const f2 KPX = sp(kappa * p[0]), KPY = sp(kappa * p[1]), KPZ = sp(kappa * p[2]), HK = sp(0.5f * kappa),
           E2 = sp(kappa * kappa * eps * eps), TE = sp(2.0f * kappa * eps), NTE = sp(-2.0f * kappa * eps),
           QMIN = sp(kappa * kappa * 1e-6f);
  f2 acc[6];
#pragma unroll
  for (int t = 0; t < 6; ++t) acc[t] = sp(0.0f);
  for (int i0 = 0; i0 < npairs; i0 += 4) {
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
      const float4 A = L.p0(i0 + ii), B = L.p1(i0 + ii);
      const f4v Wt = L.W[i0 + ii];
      const f2 W = f2{Wt.x, Wt.y};
      const f2 ex = fma2(HK, lo(A), KPX), ey = fma2(HK, hi(A), KPY), ez = fma2(HK, lo(B), KPZ);
      const f2 Q = fma2(ez, ez, fma2(ey, ey, fma2(ex, ex, E2)));
      f2 q[6] = {fma2(ex, TE, Q), fma2(ex, NTE, Q), fma2(ey, TE, Q), fma2(ey, NTE, Q), fma2(ez, TE, Q),
                 fma2(ez, NTE, Q)};
#pragma unroll
      for (int t = 0; t < 6; ++t) {
        if constexpr (CLAMP) q[t] = f2{qclamp(q[t].x, QMIN.x), qclamp(q[t].y, QMIN.y)};
        acc[t] = fma2(W, exp2v(-sqrt2(q[t])), acc[t]);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 6; ++t) s[t] = acc[t].x + acc[t].y;
}

// Distances delta_j = rho_j - r_j at p_final for a pair (shade sweep and backward sweep 1 share it).
template <bool CLAMP>
__device__ __forceinline__ f2 delta_pair(const f2& PX, const f2& PY, const f2& PZ, const f2& PP, const float4& A,
                                         const float4& B, const float4& R, f2& q_out, f2& rho_out) {
  f2 q = qpair(PX, PY, PZ, PP, A, B);
  q_out = q;
  if constexpr (CLAMP) q = clamp_q(q);
  rho_out = sqrt2(q);
  return rho_out - hi(R);
}
// The same with rho = q rsq(q): one transcendental gives rho and 1/rho (r_out). The differentiable
// modes' shade sweep and backward sweep 1 both use this form, so their delta agree bit for bit.
template <bool CLAMP>
__device__ __forceinline__ f2 delta_pair_rsq(const f2& PX, const f2& PY, const f2& PZ, const f2& PP, const float4& A,
                                             const float4& B, const float4& R, f2& q_out, f2& r_out) {
  f2 q = qpair(PX, PY, PZ, PP, A, B);
  q_out = q;
  if constexpr (CLAMP) q = clamp_q(q);
  r_out = rsq2(q);
  return q * r_out - hi(R);
}

// Shared sweep at p_final: colour softmax over -csharp*delta (renderer_diff.rs:74-82) and the mask
// soft-min over -k*delta (renderer_diff.rs:86). Both maxima sit at min delta, so one running
// minimum dmin shifts both sums; exponents are (dmin - delta) <= 0 exactly (never overflow).
template <bool CLAMP>
__device__ __forceinline__ void shade_sweep(const float p[3], const Lds& L, int npairs, float c10l, float kappa,
                                            float& dmin, f2& Zw, f2 (&C)[3], f2& Zb) {
  const f2 PX = sp(p[0]), PY = sp(p[1]), PZ = sp(p[2]), PP = sp(psq(p)), CL = sp(c10l), KA = sp(kappa);
  for (int i0 = 0; i0 < npairs; i0 += 4) {
    f2 dl[4];
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
      f2 q, rho;
      dl[ii] = delta_pair<CLAMP>(PX, PY, PZ, PP, L.p0(i0 + ii), L.p1(i0 + ii), L.p2(i0 + ii), q, rho);
    }
    float cmin = fminf(dl[0].x, dl[0].y);
#pragma unroll
    for (int ii = 1; ii < 4; ++ii) cmin = fminf(cmin, fminf(dl[ii].x, dl[ii].y));
    const float dn = fminf(dmin, cmin);
    const f2 sw = sp(fexp2((dn - dmin) * c10l)), sb = sp(fexp2((dn - dmin) * kappa));
    Zw *= sw;
    C[0] *= sw;
    C[1] *= sw;
    C[2] *= sw;
    Zb *= sb;
    dmin = dn;
    const f2 DN = sp(dn);
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
      const f2 dd = DN - dl[ii];
      const f2 ew = exp2v(dd * CL), eb = exp2v(dd * KA);
      const float4 c3 = L.p3(i0 + ii);
      const float2 c4 = L.p4(i0 + ii);
      Zw += ew;
      C[0] = fma2(ew, lo(c3), C[0]);
      C[1] = fma2(ew, hi(c3), C[1]);
      C[2] = fma2(ew, f2{c4.x, c4.y}, C[2]);
      Zb += eb;
    }
  }
}

// The differentiable modes' sweep at p_final: shade_sweep's sums plus the detached normal
// (scene.rs:81-128, as its eps -> 0 limit f = 2 eps grad D) in the same pass. grad D =
// sum_j beta_j (p - c_j) / rho_j with beta = softmax(-k delta) -- the mask soft-min's own
// weights 2^(kappa (dmin - delta_j)) / Zb -- so G accumulates eb (p - c_j) rsq(q_j) next to Zb,
// rescaled with it when dmin moves (f = 2 eps G / Zb). One rsq per sphere gives rho and 1/rho.
template <bool CLAMP>
__device__ __forceinline__ void shade_normal_sweep(const float p[3], const Lds& L, int npairs, float c10l,
                                                   float kappa, float& dmin, f2& Zw, f2 (&C)[3], f2& Zb,
                                                   f2 (&G)[3]) {
  const f2 PX = sp(p[0]), PY = sp(p[1]), PZ = sp(p[2]), PP = sp(psq(p)), CL = sp(c10l), KA = sp(kappa),
           HALF = sp(0.5f);
  for (int i0 = 0; i0 < npairs; i0 += 4) {
    f2 dl[4], r[4];
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
      f2 q;
      dl[ii] = delta_pair_rsq<CLAMP>(PX, PY, PZ, PP, L.p0(i0 + ii), L.p1(i0 + ii), L.p2(i0 + ii), q, r[ii]);
      if constexpr (CLAMP) {  // clamp_min(1e-6): that distance is constant, no gradient
        r[ii].x = q.x >= 1e-6f ? r[ii].x : 0.0f;
        r[ii].y = q.y >= 1e-6f ? r[ii].y : 0.0f;
      }
    }
    float cmin = fminf(dl[0].x, dl[0].y);
#pragma unroll
    for (int ii = 1; ii < 4; ++ii) cmin = fminf(cmin, fminf(dl[ii].x, dl[ii].y));
    const float dn = fminf(dmin, cmin);
    const f2 sw = sp(fexp2((dn - dmin) * c10l)), sb = sp(fexp2((dn - dmin) * kappa));
    Zw *= sw;
    C[0] *= sw;
    C[1] *= sw;
    C[2] *= sw;
    Zb *= sb;
    G[0] *= sb;
    G[1] *= sb;
    G[2] *= sb;
    dmin = dn;
    const f2 DN = sp(dn);
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
      const f2 dd = DN - dl[ii];
      const f2 ew = exp2v(dd * CL), eb = exp2v(dd * KA);
      const float4 c3 = L.p3(i0 + ii), A = L.p0(i0 + ii), B = L.p1(i0 + ii);
      const float2 c4 = L.p4(i0 + ii);
      Zw += ew;
      C[0] = fma2(ew, lo(c3), C[0]);
      C[1] = fma2(ew, hi(c3), C[1]);
      C[2] = fma2(ew, f2{c4.x, c4.y}, C[2]);
      Zb += eb;
      const f2 wr = eb * r[ii];  // p - c = 0.5 (-2c) + p, exactly as the backward's
      G[0] = fma2(wr, fma2(HALF, lo(A), PX), G[0]);
      G[1] = fma2(wr, fma2(HALF, hi(A), PY), G[1]);
      G[2] = fma2(wr, fma2(HALF, lo(B), PZ), G[2]);
    }
  }
}

// ---- the fused per-ray kernel ----------------------------------------------------------
// Does the ray provably end (after `steps` march steps, or at the given march t) at scene
// distance >= min_d, beyond its closest approach to the scene's bounding sphere (c0, R)?
//  * Every sphere distance is >= |p - c0| - R, and the soft-min is >= the hard min minus
//    ln(M)/k (sdf.rs:30-44), so g(t) = |o + d t - c0| - R - ln(M)/k never exceeds the march
//    step D(t). Shrinking g by a relative 1e-5 and an absolute 1e-5 (R + |c0| + 1) covers the
//    f32 rounding of the march (expansion-form distances err by ~6e-8 |p|).
//  * t + g(t) is non-decreasing (g is (1 - 1e-5)-Lipschitz), so the f64 march of g alone,
//    tau <- tau + g(tau), stays below the real t at every step (induction from t = tau = 0).
//  * Past the closest approach g only grows; so tau_S >= t_closest and g(tau_S) >= min_d give
//    D >= min_d at the march end, at the reconnected point t + D (renderer_diff.rs:30-39) and
//    hence for the mask, which is then exactly 0 -- as are out and every gradient term.
__device__ __forceinline__ bool escapes(const float o[3], const float d[3], float t_given, bool have_t, int steps,
                                     const float c0[3], float R, float slack, float min_d) {
  const double eps = 1e-5;
  const double ox = (double)o[0] - c0[0], oy = (double)o[1] - c0[1], oz = (double)o[2] - c0[2];
  const double dx = d[0], dy = d[1], dz = d[2];
  const double Rs = (double)R + (double)slack;
  const double K = eps * (Rs + sqrt((double)c0[0] * c0[0] + (double)c0[1] * c0[1] + (double)c0[2] * c0[2]) + 1.0);
  auto g = [&](double tt) {
    const double x = fma(dx, tt, ox), y = fma(dy, tt, oy), z = fma(dz, tt, oz);
    return (1.0 - eps) * (sqrt(x * x + y * y + z * z) - Rs) - K;
  };
  const double tc = -(ox * dx + oy * dy + oz * dz) / (dx * dx + dy * dy + dz * dz);
  double tau = 0.0;
  if (have_t) {
    tau = t_given;
  } else {
    for (int s = 0; s < steps; ++s) tau += g(tau);
  }
  return tau >= tc && g(tau) >= (double)min_d;
}

// The cost-ordered dispatch's list sets of this launch: with a.oturn the pointers of KArgs are
// set 0's and the sets follow the device turn word w: read (w + 2) % 3, append w, clear (w + 1) % 3.
struct OrderSets {
  const int* list_r;
  const int* cnt_r;
  int* list_w;
  int* cnt_w;
  int* cnt_z;
};
__device__ __forceinline__ OrderSets order_sets(const KArgs& a) {
  OrderSets o{a.olist_r, a.ocnt_r, a.olist_w, a.ocnt_w, a.ocnt_z};
  if (a.oturn != nullptr) {
    const int w = __builtin_amdgcn_readfirstlane(*a.oturn);
    const int r = (w + 2) % 3, z = (w + 1) % 3;
    constexpr long long kSet = (long long)RM_ORDER_CLASSES * kMaxBlocksPerLaunch;
    if (o.list_r != nullptr) {
      o.list_r += r * kSet;
      o.cnt_r += r * RM_ORDER_CNT_STRIDE;
    }
    if (o.list_w != nullptr) {
      o.list_w += w * kSet;
      o.cnt_w += w * RM_ORDER_CNT_STRIDE;
    }
    if (o.cnt_z != nullptr) o.cnt_z += z * RM_ORDER_CNT_STRIDE;
  }
  return o;
}

// Launch position -> logical ray block. With block_order (whole 16x16-tiled views per launch) the
// blocks are dispatched tile rank by tile rank, the views interleaved, in the order of
// block_order: the tiles nearest the image centre -- where the scene usually is, and so the
// rays that march all their steps -- first, the cheap border tiles last, where they fill the
// machine while the heavy blocks finish. Partials stay indexed by the logical block, so the
// gradient sums (and every result) do not depend on the order.
__device__ __forceinline__ long long ray_block(const KArgs& a) {
  int b = blockIdx.x;
  if (a.block_order == nullptr) return b;
  // The dispatcher hands block i to XCD i % 8. With the views interleaved (b = rank * V + v),
  // V = 2 or 4 would pin each view to a fixed subset of XCDs, and views differ in cost (how much
  // of the scene they see): the XCDs of the dearest view finish last. Rotating the positions
  // inside every full round of 8 blocks by the round number makes each XCD cycle through all
  // views (rank order is kept up to 8 positions, so heavy tiles still start first).
  const int g = b >> 3;
  if ((g + 1) * 8 <= (int)gridDim.x) b = (g << 3) + (((b & 7) + g) & 7);
  const OrderSets os = order_sets(a);
  if (os.cnt_r != nullptr) {
    // position b of the class-major concatenation of the previous launch's lists; every block
    // reads the same counts, so a short total (never expected) sends all blocks to the static order
    int tot = 0, cb = -1, base = 0;
#pragma unroll
    for (int c = 0; c < RM_ORDER_CLASSES; ++c) {
      const int n = os.cnt_r[c * RM_ORDER_CLS_STRIDE];
      if (cb < 0 && b < tot + n) {
        cb = c;
        base = tot;
      }
      tot += n;
    }
    if (tot == (int)gridDim.x && cb >= 0) return os.list_r[cb * kMaxBlocksPerLaunch + (b - base)];
  }
  const int r = b / a.order_views, v = b - r * a.order_views;
  return (long long)v * a.order_tiles + a.block_order[r];
}

// Appends the block to its cost class's list for the next launch's dispatch order (class 0: the
// dearest blocks; cost in march-step units, see the hand-off in rm_ray_kernel).
__device__ __forceinline__ void order_append(const KArgs& a, long long blk, int cost) {
  constexpr int kCls = RM_ORDER_CLASSES;
  const float cls_scale = (float)kCls / (float)((a.split ? 1 : kWaves) * (a.steps + kPostCost) + 1);
  const int c = kCls - 1 - (int)fminf((float)cost * cls_scale, (float)(kCls - 1));
  const OrderSets os = order_sets(a);
  const int idx = atomicAdd(os.cnt_w + c * RM_ORDER_CLS_STRIDE, 1);
  // counts left uncleared (a failed launch in the rotation) overrun the total, and ray_block
  // then falls back to the static order: never write past the list
  if (idx < kMaxBlocksPerLaunch) os.list_w[c * kMaxBlocksPerLaunch + idx] = (int)blk;
}

// compute_loss's progress (training.rs:17-34 weights): the call's argument, or with device step
// scalars bound (rm_bind_step_scalars) index / total in fp32 as train.rs:171-172 forms it.
__device__ __forceinline__ float progress_of(const KArgs& a) {
  if (a.sdev == nullptr) return a.progress;
  return fminf((float)a.sdev->index / (float)a.sdev->total, 1.0f);
}

// A block of escaping rays: out = 0 (requested outputs), zero gradient partials, and for the
// train step the L1 loss of out = 0, reduced exactly as in the full path.
template <int MODE>
__device__ __forceinline__ void escaped_block(const KArgs& a, const Lds& L, long long blk, long long ri, bool valid,
                                           int tid, int lane, int wave) {
  if (MODE != kBwd && a.out != nullptr && valid) {
    a.out[3 * ri] = 0.0f;
    a.out[3 * ri + 1] = 0.0f;
    a.out[3 * ri + 2] = 0.0f;
  }
  if constexpr (MODE == kFwd || MODE == kRender) return;
  float* rec = a.partials + blk * a.rec;  // per-sphere columns stay unwritten: live flag 0
  float loss = 0.0f;
  if (MODE == kTrain && valid) {  // training.rs:17-34 with out = 0
    const float t0 = a.targets[3 * ri], t1 = a.targets[3 * ri + 1], t2 = a.targets[3 * ri + 2];
    const float W = (t0 + t1 + t2) > 0.01f ? 10.0f : fmaf(progress_of(a), 4.0f, 1.0f);
    const float tg[3] = {t0, t1, t2};
#pragma unroll
    for (int c = 0; c < 3; ++c) loss = fmaf(fabsf(0.0f - tg[c]), W, loss);
  }
  const float vals[8] = {0.0f, 0.0f, 0.0f, 0.0f, loss, 0.0f, 0.0f, 0.0f};
  const float red = wave_reduce8(vals, lane);
  if ((lane & 7) == 7) L.slots[wave * 8 + (lane >> 3)] = red;
  __syncthreads();
  if (tid < 8) {
    float acc = L.slots[tid];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) acc += L.slots[w * 8 + tid];
    rec[(long long)a.Mpad * 8 + tid] = acc;
  }
}

// Ray of thread row ri (camera.rs:58-87 in camera mode). In camera mode ri is remapped from
// the launch order (16x16 pixel tiles per block, 8x8 per wave) to the pixel's row of the
// [N,3] tensors.
template <bool CAM>
__device__ __forceinline__ void setup_ray(const KArgs& a, long long& ri, float o[3], float d[3], int& view) {
  view = 0;
  if constexpr (CAM) {
    const long long npix = (long long)a.width * a.height;
    const int v = (int)(ri / npix);
    view = v;
    const long long pix = ri - (long long)v * npix;
    int x, y;
    if (a.tiling == 2) {
      // a block takes a 16x16 tile, each wave an 8x8 quadrant: compact ray bundles keep the
      // wave-uniform fast paths on and let whole blocks pass the escape test
      const long long tl = pix >> 8;
      const int w = (int)(pix & 255), tiles_x = a.width >> 4;
      const int ty = (int)(tl / tiles_x), tx = (int)(tl - (long long)ty * tiles_x);
      const int qd = w >> 6, l = w & 63;
      y = (ty << 4) + ((qd >> 1) << 3) + (l >> 3);
      x = (tx << 4) + ((qd & 1) << 3) + (l & 7);
    } else {
      y = (int)(pix / a.width);
      x = (int)(pix - (long long)y * a.width);
    }
    ri = (long long)v * npix + (long long)y * a.width + x;
    if (a.cams_dev != nullptr) camera_ray(a.cams_dev[v], x, y, a.width, a.height, o, d);
    else camera_ray(a.cams[v], x, y, a.width, a.height, o, d);
  } else {
    o[0] = a.org[3 * ri];
    o[1] = a.org[3 * ri + 1];
    o[2] = a.org[3 * ri + 2];
    d[0] = a.dir[3 * ri];
    d[1] = a.dir[3 * ri + 1];
    d[2] = a.dir[3 * ri + 2];
  }
}

// Escape pre-pass (RM_MARCH_SKIP_ESCAPED): one thread per ray of the coming per-ray launch
// (same blocks, same rays); flags[b] = 1 when every ray of block b escapes. Kept out of the
// per-ray kernel so its f64 arithmetic costs that kernel no registers.
template <int MODE, bool CAM>
__global__ __launch_bounds__(kBlock) void rm_escape_kernel(const KArgs a, int* __restrict__ flags) {
  __shared__ float scratch[8 * kWaves];
  const int tid = threadIdx.x;
  const long long blk = ray_block(a);
  const long long li = blk * kBlock + tid;
  const bool valid = li < a.n_rays;
  long long ri = a.ray_begin + (valid ? li : 0);
  float o[3], d[3];
  int view;
  setup_ray<CAM>(a, ri, o, d, view);
  float c0[3], R;
  scene_bound(a, scratch, tid, c0, R);
  const bool have_t = MODE == kBwd && a.t_in != nullptr;
  const bool esc = !valid || escapes(o, d, have_t ? a.t_in[ri] : -1.0f, have_t, a.steps, c0, R, a.lse_slack,
                                     a.cull_min_d);
  const int all = __syncthreads_and(esc);
  if (tid == 0) flags[blk] = all;
}

template <int MODE, bool CAM, bool SPLIT>
__device__ __forceinline__ void ray_body(const KArgs& a);

// The per-ray kernel. Measurement build (-DRM_BLOCK_TRACE): every wave also records {start, end}
// (s_memrealtime, 100 MHz), its hardware slot (HW_ID | XCC_ID << 32), {logical block, launch
// position}, the times its march and its post-march forward ended and its march steps saved into
// a.btrace[kTraceWords * (blockIdx.x * kWaves + wave) ...] (tools/block_trace.py).
// SPLIT: the split march (RM_MARCH_SPLIT, KArgs::split).
template <int MODE, bool CAM, bool SPLIT>
__device__ __forceinline__ void ray_entry(const KArgs& a) {
#ifdef RM_BLOCK_TRACE
  const unsigned long long t_begin = __builtin_amdgcn_s_memrealtime();
  ray_body<MODE, CAM, SPLIT>(a);
  const unsigned long long t_end = __builtin_amdgcn_s_memrealtime();
  if (a.btrace != nullptr && (threadIdx.x & 63) == 0) {
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_REG_HW_ID
    const unsigned xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);  // HW_REG_XCC_ID
    unsigned long long* r = a.btrace + kTraceWords * ((unsigned long long)blockIdx.x * kWaves + (threadIdx.x >> 6));
    r[0] = t_begin;
    r[1] = t_end;
    r[2] = (unsigned long long)hw | ((unsigned long long)xcc << 32);
    r[3] = (unsigned long long)ray_block(a) | ((unsigned long long)blockIdx.x << 32);
  }
#else
  ray_body<MODE, CAM, SPLIT>(a);
#endif
}
template <int MODE, bool CAM, bool SPLIT>
__global__ __launch_bounds__(kBlock, SPLIT ? RM_SPLIT_MIN_WAVES : kMinWavesPerSimd) void rm_ray_kernel(const KArgs a) {
  ray_entry<MODE, CAM, SPLIT>(a);
}
// The split continuation launch (KArgs::cont_resume > 0) as its own kernel: the same code at the
// register budget RM_CONT_MIN_WAVES (waves per SIMD), so that more of its blocks are resident at once.
template <int MODE, bool CAM>
__global__ __launch_bounds__(kBlock, RM_CONT_MIN_WAVES) void rm_cont_kernel(const KArgs a) {
  ray_entry<MODE, CAM, true>(a);
}

// Split march (SPLIT): a block takes 64 rays (one 8x8 quadrant of a 16x16 tile in camera mode)
// and all four of its waves hold them; every march step each wave sums a quarter of the sphere
// row blocks on the matrix cores and the quarters are added in wave order (split_combine), so
// the four waves march in lockstep through identical decisions (shift, clamp, exit). After the
// march only wave 0 goes on (post-march forward, backward); the others end as escaped waves
// with zero contributions. A ray that marches every step then occupies four SIMDs instead of one.
template <int MODE, bool CAM, bool SPLIT>
__device__ __forceinline__ void ray_body(const KArgs& a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Lds L;
  {
    const int np = a.Mpad / 2;
    L.P0 = (cf4_ptr)a.rec_buf;
    L.P1 = L.P0 + np;
    L.P2 = L.P1 + np;
    L.P3 = L.P2 + np;
    L.S0 = L.P3 + np;
    L.S1 = L.S0 + np;
    L.W = L.S1 + np;
    L.P4 = (cf2_ptr)(L.W + np);
    L.At = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(a.rec_buf) + tiles_offset(np, (np + 255) / 256));
    L.Wt = reinterpret_cast<const float*>(L.At + (size_t)(np / 8) * 64);
  }
  L.slots = reinterpret_cast<float*>(smem);
  L.misc = L.slots + kSlotBytes / sizeof(float);

  // wave: the wave's index, made scalar (readfirstlane) so that everything derived from it -- a
  // split wave's quarter of the row blocks, its loop bounds and fragment addresses, LDS slots --
  // stays wave-uniform for the compiler (threadIdx-derived values are otherwise vector values)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  long long blk;
  // ray_cont (ray mode): this block marches listed rays [32 b, 32 b + 32) of ray_list, one per lane
  // (lanes l and l + 32 the same ray); lanes past the list's end are invalid copies of its first
  long long li_listed = -1;
  bool listed = true;
  if (SPLIT && a.cont_resume > 0 && a.ray_cont) {
    const int n = *a.ray_count;
    const int i0 = (int)blockIdx.x * kSplitRays;
    if (i0 >= n) return;
    const int i = i0 + (lane & (kSplitRays - 1));
    listed = i < n;
    li_listed = a.ray_list[listed ? i : i0];
    blk = -1;  // no group of its own
  } else if (SPLIT && a.cont_resume > 0) {  // resume launch: the groups the first launch deferred
    if ((int)blockIdx.x >= *a.cont_count) return;
    blk = a.cont_list[blockIdx.x];
  } else {
    blk = ray_block(a);
  }
  // SPLIT: lane l holds ray l mod kSplitRays of the group (kSplitRays < 64: copies, see kSplitRays)
  const long long li = li_listed >= 0 ? li_listed
                                      : (SPLIT ? blk * kSplitRays + (lane & (kSplitRays - 1)) : blk * kBlock + tid);
  const bool valid = listed && li < a.n_rays;
  long long ri = a.ray_begin + (valid ? li : 0);  // becomes the ray's row in the [N,3] tensors
  // the wave that writes this ray's outputs; SPLIT: all four waves run the post-march forward
  // (each over a quarter of the spheres, merged) and wave w seeds the backward of the group's rays
  // [w R / 4, (w + 1) R / 4) (R = kSplitRays; lanes past R carry copies and seed nothing)
  const bool own_rays = !SPLIT || (wave == 0 && lane < kSplitRays);
  const bool seed_lane = !SPLIT || (wave == 0 && lane < kSplitRays);

  const float kappa = a.k * kLog2e, nkappa = -kappa, inv_kappa = 1.0f / kappa;

  // ray (camera.rs:58-87 in camera mode)
  float o[3], d[3];
  int view;
  setup_ray<CAM>(a, ri, o, d, view);

  // ---- escape skip (RM_MARCH_SKIP_ESCAPED): a block whose rays all provably leave the scene
  // (rm_escape_kernel) gets out = 0 and zero gradients without marching -- exactly what the full
  // computation yields for them, since their silhouette mask is 0 in f32 (see escapes()).
  if (a.ocnt_z != nullptr && blockIdx.x == 0 && tid < RM_ORDER_CLASSES) order_sets(a).cnt_z[tid * RM_ORDER_CLS_STRIDE] = 0;
  if (a.esc_flags != nullptr && blk >= 0 && a.esc_flags[blk]) {
    if (a.stats != nullptr && tid == 0) atomicAdd(a.stats, 1ull);
    if (a.ocnt_w != nullptr && tid == 0) order_append(a, blk, 0);
    escaped_block<MODE>(a, L, blk, ri, valid, tid, lane, wave);
    return;
  }

  // Scene radius bounds from the record header: with r_min, a lower bound on the scene distance
  // proves rho_j = dist_j + r_j >= kSafeRho for every sphere, so max(q, 1e-6) cannot bind and
  // the sweeps may skip it (exactly the same results).
  const cf1_ptr hdr = (cf1_ptr)(L.P4 + a.Mpad / 2);
  const float rmin = hdr[0], rmax = hdr[1], spread = hdr[2];
  // Block-uniform permissions for the cheaper log-sum-exp shifts of the march:
  // |v_j - v_0| = kappa |r_j - r_0 - (rho_j - rho_0)| <= kappa (r_max + |c_j - c_0|); v <= kappa r_max;
  // the weighted form 2^(k r) 2^(-k rho) also needs 2^(-k rho) of the nearest sphere normal:
  // k rho <= 90 + k r_max <= 120
  // (RM_MARCH_FORCE_MAX_SHIFT: neither, every step takes the running maximum -- tests)
  const bool shift_fixed_ok = !a.shift_max && kappa * (rmax + spread) * 1.001f <= 100.0f;
  const bool shift_none_ok = !a.shift_max && kappa * rmax * 1.001f <= 30.0f;
  const float kr_first = kappa * a.radius[0];
  // Wave-uniform choice of the clamp-free path from a per-lane lower bound on the distance.
  // Rays proven to escape (`gone`, see the march) no longer take part in the wave-uniform
  // choices: their outputs and gradient terms are exactly 0 whatever they compute.
  bool gone = false;
  // Ray mode: the ray's state repeats with period 2; its t is final (see the march)
  bool retired = false;
  // A second proof per ray (camera mode): rho_lb, a lower bound on the distance to the nearest
  // sphere CENTRE -- the eye's (write_origins), less the path marched since (every centre distance
  // is 1-Lipschitz along the ray). Where the soft-min runs far below the hard min (small k: at
  // k = 5 by up to ln(M)/k = 1.1) the scene-distance bound above fails inside the scene long
  // before any centre comes near; either proof skips the clamp, with the same bits.
  float rho_lb = -INFINITY;
  const float onorm = fabsf(o[0]) + fabsf(o[1]) + fabsf(o[2]);
  // rho_lb after the ray moved from march distance t0 to t1 (|d| <= 1 + 1e-6; the fp32 rounding of
  // both points p = o + d t, ~1.1e-7 (|o|_1 + 1.74 t) each, inside the absolute 1e-6 (1 + |o|_1 + t))
  auto rho_moved = [&](float rl, float t0, float t1) {
    return rl - (fabsf(t1 - t0) * 1.000001f + 1e-6f * (1.0f + onorm + fmaxf(t0, t1)));
  };
  auto all_safe = [&](float dist_lb, float rlb) {
    return __all(dist_lb + rmin >= kSafeRho || rlb >= kSafeRho || gone) != 0;
  };
  int split_par = 0;  // SPLIT: which of the two combine buffers the next step uses

  // every sweep visits all sphere pairs in one pass (records are not staged)
  auto for_tiles = [&](auto&& body) { body(0, a.Mpad); };
  // soft-min scene SDF at one point (scene.rs:60-79 + sdf.rs:30-44); returns D, keeps (m, s)
  auto soft_min = [&](const float p[3], bool fast, float& m, float& s) {
    m = -INFINITY;
    s = 0.0f;
    if (fast)
      for_tiles([&](int, int tn) { lse_point<false, kShiftMax>(p, L, tn / 2, nkappa, m, s); });
    else
      for_tiles([&](int, int tn) { lse_point<true, kShiftMax>(p, L, tn / 2, nkappa, m, s); });
    return -(flog2(fmaxf(s, 1e-8f)) + m) * inv_kappa;
  };
  // SPLIT: the post-march vector sweeps of a 64-ray block run on its four waves, wave w over the
  // pairs [split_pair(w), split_pair(w + 1)) (multiples of 8), and the partial states are merged
  // through LDS in wave order (every wave then holds the same totals).
  auto split_pair = [&](int w) { return (((a.Mpad / 2) * w) / kSplitWaves) & ~7; };
  auto soft_min_split = [&](const float p[3], bool fast, float& m, float& s) {
    const int b0 = split_pair(wave), b1 = split_pair(wave + 1);
    const Lds Lq = L.from_pair(b0);
    m = -INFINITY;
    s = 0.0f;
    if (fast) lse_point<false, kShiftMax>(p, Lq, b1 - b0, nkappa, m, s);
    else lse_point<true, kShiftMax>(p, Lq, b1 - b0, nkappa, m, s);
    float* xm = L.slots;
    float* xs = L.slots + kSplitWaves * 64;
    __syncthreads();  // the march's last exchange is read
    xm[wave * 64 + lane] = m;
    xs[wave * 64 + lane] = s;
    __syncthreads();
    float mm = xm[lane];
#pragma unroll
    for (int w = 1; w < kSplitWaves; ++w) mm = fmaxf(mm, xm[w * 64 + lane]);
    float ss = 0.0f;
#pragma unroll
    for (int w = 0; w < kSplitWaves; ++w) ss += xs[w * 64 + lane] * fexp2(xm[w * 64 + lane] - mm);
    m = mm;
    s = ss;
    return -(flog2(fmaxf(s, 1e-8f)) + m) * inv_kappa;
  };
  // shade_normal_sweep's state (dmin; colour sums at c10l, mask and normal sums at kappa, each
  // relative to dmin) merged over the four waves; the totals come back in the .x lanes
  auto shade_merge = [&](float c10l, float& dmin, f2& Zw, f2 (&C)[3], f2& Zb, f2 (&G)[3]) {
    constexpr int kF = 9;
    float* xb = L.slots + 2 * kSplitWaves * 64;  // [kF][wave][64], after soft_min_split's buffers
    const float v[kF] = {dmin, Zw.x + Zw.y, C[0].x + C[0].y, C[1].x + C[1].y, C[2].x + C[2].y,
                         Zb.x + Zb.y, G[0].x + G[0].y, G[1].x + G[1].y, G[2].x + G[2].y};
#pragma unroll
    for (int f = 0; f < kF; ++f) xb[(f * kSplitWaves + wave) * 64 + lane] = v[f];
    __syncthreads();
    float dm = xb[lane];
#pragma unroll
    for (int w = 1; w < kSplitWaves; ++w) dm = fminf(dm, xb[w * 64 + lane]);
    float acc[kF - 1] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int w = 0; w < kSplitWaves; ++w) {
      const float dw = xb[w * 64 + lane];
      const float sw = fexp2((dm - dw) * c10l), sb = fexp2((dm - dw) * kappa);
#pragma unroll
      for (int f = 1; f < kF; ++f) acc[f - 1] = fmaf(xb[(f * kSplitWaves + w) * 64 + lane], f < 5 ? sw : sb, acc[f - 1]);
    }
    dmin = dm;
    Zw = f2{acc[0], 0.0f};
    C[0] = f2{acc[1], 0.0f};
    C[1] = f2{acc[2], 0.0f};
    C[2] = f2{acc[3], 0.0f};
    Zb = f2{acc[4], 0.0f};
    G[0] = f2{acc[5], 0.0f};
    G[1] = f2{acc[6], 0.0f};
    G[2] = f2{acc[7], 0.0f};
  };
  // The march's soft-min with the cheapest safe shift (the result differs only by fp32 rounding).
  // kShiftNone needs the hard maximum -kappa d_min >= -100 at the new point: d_min(new) <=
  // d_min(old) + |D| <= D + ln(M)/k + |D| (the soft-min is within ln(M)/k below the hard min).
#ifdef RM_BLOCK_TRACE
  // measurement build: march steps per path (16 bits each: none fast, none clamped, fixed fast,
  // fixed clamped), shader cycles inside the matrix-core steps, vector-path steps
  unsigned long long tr_paths = 0, tr_lse_cyc = 0, tr_vec = 0;
#endif
  // What the unsplit march's packed step reads of the march's state (see the march): the ray's t
  // now, one and two steps back (the cycle exit's history), the D of the step two back (Dprev is
  // the D one step back) and the wave's choice history.
  struct Memo {
    float t, t1, t2, D2;
    int chist;
  };
  int skipped_cb = 0;  // wave-uniform: column blocks the packed steps did not multiply (work statistics)
  // choice: the step's wave-uniform choices, bit 0 unshifted, bit 1 fixed shift, bit 2 clamp-free
  // force: 0 the cheapest safe shift for the wave (above); 1 the fixed shift, 2 the running maximum,
  // 3 unshifted (ray mode: see soft_min_march)
  auto soft_min_core = [&](const float p[3], bool fast, float Dprev, int& choice, int force, const Memo& mm) {
    bool none = force == 3 || (force == 0 && shift_none_ok &&
                __all(2.0f * fmaxf(Dprev, 0.0f) + a.lse_slack <= 90.0f * inv_kappa || gone));
    // or: the nearest sphere is no farther than sphere 0, k (rho_0 - r_0) = rho'_0 - k r_0 <= 90
    // bounds k d_min just as well (the first steps after the eye, where the 2 D bound is loose)
    if (!none && force == 0 && shift_none_ok && a.mfma)
      none = __all(fixed_shift(p, kappa * kappa, Lds::v4(L.S0[0]), Lds::v4(L.S1[0])) - kr_first <= 90.0f || gone);
    float m = none ? 0.0f : -INFINITY, s = 0.0f;
    const bool fixed = force == 1 || (force == 0 && !none && shift_fixed_ok && __all(psq(p) <= 1e10f || gone));
    choice = (none ? 1 : 0) | (fixed ? 2 : 0) | (fast ? 4 : 0);
    if ((none || fixed) && a.mfma) {
      const float k2 = kappa * kappa;
      // opaque per step: the row-block count's derived guards are formed here, not hoisted out
      // of the march loop as long-lived lane masks (SGPR pressure: spills to v_writelane)
      int nrb = a.Mpad / 16;
      asm volatile("" : "+s"(nrb));
      uint4* xa = reinterpret_cast<uint4*>(L.slots) + wave * 64;
      uint4* xb = reinterpret_cast<uint4*>(L.slots) + kWaves * 64 + wave * 64;
      float* xs = L.slots + kWaves * 64 * 8 + wave * 64;
#ifdef RM_BLOCK_TRACE
      const unsigned long long tq0 = __builtin_readcyclecounter();
      tr_paths += 1ull << (16 * ((fixed ? 2 : 0) + (fast ? 0 : 1)));
#endif
      float Dm;
      const uint4* At = L.At;
      const float* Wt = L.Wt;
      int nq = nrb;
      float* comb = nullptr;
      if constexpr (SPLIT) {  // this wave's quarter of the row blocks; combine buffers alternate
        const int r0 = part_rb(nrb, wave);
        nq = part_rb(nrb, wave + 1) - r0;
        At += (size_t)r0 * 64;
        Wt += (size_t)r0 * 32;
        comb = L.slots + kSplitCombOff + (split_par ^= 1) * (kWaves * 64);
      }
      constexpr int kNcb = SPLIT ? kSplitCB : 4;  // column blocks of this wave's rays
      if (!SPLIT && a.early_exit) {
        // Packed step (exact). A step's D is a function of the ray's t and the step's shift form
        // (choice & 3; the clamp bit changes no bit), so a ray whose t equals its t one or two steps
        // back, under the form of that step, has the D of that step: it is known, not summed again
        // (hit rays settle into a period-1 or period-2 cycle long before their wave does). The
        // choice above came from every ray's own votes as before. Only the live rays -- not gone
        // (their D is unused), not known -- are summed, packed into ceil(live / 16) column blocks.
        // Lanes past n_rays are copies of ray 0 that vote like rays: they stay in. Exit off: the
        // unpacked step below (every ray does every step's work), so exit on == off tests the bits
        // of the memo and of the packing. Render mode keeps no history: no ray is ever known there.
        const int form = choice & 3;
        const bool memo = MODE != kRender;
        const bool known2 = memo && mm.t == mm.t2 && form == ((mm.chist >> 3) & 3);
        const bool known1 = memo && mm.t == mm.t1 && form == (mm.chist & 3);
        const bool live = !gone && !known1 && !known2;
        const unsigned long long bm = __ballot(live);
        skipped_cb += 4 - ((__popcll(bm) + 15) >> 4);
        if (fixed) {
          const float4 A = Lds::v4(L.S0[0]), B = Lds::v4(L.S1[0]);
          Dm = fast ? march_d_fixed<false, 4, true>(p, kappa, inv_kappa, kr_first, A, B, At, Wt, nq, xa, xb, xs, lane,
                                                    nullptr, 0, bm, live)
                    : march_d_fixed<true, 4, true>(p, kappa, inv_kappa, kr_first, A, B, At, Wt, nq, xa, xb, xs, lane,
                                                   nullptr, 0, bm, live);
        } else {
          Dm = fast ? march_d_none<false, 4, true>(p, kappa, inv_kappa, At, Wt, nq, xa, xb, xs, lane, nullptr, 0, bm, live)
                    : march_d_none<true, 4, true>(p, kappa, inv_kappa, At, Wt, nq, xa, xb, xs, lane, nullptr, 0, bm, live);
        }
        Dm = known2 ? mm.D2 : (known1 ? Dprev : Dm);
      } else if (fixed) {  // the ray's shift: rho'_0 of sphere 0 (any value near it keeps +-100 headroom)
        const float4 A = Lds::v4(L.S0[0]), B = Lds::v4(L.S1[0]);
        Dm = fast ? march_d_fixed<false, kNcb>(p, kappa, inv_kappa, kr_first, A, B, At, Wt, nq, xa, xb, xs, lane, comb, wave)
                  : march_d_fixed<true, kNcb>(p, kappa, inv_kappa, kr_first, A, B, At, Wt, nq, xa, xb, xs, lane, comb, wave);
      } else {
        Dm = fast ? march_d_none<false, kNcb>(p, kappa, inv_kappa, At, Wt, nq, xa, xb, xs, lane, comb, wave)
                  : march_d_none<true, kNcb>(p, kappa, inv_kappa, At, Wt, nq, xa, xb, xs, lane, comb, wave);
      }
      (void)k2;
#ifdef RM_BLOCK_TRACE
      tr_lse_cyc += __builtin_readcyclecounter() - tq0;
#endif
      return Dm;
    }
#ifdef RM_BLOCK_TRACE
    ++tr_vec;
#endif
    if (none || fixed) {
      const float k2 = kappa * kappa;
      const int np = a.Mpad / 2;
      float sh;
      if (none) {
        s = fast ? lse_weighted<false, false>(p, L, np, k2, sh) : lse_weighted<true, false>(p, L, np, k2, sh);
      } else {
        s = fast ? lse_weighted<false, true>(p, L, np, k2, sh) : lse_weighted<true, true>(p, L, np, k2, sh);
        m = kr_first - sh;
      }
      return -(flog2(fmaxf(s, 1e-30f)) + m) * inv_kappa;
    }
    if (none) {
      if (fast) for_tiles([&](int, int tn) { lse_point<false, kShiftNone>(p, L, tn / 2, nkappa, m, s); });
      else for_tiles([&](int, int tn) { lse_point<true, kShiftNone>(p, L, tn / 2, nkappa, m, s); });
    } else if (fixed) {
      // |p| <= 1e5: the expansion-form rounding of rho (~1.5 ulp(|p|)) moves the exponents by
      // < 0.5; far out it can exceed the +-100 headroom, so distant points keep the running max
      if (fast) for_tiles([&](int, int tn) { lse_point<false, kShiftFixed>(p, L, tn / 2, nkappa, m, s); });
      else for_tiles([&](int, int tn) { lse_point<true, kShiftFixed>(p, L, tn / 2, nkappa, m, s); });
    } else {
      if (fast) for_tiles([&](int, int tn) { lse_point<false, kShiftMax>(p, L, tn / 2, nkappa, m, s); });
      else for_tiles([&](int, int tn) { lse_point<true, kShiftMax>(p, L, tn / 2, nkappa, m, s); });
    }
    return -(flog2(fmaxf(s, 1e-30f)) + m) * inv_kappa;
  };
  // The march's soft-min. Ray mode (the split kernels): each ray's own choice, so that its step is
  // a function of its own state (its p and previous D) -- unshifted when the ray's own bound admits
  // it (the tests of soft_min_core, per ray), else the scene-uniform fixed shift when its |p| admits
  // it (|p| <= 1e5, the fixed form's fp32 headroom), else the running maximum (a vector sweep over
  // all spheres, lane by lane); a wave runs each form only when one of its live rays takes it
  // (two forms in the waves whose rays disagree).
  auto soft_min_march = [&](const float p[3], bool fast, float Dprev, int& choice, const Memo& mm) {
    if constexpr (SPLIT) {
      const bool live = !gone && !retired;
      bool nr = live && shift_none_ok && 2.0f * fmaxf(Dprev, 0.0f) + a.lse_slack <= 90.0f * inv_kappa;
      if (live && !nr && shift_none_ok && a.mfma)
        nr = fixed_shift(p, kappa * kappa, Lds::v4(L.S0[0]), Lds::v4(L.S1[0])) - kr_first <= 90.0f;
      const bool far = live && !nr && !(psq(p) <= 1e10f);
      const bool use_fixed = !nr && shift_fixed_ok && !far;
      unsigned long long bn = __ballot(nr);
      const unsigned long long bf = __ballot(live && use_fixed), bx = __ballot(live && !nr && !use_fixed);
      // exit off (the capability measurement: every ray does every step's work): a wave whose
      // rays are all gone still runs a sweep, as the wave-uniform march does (results unused)
      if (!a.early_exit && (bn | bf | bx) == 0ull) bn = 1ull;
      int cm = 0;
      float Dn = 0.0f, Dm = 0.0f, Dx = 0.0f;
      if (bn != 0ull) Dn = soft_min_core(p, fast, Dprev, cm, 3, mm);
      if (bf != 0ull) Dm = soft_min_core(p, fast, Dprev, cm, 1, mm);
      if (bx != 0ull) Dx = soft_min_core(p, fast, Dprev, cm, 2, mm);
      choice = (nr ? 1 : 0) | (use_fixed ? 2 : 0) | (fast ? 4 : 0);
      return nr ? Dn : (use_fixed ? Dm : Dx);
    } else {
      return soft_min_core(p, fast, Dprev, choice, 0, mm);
    }
  };

  // ---- march: t <- (t + sdf(o + d t)).detach(), S times (renderer_diff.rs:20-26)
  // The fast path needs a distance lower bound: the previous point's hard minimum (>= its
  // soft-min D) minus the step just taken (every dist_j is 1-Lipschitz and |d| = 1).
  float t = 0.0f;
  float lb = -INFINITY;  // lower bound on the scene distance at the current point
  float Dprev = INFINITY;  // previous march step (none yet)
  bool dead = false;       // wave-uniform: every ray of the wave has escaped (see below)
  int steps_saved = 0;     // wave-uniform: march steps this wave did not run (work statistics)
  // the scene's bounding sphere (c, R) (scene_bound, in the record header); R' = R + soft-min
  // slack + 1e-3 (fp32 margin of the march)
  const float c0x = hdr[4], c0y = hdr[5], c0z = hdr[6];
  const cf1_ptr esc_tab = (cf1_ptr)(reinterpret_cast<const char*>(a.rec_buf) + esc_offset(a.Mpad / 2, (a.Mpad / 2 + 255) / 256));
  if (MODE == kBwd && a.t_in != nullptr) {
    t = a.t_in[ri];
  } else {
    // Escaped rays: receding from the scene's bounding sphere (c_0, R) with every later
    // soft-min >= |p - c_0| - R - ln(M)/k >= gone_d (the distance only grows along a
    // receding ray, so t keeps increasing); the reconnected point and the mask argument
    // are then >= gone_d too, where sigmoid(-msharp D) (or exp(-10 D^2)) is exactly 0 in
    // fp32: out = 0 and every gradient term is 0, whatever the remaining steps would give.
    // Margins: 1e-5 relative + 1e-3 cover the fp32 rounding of the march at any |p|.
    // Each remaining step is >= dist - R' long and keeps the ray receding, so the distance
    // grows step by step (write_bound): with n steps left the ray is gone once
    // (1 - 1e-5) dist >= T(n) -- proven long before the ray gets there.
    // A gone ray (sticky) steps by that bound, dist - R', instead of its soft-min: the proof
    // holds for any steps >= the bound, so its outputs stay exactly 0, and it leaves the
    // wave's shift / clamp choices (far points would force the running-max vector sweep on
    // the whole wave: 48 % of the march steps at 4096 spheres / 128 steps). A wave whose
    // rays are all gone stops (a.early_exit). The same in every mode that builds the table,
    // exit on or off, so both give the same bits.
    const float rprime = (hdr[7] + a.lse_slack + 1e-3f) * (1.0f + 1e-6f);  // R' as in write_bound
    float gone_step = 0.0f;  // dist - R' of a gone ray at the current point
    auto wave_escaped = [&](int st, const float p[3]) {
      if (!(a.gone_d > 0.0f)) return false;
      const float ex = p[0] - c0x, ey = p[1] - c0y, ez = p[2] - c0z;
      const float Tn = esc_tab[min(a.steps - st, kEscTab - 1)];
      const float dist = fsqrt(fmaf(ez, ez, fmaf(ey, ey, ex * ex)));
      gone = gone || (!retired && fmaf(ez, d[2], fmaf(ey, d[1], ex * d[0])) >= 0.0f && dist * (1.0f - 1e-5f) >= Tn);
      gone_step = dist - rprime;
      if (a.early_exit && __all(gone || !valid)) {
        steps_saved += a.steps - st;
        return true;
      }
      return false;
    };
    // A gone ray's remaining bound steps from step `from` to the end (what the march would do):
    // where the march of its wave stops early but its rays' final states are used later (ray mode:
    // the continuation caps and the listed rays' write-back) -- a gone ray's mask is exactly 0
    // only where the bound steps end, not where it was proven
    auto gone_finish = [&](int from) {
      if (gone && !retired)
        for (int k = from; k < a.steps; ++k) {
          const float q[3] = {fmaf(d[0], t, o[0]) - c0x, fmaf(d[1], t, o[1]) - c0y, fmaf(d[2], t, o[2]) - c0z};
          t = fminf(t + (fsqrt(fmaf(q[2], q[2], fmaf(q[1], q[1], q[0] * q[0]))) - rprime), kTMax);
        }
    };
    int st_stop = -1;  // the step at which the march found every ray of the wave gone (not taken)
    int st0 = 0;
#ifdef RM_BLOCK_TRACE
    const unsigned long long tr_c_begin = __builtin_readcyclecounter();
    unsigned long long tr_cyc = 0;  // period | step << 8 of the cycle exit
#endif
    if constexpr (CAM) {
      // Camera mode: step 0 from the soft-min at the eye, evaluated once per view by the same
      // code path (write_origins), when every lane of the wave has it (not NaN). Taken before
      // the loop so that D0 holds no register through the march.
      if (a.origin != nullptr && a.steps > 0 && !(SPLIT && a.cont_resume > 0)) {
        const float D0 = a.origin[view];
        rho_lb = a.origin[RM_MAX_VIEWS_PER_CALL + view];  // at the eye
        if (__all((__float_as_uint(D0) & 0x7fffffffu) <= 0x7f800000u)) {
          const float p[3] = {fmaf(d[0], t, o[0]), fmaf(d[1], t, o[1]), fmaf(d[2], t, o[2])};
          if (wave_escaped(0, p)) {
            dead = true;
          } else {  // == soft_min_march(p, all_safe(-inf) = false, inf) at p = o = the eye
            t = fminf(t + (gone ? gone_step : D0), kTMax);
            rho_lb = rho_moved(rho_lb, 0.0f, t);
            lb = D0 - fabsf(D0);
            Dprev = D0;
            st0 = 1;
            steps_saved = 1;  // a step this wave did not run
          }
        }
      }
    }
    // the cycle exit's history: t one and two steps back, and the choices (3 bits per step,
    // the latest in the low bits; 7 is no valid choice)
    float cyc_t1 = __builtin_nanf(""), cyc_t2 = __builtin_nanf("");
    int chist = 0xFFF;
    float Dprev2 = INFINITY;  // the D two steps back (the packed step's memo)
    int rhist = 0xFFF;  // ray mode: the ray's own choice history (per lane: listed rays come from many groups)
    if (SPLIT && a.cont_resume > 0) {  // the state the first launch saved at step cont_resume
      const float* cs = a.cont_state;
      const long long R = a.cont_rays;
      const long long G = 8 * R;  // the per-group words after the per-ray rows
      t = cs[li];
      lb = cs[R + li];
      Dprev = cs[2 * R + li];
      cyc_t1 = cs[3 * R + li];
      cyc_t2 = cs[4 * R + li];
      const float gflag = cs[5 * R + li];  // 1 gone, 2 retired
      gone = gflag == 1.0f;
      retired = gflag == 2.0f;
      rho_lb = cs[6 * R + li];
      rhist = __float_as_int(cs[7 * R + li]);
      if (!a.ray_cont) {
        chist = __float_as_int(cs[G + 2 * blk]);
        steps_saved = __float_as_int(cs[G + 2 * blk + 1]);
      }
      st0 = a.cont_resume;
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int st = st0; !dead && st < a.steps; ++st) {
      if (SPLIT && a.cont_cap > 0 && st == a.cont_cap) {
        // ray mode, defer at the top of this step: every ray's state, the marching rays to the
        // ray list; a group (not a ray_cont block) also to the resume list, its not-run steps
        // counted as saved now (the ray_cont blocks subtract the steps they run)
        float* cs = a.cont_state;
        const long long R = a.cont_rays;
        const bool act = valid && !gone && !retired && lane < kSplitRays;
        gone_finish(st);
        if (wave == 0 && lane < kSplitRays && valid) {
          cs[li] = t;
          cs[R + li] = lb;
          cs[2 * R + li] = Dprev;
          cs[3 * R + li] = cyc_t1;
          cs[4 * R + li] = cyc_t2;
          cs[5 * R + li] = gone ? 1.0f : (retired ? 2.0f : 0.0f);
          cs[6 * R + li] = rho_lb;
          cs[7 * R + li] = __int_as_float(rhist);
        }
        if (wave == 0) {
          const unsigned long long am = __ballot(act);
          const int na = __popcll(am);
          int base = 0;
          if (lane == 0 && na > 0) base = atomicAdd(a.ray_count_w, na);
          base = __shfl(base, 0);
          if (act) a.ray_list_w[base + __popcll(am & below)] = (int)li;
          if (lane == 0) {
            if (!a.ray_cont) {
              cs[8 * R + 2 * blk] = __int_as_float(chist);
              cs[8 * R + 2 * blk + 1] = __int_as_float(steps_saved + (a.steps - st));
              a.cont_list_w[atomicAdd(a.cont_count_w, 1)] = (int)blk;
            } else if (a.stats != nullptr && st > st0) {
              atomicAdd(a.stats + 2, (unsigned long long)(-(long long)(st - st0)));
            }
          }
        }
        return;
      }
      const float p[3] = {fmaf(d[0], t, o[0]), fmaf(d[1], t, o[1]), fmaf(d[2], t, o[2])};
      if (wave_escaped(st, p)) {
        dead = true;
        st_stop = st;
        break;
      }
      int choice;
      const Memo mm{t, cyc_t1, cyc_t2, Dprev2, chist};
      const float D = soft_min_march(p, all_safe(lb, rho_lb), Dprev, choice, mm);
      const float t_step = t;  // this step's state: (t_step, choice)
      if constexpr (SPLIT) {
        // Ray mode: a ray's step is a function of its own t (the shift is scene-uniform; the clamp
        // choice changes no bit), so a ray whose t repeats with period 2 (t_step == t two steps
        // back, under the same shift choice) keeps repeating: it retires with the state the march
        // would end in -- this step's when an even number of steps is left, the next one's
        // otherwise -- and keeps it (its lanes still run, their results unused). Gone rays
        // (sticky) and retired rays leave the wave-uniform choices.
        const float rl0 = rho_lb;
        if (!retired) {
          t = fminf(t + (gone ? gone_step : D), kTMax);
          rho_lb = rho_moved(rl0, t_step, t);
          lb = D - fabsf(D);
          Dprev = D;
        }
        if (a.early_exit && MODE != kRender) {
          if (!retired && !gone && valid && t_step == cyc_t2 && (choice & 3) == ((rhist >> 3) & 3)) {
            retired = true;
            if (((a.steps - st) & 1) == 0) {  // the state after the last step is this step's
              t = t_step;
              rho_lb = rl0;
            }
          }
          if (!retired) {
            cyc_t2 = cyc_t1;
            cyc_t1 = t_step;
          }
          rhist = ((rhist << 3) | choice) & 0xFFF;
          if (__all(gone || !valid || retired)) {  // every ray final or gone: gone rays take their bound steps
            if (gone) {
              for (int k = st + 1; k < a.steps; ++k) {
                const float q[3] = {fmaf(d[0], t, o[0]) - c0x, fmaf(d[1], t, o[1]) - c0y, fmaf(d[2], t, o[2]) - c0z};
                t = fminf(t + (fsqrt(fmaf(q[2], q[2], fmaf(q[1], q[1], q[0] * q[0]))) - rprime), kTMax);
              }
            }
            steps_saved += a.steps - 1 - st;
            break;
          }
        }
        continue;
      }
      t = fminf(t + (gone ? gone_step : D), kTMax);
      rho_lb = rho_moved(rho_lb, t_step, t);
      // next point: hard min >= soft-min D here, moved by |D|
      lb = D - fabsf(D);
      Dprev2 = Dprev;
      Dprev = D;
      // Cycle exit (exact). A march step is a deterministic function of the wave's state: the t
      // of every ray that is not gone and the step's wave-uniform choice (which carries all the
      // previous step's D decides). When this step's state equals the state P = 2 steps back
      // the march repeats with period P from there, so the state after the last step is the
      // one (steps left) mod P steps after that earlier state. A ray cycling
      // between fixed points cannot become gone later (its thresholds only grow); gone rays take
      // their remaining bound steps here, as the march would. Of the last step's D the post-march
      // needs only the clamp-free choice of the reconnect: the final state's choice bit 2.
      if (a.early_exit && MODE != kRender) {
        if (choice == ((chist >> 3) & 7) && __all(gone || t_step == cyc_t2)) {
          constexpr int P = 2;
          // the state after the last step (step a.steps) is this step's state or the one `back`
          // steps before it; `left` steps remain after this one
          const int left = a.steps - 1 - st, m = a.steps - st, back = (P - m % P) % P;
          const int cf = back == 0 ? choice : (chist >> (3 * (back - 1))) & 7;
          if (!gone) {
            if (back == 0) t = t_step;
            else if (back == 1) t = cyc_t1;
            lb = (cf & 4) ? INFINITY : -INFINITY;  // all_safe(lb, rho_lb) of the final state = its bit 2
            rho_lb = -INFINITY;
          } else {
            for (int k = st + 1; k < a.steps; ++k) {
              const float q[3] = {fmaf(d[0], t, o[0]) - c0x, fmaf(d[1], t, o[1]) - c0y, fmaf(d[2], t, o[2]) - c0z};
              t = fminf(t + (fsqrt(fmaf(q[2], q[2], fmaf(q[1], q[1], q[0] * q[0]))) - rprime), kTMax);
            }
          }
          steps_saved += left;
#ifdef RM_BLOCK_TRACE
          tr_cyc = (unsigned long long)P | ((unsigned long long)st << 8);
#endif
          break;
        }
        cyc_t2 = cyc_t1;
        cyc_t1 = t_step;
        chist = ((chist << 3) | choice) & 0xFFF;
      }
    }
    // the column blocks the packed steps did not multiply, in whole steps of the wave (four
    // blocks), rounded down: the work counters keep counting executed lane work
    if constexpr (!SPLIT) steps_saved += skipped_cb >> 2;
    if (SPLIT && a.ray_cont) {
      // ray mode: the listed rays' final states back into their groups' rows (the resume launch
      // runs the groups' post-march forward and backward); the steps this block ran uncounted
      // from the saved steps its groups booked at the cap
      float* cs = a.cont_state;
      const long long R = a.cont_rays;
      if (st_stop >= 0) gone_finish(st_stop);
      if (wave == 0 && lane < kSplitRays && valid) {
        cs[li] = t;
        cs[R + li] = lb;
        cs[5 * R + li] = gone ? 1.0f : (retired ? 2.0f : 0.0f);
        cs[6 * R + li] = rho_lb;
      }
      const long long run = (long long)(a.steps - st0) - steps_saved;
      if (wave == 0 && lane == 0 && a.stats != nullptr && run > 0) atomicAdd(a.stats + 2, (unsigned long long)(-run));
      return;
    }
  RM_TRACE(4, __builtin_amdgcn_s_memrealtime());
  RM_TRACE(6, (unsigned long long)steps_saved);
#ifdef RM_BLOCK_TRACE
  RM_TRACE(7, tr_paths);
  RM_TRACE(8, tr_lse_cyc);
  RM_TRACE(9, tr_vec);
  RM_TRACE(10, __builtin_readcyclecounter() - tr_c_begin);
  RM_TRACE(11, tr_cyc);
#endif
  }
  if ((MODE == kFwd || MODE == kRender) && a.t_out != nullptr && valid && own_rays) a.t_out[ri] = t;
  // work statistics: per wave here in the forward modes; per block at the hand-off barrier in the
  // backward modes (one pair of atomics per block, not per wave)
  if constexpr (MODE == kFwd || MODE == kRender) {
    if (a.stats != nullptr && lane == 0 && own_rays) {
      if (dead) atomicAdd(a.stats + 1, 1ull);
      if (steps_saved != 0) atomicAdd(a.stats + 2, (unsigned long long)steps_saved);
    }
  }

  // Post-march forward state. A wave whose rays have all escaped (see the march loop) keeps
  // the defaults: out = mix L mu = 0 with mu = 0, and every backward seed is 0.
  const float c10l = a.csharp * kLog2e;
  float pa[3] = {fmaf(d[0], t, o[0]), fmaf(d[1], t, o[1]), fmaf(d[2], t, o[2])};
  float p[3] = {pa[0], pa[1], pa[2]};
  float mA = 0.0f, sA = 1.0f, Da = 0.0f, tf = t;
  bool fast_a = false, fast_f = false;
  float nrm[3] = {0.0f, 0.0f, 0.0f}, D6[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float amb = 0.0f, sdot = 0.0f, dif = 0.0f, Lgt = 0.0f;
  float dmin = 0.0f, Zw = 1.0f, Zb = 1.0f, Df = 0.0f, mix[3] = {0.0f, 0.0f, 0.0f}, mu = 0.0f;
  if (!dead) {
    // ---- reconnect: t_final = t + sdf(p_approx) (renderer_diff.rs:30-39); renderer.rs has none
    fast_a = all_safe(lb, rho_lb);
    if constexpr (MODE != kRender) {
      if constexpr (SPLIT) Da = soft_min_split(pa, fast_a, mA, sA);
      else Da = soft_min(pa, fast_a, mA, sA);
    }
    tf = t + Da;
    p[0] = fmaf(d[0], tf, o[0]);
    p[1] = fmaf(d[1], tf, o[1]);
    p[2] = fmaf(d[2], tf, o[2]);
    // p_final is |Da| from p_approx; the taps another eps away
    fast_f = MODE == kRender ? all_safe(lb - a.eps, rho_lb - a.eps)
                             : all_safe(-mA * inv_kappa - fabsf(Da) - a.eps, rho_moved(rho_lb, t, tf) - a.eps);

    // ---- detached normal (scene.rs:81-128): n = f / sqrt(|f|^2 + 1e-6) with f the central
    // differences (D(p + eps e_a) - D(p - eps e_a))_a; the 1e-6 keeps |n| ~ 0.2 at eps = 1e-4.
    // ---- colour softmax + mask (renderer_diff.rs:64-90)
    dmin = INFINITY;
    f2 Zw2 = sp(0.0f), Zb2 = sp(0.0f), C2[3] = {sp(0.0f), sp(0.0f), sp(0.0f)};
    if constexpr (MODE != kRender) {
      // one sweep for both: f = 2 eps grad D (its eps -> 0 limit) with grad D = G / Zb
      f2 G2[3] = {sp(0.0f), sp(0.0f), sp(0.0f)};
      if constexpr (SPLIT) {  // this wave's quarter of the pairs, then the four partial states merged
        const int b0 = split_pair(wave), b1 = split_pair(wave + 1);
        const Lds Lq = L.from_pair(b0);
        if (fast_f) shade_normal_sweep<false>(p, Lq, b1 - b0, c10l, kappa, dmin, Zw2, C2, Zb2, G2);
        else shade_normal_sweep<true>(p, Lq, b1 - b0, c10l, kappa, dmin, Zw2, C2, Zb2, G2);
        shade_merge(c10l, dmin, Zw2, C2, Zb2, G2);
      } else {
        if (fast_f) shade_normal_sweep<false>(p, L, a.Mpad / 2, c10l, kappa, dmin, Zw2, C2, Zb2, G2);
        else shade_normal_sweep<true>(p, L, a.Mpad / 2, c10l, kappa, dmin, Zw2, C2, Zb2, G2);
      }
      const float te = 2.0f * a.eps * frcp(Zb2.x + Zb2.y);
      const float nx = te * (G2[0].x + G2[0].y), ny = te * (G2[1].x + G2[1].y), nz = te * (G2[2].x + G2[2].y);
      const float inv_len = frsq(fmaf(nz, nz, fmaf(ny, ny, fmaf(nx, nx, 1e-6f))));
      nrm[0] = nx * inv_len;
      nrm[1] = ny * inv_len;
      nrm[2] = nz * inv_len;
    } else {  // renderer.rs: the six taps themselves, then the shade sums
      float m6[6], s6[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        m6[q] = -INFINITY;
        s6[q] = 0.0f;
      }
      const float eps = a.eps;
      // weighted (unshifted) taps when the hard maximum at every tap is provably >= -90:
      // d_min(tap) <= d_min(p_a) + |Da| + eps <= 2 max(Da, 0) + ln(M)/k + eps (as in the march)
      const bool none = shift_none_ok && __all(2.0f * fmaxf(Da, 0.0f) + a.lse_slack + eps <= 90.0f * inv_kappa);
      if (none) {
        if (fast_f) lse_taps_w<false>(p, L, a.Mpad / 2, kappa, eps, s6);
        else lse_taps_w<true>(p, L, a.Mpad / 2, kappa, eps, s6);
#pragma unroll
        for (int q = 0; q < 6; ++q) m6[q] = 0.0f;
      } else if (fast_f) {
        for_tiles([&](int, int tn) { lse_taps<false>(p, L, tn / 2, nkappa, 2.0f * eps, eps * eps, m6, s6); });
      } else {
        for_tiles([&](int, int tn) { lse_taps<true>(p, L, tn / 2, nkappa, 2.0f * eps, eps * eps, m6, s6); });
      }
#pragma unroll
      for (int q = 0; q < 6; ++q) D6[q] = -(flog2(fmaxf(s6[q], 1e-30f)) + m6[q]) * inv_kappa;
      const float nx = D6[0] - D6[1], ny = D6[2] - D6[3], nz = D6[4] - D6[5];
      const float inv_len = frsq(fmaf(nz, nz, fmaf(ny, ny, fmaf(nx, nx, 1e-6f))));
      nrm[0] = nx * inv_len;
      nrm[1] = ny * inv_len;
      nrm[2] = nz * inv_len;
      if (fast_f)
        for_tiles([&](int, int tn) { shade_sweep<false>(p, L, tn / 2, c10l, kappa, dmin, Zw2, C2, Zb2); });
      else
        for_tiles([&](int, int tn) { shade_sweep<true>(p, L, tn / 2, c10l, kappa, dmin, Zw2, C2, Zb2); });
    }

    // ---- lighting (renderer_diff.rs:48-62; renderer.rs:27-40 in kRender)
    float ldn[3];
    if constexpr (MODE == kRender) {
      ldn[0] = a.light_fixed[0];
      ldn[1] = a.light_fixed[1];
      ldn[2] = a.light_fixed[2];
    } else {
      amb = a.ambient[0];
      light_unit(a.light_dir, ldn);
    }
    sdot = fmaf(nrm[2], ldn[2], fmaf(nrm[1], ldn[1], nrm[0] * ldn[0]));
    dif = fmaxf(sdot, 0.0f);
    Lgt = MODE == kRender ? dif + 0.1f : fmaf(dif, 1.0f - amb, amb);

    Zw = Zw2.x + Zw2.y;
    Zb = Zb2.x + Zb2.y;
    Df = dmin - flog2(fmaxf(Zb, 1e-8f)) * inv_kappa;
    if constexpr (MODE == kRender) {
      // renderer.rs:52-71: raw exp(-10 d) weights, mixed = sum(col w) / (sum(w) + 1e-5); the sums
      // above are shifted by exp(10 dmin), undone here; mask = exp(-10 D^2) (renderer.rs:77)
      const float e = fexp2(-c10l * dmin);
      const float den = Zw * e + 1e-5f;
      mix[0] = (C2[0].x + C2[0].y) * e / den;
      mix[1] = (C2[1].x + C2[1].y) * e / den;
      mix[2] = (C2[2].x + C2[2].y) * e / den;
      mu = fexp2(-10.0f * kLog2e * Df * Df);
    } else {
      const float invZw0 = frcp(Zw);
      mix[0] = (C2[0].x + C2[0].y) * invZw0;
      mix[1] = (C2[1].x + C2[1].y) * invZw0;
      mix[2] = (C2[2].x + C2[2].y) * invZw0;
      mu = frcp(1.0f + fexp2(a.msharp * kLog2e * Df));  // sigmoid(-msharp * D)
    }
  }
  const float invZw = frcp(Zw);
  const float scale = Lgt * mu;
  const float outv[3] = {mix[0] * scale, mix[1] * scale, mix[2] * scale};

  if (MODE == kFwd && a.dbg != nullptr && valid && own_rays) {
    float* q = a.dbg + 24 * ri;
    const float vals[24] = {t, tf, nrm[0], nrm[1], nrm[2], Lgt, mix[0], mix[1], mix[2], Df, mu, sdot, dmin,
                            Zw, Zb, 0.0f, D6[0], D6[1], D6[2], D6[3], D6[4], D6[5], 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < 24; ++c) q[c] = vals[c];
  }
  const bool write_out = MODE != kBwd && a.out != nullptr && valid && own_rays;
  if (write_out) {
    a.out[3 * ri] = outv[0];
    a.out[3 * ri + 1] = outv[1];
    a.out[3 * ri + 2] = outv[2];
  }
  RM_TRACE(5, __builtin_amdgcn_s_memrealtime());
  if constexpr (MODE == kFwd || MODE == kRender) return;

  // ---- seed g = dL/dout
  float g[3] = {0.0f, 0.0f, 0.0f};
  float loss = 0.0f;
  if (valid && seed_lane) {
    if constexpr (MODE == kBwd) {
      g[0] = a.gout[3 * ri];
      g[1] = a.gout[3 * ri + 1];
      g[2] = a.gout[3 * ri + 2];
    } else {  // training.rs:17-34
      const float t0 = a.targets[3 * ri], t1 = a.targets[3 * ri + 1], t2 = a.targets[3 * ri + 2];
      const float W = (t0 + t1 + t2) > 0.01f ? 10.0f : fmaf(progress_of(a), 4.0f, 1.0f);
      const float tg[3] = {t0, t1, t2};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float df = outv[c] - tg[c];
        loss = fmaf(fabsf(df), W, loss);
        const float sg = df > 0.0f ? 1.0f : (df < 0.0f ? -1.0f : 0.0f);
        g[c] = W * sg * a.inv_count;
      }
    }
  }

  // ---- backward seeds (out = mix * L * mu)
  const float gdotm = fmaf(g[2], mix[2], fmaf(g[1], mix[1], g[0] * mix[0]));
  const float gm[3] = {g[0] * scale, g[1] * scale, g[2] * scale};
  const float gL = gdotm * mu, gmu = gdotm * Lgt;
  const float gamb = gL * (1.0f - dif);
  const float gs = sdot >= 0.0f ? gL * (1.0f - amb) : 0.0f;  // clamp_min passes at x >= min
  const float gell[3] = {gs * nrm[0], gs * nrm[1], gs * nrm[2]};
  const float cmu = gmu * mu * (1.0f - mu) * (-a.msharp);
  const float mg = fmaf(mix[2], gm[2], fmaf(mix[1], gm[1], mix[0] * gm[0]));
  const float b_scale = cmu * frcp(Zb);

  float* rec = a.partials + blk * a.rec;

  // ---- per-ray scalars (light before the projection, ambient, loss) and the early-exit
  // hand-off: every wave publishes its scalar sums and whether it left the march early; after
  // this barrier such waves end (an ended wave no longer counts in s_barrier) and the others
  // run the backward sweeps and combine only their own partials. The escaped waves' terms are
  // exactly 0, so the record is the one the full computation would write.
  static_assert(2 * kWaves <= 8, "misc layout: flags before the scalars");
  int* wflag = reinterpret_cast<int*>(L.misc);  // [kWaves] dead flags, [kWaves] steps saved
  float* wscal = L.misc + 8;                     // [kWaves][8]
  {
    const float vals[8] = {gell[0], gell[1], gell[2], gamb, loss, 0.0f, 0.0f, 0.0f};
    const float red = wave_reduce8(vals, lane);
    if ((lane & 7) == 7) wscal[wave * 8 + (lane >> 3)] = red;
    if (lane == 0) {
      wflag[wave] = dead ? 1 : 0;
      wflag[kWaves + wave] = steps_saved;
    }
  }
  // the block's hand-off work, by one wave once every wave has published: the cost in march-step
  // units (steps its waves ran, + kPostCost per wave that runs the post-march forward and the
  // backward: the next call's cost-ordered dispatch) and the work statistics
  auto handoff_work = [&]() {
    if (a.ocnt_w != nullptr) {
      int cost = 0;
#pragma unroll
      for (int w = 0; w < (SPLIT ? 1 : kWaves); ++w) cost += a.steps - wflag[kWaves + w] + (wflag[w] ? 0 : kPostCost);
      order_append(a, blk, cost);
    }
    if (a.stats != nullptr) {
      int ex = 0, sv = 0;
#pragma unroll
      for (int w = 0; w < (SPLIT ? 1 : kWaves); ++w) {
        ex += wflag[w];
        sv += wflag[kWaves + w];
      }
      if (ex != 0) atomicAdd(a.stats + 1, (unsigned long long)ex);
      if (sv != 0) atomicAdd(a.stats + 2, (unsigned long long)sv);
    }
  };
  // the whole block escaped: scalar totals, live flag 0 (the reduction skips the per-sphere
  // columns, all zero)
  auto escaped_record = [&]() {
    if (lane < 8) {
      float acc = wscal[lane];
#pragma unroll
      for (int w = 1; w < (SPLIT ? kSplitWaves : kWaves); ++w) acc += wscal[w * 8 + lane];
      rec[(long long)a.Mpad * 8 + lane] = acc;
    }
  };
  __syncthreads();
  int alive = 0;
#pragma unroll
  for (int w = 0; w < (SPLIT ? kSplitWaves : kWaves); ++w) alive |= wflag[w] ? 0 : (1 << w);
  alive = __builtin_amdgcn_readfirstlane(alive);  // block-uniform: scalar for the compiler
  // the hand-off work: the block's first live wave (wave 0 when every wave escaped)
  if (lane == 0 && wave == (alive != 0 ? __builtin_ctz(alive) : 0)) handoff_work();
  if (dead) {
    if (alive == 0 && wave == 0) escaped_record();
    return;
  }
  const int arank = __popc(alive & ((1 << wave) - 1));

  // ---- backward sweeps with one sphere per lane (transposed), the work shared out over the
  // block's live waves. Each live wave publishes its rays with non-zero seeds (a source) as a
  // compacted field-major LDS image. The work units are (64-sphere group, source wave) pairs in
  // group-major order; live wave r of n takes the units [r U / n, (r + 1) U / n) (U = groups x
  // sources). For each sphere of its lane a wave sums the terms of the rays of its units (sources
  // in wave order, their rays two per packed instruction) in registers, and writes the group's
  // record columns itself when it holds every source of the group; a group whose sources span
  // waves is added up from the waves' partials in LDS, in source order, by the wave that holds its
  // first unit. So each sphere group is loaded by one wave (two at a split), and there is no
  // combine of wave partials and no barrier per group. A split block's waves hold the same rays:
  // wave 0 is its one source (it seeds every lane) and the waves share the groups.
  // Only the position gradient g_p of sweep 1 is a per-ray sum over spheres, and only g_t = g_p . d
  // (the ray direction) is needed (t_final = t + D(p_a), p = o + d t_final): each computing wave
  // reduces its share across the lanes for batches of 8 rays (one transposing reduction) into an
  // LDS slot per (computing wave, source wave, ray), and the ray's owner adds the computing waves'
  // shares in wave order. Rays whose seeds are zero contribute exact zeros and are not listed
  // (sweep 1: gm = 0 and b_scale = 0; sweep 2: g_t = 0) -- in practice the escaped rays of live
  // waves; an odd count is padded with a copy of the last ray whose seeds are zero (exact zero
  // terms). Distances are formed with the same fp32 operations and operands as the forward sweeps
  // (qpair, delta_pair_rsq), so dd = dmin - delta <= 0 and v - mA <= 0 hold exactly.
  bool any_seed = true;  // block-uniform: some ray of the block has a non-zero seed
  {
    constexpr int kFields = kBwdFields;  // sweep 1: px py pz |p|^2 dmin 1/Zw b_scale mg gm.xyz d.xyz (14); sweep 2: 6
    constexpr int kWv = SPLIT ? kSplitWaves : kWaves;
    float* rayf_all = L.slots;                     // [wave][field][64 ray slots]; after a sweep: partials
    float* rayf = rayf_all + wave * 64 * kFields;  // this wave's rays
    float* gta = L.slots + kWaves * 64 * kFields;  // [computing wave][source wave][64] g_t shares
    int* nsrc = reinterpret_cast<int*>(L.misc) + 40;  // [kWaves] the sources' ray counts (sweep 1, then 2)
    const int np = a.Mpad / 2;
    const float4* R4 = reinterpret_cast<const float4*>(a.rec_buf);
    const float2* R2 = reinterpret_cast<const float2*>(R4 + 7 * (size_t)np);
    const int ngrp = (a.Mpad + 63) / 64;
    // The computing waves of a sweep: the block's source waves -- a set that does not depend on
    // which rayless waves left the march early, so the partition and every sum order are the same
    // with the early exit on and off -- or, in a split block, its waves (alive together).
    // the packed pair (slots s, s + 1) of field f of source wave sw's image
    auto pair = [&](int sw, int f, int s) {
      return *reinterpret_cast<const f2*>(rayf_all + (sw * kFields + f) * 64 + s);
    };
    const unsigned long long below = (1ull << lane) - 1ull;
    // this wave's units of a sweep with nsw sources: [u0, u1)
    auto unit_range = [&](int r, int nsw, int ncw, int& u0, int& u1) {
      const int U = ngrp * nsw;
      u0 = (r * U) / ncw;
      u1 = ((r + 1) * U) / ncw;
    };
    // the block's source waves (bits) from the published counts
    auto sources = [&]() {
      int m = 0;
#pragma unroll
      for (int sw = 0; sw < kWv; ++sw)
        if ((alive >> sw) & 1) m |= nsrc[sw] > 0 ? (1 << sw) : 0;
      return __builtin_amdgcn_readfirstlane(m);
    };
    // Partials of the groups a wave holds only in part: slot 0 its first group, slot 1 its last,
    // kept in registers through the sweep and written over the wave's own ray image after it
    // (ncomp floats x 64 per slot). The wave that holds a split group's first unit adds the
    // partials of the waves that hold its units, in order, and writes (ncomp 8) or adds to (4)
    // the record columns.
    // Does a wave boundary fall inside a group (a multiple of nsw units is a group boundary)?
    auto has_split = [&](int nsw, int ncw) {
      const int U = ngrp * nsw;
      for (int r = 1; r < ncw; ++r)
        if (((r * U) / ncw) % nsw != 0) return true;
      return false;
    };
    // (always inlined: as a call its array arguments went to scratch memory)
    auto finish_split = [&](int nsw, int ncw, int crank, bool in, int ncomp, const float (&p0)[8],
                            const float (&p1)[8]) __attribute__((always_inline)) {
      __syncthreads();  // every wave is done with the sweep's images
      // the partials indexed by live rank: slot 0 in rows [0, nst), slot 1 in [nst, 2 nst) (a
      // sweep-1 partial's column 7 is 0 and not stored: 14 rows fit a wave's 15-row image)
      const int nst = ncomp == 8 ? 7 : 4;
      float* mine = rayf_all + crank * 64 * kFields;  // by computing rank
      if (in) {
#pragma unroll
        for (int c = 0; c < 7; ++c)
          if (c < nst) {
            mine[c * 64 + lane] = p0[c];
            mine[(nst + c) * 64 + lane] = p1[c];
          }
      }
      __syncthreads();
      if (!in) return;
      int u0, u1;
      unit_range(crank, nsw, ncw, u0, u1);
      if (u1 <= u0) return;
      const int gl = (u1 - 1) / nsw;  // this wave's last group
      const int kb = max(u0, gl * nsw) - gl * nsw;
      if (kb != 0 || u1 - gl * nsw >= nsw) return;  // not the first unit of a split group
      // this wave holds units [0, u1 - gl nsw) of group gl: its last group, or its only one
      float acc[8];
      const int own_slot = (u0 / nsw == gl) ? 0 : 1;
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[c] = c < nst ? mine[(nst * own_slot + c) * 64 + lane] : 0.0f;
      for (int rr = crank + 1; rr < ncw; ++rr) {  // the next waves hold the group's next units
        int v0, v1;
        unit_range(rr, nsw, ncw, v0, v1);
        if (v0 >= (gl + 1) * nsw) break;
        if (v1 <= v0) continue;
        const float* part = rayf_all + rr * 64 * kFields;  // its first group: slot 0
#pragma unroll
        for (int c = 0; c < 7; ++c)
          if (c < nst) acc[c] += part[c * 64 + lane];
      }
      const int j = gl * 64 + lane;
      if (ncomp == 8) {
        store_group_cols(rec + (long long)gl * 64 * 8, acc, lane, min(64, a.Mpad - gl * 64));
      } else if (j < a.Mpad) {
        float4* dst = reinterpret_cast<float4*>(rec + (long long)j * 8);
        {
          float4 v = dst[0];
          v.x += acc[0];
          v.y += acc[1];
          v.z += acc[2];
          v.w += acc[3];
          dst[0] = v;
        }
      }
    };

    // ---- sweep 1 at p_final: colour softmax + mask soft-min + p_final(t_final)
    const unsigned long long act1 = __ballot(gm[0] != 0.0f || gm[1] != 0.0f || gm[2] != 0.0f || b_scale != 0.0f);
    const int n1 = __popcll(act1), rank1 = __popcll(act1 & below);
    const bool on1 = ((act1 >> lane) & 1ull) != 0ull;
    if (on1) {
      const float vals[14] = {p[0], p[1], p[2], psq(p), dmin, invZw, b_scale, mg, gm[0], gm[1], gm[2],
                              d[0], d[1], d[2]};
#pragma unroll
      for (int f = 0; f < 14; ++f) rayf[f * 64 + rank1] = vals[f];
      if ((n1 & 1) && rank1 == n1 - 1) {  // pad: this ray again, zero seeds
        const float pad[14] = {p[0], p[1], p[2], psq(p), dmin, invZw, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f,
                               d[0], d[1], d[2]};
#pragma unroll
        for (int f = 0; f < 14; ++f) rayf[f * 64 + n1] = pad[f];
      }
    }
    if (lane == 0) nsrc[wave] = n1;
    // work statistics: the rays the backward sweeps run for (a split block's rays are wave 0's)
    if (a.stats != nullptr && lane == 0 && n1 > 0 && (!SPLIT || wave == 0))
      atomicAdd(a.stats + 4, (unsigned long long)n1);
#pragma unroll
    for (int sw = 0; sw < kWv; ++sw) gta[(wave * kWaves + sw) * 64 + lane] = 0.0f;
    __syncthreads();  // every live wave's image and count
    const int srcs1 = sources();
    const int nsw1 = __popc(srcs1);
    const int cmask1 = SPLIT ? alive : srcs1, ncw1 = __popc(cmask1), crank1 = __popc(cmask1 & ((1 << wave) - 1));
    const bool in1 = ((cmask1 >> wave) & 1) != 0;
    bool split1 = false;
    {
      const f2 CL = sp(c10l), KA = sp(kappa), NCS = sp(-a.csharp);
      float p0[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, p1[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      auto sweep1 = [&](auto clamp_tag) {
        constexpr bool CLAMP = decltype(clamp_tag)::value;
        int u0 = 0, u1 = 0;
        if (in1) unit_range(crank1, nsw1, ncw1, u0, u1);
        for (int u = u0; u < u1;) {
          const int grp = u / nsw1, kb = u - grp * nsw1, ke = min(u1 - grp * nsw1, nsw1);
          u = grp * nsw1 + ke;
          const int j = grp * 64 + lane;
          float gx = -2.0f * kPadCenter, gy = 0.0f, gz = 0.0f, cc = kPadCenter * kPadCenter, rr = 0.0f, cr = 0.0f,
                cg = 0.0f, cbl = 0.0f;
          if (j < a.Mpad) {  // sphere j of pair j/2 (records of rm_prep_kernel)
            const int i = j >> 1;
            const bool h = (j & 1) != 0;
            const float4 A = R4[i], B = R4[np + i], R = R4[2 * np + i], C3 = R4[3 * np + i];
            const float2 C4 = R2[i];
            gx = h ? A.y : A.x;
            gy = h ? A.w : A.z;
            gz = h ? B.y : B.x;
            cc = h ? B.w : B.z;
            rr = h ? R.w : R.z;
            cr = h ? C3.y : C3.x;
            cg = h ? C3.w : C3.z;
            cbl = h ? C4.y : C4.x;
          }
          const f2 GX = sp(gx), GY = sp(gy), GZ = sp(gz), CC = sp(cc), RR = sp(rr), CR = sp(cr), CG = sp(cg),
                   CB = sp(cbl), HX = sp(0.5f * gx), HY = sp(0.5f * gy), HZ = sp(0.5f * gz);
          f2 agc[3] = {sp(0.0f), sp(0.0f), sp(0.0f)}, agr = sp(0.0f), acol[3] = {sp(0.0f), sp(0.0f), sp(0.0f)};
          for (int sw = 0, k = 0; sw < kWv; ++sw) {
            if (!((srcs1 >> sw) & 1)) continue;
            const int kk = k++;
            if (kk < kb || kk >= ke) continue;
            const int ns = nsrc[sw], nps = (ns + 1) >> 1;
            float* gacc = gta + (wave * kWaves + sw) * 64;
            for (int b = 0; b < nps; b += 4) {  // batches of 4 pairs = 8 slots
              float gtv[8];
#pragma unroll
              for (int uu = 0; uu < 4; ++uu) {
                if (b + uu >= nps) {  // batch slots past the last pair
                  gtv[2 * uu] = gtv[2 * uu + 1] = 0.0f;
                  continue;
                }
                const int s0 = 2 * (b + uu);
                const f2 PX = pair(sw, 0, s0), PY = pair(sw, 1, s0), PZ = pair(sw, 2, s0);
                const f2 PP = pair(sw, 3, s0);
                const f2 DM = pair(sw, 4, s0), IZ = pair(sw, 5, s0), BS = pair(sw, 6, s0), MG = pair(sw, 7, s0);
                const f2 G0 = pair(sw, 8, s0), G1 = pair(sw, 9, s0), G2 = pair(sw, 10, s0);
                const f2 DX = pair(sw, 11, s0), DY = pair(sw, 12, s0), DZ = pair(sw, 13, s0);
                f2 q = fma2(PZ, GZ, fma2(PY, GY, fma2(PX, GX, PP + CC)));  // == qpair: the shade sweep's q
                const f2 qraw = q;
                if constexpr (CLAMP) q = clamp_q(q);
                const f2 ir = rsq2(q);  // == delta_pair_rsq: the shade sweep's delta, and 1/rho
                const f2 dl = q * ir - RR;
                const f2 dd = DM - dl;  // <= 0 exactly
                const f2 w = exp2v(dd * CL) * IZ;
                const f2 bt = exp2v(dd * KA) * BS;
                const f2 cgm = fma2(CB, G2, fma2(CG, G1, CR * G0));
                const f2 gd = fma2(w * NCS, cgm - MG, bt);
                f2 gu = gd * ir;
                if constexpr (CLAMP) {  // clamp_min(1e-6) gate
                  gu.x = qraw.x >= 1e-6f ? gu.x : 0.0f;
                  gu.y = qraw.y >= 1e-6f ? gu.y : 0.0f;
                }
                const f2 ex = HX + PX, ey = HY + PY, ez = HZ + PZ;  // == fma2(HALF, -2c, p) = p - c
                const f2 ngu = -gu;
                agc[0] = fma2(ngu, ex, agc[0]);  // gc_j -= g_delta_j u_j
                agc[1] = fma2(ngu, ey, agc[1]);
                agc[2] = fma2(ngu, ez, agc[2]);
                const f2 gt2 = gu * fma2(ez, DZ, fma2(ey, DY, ex * DX));  // (g_delta_j u_j) . d
                gtv[2 * uu] = gt2.x;
                gtv[2 * uu + 1] = gt2.y;
                agr -= gd;
                acol[0] = fma2(w, G0, acol[0]);
                acol[1] = fma2(w, G1, acol[1]);
                acol[2] = fma2(w, G2, acol[2]);
              }
              const float r0 = wave_reduce8(gtv, lane);
              const int slot = 2 * b + (lane >> 3);
              if ((lane & 7) == 7 && slot < ns) gacc[slot] += r0;
            }
          }
          const float v[8] = {agc[0].x + agc[0].y, agc[1].x + agc[1].y, agc[2].x + agc[2].y, agr.x + agr.y,
                              acol[0].x + acol[0].y, acol[1].x + acol[1].y, acol[2].x + acol[2].y, 0.0f};
          if (kb == 0 && ke == nsw1) {  // every source: the group's columns, written by this wave alone
            store_group_cols(rec + (long long)grp * 64 * 8, v, lane, min(64, a.Mpad - grp * 64));
          } else if (grp == u0 / nsw1) {
#pragma unroll
            for (int c = 0; c < 8; ++c) p0[c] = v[c];
          } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) p1[c] = v[c];
          }
        }
      };
      if (nsw1 == 0) {  // no ray of the block has a seed: its columns are zeros, not written (live flag 0)
        any_seed = false;
      } else if (fast_f) {
        sweep1(std::false_type{});
      } else {
        sweep1(std::true_type{});
      }
      split1 = nsw1 > 0 && has_split(nsw1, ncw1);
      if (split1) finish_split(nsw1, ncw1, crank1, in1, 8, p0, p1);
      else __syncthreads();  // every computing wave's g_t shares
    }

    // ---- sweep 2 at p_approx: t_final = t + D(p_approx) -> g_t * softmax(-k dist_a)
    float gt = 0.0f;
    if (on1) {
      bool first = true;
#pragma unroll
      for (int w = 0; w < kWv; ++w)
        if ((cmask1 >> w) & 1) {
          const float v = gta[(w * kWaves + wave) * 64 + rank1];
          gt = first ? v : gt + v;
          first = false;
        }
    }
    const float hs = gt * frcp(sA);
    if (split1) __syncthreads();  // every split partial read (the images hold them)
    const unsigned long long act2 = __ballot(hs != 0.0f);
    const int n2 = __popcll(act2), rank2 = __popcll(act2 & below);
    if (((act2 >> lane) & 1ull) != 0ull) {
      const float vals[6] = {pa[0], pa[1], pa[2], psq(pa), mA, hs};
#pragma unroll
      for (int f = 0; f < 6; ++f) rayf[f * 64 + rank2] = vals[f];
      if ((n2 & 1) && rank2 == n2 - 1) {  // pad: this ray again, zero seed
        const float pad[6] = {pa[0], pa[1], pa[2], psq(pa), mA, 0.0f};
#pragma unroll
        for (int f = 0; f < 6; ++f) rayf[f * 64 + n2] = pad[f];
      }
    }
    if (lane == 0) nsrc[wave] = n2;
    if (a.stats != nullptr && lane == 0 && n2 > 0 && (!SPLIT || wave == 0))
      atomicAdd(a.stats + 5, (unsigned long long)n2);
    __syncthreads();  // every live wave's sweep-2 image and count
    const int srcs2 = sources();
    const int nsw2 = __popc(srcs2);
    const int cmask2 = SPLIT ? alive : srcs2, ncw2 = __popc(cmask2), crank2 = __popc(cmask2 & ((1 << wave) - 1));
    const bool in2 = ((cmask2 >> wave) & 1) != 0;
    if (nsw2 > 0) {
      const f2 NK = sp(nkappa);
      float p0[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, p1[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      auto sweep2 = [&](auto clamp_tag) {
        constexpr bool CLAMP = decltype(clamp_tag)::value;
        int u0 = 0, u1 = 0;
        if (in2) unit_range(crank2, nsw2, ncw2, u0, u1);
        for (int u = u0; u < u1;) {
          const int grp = u / nsw2, kb = u - grp * nsw2, ke = min(u1 - grp * nsw2, nsw2);
          u = grp * nsw2 + ke;
          const int j = grp * 64 + lane;
          float gx = -2.0f * kPadCenter, gy = 0.0f, gz = 0.0f, cc = kPadCenter * kPadCenter, kr = 0.0f;
          if (j < a.Mpad) {
            const int i = j >> 1;
            const bool h = (j & 1) != 0;
            const float4 A = R4[i], B = R4[np + i], R = R4[2 * np + i];
            gx = h ? A.y : A.x;
            gy = h ? A.w : A.z;
            gz = h ? B.y : B.x;
            cc = h ? B.w : B.z;
            kr = h ? R.y : R.x;
          }
          const f2 GX = sp(gx), GY = sp(gy), GZ = sp(gz), CC = sp(cc), KR = sp(kr), HX = sp(0.5f * gx),
                   HY = sp(0.5f * gy), HZ = sp(0.5f * gz);
          f2 agc[3] = {sp(0.0f), sp(0.0f), sp(0.0f)}, agr = sp(0.0f);
          for (int sw = 0, k = 0; sw < kWv; ++sw) {
            if (!((srcs2 >> sw) & 1)) continue;
            const int kk = k++;
            if (kk < kb || kk >= ke) continue;
            const int nps = (nsrc[sw] + 1) >> 1;
            for (int i2 = 0; i2 < nps; ++i2) {
              const int s0 = 2 * i2;
              const f2 PX = pair(sw, 0, s0), PY = pair(sw, 1, s0), PZ = pair(sw, 2, s0);
              const f2 PP = pair(sw, 3, s0);
              const f2 MA = pair(sw, 4, s0), HS = pair(sw, 5, s0);
              f2 q = fma2(PZ, GZ, fma2(PY, GY, fma2(PX, GX, PP + CC)));  // == qpair: the reconnect sweep's q
              const f2 qraw = q;
              if constexpr (CLAMP) q = clamp_q(q);
              const f2 r = rsq2(q);  // rho = q rsq(q) as in lse_point, 1/rho = rsq(q)
              const f2 h = exp2v(fma2(q * r, NK, KR) - MA) * HS;  // v - mA <= 0 exactly
              f2 hu = h * r;
              if constexpr (CLAMP) {
                hu.x = qraw.x >= 1e-6f ? hu.x : 0.0f;
                hu.y = qraw.y >= 1e-6f ? hu.y : 0.0f;
              }
              agc[0] = fma2(-hu, HX + PX, agc[0]);
              agc[1] = fma2(-hu, HY + PY, agc[1]);
              agc[2] = fma2(-hu, HZ + PZ, agc[2]);
              agr -= h;
            }
          }
          const float v[8] = {agc[0].x + agc[0].y, agc[1].x + agc[1].y, agc[2].x + agc[2].y, agr.x + agr.y,
                              0.0f, 0.0f, 0.0f, 0.0f};
          if (kb == 0 && ke == nsw2) {  // added to the group's sweep-1 columns 0-3
            if (j < a.Mpad) {
              float4* dst = reinterpret_cast<float4*>(rec + (long long)j * 8);
              float4 o = dst[0];
              o.x += v[0];
              o.y += v[1];
              o.z += v[2];
              o.w += v[3];
              dst[0] = o;
            }
          } else if (grp == u0 / nsw2) {
#pragma unroll
            for (int c = 0; c < 8; ++c) p0[c] = v[c];
          } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) p1[c] = v[c];
          }
        }
      };
      if (fast_a) sweep2(std::false_type{});
      else sweep2(std::true_type{});
      if (has_split(nsw2, ncw2)) finish_split(nsw2, ncw2, crank2, in2, 4, p0, p1);
    }
  }
  __syncthreads();

  // ---- per-ray scalar totals of the block (published before the sweeps)
  if (arank == 0 && lane < 8) {
    float acc = wscal[lane];
#pragma unroll
    for (int w = 1; w < (SPLIT ? kSplitWaves : kWaves); ++w) acc += wscal[w * 8 + lane];
    const float live = any_seed ? 1.0f : 0.0f;
    rec[(long long)a.Mpad * 8 + lane] = lane == 7 ? live : acc;  // scalar 7: live flag
  }
}

#include "rm_reduce.h"
#include "rm_small.h"
#include "rm_raygrad.h"
#include "rm_view.h"

// rm_debug_stall: one wave that holds its stream until the host sets *flag (a system-scope load
// of host-mapped memory, polled with s_sleep) or max_ticks of the 100 MHz real-time counter have
// passed -- every run of it ends by itself. Tests use it to stand for a stuck collective.
__global__ __launch_bounds__(64) void rm_stall_kernel(const int* flag, unsigned long long max_ticks) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0) {
    if (__builtin_amdgcn_s_memrealtime() - t0 > max_ticks) break;
    __builtin_amdgcn_s_sleep(100);
  }
}

}  // namespace rm

// =======================================================================================
// Host side (one translation unit): the context and its device buffers, the launch
// orchestration, and the C ABI of include/raymarch.h
// =======================================================================================
#include "rm_context.h"
#include "rm_launch.h"
#include "rm_api.h"
