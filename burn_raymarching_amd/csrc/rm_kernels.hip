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
// Sphere records are built once per call (rm_prep_kernel; rm_records.h) and read through the constant
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
#include <list>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/raymarch.h"
#include "rm_device.h"

namespace rm {

constexpr int kOrderClasses = 16;  // cost classes of the cost-ordered dispatch (order_append)
// The last class -- the blocks the proofs take at entry, two thirds of an 80-view launch, each alive
// for a few microseconds and all dispatched at the end of the launch -- appends to kOrderShards lists
// (by launch position & 3: an XCD pair each) where the launch is large (order_shard_policy,
// rm_launch.h), not to one: one word saturates near 88 returning device-scope
// atomics per microsecond (MI355X_MICROARCH.md, the dequeue row of its cross-CU primitives; not measured
// here), and that tail starts 85 blocks per microsecond -- inferred from the trace: sharded, a block of the tail lives
// 5.6 us instead of 7.8 (profiles/r27_order_shards.txt). The lists of the class follow each other
// in the dispatch order: the class-major order with the last class's blocks permuted.
constexpr int kOrderShards = RM_ORDER_SHARDS;
constexpr int kOrderLists = kOrderClasses - 1 + kOrderShards;
static_assert(kOrderShards > 0 && (kOrderShards & (kOrderShards - 1)) == 0, "launch position & (kOrderShards - 1) picks the list");
// ints between a set's class counts: each class on a 128-byte line of its own, as the reduction's
// arrival counters below (both: C2cj 4348-4404 vs 4305-4315 Mrays/s with neither, the metric
// equal; tools/gpu_ab.sh, profiles/r05e_ab.txt)
constexpr int kOrderClsStride = 32;
// ints between the three list sets' class counts and before the turn word: each on cache lines of
// its own (every block of a launch reads the turn and the previous set's counts while the blocks'
// appends hit the current set's counts with atomics; sharing a 128-byte line made every launch
// that appended to the set next to the turn word 50 % slower at C2: tools/order_probe.py)
constexpr int kOrderCntStride = kOrderLists * kOrderClsStride > 64 ? kOrderLists * kOrderClsStride : 64;
static_assert(kOrderCntStride >= kOrderLists * kOrderClsStride && kOrderCntStride % 32 == 0, "128-byte lines per set");
constexpr int kRedArrStride = 32;  // unsigneds between rm_reduce_partials' arrival counters: a 128-byte line each

// kRender: the non-differentiable target renderer of renderer.rs:4-80 (generate.rs)
enum Mode { kFwd = 0, kBwd = 1, kTrain = 2, kRender = 3 };

// bounds the partial-gradient workspace per launch: 128 views of 512 x 512 in one launch (per-launch
// ramp-down and the per-call record, origin and reduction launches amortised over all the views of a step)
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
// register budget of the split kernels (waves per SIMD): 3 = 168 VGPRs, no spills (4: 128 VGPRs,
// 4-12 VGPR spills, 20 B/lane scratch; C5 equal either way)
constexpr int kSplitMinWaves = 3;
constexpr int kSplitWaves = 4;  // waves per ray group of the split march (2 or 4)
static_assert(kSplitWaves == 2 || kSplitWaves == 4, "split blocks have 2 or 4 waves");
// Rays per split block (64, 32 or 16). Below 64 every wave of the block holds each of its rays
// 64 / kSplitRays times (lane l and l + kSplitRays carry the same ray, bit for bit) and the
// march's matrix-core tiles run kSplitRays / 16 column blocks instead of 4: a march step of a
// block costs its waves kSplitRays / 64 of the 64-ray step, so heavy rays hold their SIMDs for
// shorter and the blocks that march to the end are smaller work units (configs[4]).
constexpr int kSplitRays = 32;  // (same box, the work-unit backward: C5 +3.5 %, C5g +5 % against 64)
static_assert(kSplitRays == 64 || kSplitRays == 32 || kSplitRays == 16, "split blocks hold 64, 32 or 16 rays");
constexpr int kSplitCB = kSplitRays / 16;  // column blocks of 16 rays in the split march's tiles
constexpr long long kSplitMaxRays = 262144;
constexpr int kStatsWords = 6;  // rm_stats device counters (KArgs::stats)
constexpr int kReduceSegs = 128;  // block segments of the reduction (128: 12.6 + 6.9 us at 10 views vs 20.3 + 4.9 with 64)

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
  int proof;                  // the escape proof before the march (rm_ray_kernel<.., PROOF>; proof_tier): 1 the
                              // soft ball alone, 2 with the call's lattice (the tile proof before the launch, or per ray in bound_proof)
  int split;                  // split march (RM_MARCH_SPLIT): kSplitRays rays per block, a quarter of the spheres per wave
  int mfma;                   // march sums on the matrix cores (lse_mfma) instead of lse_weighted
  int shift_max;              // RM_MARCH_FORCE_MAX_SHIFT: every march step takes the running-max shift
  const int* esc_flags;       // nullable: per-block escape flags of this launch (rm_escape_kernel)
  const int* block_order;     // nullable: heavy-first dispatch order of the tiles of a view (ray_block)
  // order_views: the views in its low 16 bits; above them kOrderShards - 1 where the cost order's last
  // class appends to (and is read from) its kOrderShards lists, 0 where it keeps to the first of them
  // (order_shard_policy) -- carried here, beside what ray_block reads anyway, not in a field of its own at
  // the end of the arguments: read from there it cost the unsharded C2 launch 0.4-1.0 %, here nothing
  // (profiles/r27_order_shards.txt, section 6)
  int order_views, order_tiles;
  // cost-ordered dispatch: [list][kMaxBlocksPerLaunch] block lists (kOrderLists) + [list] counts of the
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
  // cont_state: per-ray rows of cont_rays floats, then two words per group; ContState (rm_ray.h)
  // defines the layout.
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
  // nullable: the call's escape lattice, kLatticeN^3 cell-centre soft-min values (proof == 2;
  // rm_lattice_kernel). Last, so that the kernels that never read it see the arguments where they were.
  const float* lattice;
  // nullable: one byte per wave of this launch (logical block * kWaves + wave), 1 where rm_tile_proof_kernel
  // proved every ray of the wave gone from the lattice (proof == 2, the launches tile_proof_policy picks)
  const unsigned char* tile_proof;
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

#include "rm_proof.h"
#include "rm_records.h"

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
    if (lane == 0 && wave == 0) orig[RecTail::kD0 + v] = D;
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
      orig[RecTail::kRhoLb + v] =
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
    constexpr long long kSet = (long long)kOrderLists * kMaxBlocksPerLaunch;
    if (o.list_r != nullptr) {
      o.list_r += r * kSet;
      o.cnt_r += r * kOrderCntStride;
    }
    if (o.list_w != nullptr) {
      o.list_w += w * kSet;
      o.cnt_w += w * kOrderCntStride;
    }
    if (o.cnt_z != nullptr) o.cnt_z += z * kOrderCntStride;
  }
  return o;
}

// The list and entry of position b in the concatenation of the first N lists counted by cnt; -1
// unless the counts sum to the grid.
template <int N>
__device__ __forceinline__ int order_locate(const int* cnt, int b, int& idx) {
  int tot = 0, cb = -1, base = 0;
#pragma unroll
  for (int c = 0; c < N; ++c) {
    const int n = cnt[c * kOrderClsStride];
    if (cb < 0 && b < tot + n) {
      cb = c;
      base = tot;
    }
    tot += n;
  }
  idx = b - base;
  return tot == (int)gridDim.x ? cb : -1;
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
    // reads the same counts, so a short total (never expected) sends all blocks to the static order.
    // A launch that does not shard its last class reads the first kOrderClasses lists alone.
    int idx;
    const int cb = (a.order_views >> 16) != 0 ? order_locate<kOrderLists>(os.cnt_r, b, idx)
                                           : order_locate<kOrderClasses>(os.cnt_r, b, idx);
    if (cb >= 0) return os.list_r[cb * kMaxBlocksPerLaunch + idx];
  }
  const int nv = a.order_views & 0xFFFF;
  const int r = b / nv, v = b - r * nv;
  return (long long)v * a.order_tiles + a.block_order[r];
}

// Appends the block to its cost class's list for the next launch's dispatch order (class 0: the
// dearest blocks; cost in march-step units, see the hand-off in rm_ray_kernel).
__device__ __forceinline__ void order_append(const KArgs& a, long long blk, int cost) {
  constexpr int kCls = kOrderClasses;
  const float cls_scale = (float)kCls / (float)((a.split ? 1 : kWaves) * (a.steps + kPostCost) + 1);
  int c = kCls - 1 - (int)fminf((float)cost * cls_scale, (float)(kCls - 1));
  if (c == kCls - 1) c += (int)blockIdx.x & (a.order_views >> 16);  // the last class: the list of this position's XCD pair
  const OrderSets os = order_sets(a);
  const int idx = atomicAdd(os.cnt_w + c * kOrderClsStride, 1);
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

#include "rm_ray.h"
#include "rm_reduce.h"
#include "rm_small.h"
#include "rm_raygrad.h"
#include "rm_view.h"
#include "rm_sdf.h"
#include "rm_sh.h"
#include "rm_loss.h"

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
