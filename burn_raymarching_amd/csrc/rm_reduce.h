// rm_reduce.h -- the kernels around the per-ray kernel: the fixed-order cross-block
// reduction of the partial records and its finalize, the gather / sample / activate helpers, the
// repulsion penalty and the Adam optimizer kernels. Included by rm_kernels.hip inside namespace rm,
// after rm_ray_kernel and before the small-scene kernel (rm_small.h), which shares FinalArgs and
// the finalize and optimizer helpers.
#pragma once

// ---- cross-block reduction (fixed order => deterministic) --------------------------------
// Partial record of one ray block (rec = Mpad*8 + 8 floats):
//   [Mpad][8] (gc.xyz, gr, gcol.rgb, 0) -- backward sweep 1's terms, sweep 2's (gc, gr) terms added
//   by the block itself -- | 8 scalars
// Scalar 7 is the block's live flag: 0 when every wave of the block left the march early or no ray
// of it has a non-zero backward seed (its per-sphere columns are all zero and were not written),
// 1 otherwise.
// Output columns (ncols = Mpad*8 + 8): [Mpad][8] combined per-sphere grads | 8 scalars.
//
// Pass 1, grid (column blocks x segments of ray blocks): each block sums its segment for its 256
// columns into S[seg][col] -- one addition chain per column in ray-block order, loads batched
// eight rows at a time. Rows of dead
// blocks are skipped: they only hold zeros, and adding +0 leaves a chain unchanged, so the sums
// are those of the full chain.
struct FinalArgs {
  const float* light_dir;
  float *gc, *gcol, *gr, *gld, *gamb, *loss_sum;
  int accumulate;
  int* oturn;  // nullable: the cost-order turn word the reduction advances (KArgs::oturn)
  // rm_train_step_camera_adam on a model of M <= kOptSmallMaxM spheres: the optimizer step on the
  // packed gradient (grad = gc: the packed layout) runs in the reduction's last block
  // (fused_optimizer); raw == nullptr otherwise
  float *raw, *m1, *m2, *act_out, *loss_penalty;
  _Float16* col_h;
  rm_step_scalars* sdev;
  unsigned* opt_arrival;  // the column blocks' arrival counter (zero between launches)
  int step, with_pen;
  float lr, wd;
};
__device__ void fused_optimizer(const FinalArgs& f, int M);

constexpr int kReduceBatch = 8;  // partial rows in flight per thread
constexpr int kFinU = 16;        // finalize_block: 4 * kFinU loads in flight (32 with batch 16: no gain at C2)
static_assert((kReduceSegs / 4) % kFinU == 0, "finalize_block rounds");

__device__ void finalize_block(const float* S, int nseg, int M, int Mpad, const FinalArgs& f, float* tot);

// Segments of the reduction of nblocks ray blocks: kReduceSegs, or as many multiples of 64 as a
// launch of more than kReduceSegs * 256 blocks needs (a segment's rows fit pass 1's 256-entry list)
__host__ __device__ inline int reduce_segs(long long nblocks) {
  const long long need = (nblocks + 255) / 256;
  return need <= kReduceSegs ? kReduceSegs : (int)((need + 63) / 64 * 64);
}

__global__ __launch_bounds__(256) void rm_reduce_partials(const float* __restrict__ P, long long rec, int M, int Mpad,
                                                          int nblocks, int seg_len, float* __restrict__ S,
                                                          const FinalArgs f, unsigned* __restrict__ arrivals) {
  __shared__ int rows[256];
  __shared__ int wcount[4];
  __shared__ float tot[256];
  __shared__ int last;
  const int ncols = Mpad * 8 + 8;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the launch whose partials these are has finished: the cost-ordered dispatch turns one set on
  if (f.oturn != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) *f.oturn = (*f.oturn + 1) % 3;
  const int col = blockIdx.x * 256 + tid;
  const bool scalars = (int)blockIdx.x * 256 >= Mpad * 8;  // the column block of the 8 scalars
  const int b0 = blockIdx.y * seg_len;
  const int b1 = min(b0 + seg_len, nblocks);
  // rows of this segment to visit, in order: every row for the scalars, live rows otherwise
  {
    const int b = b0 + tid;
    const bool take = b < b1 && (scalars || P[(long long)b * rec + (long long)Mpad * 8 + 7] != 0.0f);
    const unsigned long long m = __ballot(take);
    if (lane == 0) wcount[wave] = __popcll(m);
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += wcount[w];
    if (take) rows[base + __popcll(m & ((1ull << lane) - 1))] = b;
    __syncthreads();
  }
  const int nrows = wcount[0] + wcount[1] + wcount[2] + wcount[3];
  if (col < ncols) {
    float acc = 0.0f;  // columns map 1:1 onto the record (per-sphere block, then the scalars)
    for (int i0 = 0; i0 < nrows; i0 += kReduceBatch) {
      float v1[kReduceBatch];
#pragma unroll
      for (int u = 0; u < kReduceBatch; ++u) v1[u] = P[(long long)rows[min(i0 + u, nrows - 1)] * rec + col];
#pragma unroll
      for (int u = 0; u < kReduceBatch; ++u)
        if (i0 + u < nrows) acc += v1[u];
    }
    if (arrivals == nullptr) S[(long long)blockIdx.y * ncols + col] = acc;
    else __hip_atomic_store(S + (long long)blockIdx.y * ncols + col, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (arrivals == nullptr) return;
  // Pass 2 in the same launch: the segment block that arrives last for this column block sums
  // the segments and scatters them (finalize_block, the bits of rm_finalize_grads). Hand-off
  // (MI355X_MICROARCH.md, inter-workgroup visibility): write-through segment stores drained by
  // every wave before the block barrier, one lane's agent-scope arrival, an agent-scope acquire
  // and write-through-cache loads in the last block -- the guide's write-through variant of the
  // counter hand-off, which needs no release fence (cdna_hip_programming.md §5 split-K item 2);
  // stressed under uneven load against the two-launch reduction in tests/test_gpu_fusion.py.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const unsigned prev = __hip_atomic_fetch_add(arrivals + blockIdx.x * kRedArrStride, 1u, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
    last = prev == gridDim.y - 1 ? 1 : 0;
  }
  __syncthreads();
  if (!last) return;
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  finalize_block(S, (int)gridDim.y, M, Mpad, f, tot);
  if (tid == 0) __hip_atomic_store(arrivals + blockIdx.x * kRedArrStride, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (f.raw == nullptr) return;
  // the optimizer step on the whole gradient, by the column block that finishes last: the same
  // write-through hand-off one level up (finalize_block stored its gradient elements write-through)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const unsigned prev = __hip_atomic_fetch_add(f.opt_arrival, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = prev == gridDim.x - 1 ? 1 : 0;
  }
  __syncthreads();
  if (!last) return;
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  fused_optimizer(f, M);
  if (tid == 0) __hip_atomic_store(f.opt_arrival, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Pass 2 for the 256 columns of pass-1 column block blockIdx.x, by the block of that column block
// that arrived last: thread t sums column t's kReduceSegs segments in the four chains s mod 4 of
// rm_finalize_grads, combined (a0 + a1) + (a2 + a3) -- the same bits -- then the scatter.
// The light-direction gradient: light_grad (contraction off), the same function in both pass-2
// forms (finalize_block, rm_finalize_grads) and in the small kernel's final block.

// a gradient element of the final scatter: write-through when the fused optimizer reads it
__device__ __forceinline__ void put_grad(const FinalArgs& f, float* dst, float v) {
  const float x = f.accumulate ? *dst + v : v;
  if (f.raw != nullptr) __hip_atomic_store(dst, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *dst = x;
}
__device__ void finalize_block(const float* S, int nseg, int M, int Mpad, const FinalArgs& f, float* tot) {
  const int ncols = Mpad * 8 + 8;
  const int tid = threadIdx.x;
  const int col = blockIdx.x * 256 + tid;
  const int c = min(col, ncols - 1);
  // kU * 4 loads in flight per thread (the last block runs alone: registers are free)
  constexpr int kU = kFinU;
  float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int u0 = 0; u0 < nseg / 4; u0 += kU) {
    float v[kU][4];
#pragma unroll
    for (int u = 0; u < kU; ++u)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        v[u][k] = __hip_atomic_load(S + (long long)(4 * (u0 + u) + k) * ncols + c, __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int u = 0; u < kU; ++u)
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] += v[u][k];
  }
  tot[tid] = (a[0] + a[1]) + (a[2] + a[3]);
  __syncthreads();
  if (col >= ncols) return;
  if (col < Mpad * 8) {
    const int j = col >> 3, comp = col & 7;
    if (j >= M || comp == 7) return;
    const float v = tot[tid];
    float* dst = comp < 3 ? (f.gc ? f.gc + 3 * j + comp : nullptr)
                          : (comp == 3 ? (f.gr ? f.gr + j : nullptr) : (f.gcol ? f.gcol + 3 * j + (comp - 4) : nullptr));
    if (dst) put_grad(f, dst, v);
    return;
  }
  const int sc = col - Mpad * 8;  // the scalars open their column block (Mpad * 8 % 256 == 0)
  if (sc == 0 && f.gld) {
    const float r[3] = {tot[tid], tot[tid + 1], tot[tid + 2]};
#pragma unroll
    for (int k = 0; k < 3; ++k) put_grad(f, f.gld + k, light_grad(r, f.light_dir, k));
  } else if (sc == 3 && f.gamb) {
    put_grad(f, f.gamb, tot[tid]);
  } else if (sc == 4 && f.loss_sum) {
    f.loss_sum[0] = f.accumulate ? f.loss_sum[0] + tot[tid] : tot[tid];
  }
}

// Pass 2 as its own launch (RM_REDUCE_FUSED=0): sum the segments in order and scatter into the
// caller's gradient layout.
// gld = (g_ell - ldn (ldn . g_ell)) / |ld| applies the Jacobian of ld / |ld| (renderer_diff.rs:49-50).
__global__ __launch_bounds__(256) void rm_finalize_grads(const float* __restrict__ S, int nseg, int M, int Mpad,
                                                         FinalArgs f) {
  // 64 columns per block, four threads per column: thread (chain k, column) sums the segments
  // s = k mod 4 in order -- the four chains of one thread's former loop (a[s & 3] += v[s]) --
  // and the chains are combined as before, (a0 + a1) + (a2 + a3): the same bits, the loads
  // spread over four times as many CUs
  __shared__ float part[4][64];
  const int ncols = Mpad * 8 + 8;
  const int cl = threadIdx.x & 63, chain = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cl;
  static_assert(kReduceSegs % 64 == 0, "four chains of 16-load rounds");
  {
    // nseg (reduce_segs: a multiple of 64) segments, chain `chain` sums s = chain mod 4 in order,
    // kReduceSegs / 4 loads in flight
    constexpr int kC = kReduceSegs / 4;
    const int c = min(col, ncols - 1);
    float acc = 0.0f;
    for (int u0 = 0; u0 < nseg / 4; u0 += kC) {
      float v[kC];
#pragma unroll
      for (int u = 0; u < kC; ++u) v[u] = u0 + u < nseg / 4 ? S[(long long)(4 * (u0 + u) + chain) * ncols + c] : 0.0f;
#pragma unroll
      for (int u = 0; u < kC; ++u)
        if (u0 + u < nseg / 4) acc += v[u];
    }
    part[chain][cl] = acc;
  }
  __syncthreads();
  if (chain != 0 || col >= ncols) return;
  auto seg_sum = [&](int l) { return (part[0][l] + part[1][l]) + (part[2][l] + part[3][l]); };
  if (col < Mpad * 8) {
    const int j = col >> 3, comp = col & 7;
    if (j >= M || comp == 7) return;
    const float v = seg_sum(cl);
    float* dst = comp < 3 ? (f.gc ? f.gc + 3 * j + comp : nullptr)
                          : (comp == 3 ? (f.gr ? f.gr + j : nullptr) : (f.gcol ? f.gcol + 3 * j + (comp - 4) : nullptr));
    if (dst) *dst = f.accumulate ? *dst + v : v;
    return;
  }
  const int sc = col - Mpad * 8;  // Mpad * 8 is a multiple of 64: the scalars open their block
  if (sc == 0 && f.gld) {
    const float r[3] = {seg_sum(cl), seg_sum(cl + 1), seg_sum(cl + 2)};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float gv = light_grad(r, f.light_dir, c);
      f.gld[c] = f.accumulate ? f.gld[c] + gv : gv;
    }
  } else if (sc == 3 && f.gamb) {
    const float v = seg_sum(cl);
    f.gamb[0] = f.accumulate ? f.gamb[0] + v : v;
  } else if (sc == 4 && f.loss_sum) {
    const float v = seg_sum(cl);
    f.loss_sum[0] = f.accumulate ? f.loss_sum[0] + v : v;
  }
}

// ---- model helpers (scene.rs:41-45, training.rs:38-82, Burn Adam) -------------------------
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
// burn::tensor::activation::softplus(x, 1) = log(1 + exp(x))
__device__ __forceinline__ float softplusf_(float x) { return logf(1.0f + expf(x)); }

// scene.rs:41-45 on packed element i (layout [centers 3M | colors 3M | radius M | light 3 | ambient 1]).
__device__ __forceinline__ float activate_elem(float x, int i, int M) {
#pragma clang fp contract(off)
  if (i < 3 * M) return x;                           // centers
  if (i < 6 * M) return sigmoidf_(x);                // colors = sigmoid(raw)        scene.rs:41
  if (i < 7 * M) return softplusf_(x) + 0.01f;       // radius = softplus(raw)+0.01  scene.rs:43
  if (i < 7 * M + 3) return x;                       // light_dir raw                scene.rs:44
  return sigmoidf_(x);                               // ambient = sigmoid(raw)       scene.rs:45
}

// dataset.rs:75-79: rows idx[i] of the ray / target arrays -> the batch (3 floats per row per
// array). An index outside [0, num_src) yields a zero row rather than an out-of-bounds read.
__global__ __launch_bounds__(256) void rm_gather_kernel(const float* __restrict__ org, const float* __restrict__ dir,
                                                        const float* __restrict__ tgt, long long num_src,
                                                        const int32_t* __restrict__ idx, long long n,
                                                        float* __restrict__ oo, float* __restrict__ od,
                                                        float* __restrict__ ot) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;  // one float of the [n,3] batch
  if (e >= 3 * n) return;
  const long long i = e / 3;
  const int c = (int)(e - 3 * i);
  const long long j = idx[i];
  const bool ok = j >= 0 && j < num_src;
  const long long s = 3 * j + c;
  if (oo) oo[e] = ok ? org[s] : 0.0f;
  if (od) od[e] = ok ? dir[s] : 0.0f;
  if (ot) ot[e] = ok ? tgt[s] : 0.0f;
}

// SceneDataset::sample_batch on the device (dataset.rs:47-82): batch row i draws its pixel from
// a counter-based generator -- splitmix64 over key + (i + 1) * golden, the key mixing (seed,
// stream, counter) -- so a draw depends only on its position, not on the launch geometry: rows
// i < n_uniform take a pixel uniformly from [0, num_src), the rest a foreground pixel uniformly
// from fg[0, num_fg) (the index is the high 64 bits of r * n: bias n / 2^64). Then the row's
// ray origin, direction and target are gathered (dataset.rs:75-79). One thread per row.
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__global__ __launch_bounds__(256) void rm_sample_kernel(const float* __restrict__ org, const float* __restrict__ dir,
                                                        const float* __restrict__ tgt, long long num_src,
                                                        const int32_t* __restrict__ fg, long long num_fg,
                                                        long long n_uniform, long long n, unsigned long long key,
                                                        float* __restrict__ oo, float* __restrict__ od,
                                                        float* __restrict__ ot, int32_t* __restrict__ idx_out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long r = splitmix64(key + (unsigned long long)(i + 1) * 0x9E3779B97F4A7C15ull);
  long long j;
  if (i < n_uniform) j = (long long)__umul64hi(r, (unsigned long long)num_src);
  else j = fg[__umul64hi(r, (unsigned long long)num_fg)];
  if (idx_out) idx_out[i] = (int32_t)j;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (oo) oo[3 * i + c] = org[3 * j + c];
    if (od) od[3 * i + c] = dir[3 * j + c];
    if (ot) ot[3 * i + c] = tgt[3 * j + c];
  }
}

__global__ __launch_bounds__(256) void rm_activate_kernel(const float* __restrict__ raw, int M,
                                                          float* __restrict__ act) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 7 * M + 4) return;
  act[i] = activate_elem(raw[i], i, M);
}

// Block reduction of 4 floats over 256 threads in fixed tree order (deterministic).
__device__ __forceinline__ void block_sum4(float (&v)[4], float* red) {
#pragma unroll
  for (int c = 0; c < 4; ++c) red[c * 256 + threadIdx.x] = v[c];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) {
#pragma unroll
      for (int c = 0; c < 4; ++c) red[c * 256 + threadIdx.x] += red[c * 256 + threadIdx.x + w];
    }
    __syncthreads();
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) v[c] = red[c * 256];
}

// Repulsion row of sphere s (training.rs:73-82) over j = j0, j0 + stride, ... < M, added to v:
// dist_sj = sqrt(max(|c_s|^2 + |c_j|^2 - 2 c_s.c_j, 1e-6)), value (dist + 100 I + 1e-6)^-1 into
// v[3], its gradient w.r.t. c_s through both the (s, j) and (j, s) entries into v[0..2].
// c: the pre-step centres [M][3] (raw = activated).
__device__ __forceinline__ void repulsion_row(const float* c, int M, int s, int j0, int stride, float (&v)[4]) {
#pragma clang fp contract(off)
  const float cx = c[3 * s], cy = c[3 * s + 1], cz = c[3 * s + 2];
  const float csq = cx * cx + cy * cy + cz * cz;
  for (int j = j0; j < M; j += stride) {
    const float ox = c[3 * j], oy = c[3 * j + 1], oz = c[3 * j + 2];
    const float q = (csq + (ox * ox + oy * oy + oz * oz)) - (cx * ox + cy * oy + cz * oz) * 2.0f;
    const float qc = fmaxf(q, 1e-6f);
    const float rho = sqrtf(qc);
    const float den = rho + (j == s ? 100.0f : 0.0f) + 1e-6f;
    const float inv = frcp(den);  // v_rcp / v_rsq (1 ulp) instead of IEEE divisions: O(M^2) pairs
    v[3] += inv;
    if (j != s && q >= 1e-6f) {  // clamp_min(1e-6) gate (the diagonal has q ~ 0)
      const float gs = -2.0f * inv * inv * frsq(qc);
      v[0] += gs * (cx - ox);
      v[1] += gs * (cy - oy);
      v[2] += gs * (cz - oz);
    }
  }
}

// Pass A of the optimizer: block s owns sphere s. It snapshots the sphere's raw parameters
// (the update kernel reads neighbours' pre-step values) and, with penalties, sums the
// repulsion row of training.rs:73-82 over j (repulsion_row), block tree reduction.
__global__ __launch_bounds__(256) void rm_penalty_pairs(const float* __restrict__ raw, int M, int with_pen,
                                                        float* __restrict__ snap, float* __restrict__ pair) {
  __shared__ float red[4 * 256];
  const int s = blockIdx.x;
  if (threadIdx.x < 7) {
    const int idx = threadIdx.x < 3 ? 3 * s + threadIdx.x
                                    : (threadIdx.x < 6 ? 3 * M + 3 * s + (threadIdx.x - 3) : 6 * M + s);
    snap[idx] = raw[idx];
  }
  if (s == 0 && threadIdx.x >= 32 && threadIdx.x < 36) snap[7 * M + threadIdx.x - 32] = raw[7 * M + threadIdx.x - 32];
  if (!with_pen) return;
  float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  repulsion_row(raw, M, s, threadIdx.x, 256, v);
  block_sum4(v, red);
  if (threadIdx.x < 4) pair[4 * s + threadIdx.x] = v[threadIdx.x];
}

// One parameter element i of the packed layout: chain rule of the activations, the compute_loss
// penalties (training.rs:38-82), coupled weight decay and Burn's Adam; optionally the activated
// parameters of the updated model (scene.rs:41-45) for the next step's render. Contraction is off
// in these functions (explicit fmaf where a fused multiply-add is meant): the optimizer runs inside
// several kernels (its own launches, the reduction's and the small kernel's last blocks), and its
// bits must not depend on which. Split in two: the
// part that depends on the pre-step parameters only (optimizer_pre: the chain-rule factor, the
// penalties' gradient terms and loss share -- the fused iteration runs it while the gradient is
// still being summed) and the update itself (optimizer_apply).
struct ElemPre {
  float fac;         // d activation / d raw (1 for centres and light)
  float t0, t1, t2;  // penalty gradient terms, added in this order after the chain rule
  float pen;         // the element's penalty-loss share
};
// raw: the pre-step parameters (a snapshot: neighbours are read); pair: the repulsion rows.
__device__ __forceinline__ ElemPre optimizer_pre(int i, const float* raw, const float* pair, int M, int with_pen) {
#pragma clang fp contract(off)
  ElemPre e{1.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  const float x = raw[i];
  const float invM = 1.0f / (float)M;
  const float rep_scale = 1e-5f / ((float)M * (float)M);
  if (i < 3 * M) {  // centers (identity activation)
    if (with_pen) {
      const int s = i / 3, ax = i - 3 * s;
      const float cx = raw[3 * s], cy = raw[3 * s + 1], cz = raw[3 * s + 2];
      const float rs = softplusf_(raw[6 * M + s]);  // penalties use softplus without +0.01 (training.rs:41)
      e.t0 = 0.05f * 2.0f * x / (3.0f * M);         // [b] mean(c^2) over [M,3] * 0.05
      const float csq = cx * cx + cy * cy + cz * cz;
      const float dist = sqrtf(csq + 1e-6f);
      const float reach = dist + rs;                // [c] mean(mask * (|c| + r - 1.2)^2) * 5
      if (reach > 1.2f) e.t1 = 5.0f * invM * 2.0f * (reach - 1.2f) * (x / dist);
      e.t2 = rep_scale * pair[4 * s + ax];          // [d] repulsion (repulsion_row)
      if (ax == 0) {
        e.pen += 0.05f * csq / (3.0f * M);
        if (reach > 1.2f) e.pen += 5.0f * invM * (reach - 1.2f) * (reach - 1.2f);
        e.pen += rep_scale * pair[4 * s + 3];
      }
    }
  } else if (i < 6 * M) {  // colors: d sigmoid = c (1 - c)
    const float c = sigmoidf_(x);
    e.fac = c * (1.0f - c);
  } else if (i < 7 * M) {  // radius: d (softplus + 0.01) = sigmoid
    const float sg = sigmoidf_(x);
    e.fac = sg;
    if (with_pen) {
      const int s = i - 6 * M;
      const float rs = softplusf_(x);
      e.t0 = 0.002f * invM * (rs > 0.0f ? 1.0f : (rs < 0.0f ? -1.0f : 0.0f)) * sg;  // [a] L1
      e.pen += 0.002f * invM * fabsf(rs);
      if (rs > 1.0f) {  // [a] large radius
        e.t1 = 0.04f * invM * 2.0f * rs * sg;
        e.pen += 0.04f * invM * rs * rs;
      }
      const float cx = raw[3 * s], cy = raw[3 * s + 1], cz = raw[3 * s + 2];
      const float reach = sqrtf(cx * cx + cy * cy + cz * cz + 1e-6f) + rs;
      if (reach > 1.2f) e.t2 = 5.0f * invM * 2.0f * (reach - 1.2f) * sg;  // [c] w.r.t. radius
    }
  } else if (i >= 7 * M + 3) {  // ambient: d sigmoid (light_dir raw: identity)
    const float a = sigmoidf_(x);
    e.fac = a * (1.0f - a);
  }
  return e;
}

// Adam's bias corrections 1 - beta^t (Burn Adam: beta1 0.9, beta2 0.999)
struct AdamBias {
  float c1, c2;
};
__device__ __forceinline__ AdamBias adam_bias(int step) {
  return AdamBias{1.0f - powf(0.9f, (float)step), 1.0f - powf(0.999f, (float)step)};
}

// The update of element i from its gradient g w.r.t. the activated value, its pre-step raw value
// x and moments mo1 / mo2: gv = g fac + t0 + t1 + t2, Burn Adam with coupled weight decay
// (g += wd theta; moments; bias correction).
__device__ __forceinline__ void optimizer_apply(int i, const ElemPre& e, float g, float x, float mo1, float mo2,
                                                const AdamBias& bias, float lr, float wd, int M,
                                                float* __restrict__ raw_out, float* __restrict__ m1,
                                                float* __restrict__ m2, float* __restrict__ act_out,
                                                _Float16* __restrict__ col_h_out) {
#pragma clang fp contract(off)
  float gv = ((g * e.fac + e.t0) + e.t1) + e.t2;
  gv = fmaf(wd, x, gv);
  const float b1 = 0.9f, b2 = 0.999f, eps = 1e-5f;
  const float mm = fmaf(b1, mo1, (1.0f - b1) * gv);
  const float vv = fmaf(b2, mo2, (1.0f - b2) * gv * gv);
  m1[i] = mm;
  m2[i] = vv;
  const float mh = mm / bias.c1;
  const float vh = vv / bias.c2;
  const float xn = x - lr * (mh / (sqrtf(vh) + eps));
  raw_out[i] = xn;
  if (act_out) act_out[i] = activate_elem(xn, i, M);
  // fp16 colour models (RM_MARCH_COLOR_F16): the next render's colours, rounded to nearest
  if (col_h_out != nullptr && i >= 3 * M && i < 6 * M) col_h_out[i - 3 * M] = (_Float16)activate_elem(xn, i, M);
}

// Both parts for one element; returns the element's penalty-loss share.
__device__ __forceinline__ float optimizer_elem(int i, const float* raw, float* __restrict__ raw_out,
                                                const float* __restrict__ gact, const float* m1_in,
                                                const float* m2_in, float* __restrict__ m1, float* __restrict__ m2,
                                                const float* pair, int M, int step, float lr, float wd, int with_pen,
                                                float* __restrict__ act_out, _Float16* __restrict__ col_h_out) {
  const ElemPre e = optimizer_pre(i, raw, pair, M, with_pen);
  optimizer_apply(i, e, gact[i], raw[i], m1_in[i], m2_in[i], adam_bias(step), lr, wd, M, raw_out, m1, m2, act_out,
                  col_h_out);
  return e.pen;
}

// Pass B: one thread per parameter element (optimizer_elem); per-block penalty partials.
__global__ __launch_bounds__(256) void rm_optimizer_kernel(const float* __restrict__ raw, float* __restrict__ raw_out,
                                                           const float* __restrict__ gact,
                                                           float* __restrict__ m1, float* __restrict__ m2,
                                                           const float* __restrict__ pair, int M, int step,
                                                           float lr, float wd, int with_pen,
                                                           float* __restrict__ pen_parts,
                                                           float* __restrict__ act_out,
                                                           _Float16* __restrict__ col_h_out,
                                                           const rm_step_scalars* __restrict__ sdev) {
  __shared__ float red[4 * 256];
  if (sdev != nullptr) step = sdev->step;  // device step scalars (rm_bind_step_scalars)
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int n = 7 * M + 4;
  float pen = 0.0f;
  if (i < n)
    pen = optimizer_elem(i, raw, raw_out, gact, m1, m2, m1, m2, pair, M, step, lr, wd, with_pen, act_out, col_h_out);
  if (pen_parts != nullptr) {
    float v[4] = {pen, 0.0f, 0.0f, 0.0f};
    block_sum4(v, red);
    if (threadIdx.x == 0) pen_parts[blockIdx.x] = v[0];
  }
}

// The optimizer step of a small model (M <= kOptSmallMaxM) in one block: the pre-step parameters
// into LDS (the snapshot rm_penalty_pairs writes), the repulsion rows of training.rs:73-82 (four
// threads per sphere, their partials added in order), optimizer_pre per element and the penalty
// sum (block tree reduction) -- everything that does not need the gradient (opt_small_pre) --
// then optimizer_apply per element (opt_small_post). One launch instead of three.
// OptPrefetch: the block's loads of the parameters and moments (elements tid and tid + 256),
// issued before whatever the block does next (the fused iteration's final reduction) so that
// their latency overlaps it.
constexpr int kOptSmallMaxM = 64;
struct OptPrefetch {
  float x[2], a[2], b[2];
};
__device__ __forceinline__ OptPrefetch opt_prefetch(const float* raw, const float* m1, const float* m2, int M) {
  OptPrefetch f;
  const int n = 7 * M + 4;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = (int)threadIdx.x + 256 * h;
    f.x[h] = i < n ? raw[i] : 0.0f;
    f.a[h] = i < n ? m1[i] : 0.0f;
    f.b[h] = i < n ? m2[i] : 0.0f;
  }
  return f;
}
struct OptPre {
  ElemPre e[2];  // elements tid and tid + 256
  AdamBias bias;
};

// The gradient-independent part, for a 256-thread block (every thread calls it: block barriers).
__device__ __forceinline__ OptPre opt_small_pre(const OptPrefetch& pf, int M, int step, int with_pen,
                                                float* __restrict__ loss_penalty) {
  static_assert(7 * kOptSmallMaxM + 4 <= 512, "two elements per thread");
  __shared__ float snap[7 * kOptSmallMaxM + 4];
  __shared__ float part[4][kOptSmallMaxM][4];
  __shared__ float pair[kOptSmallMaxM * 4];
  __shared__ float red[4 * 256];
  const int tid = threadIdx.x;
  const int n = 7 * M + 4;
  OptPre o;
  o.bias = adam_bias(step);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = tid + 256 * h;
    if (i < n) snap[i] = pf.x[h];
  }
  __syncthreads();
  if (with_pen) {
    const int s = tid >> 2, k = tid & 3;  // sphere s, columns j = k mod 4
    if (s < M) {
      float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      repulsion_row(snap, M, s, k, 4, v);
#pragma unroll
      for (int c = 0; c < 4; ++c) part[k][s][c] = v[c];
    }
    __syncthreads();
    if (tid < 4 * M) {
      const int s2 = tid >> 2, c = tid & 3;
      pair[4 * s2 + c] = ((part[0][s2][c] + part[1][s2][c]) + part[2][s2][c]) + part[3][s2][c];
    }
    __syncthreads();
  }
  float pen = 0.0f;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = tid + 256 * h;
    o.e[h] = i < n ? optimizer_pre(i, snap, pair, M, with_pen) : ElemPre{1.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    pen += o.e[h].pen;
  }
  if (loss_penalty != nullptr) {
    float v[4] = {pen, 0.0f, 0.0f, 0.0f};
    block_sum4(v, red);
    if (tid == 0) loss_penalty[0] = v[0];
  }
  return o;
}

// The update on the gradient g (w.r.t. the activated values) of elements tid and tid + 256.
__device__ __forceinline__ void opt_small_post(const OptPre& o, const OptPrefetch& pf, const float (&g)[2],
                                               float* __restrict__ raw, float* __restrict__ m1,
                                               float* __restrict__ m2, int M, float lr, float wd,
                                               float* __restrict__ act_out, _Float16* __restrict__ col_h_out) {
  const int n = 7 * M + 4;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = (int)threadIdx.x + 256 * h;
    if (i < n)
      optimizer_apply(i, o.e[h], g[h], pf.x[h], pf.a[h], pf.b[h], o.bias, lr, wd, M, raw, m1, m2, act_out,
                      col_h_out);
  }
}

__global__ __launch_bounds__(256) void rm_optimizer_small(float* __restrict__ raw, const float* __restrict__ gact,
                                                          float* __restrict__ m1, float* __restrict__ m2, int M,
                                                          int step, float lr, float wd, int with_pen,
                                                          float* __restrict__ loss_penalty, float* __restrict__ act_out,
                                                          _Float16* __restrict__ col_h_out,
                                                          rm_step_scalars* __restrict__ sdev) {
  const OptPrefetch pf = opt_prefetch(raw, m1, m2, M);
  if (sdev != nullptr) step = sdev->step;  // device step scalars (rm_bind_step_scalars)
  const int n = 7 * M + 4, i0 = (int)threadIdx.x;
  const float g[2] = {i0 < n ? gact[i0] : 0.0f, i0 + 256 < n ? gact[i0 + 256] : 0.0f};
  const OptPre o = opt_small_pre(pf, M, step, with_pen, loss_penalty);
  opt_small_post(o, pf, g, raw, m1, m2, M, lr, wd, act_out, col_h_out);
  if (sdev != nullptr) {  // every thread has read the step: the training step ends here
    __syncthreads();
    if (threadIdx.x == 0) {
      sdev->step += 1;
      sdev->index += 1;
    }
  }
}

// rm_optimizer_small's step inside the gradient reduction's last block (rm_reduce_partials,
// FinalArgs::raw): the same functions on the same values -- the gradient read with agent-scope
// loads after the hand-off -- so the same bits as the separate launch.
__device__ void fused_optimizer(const FinalArgs& f, int M) {
  const OptPrefetch pf = opt_prefetch(f.raw, f.m1, f.m2, M);
  const int step = f.sdev != nullptr ? f.sdev->step : f.step;
  const int n = 7 * M + 4, i0 = (int)threadIdx.x;
  float g[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = i0 + 256 * h;
    g[h] = i < n ? __hip_atomic_load(f.gc + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0f;
  }
  const OptPre o = opt_small_pre(pf, M, step, f.with_pen, f.loss_penalty);
  opt_small_post(o, pf, g, f.raw, f.m1, f.m2, M, f.lr, f.wd, f.act_out, f.col_h);
  if (f.sdev != nullptr) {  // every thread has read the step: the training step ends here
    __syncthreads();
    if (threadIdx.x == 0) {
      f.sdev->step += 1;
      f.sdev->index += 1;
    }
  }
}

// The end of a training step with device step scalars bound (multi-block optimizer path).
__global__ void rm_step_advance(rm_step_scalars* sdev) {
  if (threadIdx.x == 0) {
    sdev->step += 1;
    sdev->index += 1;
  }
}

__global__ void rm_sum_small(const float* __restrict__ parts, int n, float* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    float acc = 0.0f;
    for (int i = 0; i < n; ++i) acc += parts[i];
    out[0] = acc;
  }
}
