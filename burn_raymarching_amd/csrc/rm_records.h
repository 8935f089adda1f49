// rm_records.h -- the sphere-record buffer of a call: its layout (RecLayout), the readers' binding (Lds,
// bind_records) and the kernels that write it (rm_prep_kernel, rm_prep_finish, rm_origin_kernel). Included by
// rm_kernels.hip inside namespace rm, after KArgs and the matrix-core fragment helpers the record kernel needs.
#pragma once

// ---- sphere records: pair-interleaved, in global memory, read through scalar loads ----------
// rm_prep_kernel writes the buffer once per call; every kernel but the small-scene kernel reads it. In order:
//   1. eight planes of np = Mpad / 2 sphere pairs: P0 P1 P2 P3 S0 S1 W (16 B a pair), P4 (8 B a pair). Pair i
//      holds spheres (2i, 2i+1) so every sweep runs two spheres per v_pk_* instruction:
//        P0 = {-2cx0, -2cx1, -2cy0, -2cy1}   P1 = {-2cz0, -2cz1, |c0|^2, |c1|^2}
//        P2 = {k r0, k r1, r0, r1}           P3 = {red0, red1, green0, green1}   P4 = {blue0, blue1}
//        S0, S1 = P0, P1 scaled by k^2       W  = {2^(k r0), 2^(k r1), 2^(k (r0 - r_first)), 2^(k (r1 - r_first))}
//      (k = smooth_k log2 e). Every lane of a wave reads the same record at the same time, so the kernels read
//      them through the constant address space: s_load into SGPRs that feed the packed VALU ops as scalar operands
//      -- no LDS staging, no LDS broadcast traffic, and no limit on M (they stream through the scalar cache / L2).
//   2. the header (Hdr): {r_min, r_max, max |c_j - c_0|, R_soft (soft_radius), c_x, c_y, c_z, R} of the real
//      spheres ((c, R): their bounding sphere, scene_bound);
//   3. one partial header per rm_prep_kernel block (256 pairs each), folded by rm_prep_finish if more than one;
//   4. 16-byte aligned, the matrix-core tiles of the march (lse_mfma): At, per row block of 16 spheres 64
//      lanes x 16 B of A fragments, then Wt, per row block 32 floats {w(16), w_fixed(16)};
//   5. the tail (RecTail), of one size for every scene: the march's escape thresholds (write_bound); camera
//      mode's origin rows (write_origins), per view the first march step's D at the eye and a lower bound on the
//      eye's distance to the nearest sphere centre (the march's clamp-free proof, rho_lb in rm_ray_kernel); the
//      geometry of the call's escape lattice (Lat; write_bound, rm_tile_proof_kernel, bound_proof): {x, y, z of cell
//      centre 0, h, half-side, 1 / h, slack, 0} -- from the scene's bounding sphere, which only the record
//      kernel knows, so it lives here and not in KArgs.
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(4))) f4v* cf4_ptr;
typedef const __attribute__((address_space(4))) f2v* cf2_ptr;
typedef const __attribute__((address_space(4))) float* cf1_ptr;

struct Hdr { enum { kRmin = 0, kRmax, kSpread, kRsoft, kCx, kCy, kCz, kR, kCount }; };      // the header's fields
struct Lat { enum { kX0 = 0, kY0, kZ0, kH, kHalf, kInvH, kSlack, kZero, kCount }; };  // the lattice geometry's
constexpr int kEscTab = 64;
struct RecTail {
  // where the origin rows start, in floats from KArgs::origin: view v's entry is [row + v]
  static constexpr int kD0 = 0, kRhoLb = RM_MAX_VIEWS_PER_CALL;
  float esc[kEscTab], origin[2 * RM_MAX_VIEWS_PER_CALL], lat[Lat::kCount];
};

// The one place that knows the layout, for the kernels and for the host's buffer size: byte offsets of the
// sections from the buffer's start, for a scene of Mpad (padded) spheres.
struct RecLayout {
  enum Plane { kP0 = 0, kP1, kP2, kP3, kS0, kS1, kW, kP4 };
  int np;        // sphere pairs
  int launched;  // a record kernel's block count as its launch has it (gridDim.x, the host's argument); else 0
  __host__ __device__ constexpr explicit RecLayout(int Mpad, int launched = 0) : np(Mpad / 2), launched(launched) {}
  // blocks of rm_prep_kernel = partial headers; the host launches this many, so `launched` says the same
  __host__ __device__ constexpr int nprep() const { return launched ? launched : (np + 255) / 256; }
  // pair i of plane p < kP4 as an index into the buffer's float4s; the float4 at which P4's float2s start
  __host__ __device__ constexpr int pair(Plane p, int i) const { return (int)p * np + i; }
  __host__ __device__ constexpr size_t p4_first() const { return kP4 * (size_t)np; }
  __host__ __device__ constexpr size_t header() const { return (size_t)np * (7 * 16 + 8); }
  __host__ __device__ constexpr size_t partial(int b) const { return header() + (size_t)(1 + b) * Hdr::kCount * sizeof(float); }
  __host__ __device__ constexpr size_t at_after(int blocks) const { return (partial(blocks) + 15) & ~(size_t)15; }
  __host__ __device__ constexpr size_t at() const { return at_after(nprep()); }
  __host__ __device__ constexpr size_t wt() const { return at() + (size_t)np / 8 * 64 * 16; }  // np / 8 row blocks of 16 spheres
  // == wt() + np / 8 * 32 floats. One sum, the block count first: the per-ray kernels keep their instruction
  // order and registers only with the operations in this order (rm_ray.h's head comment; HISTORY.md §3)
  __host__ __device__ constexpr size_t tail() const {
    const int blocks = nprep();
    const size_t n = (size_t)np / 8;
    return at_after(blocks) + n * 64 * 16 + n * 32 * sizeof(float);
  }
  __host__ __device__ constexpr size_t esc() const { return tail() + offsetof(RecTail, esc); }
  __host__ __device__ constexpr size_t origin(int row) const { return tail() + offsetof(RecTail, origin) + row * sizeof(float); }
  __host__ __device__ constexpr size_t lattice() const { return tail() + offsetof(RecTail, lat); }
  __host__ __device__ constexpr size_t bytes() const { return tail() + sizeof(RecTail); }
  template <class T, class B>  // the section at byte offset `off` of the buffer at `rec` (T const for a const buffer)
  __host__ __device__ static T* at(B* rec, size_t off) { return (T*)((const char*)rec + off); }
};

// What the kernels rely on: the sections in this order without overlap, At 16-byte and the floats 4-byte aligned
constexpr bool rec_layout_ok(int Mpad) {
  const RecLayout l(Mpad);
  const size_t f = sizeof(float), v = RM_MAX_VIEWS_PER_CALL * f;
  return l.header() == l.p4_first() * 16 + (size_t)l.np * 8 && l.partial(0) == l.header() + Hdr::kCount * f &&
         l.at() >= l.partial(l.nprep()) && l.at() < l.partial(l.nprep()) + 16 && l.at() % 16 == 0 &&
         l.wt() == l.at() + (size_t)l.np * 128 && l.tail() == l.wt() + (size_t)l.np * 4 * f && l.esc() == l.tail() &&
         l.origin(RecTail::kD0) == l.esc() + kEscTab * f && l.origin(RecTail::kRhoLb) == l.origin(RecTail::kD0) + v &&
         l.lattice() == l.origin(RecTail::kRhoLb) + v && l.bytes() == l.lattice() + Lat::kCount * f &&
         l.header() % f == 0 && l.wt() % f == 0 && l.tail() % f == 0 && l.bytes() == l.tail() + sizeof(RecTail);
}
static_assert(RecLayout(512).nprep() == 1 && RecLayout(544).nprep() == 2 && RecLayout(544, 2).bytes() == RecLayout(544).bytes() &&
              rec_layout_ok(32) && rec_layout_ok(512) && rec_layout_ok(544) && rec_layout_ok(RM_MAX_SPHERES),
              "the record buffer: one record-kernel block per 256 pairs; the sections' order, alignment, size");

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

// The record pointers of a call, for every kernel that reads them (no LDS scratch: bind_lds adds it).
__device__ __forceinline__ Lds bind_records(const float4* rec_buf, int Mpad) {
  const RecLayout lay(Mpad);
  const int np = lay.np;
  Lds L{};
  L.P0 = (cf4_ptr)rec_buf;
  L.P1 = L.P0 + np;
  L.P2 = L.P1 + np;
  L.P3 = L.P2 + np;
  L.S0 = L.P3 + np;
  L.S1 = L.S0 + np;
  L.W = L.S1 + np;
  L.P4 = (cf2_ptr)(L.W + np);
  L.At = RecLayout::at<const uint4>(rec_buf, lay.at());
  L.Wt = reinterpret_cast<const float*>(L.At + (size_t)(np / 8) * 64);  // == lay.wt()
  return L;
}
// The header (Hdr) for a reader's scalar loads: the end of the bound planes (== header(), rec_layout_ok). Formed
// where it is read, as the other sections' addresses, not an Lds member (the per-ray kernels' registers: rm_ray.h).
__device__ __forceinline__ cf1_ptr rec_header(const Lds& bound, int Mpad) { return (cf1_ptr)(bound.P4 + RecLayout(Mpad).np); }

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
    dst[Hdr::kRmin] = red[0][0];
    dst[Hdr::kRmax] = red[1][0];
    dst[Hdr::kSpread] = red[2][0];
    dst[Hdr::kRsoft] = 0.0f;  // write_bound's
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

// The soft radius of the scene about c0 (Hdr::kRsoft; the escape proof's bound, bound_proof in
// rm_ray_kernel): R_soft = (1/k) ln sum_j exp(k (|c_j - c0| + r_j)), rounded up. Every sphere has
// |p - c_j| >= |p - c0| - |c_j - c0|, so exp(-k (|p - c_j| - r_j)) <= exp(-k |p - c0|)
// exp(k (|c_j - c0| + r_j)); summed over j, the soft-min D(p) >= |p - c0| - R_soft at every p (the
// padding spheres add 0 to D's sum in fp32, the clamp max(q, 1e-6) only raises D). R <= R_soft <=
// R + ln(M)/k: the ball bound |p - c0| - R - ln(M)/k charges every sphere as if it sat at the rim.
// In fp32, relative to R of scene_bound: v_j = (|c_j - c0| + r_j) (1 + 1e-5) + 1e-6 is scene_bound's
// own rounded-up term, so v_j <= R and every exponent is <= 0; the sum (a term's relative error
// below 2e-6 where it matters, at most M / 256 + 14 additions per chain) is taken 1e-5 up, the
// logarithm's 1e-7 and the division go into the final 1e-5 relative + 1e-6. scratch as scene_bound's.
__device__ __forceinline__ float soft_radius(const KArgs& a, float* scratch, int tid, const float c0[3], float R) {
  const int lane = tid & 63, wave = tid >> 6, nt = (int)blockDim.x, nw = nt >> 6;
  const float kappa = a.k * kLog2e;
  float s = 0.0f;
  for (int j = tid; j < a.M; j += nt) {
    const float dx = a.centers[3 * j] - c0[0], dy = a.centers[3 * j + 1] - c0[1], dz = a.centers[3 * j + 2] - c0[2];
    const float v = (fsqrt(dx * dx + dy * dy + dz * dz) + a.radius[j]) * (1.0f + 1e-5f) + 1e-6f;
    s += fexp2(kappa * fminf(v - R, 0.0f));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) scratch[8 * wave] = s;
  __syncthreads();
  float sum = scratch[0];
  for (int w = 1; w < nw; ++w) sum += scratch[8 * w];
  __syncthreads();  // scratch is reused by the caller
  // sum >= 1 up to rounding (the sphere that sets R has exponent ~0); never above the ball's slack
  const float rs = (R + flog2(fmaxf(sum, 1.0f) * (1.0f + 1e-5f)) / kappa) * (1.0f + 1e-5f) + 1e-6f;
  return fminf(rs, R + a.lse_slack);
}

// Hdr::kCx..kR = the bounding sphere (c, R) of scene_bound, for the march's escape test, and its
// distance thresholds T(n), n < kEscTab: a receding ray at distance d from c with n march steps
// left ends them at distance >= gone_d + R' from c if (1 - 1e-5) d >= T(n). Every step is at
// least g = d - R' long (R' = proof_rprime: the soft-min is >= the hard min - ln(M)/k, kMarchAbs
// covers the fp32 march; rm_proof.h) and keeps the ray receding, so one step takes d to at least
// F(d) = (1 - 1e-5) sqrt(d^2 + (d - R')^2); T(0) = gone_d + R' and T(n) = F^-1(T(n - 1)) =
// (R' + sqrt(2 y^2 - R'^2)) / 2 with y = T(n - 1) / (1 - 1e-5), rounded up. For n >= kEscTab the
// march uses T(kEscTab - 1) >= T(n).
__device__ void write_bound(const KArgs& a, float* hdr, RecTail* tail) {
  __shared__ float scratch[8 * 16];
  float c[3], R;
  scene_bound(a, scratch, threadIdx.x, c, R);
  const float rsoft = a.proof ? soft_radius(a, scratch, threadIdx.x, c, R)
                                                                    : R + a.lse_slack;
  if (threadIdx.x == 0) {
    hdr[Hdr::kRsoft] = rsoft;
    hdr[Hdr::kCx] = c[0];
    hdr[Hdr::kCy] = c[1];
    hdr[Hdr::kCz] = c[2];
    hdr[Hdr::kR] = R;
    if (a.lattice != nullptr) {
      // The escape lattice of this call (kLatticeN; rm_lattice_kernel fills it, rm_tile_proof_kernel or bound_proof reads it): the
      // cube of half-side R' + kLatticeMargin about c_0 in kLatticeN^3 cells of side h, cell i's centre at
      // -half + (i + 0.5) h per axis. The division is done here, once: the ray kernel multiplies by 1 / h.
      // slack: the per-ray lookup's half-diagonal allowance (the cell reader of rm_proof.h's ledger); the
      // tile proof takes actual distances and does not read it.
      const float half = proof_rprime(R, a.lse_slack) + kLatticeMargin;
      const float h = 2.0f * half / (float)kLatticeN;
      for (int k = 0; k < 3; ++k) tail->lat[Lat::kX0 + k] = (c[k] - half) + 0.5f * h;
      tail->lat[Lat::kH] = h;
      tail->lat[Lat::kHalf] = half;
      tail->lat[Lat::kInvH] = 1.0f / h;
      tail->lat[Lat::kSlack] = h * ((float)kLatticeHalfDiag * (1.0f + (float)kLatticeCellRel)) + (float)kLatticeKernelAbs;
      tail->lat[Lat::kZero] = 0.0f;
    }
  }
  if (threadIdx.x < kEscTab) {
    // f32 with a 1e-5 relative + 1e-6 absolute round-up per iteration (the f32 rounding of one
    // iteration is a few 1e-7): every T(n) stays above the exact inverse iterate. (R' rounded up
    // is conservative too: F^-1 grows with R' for y > R', which holds along the table.)
    float tv = INFINITY;
    if (a.gone_d > 0.0f) {
      const float rp = proof_rprime(R, a.lse_slack);
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
    tail->esc[threadIdx.x] = tv;
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
  const RecLayout lay(a.Mpad, (int)gridDim.x);
  const int np = lay.np;
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
    rec[lay.pair(RecLayout::kP0, ip)] = make_float4(gx[0], gx[1], gy[0], gy[1]);
    rec[lay.pair(RecLayout::kP1, ip)] = make_float4(gz[0], gz[1], cc[0], cc[1]);
    rec[lay.pair(RecLayout::kP2, ip)] = make_float4(kr[0], kr[1], rr[0], rr[1]);
    rec[lay.pair(RecLayout::kP3, ip)] = make_float4(cr[0], cr[1], cg[0], cg[1]);
    reinterpret_cast<float2*>(rec + lay.p4_first())[ip] = make_float2(cb[0], cb[1]);
    rec[lay.pair(RecLayout::kS0, ip)] = make_float4(k2 * gx[0], k2 * gx[1], k2 * gy[0], k2 * gy[1]);
    rec[lay.pair(RecLayout::kS1, ip)] = make_float4(k2 * gz[0], k2 * gz[1], k2 * cc[0], k2 * cc[1]);
    rec[lay.pair(RecLayout::kW, ip)] = make_float4(w[0], w[1], wf[0], wf[1]);
  }
  // matrix-core tiles of the march (lse_mfma)
  const int nrb = np / 8;
  uint4* At = RecLayout::at<uint4>(rec, lay.at());
  float* Wt = RecLayout::at<float>(rec, lay.wt());
  for (int e = blockIdx.x * nt + threadIdx.x; e < nrb * 64; e += gridDim.x * nt) At[e] = mfma_a_frag(a, e);
  for (int e = blockIdx.x * nt + threadIdx.x; e < nrb * 32; e += gridDim.x * nt) {
    const int j = mfma_w_sphere(e);
    const float krj = j < a.M ? kappa * a.radius[j] : 0.0f;
    Wt[e] = j >= a.M ? 0.0f : (mfma_w_fixed(e) ? fexp2(krj - kr_first) : fexp2(krj));
  }
  float* hdr = RecLayout::at<float>(rec, lay.header());
  header_reduce(rmin, rmax, spread, gridDim.x == 1 ? hdr : RecLayout::at<float>(rec, lay.partial(blockIdx.x)));
  if (gridDim.x == 1) write_bound(a, hdr, RecLayout::at<RecTail>(rec, lay.tail()));
}

__global__ __launch_bounds__(256) void rm_prep_finish(const KArgs a, float* __restrict__ hdr, float* __restrict__ esc,
                                                      int nprep) {
  float rmin = INFINITY, rmax = 0.0f, spread = 0.0f;
  const RecLayout lay(a.Mpad, nprep);
  for (int b = threadIdx.x; b < nprep; b += 256) {
    const float* h = RecLayout::at<const float>(hdr, lay.partial(b) - lay.header());
    rmin = fminf(rmin, h[Hdr::kRmin]);
    rmax = fmaxf(rmax, h[Hdr::kRmax]);
    spread = fmaxf(spread, h[Hdr::kSpread]);
  }
  header_reduce(rmin, rmax, spread, hdr);
  write_bound(a, hdr, reinterpret_cast<RecTail*>(esc));  // esc: the tail's first section
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
  const RecLayout lay(a.Mpad, nprep);
  const float* hdr = RecLayout::at<const float>(rec, lay.header());
  write_origins<SPLIT>(a, rec[lay.pair(RecLayout::kS0, 0)], rec[lay.pair(RecLayout::kS1, 0)], hdr[Hdr::kRmax],
                       hdr[Hdr::kSpread], RecLayout::at<const uint4>(rec, lay.at()), RecLayout::at<const float>(rec, lay.wt()),
                       a.origin, xch, blockIdx.x);
}
