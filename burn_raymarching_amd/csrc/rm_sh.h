// rm_sh.h -- view-dependent sphere colour: real spherical harmonics of degree 1 or 2 over each sphere's
// base colour (rm_render_diff_sh and its backward). Included by rm_kernels.hip inside namespace rm, after
// the sweeps it shares with the per-ray and the ray-gradient kernels and after rm_sdf.h (kSdfSums).
//
// B = (degree + 1)^2 - 1 coefficients per sphere and channel, sh[j][b][c]. For a ray of direction d,
// u = d / |d| (Y = 0 for d = 0) and the basis of 3D Gaussian splatting (sh_basis):
//   Y_1..3 = -C1 u.y, C1 u.z, -C1 u.x
//   Y_4..8 = C2[0] xy, C2[1] yz, C2[2] (2zz - xx - yy), C2[3] xz, C2[4] (xx - yy)
// the albedo of sphere j on that ray is a_jc = max(col_jc + sum_b sh[j][b][c] Y_b, 0), and the render is
// render_diff's (renderer_diff.rs:6-91) with the colours replaced by a, t and the normal detached:
//   mix_c = sum_j w_j a_jc, w = softmax(-csharp delta),   out = mix L mu.
// The march does not depend on colour: t comes from the existing kernels (saved, or replayed by the
// existing forward), and the two kernels here start from it, as rm_raygrad_kernel does:
//   rm_sh_shade_kernel<CAM, B>  one ray per lane: p_a, D(p_a), t_f, p_f (lse_point), the normal, the mask
//       soft-min and dmin (shade_normal_sweep), then one more sweep at p_f for the blend with a_j(u)
//       (sh_colour_sweep: delta from delta_pair_rsq, the shade sweep's bits, so dmin - delta <= 0 exactly);
//   rm_sh_grad_kernel<CAM, B>   one block per 256 rays. Pass 1, one ray per lane: that forward state, the
//       seeds (with g = dL/dout, gm = g L mu, mg = gm . mix, the mask's b_scale) and g_p = dL/dp_f by a
//       sweep of its own (g_t = g_p . d feeds the reconnect term through D(p_a)). The light and ambient
//       terms are summed over the block in a fixed order (wave_reduce8, then the waves in order). A ray
//       whose seeds are all zero (every escaped ray) is not swept. Pass 2, the roles turned around: the
//       seeded rays park their values in LDS in ray order {p_f, |p_f|^2 | dmin, b_scale, mg / Zw, g_t / s_A |
//       gm / Zw, m_A | p_a, |p_a|^2 | Y_b}, then a lane owns a sphere pair and runs over the parked rays in
//       order, both sweeps (at p_f and at p_a) in one loop:
//         dL/ddelta_j = -csharp w_j (gm . a_j - mg) + b_scale beta_j        (delta_j = rho_j - r_j at p_f)
//         dL/dc_j = -dL/ddelta_j e_j / rho_j - g_t alpha_j e'_j / rho'_j,  dL/dr_j = -dL/ddelta_j - g_t alpha_j
//         dL/dcol_jc = w_j gm_c [a_jc > 0],   dL/dsh[j][b][c] = w_j gm_c Y_b [a_jc > 0]
//       (alpha = softmax(-k d) at p_a, primes at p_a; no e / rho term from a sphere with q < 1e-6). The 7 + 3B
//       sums of a sphere sit in the lane's registers: one plain addition chain each, no cross-lane reduction.
//       Scenes of fewer than 256 pairs deal the rays out over G = 256 / lanes groups of lanes =
//       pow2ceil(pairs) >= 16 lanes (group g takes the parked rays g mod G, in order); the groups' sums are
//       added in group order through LDS, seven sums at a time. More than 256 pairs: one pass per 256 pairs.
// The block writes one partial record in the per-ray kernels' layout ([Mpad][8] | 8 scalars, scalar 7 the
// live flag; rm_reduce.h), which rm_reduce_partials and the finalize turn into rm_grads unchanged, and
// beside it [Mpad][3B] for the coefficients, which rm_sh_reduce_partials and rm_sh_finalize add in a fixed
// order (kShSegs segments of consecutive blocks, each a chain in block order, then the segments in order).
// No floating-point atomics: two calls give the same bits, whatever outputs are asked for.
//
// The coefficients reach the ray-per-lane sweeps as the records do: rm_sh_pack_kernel interleaves them per
// sphere pair ([pair][3B] float2, zeros past M) and the sweeps read them through the constant address
// space, so they stay in SGPRs (every lane of a wave is at the same pair).
#pragma once

constexpr int kShSegs = 64;  // block segments of the coefficient reduction

struct ShArgs {
  const f2v* shp;   // packed coefficients: [Mpad / 2][3B] float2, spheres (2i, 2i + 1)
  float* gsh_part;  // backward: one [Mpad][3B] record per block of the launch
};

__global__ __launch_bounds__(256) void rm_sh_pack_kernel(const float* __restrict__ sh, int M, int npairs, int cols,
                                                         float2* __restrict__ out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= npairs * cols) return;
  const int i = idx / cols, k = idx - i * cols;
  const int j0 = 2 * i, j1 = 2 * i + 1;
  out[idx] = make_float2(j0 < M ? sh[(long long)j0 * cols + k] : 0.0f, j1 < M ? sh[(long long)j1 * cols + k] : 0.0f);
}

// A ray's basis values travel as whole float4s in LDS (degree 1: Y_1..3 and a zero) and, in registers, as the
// splats the packed sweeps multiply with.
template <int B>
constexpr int kShY = (B + 3) / 4 * 4;

// Y_1..B of the ray direction d (not normalised by the caller). Contraction off: both kernels form the
// same bits, so the forward's and the backward's clamp decisions agree.
template <int B>
__device__ __forceinline__ void sh_basis(const float d[3], f2 (&Y)[kShY<B>]) {
#pragma clang fp contract(off)
  static_assert(B == 3 || B == 8, "degree 1 or 2");
  const float l2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  const float il = l2 > 0.0f ? 1.0f / sqrtf(l2) : 0.0f;
  const float x = d[0] * il, y = d[1] * il, z = d[2] * il;
  constexpr float C1 = 0.4886025119029199f;
  Y[0] = sp(-C1 * y);
  Y[1] = sp(C1 * z);
  Y[2] = sp(-C1 * x);
  if constexpr (B == 3) Y[3] = sp(0.0f);
  if constexpr (B == 8) {
    const float xx = x * x, yy = y * y, zz = z * z;
    Y[3] = sp(1.0925484305920792f * (x * y));
    Y[4] = sp(-1.0925484305920792f * (y * z));
    Y[5] = sp(0.31539156525252005f * ((2.0f * zz - xx) - yy));
    Y[6] = sp(-1.0925484305920792f * (x * z));
    Y[7] = sp(0.5462742152960396f * (xx - yy));
  }
}

// a_c = max(col_c + sum_b sh[b][c] Y_b, 0) for a sphere pair: one fused chain per channel in band order,
// the same in every sweep. shv(k): coefficient k = 3 b + c of the pair.
template <int B, class F>
__device__ __forceinline__ void sh_albedo(const f2 (&col)[3], F&& shv, const f2 (&Y)[kShY<B>], f2 (&a)[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    f2 acc = col[c];
#pragma unroll
    for (int b = 0; b < B; ++b) acc = fma2(shv(3 * b + c), Y[b], acc);
    a[c] = f2{fmaxf(acc.x, 0.0f), fmaxf(acc.y, 0.0f)};
  }
}

// The colour blend at p_f with a_j(u): Zw = sum_j 2^(c10l (dmin - delta_j)), C_c = sum_j the same a_jc.
// dmin: shade_normal_sweep's final minimum, delta: delta_pair_rsq's, so no exponent is positive.
template <int B>
__device__ __forceinline__ void sh_colour_sweep(const float p[3], const Lds& L, const f2v* shp_, int np, float c10l,
                                                float dmin, const f2 (&Y)[kShY<B>], float& Zw, float (&C)[3]) {
  const cf2_ptr shp = (cf2_ptr)shp_;
  const f2 PX = sp(p[0]), PY = sp(p[1]), PZ = sp(p[2]), PP = sp(psq(p)), CL = sp(c10l), DM = sp(dmin);
  f2 Z = sp(0.0f), Cc[3] = {sp(0.0f), sp(0.0f), sp(0.0f)};
#pragma unroll 1
  for (int i = 0; i < np; ++i) {
    const float4 C3 = L.p3(i);
    const float2 C4 = L.p4(i);
    f2 q, ir;
    const f2 dl = delta_pair_rsq<true>(PX, PY, PZ, PP, L.p0(i), L.p1(i), L.p2(i), q, ir);
    const f2 w = exp2v((DM - dl) * CL);
    const f2 col[3] = {lo(C3), hi(C3), f2{C4.x, C4.y}};
    f2 al[3];
    sh_albedo<B>(col, [&](int k) { const f2v v = shp[i * (3 * B) + k]; return f2{v.x, v.y}; }, Y, al);
    Z += w;
#pragma unroll
    for (int c = 0; c < 3; ++c) Cc[c] = fma2(w, al[c], Cc[c]);
  }
  Zw = Z.x + Z.y;
#pragma unroll
  for (int c = 0; c < 3; ++c) C[c] = Cc[c].x + Cc[c].y;
}

// The post-march forward state of one ray from its march distance t (renderer_diff.rs:28-90 with a_j(u)).
template <int B>
struct ShRay {
  float pa[3], mA, sA, tf, p[3], dmin, Zb, nrm[3], amb, sdot, Lgt, invZw, mix[3], mu;
  f2 Y[kShY<B>];  // splats
};
template <int B>
__device__ __forceinline__ void sh_forward(const KArgs& a, const Lds& L, const ShArgs& s, int np, const float o[3],
                                           const float d[3], float t, ShRay<B>& f) {
  const float kappa = a.k * kLog2e, nkappa = -kappa, inv_kappa = 1.0f / kappa, c10l = a.csharp * kLog2e;
#pragma unroll
  for (int k = 0; k < 3; ++k) f.pa[k] = fmaf(d[k], t, o[k]);
  f.mA = -INFINITY;
  f.sA = 0.0f;
  lse_point<true, kShiftMax>(f.pa, L, np, nkappa, f.mA, f.sA);
  const float Da = -(flog2(fmaxf(f.sA, 1e-8f)) + f.mA) * inv_kappa;
  f.tf = t + Da;
#pragma unroll
  for (int k = 0; k < 3; ++k) f.p[k] = fmaf(d[k], f.tf, o[k]);
  f.dmin = INFINITY;
  f2 Zw2 = sp(0.0f), Zb2 = sp(0.0f), C2[3] = {sp(0.0f), sp(0.0f), sp(0.0f)}, G2[3] = {sp(0.0f), sp(0.0f), sp(0.0f)};
  shade_normal_sweep<true>(f.p, L, np, c10l, kappa, f.dmin, Zw2, C2, Zb2, G2);
  f.Zb = Zb2.x + Zb2.y;
  const float te = 2.0f * a.eps * frcp(f.Zb);
  const float nx = te * (G2[0].x + G2[0].y), ny = te * (G2[1].x + G2[1].y), nz = te * (G2[2].x + G2[2].y);
  const float inv_len = frsq(fmaf(nz, nz, fmaf(ny, ny, fmaf(nx, nx, 1e-6f))));
  f.nrm[0] = nx * inv_len;
  f.nrm[1] = ny * inv_len;
  f.nrm[2] = nz * inv_len;
  float ldn[3];
  light_unit(a.light_dir, ldn);
  f.amb = a.ambient[0];
  f.sdot = fmaf(f.nrm[2], ldn[2], fmaf(f.nrm[1], ldn[1], f.nrm[0] * ldn[0]));
  f.Lgt = fmaf(fmaxf(f.sdot, 0.0f), 1.0f - f.amb, f.amb);
  const float Df = f.dmin - flog2(fmaxf(f.Zb, 1e-8f)) * inv_kappa;
  f.mu = frcp(1.0f + fexp2(a.msharp * kLog2e * Df));  // sigmoid(-msharp * D)
  sh_basis<B>(d, f.Y);
  float Zw, C[3];
  sh_colour_sweep<B>(f.p, L, s.shp, np, c10l, f.dmin, f.Y, Zw, C);
  f.invZw = frcp(Zw);
#pragma unroll
  for (int c = 0; c < 3; ++c) f.mix[c] = C[c] * f.invZw;
}

// The ray of lane `tid` of block blockIdx.x of a launch: ray a.ray_begin + 256 blockIdx.x + tid of the call
// (camera mode: in setup_ray's launch order). A lane past the launch takes the launch's first ray and
// writes nothing.
template <bool CAM>
__device__ __forceinline__ bool sh_ray(const KArgs& a, long long& ri, float o[3], float d[3]) {
  const long long li = (long long)blockIdx.x * kBlock + threadIdx.x;
  const bool valid = li < a.n_rays;
  ri = a.ray_begin + (valid ? li : 0);
  int view;
  setup_ray<CAM>(a, ri, o, d, view);
  return valid;
}

template <bool CAM, int B>
__global__ __launch_bounds__(kBlock, kMinWavesPerSimd) void rm_sh_shade_kernel(const KArgs a, const ShArgs s) {
  const Lds L = bind_records(a.rec_buf, a.Mpad);
  long long ri;
  float o[3], d[3];
  const bool valid = sh_ray<CAM>(a, ri, o, d);
  ShRay<B> f;
  sh_forward<B>(a, L, s, a.Mpad / 2, o, d, a.t_in[ri], f);
  if (!valid) return;
  const float scale = f.Lgt * f.mu;
#pragma unroll
  for (int c = 0; c < 3; ++c) a.out[3 * ri + c] = f.mix[c] * scale;
}

// Register budget: a pair-owning lane holds 2 (7 + 3B) sums and the pair's 6B coefficients next to the sweep's
// temporaries. Degree 1 spilled 17 VGPRs at 4 waves per SIMD (128 VGPRs) and kept a 20-byte private segment at
// 3 (160 of 168 VGPRs); degree 2 holds 62 sums and 48 coefficient registers. Both take the budget of 2 waves
// per SIMD: no vector spill and no private segment at either, 159 / 230 VGPRs (tools/resource_usage.py). Every
// instance sits at the SGPR limit (the ray-per-lane sweeps hold up to 64 record SGPRs), so pass 1's wave skip is
// a trip count: as a branch around the g_p sweep it left the array-mode degree-1 instance a 20-byte frame (a
// 128-bit scalar spill slot that register allocation opened and then no longer used, and the scavenging slot
// that comes with any frame), and with it a scratch set-up on every dispatch.
template <bool CAM, int B>
__global__ __launch_bounds__(kBlock, 2) void rm_sh_grad_kernel(const KArgs a, const ShArgs s) {
  static_assert(kBlock == 256, "256 rays, up to 256 sphere pairs a pass");
  constexpr int NF4 = 4 + (B + 3) / 4;  // float4s a ray parks
  constexpr int NS = 7 + 3 * B;         // sums of a sphere (f2: of a pair)
  __shared__ float4 park[kBlock * NF4];
  __shared__ float comb[kSdfSums * kBlock];
  __shared__ float wscal[kWaves][8];
  __shared__ int wcnt[kWaves];
  const Lds L = bind_records(a.rec_buf, a.Mpad);
  const int np = a.Mpad / 2, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float kappa = a.k * kLog2e, nkappa = -kappa, c10l = a.csharp * kLog2e;

  // ---- pass 1: one ray per lane
  long long ri;
  float o[3], d[3];
  const bool valid = sh_ray<CAM>(a, ri, o, d);
  const float dx = d[0], dy = d[1], dz = d[2];  // for g_t, after the sweeps
  const float t = a.t_in[ri];
  float g[3] = {0.0f, 0.0f, 0.0f};
  if (valid) {
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = a.gout[3 * ri + c];
  }
  ShRay<B> f;
  sh_forward<B>(a, L, s, np, o, d, t, f);

  // the seeds (out = mix L mu), as the per-ray kernel forms them
  const float scale = f.Lgt * f.mu;
  const float gdotm = fmaf(g[2], f.mix[2], fmaf(g[1], f.mix[1], g[0] * f.mix[0]));
  const float gm[3] = {g[0] * scale, g[1] * scale, g[2] * scale};
  const float gL = gdotm * f.mu, gmu = gdotm * f.Lgt;
  const float dif = fmaxf(f.sdot, 0.0f);
  const float gs = f.sdot >= 0.0f ? gL * (1.0f - f.amb) : 0.0f;  // clamp_min passes at x >= min
  const float cmu = gmu * f.mu * (1.0f - f.mu) * (-a.msharp);
  const float mg = fmaf(f.mix[2], gm[2], fmaf(f.mix[1], gm[1], f.mix[0] * gm[0]));
  const float b_scale = cmu * frcp(f.Zb);
  const bool seeded = valid && (gm[0] != 0.0f || gm[1] != 0.0f || gm[2] != 0.0f || b_scale != 0.0f);

  // the block's scalars (light before the projection, ambient) in a fixed order, and its seeded rays
  {
    const float vals[8] = {gs * f.nrm[0], gs * f.nrm[1], gs * f.nrm[2], gL * (1.0f - dif), 0.0f, 0.0f, 0.0f, 0.0f};
    const float red = wave_reduce8(vals, lane);
    if ((lane & 7) == 7) wscal[wave][lane >> 3] = red;
  }
  const unsigned long long sm = __ballot(seeded);
  if (lane == 0) wcnt[wave] = __popcll(sm);
  __syncthreads();
  int first = 0;
  for (int w = 0; w < wave; ++w) first += wcnt[w];
  const int ns = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
  float* prow = a.partials + (long long)blockIdx.x * a.rec;
  if (tid < 8) {
    float acc = wscal[0][tid];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) acc += wscal[w][tid];
    prow[(long long)a.Mpad * 8 + tid] = tid == 7 ? (ns > 0 ? 1.0f : 0.0f) : acc;
  }
  if (ns == 0) return;  // no ray of the block has a seed: live flag 0, the columns are not read

  // g_p = sum_j dL/ddelta_j (p_f - c_j) / rho_j, then g_t = g_p . d (rm_raygrad_kernel's sweep 1 with a_j)
  const float gmz[3] = {gm[0] * f.invZw, gm[1] * f.invZw, gm[2] * f.invZw}, mgz = mg * f.invZw;
  float gt = 0.0f;
  const int npg = sm != 0ull ? np : 0;  // a wave without a seeded ray sweeps nothing (a trip count, not a branch)
  {
    const cf2_ptr shp = (cf2_ptr)s.shp;
    const f2 PX = sp(f.p[0]), PY = sp(f.p[1]), PZ = sp(f.p[2]), PP = sp(psq(f.p)), CL = sp(c10l), KA = sp(kappa),
             DM = sp(f.dmin), BS = sp(b_scale), G0 = sp(gmz[0]), G1 = sp(gmz[1]), G2s = sp(gmz[2]), MG = sp(mgz),
             NCS = sp(-a.csharp), HALF = sp(0.5f);
    f2 GP[3] = {sp(0.0f), sp(0.0f), sp(0.0f)};
#pragma unroll 1
    for (int i = 0; i < npg; ++i) {
      const float4 A = L.p0(i), Bq = L.p1(i), C3 = L.p3(i);
      const float2 C4 = L.p4(i);
      f2 q, ir;
      const f2 dl = delta_pair_rsq<true>(PX, PY, PZ, PP, A, Bq, L.p2(i), q, ir);
      const f2 dd = DM - dl;  // <= 0 exactly
      const f2 w = exp2v(dd * CL);
      const f2 bt = exp2v(dd * KA) * BS;
      const f2 col[3] = {lo(C3), hi(C3), f2{C4.x, C4.y}};
      f2 al[3];
      sh_albedo<B>(col, [&](int k) { const f2v v = shp[i * (3 * B) + k]; return f2{v.x, v.y}; }, f.Y, al);
      const f2 cg = fma2(al[2], G2s, fma2(al[1], G1, al[0] * G0));
      const f2 gd = fma2(w * NCS, cg - MG, bt);
      f2 gu = gd * ir;
      gu.x = q.x >= 1e-6f ? gu.x : 0.0f;  // clamp_min(1e-6) gate
      gu.y = q.y >= 1e-6f ? gu.y : 0.0f;
      GP[0] = fma2(gu, fma2(HALF, lo(A), PX), GP[0]);
      GP[1] = fma2(gu, fma2(HALF, hi(A), PY), GP[1]);
      GP[2] = fma2(gu, fma2(HALF, lo(Bq), PZ), GP[2]);
    }
    const float gp[3] = {GP[0].x + GP[0].y, GP[1].x + GP[1].y, GP[2].x + GP[2].y};
    gt = fmaf(gp[2], dz, fmaf(gp[1], dy, gp[0] * dx));
  }

  // ---- pass 2: the seeded rays park in ray order, a lane owns a sphere pair
  if (seeded) {
    float4* slot = park + (first + __popcll(sm & ((1ull << lane) - 1ull))) * NF4;
    slot[0] = make_float4(f.p[0], f.p[1], f.p[2], psq(f.p));
    slot[1] = make_float4(f.dmin, b_scale, mgz, gt * frcp(f.sA));
    slot[2] = make_float4(gmz[0], gmz[1], gmz[2], f.mA);
    slot[3] = make_float4(f.pa[0], f.pa[1], f.pa[2], psq(f.pa));
    slot[4] = make_float4(f.Y[0].x, f.Y[1].x, f.Y[2].x, f.Y[3].x);
    if constexpr (B == 8) slot[5] = make_float4(f.Y[4].x, f.Y[5].x, f.Y[6].x, f.Y[7].x);
  }
  __syncthreads();
  int lanes = 16;  // of a group: pow2ceil(pairs), 16 ... 256
  while (lanes < np && lanes < kBlock) lanes *= 2;
  const int groups = kBlock / lanes, li = tid & (lanes - 1), grp = tid / lanes;
  float* psh = s.gsh_part + (long long)blockIdx.x * a.Mpad * (3 * B);
  const float2* P4 = reinterpret_cast<const float2*>(a.rec_buf + RecLayout(a.Mpad).p4_first());
  const float2* shg = reinterpret_cast<const float2*>(s.shp);
  const f2 HALF = sp(0.5f), KA = sp(kappa), CL = sp(c10l), NCS = sp(-a.csharp), NK = sp(nkappa);
  for (int base = 0; base < np; base += kBlock) {
    const int ip = base + li;
    const bool own = ip < np;
    const int ic = own ? ip : np - 1;
    const RecLayout lay(a.Mpad);
    const float4 P0 = a.rec_buf[lay.pair(RecLayout::kP0, ic)], P1 = a.rec_buf[lay.pair(RecLayout::kP1, ic)],
                 R = a.rec_buf[lay.pair(RecLayout::kP2, ic)], C3 = a.rec_buf[lay.pair(RecLayout::kP3, ic)];
    const float2 C4 = P4[ic];
    const f2 col[3] = {lo(C3), hi(C3), f2{C4.x, C4.y}}, KR = lo(R);
    f2 shv[3 * B];
#pragma unroll
    for (int k = 0; k < 3 * B; ++k) {
      const float2 v = shg[(long long)ic * (3 * B) + k];
      shv[k] = f2{v.x, v.y};
    }
    f2 S[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) S[k] = sp(0.0f);
#pragma unroll 1
    for (int r = grp; r < ns; r += groups) {
      const float4* v = park + r * NF4;
      const float4 v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3], v4 = v[4];
      f2 Y[kShY<B>];
      Y[0] = sp(v4.x);
      Y[1] = sp(v4.y);
      Y[2] = sp(v4.z);
      Y[3] = sp(v4.w);
      if constexpr (B == 8) {
        const float4 v5 = v[5];
        Y[4] = sp(v5.x);
        Y[5] = sp(v5.y);
        Y[6] = sp(v5.z);
        Y[7] = sp(v5.w);
      }
      {  // at p_f: the colour softmax and the mask soft-min
        const f2 PX = sp(v0.x), PY = sp(v0.y), PZ = sp(v0.z);
        f2 q, ir;
        const f2 dl = delta_pair_rsq<true>(PX, PY, PZ, sp(v0.w), P0, P1, R, q, ir);  // bitwise pass 1's
        const f2 dd = sp(v1.x) - dl;                                                  // <= 0 exactly
        const f2 w = exp2v(dd * CL);
        const f2 bt = exp2v(dd * KA) * sp(v1.y);
        f2 al[3];
        sh_albedo<B>(col, [&](int k) { return shv[k]; }, Y, al);
        const f2 cg = fma2(al[2], sp(v2.z), fma2(al[1], sp(v2.y), al[0] * sp(v2.x)));
        const f2 gd = fma2(w * NCS, cg - sp(v1.z), bt);
        f2 gu = gd * ir;
        gu.x = q.x >= 1e-6f ? gu.x : 0.0f;
        gu.y = q.y >= 1e-6f ? gu.y : 0.0f;
        S[0] = S[0] - gu * fma2(HALF, lo(P0), PX);
        S[1] = S[1] - gu * fma2(HALF, hi(P0), PY);
        S[2] = S[2] - gu * fma2(HALF, lo(P1), PZ);
        S[3] = S[3] - gd;
        const float gmc[3] = {v2.x, v2.y, v2.z};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          f2 wg = w * sp(gmc[c]);
          wg.x = al[c].x > 0.0f ? wg.x : 0.0f;  // the clamp's indicator
          wg.y = al[c].y > 0.0f ? wg.y : 0.0f;
          S[4 + c] += wg;
#pragma unroll
          for (int b = 0; b < B; ++b) S[7 + 3 * b + c] = fma2(wg, Y[b], S[7 + 3 * b + c]);
        }
      }
      {  // at p_a: t_f = t + D(p_a)
        const f2 PX = sp(v3.x), PY = sp(v3.y), PZ = sp(v3.z);
        const f2 qraw = qpair(PX, PY, PZ, sp(v3.w), P0, P1);  // bitwise lse_point's q
        const f2 q = clamp_q(qraw);
        const f2 ir = rsq2(q);
        const f2 h = exp2v(fma2(q * ir, NK, KR) - sp(v2.w)) * sp(v1.w);  // v - mA <= 0 exactly
        f2 hu = h * ir;
        hu.x = qraw.x >= 1e-6f ? hu.x : 0.0f;
        hu.y = qraw.y >= 1e-6f ? hu.y : 0.0f;
        S[0] = S[0] - hu * fma2(HALF, lo(P0), PX);
        S[1] = S[1] - hu * fma2(HALF, hi(P0), PY);
        S[2] = S[2] - hu * fma2(HALF, lo(P1), PZ);
        S[3] = S[3] - h;
      }
    }
    // the groups' sums, seven at a time, added in group order by the first group's lanes
#pragma unroll
    for (int c0 = 0; c0 < NS; c0 += 7) {
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        if (c0 + k < NS) {
          comb[(2 * k) * kBlock + tid] = S[c0 + k].x;
          comb[(2 * k + 1) * kBlock + tid] = S[c0 + k].y;
        }
      }
      __syncthreads();
      if (grp == 0 && own) {
#pragma unroll
        for (int k = 0; k < 7; ++k) {
          if (c0 + k < NS) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              float acc = comb[(2 * k + h) * kBlock + li];
              for (int gi = 1; gi < groups; ++gi) acc += comb[(2 * k + h) * kBlock + gi * lanes + li];
              const long long j = 2 * (long long)ip + h;  // the sphere
              if (c0 + k < 7) prow[j * 8 + (c0 + k)] = acc;
              else psh[j * (3 * B) + (c0 + k - 7)] = acc;
            }
          }
        }
      }
      __syncthreads();  // comb is free for the next seven
    }
    if (grp == 0 && own) {
      prow[(2 * (long long)ip) * 8 + 7] = 0.0f;
      prow[(2 * (long long)ip + 1) * 8 + 7] = 0.0f;
    }
  }
}

// ---- the coefficient gradient's cross-block reduction (fixed order => deterministic) ---------------------
// P: the launch's [nblocks][cols] coefficient records; live: the live flag of block b at live[b * rec]
// (scalar 7 of the main partial record). Grid (column blocks x kShSegs): S[seg][col] = the segment's live
// rows added in block order, eight loads in flight.
__global__ __launch_bounds__(256) void rm_sh_reduce_partials(const float* __restrict__ P, int cols,
                                                             const float* __restrict__ live, long long rec, int nblocks,
                                                             int seg_len, float* __restrict__ S) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= cols) return;
  const int b0 = blockIdx.y * seg_len, b1 = min(b0 + seg_len, nblocks);
  float acc = 0.0f;
  for (int b = b0; b < b1; b += kReduceBatch) {
    float v[kReduceBatch];
#pragma unroll
    for (int u = 0; u < kReduceBatch; ++u) {
      const int bb = min(b + u, b1 - 1);
      const bool take = b + u < b1 && live[(long long)bb * rec] != 0.0f;
      v[u] = take ? P[(long long)bb * cols + col] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < kReduceBatch; ++u) acc += v[u];
  }
  S[(long long)blockIdx.y * cols + col] = acc;
}

// grad_sh[col] (+)= the kShSegs segment sums in order; cols: M * 3B (the padding spheres' columns are not
// read), stride: Mpad * 3B.
__global__ __launch_bounds__(256) void rm_sh_finalize(const float* __restrict__ S, int stride, int cols,
                                                      float* __restrict__ gsh, int accumulate) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= cols) return;
  float acc = 0.0f;
  for (int sg = 0; sg < kShSegs; ++sg) acc += S[(long long)sg * stride + col];
  gsh[col] = accumulate ? gsh[col] + acc : acc;
}
