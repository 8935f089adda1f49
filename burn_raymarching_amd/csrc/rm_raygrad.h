// rm_raygrad.h -- the ray / camera-pose gradient of render_diff: rm_raygrad_kernel<CAM> and its
// per-view finish (rm_render_diff_backward_rays, rm_render_diff_backward_cameras). Included by
// rm_kernels.hip inside namespace rm, after the sweeps it shares with the per-ray kernel.
//
// The reference's graph (renderer_diff.rs:6-91) with t the detached march distance:
//   p_a = o + d t,  t_f = t + D(p_a),  p_f = o + d t_f,  out = mix(p_f) L mu(p_f)   (normal detached)
// so with g_p = dL/dp_f (backward sweep 1 at p_f: colour softmax + mask soft-min), g_t = g_p . d and
// g_pa = g_t grad D(p_a) (backward sweep 2 at p_a):
//   dL/do = g_p + g_pa          dL/dd = t_f g_p + t g_pa
// One ray per lane, no per-sphere output: the sweeps are those of the per-ray kernel's backward
// (one ray per lane form) with the per-ray sums kept and the per-sphere terms dropped, so there are
// no transposed sweeps, no partial records and no cross-block sphere reduction. Distances come from
// the same fp32 operations and operands as the forward sweeps (lse_point, delta_pair_rsq, qpair):
// dmin - delta <= 0 and v - mA <= 0 hold exactly. The sweeps always apply max(q, 1e-6) (the clamp
// is a no-op where the per-ray kernel proves it away, so the results are the same).
//
// CAM: the rays of a view all share eye / right / up / forward / half_h (camera.rs:41-79):
//   raw = r_scale right + u_scale up + forward, d = raw / |raw|, g_raw = (g_d - d (d . g_d)) / |raw|
// and a view's gradient needs 13 sums over its rays: sum g_o (3), sum g_raw (3), sum r_scale g_raw
// (3), sum u_scale g_raw (3), sum (u aspect right + v up) . g_raw (1). Every block belongs to one
// view (grid: blocks per view x views); it reduces the 13 sums in a fixed lane / wave order into one
// partial row, and rm_raygrad_finish adds a view's rows in block order and applies the 13 -> 7
// tail through up = right x forward, right = normalize(forward x (0,1,0)), forward =
// normalize(target - eye) and half_h = tan(fov_deg pi / 360). No floating-point atomics.
#pragma once

constexpr int kRgCols = 16;  // a partial row: the 13 sums padded to 64 bytes

struct RayGradArgs {
  float* g_org;  // array mode, nullable: [N,3]
  float* g_dir;  // array mode, nullable: [N,3]
  int accumulate;
  float* partial;  // CAM: [views][blocks per view][kRgCols]
};

struct RayGradCams {
  rm_camera c[RM_MAX_VIEWS_PER_CALL];
};

// camera.rs:58-75 up to the normalisation, with camera_ray's own operations: the pixel's
// r_scale / u_scale and |raw| (camera_ray returns only raw / |raw|).
__device__ __forceinline__ void camera_raw(const CamBasis& c, int x, int y, int W, int H, float& rs, float& us,
                                           float& len) {
#pragma clang fp contract(off)
  const float u = ((float)x / (float)W) * 2.0f - 1.0f;
  const float v = -(((float)y / (float)H) * 2.0f - 1.0f);
  rs = u * c.half_w;
  us = v * c.half_h;
  const float dx = c.right[0] * rs + c.up[0] * us + c.fwd[0];
  const float dy = c.right[1] * rs + c.up[1] * us + c.fwd[1];
  const float dz = c.right[2] * rs + c.up[2] * us + c.fwd[2];
  len = (float)__builtin_sqrt((double)(dx * dx + dy * dy + dz * dz));
}

template <bool CAM>
__global__ __launch_bounds__(kBlock, kMinWavesPerSimd) void rm_raygrad_kernel(const KArgs a, const RayGradArgs r) {
  __shared__ float red[kWaves][kRgCols];
  const Lds L = bind_records(a.rec_buf, a.Mpad);
  const int np = a.Mpad / 2;

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long npix = (long long)a.width * a.height;
  bool valid;
  long long ri;
  if constexpr (CAM) {
    const long long pix = (long long)blockIdx.x * kBlock + tid;
    valid = pix < npix;
    ri = (long long)blockIdx.y * npix + (valid ? pix : 0);
  } else {
    const long long li = (long long)blockIdx.x * kBlock + tid;
    valid = li < a.n_rays;
    ri = a.ray_begin + (valid ? li : 0);
  }
  float o[3], d[3];
  int view;
  setup_ray<CAM>(a, ri, o, d, view);  // ri: now the ray's row in the [N,3] tensors

  const float kappa = a.k * kLog2e, nkappa = -kappa, inv_kappa = 1.0f / kappa, c10l = a.csharp * kLog2e;
  const float t = a.t_in[ri];
  float g[3] = {0.0f, 0.0f, 0.0f};
  if (valid) {
    g[0] = a.gout[3 * ri];
    g[1] = a.gout[3 * ri + 1];
    g[2] = a.gout[3 * ri + 2];
  }

  // ---- forward state at p_a and p_f (renderer_diff.rs:28-90), as the per-ray kernel forms it
  const float pa[3] = {fmaf(d[0], t, o[0]), fmaf(d[1], t, o[1]), fmaf(d[2], t, o[2])};
  float mA = -INFINITY, sA = 0.0f;
  lse_point<true, kShiftMax>(pa, L, np, nkappa, mA, sA);
  const float Da = -(flog2(fmaxf(sA, 1e-8f)) + mA) * inv_kappa;
  const float tf = t + Da;
  const float p[3] = {fmaf(d[0], tf, o[0]), fmaf(d[1], tf, o[1]), fmaf(d[2], tf, o[2])};
  float dmin = INFINITY;
  f2 Zw2 = sp(0.0f), Zb2 = sp(0.0f), C2[3] = {sp(0.0f), sp(0.0f), sp(0.0f)}, G2[3] = {sp(0.0f), sp(0.0f), sp(0.0f)};
  shade_normal_sweep<true>(p, L, np, c10l, kappa, dmin, Zw2, C2, Zb2, G2);
  const float te = 2.0f * a.eps * frcp(Zb2.x + Zb2.y);
  const float nx = te * (G2[0].x + G2[0].y), ny = te * (G2[1].x + G2[1].y), nz = te * (G2[2].x + G2[2].y);
  const float inv_len = frsq(fmaf(nz, nz, fmaf(ny, ny, fmaf(nx, nx, 1e-6f))));
  const float nrm[3] = {nx * inv_len, ny * inv_len, nz * inv_len};
  float ldn[3];
  light_unit(a.light_dir, ldn);
  const float amb = a.ambient[0];
  const float sdot = fmaf(nrm[2], ldn[2], fmaf(nrm[1], ldn[1], nrm[0] * ldn[0]));
  const float Lgt = fmaf(fmaxf(sdot, 0.0f), 1.0f - amb, amb);
  const float Zw = Zw2.x + Zw2.y, Zb = Zb2.x + Zb2.y;
  const float Df = dmin - flog2(fmaxf(Zb, 1e-8f)) * inv_kappa;
  const float invZw = frcp(Zw);
  const float mix[3] = {(C2[0].x + C2[0].y) * invZw, (C2[1].x + C2[1].y) * invZw, (C2[2].x + C2[2].y) * invZw};
  const float mu = frcp(1.0f + fexp2(a.msharp * kLog2e * Df));  // sigmoid(-msharp * D)

  // ---- backward seeds (out = mix * L * mu); the light and ambient terms belong to the scene
  const float scale = Lgt * mu;
  const float gdotm = fmaf(g[2], mix[2], fmaf(g[1], mix[1], g[0] * mix[0]));
  const float gm[3] = {g[0] * scale, g[1] * scale, g[2] * scale};
  const float cmu = gdotm * Lgt * mu * (1.0f - mu) * (-a.msharp);
  const float mg = fmaf(mix[2], gm[2], fmaf(mix[1], gm[1], mix[0] * gm[0]));
  const float b_scale = cmu * frcp(Zb);
  // a ray whose seeds are all zero (every escaped ray: mu = 0) has exact zero gradients: not swept
  const bool seeded = valid && (gm[0] != 0.0f || gm[1] != 0.0f || gm[2] != 0.0f || b_scale != 0.0f);

  float gp[3] = {0.0f, 0.0f, 0.0f}, ga[3] = {0.0f, 0.0f, 0.0f};
  if (__any(seeded)) {
    // ---- sweep 1 at p_f: g_p = sum_j gdl_j (p_f - c_j) / rho_j
    f2 GP[3] = {sp(0.0f), sp(0.0f), sp(0.0f)};
    {
      const f2 PX = sp(p[0]), PY = sp(p[1]), PZ = sp(p[2]), PP = sp(psq(p)), CL = sp(c10l), KA = sp(kappa),
               DM = sp(dmin), IZ = sp(invZw), BS = sp(b_scale), G0 = sp(gm[0]), G1 = sp(gm[1]), G2s = sp(gm[2]),
               MG = sp(mg), NCS = sp(-a.csharp), HALF = sp(0.5f);
      for (int i0 = 0; i0 < np; i0 += 4) {
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
          const int i = i0 + ii;
          const float4 A = L.p0(i), B = L.p1(i), R = L.p2(i), C3 = L.p3(i);
          const float2 C4 = L.p4(i);
          f2 q, ir;
          const f2 dl = delta_pair_rsq<true>(PX, PY, PZ, PP, A, B, R, q, ir);  // bitwise the shade sweep's
          const f2 dd = DM - dl;  // <= 0 exactly
          const f2 w = exp2v(dd * CL) * IZ;
          const f2 bt = exp2v(dd * KA) * BS;
          const f2 cg = fma2(f2{C4.x, C4.y}, G2s, fma2(hi(C3), G1, lo(C3) * G0));
          const f2 gd = fma2(w * NCS, cg - MG, bt);
          f2 gu = gd * ir;
          gu.x = q.x >= 1e-6f ? gu.x : 0.0f;  // clamp_min(1e-6) gate
          gu.y = q.y >= 1e-6f ? gu.y : 0.0f;
          GP[0] = fma2(gu, fma2(HALF, lo(A), PX), GP[0]);
          GP[1] = fma2(gu, fma2(HALF, hi(A), PY), GP[1]);
          GP[2] = fma2(gu, fma2(HALF, lo(B), PZ), GP[2]);
        }
      }
    }
    gp[0] = seeded ? GP[0].x + GP[0].y : 0.0f;
    gp[1] = seeded ? GP[1].x + GP[1].y : 0.0f;
    gp[2] = seeded ? GP[2].x + GP[2].y : 0.0f;
    // ---- sweep 2 at p_a: t_f = t + D(p_a) -> g_pa = g_t sum_j alpha_j (p_a - c_j) / rho_j
    const float gt = fmaf(gp[2], d[2], fmaf(gp[1], d[1], gp[0] * d[0]));
    if (__any(gt != 0.0f)) {
      f2 GA[3] = {sp(0.0f), sp(0.0f), sp(0.0f)};
      const f2 PX = sp(pa[0]), PY = sp(pa[1]), PZ = sp(pa[2]), PP = sp(psq(pa)), NK = sp(nkappa), MA = sp(mA),
               HS = sp(gt * frcp(sA)), HALF = sp(0.5f);
      for (int i0 = 0; i0 < np; i0 += 4) {
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
          const int i = i0 + ii;
          const float4 A = L.p0(i), B = L.p1(i);
          const float2 K = L.kr(i);
          const f2 qraw = qpair(PX, PY, PZ, PP, A, B);  // bitwise the reconnect sweep's q
          const f2 q = clamp_q(qraw);
          const f2 ir = rsq2(q);  // rho = q rsq(q) as in lse_point, 1/rho = rsq(q)
          const f2 h = exp2v(fma2(q * ir, NK, f2{K.x, K.y}) - MA) * HS;  // v - mA <= 0 exactly
          f2 hu = h * ir;
          hu.x = qraw.x >= 1e-6f ? hu.x : 0.0f;
          hu.y = qraw.y >= 1e-6f ? hu.y : 0.0f;
          GA[0] = fma2(hu, fma2(HALF, lo(A), PX), GA[0]);
          GA[1] = fma2(hu, fma2(HALF, hi(A), PY), GA[1]);
          GA[2] = fma2(hu, fma2(HALF, lo(B), PZ), GA[2]);
        }
      }
      const bool on = seeded && gt != 0.0f;
      ga[0] = on ? GA[0].x + GA[0].y : 0.0f;
      ga[1] = on ? GA[1].x + GA[1].y : 0.0f;
      ga[2] = on ? GA[2].x + GA[2].y : 0.0f;
    }
  }
  // an unseeded ray: gp = ga = 0, so both gradients are exact zeros whatever t is
  const float go[3] = {gp[0] + ga[0], gp[1] + ga[1], gp[2] + ga[2]};
  const float gd3[3] = {seeded ? fmaf(tf, gp[0], t * ga[0]) : 0.0f, seeded ? fmaf(tf, gp[1], t * ga[1]) : 0.0f,
                        seeded ? fmaf(tf, gp[2], t * ga[2]) : 0.0f};

  if constexpr (!CAM) {
    if (valid) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (r.g_org != nullptr) r.g_org[3 * ri + c] = r.accumulate ? r.g_org[3 * ri + c] + go[c] : go[c];
        if (r.g_dir != nullptr) r.g_dir[3 * ri + c] = r.accumulate ? r.g_dir[3 * ri + c] + gd3[c] : gd3[c];
      }
    }
  } else {
    // ---- the ray's 13 terms of its view's sums (zeros for unseeded and invalid lanes)
    float va[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, vb[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (seeded) {
      const int bv = blockIdx.y;  // == view, block-uniform: the basis comes through scalar loads
      const CamBasis& cb = a.cams_dev != nullptr ? a.cams_dev[bv] : a.cams[bv];
      const long long pix = ri - (long long)view * npix;
      const int y = (int)(pix / a.width), x = (int)(pix - (long long)y * a.width);
      float rs, us, len;
      camera_raw(cb, x, y, a.width, a.height, rs, us, len);
      const float dg = fmaf(d[2], gd3[2], fmaf(d[1], gd3[1], d[0] * gd3[0]));
      const float il = 1.0f / len;
      const float gr[3] = {(gd3[0] - d[0] * dg) * il, (gd3[1] - d[1] * dg) * il, (gd3[2] - d[2] * dg) * il};
      const float rg = fmaf(cb.right[2], gr[2], fmaf(cb.right[1], gr[1], cb.right[0] * gr[0]));
      const float ug = fmaf(cb.up[2], gr[2], fmaf(cb.up[1], gr[1], cb.up[0] * gr[0]));
      va[0] = go[0];
      va[1] = go[1];
      va[2] = go[2];
      va[3] = gr[0];
      va[4] = gr[1];
      va[5] = gr[2];
      va[6] = rs * gr[0];
      va[7] = rs * gr[1];
      vb[0] = rs * gr[2];
      vb[1] = us * gr[0];
      vb[2] = us * gr[1];
      vb[3] = us * gr[2];
      vb[4] = fmaf(rs, rg, us * ug) / cb.half_h;  // (u aspect right + v up) . g_raw
    }
    // fixed order: the transposing wave reduction, then the waves in wave order
    const float ra = wave_reduce8(va, lane), rb = wave_reduce8(vb, lane);
    if ((lane & 7) == 7) {
      red[wave][lane >> 3] = ra;
      red[wave][8 + (lane >> 3)] = rb;
    }
    __syncthreads();
    if (tid < kRgCols) {
      float acc = red[0][tid];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) acc += red[w][tid];
      r.partial[((long long)blockIdx.y * gridDim.x + blockIdx.x) * kRgCols + tid] = acc;
    }
  }
}

// One block per view: the view's partial rows added in block order (16 segments of consecutive
// rows, each a chain in block order, then the segments in order), then the 13 -> 7 tail in f64 on
// one thread. out: rm_camera records (7 floats per view).
__global__ __launch_bounds__(256) void rm_raygrad_finish(const float* __restrict__ partial, int bpv,
                                                         const RayGradCams cams, float* __restrict__ out,
                                                         int accumulate) {
  __shared__ float seg[16][kRgCols];
  const int tid = threadIdx.x, col = tid & 15, s = tid >> 4, v = blockIdx.x;
  const int len = (bpv + 15) / 16;
  const float* rows = partial + (long long)v * bpv * kRgCols;
  float acc = 0.0f;
  for (int b = s * len; b < min((s + 1) * len, bpv); ++b) acc += rows[(long long)b * kRgCols + col];
  seg[s][col] = acc;
  __syncthreads();
  if (tid < kRgCols) {
    float tot = seg[0][tid];
    for (int k = 1; k < 16; ++k) tot += seg[k][tid];
    seg[0][tid] = tot;
  }
  __syncthreads();
  if (tid != 0) return;
  const rm_camera& c = cams.c[v];
  const double S[13] = {seg[0][0], seg[0][1], seg[0][2], seg[0][3], seg[0][4], seg[0][5], seg[0][6],
                        seg[0][7], seg[0][8], seg[0][9], seg[0][10], seg[0][11], seg[0][12]};
  auto cross = [](const double x[3], const double y[3], double z[3]) {
    z[0] = x[1] * y[2] - x[2] * y[1];
    z[1] = x[2] * y[0] - x[0] * y[2];
    z[2] = x[0] * y[1] - x[1] * y[0];
  };
  // x = normalize(raw) and the Jacobian applied to gx: (gx - x (x . gx)) / |raw|; math::normalize
  // returns zeros for a zero vector, its Jacobian is taken as zero there
  auto normalize = [](const double raw[3], double x[3], double& len) {
    len = sqrt(raw[0] * raw[0] + raw[1] * raw[1] + raw[2] * raw[2]);
    for (int k = 0; k < 3; ++k) x[k] = len == 0.0 ? 0.0 : raw[k] / len;
  };
  auto normalize_bwd = [](const double x[3], double len, const double gx[3], double graw[3]) {
    const double dot = x[0] * gx[0] + x[1] * gx[1] + x[2] * gx[2];
    for (int k = 0; k < 3; ++k) graw[k] = len == 0.0 ? 0.0 : (gx[k] - x[k] * dot) / len;
  };
  const double up_w[3] = {0.0, 1.0, 0.0};
  const double fr[3] = {(double)c.target[0] - c.eye[0], (double)c.target[1] - c.eye[1], (double)c.target[2] - c.eye[2]};
  double fwd[3], rr[3], right[3], flen, rlen;
  normalize(fr, fwd, flen);
  cross(fwd, up_w, rr);
  normalize(rr, right, rlen);
  const double Gf[3] = {S[3], S[4], S[5]}, Gr[3] = {S[6], S[7], S[8]}, Gu[3] = {S[9], S[10], S[11]};
  // up = right x fwd: dL/dright += fwd x G_u, dL/dfwd += G_u x right
  double a1[3], a2[3], a3[3], grr[3], gfr[3];
  cross(fwd, Gu, a1);
  cross(Gu, right, a2);
  const double gright[3] = {Gr[0] + a1[0], Gr[1] + a1[1], Gr[2] + a1[2]};
  normalize_bwd(right, rlen, gright, grr);
  cross(up_w, grr, a3);  // rr = fwd x up_w: dL/dfwd += up_w x g_rr
  const double gfwd[3] = {Gf[0] + a2[0] + a3[0], Gf[1] + a2[1] + a3[1], Gf[2] + a2[2] + a3[2]};
  normalize_bwd(fwd, flen, gfwd, gfr);
  const double th = (double)c.fov_deg * (3.14159265358979323846 / 360.0), hh = tan(th);
  const double res[7] = {S[0] - gfr[0], S[1] - gfr[1], S[2] - gfr[2], gfr[0], gfr[1], gfr[2],
                         S[12] * (1.0 + hh * hh) * (3.14159265358979323846 / 360.0)};
  float* dst = out + 7 * (long long)v;
  for (int k = 0; k < 7; ++k) dst[k] = accumulate ? dst[k] + (float)res[k] : (float)res[k];
}
