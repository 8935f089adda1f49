// rm_view.h -- the reference viewer's sphere-traced frame render (src/bin/viewer.rs +
// src/bin/shader.wgsl), headless: rm_view_kernel (rm_view). Included by rm_kernels.hip inside
// namespace rm, after the record accessors (rm_records.h) and packed helpers it shares with the other kernels.
//
// The viewer's math is not the training render's (shader.wgsl:43-128):
//   rays   ux = (2 (i + .5) / W - 1) W / H, uy = 1 - 2 (j + .5) / H, rd = normalize(ux uu + uy vv + focal ww)
//   trace  t = 0; up to max_steps times: d = D(ro + t rd); d < hit_eps: hit; t > t_max: miss; t += d
//   D      soft-min -log(sum_j exp(-k (|p - c_j| - r_j))) / k (the shader's pairwise smin_exp fold is
//          this function), here as a base-2 log-sum-exp with the running-maximum shift: where the
//          shader's unshifted fp32 fold underflows to log(0) (every sphere farther than about 2.7
//          units at k = 32) and the reference viewer goes black, this one keeps rendering
//   normal n = normalize(sum_s s D(p + eps s)) over the four tetrahedral taps s; a tap sum of exactly
//          zero gives a zero diffuse term instead of the shader's NaN
//   colour col = sum_j c_j exp(-csharp d_j) / (sum_j exp(-csharp d_j) + 1e-5), unshifted as the shader
//   out    col (ambient + max(n . normalize(light), 0) (1 - ambient)); a miss is exactly 0, no mask
//
// One ray per lane, 8x8 pixels per wave, 16x16 per block, grid = tiles x frames; lanes past a ragged
// edge are masked (they never march and write nothing). The trace is a data-dependent loop: a lane
// stops at its own hit test, the wave leaves the loop when all its lanes have ended. Every distance
// comes from e = p - c in direct form (e = 0.5 (-2c) + p from the records, one rounding): at
// normal_eps = 1e-3 the expansion form's rounding of |p|^2 + |c|^2 - 2 p.c would be amplified by
// 1 / eps in the normal. The records are read through scalar loads (Lds), so fp16 colours
// (RM_MARCH_COLOR_F16, widened by rm_prep_kernel) work and M has no limit.
//
// Exact skip. A hit needs D(p) < hit_eps. D(p) >= min_j (|p - c_j| - r_j) - ln(M) / k (the
// log-sum-exp of M terms exceeds its largest term by at most ln M), and with the scene's bounding
// sphere (c0, R) of the record header, R >= |c_j - c0| + r_j, every |p - c_j| - r_j >= |p - c0| - R.
// So a hit at p needs |p - c0| < R + hit_eps + ln(M) / k =: Rs. The kernel uses
//   Rs' = (Rs + 1e-3) (1 + 1e-5) + 4e-6 |ro - c0|
// for Rs: 1e-3 is far above the fp32 error of the computed D (below 1e-5 for |p - c0| near Rs: the
// exponents carry k |p - c| 2^-24 and v_log / v_exp / v_sqrt are 1 ulp) and of hit_eps' own compare;
// the relative terms cover the rounding of |p - c0| itself (a few 2^-24 of it), of the points
// p = ro + t rd against the exact line (a few ulp of |ro - c0| + t) and of |rd| = 1 +- 2^-22. Hence
//   (a) a ray whose line (t >= 0) never comes within Rs' of c0 cannot hit: it is a miss without
//       marching -- tca = (c0 - ro) . rd <= 0 and |ro - c0| > Rs', or |(c0 - ro) - tca rd| > Rs';
//   (b) a marching ray at a point with (p - c0) . rd > 0 (receding: |p - c0| only grows with t, and
//       t only grows, every step being d >= hit_eps > 0) and |p - c0| > Rs' cannot hit later: a miss.
// A miss writes the same bits however it was found (0, 0, 0 / alpha 255 / +inf), and a hit ray is
// never touched by (a) or (b), so the exits change no bit of any output. RM_MARCH_NO_EARLY_EXIT
// turns both off (A/B timing, tests). No atomics of any kind: two calls give the same bits.
#pragma once

constexpr int kViewInline = 16;  // frames per launch: their bases travel in the kernel arguments

struct ViewCam {  // viewer.rs:65-86 on the host in fp32: ro and the orthonormal basis
  float pos[3], uu[3], vv[3], ww[3];
};

struct ViewArgs {
  const float4* rec_buf;  // sphere records of this call (rm_prep_kernel)
  int Mpad;
  int width, height, tiles_x;
  int max_steps;
  float kappa;  // smooth_k log2(e)
  float hit_eps, t_max, normal_eps, c10l, focal;
  float skip_add;  // hit_eps + ln(M) / k (rounded up) + 1e-3: Rs' - R before the relative terms; 0 = exits off
  int count_iters;  // RM_VIEW_COUNT_ITERATIONS: out_depth receives the ray's soft-min evaluations
  const float* light_dir;
  const float* ambient;
  float* out_rgb;            // nullable [F,H,W,3]
  unsigned char* out_rgba8;  // nullable [F,H,W,4], 4-byte aligned
  float* out_depth;          // nullable [F,H,W]
  long long frame0;          // first frame of this launch in the outputs
  ViewCam cams[kViewInline];
};

// D(p): running-maximum log-sum-exp over all pairs, 16 spheres per rescale (as lse_point, direct form)
__device__ __forceinline__ float view_sdf(const float p[3], const Lds& L, int npairs, float nkappa, float inv_kappa) {
  const f2 PX = sp(p[0]), PY = sp(p[1]), PZ = sp(p[2]), NK = sp(nkappa), HALF = sp(0.5f);
  float m = -INFINITY, s = 0.0f;
  for (int i0 = 0; i0 < npairs; i0 += 8) {
    f2 v[8];
#pragma unroll
    for (int ii = 0; ii < 8; ++ii) {
      const float4 A = L.p0(i0 + ii), B = L.p1(i0 + ii);
      const float2 K = L.kr(i0 + ii);
      const f2 ex = fma2(HALF, lo(A), PX), ey = fma2(HALF, hi(A), PY), ez = fma2(HALF, lo(B), PZ);
      const f2 q = fma2(ez, ez, fma2(ey, ey, ex * ex));
      v[ii] = fma2(sqrt2(q), NK, f2{K.x, K.y});
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
  return -(flog2(s) + m) * inv_kappa;
}

// The four tetrahedral taps D(p + eps s) and the colour sums at p in one pass. With e = p - c,
// |e + eps s|^2 = |e|^2 + 3 eps^2 + 2 eps (s . e): the taps differ only in the last term (lse_taps'
// form), so the finite difference keeps its accuracy in fp32.
__device__ __forceinline__ void view_shade_sweep(const float p[3], const Lds& L, int npairs, float nkappa,
                                                 float inv_kappa, float eps, float c10l, float (&dtap)[4], float& zw,
                                                 float (&col)[3]) {
  const f2 PX = sp(p[0]), PY = sp(p[1]), PZ = sp(p[2]), NK = sp(nkappa), HALF = sp(0.5f), E3 = sp(3.0f * eps * eps),
           TE = sp(2.0f * eps), NCL = sp(-c10l);
  float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  f2 Zw = sp(0.0f), C[3] = {sp(0.0f), sp(0.0f), sp(0.0f)};
  for (int i0 = 0; i0 < npairs; i0 += 4) {
    f2 v[4][4];
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
      const float4 A = L.p0(i0 + ii), B = L.p1(i0 + ii), R = L.p2(i0 + ii), C3 = L.p3(i0 + ii);
      const float2 C4 = L.p4(i0 + ii);
      const f2 ex = fma2(HALF, lo(A), PX), ey = fma2(HALF, hi(A), PY), ez = fma2(HALF, lo(B), PZ);
      const f2 q0 = fma2(ez, ez, fma2(ey, ey, ex * ex));
      // colour: w = exp(-csharp (rho - r)), unshifted as the shader (the 1e-5 is absolute)
      const f2 w = exp2v((sqrt2(q0) - hi(R)) * NCL);
      Zw += w;
      C[0] = fma2(w, lo(C3), C[0]);
      C[1] = fma2(w, hi(C3), C[1]);
      C[2] = fma2(w, f2{C4.x, C4.y}, C[2]);
      // taps s = (1,-1,-1), (-1,-1,1), (-1,1,-1), (1,1,1)
      const f2 Q = q0 + E3;
      const f2 se[4] = {ex - ey - ez, ez - ex - ey, ey - ex - ez, ex + ey + ez};
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t][ii] = fma2(sqrt2(fma2(se[t], TE, Q)), NK, lo(R));
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
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
#pragma unroll
  for (int t = 0; t < 4; ++t) dtap[t] = -(flog2(s[t]) + m[t]) * inv_kappa;
  zw = Zw.x + Zw.y;
  col[0] = C[0].x + C[0].y;
  col[1] = C[1].x + C[1].y;
  col[2] = C[2].x + C[2].y;
}

// piecewise sRGB encode of a linear value, rounded to the nearest of 0..255 (NaN -> 0)
__device__ __forceinline__ unsigned srgb8(float c) {
  c = fminf(fmaxf(c, 0.0f), 1.0f);  // fmaxf(NaN, 0) = 0
  const float e = c < 0.0031308f ? 12.92f * c : fmaf(1.055f, fexp2(flog2(c) * (1.0f / 2.4f)), -0.055f);
  return (unsigned)(int)fmaf(e, 255.0f, 0.5f);
}

__global__ __launch_bounds__(kBlock, kMinWavesPerSimd) void rm_view_kernel(const ViewArgs a) {
  static_assert(kBlock == 256, "16x16 pixel tiles: four 8x8 waves");
  const Lds L = bind_records(a.rec_buf, a.Mpad);
  const int np = a.Mpad / 2;
  const cf1_ptr hdr = rec_header(L, a.Mpad);  // the bounding sphere (c0, R) of scene_bound

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x, tile_y = tile / a.tiles_x, tile_x = tile - tile_y * a.tiles_x;
  const int px = 16 * tile_x + 8 * (wave & 1) + (lane & 7), py = 16 * tile_y + 8 * (wave >> 1) + (lane >> 3);
  const bool valid = px < a.width && py < a.height;
  const ViewCam& cam = a.cams[blockIdx.y];  // block-uniform: scalar loads

  // the ray (shader.wgsl:104-112); a masked lane gets the frame's centre direction and never marches
  const float aspect = (float)a.width / (float)a.height;
  const float ux = valid ? ((2.0f * ((float)px + 0.5f)) / (float)a.width - 1.0f) * aspect : 0.0f;
  const float uy = valid ? 1.0f - (2.0f * ((float)py + 0.5f)) / (float)a.height : 0.0f;
  const float ro[3] = {cam.pos[0], cam.pos[1], cam.pos[2]};
  float rd[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) rd[k] = fmaf(ux, cam.uu[k], fmaf(uy, cam.vv[k], a.focal * cam.ww[k]));
  {
    const float il = 1.0f / sqrtf(fmaf(rd[2], rd[2], fmaf(rd[1], rd[1], rd[0] * rd[0])));
    rd[0] *= il;
    rd[1] *= il;
    rd[2] *= il;
  }

  const float nkappa = -a.kappa, inv_kappa = 1.0f / a.kappa;
  const float c0[3] = {hdr[Hdr::kCx], hdr[Hdr::kCy], hdr[Hdr::kCz]};
  const bool exits = a.skip_add > 0.0f;
  float rs2 = INFINITY;  // Rs'^2 of this launch's frame
  enum { kLive = 0, kHit = 1, kMiss = 2 };
  int code = valid ? kLive : kMiss;
  if (exits) {
    const float oc[3] = {c0[0] - ro[0], c0[1] - ro[1], c0[2] - ro[2]};
    const float oc_len = sqrtf(fmaf(oc[2], oc[2], fmaf(oc[1], oc[1], oc[0] * oc[0])));
    const float rs = fmaf(4e-6f, oc_len, (hdr[Hdr::kR] + a.skip_add) * (1.0f + 1e-5f));
    rs2 = rs * rs;
    const float tca = fmaf(oc[2], rd[2], fmaf(oc[1], rd[1], oc[0] * rd[0]));
    const float pe[3] = {fmaf(-tca, rd[0], oc[0]), fmaf(-tca, rd[1], oc[1]), fmaf(-tca, rd[2], oc[2])};
    const float perp2 = fmaf(pe[2], pe[2], fmaf(pe[1], pe[1], pe[0] * pe[0]));
    // (a): the closest point of the half-line t >= 0 to c0 is ro (tca <= 0) or the foot of c0
    if (tca <= 0.0f ? oc_len > rs : perp2 > rs2) code = kMiss;
  }

  float t = 0.0f;
  int iters = 0;
  for (int it = 0; it < a.max_steps; ++it) {
    if (!__any(code == kLive)) break;
    const float p[3] = {fmaf(rd[0], t, ro[0]), fmaf(rd[1], t, ro[1]), fmaf(rd[2], t, ro[2])};
    const float d = view_sdf(p, L, np, nkappa, inv_kappa);
    if (code == kLive) {
      ++iters;
      if (d < a.hit_eps) {
        code = kHit;
      } else if (t > a.t_max) {
        code = kMiss;
      } else {
        const float e0[3] = {p[0] - c0[0], p[1] - c0[1], p[2] - c0[2]};
        const float along = fmaf(e0[2], rd[2], fmaf(e0[1], rd[1], e0[0] * rd[0]));
        const float dist2 = fmaf(e0[2], e0[2], fmaf(e0[1], e0[1], e0[0] * e0[0]));
        if (exits && along > 0.0f && dist2 > rs2) code = kMiss;  // (b)
        else t += d;
      }
    }
  }

  float out[3] = {0.0f, 0.0f, 0.0f};
  if (__any(code == kHit)) {
    const float p[3] = {fmaf(rd[0], t, ro[0]), fmaf(rd[1], t, ro[1]), fmaf(rd[2], t, ro[2])};
    float dt[4], zw, col[3];
    view_shade_sweep(p, L, np, nkappa, inv_kappa, a.normal_eps, a.c10l, dt, zw, col);
    if (code == kHit) {
      const float n[3] = {dt[0] - dt[1] - dt[2] + dt[3], dt[2] + dt[3] - dt[0] - dt[1], dt[1] + dt[3] - dt[0] - dt[2]};
      const float len2 = fmaf(n[2], n[2], fmaf(n[1], n[1], n[0] * n[0]));
      float ldn[3];
      light_unit(a.light_dir, ldn);
      const float ndl = fmaf(n[2], ldn[2], fmaf(n[1], ldn[1], n[0] * ldn[0]));
      const float diff = len2 > 0.0f ? fmaxf(ndl * frsq(len2), 0.0f) : 0.0f;
      const float amb = a.ambient[0];
      const float lgt = fmaf(diff, 1.0f - amb, amb);
      const float iz = 1.0f / (zw + 1e-5f);
      out[0] = col[0] * iz * lgt;
      out[1] = col[1] * iz * lgt;
      out[2] = col[2] * iz * lgt;
    }
  }

  if (!valid) return;
  const long long pix = ((a.frame0 + blockIdx.y) * (long long)a.height + py) * a.width + px;
  if (a.out_rgb != nullptr) {
    a.out_rgb[3 * pix] = out[0];
    a.out_rgb[3 * pix + 1] = out[1];
    a.out_rgb[3 * pix + 2] = out[2];
  }
  if (a.out_rgba8 != nullptr)
    reinterpret_cast<unsigned*>(a.out_rgba8)[pix] = srgb8(out[0]) | (srgb8(out[1]) << 8) | (srgb8(out[2]) << 16) | 0xFF000000u;
  if (a.out_depth != nullptr) a.out_depth[pix] = a.count_iters ? (float)iters : (code == kHit ? t : INFINITY);
}
