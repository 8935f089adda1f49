// rm_sdf.h -- the scene's distance field at points of the caller's choosing: rm_sdf_kernel<GRID, FULL>
// (rm_sdf_query, rm_sdf_grid). Included by rm_kernels.hip inside namespace rm, after the record
// accessors (rm_records.h) and packed helpers it shares with the other kernels.
//
// For a point p and every sphere j (scene.rs:60-79; the reference's expansion form of |p - c|^2
// differs only in rounding):
//   e_j = p - c_j (direct form, one rounding: e = 0.5 (-2c) + p from the records, as rm_view.h)
//   q_j = |e_j|^2,  rho_j = sqrt(max(q_j, 1e-6)),  d_j = rho_j - r_j
//   dist   D = -ln(max(sum_j exp(-k (d_j - d_min)), 1e-8)) / k + d_min     (sdf.rs:30-44)
//   grad   sum_j beta_j e_j / rho_j, beta = softmax(-k d); no term from a sphere with q_j < 1e-6
//          (the zero Jacobian of clamp_min, what autograd of the reference's graph gives)
//   color  sum_j w_j col_j, w = softmax(-color_sharpness d)                 (renderer_diff.rs:64-80)
// One point per lane, one pass over the spheres: the three sums share the shift d_min, the running
// minimum of d, rescaled once per 16 spheres (as view_sdf). Every exponent is (d_min - d_j) times a
// positive constant, <= 0 exactly, so D stays finite however far the point is: the nearest sphere's
// term is 1. The records are read through scalar loads (Lds): fp16 colours (RM_MARCH_COLOR_F16,
// widened by rm_prep_kernel) work and M has no limit. No LDS, no atomics, no per-sphere output:
// two calls give the same bits. FULL = false is the distance alone (the mesh extraction's grid);
// its distance has the bits of the FULL instance's -- the same operations in the same order, fp
// contraction off in the whole sweep, so neither instance's code generation can move them.
//
// GRID: the lattice point is formed here, p = origin + (float)i * spacing per axis (two roundings,
// contraction off: a host reproduces it bit for bit), output index (iz ny + iy) nx + ix. Lanes take
// consecutive indices, so a wave's stores are contiguous; lanes past the end write nothing.
#pragma once

struct SdfArgs {
  const float4* rec_buf;  // sphere records of this call (rm_prep_kernel)
  int Mpad;
  float kappa;  // smooth_k log2(e)
  float c10l;   // color_sharpness log2(e)
  const float* points;  // !GRID: [n,3]
  long long begin, n;   // first point of this launch, points in all
  int nx, ny;           // GRID: extents of the fast axes
  float origin[3], spacing;
  float* dist;   // nullable [n]
  float* grad;   // nullable [n,3]
  float* color;  // nullable [n,3]
  const float* geom;  // rm_lattice_kernel: the record buffer's lattice geometry (Lat; origin / spacing unused)
};

template <bool FULL>
__device__ __forceinline__ void sdf_sweep(const float p[3], const Lds& L, int npairs, float kappa, float c10l,
                                          float& dmin_out, float& s_out, float& zw_out, float (&g)[3],
                                          float (&col)[3]) {
#pragma clang fp contract(off)
  const f2 PX = sp(p[0]), PY = sp(p[1]), PZ = sp(p[2]), HALF = sp(0.5f), KA = sp(kappa), CL = sp(c10l);
  float dmin = INFINITY, s = 0.0f;
  f2 Zw = sp(0.0f), C[3] = {sp(0.0f), sp(0.0f), sp(0.0f)}, G[3] = {sp(0.0f), sp(0.0f), sp(0.0f)};
  for (int i0 = 0; i0 < npairs; i0 += 8) {
    f2 d[8], ir[8];
#pragma unroll
    for (int ii = 0; ii < 8; ++ii) {
      const float4 A = L.p0(i0 + ii), B = L.p1(i0 + ii), R = L.p2(i0 + ii);
      const f2 ex = fma2(HALF, lo(A), PX), ey = fma2(HALF, hi(A), PY), ez = fma2(HALF, lo(B), PZ);
      const f2 q = fma2(ez, ez, fma2(ey, ey, ex * ex));
      const f2 qc = clamp_q(q);
      d[ii] = sqrt2(qc) - hi(R);
      if constexpr (FULL) {
        // 1 / rho, zero under the clamp: the sphere's gradient term drops out
        const f2 r = rsq2(qc);
        ir[ii] = f2{q.x >= 1e-6f ? r.x : 0.0f, q.y >= 1e-6f ? r.y : 0.0f};
      }
    }
    float cm = fminf(d[0].x, d[0].y);
#pragma unroll
    for (int ii = 1; ii < 8; ++ii) cm = fminf(cm, fminf(d[ii].x, d[ii].y));
    const float dn = fminf(dmin, cm);
    // the sums so far, moved to the new shift (the first chunk has none: dmin = inf)
    const float back = dn - dmin;  // <= 0
    const float rs = dmin == INFINITY ? 0.0f : fexp2(kappa * back);
    const f2 DN = sp(dn);
    f2 acc = f2{s * rs, 0.0f};
    if constexpr (FULL) {
      const f2 RS = sp(rs), RC = sp(dmin == INFINITY ? 0.0f : fexp2(c10l * back));
      Zw = Zw * RC;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        C[k] = C[k] * RC;
        G[k] = G[k] * RS;
      }
    }
#pragma unroll
    for (int ii = 0; ii < 8; ++ii) {
      const f2 dd = DN - d[ii];  // <= 0 exactly
      const f2 b = exp2v(dd * KA);
      acc += b;
      if constexpr (FULL) {
        const float4 A = L.p0(i0 + ii), B = L.p1(i0 + ii), C3 = L.p3(i0 + ii);
        const float2 C4 = L.p4(i0 + ii);
        const f2 w = exp2v(dd * CL);
        Zw += w;
        C[0] = fma2(w, lo(C3), C[0]);
        C[1] = fma2(w, hi(C3), C[1]);
        C[2] = fma2(w, f2{C4.x, C4.y}, C[2]);
        const f2 bu = b * ir[ii];
        G[0] = fma2(bu, fma2(HALF, lo(A), PX), G[0]);
        G[1] = fma2(bu, fma2(HALF, hi(A), PY), G[1]);
        G[2] = fma2(bu, fma2(HALF, lo(B), PZ), G[2]);
      }
    }
    s = acc.x + acc.y;
    dmin = dn;
  }
  dmin_out = dmin;
  s_out = s;
  if constexpr (FULL) {
    zw_out = Zw.x + Zw.y;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      g[k] = G[k].x + G[k].y;
      col[k] = C[k].x + C[k].y;
    }
  }
}

// DEV: the lattice's origin and spacing come from device memory (a.geom: {x, y, z, spacing}) instead of
// the arguments -- the escape lattice's, which the record kernel forms (write_bound).
template <bool GRID, bool FULL, bool DEV>
__device__ __forceinline__ void sdf_body(const SdfArgs& a) {
  const Lds L = bind_records(a.rec_buf, a.Mpad);
  const int np = a.Mpad / 2;

  const long long idx = a.begin + (long long)blockIdx.x * kBlock + threadIdx.x;
  const bool valid = idx < a.n;
  float p[3] = {0.0f, 0.0f, 0.0f};  // a masked lane sweeps the origin and writes nothing
  if (valid) {
    if constexpr (GRID) {
#pragma clang fp contract(off)
      const long long row = idx / a.nx;
      const int ix = (int)(idx - row * a.nx);
      const int iz = (int)(row / a.ny), iy = (int)(row - (long long)iz * a.ny);
      if constexpr (DEV) {
        const cf1_ptr g = (cf1_ptr)a.geom;
        const float h = g[Lat::kH];
        p[0] = g[Lat::kX0] + (float)ix * h;
        p[1] = g[Lat::kY0] + (float)iy * h;
        p[2] = g[Lat::kZ0] + (float)iz * h;
      } else {
        p[0] = a.origin[0] + (float)ix * a.spacing;
        p[1] = a.origin[1] + (float)iy * a.spacing;
        p[2] = a.origin[2] + (float)iz * a.spacing;
      }
    } else {
      p[0] = a.points[3 * idx];
      p[1] = a.points[3 * idx + 1];
      p[2] = a.points[3 * idx + 2];
    }
  }
  float dmin, s, zw = 1.0f, g[3] = {0.0f, 0.0f, 0.0f}, col[3] = {0.0f, 0.0f, 0.0f};
  sdf_sweep<FULL>(p, L, np, a.kappa, a.c10l, dmin, s, zw, g, col);
  if (!valid) return;
  if (a.dist != nullptr) a.dist[idx] = dmin - flog2(fmaxf(s, 1e-8f)) / a.kappa;
  if constexpr (FULL) {
    if (a.grad != nullptr) {
      const float is = 1.0f / s;
      a.grad[3 * idx] = g[0] * is;
      a.grad[3 * idx + 1] = g[1] * is;
      a.grad[3 * idx + 2] = g[2] * is;
    }
    if (a.color != nullptr) {
      const float iz = 1.0f / zw;
      a.color[3 * idx] = col[0] * iz;
      a.color[3 * idx + 1] = col[1] * iz;
      a.color[3 * idx + 2] = col[2] * iz;
    }
  }
}

template <bool GRID, bool FULL>
__global__ __launch_bounds__(kBlock, kMinWavesPerSimd) void rm_sdf_kernel(const SdfArgs a) {
  sdf_body<GRID, FULL, false>(a);
}

// The escape lattice of a call (KArgs::lattice; bound_proof in rm_ray_kernel): the distance-only lattice
// sweep above, bit for bit, at the cell centres write_bound laid out for this call's scene.
__global__ __launch_bounds__(kBlock, kMinWavesPerSimd) void rm_lattice_kernel(const SdfArgs a) {
  sdf_body<true, false, true>(a);
}
