// rm_sdf.h -- the scene's distance field at points of the caller's choosing: rm_sdf_kernel<GRID, FULL>
// (rm_sdf_query, rm_sdf_grid) and, at the end of the file, its backward rm_sdf_grad_kernel
// (rm_sdf_query_backward). Included by rm_kernels.hip inside namespace rm, after the record
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

// The escape lattice of a call (KArgs::lattice; rm_tile_proof_kernel below reads it): the distance-only lattice
// sweep above, bit for bit, at the cell centres write_bound laid out for this call's scene.
__global__ __launch_bounds__(kBlock, kMinWavesPerSimd) void rm_lattice_kernel(const SdfArgs a) {
  sdf_body<true, false, true>(a);
}

// ---- the tile proof: rm_tile_proof_kernel (KArgs::tile_proof; the escape proof of rm_ray_kernel) ----
// The lattice's part of the escape proof of a camera call (KArgs::proof == 2), ahead of the per-ray launch:
// one lane per wave tile of the coming per-ray launch -- rays [64 w, 64 w + 64) of the launch, wave w & 3 of
// logical block w >> 2, which setup_ray's 16x16 tiling makes one 8x8 pixel quadrant of one view -- marches ONE
// bound trajectory for the tile's 64 rays and writes taken[w] = 1 when every ray of the tile is proven gone,
// 0 when it is not known. A wave whose byte is 1 stops where bound_proof would have stopped it; a wave whose
// byte is 0 runs the soft-ball bound_proof, so the waves taken are a superset of the soft ball's.
//
// The cone. The rays of a tile share the eye o, and after the origin step they share t (rays already gone
// step differently, and need no proof). d_c is the normalised sum of the tile's four corner rays and
// delta >= |d_r - d_c| for every ray r of the tile: the pixel rectangle is a convex quadrilateral of the image
// plane, its central projection a convex spherical quadrilateral far inside a hemisphere about d_c, and the
// distance from d_c is convex along great-circle arcs there, so it is largest at a corner. The corners are the
// tile's own corner pixels' rays (camera_ray maps pixel x to x / W, not to its centre), in their fp32 bits;
// the other rays' fp32 directions lie within 2e-7 of the exact quadrilateral, and delta is taken kTileConeRel
// relative + kTileConeAbs up. With p_c(u) = o + d_c u, every ray has |p_r(u) - p_c(u)| <= |u| delta, and D is 1-Lipschitz:
//   t_r + D(p_r(t_r)) >= u + D(p_r(u)) >= u + L(p_c(u)) - |u| delta        for u <= t_r, any L <= D,
// so u <- u + L(p_c(u)) - |u| delta stays at or behind every ray's march step for step, as bound_proof's u does
// for its own ray. The tile is proven at a bound step once wave_escaped's test holds at p_r(u) for every
// r, in the conservative forms
//   distance   |p_c - c_0| - |u| delta >= T(steps left) kProofDistUp             (|p_r - c_0| >= |p_c - c_0| - |u| delta)
//   receding   (o - c_0) . d_c - |o - c_0| delta + u (1 -+ kTileRecedeRel) >= 0  ((p_r - c_0) . d_r = (o - c_0) . d_r + u |d_r|^2)
// (the sign that makes the term smaller); the ray at t_r >= u is then receding and at least as far out.
// The spare-lane alternative (the per-ray test, 64 lanes per tile) was not taken: one lane per tile is the point.
//
// The bound. L = max(|p - c_0| - R_soft, max over the 8 lattice points n around p of G[n] - |p - x_n|), less the
// margins: D(p) >= D(x_n) - |p - x_n| holds for EVERY lattice point, so the cell's half-diagonal slack and the
// cell-index rounding argument of a one-cell lookup are not needed, and no inside test either -- the base index
// is held to [0, N - 2] per axis, and a far lattice point only gives a weak bound. x_n is formed as
// rm_lattice_kernel forms it, origin + (float)i h in fp32 without contraction: the same bits, the point G[n] was
// evaluated at.
// Margins: the tile reader of rm_proof.h's ledger. Specific to this reader: the pre-pass is latency-bound (one
// lane per tile: a 10-view call is 640 waves of it, each a chain of up to S dependent bound steps), so a bound
// step is kept short. The cone's own state -- u, p_c, e, the sums of squares, the tests -- runs in fp64
// (contraction off), roundings below 1e-13 at the magnitudes the guard admits. Its square roots are fp32 (no fp64
// square root or division in the loop), each taken kTileRootRel to the safe side: up (sqrt_up) for |o - c_0| and
// delta, down (sqrt_down) for |p_c - c_0|, which enters the bound step and the distance test from below. The
// lattice term is fp32 throughout: p rounded to fp32, q = p - x_n (x_n exact: the lattice kernel's bits), the
// three squares summed, the square root, g - |q| (1 + kTileLatticeRel), less kTileLatticeAbs: what bound_proof
// charges on both terms, the lattice kernel's fp32 and this reader's own rounding of p and of g - |q|.
// The give-up rule is bound_proof's: a net bound step of kProofMinStep or less ends the tile's proof with 0.
// Tiles that get 0 unseen: a tile whose 64 lanes are not all rays of the launch (none under tiling 2: a view is
// whole 256-ray blocks), the magnitude guard. The host launches this kernel only for tiled launches large enough
// to pay for it (tile_proof_policy, rm_launch.h): in rows order (tiling != 2) a wave is no pixel rectangle, and
// those launches and the small ones read the lattice per ray inside bound_proof instead. A wave whose byte is 0
// pays for the soft ball twice -- this trajectory's L held the soft-ball term already -- which keeps the taken
// set a superset of the soft ball's by construction and costs such a wave one more soft-ball bound march.
__device__ __forceinline__ double sqrt_up(double x) { return (double)fsqrt((float)x) * (1.0 + kTileRootRel) + kTileRootFloor; }
__device__ __forceinline__ double sqrt_down(double x) { return (double)fsqrt((float)x) * (1.0 - kTileRootRel); }
__device__ __forceinline__ bool tile_proven(const KArgs& a, long long w) {
#pragma clang fp contract(off)
  if (a.tiling != 2 || !(a.gone_d > 0.0f) || a.lattice == nullptr || 64 * w + 64 > a.n_rays) return false;
  const long long npix = (long long)a.width * a.height, ri = a.ray_begin + 64 * w;
  const int v = (int)(ri / npix);
  const long long pix = ri - (long long)v * npix, tl = pix >> 8;
  if ((ri + 63) / npix != v) return false;
  const int qd = (int)(pix & 255) >> 6, tiles_x = a.width >> 4;
  const int ty = (int)(tl / tiles_x), tx = (int)(tl - (long long)ty * tiles_x);
  const int x0 = (tx << 4) + ((qd & 1) << 3), y0 = (ty << 4) + ((qd >> 1) << 3);  // setup_ray's lane 0
  const CamBasis& cam = a.cams_dev != nullptr ? a.cams_dev[v] : a.cams[v];

  const Lds L = bind_records(a.rec_buf, a.Mpad);
  const cf1_ptr hdr = rec_header(L, a.Mpad);
  const cf1_ptr esc_tab = (cf1_ptr)RecLayout::at<const char>(a.rec_buf, RecLayout(a.Mpad).esc());
  const cf1_ptr lg = (cf1_ptr)RecLayout::at<const char>(a.rec_buf, RecLayout(a.Mpad).lattice());
  const float c0x = hdr[Hdr::kCx], c0y = hdr[Hdr::kCy], c0z = hdr[Hdr::kCz];

  float o[3], dk[4][3];
  for (int k = 0; k < 4; ++k) camera_ray(cam, x0 + 7 * (k & 1), y0 + 7 * (k >> 1), a.width, a.height, o, dk[k]);
  // bound_proof's magnitude guard, in its fp32 form
  if (!(fabsf(o[0]) + fabsf(o[1]) + fabsf(o[2]) + fabsf(c0x) + fabsf(c0y) + fabsf(c0z) + 3.0f * esc_tab[0] <= (float)kProofMaxMagnitude))
    return false;
  double dc[3];
  for (int k = 0; k < 3; ++k) dc[k] = ((double)dk[0][k] + (double)dk[1][k]) + ((double)dk[2][k] + (double)dk[3][k]);
  // d_c need not be a unit vector to the last bit: delta is taken against the d_c used, and nothing else asks
  const double il = (double)frsq((float)(dc[0] * dc[0] + dc[1] * dc[1] + dc[2] * dc[2]));
  for (int k = 0; k < 3; ++k) dc[k] *= il;
  double delta = 0.0;
  for (int k = 0; k < 4; ++k) {
    const double ex = (double)dk[k][0] - dc[0], ey = (double)dk[k][1] - dc[1], ez = (double)dk[k][2] - dc[2];
    delta = fmax(delta, sqrt_up(ex * ex + ey * ey + ez * ez));
  }
  delta = delta * (1.0 + kTileConeRel) + kTileConeAbs;

  const double c0[3] = {(double)c0x, (double)c0y, (double)c0z};
  const double oc[3] = {(double)o[0] - c0[0], (double)o[1] - c0[1], (double)o[2] - c0[2]};
  const double rec0 = (oc[0] * dc[0] + oc[1] * dc[1] + oc[2] * dc[2]) -
                      sqrt_up(oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2]) * delta;
  // bound_proof's rs: the same formula, compiled here without contraction, so the last bit may differ. Both are
  // sound (allowances of 1e-3 against a rounding of 1e-7); the taken set is a superset of the soft ball's because
  // a wave whose byte is 0 runs bound_proof, not because the bits agree
  const double rs = (double)((hdr[Hdr::kRsoft] + (float)kMarchAbs) * (1.0f + (float)kRadiusRel) + (float)kBoundStepAbs);
  const float h = lg[Lat::kH], x0f[3] = {lg[Lat::kX0], lg[Lat::kY0], lg[Lat::kZ0]};
  const float half = lg[Lat::kHalf], inv_h = lg[Lat::kInvH];

  // the state the per-ray kernel's waves bring to bound_proof: after the shared origin step where it is taken
  double u = 0.0;
  int st0 = 0;
  if (a.origin != nullptr && a.steps > 0) {
    const float D0 = a.origin[RecTail::kD0 + v];
    if ((__float_as_uint(D0) & 0x7fffffffu) <= 0x7f800000u) {
      u = (double)fminf(D0, kTMax);
      st0 = 1;
    }
  }
  for (int n = st0; n < a.steps; ++n) {
    const double p[3] = {(double)o[0] + dc[0] * u, (double)o[1] + dc[1] * u, (double)o[2] + dc[2] * u};
    const double e[3] = {p[0] - c0[0], p[1] - c0[1], p[2] - c0[2]};
    const double dist = sqrt_down(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);  // enters both uses from below
    const double ud = fabs(u) * delta;
    const double Tn = (double)esc_tab[min(a.steps - n, kEscTab - 1)];
    if (rec0 + u * (u >= 0.0 ? 1.0 - kTileRecedeRel : 1.0 + kTileRecedeRel) >= 0.0 && dist - ud >= Tn * kProofDistUp) return true;
    double Lb = dist - rs;
    // the lattice term, fp32: per axis the base index (>= 0: the conversion truncates as floor would) and the
    // squared offsets of p from the two lattice planes beside it; then the 8 points, one base address
    int i0[3];
    float q2[3][2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float f = fminf(fmaxf(((float)e[k] + half) * inv_h - 0.5f, 0.0f), (float)(kLatticeN - 2));
      i0[k] = (int)f;
      const float pk = (float)p[k];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const float q = pk - (x0f[k] + (float)(i0[k] + j) * h);
        q2[k][j] = q * q;
      }
    }
    const float* g0 = a.lattice + (i0[2] * kLatticeN + i0[1]) * kLatticeN + i0[0];
    float best = -INFINITY;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int jx = c & 1, jy = (c >> 1) & 1, jz = c >> 2;
      const float dn = fsqrt(q2[0][jx] + q2[1][jy] + q2[2][jz]);
      best = fmaxf(best, fmaf(dn, -(1.0f + (float)kTileLatticeRel), g0[(jz * kLatticeN + jy) * kLatticeN + jx]));
    }
    Lb = fmax(Lb, (double)best - kTileLatticeAbs);
    const double step = Lb - ud;
    if (!(step > (double)kProofMinStep)) return false;
    u += step;
  }
  return false;
}

__global__ __launch_bounds__(kBlock) void rm_tile_proof_kernel(const KArgs a, unsigned char* __restrict__ taken,
                                                               long long n_tiles) {
  const long long w = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (w < n_tiles) taken[w] = tile_proven(a, w) ? 1 : 0;
}

// ---- the field's backward: rm_sdf_grad_kernel (rm_sdf_query_backward) -------------------------
// Upstream gD_i (a scalar per point) and gC_i (three per point), either possibly absent. With e_j, q_j,
// rho_j, d_j, beta, w and C = sum_j w_j col_j as above, per point
//   a_j = gD beta_j - cs w_j (gC . (col_j - C)),   u_j = e_j / rho_j if q_j >= 1e-6, else 0
//   dL/dc_j += -a_j u_j,  dL/dr_j += -a_j,  dL/dcol_j += w_j gC,  dL/dp_i = sum_j a_j u_j
// (cs = color_sharpness). The clamp max(sum, 1e-8) of the shifted log-sum-exp is never active -- the
// nearest sphere's term is 1 -- so it has no branch here. One block takes 256 points, in three sweeps:
//   1. forward: sdf_sweep<true>, one point per lane: d_min, s, Zw, C;
//   2. points (only when grad_points is asked for): one point per lane again, sum_j a_j u_j -- a_j needs
//      the finished C;
//   3. spheres (only when a scene gradient is asked for), with the roles turned around: every lane parks
//      its point's twelve values {p, d_min | gD / s, gC / Zw | C} in LDS, then a lane owns a sphere
//      pair and runs over the points in index order, reading them at an address the lanes of a group
//      share (an LDS broadcast). The seven sums of a sphere sit in the lane's registers: no cross-lane
//      reduction, one plain addition chain. Scenes of fewer than 256 pairs deal the points out over
//      G = 256 / lanes groups of lanes = pow2ceil(pairs) >= 16 lanes each (group g takes the points
//      i = g mod G, in order); the groups' sums are added in group order through LDS. More than 256
//      pairs: one pass of the points per 256 pairs.
// The block's sums are one partial record in the per-ray kernels' layout ([Mpad][8] | 8 scalars, scalar
// 7 the live flag; rm_reduce.h), which rm_reduce_partials and the finalize turn into rm_grads in a
// fixed order: no atomics, two calls give the same bits. A point whose seeds are all zero writes exact
// zeros and adds exact zeros; a block of such points writes its live flag 0 and its points' zeros and
// leaves before the first sweep -- the bits of not skipping. d_j has the forward sweep's bits (the same
// operations, contraction off), so no exponent is positive.
struct SdfGradArgs {
  const float4* rec_buf;
  int Mpad;
  float kappa, c10l;  // smooth_k log2(e), color_sharpness log2(e)
  float cs;           // color_sharpness
  const float* points;  // [n,3]
  long long begin, n;   // first point of this launch, points in all
  const float* g_dist;   // nullable [n]
  const float* g_color;  // nullable [n,3]
  float* g_points;       // nullable [n,3]
  int accumulate;        // g_points += (the scene gradient's accumulate is the finalize's)
  float* partials;       // nullable: one record of `rec` floats per block of this launch
  long long rec;
};

constexpr int kSdfPark = 12;  // floats a point parks for the sphere sweep (three float4)
constexpr int kSdfSums = 14;  // sums of a sphere pair: (gc.xyz, gr, gcol.rgb) x 2

// a_j for a sphere pair at shifted distance dd = d_min - d (<= 0): A = gD / s, GZ = gC / Zw
__device__ __forceinline__ f2 sdf_pair_a(f2 dd, f2 KA, f2 CL, f2 CS, f2 A, const f2 (&GZ)[3], const f2 (&CC)[3], f2 c0,
                                         f2 c1, f2 c2, f2& w) {
#pragma clang fp contract(off)
  const f2 b = exp2v(dd * KA);
  w = exp2v(dd * CL);
  const f2 t = fma2(GZ[2], c2 - CC[2], fma2(GZ[1], c1 - CC[1], GZ[0] * (c0 - CC[0])));
  return A * b - (CS * w) * t;
}

// sweep 2: dL/dp of one point, sum_j a_j u_j
__device__ __forceinline__ void sdf_point_grad(const float p[3], const Lds& L, int npairs, float kappa, float c10l,
                                               float cs, float dmin, float A, const float gz[3], const float c[3],
                                               float (&gp)[3]) {
#pragma clang fp contract(off)
  const f2 PX = sp(p[0]), PY = sp(p[1]), PZ = sp(p[2]), HALF = sp(0.5f), KA = sp(kappa), CL = sp(c10l), CS = sp(cs);
  const f2 DN = sp(dmin), AA = sp(A), GZ[3] = {sp(gz[0]), sp(gz[1]), sp(gz[2])}, CC[3] = {sp(c[0]), sp(c[1]), sp(c[2])};
  f2 G[3] = {sp(0.0f), sp(0.0f), sp(0.0f)};
#pragma unroll 4
  for (int i = 0; i < npairs; ++i) {
    const float4 P0 = L.p0(i), P1 = L.p1(i), R = L.p2(i), C3 = L.p3(i);
    const float2 C4 = L.p4(i);
    const f2 ex = fma2(HALF, lo(P0), PX), ey = fma2(HALF, hi(P0), PY), ez = fma2(HALF, lo(P1), PZ);
    const f2 q = fma2(ez, ez, fma2(ey, ey, ex * ex));
    const f2 qc = clamp_q(q);
    const f2 d = sqrt2(qc) - hi(R);
    const f2 r = rsq2(qc);
    const f2 ir = f2{q.x >= 1e-6f ? r.x : 0.0f, q.y >= 1e-6f ? r.y : 0.0f};
    f2 w;
    const f2 aj = sdf_pair_a(DN - d, KA, CL, CS, AA, GZ, CC, lo(C3), hi(C3), f2{C4.x, C4.y}, w);
    const f2 au = aj * ir;
    G[0] = fma2(au, ex, G[0]);
    G[1] = fma2(au, ey, G[1]);
    G[2] = fma2(au, ez, G[2]);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) gp[k] = G[k].x + G[k].y;
}

__global__ __launch_bounds__(kBlock, kMinWavesPerSimd) void rm_sdf_grad_kernel(const SdfGradArgs a) {
  static_assert(kBlock == 256, "256 points, up to 256 sphere pairs a pass");
  __shared__ float4 park[kBlock * kSdfPark / 4];
  __shared__ float comb[kSdfSums * kBlock];
  const Lds L = bind_records(a.rec_buf, a.Mpad);
  const int np = a.Mpad / 2, tid = threadIdx.x;
  const long long idx = a.begin + (long long)blockIdx.x * kBlock + tid;
  const bool valid = idx < a.n;
  float p[3] = {0.0f, 0.0f, 0.0f}, gD = 0.0f, gC[3] = {0.0f, 0.0f, 0.0f};  // a masked lane: the origin, no seed
  if (valid) {
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = a.points[3 * idx + k];
    if (a.g_dist != nullptr) gD = a.g_dist[idx];
    if (a.g_color != nullptr)
#pragma unroll
      for (int k = 0; k < 3; ++k) gC[k] = a.g_color[3 * idx + k];
  }
  const bool seeded = gD != 0.0f || gC[0] != 0.0f || gC[1] != 0.0f || gC[2] != 0.0f;
  const bool live = __syncthreads_or(seeded ? 1 : 0) != 0;
  float* prow = a.partials != nullptr ? a.partials + (long long)blockIdx.x * a.rec : nullptr;
  if (prow != nullptr && tid < 8) prow[(long long)a.Mpad * 8 + tid] = tid == 7 && live ? 1.0f : 0.0f;

  float gp[3] = {0.0f, 0.0f, 0.0f};
  if (live) {
    float dmin, s, zw = 1.0f, g[3] = {0.0f, 0.0f, 0.0f}, col[3] = {0.0f, 0.0f, 0.0f};
    sdf_sweep<true>(p, L, np, a.kappa, a.c10l, dmin, s, zw, g, col);
    const float is = 1.0f / s, iz = 1.0f / zw;
    const float A = gD * is, gz[3] = {gC[0] * iz, gC[1] * iz, gC[2] * iz}, c[3] = {col[0] * iz, col[1] * iz, col[2] * iz};
    if (a.g_points != nullptr) sdf_point_grad(p, L, np, a.kappa, a.c10l, a.cs, dmin, A, gz, c, gp);
    if (prow != nullptr) {
#pragma clang fp contract(off)
      park[3 * tid] = make_float4(p[0], p[1], p[2], dmin);
      park[3 * tid + 1] = make_float4(A, gz[0], gz[1], gz[2]);
      park[3 * tid + 2] = make_float4(c[0], c[1], c[2], 0.0f);
      __syncthreads();
      int lanes = 16;  // of a group: pow2ceil(pairs), 16 ... 256
      while (lanes < np && lanes < kBlock) lanes *= 2;
      const int groups = kBlock / lanes, li = tid & (lanes - 1), grp = tid / lanes;
      const f2 HALF = sp(0.5f), KA = sp(a.kappa), CL = sp(a.c10l), CS = sp(a.cs);
      const float2* P4 = reinterpret_cast<const float2*>(a.rec_buf + RecLayout(a.Mpad).p4_first());
      for (int base = 0; base < np; base += kBlock) {
        const int ip = base + li;
        const bool own = ip < np;
        const int ic = own ? ip : np - 1;
        const RecLayout lay(a.Mpad);
        const float4 P0 = a.rec_buf[lay.pair(RecLayout::kP0, ic)], P1 = a.rec_buf[lay.pair(RecLayout::kP1, ic)],
                     R = a.rec_buf[lay.pair(RecLayout::kP2, ic)], C3 = a.rec_buf[lay.pair(RecLayout::kP3, ic)];
        const float2 C4 = P4[ic];
        const f2 c0 = lo(C3), c1 = hi(C3), c2 = f2{C4.x, C4.y}, rad = hi(R);
        f2 S[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) S[k] = sp(0.0f);
        for (int i = grp; i < kBlock; i += groups) {
          const float4 v0 = park[3 * i], v1 = park[3 * i + 1], v2 = park[3 * i + 2];
          const f2 ex = fma2(HALF, lo(P0), sp(v0.x)), ey = fma2(HALF, hi(P0), sp(v0.y)), ez = fma2(HALF, lo(P1), sp(v0.z));
          const f2 q = fma2(ez, ez, fma2(ey, ey, ex * ex));
          const f2 qc = clamp_q(q);
          const f2 d = sqrt2(qc) - rad;
          const f2 r = rsq2(qc);
          const f2 ir = f2{q.x >= 1e-6f ? r.x : 0.0f, q.y >= 1e-6f ? r.y : 0.0f};
          const f2 GZ[3] = {sp(v1.y), sp(v1.z), sp(v1.w)}, CC[3] = {sp(v2.x), sp(v2.y), sp(v2.z)};
          f2 w;
          const f2 aj = sdf_pair_a(sp(v0.w) - d, KA, CL, CS, sp(v1.x), GZ, CC, c0, c1, c2, w);
          const f2 nau = -(aj * ir);
          S[0] = fma2(nau, ex, S[0]);
          S[1] = fma2(nau, ey, S[1]);
          S[2] = fma2(nau, ez, S[2]);
          S[3] = S[3] - aj;
          S[4] = fma2(w, GZ[0], S[4]);
          S[5] = fma2(w, GZ[1], S[5]);
          S[6] = fma2(w, GZ[2], S[6]);
        }
        // the groups' sums, added in group order by the first group's lanes; sum k of sphere h at comb[2k + h]
#pragma unroll
        for (int k = 0; k < 7; ++k) {
          comb[(2 * k) * kBlock + tid] = S[k].x;
          comb[(2 * k + 1) * kBlock + tid] = S[k].y;
        }
        __syncthreads();
        if (grp == 0 && own) {
          float t[kSdfSums];
#pragma unroll
          for (int k = 0; k < kSdfSums; ++k) {
            float acc = comb[k * kBlock + li];
            for (int gi = 1; gi < groups; ++gi) acc += comb[k * kBlock + gi * lanes + li];
            t[k] = acc;
          }
          float4* dst = reinterpret_cast<float4*>(prow + (long long)ip * 16);  // spheres 2 ip, 2 ip + 1
          dst[0] = make_float4(t[0], t[2], t[4], t[6]);
          dst[1] = make_float4(t[8], t[10], t[12], 0.0f);
          dst[2] = make_float4(t[1], t[3], t[5], t[7]);
          dst[3] = make_float4(t[9], t[11], t[13], 0.0f);
        }
        __syncthreads();  // comb is free for the next pass
      }
    }
  }
  if (a.g_points != nullptr && valid) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float v = seeded ? gp[k] : 0.0f;
      float* dst = a.g_points + 3 * idx + k;
      *dst = a.accumulate ? *dst + v : v;
    }
  }
}
