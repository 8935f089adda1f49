// rm_loss.h -- the image-space loss of rm_image_loss: weighted L1 + D-SSIM over whole views, its gradient
// with respect to the rendered image, and the per-view sums behind PSNR / SSIM / L1. Included by
// rm_kernels.hip inside namespace rm.
//
// x: the rendered image, y: the target, both fp32 [V, H, W, 3], pixel (v, row, col) at
// ((v*H + row)*W + col)*3 + c. Every view and channel is its own image; outside it there are zeros
// (conv2d(padding = 5)). w(i, j) = g(i) g(j), g the 11-tap Gaussian of sigma 1.5 normalised to sum 1;
// F(a) = sum w a over the window, and per pixel and channel
//   mux = F(x), muy = F(y), sx = F(x^2) - mux^2, sy = F(y^2) - muy^2, sxy = F(xy) - mux muy
//   n1 = 2 mux muy + c1, n2 = 2 sxy + c2, d1 = mux^2 + muy^2 + c1, d2 = sx + sy + c2,  S = n1 n2 / (d1 d2)
//   B = dS/dsx = -S / d2,  C = dS/dsxy = 2 n1 / (d1 d2),
//   A = dS/dmux - 2 mux B - muy C,  dS/dmux = 2 muy n2 / (d1 d2) - 2 mux S / d1
// so that d(sum S)/dx_p = sum_q w(q - p) (A_q + 2 x_p B_q + y_p C_q) = F(A)_p + 2 x_p F(B)_p + y_p F(C)_p
// (w is symmetric; A, B, C are zero outside the image, where no S exists).
//
// Two kernels over tiles of kLossTW x kLossTH pixels of one view (a tile never straddles two views), one block
// of three waves each. A row of kLossTW pixels is 96 consecutive floats, so a "column" below is a (pixel,
// channel) pair and a horizontal tap is 3 floats away: the interleaved layout is convolved as it lies.
//   rm_loss_stats_kernel  stages the tile of x and of y with its 5-pixel halo in LDS (reads outside the image are
//       predicated: zeros, no clamped address), runs the horizontal pass for the five window sums (a lane forms
//       four neighbouring outputs of one channel from 14 taps) into LDS and the vertical pass from there (a lane
//       owns a column and four rows: 14 taps; both passes carry two maps a packed-fp32 FMA), then writes S (optional) and A, B, C (when a gradient follows), and
//       one partial record per tile: sum W|x - y|, sum (x - y)^2, sum S over the tile's pixels, added over the
//       block in a fixed order (wave_reduce8, then the waves in order).
//   rm_loss_grad_kernel   stages A, B, C the same way, convolves them and writes
//       grad = W sign(x - y) s - ssim_weight inv_count (F(A) + 2 x F(B) + y F(C)),  s = l1_weight inv_count.
//       With ssim_weight == 0 it is the L1 seed alone, the bits rm_train_step forms.
// LDS: the staged rows are kLossSS floats apart and the horizontal sums kLossHS, both odd multiples apart mod 4: a
// 32-lane group of the horizontal pass is 8 pixel groups (12 floats apart: banks 0, 12, 24, 4, ...) x 4 rows, which
// then fall on 32 different banks for every tap, reads and writes alike; the vertical pass reads consecutive
// columns. 12.3 / 13.5 K floats a block: three blocks a CU.
//   rm_loss_view_sums     one wave per view adds the view's partial records in tile order in fp64 and rounds once
//       (view_stats); rm_loss_total adds the views in order, also fp64, and writes the loss.
// No floating-point atomics; an output's bits do not depend on which other outputs are asked for.
#pragma once

constexpr int kLossR = 5;                                // the window's radius
constexpr int kLossTW = 32, kLossTH = 8;                 // pixels of a tile
constexpr int kLossCols = 3 * kLossTW;                   // float columns of a tile row
constexpr int kLossSW = 3 * (kLossTW + 2 * kLossR);      // staged floats of a row (with the halo)
constexpr int kLossRows = kLossTH + 2 * kLossR;          // staged rows
constexpr int kLossSS = 131;                             // LDS stride of a staged row (>= kLossSW, 3 mod 4)
constexpr int kLossHS = 97;                              // LDS stride of a row of horizontal sums (>= kLossCols, 1 mod 4)
constexpr int kLossThreads = 2 * kLossCols;              // a lane per column and half tile in the vertical pass
constexpr int kLossOut = kLossTH / 2;                    // output rows of a lane
constexpr int kLossTaps = 2 * kLossR + 1;
constexpr int kLossPart = 4;                             // floats of a tile's partial record (3 used)
static_assert(kLossSS >= kLossSW && kLossSS % 4 == 3 && kLossHS >= kLossCols && kLossHS % 4 == 1, "bank layout");
static_assert(kLossRows % 2 == 0 && kLossThreads == 192, "three waves");

struct LossArgs {
  const float* x;        // rendered [V, H, W, 3]
  const float* y;        // targets
  int H, W;
  int tiles_x, tiles_y;  // of a view
  float c1, c2;
  float progress;        // the background weight is 1 + 4 progress
  int plain_l1;          // W = 1
  float l1_scale;        // l1_weight * inv_count
  float ssim_scale;      // -ssim_weight * inv_count; 0: the gradient kernel convolves nothing
  float* S;              // stats: nullable
  float* A;              // stats: nullable (with B, C); grad: the inputs
  float* B;
  float* C;
  float* partials;       // stats: [V * tiles][kLossPart]
  float* grad;           // grad
};

// g(k), k = 0 .. 10: exp(-(k - 5)^2 / 4.5) normalised in fp64, rounded to float
__device__ __forceinline__ float loss_tap(int k) {
  constexpr float g[kLossTaps] = {0.0010283800844791101f, 0.007598758135239185f, 0.036000772128430829f,
                                  0.10936068950970002f,   0.21300553771125369f,  0.26601172486179436f,
                                  0.21300553771125369f,   0.10936068950970002f,  0.036000772128430829f,
                                  0.007598758135239185f,  0.0010283800844791101f};
  return g[k];
}

// compute_loss's weight of a pixel from its target (rm_ray.h forms the same bits)
__device__ __forceinline__ float loss_weight(const LossArgs& a, float t0, float t1, float t2) {
  if (a.plain_l1) return 1.0f;
  return (t0 + t1 + t2) > 0.01f ? 10.0f : fmaf(a.progress, 4.0f, 1.0f);
}

struct LossTile {
  int view, row0, col0;  // the tile's first pixel
};
__device__ __forceinline__ LossTile loss_tile(const LossArgs& a) {
  const int tpv = a.tiles_x * a.tiles_y;
  const int v = (int)(blockIdx.x / (unsigned)tpv), t = (int)(blockIdx.x - (unsigned)v * (unsigned)tpv);
  const int ty = t / a.tiles_x;
  return LossTile{v, ty * kLossTH, (t - ty * a.tiles_x) * kLossTW};
}

// The tile of each src[m] with its halo into dst[m][kLossRows][kLossSS]; zeros outside the image. Every load of
// the lane (12 an array) is issued before the first LDS write waits for one: the global latency is paid once.
template <int NA>
__device__ __forceinline__ void loss_stage(const float* const (&src)[NA], const LossArgs& a, const LossTile& t,
                                           float* const (&dst)[NA]) {
  constexpr int kTotal = kLossRows * kLossSW, kPer = (kTotal + kLossThreads - 1) / kLossThreads;
  const long long view0 = (long long)t.view * a.H;
  const int fcol0 = 3 * (t.col0 - kLossR), fw = 3 * a.W;
  float v[NA][kPer];
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int i = threadIdx.x + k * kLossThreads;
    const int r = i / kLossSW, j = i - r * kLossSW;
    const int grow = t.row0 - kLossR + r, gcol = fcol0 + j;
    const bool in = i < kTotal && grow >= 0 && grow < a.H && gcol >= 0 && gcol < fw;
    const long long idx = (view0 + grow) * fw + gcol;
#pragma unroll
    for (int m = 0; m < NA; ++m) {
      v[m][k] = 0.0f;
      if (in) v[m][k] = src[m][idx];
    }
  }
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int i = threadIdx.x + k * kLossThreads;
    const int r = i / kLossSW, j = i - r * kLossSW;
    if (i < kTotal) {
#pragma unroll
      for (int m = 0; m < NA; ++m) dst[m][r * kLossSS + j] = v[m][k];
    }
  }
}

// Horizontal-pass item i of a block: pixel group g (4 pixels), channel ch, staged row `row`. 32 consecutive
// items are 8 groups x 4 rows of one channel. False past the last row.
__device__ __forceinline__ bool loss_hitem(int i, int& g, int& ch, int& row) {
  g = i & 7;
  const int rest = i >> 5;
  ch = rest % 3;
  row = (rest / 3) * 4 + ((i >> 3) & 3);
  return row < kLossRows;
}
constexpr int kLossHItems = (kLossRows + 3) / 4 * 4 * 24;

// The vertical pass of one map for a lane's column: kLossOut outputs from kLossOut + 10 rows of horizontal sums.
__device__ __forceinline__ void loss_vpass(const float* h, int col, int half, float (&out)[kLossOut]) {
  const float* p = h + (half * kLossOut) * kLossHS + col;
  float v[kLossOut + 2 * kLossR];
#pragma unroll
  for (int k = 0; k < kLossOut + 2 * kLossR; ++k) v[k] = p[k * kLossHS];
#pragma unroll
  for (int o = 0; o < kLossOut; ++o) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < kLossTaps; ++k) acc = fmaf(loss_tap(k), v[o + k], acc);
    out[o] = acc;
  }
}

// Two maps at once, as packed fp32 (v_pk_fma_f32: the bits of two scalar chains at one issue slot each tap).
__device__ __forceinline__ void loss_vpass2(const float* h0, const float* h1, int col, int half, f2 (&out)[kLossOut]) {
  const int off = (half * kLossOut) * kLossHS + col;
  f2 v[kLossOut + 2 * kLossR];
#pragma unroll
  for (int k = 0; k < kLossOut + 2 * kLossR; ++k) v[k] = f2{h0[off + k * kLossHS], h1[off + k * kLossHS]};
#pragma unroll
  for (int o = 0; o < kLossOut; ++o) {
    f2 acc = sp(0.0f);
#pragma unroll
    for (int k = 0; k < kLossTaps; ++k) acc = fma2(sp(loss_tap(k)), v[o + k], acc);
    out[o] = acc;
  }
}

__global__ __launch_bounds__(kLossThreads) void rm_loss_stats_kernel(const LossArgs a) {
  __shared__ float sx[kLossRows * kLossSS];
  __shared__ float sy[kLossRows * kLossSS];
  __shared__ float hs[5][kLossRows * kLossHS];
  __shared__ float wsum[3][4];
  const LossTile t = loss_tile(a);
  const int tid = threadIdx.x;
  {
    const float* const src[2] = {a.x, a.y};
    float* const dst[2] = {sx, sy};
    loss_stage<2>(src, a, t, dst);
  }
  __syncthreads();

  // ---- horizontal pass: F_h(x), F_h(y), F_h(x^2), F_h(y^2), F_h(xy)
  for (int i = tid; i < kLossHItems; i += kLossThreads) {
    int g, ch, row;
    if (!loss_hitem(i, g, ch, row)) continue;
    const int base = row * kLossSS + 12 * g + ch;
    f2 P[14], Q[14];  // (x, y), (x^2, y^2)
    float xy[14];
#pragma unroll
    for (int m = 0; m < 14; ++m) {
      P[m] = f2{sx[base + 3 * m], sy[base + 3 * m]};
      Q[m] = P[m] * P[m];
      xy[m] = P[m].x * P[m].y;
    }
    const int ob = row * kLossHS + 12 * g + ch;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      f2 s01 = sp(0.0f), s23 = sp(0.0f);
      float s4 = 0.0f;
#pragma unroll
      for (int k = 0; k < kLossTaps; ++k) {
        const float w = loss_tap(k);
        s01 = fma2(sp(w), P[o + k], s01);
        s23 = fma2(sp(w), Q[o + k], s23);
        s4 = fmaf(w, xy[o + k], s4);
      }
      hs[0][ob + 3 * o] = s01.x;
      hs[1][ob + 3 * o] = s01.y;
      hs[2][ob + 3 * o] = s23.x;
      hs[3][ob + 3 * o] = s23.y;
      hs[4][ob + 3 * o] = s4;
    }
  }
  __syncthreads();

  // ---- vertical pass: a lane owns column `col` and rows half * kLossOut ... of the tile
  const int col = tid % kLossCols, half = tid / kLossCols;
  f2 mu[kLossOut], f2nd[kLossOut];  // (F(x), F(y)), (F(x^2), F(y^2))
  float fxy[kLossOut];
  loss_vpass2(hs[0], hs[1], col, half, mu);
  loss_vpass2(hs[2], hs[3], col, half, f2nd);
  loss_vpass(hs[4], col, half, fxy);
  const int fw = 3 * a.W, gcol = 3 * t.col0 + col, pix = col / 3;
  float l1 = 0.0f, sq = 0.0f, ss = 0.0f;
#pragma unroll
  for (int o = 0; o < kLossOut; ++o) {
    const int r = half * kLossOut + o, grow = t.row0 + r;
    if (grow >= a.H || gcol >= fw) continue;
    const float mx = mu[o].x, my = mu[o].y;
    const float vx = f2nd[o].x - mx * mx, vy = f2nd[o].y - my * my, cxy = fxy[o] - mx * my;
    const float n1 = fmaf(2.0f * mx, my, a.c1), n2 = fmaf(2.0f, cxy, a.c2);
    const float d1 = fmaf(mx, mx, fmaf(my, my, a.c1)), d2 = vx + vy + a.c2;
    const float i1 = 1.0f / d1, i2 = 1.0f / d2, inv = i1 * i2;
    const float S = n1 * n2 * inv;
    const long long idx = ((long long)t.view * a.H + grow) * fw + gcol;
    if (a.S) a.S[idx] = S;
    if (a.A) {
      const float Bq = -S * i2, Cq = 2.0f * n1 * inv;
      const float dmu = 2.0f * my * n2 * inv - 2.0f * mx * S * i1;
      a.A[idx] = dmu - 2.0f * mx * Bq - my * Cq;
      a.B[idx] = Bq;
      a.C[idx] = Cq;
    }
    const int c0 = (r + kLossR) * kLossSS + 3 * kLossR;  // the tile row's first float in the staged rows
    const float df = sx[c0 + col] - sy[c0 + col];
    const float Wt = loss_weight(a, sy[c0 + 3 * pix], sy[c0 + 3 * pix + 1], sy[c0 + 3 * pix + 2]);
    l1 = fmaf(fabsf(df), Wt, l1);
    sq = fmaf(df, df, sq);
    ss += S;
  }

  // ---- the tile's partial record: the lanes of a wave, then the three waves in order
  const int lane = tid & 63, wave = tid >> 6;
  const float vals[8] = {l1, sq, ss, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  const float red = wave_reduce8(vals, lane);
  if ((lane & 7) == 7 && (lane >> 3) < 3) wsum[wave][lane >> 3] = red;
  __syncthreads();
  if (tid < 3) a.partials[(long long)blockIdx.x * kLossPart + tid] = wsum[0][tid] + wsum[1][tid] + wsum[2][tid];
}

__global__ __launch_bounds__(kLossThreads) void rm_loss_grad_kernel(const LossArgs a) {
  __shared__ float sm[3][kLossRows * kLossSS];
  __shared__ float hs[3][kLossRows * kLossHS];
  const LossTile t = loss_tile(a);
  const int tid = threadIdx.x;
  const int col = tid % kLossCols, half = tid / kLossCols;
  const bool ssim = a.ssim_scale != 0.0f;  // uniform
  f2 fab[kLossOut];  // (F(A), F(B))
  float fc[kLossOut];
  if (ssim) {
    {
      const float* const src[3] = {a.A, a.B, a.C};
      float* const dst[3] = {sm[0], sm[1], sm[2]};
      loss_stage<3>(src, a, t, dst);
    }
    __syncthreads();
    for (int i = tid; i < kLossHItems; i += kLossThreads) {
      int g, ch, row;
      if (!loss_hitem(i, g, ch, row)) continue;
      const int base = row * kLossSS + 12 * g + ch, ob = row * kLossHS + 12 * g + ch;
      f2 ab[14];
      float cv[14];
#pragma unroll
      for (int k = 0; k < 14; ++k) {
        ab[k] = f2{sm[0][base + 3 * k], sm[1][base + 3 * k]};
        cv[k] = sm[2][base + 3 * k];
      }
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        f2 s01 = sp(0.0f);
        float s2 = 0.0f;
#pragma unroll
        for (int k = 0; k < kLossTaps; ++k) {
          s01 = fma2(sp(loss_tap(k)), ab[o + k], s01);
          s2 = fmaf(loss_tap(k), cv[o + k], s2);
        }
        hs[0][ob + 3 * o] = s01.x;
        hs[1][ob + 3 * o] = s01.y;
        hs[2][ob + 3 * o] = s2;
      }
    }
    __syncthreads();
    loss_vpass2(hs[0], hs[1], col, half, fab);
    loss_vpass(hs[2], col, half, fc);
  }
  const int fw = 3 * a.W, gcol = 3 * t.col0 + col, pix3 = 3 * (col / 3);
  if (gcol >= fw) return;
#pragma unroll
  for (int o = 0; o < kLossOut; ++o) {
    const int grow = t.row0 + half * kLossOut + o;
    if (grow >= a.H) continue;
    const long long row_idx = ((long long)t.view * a.H + grow) * fw;
    const long long idx = row_idx + gcol, p0 = row_idx + 3 * t.col0 + pix3;
    const float xv = a.x[idx], yv = a.y[idx];
    const float Wt = loss_weight(a, a.y[p0], a.y[p0 + 1], a.y[p0 + 2]);
    const float df = xv - yv;
    const float sg = df > 0.0f ? 1.0f : (df < 0.0f ? -1.0f : 0.0f);
    float gr = Wt * sg * a.l1_scale;
    if (ssim) gr = fmaf(a.ssim_scale, fmaf(yv, fc[o], fmaf(2.0f * xv, fab[o].y, fab[o].x)), gr);
    a.grad[idx] = gr;
  }
}

// The view's partial records in tile order, fp64, rounded once. One wave per view: 64 records are loaded at a
// time, lanes 0..2 add them in order.
__global__ __launch_bounds__(64) void rm_loss_view_sums(const float* __restrict__ partials, int tpv,
                                                        double* __restrict__ vsum, float* __restrict__ view_stats) {
  __shared__ double buf[3][64];
  const int lane = threadIdx.x;
  const long long first = (long long)blockIdx.x * tpv;
  double acc = 0.0;
  for (int b0 = 0; b0 < tpv; b0 += 64) {
    const int b = b0 + lane;
#pragma unroll
    for (int s = 0; s < 3; ++s) buf[s][lane] = b < tpv ? (double)partials[(first + b) * kLossPart + s] : 0.0;
    __syncthreads();
    if (lane < 3) {
      const int n = min(64, tpv - b0);
      for (int i = 0; i < n; ++i) acc += buf[lane][i];
    }
    __syncthreads();
  }
  if (lane < 3) {
    vsum[(long long)blockIdx.x * 3 + lane] = acc;
    if (view_stats) view_stats[(long long)blockIdx.x * 3 + lane] = (float)acc;
  }
}

// loss = inv_count (l1_weight sum W|x - y| + ssim_weight (count - sum S)): the views in order, fp64.
__global__ void rm_loss_total(const double* __restrict__ vsum, int V, double count, float l1_weight, float ssim_weight,
                              float inv_count, float* __restrict__ loss) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double l1 = 0.0, ss = 0.0;
  for (int v = 0; v < V; ++v) {
    l1 += vsum[(long long)v * 3];
    ss += vsum[(long long)v * 3 + 2];
  }
  *loss = (float)((double)inv_count * ((double)l1_weight * l1 + (double)ssim_weight * (count - ss)));
}
