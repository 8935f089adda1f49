// rm_ray.h -- the fused per-ray kernel (rm_ray_kernel), included by rm_kernels.hip after rm_records.h
// and the sweeps and helpers it is built from: the continuation state's layout (ContState), the record
// binding plus LDS scratch (bind_lds) and the backward's small helpers, then ray_entry / rm_ray_kernel and ray_body.
// ray_body runs the phases of DESIGN.md §4.2 in order -- block setup, march, continuation save /
// restore, post-march forward, seeds, hand-off, backward -- as one function whose phases are lambdas
// over its locals: the kernels sit at their register budget (117-123 of 128 VGPRs, SGPRs spilled
// to lanes), and moving a phase that carries control flow, or the clamp dispatch, into a function
// of its own changed the register allocation of some instance each time it was tried
// (profiles/r13_resource_usage.txt). What is a function here kept every instance's registers.
#pragma once

// The continuation state of a split launch, KArgs::cont_state (see KArgs::cont_cap): kRayRows
// per-ray rows of cont_rays floats, then kGroupWords words per group. The one place that knows the
// layout, for the kernel and for the host's buffer size.
struct ContState {
  enum Row { kT = 0, kLb, kDprev, kCycT1, kCycT2, kCode, kRhoLb, kRhist, kRayRows };
  static constexpr int kGroupWords = 2;  // the group's choice history and its steps saved (as int bits)
  // what a ray saves at a cap: t, lb, D_prev, t one and two steps back, gone / retired (the code:
  // 0 marching, 1 gone, 2 retired), rho_lb and the ray's own choice history (as int bits)
  struct Ray {
    float t, lb, Dprev, cyc_t1, cyc_t2, rho_lb;
    int rhist;
    bool gone, retired;
  };
  float* cs;
  long long R;  // rays of the first launch
  __host__ __device__ static size_t floats(long long rays, long long groups) {
    return (size_t)(kRayRows * rays + kGroupWords * groups);
  }
  __device__ __forceinline__ explicit ContState(const KArgs& a) : cs(a.cont_state), R(a.cont_rays) {}
  __device__ __forceinline__ float& row(int r, long long li) const { return cs[r * R + li]; }
  __device__ __forceinline__ float& group(long long blk, int w) const { return cs[kRayRows * R + kGroupWords * blk + w]; }
  __device__ __forceinline__ static float code(const Ray& s) { return s.gone ? 1.0f : (s.retired ? 2.0f : 0.0f); }
  __device__ __forceinline__ Ray load(long long li) const {
    Ray s;
    s.t = row(kT, li);
    s.lb = row(kLb, li);
    s.Dprev = row(kDprev, li);
    s.cyc_t1 = row(kCycT1, li);
    s.cyc_t2 = row(kCycT2, li);
    const float gflag = row(kCode, li);
    s.gone = gflag == 1.0f;
    s.retired = gflag == 2.0f;
    s.rho_lb = row(kRhoLb, li);
    s.rhist = __float_as_int(row(kRhist, li));
    return s;
  }
  __device__ __forceinline__ void save(long long li, const Ray& s) const {
    row(kT, li) = s.t;
    row(kLb, li) = s.lb;
    row(kDprev, li) = s.Dprev;
    row(kCycT1, li) = s.cyc_t1;
    row(kCycT2, li) = s.cyc_t2;
    row(kCode, li) = code(s);
    row(kRhoLb, li) = s.rho_lb;
    row(kRhist, li) = __int_as_float(s.rhist);
  }
  // a listed ray's final state back into its group's rows: what the resume launch reads of it
  __device__ __forceinline__ void write_back(long long li, const Ray& s) const {
    row(kT, li) = s.t;
    row(kLb, li) = s.lb;
    row(kCode, li) = code(s);
    row(kRhoLb, li) = s.rho_lb;
  }
};

// The record pointers of the call (bind_records) and the kernel's LDS scratch.
__device__ __forceinline__ Lds bind_lds(const KArgs& a, unsigned char* smem) {
  Lds L = bind_records(a.rec_buf, a.Mpad);
  L.slots = reinterpret_cast<float*>(smem);
  L.misc = L.slots + kSlotBytes / sizeof(float);
  return L;
}

// ---- backward helpers --------------------------------------------------------------------------
// The sphere of a lane in the backward sweeps: sphere j of pair j / 2 from the records of
// rm_prep_kernel (R4 the buffer, R2 its blue pairs), past Mpad the padding sphere.
// COLOUR (sweep 1): r and the colour; else (sweep 2) k r.
struct LaneSphere {
  float gx = -2.0f * kPadCenter, gy = 0.0f, gz = 0.0f, cc = kPadCenter * kPadCenter;  // -2 c, |c|^2
  float kr = 0.0f, rr = 0.0f, cr = 0.0f, cg = 0.0f, cbl = 0.0f;
};
template <bool COLOUR>
__device__ __forceinline__ LaneSphere load_sphere(const float4* R4, const float2* R2, const RecLayout& lay, int j, int Mpad) {
  LaneSphere s;
  if (j < Mpad) {
    const int i = j >> 1;
    const bool h = (j & 1) != 0;
    const float4 A = R4[lay.pair(RecLayout::kP0, i)], B = R4[lay.pair(RecLayout::kP1, i)], R = R4[lay.pair(RecLayout::kP2, i)];
    s.gx = h ? A.y : A.x;
    s.gy = h ? A.w : A.z;
    s.gz = h ? B.y : B.x;
    s.cc = h ? B.w : B.z;
    if constexpr (COLOUR) {
      const float4 C3 = R4[lay.pair(RecLayout::kP3, i)];
      const float2 C4 = R2[i];
      s.rr = h ? R.w : R.z;
      s.cr = h ? C3.y : C3.x;
      s.cg = h ? C3.w : C3.z;
      s.cbl = h ? C4.y : C4.x;
    } else {
      s.kr = h ? R.y : R.x;
    }
  }
  return s;
}
// columns 0-3 of v added to sphere j's record columns (sweep 2 on top of sweep 1)
__device__ __forceinline__ void add_cols4(float* rec, int j, const float (&v)[8]) {
  float4* dst = reinterpret_cast<float4*>(rec + (long long)j * 8);
  float4 o = dst[0];
  o.x += v[0];
  o.y += v[1];
  o.z += v[2];
  o.w += v[3];
  dst[0] = o;
}

template <int MODE, bool CAM, bool SPLIT, bool PROOF>
__device__ __forceinline__ void ray_body(const KArgs& a);

// The per-ray kernel. Measurement build (-DRM_BLOCK_TRACE): every wave also records {start, end}
// (s_memrealtime, 100 MHz), its hardware slot (HW_ID | XCC_ID << 32), {logical block, launch
// position}, the times its march and its post-march forward ended and its march steps saved into
// a.btrace[kTraceWords * (blockIdx.x * kWaves + wave) ...] (tools/block_trace.py).
// SPLIT: the split march (RM_MARCH_SPLIT, KArgs::split). PROOF: the escape proof before the march
// (KArgs::proof; an instance of its own, so that a call without it runs the code it ran before).
template <int MODE, bool CAM, bool SPLIT, bool PROOF>
__device__ __forceinline__ void ray_entry(const KArgs& a) {
#ifdef RM_BLOCK_TRACE
  const unsigned long long t_begin = __builtin_amdgcn_s_memrealtime();
  ray_body<MODE, CAM, SPLIT, PROOF>(a);
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
  ray_body<MODE, CAM, SPLIT, PROOF>(a);
#endif
}
template <int MODE, bool CAM, bool SPLIT, bool PROOF = false>
__global__ __launch_bounds__(kBlock, SPLIT ? kSplitMinWaves : kMinWavesPerSimd) void rm_ray_kernel(const KArgs a) {
  static_assert(!PROOF || (!SPLIT && MODE != kRender), "the escape proof: unsplit training kernels");
  ray_entry<MODE, CAM, SPLIT, PROOF>(a);
}

// Split march (SPLIT): a block takes 64 rays (one 8x8 quadrant of a 16x16 tile in camera mode)
// and all four of its waves hold them; every march step each wave sums a quarter of the sphere
// row blocks on the matrix cores and the quarters are added in wave order (split_combine), so
// the four waves march in lockstep through identical decisions (shift, clamp, exit). After the
// march only wave 0 goes on (post-march forward, backward); the others end as escaped waves
// with zero contributions. A ray that marches every step then occupies four SIMDs instead of one.
template <int MODE, bool CAM, bool SPLIT, bool PROOF>
__device__ __forceinline__ void ray_body(const KArgs& a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Lds L = bind_lds(a, smem);

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
  // the wave that writes this ray's outputs and seeds its backward; SPLIT: all four waves run the post-march forward
  // (each over a quarter of the spheres, merged) and wave w seeds the backward of the group's rays
  // [w R / 4, (w + 1) R / 4) (R = kSplitRays; lanes past R carry copies and seed nothing)
  const bool own_rays = !SPLIT || (wave == 0 && lane < kSplitRays);

  const float kappa = a.k * kLog2e, nkappa = -kappa, inv_kappa = 1.0f / kappa;

  // ray (camera.rs:58-87 in camera mode)
  float o[3], d[3];
  int view;
  setup_ray<CAM>(a, ri, o, d, view);

  // ---- escape skip (RM_MARCH_SKIP_ESCAPED): a block whose rays all provably leave the scene
  // (rm_escape_kernel) gets out = 0 and zero gradients without marching -- exactly what the full
  // computation yields for them, since their silhouette mask is 0 in f32 (see escapes()).
  if (a.ocnt_z != nullptr && blockIdx.x == 0 && tid < kOrderLists) order_sets(a).cnt_z[tid * kOrderClsStride] = 0;
  if (a.esc_flags != nullptr && blk >= 0 && a.esc_flags[blk]) {
    if (a.stats != nullptr && tid == 0) atomicAdd(a.stats, 1ull);
    if (a.ocnt_w != nullptr && tid == 0) order_append(a, blk, 0);
    escaped_block<MODE>(a, L, blk, ri, valid, tid, lane, wave);
    return;
  }

  // Scene radius bounds from the record header: with r_min, a lower bound on the scene distance
  // proves rho_j = dist_j + r_j >= kSafeRho for every sphere, so max(q, 1e-6) cannot bind and
  // the sweeps may skip it (exactly the same results).
  const cf1_ptr hdr = rec_header(L, a.Mpad);
  const float rmin = hdr[Hdr::kRmin], rmax = hdr[Hdr::kRmax], spread = hdr[Hdr::kSpread];
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

  // soft-min scene SDF at one point (scene.rs:60-79 + sdf.rs:30-44); returns D, keeps (m, s)
  auto soft_min = [&](const float p[3], bool fast, float& m, float& s) {
    m = -INFINITY;
    s = 0.0f;
    if (fast)
      lse_point<false, kShiftMax>(p, L, a.Mpad / 2, nkappa, m, s);
    else
      lse_point<true, kShiftMax>(p, L, a.Mpad / 2, nkappa, m, s);
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
    // neither cheaper shift is admitted: the running maximum
    if (fast) lse_point<false, kShiftMax>(p, L, a.Mpad / 2, nkappa, m, s);
    else lse_point<true, kShiftMax>(p, L, a.Mpad / 2, nkappa, m, s);
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
  // slack + the march's allowance (proof_rprime, rm_proof.h)
  const float c0x = hdr[Hdr::kCx], c0y = hdr[Hdr::kCy], c0z = hdr[Hdr::kCz];
  const cf1_ptr esc_tab = (cf1_ptr)RecLayout::at<const char>(a.rec_buf, RecLayout(a.Mpad).esc());
  if (MODE == kBwd && a.t_in != nullptr) {
    t = a.t_in[ri];
  } else {
    // Escaped rays: receding from the scene's bounding sphere (c_0, R) with every later
    // soft-min >= |p - c_0| - R - ln(M)/k >= gone_d (the distance only grows along a
    // receding ray, so t keeps increasing); the reconnected point and the mask argument
    // are then >= gone_d too, where sigmoid(-msharp D) (or exp(-10 D^2)) is exactly 0 in
    // fp32: out = 0 and every gradient term is 0, whatever the remaining steps would give.
    // Margins: kEscapeRel relative + kMarchAbs cover the fp32 rounding of the march at any |p| (the ledger
    // of rm_proof.h). Each remaining step is >= dist - R' long and keeps the ray receding, so the distance
    // grows step by step (write_bound): with n steps left the ray is gone once
    // (1 - 1e-5) dist >= T(n) -- proven long before the ray gets there.
    // A gone ray (sticky) steps by that bound, dist - R', instead of its soft-min: the proof
    // holds for any steps >= the bound, so its outputs stay exactly 0, and it leaves the
    // wave's shift / clamp choices (far points would force the running-max vector sweep on
    // the whole wave: 48 % of the march steps at 4096 spheres / 128 steps). A wave whose
    // rays are all gone stops (a.early_exit). The same in every mode that builds the table,
    // exit on or off, so both give the same bits.
    const float rprime = proof_rprime(hdr[Hdr::kR], a.lse_slack);  // R' as in write_bound
    float gone_step = 0.0f;  // dist - R' of a gone ray at the current point
    auto wave_escaped = [&](int st, const float p[3]) {
      if (!(a.gone_d > 0.0f)) return false;
      const float ex = p[0] - c0x, ey = p[1] - c0y, ez = p[2] - c0z;
      const float Tn = esc_tab[min(a.steps - st, kEscTab - 1)];
      const float dist = fsqrt(fmaf(ez, ez, fmaf(ey, ey, ex * ex)));
      gone = gone || (!retired && fmaf(ez, d[2], fmaf(ey, d[1], ex * d[0])) >= 0.0f && dist * (1.0f - (float)kEscapeRel) >= Tn);
      gone_step = dist - rprime;
      if (a.early_exit && __all(gone || !valid)) {
        steps_saved += a.steps - st;
        return true;
      }
      return false;
    };
    // A gone ray's remaining bound steps from step `from` to the end (what the march would do):
    // where the march of its wave stops early but its rays' final states are used later (the cycle
    // exits; ray mode: the continuation caps and the listed rays' write-back) -- a gone ray's mask
    // is exactly 0 only where the bound steps end, not where it was proven
    auto gone_steps = [&](int from) {
      for (int k = from; k < a.steps; ++k) {
        const float q[3] = {fmaf(d[0], t, o[0]) - c0x, fmaf(d[1], t, o[1]) - c0y, fmaf(d[2], t, o[2]) - c0z};
        t = fminf(t + (fsqrt(fmaf(q[2], q[2], fmaf(q[1], q[1], q[0] * q[0]))) - rprime), kTMax);
      }
    };
    auto gone_finish = [&](int from) {
      if (gone && !retired) gone_steps(from);
    };
    // Escape proof by a lower-bound march (exact; PROOF: the unsplit training kernels with the exit on,
    // no per-ray t or debug output and at least kProofMinSpheres spheres; tried once, before the march's first loop step: a second try
    // inside the loop proves more waves but costs the loop more than it saves, HISTORY.md §3).
    // The step t <- t + D(p(t)) is monotone: D is 1-Lipschitz along the ray, so u <= t gives
    // u + D(p(u)) <= t + D(p(t)). With any L <= D the bound trajectory u <- u + L(p(u)), started at
    // the ray's t, therefore stays at or behind the ray step for step. Once the bound point recedes
    // from c_0 at distance >= T(steps left) so does the ray, at least as far out: wave_escaped's test
    // would hold for it at that step, and the ray ends gone. When that is proven for every ray of
    // the wave that is not gone already, the wave stops here as it would have stopped there, with the
    // same outputs (exactly 0). Otherwise nothing changes: a proven ray of a wave that marches on
    // is not marked gone (gone rays leave the wave's votes, which would change other rays' bits).
    // L = |p - c_0| - R_soft (soft_radius): the ball bound without the ln(M)/k that R' charges.
    // Margins: the ball reader of rm_proof.h's ledger -- rs carries the march's allowance as R' does and
    // another per bound step, the distance test takes kProofRel where wave_escaped takes kEscapeRel, and
    // the proof is tried only where the magnitude guard holds for every lane of the wave. A wave gives
    // up once a ray's bound step falls to kProofMinStep: what the proof tries changes no result.
    // Camera mode with the call's lattice (KArgs::lattice, march_policy). The soft ball needs spheres out of
    // the way in every direction; the lattice sees the gaps between them (once the optimizer has thrown a few
    // spheres outwards, R_soft covers all the rays thread through: profiles/r19_escape_lattice_sim.txt). It
    // enters in one of two places, the host's choice per launch (tile_proof_policy, rm_launch.h):
    // (a) Before this launch (KArgs::tile_proof bound). rm_tile_proof_kernel (rm_sdf.h) marches one bound
    // trajectory per wave tile, stepping by the larger of the soft ball and the lattice's bound, and leaves a
    // byte per wave: 1, every ray of the wave is proven gone, and the wave stops here, booking what
    // bound_proof books; 0, not known, and the wave runs bound_proof below, the soft ball alone -- the waves
    // taken are a superset of the soft ball's, and the lookup below is skipped by a wave-uniform branch.
    // (b) Here, per ray (KArgs::tile_proof null: rows order, where a wave is no pixel rectangle, and launches
    // too small to hide the pre-pass's chain): L = max(|p - c_0| - R_soft, G[cell] - slack)
    // inside the lattice's cube, the soft ball alone outside it. G[cell] is the soft-min at the cell's centre
    // x_c (rm_lattice_kernel) and D is 1-Lipschitz, so D(p) >= D(x_c) - |p - x_c|: a point of the cell is at
    // most the half-diagonal h sqrt(3)/2 from x_c.
    // Margins: the cell reader of rm_proof.h's ledger -- the slack write_bound formed (half-diagonal, cell
    // index, the lattice kernel's fp32) and kBallAbs, the soft ball's two absolute allowances, on top. The
    // maximum of two lower bounds is a lower bound; the give-up rule, the votes and steps_saved are the soft
    // ball's. Array mode keeps the soft ball alone.
    static_assert((kLatticeN & (kLatticeN - 1)) == 0, "the inside test takes a power of two");
    auto bound_proof = [&](int st) {
      // a wave vote: origins differ per lane (array mode; a wave across two views), and every lane
      // takes part in the votes below and must leave with the same answer (dead is wave-uniform)
      if (__any(!(onorm + fabsf(c0x) + fabsf(c0y) + fabsf(c0z) + 3.0f * esc_tab[0] <= (float)kProofMaxMagnitude))) return false;
      const float rs = (hdr[Hdr::kRsoft] + (float)kMarchAbs) * (1.0f + (float)kRadiusRel) + (float)kBoundStepAbs;
      // the lattice's geometry (write_bound): half-side, 1 / h and the slack with rs's two absolute allowances on top
      const bool lat = CAM && a.lattice != nullptr && a.tile_proof == nullptr;
      float lat_half = 0.0f, lat_inv_h = 0.0f, lat_slack = 0.0f;
      if constexpr (CAM) {
        if (lat) {
          const cf1_ptr lg = (cf1_ptr)RecLayout::at<const char>(a.rec_buf, RecLayout(a.Mpad).lattice());
          lat_half = lg[Lat::kHalf];
          lat_inv_h = lg[Lat::kInvH];
          lat_slack = lg[Lat::kSlack] + (float)kBallAbs;
        }
      }
      float u = t;
      bool proven = gone || !valid;
      for (int n = st; n < a.steps; ++n) {
        const float ex = fmaf(d[0], u, o[0]) - c0x, ey = fmaf(d[1], u, o[1]) - c0y, ez = fmaf(d[2], u, o[2]) - c0z;
        const float dist = fsqrt(fmaf(ez, ez, fmaf(ey, ey, ex * ex)));
        const float Tn = esc_tab[min(a.steps - n, kEscTab - 1)];
        proven = proven || (fmaf(ez, d[2], fmaf(ey, d[1], ex * d[0])) >= 0.0f && dist * (1.0f - (float)kProofRel) >= Tn);
        if (__all(proven)) {
          steps_saved += a.steps - st;
          return true;
        }
        float Lb = dist - rs;
        if constexpr (CAM) {
          if (lat) {
            // the cell per axis, floor((e + half) / h), from a coordinate held to [-1, N] (no conversion out
            // of range); inside the cube is decided on the integers, and a lane outside reads a clamped
            // cell whose value the select drops: one load per lane, no branch per lane
            constexpr float kN = (float)kLatticeN;
            const int ix = (int)__builtin_floorf(__builtin_amdgcn_fmed3f((ex + lat_half) * lat_inv_h, -1.0f, kN));
            const int iy = (int)__builtin_floorf(__builtin_amdgcn_fmed3f((ey + lat_half) * lat_inv_h, -1.0f, kN));
            const int iz = (int)__builtin_floorf(__builtin_amdgcn_fmed3f((ez + lat_half) * lat_inv_h, -1.0f, kN));
            const bool inside = (unsigned)(ix | iy | iz) < (unsigned)kLatticeN;
            const int cx = min(max(ix, 0), kLatticeN - 1), cy = min(max(iy, 0), kLatticeN - 1),
                      cz = min(max(iz, 0), kLatticeN - 1);
            const float g = a.lattice[(cz * kLatticeN + cy) * kLatticeN + cx];
            Lb = fmaxf(Lb, inside ? g - lat_slack : -INFINITY);
          }
        }
        if (__any(!proven && !(Lb > kProofMinStep))) return false;
        u += proven ? 0.0f : Lb;
      }
      return false;
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
        const float D0 = a.origin[RecTail::kD0 + view];
        rho_lb = a.origin[RecTail::kRhoLb + view];  // at the eye
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
      const ContState cs(a);
      const ContState::Ray s = cs.load(li);
      t = s.t;
      lb = s.lb;
      Dprev = s.Dprev;
      cyc_t1 = s.cyc_t1;
      cyc_t2 = s.cyc_t2;
      gone = s.gone;
      retired = s.retired;
      rho_lb = s.rho_lb;
      rhist = s.rhist;
      if (!a.ray_cont) {
        chist = __float_as_int(cs.group(blk, 0));
        steps_saved = __float_as_int(cs.group(blk, 1));
      }
      st0 = a.cont_resume;
    }
    if constexpr (PROOF) {  // the host's choice (march_policy): exit on, no debug output, kProofMinSpheres
      bool taken = false;  // wave-uniform: the tile proof's byte of this wave (a scalar load)
      if constexpr (CAM) {
        if (!dead && a.tile_proof != nullptr) taken = a.tile_proof[blk * kWaves + wave] != 0;
      }
      if (taken) {
        steps_saved += a.steps - st0;
        dead = true;
      } else if (!dead && bound_proof(st0)) {
        dead = true;
      }
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int st = st0; !dead && st < a.steps; ++st) {
      if (SPLIT && a.cont_cap > 0 && st == a.cont_cap) {
        // ray mode, defer at the top of this step: every ray's state, the marching rays to the
        // ray list; a group (not a ray_cont block) also to the resume list, its not-run steps
        // counted as saved now (the ray_cont blocks subtract the steps they run)
        const ContState cs(a);
        const bool act = valid && !gone && !retired && lane < kSplitRays;
        gone_finish(st);
        if (wave == 0 && lane < kSplitRays && valid)
          cs.save(li, ContState::Ray{t, lb, Dprev, cyc_t1, cyc_t2, rho_lb, rhist, gone, retired});
        if (wave == 0) {
          const unsigned long long am = __ballot(act);
          const int na = __popcll(am);
          int base = 0;
          if (lane == 0 && na > 0) base = atomicAdd(a.ray_count_w, na);
          base = __shfl(base, 0);
          if (act) a.ray_list_w[base + __popcll(am & below)] = (int)li;
          if (lane == 0) {
            if (!a.ray_cont) {
              cs.group(blk, 0) = __int_as_float(chist);
              cs.group(blk, 1) = __int_as_float(steps_saved + (a.steps - st));
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
            if (gone) gone_steps(st + 1);
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
            gone_steps(st + 1);
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
      if (st_stop >= 0) gone_finish(st_stop);
      if (wave == 0 && lane < kSplitRays && valid)
        ContState(a).write_back(li, ContState::Ray{t, lb, Dprev, cyc_t1, cyc_t2, rho_lb, rhist, gone, retired});
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
        lse_taps<false>(p, L, a.Mpad / 2, nkappa, 2.0f * eps, eps * eps, m6, s6);
      } else {
        lse_taps<true>(p, L, a.Mpad / 2, nkappa, 2.0f * eps, eps * eps, m6, s6);
      }
#pragma unroll
      for (int q = 0; q < 6; ++q) D6[q] = -(flog2(fmaxf(s6[q], 1e-30f)) + m6[q]) * inv_kappa;
      const float nx = D6[0] - D6[1], ny = D6[2] - D6[3], nz = D6[4] - D6[5];
      const float inv_len = frsq(fmaf(nz, nz, fmaf(ny, ny, fmaf(nx, nx, 1e-6f))));
      nrm[0] = nx * inv_len;
      nrm[1] = ny * inv_len;
      nrm[2] = nz * inv_len;
      if (fast_f)
        shade_sweep<false>(p, L, a.Mpad / 2, c10l, kappa, dmin, Zw2, C2, Zb2);
      else
        shade_sweep<true>(p, L, a.Mpad / 2, c10l, kappa, dmin, Zw2, C2, Zb2);
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
  if (valid && own_rays) {
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
    const RecLayout lay(a.Mpad);
    const float4* R4 = reinterpret_cast<const float4*>(a.rec_buf);
    const float2* R2 = reinterpret_cast<const float2*>(R4 + lay.p4_first());
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
        add_cols4(rec, j, acc);
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
          const LaneSphere S = load_sphere<true>(R4, R2, lay, j, a.Mpad);
          const f2 GX = sp(S.gx), GY = sp(S.gy), GZ = sp(S.gz), CC = sp(S.cc), RR = sp(S.rr), CR = sp(S.cr), CG = sp(S.cg),
                   CB = sp(S.cbl), HX = sp(0.5f * S.gx), HY = sp(0.5f * S.gy), HZ = sp(0.5f * S.gz);
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
          const LaneSphere S = load_sphere<false>(R4, R2, lay, j, a.Mpad);
          const f2 GX = sp(S.gx), GY = sp(S.gy), GZ = sp(S.gz), CC = sp(S.cc), KR = sp(S.kr), HX = sp(0.5f * S.gx),
                   HY = sp(0.5f * S.gy), HZ = sp(0.5f * S.gz);
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
            if (j < a.Mpad) add_cols4(rec, j, v);
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

