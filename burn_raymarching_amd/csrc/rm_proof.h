// rm_proof.h -- the escape proof of the unsplit march as numbers: its sizes, its allowances (the margin ledger)
// and R'. No kernel. Included by rm_kernels.hip inside namespace rm, just before rm_records.h; the code that
// argues with these numbers is write_bound (rm_records.h), wave_escaped and bound_proof (rm_ray.h) and
// tile_proven (rm_sdf.h), the host's policy is rm_launch.h's section "the escape proof", and
// tests/escape_ref.py restates all of it on the CPU under the same names (tests/test_source_guards.py keeps
// the two in step). DESIGN.md §4.2 (iii) has the argument and the measurements.
#pragma once

// ---- sizes ------------------------------------------------------------------------------------------------
// The escape proof runs from kProofMinSpheres (padded) spheres on: a bound step costs about a tenth of a real
// march step at 64 spheres, and the C2 shape (256x256, 64 spheres, 10 views) ran 1.6 % slower with the proof.
// A call without the proof (KArgs::proof, proof_tier) launches the kernel instance without it, and its record
// kernel skips the soft-radius pass: R_soft = R + ln(M)/k, the ball's bound.
constexpr int kProofMinSpheres = 128;
// The escape lattice of the camera-mode proof (rm_tile_proof_kernel, bound_proof; KArgs::lattice): kLatticeN^3
// cells over the cube of half-side R' + kLatticeMargin about c_0. Sized by tools/escape_proof_sim.py on the
// bench scene after 35 optimizer steps (profiles/r19_escape_lattice_sim.txt): 64 cells save 26.7 % of the
// march's packed column blocks where the soft ball alone saves 2.9 %; 96 / 128 add 2 / 4 points for 3.4 / 8
// times the fill and a table of 3.5 / 8 MB against the 4 MB L2; the margin hardly matters (0.1 / 0.25 / 0.5:
// 27.0 / 26.7 / 25.7 %).
constexpr int kLatticeN = 64;
constexpr float kLatticeMargin = 0.25f;
// the net bound step at or below which a proof gives its wave up (not 0: a ray creeping along the ball is not
// proven in the steps left either, tools/escape_proof_sim.py). What a proof tries changes no result.
constexpr float kProofMinStep = 0.02f;

// ---- the margin ledger ------------------------------------------------------------------------------------
// Every allowance of the proof, once. The three readers:
//   ball   bound_proof's soft ball,            L = |p - c_0| - rs                               (fp32, per ray)
//   cell   bound_proof's per-ray lattice cell, L = max(ball, G[cell] - slack - kBallAbs)        (fp32, per ray)
//   tile   tile_proven's cone,                 L = max(ball, max_n G[n] - |p - x_n| (1 + kTileLatticeRel)
//                                                  - kTileLatticeAbs) - |u| delta               (fp64 / fp32, per tile)
// with R' = (R + ln(M)/k + kMarchAbs) (1 + kRadiusRel) and rs = (R_soft + kMarchAbs) (1 + kRadiusRel) +
// kBoundStepAbs. The allowances are doubles so that tests/escape_ref.py's are the same numbers; fp32 code
// converts at the use, (float)kMarchAbs == 1e-3f. All of them lean on one magnitude bound: a proof is tried
// only where B = |o|_1 + |c_0|_1 + 3 T(0) <= kProofMaxMagnitude (the bound march stops within a step of
// distance T(0), and a step at most doubles the distance), so every value in it is at most 256 and one fp32
// rounding at most 256 x 6e-8 = 1.5e-5.
//
//   allowance           value   charged by         covers
//   kMarchAbs           1e-3    R'; ball cell tile the fp32 rounding of the real rays' march at any |p| (in R',
//                                                  with wave_escaped's kEscapeRel) and so in rs: the bound must
//                                                  stay behind the march as computed, not the exact one
//   kBoundStepAbs       1e-3    ball cell tile     a bound step's own rounding, per step: five fp32 roundings
//                                                  below 1.5e-5 each at B, 1e-4 in all (tile: fp64, far less)
//   kRadiusRel          1e-6    R'; ball cell tile the fp32 sums that form R' and rs (three roundings, 2e-7)
//   kEscapeRel          1e-5    wave_escaped       dist of the march's own escape test: fsqrt and two fmas
//   kProofRel           2e-5    ball cell tile     the same test on the bound point: kEscapeRel and the bound
//                                                  point's own dist (tile: as the factor kProofDistUp on T)
//   kProofMaxMagnitude  256     ball cell tile     the guard that makes the absolute allowances enough
//   kLatticeHalfDiag    sqrt(3)/2       cell       a point of a cell is at most h sqrt(3)/2 from its centre
//   kLatticeCellRel     1e-4            cell       the cell index: (e + half) / h has three roundings, below
//                                                  3e-7 N cells in all, so a point rounded into a neighbouring
//                                                  cell is within (1/2 + 2e-5) h of that centre per axis; and
//                                                  kLatticeHalfDiag's own shortfall of 4e-9
//   kLatticeKernelAbs   1e-3            cell tile  rm_lattice_kernel's fp32: its cell centres origin + i h (three
//                                                  roundings at B, 5e-5 per axis), its direct-form distances (one
//                                                  rounding of e at B, 3e-5; root and sum 1e-6 relative of a
//                                                  distance below 2 B) and its logarithm (1e-6 / kappa)
//   kTileRootRel        1e-6                 tile  a v_sqrt_f32 of an fp64 sum rounded to fp32 (6e-8 + 1.2e-7),
//                                                  each root taken to the safe side (sqrt_up, sqrt_down);
//                                                  kTileRootFloor for an argument fp32 flushes to 0
//   kTileLatticeRel     2e-6                 tile  |p - x_n| in fp32: the sum of squares, the root and the last
//                                                  product (4e-7)
//   kTileRoundAbs       1e-4                 tile  p rounded to fp32 (1.5e-5 per axis at B) and the difference
//                                                  g - |q| (below 6e-5 at B)
//   kTileConeRel, Abs   1e-4, 2e-6           tile  delta: the tile's other rays' fp32 directions lie within 2e-7
//                                                  of the exact quadrilateral the corner rays span
//   kTileRecedeRel      2e-6                 tile  u |d_r|^2 of the receding test: fp32 directions are unit to
//                                                  1e-6, taken to the side that makes the term smaller
// The cell reader's slack is formed once per call (write_bound: h kLatticeHalfDiag (1 + kLatticeCellRel) +
// kLatticeKernelAbs, in Lat::kSlack), the sums below are what a reader adds on top. The tile reader's cell
// index is fp32 and carries no allowance: every lattice point gives a valid bound.
constexpr double kMarchAbs = 1e-3;
constexpr double kBoundStepAbs = 1e-3;
constexpr double kRadiusRel = 1e-6;
constexpr double kEscapeRel = 1e-5;
constexpr double kProofRel = 2e-5;
constexpr double kProofMaxMagnitude = 256.0;
constexpr double kLatticeHalfDiag = 0.8660254;
constexpr double kLatticeCellRel = 1e-4;
constexpr double kLatticeKernelAbs = 1e-3;
constexpr double kTileRootRel = 1e-6;
constexpr double kTileRootFloor = 1e-15;
constexpr double kTileLatticeRel = 2e-6;
constexpr double kTileRoundAbs = 1e-4;
constexpr double kTileConeRel = 1e-4;
constexpr double kTileConeAbs = 2e-6;
constexpr double kTileRecedeRel = 2e-6;
// derived: the two absolute allowances of rs (the cell reader takes them off G[cell] as well); everything
// absolute on the tile reader's lattice term; 1 / (1 - kProofRel) rounded up, a literal (its division is not
// the kernel's to redo per step, and another rounding of it would move the kernel)
constexpr double kBallAbs = kMarchAbs + kBoundStepAbs;
constexpr double kTileLatticeAbs = kMarchAbs + kBoundStepAbs + kLatticeKernelAbs + kTileRoundAbs;
constexpr double kProofDistUp = 1.0000200005;
static_assert(kProofDistUp * (1.0 - kProofRel) >= 1.0 && kProofDistUp < 1.0 + 1.01 * kProofRel,
              "T kProofDistUp >= T / (1 - kProofRel), and no more than it has to be");
static_assert(kLatticeHalfDiag * (1.0 + kLatticeCellRel) > 0.86602540379 * (1.0 + 4e-5),
              "the slack's factor covers sqrt(3)/2 and the cell index's (1/2 + 2e-5) h per axis");
static_assert(kProofRel >= 2.0 * kEscapeRel && kTileLatticeAbs >= kBallAbs + kLatticeKernelAbs,
              "the bound point's test holds the march's own; the tile's lattice term charges what the cell's does");

// R' = R + ln(M)/k + the march's allowance, rounded up: the radius about c_0 outside which every step of the
// real march is at least dist - R' long. One definition for the threshold table and the lattice's cube
// (write_bound) and for the gone rays' step (rm_ray_kernel): they must agree to the bit.
__device__ __forceinline__ float proof_rprime(float R, float lse_slack) {
  return (R + lse_slack + (float)kMarchAbs) * (1.0f + (float)kRadiusRel);
}
