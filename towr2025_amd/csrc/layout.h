// layout.h — host-side problem builder for the HIP engine.
//
// Replaces, for the eval path, what the reference derives at setup in
//   NlpFormulation::GetVariableSets / GetConstraints (towr/src/nlp_formulation.cc:76-378),
//   NodesVariables*::GetPhaseBasedEEParameterization (nodes_variables_phase_based.cc:201-396),
//   TimeDiscretizationConstraint ctor (time_discretization_constraint.cc:37-50),
//   ifopt's Jacobian assembly (ConstraintSet::GetJacobian / setFromTriplets),
// and emits flat, batch-shared device tables: node->column map, polynomial durations, work items,
// CSR pattern, per-candidate slot table and LDS tiles.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "engine_math.h"

namespace tg {

struct TileDesc {
  int32_t i0, i1;   // items [i0, i1): exactly one item (or IT_NONE padding) per thread of the block
  int32_t r0, r1;   // rows  [r0, r1)
  int32_t v0, v1;   // values (CSR positions) [v0, v1)
  int32_t type, reserved;
};

// Wave w of small-kind group g (Layout::misc_tiles / misc_lds) as the device reads it: its tile's rows and values and
// its LDS offsets (ti -1: an empty wave), beside a copy of the tile's 64 items per (g, w) (towr_gpu.hip), so a block's
// descriptors are one load level instead of three (group -> tile -> items; tile_emit.h misc_body)
struct MiscWave {
  int32_t ti, r0, r1, v0, v1, wl_off, rows_off, reserved;
};

// Streaming composition of ForceConstraintDiscretized under phase-duration optimisation on a terrain
// without curvature (towr_gpu.hip fdisc_stream_body). One block per (problem, FsBlock) evaluates up to
// kFsInst instants once each (fdisc_instant), then writes the block's whole CSR range [v0, v0 + nv)
// — every 16-byte unit exactly once, zeros included — composing each entry from its instant's
// quantities. All rows of one constraint hold the same columns (checked): the force set's full
// PhaseSpline pattern and the schedule columns. Template entry j (fs_tmpl) = column j of a row:
//   >= 0: force column, PhaseCol index (bits 0-23) and dimension (bits 24-25); < 0: schedule column.
// The force entries polynomial p can make non-zero (its two nodes' variables) lie in the window
// [fs_ws[2 (wsoff + p)], + kFsWin) of row positions (checked); schedule columns at [js0, js0 + ns1).
#ifndef TOWR_FS_INST   // (experiment builds: -DTOWR_FS_INST)
#define TOWR_FS_INST 16
#endif
// measured on MI355X (ANYmal gait, B = 1024): 64 -> 0.501 ms, 32 -> 0.463, 16 -> 0.452, 8 -> 0.478 (round 3); with the
// round-5 composer (1 KB-aligned trips, 4 problems per block), step gait / + Torque: 16 0.584-0.593 / 1.144-1.152,
// 32 0.570-0.591 / 1.153-1.159, 8 0.638-0.650 / 1.203-1.205
constexpr int kFsInst = TOWR_FS_INST;
constexpr int kFsWin = 12;
// The composers (gstream.hip) find an entry's row (FsBlock) or instant (GsBlock) from its position e in the
// block's CSR range as (int)((e + 0.5f) * (1.0f / L)). The float product is within 2^-23 relative of
// (e + 0.5) / L, whose distance to the nearest integer is at least 0.5 / L; the result is exact while
// (e / L) 2^-23 < 0.5 / L, i.e. for e < 2^22. The layout keeps every block range below half that bound
// (build_fstream, build_gstream_class: fewer instants per block, or the tile path).
constexpr int kFloatDivMax = 1 << 21;
// FDISC record (gstream.hip fdisc_records -> the composer): S[kFsS] | b[5][3] | Jf.dx[3] | Jf.v[3] | ints ws, wd,
// cur, wq (two 32-bit ints per double, gs_int2). S = the basis sums of the force polynomial's active window in dimension 0;
// the three dimensions' windows hold PhaseCols of one structure (build_fstream checks it), so window position q
// holds S[slot q] (wq: 2 bits per position) times b[row][dim q] (wd: 2 bits per position, 3 = not an active column:
// 0). Round 5's record kept the 12 window positions' sums (36 fields instead of 29).
constexpr int kFsS = 4;   // = kGsAct (below)
constexpr int kFsB = kFsS, kFsDx = kFsS + 15, kFsV = kFsS + 18, kFsND = kFsS + 21;
constexpr int kFsRS = kFsND + 2, kFsCS = kFsRS | 1;   // record fields; LDS stride per instant
struct FsBlock {
  int32_t ee, n_inst, t0, r0;   // endeffector, instants, first instant's time index (fs_t), first row
  int32_t v0, nv, L, tmpl;      // CSR range [v0, v0 + nv), row length, template offset (fs_tmpl)
  int32_t js0, ns1, wsoff, pad;
};
static_assert(sizeof(FsBlock) % 4 == 0, "FsBlock is staged to LDS as int32 words");

// Streaming RangeOfMotion and Dynamic under phase-duration optimisation (gstream.hip), the FsBlock
// scheme generalised to rows whose columns differ by row type. Two launches per class:
//   record:  one block per problem, one lane per instant (Dynamic: per instant, per base-angular axis,
//            per (instant, endeffector)) evaluates the instant once and stores what every Jacobian
//            entry of its rows is a function of (the record, field-major in the handle's scratch);
//   compose: one block per (problem, GsBlock) streams the block's whole CSR range with 16-byte
//            stores, each unit written once, forming every entry from its instant's record and the
//            entry's position.
// Row r of an instant (its row type) is [base prefix | template]: the prefix holds the base-linear and
// base-angular columns of the instant's active base polynomials, coded per (instant, row) as
// blk << 4 | dim << 2 | basis (gs_pcode; the base node sets hold the smallest columns); the template is
// the same for every instant (checked) and codes each remaining column (gs_tmpl):
//   bit 31 set: schedule column, bits 16-18 endeffector, bits 0-15 column within its PhaseDurations;
//   else: a PhaseSpline column, bits 28-29 spline kind (0 motion, 1 force, 2 torque), 25-27
//   endeffector, 22-23 dimension, 0-21 PhaseCol index within that dimension's list.
// A PhaseSpline column is non-zero only in its instant's active window, at most kGsAct PhaseCols per
// dimension from the polynomial's first (pact); the composer's prologue forms their basis sums.
enum GsClass { GS_ROM = 0, GS_DYN = 1, GS_TQ = 2, GS_COUNT = 3 };   // GS_TQ: TorqueConstraintDiscretized (no base prefix)
constexpr int kGsRowTypes = 6;
constexpr int kGsAct = 4;
static_assert(kFsS == kGsAct, "the FDISC record's window sums are one active window");
// The composer launch (gstream.hip towr_gait_compose_kernel): the ForceConstraintDiscretized,
// RangeOfMotion and Dynamic compose blocks of every problem in one grid, kComposeBlock threads each.
// (experiment builds: -DTOWR_COMPOSE_BLOCK / -DTOWR_COMPOSE_BLOCK_RD. Round 5, ANYmal gait, B = 1024, one box, ms per step
// gait / + Torque: 512 / 256 0.606-0.619 / 1.163-1.174; FDISC composer 1024: 0.624-0.635 / 1.29; 256: 0.667-0.682 / 1.28;
// RangeOfMotion / Dynamic composer 512: 0.660-0.664 / 1.23; 128: 0.654-0.659 / 1.19)
#ifndef TOWR_COMPOSE_BLOCK
#define TOWR_COMPOSE_BLOCK 512
#endif
#ifndef TOWR_COMPOSE_BLOCK_RD
#define TOWR_COMPOSE_BLOCK_RD 256
#endif
constexpr int kComposeBlock = TOWR_COMPOSE_BLOCK;
constexpr int kComposeBlockRD = TOWR_COMPOSE_BLOCK_RD;   // a launch without FDISC blocks
inline int compose_block(int mask) { return (mask & 25) ? kComposeBlock : kComposeBlockRD; }
constexpr int kGsInstRom = 16;   // instants per compose block
constexpr int kGsInstTq = 16;
constexpr int kGsInstDyn = 2;   // measured on MI355X (ANYmal gait, B = 1024, grouped composer): 2 -> 0.201 ms, 4 -> 0.230, 8 -> 0.219
// A row type is cut into segments: its base prefix, each maximal run of template columns of one
// (spline kind, endeffector) or of one endeffector's schedule. Per instant a segment owns W values
// (GsSeg::vbase): the prefix and schedule segments all their positions, a PhaseSpline segment the
// window of W positions starting at ws(poly) (gs_ws[wsoff + poly], the active polynomial's first
// position in the segment); positions outside it are 0. The composer computes an instant's values once
// (one lane each), then every entry of the CSR range is one lookup: segment (gs_tseg, by position in
// the instant), window start, value.
// p0: first position in the instant; toff: gs_tmpl index = toff + position (prefix: gs_pcode index within the
// instant's codes = toff + position)
struct GsSeg { int8_t r, type, kind, ee; int16_t p0, len, W, vbase; int32_t wsoff, toff; };   // type 0 prefix, 1 window, 2 schedule
struct GsGeo {
  int32_t cls, ee, nrt, Li;   // class, endeffector (RangeOfMotion), row types, values per instant
  int32_t L[kGsRowTypes], P[kGsRowTypes], T[kGsRowTypes], poff[kGsRowTypes];   // per row type: length, prefix, template offset, prefix codes offset
  int32_t Psum, pc0, rec0, r0;   // prefix codes per instant, gs_pcode offset of instant 0, first record index, first row
  int32_t ns, seg0, vt, ts0;     // segments (gs_segs[seg0..]), values per instant, gs_tseg offset (Li bytes)
  int32_t vm0, K, blob0, blob_n16;   // gs_vmap offset (vt entries: segment << 16 | value index), instants,
                                     // the composer blob (gs_blob[blob0 ..], 16-byte units)
  int32_t o_vmap, o_tmpl, o_tseg, o_pcode, o_ws, reserved[3];   // byte offsets of its sections (segments at 0)
};
struct GsBlock { int32_t geo, k0, n_inst, v0, nv, reserved[3]; };   // instants [k0, k0 + n_inst) of the geometry
// a record lane's instant; kk / nb: its index in its GsBlock and the block's instants (the record chunk)
// p0: TorqueConstraintDiscretized's k_friction (ItemDesc::p0)
struct GsInst { double t; int32_t seg, row0; int16_t ee, kk, nb, reserved; double p0; };
// Records (gstream.hip gs_records): per instant RS fields, the composer's view of the instant —
// ND doubles then NI doubles of ints, two 32-bit ints per double (gs_int2; int j is dword j of that area) — so that a composer block's prologue is one contiguous
// copy. The fields of the GsBlock of instants [k0, k0 + n) form one chunk at RS * k0 (class-global
// instant index), field-major inside it (field f of instant k0 + kk at RS * k0 + f * n + kk).
//   RangeOfMotion: R[9] | HL[4] | Ag[axis][r] (9) | HA[4] | Jx.dx[3] v[3] | sums[dim][4] (12);
//                  ints cur | qa[dim] (3) | poly (3 doubles)
//   Dynamic:       fs[3] | Lp[3] | HpL[4] | HaL[4] | A[axis][p v a][r] (27) | HpA HvA HaA (12), then per
//                  endeffector Fp[3] | rv[3] | Jf.dx v[6] | Jx.dx v[6] | motion sums[dim][4] (12) | force sums[4] |
//                  torque sums[4]; ints per endeffector (6 doubles, each pair written by one record lane): curX | qaX[3] |
//                  polyX | - | curF | qaF | polyF | - | qaT | polyT (the force and torque windows start at one PhaseCol
//                  index in every dimension, spline_dims_coincide; round 5: 14 ints in 14 doubles). The force
//                  and torque sums are one set for the three dimensions, as TQDISC's below (the layout streams Dynamic
//                  only when they coincide, spline_dims_coincide): 38 doubles per endeffector instead of round 5's 54
//   TorqueConstraintDiscretized: t1[3] | t2[3] | n[3] | b[3] (= -k mu n) | Jt.dx v[6] | Jf.dx v[6] |
//                  torque sums[4] | force sums[4]; ints cur | qaT | qaF | polyT | polyF (3 doubles). The sums and qa are
//                  the same for the three dimensions (the layout streams TQDISC only when the torque and force
//                  splines' active windows hold PhaseCols of one structure in every dimension, spline_dims_coincide),
//                  so one set of 4 per spline: 35 fields instead of round 5's 57
//                  (torque_constraint_discretized.cc:139-235 without the motion block: a terrain
//                  without curvature, where every motion scale is exactly 0.0 and the block is skipped, :57)
// (kind 0 motion, 1 force, 2 torque; sums / qa: the active-window basis sums of the PhaseSpline, the
// first active PhaseCol of each dimension and the basis sums of up to kGsAct PhaseCols from it)
constexpr int kRomND = 44, kRomNI = 3;
constexpr int kDynBaseND = 53, kDynEeND = 38, kDynEeNI = 6;
// field of the window sum q of kind (0 motion, 1 force, 2 torque) and dimension e in a Dynamic record's endeffector part
TG_HD constexpr int dyn_sum_field(int kind, int e, int q) { return kind == 0 ? 18 + e * kGsAct + q : 26 + kind * kGsAct + q; }
constexpr int kTqND = 32, kTqNI = 3;
TG_HD constexpr int gs_rec_nd(int cls, int E) { return cls == GS_ROM ? kRomND : cls == GS_TQ ? kTqND : kDynBaseND + kDynEeND * E; }
TG_HD constexpr int gs_rec_ni(int cls, int E) { return cls == GS_ROM ? kRomNI : cls == GS_TQ ? kTqNI : kDynEeNI * E; }
TG_HD constexpr int gs_rec_fields(int cls, int E) { return gs_rec_nd(cls, E) + gs_rec_ni(cls, E); }
#ifndef TOWR_GS_GROUP   // (experiment builds: -DTOWR_GS_GROUP; round 5, one box, gait / + Torque / headline ms: 2 0.592-0.595 /
                        // 1.161-1.165 / 0.2365-0.2375; 1 0.620-0.629 / 1.276; 4 0.589-0.599 / 1.160-1.166 / 0.2364-0.2372;
                        // with the FDISC composer at 4 (towr_gpu.hip kFsGroup), the others at 4: 0.589-0.594 / 1.146-1.150
                        // vs 0.584-0.599 / 1.141-1.144, at 1: 0.600-0.601 / 1.160-1.166)
#define TOWR_GS_GROUP 2
#endif
constexpr int kGsGroup = TOWR_GS_GROUP;   // problems per composer block (gstream and fstream; 1 -> 0.333 ms, 2 -> 0.321, 8+ slower: a block
                              // waits for its stores to drain before the next problem's records land)
constexpr int kGsChunkMax = 2048;   // record doubles of a compose block (prefetched into registers: kGsChunkMax / kComposeBlock per thread)
// the RangeOfMotion / Dynamic records' arguments (gs_records)
struct GsRecArgs {
  double* rec;                 // per problem: RangeOfMotion records at 0, Dynamic records at dyn_off
  int64_t ldr, dyn_off;
  const GsInst* inst[GS_COUNT];
  int32_t K[GS_COUNT];         // instants per class (0: the class is not streamed)
  int32_t st_off, scr_off;     // LDS (doubles): the Dynamic states, the scratch (9 per instant, 9 per (ee, instant))
};

// Pattern watch (curved terrain): ForceConstraintDiscretized / TorqueConstraintDiscretized add their
// motion block of row i, dimension dim only where its scale is non-zero (force_constraint_discretized.cc:58,
// torque_constraint_discretized.cc:57), so the reference's pattern moves with x while IPOPT's structure
// (and the engine's CSR) is frozen at x0. One WatchItem per such instant: the x0 presence of each
// (dim, row) block and the entries a block holds; towr_gpu_pattern_outside counts, at any x, the
// reference entries outside the frozen pattern (blocks present at x, absent at x0), on the host.
struct WatchItem {
  double t, kf;           // instant; TorqueConstraintDiscretized's k_friction
  int32_t seg, type;      // segment-table row, IT_FDISC / IT_TQDISC
  int32_t ee, mask;       // endeffector; bit dim * rows + row: block present at x0
  int32_t cnt[2];         // entries of a block of dimension 0 / 1 (the motion spline's Jacobian row)
};

// a Dynamic instant of the RotVec coefficient pre-pass (fixed gait): its time and segment-table row
struct RvInst { double t; int32_t seg, reserved; };
constexpr int kRvCoef = 30;   // per instant: per component e, Mp[3] | Mv[3] | Ma[3] (dyn_rv_column); then the base terms ab[3]
constexpr int kRvAb = 27;     // (dyn_base_ab, read by the instant's group-0 lane)
// Scratch layout of the pre-pass: blocks of 64 (problem, instant) pairs pr = b K + q, field-major inside a block, so
// a wave's store of one field is 512 contiguous bytes and the kRvCoef fields of one pair sit in one 15 kB block
// (field-major over the whole batch put them 1.8 MB apart at B = 4096); field f of pair pr at rv_at(pr) + 64 f
__host__ __device__ constexpr int64_t rv_at(int64_t pr) { return (pr >> 6) * (int64_t)kRvCoef * 64 + (pr & 63); }

// Batched Jacobian products on the evaluated values (jprod.hip): Y_b = J_b p_b and Z_b (+)= J_b^T lam_b, one block
// per problem over fixed chunks of kJpChunk consecutive CSR entries. A chunk's products land in an LDS tile; each
// output that has entries in the chunk is one segment of it, summed in ascending order by one lane (short) or by one
// wave (len >= Layout::jp_long: lane l takes entries l, l + 64, ..., then a fixed shuffle tree):
//   J p:    a row's span of the tile (q0 = tile position). A row cut by a chunk boundary continues through a carry
//           (flags bit 0: add the carry of the chunk before; bit 1: the row goes on, store the carry, not Y);
//   J^T l:  a column's entries of the chunk, through the chunk-local by-column list Layout::jp_cidx (q0 = index
//           into it, rows ascending); the chunk's partial is added to the column's running sum in LDS.
// Chunks are visited in ascending order, so every output has one summation tree, whatever the batch.
constexpr int kJpChunk = 2048;
constexpr int kJpBlock = 256;
constexpr int kJpLongDefault = 32;
struct JpSeg { int32_t out, q0, len, flags; };
// segments [rs0, rs0 + rns) short rows then rnl long rows (jp_rseg); likewise columns (jp_cseg)
struct JpChunk { int32_t rs0, rns, rnl, cs0, cns, cnl, reserved[2]; };

struct VarSetInfo { int kind, ee, col0, n; };
struct ConsInfo { int kind, ee, row0, rows; };

// Constraint bounds (towr_gpu_constraint_bounds). ifopt's constants: inf = 1.0e20, NoBound = (-inf, +inf),
// BoundGreaterZero = (0, +inf), BoundSmallerZero = (-inf, 0); the literal, not IEEE infinity.
constexpr double kBoundInf = 1.0e20;
// A node TorqueConstraint's third row, (-L, L) with L = k mu (f . n) (torque_constraint.cc:103-127): the only bounds
// that depend on x and the terrain. pcol = the x columns of the foot position (x, y) and fcol = of the force at the
// start of the node's phase (-1: a constant node value, 0.0).
struct TqBound { int32_t row, pcol[2], fcol[3]; double k; };

// The residual kernel (resid.hip): per-problem violation summary of G against (GL, GU) and, with LAMP, the augmented
// Lagrangian's multiplier update; one block of kResBlock threads per problem. set_row0[s] .. set_row0[s + 1] are the
// rows of constraint set s (description order; a soft set's range is empty). ldb = 0: one bounds row for all problems.
// The host side of this and the following kernels (argument checks, handle tables, launches) is auglag.hip.
constexpr int kResBlock = 256;
struct ResArgs {
  const double* G; int64_t ldg;
  const double *GL, *GU; int64_t ldb;
  const double* LAM; int64_t ldl;
  double* LAMP; int64_t ldlp;
  double* SUM; int64_t lds;
  const int32_t* set_row0;   // n_sets + 1
  double rho;
  int32_t m, n_sets;
  const double* RHO;         // internal: one rho per problem (RHO[b]) instead of the scalar; NULL in every public entry
};
const void* res_kernel();

// The step kernel (step.hip): per problem XP = P_[XL, XU](X - a D) and the summary of the projected step s = XP - X
// (towr_gpu.h); one block of kStepBlock threads per problem. set_col0[s] .. set_col0[s + 1] are the columns of
// variable set s (AddVariableSet order). ldb = 0: one bounds row for all problems. ALPHA NULL: the scalar alpha.
constexpr int kStepBlock = 256;
struct StepArgs {
  const double* X; int64_t ldx;
  const double* D; int64_t ldd;
  const double* ALPHA; double alpha;
  const double *XL, *XU; int64_t ldb;
  double* XP; int64_t ldxp;
  double* SUM; int64_t lds;
  const int32_t* set_col0;   // n_sets + 1
  int32_t n, n_sets;
};
const void* step_kernel();

// The L-BFGS kernels (lbfgs.hip): the per-problem ring of (s, y) pairs and the two-loop recursion on the free columns
// (towr_gpu.h); one block of kLbfgsBlock threads per problem. Pair k of problem b starts at HS / HY + (b*mem + k)*ldh,
// HMETA[2b] = count, HMETA[2b + 1] = next. The kernels keep per-column state in dynamic LDS: lbfgs_update_lds(n) /
// lbfgs_direction_lds(n) bytes (the host side, auglag.hip, refuses an n whose state does not fit kLbfgsMaxLds).
constexpr int kLbfgsBlock = 256;
constexpr int64_t kLbfgsMaxLds = 60 * 1024;   // beside the kernels' static reduction buffers, within the default 64 KiB
inline int64_t lbfgs_update_lds(int n) { return 16 * (int64_t)n; }      // s and y
inline int64_t lbfgs_direction_lds(int n) { return 16 * (int64_t)n; }   // q / r and the pair's row kept for the update
struct LbfgsUpdateArgs {
  const double* X; int64_t ldx;
  const double* XN; int64_t ldxn;
  const double* GR; int64_t ldgr;
  const double* GRN; int64_t ldgrn;
  double *HS, *HY; int64_t ldh;
  int32_t* HMETA;
  double* SUM; int64_t lds;
  double curv_eps;
  int32_t n, mem;
};
struct LbfgsDirArgs {
  const double* X; int64_t ldx;   // NULL: every column is free
  const double* GR; int64_t ldgr;
  const double *XL, *XU; int64_t ldb;
  const double *HS, *HY; int64_t ldh;
  const int32_t* HMETA;
  double* D; int64_t ldd;
  double* SUM; int64_t lds;
  int32_t n, mem;
  const int32_t* RUN; int64_t run_stride;   // internal: a block whose RUN[b*run_stride] & 2 is zero returns at once (D and
                                            // SUM rows untouched); NULL in every public entry
};
const void* lbfgs_update_kernel();
const void* lbfgs_direction_kernel();

// The resident AL loop's kernels (towr_gpu.h, towr_alsolve_state_t; all in lbfgs.hip): the line search (it offers the
// accepted pair with the update kernel's own device code and needs its lbfgs_update_lds(n) bytes), the outer update and
// the state initialisation; one block of kLbfgsBlock threads per problem. XL / XU / ldb as in StepArgs.
enum AlPhase : int32_t {
  kAlRestart = 0, kAlSearch = 1, kAlConverged = 2, kAlStalled = 3, kAlMaxed = 4, kAlAcceptable = 5, kAlInfeasible = 6
};
struct LineSearchArgs {
  towr_alsolve_state_t st;
  const double *XL, *XU; int64_t ldb;
  double c1, shrink, alpha0, alpha_min, curv_eps;
  int32_t n, mem;
};
struct OuterArgs {
  towr_alsolve_state_t st;
  towr_alsolve_params_t pr;
  int32_t m;
};
// the stop rule (towr_gpu_alsolve_stop_batch_device): one thread per problem, blocks of kLbfgsBlock over B
struct StopArgs {
  int32_t* ISTATE;
  double* SCAL; int64_t ldsc;
  double* ALPHA;
  const double* RHO;
  towr_alsolve_stop_t sp;
  int32_t max_inner, B;
};
struct AlInitArgs {
  towr_alsolve_state_t st;
  const double *XL, *XU; int64_t ldb;
  double rho0, eta0, omega0;
  int32_t n;
};
// The probe stage (towr_gpu_alsolve_probe_batch_device): launch t of T + 1, one block of kLbfgsBlock threads per problem.
// Launch t folds the outcome of trial t - 1 (F and RS hold f and the residual summary at the candidate XT of that trial)
// and, while the problem is undecided, writes the candidate of trial t into XT. XT, F and RS are handle scratch; PSUM
// carries the problem's running outcome between the launches ([0] = 0: undecided, [5] = gs of the candidate in XT).
struct ProbeArgs {
  towr_alsolve_state_t st;
  const double *XL, *XU; int64_t ldb;
  double* XT; int64_t ldxt;
  const double* F;
  const double* RS; int64_t ldrs;
  double* PSUM; int64_t ldps;
  double c1, shrink, alpha_min;
  int32_t n, t, T, reserved;
};
const void* alsolve_probe_kernel();
// The verdict stage (towr_gpu_alsolve_verdict_batch_device): the line search's accept test ahead of the direction, one
// block of kLbfgsBlock threads per problem. Of the state only what the test reads; VERDICT takes 0 (a base will be
// accepted) or 2, NDIR (may be NULL) counts the zeros. A products chunk launches with its rows of every pointer.
struct VerdictArgs {
  const double *X, *GR, *XC; int64_t ldx;
  const double* FC;
  const double* SCAL; int64_t ldsc;
  const int32_t* ISTATE;
  const double* RSUM; int64_t ldrs;
  int32_t* VERDICT;
  int32_t* NDIR;
  double c1;
  int32_t n, reserved;
};
const void* alsolve_verdict_kernel();
const void* linesearch_kernel();
const void* alsolve_outer_kernel();
const void* alsolve_stop_kernel();
const void* alsolve_init_kernel();

// The compacting solve's kernels (towr_gpu_alsolve_solve_batch_device; lbfgs.hip). The partition: one block of
// kLbfgsBlock threads over the B phase words. The swap: a grid of (pairs, arrays) blocks of kLbfgsBlock threads; npairs
// is the number of pairs the grid holds, and the count itself when NP is NULL (else min(NP[0], npairs)). The array
// descriptors travel in the argument struct.
struct PartitionArgs {
  const int32_t* ISTATE;
  int32_t* HEAD;
  int32_t* PAIRS;
  int32_t B, reserved;
};
constexpr int kSwapMaxArrays = TOWR_SWAP_MAX_ARRAYS;
struct SwapRows { char* base; int64_t ld_bytes, row_bytes; };
struct SwapRowsArgs {
  const int32_t* NP;
  const int32_t* PAIRS;
  int32_t npairs, n_arrays;
  SwapRows rows[kSwapMaxArrays];
};
const void* alsolve_partition_kernel();
const void* alsolve_swap_rows_kernel();

// The queued solve's kernels (towr_gpu_alsolve_solve_queue_batch_device; lbfgs.hip). The retire key: one thread per row,
// blocks of kLbfgsBlock over B; AGE[b] += add first (add = 0: AGE is only read). The move: a grid of (rows, arrays) blocks
// of kLbfgsBlock threads; block (i, k) copies row r0 + i of slot[k] to row ID[r0 + i] of out[k] (reverse: the other way).
// The descriptors travel in the argument struct, as the swap's.
struct RetireKeyArgs {
  const int32_t* ISTATE;
  int32_t* AGE;
  int32_t* KEY;
  int32_t B, add, max_age, reserved;
};
constexpr int kMoveMaxArrays = TOWR_MOVE_MAX_ARRAYS;
struct MoveRows { char* slot; int64_t slot_ld; char* out; int64_t out_ld; int64_t row_bytes; };
struct MoveRowsArgs {
  const int32_t* ID;
  int32_t r0, count, n_arrays, reverse;
  MoveRows rows[kMoveMaxArrays];
};
const void* alsolve_retire_key_kernel();
const void* alsolve_move_rows_kernel();

struct Layout {
  int n = 0, m = 0;
  int64_t nnz = 0;
  std::vector<VarSetInfo> varsets;
  std::vector<ConsInfo> cons;
  std::vector<SplineMeta> spl;
  std::vector<int32_t> nodecol;
  std::vector<double> dur;
  std::vector<SegRec> segs;     // (2 + 4 n_ee) records per time instant
  bool gait = false;            // phase-duration optimisation (PhaseSplines, schedule variables)
  bool rotvec = false;          // Parameters::RotationVector base orientation (RotVecConverter)
  std::vector<PolyPhase> pinfo; // PhaseSpline polynomial phases
  std::vector<PhaseCol> pcols;  // PhaseSpline full-pattern columns
  std::vector<int32_t> pact;    // PhaseSpline active PhaseCol ranges (SplineMeta::pact_off)
  std::vector<SchedInfo> sched; // per endeffector (col0 = -1 without schedule variables)
  std::vector<EELinDef> eelin;  // EELinearConstraint definitions (ItemDesc::a0 indexes them)
  std::vector<LinNz> lin;       // LinearEqualityConstraint rows (IT_LINEQ: ItemDesc::a0 / a1)
  std::vector<ItemDesc> items;
  std::vector<int32_t> slots;     // build-time: candidate -> global CSR position (or -1)
  std::vector<SlotGroup> slot_groups;   // device slot table (see SlotGroup); item.slot indexes it
  std::vector<ItemDirect> idirect;      // gait: per item (lane), direct-position ranges (ItemDirect)
  std::vector<int64_t> row_ptr;
  std::vector<int32_t> col;
  std::vector<TileDesc> tiles;
  std::vector<double> x0;
  RobotC rb{};
  towr_terrain_t terrain{};
  int32_t fdisc_motion = 0;
  towr_problem_desc_t desc{};
  // tiles are grouped by item type: tiles [type_tile0[t], type_tile0[t+1]) run in one launch of
  // the type's kernel with type_block[t] threads and type_lds[t] doubles of dynamic LDS
  int32_t type_tile0[IT_COUNT + 1] = {};
  int32_t type_block[IT_COUNT] = {};
  int32_t type_lds[IT_COUNT] = {};
  int32_t type_lds_rows_off[IT_COUNT] = {};   // start of the g buffer inside the type's LDS
  int32_t type_lds_dummy_off[IT_COUNT] = {};  // per-lane dummy slots for absent candidates
  int32_t dyn_scr_off = 0;                    // DYN LDS: endeffector sum terms after the g rows
  // fixed gait, RotVec: the Dynamic instants whose base-angular coefficients the pre-pass forms
  // (tiles.hip towr_rv_coef_kernel; a RotVec group-1 item's a0 indexes them)
  std::vector<RvInst> rv_inst;
  // algorithmic bytes per problem of each type's launch: CSR values + g rows written, distinct
  // x columns read (= the columns of its Jacobian rows)
  int64_t type_bytes[IT_COUNT] = {};
  // small kinds (is_misc_kind) run in one launch: kMiscWaves tiles per block, one per wave
  std::vector<int32_t> misc_tiles;   // groups of kMiscWaves tile indices (-1 = empty wave)
  std::vector<int32_t> misc_lds;     // per (group, wave): LDS offset of the wave's tile, its g-row offset (doubles)
  std::vector<int32_t> misc_xspan;   // x spans the small-kind blocks stage: (first 16-B unit, units) pairs; empty = all of x
  int32_t misc_region = 0;           // LDS of the largest group (doubles)
  int64_t misc_bytes = 0;
  // streaming ForceConstraintDiscretized (FsBlock): enabled under phase-duration optimisation on
  // terrains without curvature when every row of each constraint holds the same columns
  bool fstream = false;
  std::vector<FsBlock> fs_blocks;
  std::vector<double> fs_t;
  std::vector<int32_t> fs_tmpl;
  std::vector<int32_t> fs_ws;        // per (constraint, force polynomial): window start, window dimension codes
  std::vector<int32_t> fs_iee, fs_irow, fs_iblk;   // per instant (fs_t order): endeffector, first row, FsBlock
  int32_t fs_tmpl_max = 0;
  // streaming RangeOfMotion / Dynamic (GsGeo): per class enabled when every constraint of the class fits
  bool gstream[GS_COUNT] = {};
  std::vector<GsGeo> gs_geo;
  std::vector<GsBlock> gs_blocks[GS_COUNT];
  std::vector<GsInst> gs_inst[GS_COUNT];   // record lanes' instants (Dynamic: one per instant)
  std::vector<int32_t> gs_tmpl;
  std::vector<uint8_t> gs_pcode;
  std::vector<GsSeg> gs_segs;
  std::vector<uint8_t> gs_tseg;
  std::vector<uint32_t> gs_vmap;
  std::vector<int16_t> gs_ws;
  // per geometry, the composer's static tables in one blob staged to LDS in one pass:
  // [segments | value map | template | position -> segment | prefix codes of every instant | window starts]
  // (GsSeg::toff of a template segment indexes the blob's template, GsSeg::wsoff its window starts)
  std::vector<uint4> gs_blob;
  std::vector<WatchItem> watch;     // pattern watch (curved terrain only)
  int32_t gs_geo_max[GS_COUNT][4] = {};  // largest geometry of the class: Li, segments, values per instant, blob bytes
  int32_t gs_tmpl_max[GS_COUNT] = {};      // template ints of the largest geometry (compose LDS)
  int32_t gs_pcode_max[GS_COUNT] = {};     // prefix codes per instant, largest geometry
  int32_t gs_nmax[GS_COUNT] = {};          // instants of the largest compose block
  // cost terms (eval_f / eval_grad_f): work items sorted by CostType, one block per problem
  std::vector<CostItem> cost_items;
  std::vector<double> cost_q;        // CT_ENERGYQ Gram matrices, 16 doubles per item (CostItem::q)
  // Deterministic gradient (fixed phase durations): every present gradient entry of every cost item has an
  // LDS contribution slot, ordered by column (layout.hip build_cost_slots): entry k of item i goes to slot
  // cost_cslot[CostItem::cslot + k], and column j sums slots [cost_cptr[j], cost_cptr[j + 1]) in order.
  // cost_nslot = 0: fixed-point limbs instead (phase-duration optimisation, where the PhaseSpline windows
  // move with x, or more slots than kCostSlotMax).
  int32_t cost_nslot = 0;
  std::vector<uint16_t> cost_cptr;
  std::vector<uint16_t> cost_cslot;
  // SoftConstraint terms (TOWR_COST_SOFT), in cost order: the cost index and the wrapped constraint.
  // The wrapped sets are evaluated by a second layout (the handle's soft child) whose constraint
  // list is exactly these sets in this order (soft_desc).
  std::vector<std::pair<int32_t, int32_t>> soft;
  // The pattern by column (towr_gpu_jac_csc): column j holds entries [col_ptr[j], col_ptr[j + 1]), rows ascending;
  // csc_index = the entry's CSR position. And the product kernels' tables (JpSeg / JpChunk above): the row of every
  // CSR entry, the chunk-local by-column lists (padded to whole chunks), the segments, the rows without entries.
  std::vector<int64_t> col_ptr;
  std::vector<int32_t> csc_row, csc_index;
  std::vector<int32_t> jp_row;
  std::vector<uint16_t> jp_cidx;
  std::vector<JpSeg> jp_rseg, jp_cseg;
  std::vector<JpChunk> jp_chunks;
  std::vector<int32_t> jp_empty_rows;
  int32_t jp_long = kJpLongDefault;   // segments of at least this many entries are summed by a wave
  // The constraint bounds in ifopt row order (build_bounds: every set's GetBounds restated), at the description's
  // x0 and terrain; tq_bounds lists the rows that torque_bounds re-evaluates for another x / terrain. bounds_err is
  // non-empty when a set's bounds need side data (TOWR_DATA_BOUNDS) that was not given: the bounds calls then fail.
  std::vector<double> g_lower, g_upper;
  std::vector<TqBound> tq_bounds;
  std::string bounds_err;
  // The variable bounds in ifopt column order (build_var_bounds: the driver's AddBound calls, side data
  // TOWR_DATA_VAR_BOUNDS, replayed on the node sets; the schedule sets' duration box)
  std::vector<double> x_lower, x_upper;
};
// the variable bounds of the layout for the TOWR_DATA_VAR_BOUNDS entries of `data` (lower / upper: n doubles each)
int build_var_bounds(const Layout& L, int n_data, const towr_data_t* data, double* lower, double* upper, std::string& err);
void build_jprod(Layout& L);   // fills the jp_ / csc members above from row_ptr / col
// the (-L, L) rows of the node TorqueConstraints at x on terrain `ter`, written into lower / upper (m doubles each)
void torque_bounds(const Layout& L, const double* x, const towr_terrain_t& ter, double* lower, double* upper);
// the product kernels (jprod.hip): one block of kJpBlock threads per problem; Vec = P (ldvec >= n) and Out = Y for
// J p, Vec = LAM (>= m) and Out = Z for J^T lam; the tables are the device copies of the members above (uploaded and
// launched by auglag.hip)
struct JpArgs {
  const double* V; int64_t ldv;
  const double* Vec; int64_t ldvec;
  double* Out; int64_t ldo;
  const int32_t *col, *row;
  const uint16_t* cidx;
  const JpSeg *rseg, *cseg;
  const JpChunk* chunks;
  const int32_t *empty_rows, *col_ptr;   // col_ptr as int32 (nnz < 2^31)
  int64_t nnz;
  int32_t n, m, n_chunks, n_empty, accumulate, reserved;
};
size_t jp_vec_lds(int n, int m);    // dynamic LDS (bytes)
size_t jp_tvec_lds(int n, int m);
const void* jp_vec_kernel();
const void* jp_tvec_kernel();

// The Gauss-Newton direction (jprod.hip, towr_gpu_gn_direction_batch_device): one block of kGnBlock threads per problem
// runs the whole CG solve on (rho J^T W J)_ff + mu I, every step one J p and one J^T t pass over the problem's values
// with the product kernels' tables (jp: products_ready's; its operand members are not used). p, r, the column
// accumulator (n each), t (m), the chunk tile, the by-column list and the active-row bytes live in dynamic LDS
// (gn_direction_lds); d lives in the D row. XL / XU / ldb as in StepArgs (X NULL: every column free, bounds not read).
struct GnArgs {
  const double* V; int64_t ldv;
  const double* LAMP; int64_t ldlp;
  const double* RHO; double rho;       // RHO[b], or the scalar when RHO is NULL
  const double* X; int64_t ldx;
  const double* GR; int64_t ldgr;
  const double *XL, *XU; int64_t ldb;
  const int32_t* RUN; int64_t run_stride;   // a block whose RUN[b*run_stride] >= 2 returns at once; NULL: every block runs
  double* D; int64_t ldd;
  double* SUM; int64_t lds;
  double mu, tol;
  int32_t ncg, reserved;
  JpArgs jp;
  double* PC; int64_t ldpc;   // the preconditioned kernel's M rows (gn_direction_pc_kernel; the plain one reads neither)
};
constexpr int kGnBlock = 512;            // twice the product kernels' block: its LDS admits two blocks per CU
constexpr int kGnMaxN = 32 * kGnBlock;   // the held mask is one 32-bit word per lane
size_t gn_direction_lds(int n, int m);   // dynamic LDS (bytes)
const void* gn_direction_kernel();
const void* gn_direction_pc_kernel();   // the Jacobi-preconditioned recursion: the same block, walk and LDS

// The direct Gauss-Newton direction (jprod.hip, towr_gpu_gn_direction_direct_batch_device): one block of kGnBlock
// threads per problem assembles H = rho (J^T W J)_ff + mu I (identity on held columns) into the envelope of its lower
// triangle under the handle's ordering, factorises it L L^T in place and solves. The envelope lives in the problem's
// workspace row (W + blockIdx.x * ldw; the host offsets the other operands per launch): permuted row q holds the
// entries of permuted columns first[q] .. q at row_off[q] .. row_off[q + 1] - 1, the diagonal last. inv[q] is the
// column at permuted position q, last[c] the largest permuted row whose envelope reaches permuted column c; the
// pattern by column (col_ptr of jp, csc_row, csc_index) feeds the assembly. width = max_q (q - first[q]).
struct GnDirectArgs {
  const double* V; int64_t ldv;
  const double* LAMP; int64_t ldlp;
  const double* RHO; double rho;
  const double* X; int64_t ldx;
  const double* GR; int64_t ldgr;
  const double *XL, *XU; int64_t ldb;
  const int32_t* RUN; int64_t run_stride;
  double* D; int64_t ldd;
  double* SUM; int64_t lds;
  double* W; int64_t ldw;
  double mu;
  const int32_t *pos, *inv, *first, *last, *row_off;   // n, n, n, n, n + 1
  const int32_t *col_ptr, *csc_row, *csc_index;        // n + 1, nnz, nnz
  int32_t n, m, env, width;
};
size_t gn_direct_lds(int n, int m, int width);   // dynamic LDS (bytes)
const void* gn_direct_kernel();

// The tiled direct Gauss-Newton direction (jprod.hip, towr_gpu_gn_direction_tiled_batch_device): the same system, held
// rule, ordering and summary as the direct direction, factorised as a block Cholesky on kGnTile x kGnTile tiles inside
// the tile envelope of towr_gpu_gn_tile_info. The workspace row holds the stored tiles block row by block row: tile
// (I, K), bfirst[I] <= K <= I, at 256 (tile_off[I] + K - bfirst[I]), entry (r, c) of a tile at 16 c + r (column-major).
// tcol_ptr / tcol_rows list per block column J the block rows I > J whose envelope reaches J, ascending. The assembly is
// symbolic too: stored entry e (of permuted columns q >= c) sums the terms asm_ptr[e] .. asm_ptr[e + 1] - 1, one per row
// of J that holds both columns, rows ascending (what the direct kernel's merge finds, found once per handle).
struct GnAsmTerm { int32_t a, b, row; };   // the CSR entries of column inv[q] and of column inv[c] in that row
struct GnTiledArgs {
  const double* V; int64_t ldv;
  const double* LAMP; int64_t ldlp;
  const double* RHO; double rho;
  const double* X; int64_t ldx;
  const double* GR; int64_t ldgr;
  const double *XL, *XU; int64_t ldb;
  const int32_t* RUN; int64_t run_stride;
  double* D; int64_t ldd;
  double* SUM; int64_t lds;
  double* W; int64_t ldw;
  double mu;
  const int32_t *pos, *inv;                                  // n each
  const int32_t *bfirst, *tile_off, *tcol_ptr, *tcol_rows;   // nt, nt + 1, nt + 1, tiles - nt
  const int32_t* asm_ptr; const GnAsmTerm* asm_terms;        // 256 tiles + 1, asm_ptr[256 tiles]
  int32_t n, m, nt, tiles;
};
constexpr int kGnTile = 16;
size_t gn_tiled_lds(int n, int m);   // dynamic LDS (bytes)
const void* gn_tiled_kernel();

// The resident GN loop's select (lbfgs.hip): per problem by the flags the line search wrote, D <- DC (bit 0), else
// D <- GR (bit 2), else nothing; one block of kLbfgsBlock threads per problem.
struct GnSelectArgs {
  const int32_t* ISTATE;
  const double* DC; int64_t lddc;
  const double* GR; int64_t ldgr;
  double* D; int64_t ldd;
  int32_t n, reserved;
};
const void* gn_select_kernel();

#ifndef TOWR_COST_SLOT_MAX   // (experiment builds: -DTOWR_COST_SLOT_MAX=0, the limbs everywhere)
#define TOWR_COST_SLOT_MAX 8192
#endif
constexpr int kCostSlotMax = TOWR_COST_SLOT_MAX;   // contribution slots of the cost kernel's LDS (64 KB)
constexpr int kCostLanes = 256;   // threads of the cost kernel's blocks (kCostBlock, its wave schedule)
constexpr int kMiscWaves = 4;   // one-wave small-kind tiles per group (block)
constexpr int kSlotSpare = 4;   // spare slot groups per lane: the kernels prefetch up to this many ahead
constexpr bool is_misc_kind(int t) { return t != IT_DYN && t != IT_ROM && t != IT_FDISC && t != IT_TQDISC; }

// launch classes: the heavy kinds have their own kernels, the small kinds share one
enum LaunchClass { LC_DYN = 0, LC_ROM = 1, LC_FDISC = 2, LC_TQDISC = 3, LC_MISC = 4, LC_COUNT = 5 };
constexpr int class_type(int lc) { return lc == LC_TQDISC ? IT_TQDISC : lc; }   // tile classes

// LDS tile caps (doubles of CSR values / rows per tile)
constexpr int kTileValueCap = 8192;
constexpr int kTileRowCap = 2048;
constexpr int kMiscValueCap = 3072;   // small-kind tiles: 4 share one block's LDS
constexpr int kMiscRowCap = 512;

// Tile value cap under phase-duration optimisation: the tile classes have no LDS tile there (they
// store straight into a zero-filled V, TileEmit DIRECT), so a tile is bounded only by its lanes and
// the uint16 slot positions (values + 64 dummy slots < kSlotAbsent)
constexpr int kTileValueCapGait = 65536 - 2 - 64 - 2;

// Row-split items (phase-duration optimisation only). A PhaseSpline item emits its full-pattern
// windows and schedule columns one candidate at a time, a chain of dependent slot-table and
// PhaseCol loads; one item per instant would leave a tile of ~20 instants on 20 lanes of a 192-lane
// block. Such items are split over lanes by rows (ItemDesc::rsel, split_part_rows): every lane
// evaluates the instant, only its rows' candidates are emitted. Returns the lanes per item (1 = not split).
int split_rows(int type, int group, bool gait);

// Block size of the tile classes. Under phase-duration optimisation every wave holds one row of
// the split items (lanes = instants), so that a wave's lanes take the same branches: a wave mixing
// the rows of an item would execute every row's emission path one after the other.
//   DYN: g0 | g1 | row 0 .. 5 of the endeffector groups (lanes = ee x instant);
//   ROM: two halves of 64 instants, each g0 | g1 | row 0 | 1 | 2 of the motion group;
//   FDISC: two halves of 64 instants, each row 0 | 1 | 2 | 3 | 4;  TQDISC: rows 0 .. 3.
// A 5-wave block is placed as if it took 2 waves on every SIMD (hipOccupancy... and the measured
// residency: 1 block per CU at 168 VGPRs), and a 4-wave block with FDISC rows (0, 1) on one wave
// waits for that wave (1.5x the others): 10-wave blocks are balanced and fill 10 of the 12 wave slots.
constexpr int kDynGaitRowParts = 6;
constexpr int tile_block(int type, bool gait) {
  return type == IT_DYN ? (gait ? 64 * (2 + kDynGaitRowParts) : 256) : type == IT_ROM ? (gait ? 640 : 192) : type == IT_FDISC ? (gait ? 640 : 192)
       : type == IT_TQDISC ? (gait ? 256 : 192) : 64;
}

// Launch geometry of each item type (wave-uniform: each wave of a block runs one code path)
struct TypeSpec { int block; int max_inst; };
TypeSpec type_spec(int type, int n_ee, bool gait, bool rotvec = false);
// thread (lane) of the block that evaluates row-part `sub` (0 .. split_rows - 1) of group `g` of
// the k-th of n instances in a tile
int type_lane(int type, int group, int k, int n, int n_ee, bool gait, int sub);

inline int64_t fs_record_doubles() { return kFsRS; }   // FDISC record doubles per instant

// The streaming kernels (gstream.hip): compose LDS (bytes), record doubles per problem of one class,
// entry points. The record kernel uses fs_inst_lds_bytes' LDS layout, then its Dynamic states and
// scratch (gs_rec_lds).
size_t gs_stream_lds(const Layout& L, int cls);
size_t fs_compose_lds(const Layout& L);   // the ForceConstraintDiscretized compose block (bytes)
int64_t gs_record_doubles(const Layout& L, int cls);
const void* gait_rec_kernel(bool rotvec, int roles);   // instantiation: bit 0 the FDISC part, 1 the RangeOfMotion / Dynamic parts, 2 the TQDISC part
const void* gait_compose_kernel(int mask);   // roles: bit 0 FDISC, 1 RangeOfMotion, 2 Dynamic, 3 small kinds, 4 TQDISC
constexpr int kComposeMasks[] = {1, 2, 4, 6, 7, 15, 16, 17, 23, 31};   // the instantiated role sets
// the composer launch's arguments: the record arrays (per problem, leading dimensions; the
// TorqueConstraintDiscretized records sit in the FDISC record array at tq_off) and, per role (0 FDISC,
// 1 RangeOfMotion, 2 Dynamic, 3 small-kind groups, 4 TorqueConstraintDiscretized), its blocks per problem
// group (0: not in this launch). A problem group's units: [FDISC | TQDISC | RangeOfMotion | Dynamic | small kinds]
struct ComposeArgs {
  const double* frec; int64_t fldr, tq_off;
  const double* grec; int64_t gldr, gdyn_off;
  const GsBlock* blk[GS_COUNT];
  int32_t nt[5];
  int32_t ng;          // problem groups: a block composes problems g, g + ng, ... (kGsGroup per block)
  int32_t misc_x_off;  // small kinds: the staged x's LDS offset (doubles)
};
// the record launch's arguments (towr_gait_rec_kernel): nparts blocks per problem, block r doing part
// (parts >> 4 r) & 15 (RecPart); the FDISC records (frec, fldr, ni instants) and the
// TorqueConstraintDiscretized records (frec + tq_off, g.inst[GS_TQ]) share one array per problem
enum RecPart { kRecFdisc = 1, kRecTq = 2, kRecGs = 3, kRecGsDyn = 4, kRecGsRom = 5 };
struct RecArgs {
  GsRecArgs g;
  double* frec; int64_t fldr, tq_off;
  int32_t ni, nparts, parts;
  // the FDISC launch (gstream.hip towr_gait_frec_kernel): byte offset in LDS of the staged FsBlock / window /
  // template tables (0: the lanes read them in global memory), and their sizes in int32 words
  int32_t fs_lds, fs_nb, fs_nws, fs_ntm;
};
size_t gs_dyn_state_bytes(bool rotvec);   // the record kernel's per-Dynamic-instant LDS state
constexpr int kGsRecMaxBlock = 512;
constexpr int kFsRecBlock = 512;   // the record launch's threads when it holds FDISC records
// The frozen-pattern check (WatchItem): reference Jacobian entries at x outside the x0 pattern, evaluated
// with the structure pass's arithmetic on the host
int64_t pattern_outside_host(const Layout& L, const double* x, const towr_terrain_t& terrain);

// Returns TOWR_OK or an error code with a message in `err`. Side data (towr_gpu_create_ex): the
// LinearEqualityConstraint matrices; the SoftConstraint bounds are checked by the handle.
int build_layout(const towr_problem_desc_t& d, Layout& L, std::string& err);
int build_layout_ex(const towr_problem_desc_t& d, int n_data, const towr_data_t* data, Layout& L, std::string& err);
// the description of the soft child: the SoftConstraint terms' wrapped sets as hard constraints, no costs
towr_problem_desc_t soft_desc(const towr_problem_desc_t& d, const Layout& L);
const towr_data_t* find_data(int n_data, const towr_data_t* data, int kind, int index);

// x0 for another init/terrain on the layout built from `d` (nlp_formulation.cc:121-346).
int initial_x_for(const towr_problem_desc_t& d, const towr_init_t& init, const towr_terrain_t& ter,
                  std::vector<double>& x0, std::string& err);


}  // namespace tg
