// handle.h — the handle behind include/towr_gpu.h and the host helpers its translation units share (internal, not
// installed): towr_gpu.hip (the evaluator: handle creation, device tables, launch sequencing, host-pointer entry
// points) defines the helpers; auglag.hip (the batched solver-step entry points) uses the evaluator through them.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/towr_gpu.h"
#include "engine_math.h"
#include "kernel_common.h"
#include "layout.h"

struct towr_gpu_handle_s {
  tg::Layout L;
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  // device tables
  tg::ItemDesc* d_items = nullptr;
  tg::SlotGroup* d_slots = nullptr;
  tg::TileDesc* d_tiles = nullptr;
  int32_t* d_nodecol = nullptr;
  tg::SplineMeta* d_spl = nullptr;
  double* d_dur = nullptr;
  void* d_segs = nullptr;      // SegSoA storage
  tg::SegSoA sg{};
  tg::PolyPhase* d_pinfo = nullptr;
  tg::PhaseCol* d_pcols = nullptr;
  int32_t* d_pact = nullptr;
  tg::SchedInfo* d_sched = nullptr;
  int32_t* d_misc = nullptr;
  int32_t* d_misc_lds = nullptr;
  tg::MiscWave* d_misc_wave = nullptr;
  tg::ItemDesc* d_misc_items = nullptr;
  int32_t* d_xspan = nullptr;
  tg::EELinDef* d_eelin = nullptr;
  tg::LinNz* d_lin = nullptr;
  uint4* d_gtab = nullptr;     // GAIT: PhaseSpline tables blob (GaitTables)
  tg::ItemDirect* d_idir = nullptr;
  tg::CostItem* d_citems = nullptr;
  double* d_cq = nullptr;
  tg::FsBlock* d_fsb = nullptr;    // streaming ForceConstraintDiscretized tables (layout.h FsBlock)
  double* d_fs_t = nullptr;
  int32_t* d_fs_tmpl = nullptr;
  int32_t* d_fs_ws = nullptr;
  int32_t* d_fs_iee = nullptr;
  int32_t* d_fs_irow = nullptr;
  int32_t* d_fs_iblk = nullptr;
  double* d_fsrec = nullptr;   // per-problem instant records of the streaming path (scratch, grown on demand)
  int64_t fsrec_cap = 0;       // problems it holds
  tg::GsGeo* d_gs_geo = nullptr;   // streaming RangeOfMotion / Dynamic tables (layout.h GsGeo)
  int32_t* d_gs_tmpl = nullptr;
  uint8_t* d_gs_pcode = nullptr;
  tg::GsSeg* d_gs_segs = nullptr;
  uint8_t* d_gs_tseg = nullptr;
  uint32_t* d_gs_vmap = nullptr;
  int16_t* d_gs_ws = nullptr;
  uint4* d_gs_blob = nullptr;
  tg::GsBlock* d_gs_blk[tg::GS_COUNT] = {};
  tg::GsInst* d_gs_inst[tg::GS_COUNT] = {};
  double* d_rvc = nullptr;     // fixed gait, RotVec: the Dynamic base-angular coefficients of the pre-pass (scratch)
  int64_t rvc_cap = 0;
  tg::RvInst* d_rvi = nullptr;
  double* d_gsrec = nullptr;   // their records, both classes (scratch, grown on demand)
  int64_t gsrec_cap = 0;
  // The scratch above (and the soft child's g / values, d_sg / d_sv, and the solver-step entries' scratch in `al`) is
  // shared by every call on the handle: a call on another stream than the previous one waits for the previous call's
  // work (this event), and growing a buffer waits for it on the host before the old one is freed.
  hipEvent_t scr_ev = nullptr;
  hipStream_t scr_stream = nullptr;
  bool scr_used = false;
  bool sync_call = false;   // host_eval: the call synchronises its stream before returning (no event needed)
  // towr_gpu_eval_g_keep_jac: the Jacobian of kept_x waits in the device staging d_v (kept: until any other
  // host-pointer evaluation reuses the staging)
  bool kept = false;
  std::vector<double> kept_x;
  // fusion groups (TOWR_GPU_FUSE, see towr_step_kernel): classes that run in one launch
  struct FuseGroup {
    uint32_t mask = 0;        // bit lc: launch class lc belongs to the group
    int kblock = 0;
    tg::UnitDesc* d_units = nullptr;
    int32_t n_units = 0;
    size_t lds = 0;
  };
  static constexpr int kMaxFuse = 2;
  FuseGroup fuse[kMaxFuse];
  int n_fuse = 0;
  // one problem through host pointers (eval_g / eval_jac_values / eval_g_jac): every class in ONE
  // launch (the fused kernel over all units), so the per-call latency is one kernel, not three
  FuseGroup single;
  // host entry points: caller memory page-locked by towr_gpu_register_host (DMA straight to / from
  // it), the copy stream of the chunked host batch and its per-chunk events
  struct Pinned { const char* p; size_t n; char* dev; };   // host range and its device address
  std::vector<Pinned> pinned;
  double *hd_x = nullptr, *hd_g = nullptr, *hd_v = nullptr;   // device addresses of the pinned staging
  hipStream_t copy_stream = nullptr;
  std::vector<hipEvent_t> ev_c, ev_d;
  std::string fuse_name[kMaxFuse];   // towr_gpu_kernel_info
  // fork-join of the per-kind launches (TOWR_GPU_STREAMS = total streams incl. the caller's, 1..4)
  static constexpr int kMaxSide = 3;
  int n_side = 0;
  hipStream_t side[kMaxSide] = {};
  hipEvent_t fork = nullptr, join[kMaxSide] = {};
  bool rv_overlap = false;   // RotVec without fusion groups: Dynamic and the small kinds on side stream 0 (launch_classes)
  towr_terrain_t* d_terrain = nullptr;      // base terrain (1 entry)
  towr_terrain_t* d_bterrain = nullptr;     // per-problem batch terrains
  int32_t bterrain_n = 0;
  std::vector<towr_terrain_t> bterrain_h;   // their host copy (the frozen-pattern check)
  // staging for host-pointer entry points
  double *d_x = nullptr, *d_g = nullptr, *d_v = nullptr;
  double *h_x = nullptr, *h_g = nullptr, *h_v = nullptr;
  int32_t stage_B = 0;
  double *d_f = nullptr, *d_grad = nullptr;   // host-pointer objective entry points (one problem)
  // trajectory export: fixed phase table and the sample times of the last dt
  double* d_traj_pd = nullptr;
  int32_t* d_traj_n = nullptr;
  int32_t* d_traj_c0 = nullptr;
  double* d_traj_t = nullptr;
  double traj_dt = 0.0;
  int32_t traj_ns = 0;
  // SoftConstraint terms: a second handle over the wrapped sets (soft_desc), its CSR pattern, the
  // bounds' mid-points b (rows in its order) and its per-batch g / values scratch
  towr_gpu_handle_s* soft = nullptr;
  std::vector<double> soft_b;
  double* d_soft_b = nullptr;
  int32_t* d_soft_cptr = nullptr;   // the soft pattern by column (KParams::s_cptr / s_cent)
  int2* d_soft_cent = nullptr;
  uint16_t* d_c_cptr = nullptr;     // the cost gradient's slot lists (Layout::cost_cptr / cost_cslot)
  uint16_t* d_c_cslot = nullptr;
  int cost_grid[3] = {1, 1, 1};     // the cost kernel's persistent grid per accumulation (launch_cost)
  int32_t cost_grid_override = 0;   // towr_gpu_set_cost_grid: blocks for every accumulation (0 = the automatic grid)
  double *d_sg = nullptr, *d_sv = nullptr;
  int64_t soft_cap_g = 0, soft_cap_v = 0;   // problems the scratch holds
  // What the solver-step entry points (auglag.hip) keep on the handle: device tables uploaded by the first call that
  // needs them, and scratch grown on demand.
  struct AugLag {
    // Jacobian products (jprod.hip): the tables' device copies (products_ready) and the fused entries' own values
    // scratch (a chunk of problems; never d_v, so the kept Jacobian survives); products_chunk:
    // towr_gpu_set_products_chunk (0 = automatic)
    bool jp_ready = false;
    tg::JpArgs jp{};
    void* d_jp[8] = {};
    double* d_pv = nullptr;
    int64_t pv_cap = 0;
    int32_t products_chunk = 0;
    bool gn_ready = false;   // the GN direction kernel's LDS fits and its limit is raised (gn_ready; after products_ready)
    // The direct GN direction (towr_gpu_gn_factor_info): the ordering and the envelope of the lower triangle of the
    // pattern of J^T J under it, built on the host by the first call that asks (a layout-only handle answers too), and
    // their device copies with the pattern by column (gn_direct_ready; after products_ready)
    bool gf_built = false;
    std::vector<int32_t> gf_pos, gf_inv, gf_first, gf_last, gf_row_off;
    int64_t gf_env = 0;
    int32_t gf_width = 0;
    bool gnd_ready = false;
    void* d_gf[7] = {};
    // The tiled direct direction (towr_gpu_gn_tile_info): the 16 x 16 tile envelope of that ordering, built on the host
    // by the first call that asks, and the device copies (gn_tiled_ready; after products_ready): bfirst, tile_off,
    // tcol_ptr, tcol_rows (layout.h GnTiledArgs), pos, inv, and the assembly's terms (gt_terms of them; built for the
    // upload only)
    bool gt_built = false;
    std::vector<int32_t> gt_bfirst, gt_tile_off, gt_col_ptr, gt_col_rows;
    int64_t gt_tiles = 0, gt_terms = 0;
    bool gnt_ready = false;
    void* d_gt[8] = {};
    // Residuals (resid.hip): the device copies of the constraint sets' row ranges and of the description bounds
    // (residual_ready), and the fused entries' g / lam+ scratch (a chunk of problems)
    bool res_ready = false;
    int32_t* d_set_row0 = nullptr;
    double *d_blo = nullptr, *d_bup = nullptr;
    double *d_rg = nullptr, *d_rl = nullptr;
    int64_t rg_cap = 0, rl_cap = 0;
    // Steps (step.hip): the device copies of the variable sets' column ranges and of the description's variable
    // bounds (step_ready), and the fused entries' gradient or direction / f scratch (the batch)
    bool step_ready = false;
    int32_t* d_set_col0 = nullptr;
    double *d_xlo = nullptr, *d_xup = nullptr;
    double *d_sd = nullptr, *d_sf = nullptr;
    int64_t sd_cap = 0, sf_cap = 0;
    // The probe stage (towr_gpu_alsolve_probe_batch_device): the residual summaries of its candidates (the batch); the
    // candidates themselves, their f, g and lam+ use d_sd, d_sf, d_rg and d_rl
    double* d_pr = nullptr;
    int64_t pr_cap = 0;
    // The solve driver (towr_gpu_alsolve_solve_batch_device): page-locked host memory for the partition's HEAD (8 ints),
    // made by the first solve
    int32_t* h_head = nullptr;
    void release();   // frees every device allocation above (towr_gpu_destroy, device handles only)
  } al;
};

namespace tg {
namespace host {

constexpr size_t kLdsMax = 160 * 1024;   // LDS of a gfx950 workgroup

// records msg as the handle's (and the process's) last error and returns code
int fail(towr_gpu_handle h, int code, const std::string& msg);

#define HIPCHK(h, expr)                                                                         \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess) return ::tg::host::fail((h), TOWR_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
  } while (0)

// Every kernel launch of the engine goes through here (TOWR_GPU_LAUNCH_LOG, the TOWR_STAMPS experiment build).
hipError_t launch_kernel(const void* fn, dim3 grid, dim3 block, void** args, size_t lds, hipStream_t s);

// a device copy of src (synchronous; one element is allocated for an empty src)
template <class T>
int upload(towr_gpu_handle h, T** dst, const std::vector<T>& src) {
  const size_t bytes = sizeof(T) * (src.empty() ? 1 : src.size());
  HIPCHK(h, hipMalloc(reinterpret_cast<void**>(dst), bytes));
  if (!src.empty()) HIPCHK(h, hipMemcpy(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
  return TOWR_OK;
}

// every evaluation entry point: refuse layout-only handles, make the handle's device current
int bind(towr_gpu_handle h);

// Handle scratch ordering (see towr_gpu_handle_s::scr_ev): acquire before a call's first use on stream s,
// release after its last; grow() reallocates a per-problem buffer once every earlier use has finished.
int scratch_acquire(towr_gpu_handle h, hipStream_t s);
int scratch_release(towr_gpu_handle h, hipStream_t s);
int scratch_grow(towr_gpu_handle h, double** buf, int64_t* cap, int64_t problems, int64_t doubles_per_problem);

// Terrain of a batch launch: the per-problem set (towr_gpu_set_batch_terrain) when one is set, which
// must then hold exactly B entries; else the description's terrain for every problem. `single`
// entry points (one problem through host pointers) always use the description's terrain.
int batch_terrain(towr_gpu_handle h, int B, bool single, const towr_terrain_t** ter, int* per);

// the evaluator's launch sequence for B problems (g and / or the Jacobian values; only_class -1: every class) and
// the objective's (F and, with GR, its gradient), on stream s
int launch(towr_gpu_handle h, int B, const double* X, int64_t ldx, double* G, int64_t ldg, double* V, int64_t ldv,
           int want_g, int want_jac, hipStream_t s, const towr_terrain_t* terrains, int per_problem, int only_class);
int launch_cost(towr_gpu_handle h, int B, const double* X, int64_t ldx, double* F, double* GR, int64_t ldgr,
                hipStream_t s, const towr_terrain_t* terrains, int per_problem);

}  // namespace host
}  // namespace tg
