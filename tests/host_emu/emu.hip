// TEST INFRASTRUCTURE ONLY — host emulation of towr_eval_kernel's per-item loop, used by the
// CPU test suite to check engine_math.h values against the oracle before GPU runs. It is built
// into tests/host_emu/build/libemu.so and is never linked into or loaded by the product.
#include "../../towr2025_amd/csrc/consumer_common.h"
#include "../../towr2025_amd/csrc/gs_cls.h"
#include "../../towr2025_amd/csrc/layout.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

using namespace tg;

namespace {
// same semantics as the kernel's TileEmit: 8 tile-relative positions per SlotGroup, one plain store
// per present candidate (a position written twice would be a layout bug: the check leaves NaN)
struct AccEmit {
  const SlotGroup* slot; int stride; double* v; double* gout; int nvals; int flo = 0, fcnt = 0; ItemDirect dd{}; int j = 0;
  static constexpr bool kFilter = true;   // row-split items (ItemDesc::rsel), as the kernel's TileEmit
  bool want(int row) const { return fcnt == 0 || (unsigned)(row - flo) < (unsigned)fcnt; }
  void g(int row, double val) { gout[row] = val; }
  void operator()(int row, int col, double val, bool) {
    if (!want(row)) return;
    int s = slot_pick(slot[(j / 8) * stride], j % 8);
    // the kernel's direct ranges (TileEmit DIRECT): must give the slot table's position
    if (col >= dd.c0[0] && col < dd.c1[0]) s = dd.off[0] + col;
    else if (col >= dd.c0[1] && col < dd.c1[1]) s = dd.off[1] + col;
    ++j;
    if (s >= nvals) return;   // the lane's dummy slot (absent candidate)
    v[s] = std::isnan(v[s]) ? val : std::nan("");
  }
  void flush() {}
};
}

extern "C" int emu_eval_ex(const towr_problem_desc_t* d, int n_data, const towr_data_t* data, const double* x, double* g,
                           double* v, char* err, int errlen) {
  Layout L; std::string e;
  int rc = build_layout_ex(*d, n_data, data, L, e);
  if (rc) { if (err) std::snprintf(err, errlen, "%s", e.c_str()); return rc; }
  std::memset(g, 0, sizeof(double) * L.m);
  for (int64_t k = 0; k < L.nnz; ++k) v[k] = std::nan("");   // every slot must be stored
  Ctx c{};
  c.x = x; c.nodecol = L.nodecol.data(); c.spl = L.spl.data(); c.dur = L.dur.data();
  c.ter = &L.terrain; c.rb = L.rb; c.fdisc_motion = L.fdisc_motion;
  c.gait = L.gait; c.pinfo = L.pinfo.data(); c.pcols = L.pcols.data(); c.sched = L.sched.data();
  c.eelin = L.eelin.data(); c.lin = L.lin.data(); c.rotvec = L.rotvec;
  // the small kinds see x as the kernel stages it (Layout::misc_xspan): every column outside the spans is NaN,
  // so an item reading an unstaged column fails the comparison with the oracle
  std::vector<double> xm;
  if (!L.misc_xspan.empty()) {
    xm.assign((size_t)L.n, std::nan(""));
    for (size_t k = 0; k + 1 < L.misc_xspan.size(); k += 2)
      for (int32_t u = L.misc_xspan[k]; u < L.misc_xspan[k] + L.misc_xspan[k + 1]; ++u)
        for (int j = 2 * u; j < 2 * u + 2 && j < L.n; ++j) xm[(size_t)j] = x[j];
  }
  for (const TileDesc& td : L.tiles)
    for (int l = td.i0; l < td.i1; ++l) {
      const ItemDesc& it = L.items[l];
      if (it.type == IT_NONE) continue;
      c.x = is_misc_kind(it.type) && !xm.empty() ? xm.data() : x;
      AccEmit em{L.slot_groups.data() + it.slot, td.i1 - td.i0, v + td.v0, g, td.v1 - td.v0,
                 it.rsel > 0 ? it.row0 + rsel_first(it.rsel) : 0, it.rsel > 0 ? rsel_count(it.rsel) : 0,
                 L.idirect.empty() ? ItemDirect{} : L.idirect[l]};
      c.seg = it.seg >= 0 ? L.segs.data() + (size_t)it.seg * L.spl.size() : nullptr;
      eval_item(c, it, em);
      em.flush();
    }
  c.x = x;
  if (L.fstream) {   // the kernel's streaming ForceConstraintDiscretized composition (fdisc_stream_body)
    c.pact = L.pact.data();
    for (const FsBlock& fb : L.fs_blocks) {
      std::vector<FdiscInstant> in(fb.n_inst);
      std::vector<int> ws(fb.n_inst);
      for (int k = 0; k < fb.n_inst; ++k) {
        c.seg = nullptr;
        fdisc_instant(c, fb.ee, L.fs_t[fb.t0 + k], in[k]);
        ws[k] = L.fs_ws[3 * (fb.wsoff + in[k].poly)];   // (window start, dimension codes, slot codes) triples
        for (int i = 0; i < 5; ++i) g[fb.r0 + 5 * k + i] = in[k].g[i];
      }
      for (int e = 0; e < fb.nv; ++e) {
        const int r = (int)((e + 0.5) * (1.0 / fb.L)), j = e - r * fb.L, k = r / 5, i = r - 5 * k;
        const FdiscInstant& o = in[k];
        double val = 0.0;
        if ((unsigned)(j - fb.js0) < (unsigned)fb.ns1) {
          val = fdisc_sched_value(o.b[i], o.Jf, j - fb.js0);
        } else if ((unsigned)(j - ws[k]) < (unsigned)kFsWin) {
          const int32_t te = L.fs_tmpl[fb.tmpl + j];
          if (te >= 0) {
            const double s = phase_basis_sum(L.pcols[te & 0xFFFFFF], o.poly, o.H[0], o.H[1], o.H[2], o.H[3]);
            val = s == 0.0 ? 0.0 : o.b[i][(te >> 24) & 3] * s;
          }
        }
        v[fb.v0 + e] = val;
      }
    }
  }
  if (L.gstream[GS_TQ]) {   // the streaming TorqueConstraintDiscretized composition (gstream.hip tq_records + gs_compose)
    c.pact = L.pact.data();
    constexpr int RS = kTqND + kTqNI;
    for (const GsBlock& bl : L.gs_blocks[GS_TQ]) {
      const GsGeo& gg = L.gs_geo[bl.geo];
      std::vector<double> rec((size_t)bl.n_inst * RS);
      for (int kk = 0; kk < bl.n_inst; ++kk) {   // the record lanes
        const GsInst& gi = L.gs_inst[GS_TQ][gg.rec0 + bl.k0 + kk];
        c.seg = L.segs.data() + (size_t)gi.seg * L.spl.size();
        double gq[4];
        tq_record(c, gi, [&](int f, double val) { rec[(size_t)kk * RS + f] = val; }, gq);
        for (int i = 0; i < 4; ++i) g[gi.row0 + i] = gq[i];
      }
      for (int e = 0; e < bl.nv; ++e) {   // every entry of the block's range: segment, window, value or 0
        const int kk = e / gg.Li, rr = e - kk * gg.Li;
        const GsSeg& sg = L.gs_segs[gg.seg0 + L.gs_tseg[gg.ts0 + rr]];
        const double* d = rec.data() + (size_t)kk * RS;
        const int32_t* ci = reinterpret_cast<const int32_t*>(d + kTqND);
        const int ws = sg.type == 1 ? L.gs_ws[sg.wsoff + TqCls::poly(ci, sg.kind, sg.ee)] : 0;
        const int q = rr - (sg.p0 + ws);
        v[bl.v0 + e] = q >= 0 && q < sg.W && rr < sg.p0 + sg.len
                           ? TqCls::value(L.rb, L.gs_tmpl.data(), sg, rr, d, ci, nullptr, L.sched[gg.ee].n_phases) : 0.0;
      }
    }
  }
  return 0;
}
extern "C" int emu_eval(const towr_problem_desc_t* d, const double* x, double* g, double* v, char* err, int errlen) {
  return emu_eval_ex(d, 0, nullptr, x, g, v, err, errlen);
}

// What the LDS emitters take for granted about the tile tables, walked as the kernels walk them. AccEmit above drops
// a dummy-slot store and never looks at the LDS layout; here every lane of every tile goes through eval_item with an
// emitter that follows TileEmit / TileEmitPre (tile_emit.h, tiles.hip) load by load and store by store. The
// expectations are restated from the emitters, not from build_layout's arithmetic:
//   * a tile's lanes are the launch's threads: tile_block(type, gait) of them (the kernels' BLOCK template argument
//     and the slot table's stride), 64 for a small kind (TileEmit<64, 3> in misc_body); lane l's groups start at
//     base + l, group g at + g * block; a tile's groups end where the next tile's begin;
//   * an item emits ItemDesc::ncand candidates (of its selected rows, ItemDesc::rsel);
//   * a present candidate's position is inside [0, v1 - v0), holds the candidate's (row, column) in the CSR pattern,
//     and every position of the tile is hit exactly once; a direct range (ItemDirect, TileEmit DIRECT) gives the slot
//     table's position and holds present candidates only;
//   * an absent candidate's position is the lane's dummy slot, type_lds_dummy_off + (lane & 63); the 64 dummy slots lie
//     past the tile's values (DIRECT: `s < nvals` is the only thing that keeps them out of V) and before the g rows;
//   * the g rows (not for fixed-gait Dynamic: kGDirect) and Dynamic's scratch of instants x n_ee x 6 end inside the
//     class's LDS; a small-kind wave's [values | dummies | g rows] ends where the group's next wave begins, and the
//     last one inside misc_region;
//   * the furthest slot group an emitter loads is one of the tile's: TileEmit's ring (depth kTileDepth, the small
//     kinds' kMiscDepth) at construction, idle lanes included, and one group ahead per 8 candidates; DIRECT's
//     preloaded groups (gait_slot_pre: 6 for RangeOfMotion, else 1); TileEmitPre's four groups from
//     kDynG0PhaseA >> 3 on Dynamic's group-0 lanes; threads without a lane (the fused launch's fourth wave, a group's
//     empty waves) read from slot 0 at their launch's stride;
//   * what no candidate owns still holds the all-ones filler.
// out (8): tiles, lanes with an item, present candidates, absent candidates, candidates through a direct range,
// values covered by the tiles, the smallest number of groups left past the furthest load, the largest LDS end
// (doubles) over the classes. Returns 0, -1 (no layout) or the number of the check that failed, with `err`.
namespace {
constexpr int kTileDepth = 2, kMiscDepth = 3;   // tiles.hip slot_depth(), misc_body's TileEmit<64, 3>
constexpr int gait_pre(int type) { return type == IT_ROM ? 6 : 1; }   // tiles.hip gait_slot_pre()
static_assert(tile_block(IT_ROM, false) == 192 && tile_block(IT_FDISC, false) == 192 && tile_block(IT_TQDISC, false) == 192 &&
              tile_block(IT_DYN, false) == 256, "towr_step_kernel's tile_body<.., 192 | 256, KBLOCK, ..> instantiations");
struct BoundsEmit {
  const Layout* L; const TileDesc* td; const SlotGroup* slot; int64_t base, end; int block, lane, depth;
  bool direct; int dummy; std::vector<int>* hit; ItemDirect dd{}; int flo = 0, fcnt = 0;
  int j = 0, far = -1, bad = 0; long present = 0, absent = 0, ranged = 0; char msg[160] = {0};
  static constexpr bool kFilter = true;
  bool want(int row) const { return fcnt == 0 || (unsigned)(row - flo) < (unsigned)fcnt; }
  void fail(int code, const char* what, int a, int b) {
    if (!bad) { bad = code; std::snprintf(msg, sizeof msg, "%s (lane %d candidate %d: %d, %d)", what, lane, j, a, b); }
  }
  const SlotGroup* load(int g) {   // group g of this lane, as the kernels address it
    far = std::max(far, g);
    const int64_t at = (int64_t)(slot - L->slot_groups.data()) + (int64_t)g * block;
    if (at < base || at >= end) { fail(20, "slot group outside the tile's groups", g, (int)((end - base) / block)); return nullptr; }
    return slot + (int64_t)g * block;
  }
  void construct() {   // TileEmit's constructor: the ring, or DIRECT's preloaded groups
    for (int g = 0; g < (direct ? gait_pre(td->type) : depth); ++g) load(g);
  }
  void g(int row, double) { if (row < td->r0 || row >= td->r1) fail(10, "g row outside the tile's rows", row, td->r1); }
  void operator()(int row, int col, double, bool pres) {
    if (!want(row) || bad) return;
    const SlotGroup* q = load(j >> 3);
    if (!q) return;
    const int s = slot_pick(*q, j & 7), nv = td->v1 - td->v0;
    const bool p = pres && col >= 0;
    int sd = 0, k = -1;   // DIRECT: a direct range stores at off + col without the table
    if (direct && col >= dd.c0[0] && col < dd.c1[0]) k = 0;
    else if (direct && col >= dd.c0[1] && col < dd.c1[1]) k = 1;
    if (k >= 0) {
      sd = dd.off[k] + col;
      ++ranged;
      if (!p) fail(11, "an absent candidate in a direct range", col, sd);
      else if (sd != s) fail(12, "a direct range disagrees with the slot table", sd, s);
    }
    if (p) {
      ++present;
      if (s < 0 || s >= nv) fail(13, "a present candidate outside the tile's values", s, nv);
      else if (row < 0 || row >= L->m || td->v0 + s < L->row_ptr[row] || td->v0 + s >= L->row_ptr[row + 1] || L->col[td->v0 + s] != col)
        fail(14, "a present candidate's position is not its (row, column)", row, col);
      else ++(*hit)[s];
    } else {
      ++absent;
      if (s != dummy + (lane & 63)) fail(15, "an absent candidate is not at the lane's dummy slot", s, dummy + (lane & 63));
    }
    ++j;
    if (!direct && (j & 7) == 0) load((j >> 3) + depth - 1);   // the ring's prefetch
  }
  void flush() {}
};
}
extern "C" int emu_tile_bounds_ex(const towr_problem_desc_t* d, int n_data, const towr_data_t* data, int64_t* out, char* err, int errlen) {
  Layout L; std::string e;
  if (build_layout_ex(*d, n_data, data, L, e)) { if (err) std::snprintf(err, errlen, "%s", e.c_str()); return -1; }
  auto fail = [&](int code, const std::string& what) { if (err) std::snprintf(err, errlen, "%s", what.c_str()); return code; };
  const int E = L.rb.n_ee;
  Ctx c{};
  c.x = L.x0.data(); c.nodecol = L.nodecol.data(); c.spl = L.spl.data(); c.dur = L.dur.data();
  c.ter = &L.terrain; c.rb = L.rb; c.fdisc_motion = L.fdisc_motion;
  c.gait = L.gait; c.pinfo = L.pinfo.data(); c.pcols = L.pcols.data(); c.pact = L.pact.data(); c.sched = L.sched.data();
  c.eelin = L.eelin.data(); c.lin = L.lin.data(); c.rotvec = L.rotvec;
  const int64_t total = (int64_t)L.slot_groups.size();
  int64_t lanes = 0, present = 0, absent = 0, ranged = 0, covered = 0, spare = INT32_MAX, lds_end = 0;
  // Dynamic's scratch as the block sees it: [dyn_scr_off, type_lds) of its LDS, exactly that many doubles
  const int scr_n = L.type_lds[IT_DYN] - L.dyn_scr_off;
  if (scr_n < 0 || L.dyn_scr_off < 0) return fail(30, "Dynamic scratch before the start of its LDS");
  std::vector<double> scratch((size_t)scr_n);
  for (size_t ti = 0; ti < L.tiles.size(); ++ti) {
    const TileDesc& td = L.tiles[ti];
    const int t = td.type, block = td.i1 - td.i0, nv = td.v1 - td.v0, nr = td.r1 - td.r0;
    const bool misc = is_misc_kind(t), direct = L.gait && !misc;
    const std::string tag = "tile " + std::to_string(ti) + " type " + std::to_string(t) + ": ";
    if (block != (misc ? 64 : tile_block(t, L.gait)) || block != L.type_block[t]) return fail(1, tag + "lanes are not the kernel's block");
    if (nv < 0 || nr <= 0 || td.v0 != L.row_ptr[td.r0] || td.v1 != L.row_ptr[td.r1]) return fail(2, tag + "values are not the rows' CSR range");
    const int64_t base = L.items[td.i0].slot;
    const int64_t end = ti + 1 < L.tiles.size() ? (int64_t)L.items[L.tiles[ti + 1].i0].slot : total;
    if (base < 0 || end <= base || end > total || (end - base) % block) return fail(3, tag + "slot groups are not whole rounds of the block");
    const int ng = (int)((end - base) / block), dummy = L.type_lds_dummy_off[t];
    // LDS of the tile: [values | 64 dummy slots | g rows] (DIRECT: positions only, no tile)
    if (dummy < nv || dummy + 64 > kSlotAbsent) return fail(4, tag + "dummy slots overlap the values or leave the uint16 range");
    if (!misc && !direct) {
      const bool gdirect = t == IT_DYN;   // fixed-gait Dynamic: g straight to HBM, the scratch follows the dummies
      const int after = gdirect ? L.dyn_scr_off : L.type_lds_rows_off[t];
      if (dummy + 64 > after) return fail(5, tag + "dummy slots overlap what follows them");
      if (!gdirect && L.type_lds_rows_off[t] + nr > L.type_lds[t]) return fail(6, tag + "g rows past the class's LDS");
      lds_end = std::max<int64_t>(lds_end, L.type_lds[t]);
    }
    std::vector<int> hit((size_t)nv, 0);
    int far = -1;
    for (int l = 0; l < block; ++l) {
      const ItemDesc& it = L.items[td.i0 + l];
      if (it.slot != base + l) return fail(7, tag + "lane " + std::to_string(l) + " does not start at base + lane");
      BoundsEmit em{&L, &td, L.slot_groups.data() + it.slot, base, end, block, l, misc ? kMiscDepth : kTileDepth, direct, dummy, &hit};
      if (direct && !L.idirect.empty()) em.dd = L.idirect[td.i0 + l];
      if (it.rsel > 0) { em.flo = it.row0 + rsel_first(it.rsel); em.fcnt = rsel_count(it.rsel); }
      em.construct();
      int cand = 0;
      if (it.type != IT_NONE) {
        if (it.type != t) return fail(8, tag + "a lane of another type");
        ++lanes;
        cand = it.ncand;
        if (t == IT_DYN) {
          if (it.a2 < 0 || (int64_t)(it.a2 + 1) * E * 6 > scr_n) return fail(31, tag + "a Dynamic lane's instant past the scratch");
          if (it.group == 0)   // TileEmitPre: four groups loaded before the barrier between the phases
            for (int g = 0; g < 4; ++g) em.load((kDynG0PhaseA >> 3) + g);
        }
        c.seg = it.seg >= 0 ? L.segs.data() + (size_t)it.seg * L.spl.size() : nullptr;
        c.dyn_scratch = t == IT_DYN ? scratch.data() : nullptr;
        eval_item(c, it, em);
        if (!em.bad && em.j != it.ncand) em.fail(9, "the item's candidates are not ItemDesc::ncand", em.j, it.ncand);
      }
      if (em.bad) return fail(em.bad, tag + em.msg);
      present += em.present; absent += em.absent; ranged += em.ranged;
      far = std::max(far, em.far);
      for (int j = cand; j < 8 * ng; ++j)   // past the lane's candidates: the filler
        if (slot_pick(L.slot_groups[(size_t)(base + (int64_t)(j >> 3) * block + l)], j & 7) != kSlotAbsent)
          return fail(16, tag + "lane " + std::to_string(l) + " position " + std::to_string(j) + " is not the all-ones filler");
    }
    for (int s = 0; s < nv; ++s)
      if (hit[(size_t)s] != 1) return fail(17, tag + "position " + std::to_string(s) + " hit " + std::to_string(hit[(size_t)s]) + " times");
    covered += nv;
    spare = std::min<int64_t>(spare, ng - 1 - far);
  }
  // the small-kind groups: kMiscWaves waves back to back, each [values | dummies | g rows] of its tile's kind
  if (L.misc_tiles.size() % kMiscWaves || L.misc_lds.size() != 2 * L.misc_tiles.size()) return fail(40, "small-kind groups are not whole blocks");
  std::vector<int> seen(L.tiles.size(), 0);
  for (size_t q = 0; q < L.misc_tiles.size(); ++q) {
    const int32_t ti = L.misc_tiles[q];
    if (ti < 0) continue;
    if ((size_t)ti >= L.tiles.size() || !is_misc_kind(L.tiles[(size_t)ti].type) || seen[(size_t)ti]++) return fail(41, "a small-kind wave's tile");
    const TileDesc& td = L.tiles[(size_t)ti];
    const int wl = L.misc_lds[2 * q], rows = L.misc_lds[2 * q + 1], dummy = L.type_lds_dummy_off[td.type];
    int next = L.misc_region;   // where the group's next wave with a tile begins
    for (size_t k = q + 1; k % kMiscWaves; ++k)
      if (L.misc_tiles[k] >= 0) { next = L.misc_lds[2 * k]; break; }
    if (wl < 0 || dummy + 64 > rows || wl + rows + (td.r1 - td.r0) > next || next > L.misc_region)
      return fail(42, "small-kind tile " + std::to_string(ti) + ": its LDS overlaps the next wave's or leaves misc_region");
    lds_end = std::max<int64_t>(lds_end, L.misc_region);
  }
  for (int t = 0; t < IT_COUNT; ++t)
    for (int ti = L.type_tile0[t]; is_misc_kind(t) && ti < L.type_tile0[t + 1]; ++ti)
      if (!seen[(size_t)ti]) return fail(43, "small-kind tile " + std::to_string(ti) + " is in no group");
  // threads without a lane read their ring from slot 0 at the launch's stride
  bool fixed_tile = false;
  for (const TileDesc& td : L.tiles) fixed_tile = fixed_tile || (!L.gait && !is_misc_kind(td.type));
  if (fixed_tile && total <= (int64_t)(kTileDepth - 1) * 192) return fail(44, "the slot table is shorter than an idle thread's ring");
  if (!L.misc_tiles.empty() && total <= (int64_t)(kMiscDepth - 1) * 64) return fail(45, "the slot table is shorter than an empty wave's ring");
  const int64_t o[8] = {(int64_t)L.tiles.size(), lanes, present, absent, ranged, covered, spare, lds_end};
  for (int i = 0; i < 8; ++i) out[i] = o[i];
  return 0;
}
extern "C" int emu_tile_bounds(const towr_problem_desc_t* d, int64_t* out, char* err, int errlen) {
  return emu_tile_bounds_ex(d, 0, nullptr, out, err, errlen);
}

// objective and dense gradient through engine_math.h's cost items (host instantiation)
namespace {
struct GradEmit {
  double* grad; double f = 0.0;
  void operator()(int, int col, double v, bool pres) { if (pres && col >= 0) grad[col] += v; }
};
}
extern "C" int emu_cost(const towr_problem_desc_t* d, const double* x, double* f, double* grad, char* err, int errlen) {
  Layout L; std::string e;
  int rc = build_layout(*d, L, e);
  if (rc) { if (err) std::snprintf(err, errlen, "%s", e.c_str()); return rc; }
  std::memset(grad, 0, sizeof(double) * L.n);
  Ctx c{};
  c.x = x; c.nodecol = L.nodecol.data(); c.spl = L.spl.data(); c.dur = L.dur.data();
  c.ter = &L.terrain; c.rb = L.rb; c.fdisc_motion = L.fdisc_motion;
  c.gait = L.gait; c.pinfo = L.pinfo.data(); c.pcols = L.pcols.data(); c.sched = L.sched.data();
  c.eelin = L.eelin.data(); c.rotvec = L.rotvec; c.cq = L.cost_q.data();
  GradEmit em{grad};
  for (const CostItem& it : L.cost_items) {
    c.seg = it.seg >= 0 ? L.segs.data() + (size_t)it.seg * L.spl.size() : nullptr;
    eval_cost_item(c, it, em);
  }
  *f = em.f;
  return 0;
}

// The objective kernel's deterministic gradient (cost_traj.hip) on the host, with its own emitters:
// acc 1 = the slot path (returns 1 when the layout has no slots), 2 = the fixed-point limb path.
extern "C" int emu_cost_acc(const towr_problem_desc_t* d, const double* x, int acc, double* f, double* grad) {
  Layout L; std::string e;
  if (build_layout(*d, L, e)) return -1;
  if (acc == 1 && L.cost_nslot == 0) return 1;
  Ctx c{};
  c.x = x; c.nodecol = L.nodecol.data(); c.spl = L.spl.data(); c.dur = L.dur.data();
  c.ter = &L.terrain; c.rb = L.rb; c.fdisc_motion = L.fdisc_motion;
  c.gait = L.gait; c.pinfo = L.pinfo.data(); c.pcols = L.pcols.data(); c.pact = L.pact.data(); c.sched = L.sched.data();
  c.eelin = L.eelin.data(); c.rotvec = L.rotvec; c.cq = L.cost_q.data();
  const int n_pad = (L.n + 2) & ~1;
  std::vector<double> cs((size_t)std::max(1, L.cost_nslot), std::nan(""));
  std::vector<unsigned long long> lacc(3 * (size_t)n_pad, 0);
  int bad = 0;
  double fs = 0.0;
  for (const CostItem& it : L.cost_items) {
    c.seg = it.seg >= 0 ? L.segs.data() + (size_t)it.seg * L.spl.size() : nullptr;
    if (acc == 1) {
      CostSlotEmit em{cs.data(), L.cost_cslot.data() + it.cslot, L.n};
      eval_cost_item(c, it, em);
      if (em.slot != L.cost_cslot.data() + it.cslot + it.cn) return 2;   // the host pass's slot count disagrees
      fs += em.f;
    } else {
      CostLimbEmit em{lacc.data(), n_pad, &bad};
      eval_cost_item(c, it, em);
      fs += em.f;
    }
  }
  for (int j = 0; j < L.n; ++j) {
    if (acc == 1) {
      double s = 0.0;
      for (int k = L.cost_cptr[j]; k < L.cost_cptr[j + 1]; ++k) s += cs[k];
      grad[j] = s;
    } else {
      grad[j] = bad ? std::nan("") : limb_value((long long)lacc[j], (long long)lacc[n_pad + j], (long long)lacc[2 * n_pad + j]);
    }
  }
  *f = fs;
  return 0;
}

// The limb arithmetic alone (engine_math.h, single-source with the kernel): CostLimbEmit::operator() on one column
// (n_pad = 1) for v[0], v[1], ... in order, then limb_value of the three sums. limbs[k] = the signed sum of limb k,
// *bad = CostLimbEmit's flag (the kernel then returns NaN), *value = limb_value whatever the flag.
extern "C" void emu_limb_sum(const double* v, int k, long long limbs[3], int* bad, double* value) {
  unsigned long long acc[3] = {0, 0, 0};
  int flag = 0;
  CostLimbEmit em{acc, 1, &flag};
  for (int i = 0; i < k; ++i) em(0, 0, v[i], true);
  for (int l = 0; l < 3; ++l) limbs[l] = (long long)acc[l];
  *bad = flag;
  *value = limb_value((long long)acc[0], (long long)acc[1], (long long)acc[2]);
}

namespace {
struct CountEmit {
  static constexpr bool kSparse = true;
  double f = 0.0; long emits = 0, pres = 0; std::vector<int>* colcnt;
  void skip(int) {}
  void operator()(int, int col, double, bool p) { ++emits; if (p && col >= 0) { ++pres; ++(*colcnt)[col]; } }
};
}
// Layout::cost_nslot: the slot path's LDS slots (0: the objective's gradient goes through the limbs); -1 = no layout
extern "C" int emu_cost_slots(const towr_problem_desc_t* d) {
  Layout L; std::string e;
  if (build_layout(*d, L, e)) return -1;
  return L.cost_nslot;
}

// the largest number of gradient contributions any one column receives at x (the count emu_cost_stats prints as
// max/col, without the printing): limb_value is exact below 2^11 of them; -1 = no layout
extern "C" int emu_cost_col_max(const towr_problem_desc_t* d, const double* x) {
  Layout L; std::string e;
  if (build_layout(*d, L, e)) return -1;
  std::vector<int> colcnt(L.n + 1, 0);
  Ctx c{};
  c.x = x; c.nodecol = L.nodecol.data(); c.spl = L.spl.data(); c.dur = L.dur.data();
  c.ter = &L.terrain; c.rb = L.rb; c.fdisc_motion = L.fdisc_motion;
  c.gait = L.gait; c.pinfo = L.pinfo.data(); c.pcols = L.pcols.data(); c.pact = L.pact.data(); c.sched = L.sched.data();
  c.eelin = L.eelin.data(); c.rotvec = L.rotvec; c.cq = L.cost_q.data();
  for (const CostItem& it : L.cost_items) {
    if (it.type >= CT_COUNT) continue;   // a no-op lane of the wave schedule
    c.seg = it.seg >= 0 ? L.segs.data() + (size_t)it.seg * L.spl.size() : nullptr;
    CountEmit em{}; em.colcnt = &colcnt;
    eval_cost_item(c, it, em);
  }
  int mx = 0;
  for (int j = 0; j < L.n; ++j) mx = std::max(mx, colcnt[j]);
  return mx;
}

// cost work statistics at x (experiment aid): items per type, emissions, contributions per column
extern "C" int emu_cost_stats(const towr_problem_desc_t* d, const double* x) {
  Layout L; std::string e;
  if (build_layout(*d, L, e)) return -1;
  std::vector<int> colcnt(L.n + 1, 0);
  Ctx c{};
  c.x = x; c.nodecol = L.nodecol.data(); c.spl = L.spl.data(); c.dur = L.dur.data();
  c.ter = &L.terrain; c.rb = L.rb; c.fdisc_motion = L.fdisc_motion;
  c.gait = L.gait; c.pinfo = L.pinfo.data(); c.pcols = L.pcols.data(); c.pact = L.pact.data(); c.sched = L.sched.data();
  c.eelin = L.eelin.data(); c.rotvec = L.rotvec; c.cq = L.cost_q.data();
  long n_t[CT_COUNT] = {}, em_t[CT_COUNT] = {}, pr_t[CT_COUNT] = {}, mx_t[CT_COUNT] = {};
  for (const CostItem& it : L.cost_items) {
    if (it.type >= CT_COUNT) continue;   // a no-op lane of the wave schedule
    c.seg = it.seg >= 0 ? L.segs.data() + (size_t)it.seg * L.spl.size() : nullptr;
    CountEmit em{}; em.colcnt = &colcnt;
    eval_cost_item(c, it, em);
    n_t[it.type]++; em_t[it.type] += em.emits; pr_t[it.type] += em.pres; mx_t[it.type] = std::max(mx_t[it.type], em.emits);
  }
  for (int t = 0; t < CT_COUNT; ++t)
    if (n_t[t]) std::printf("cost type %d: items %ld emits %ld present %ld max/item %ld\n", t, n_t[t], em_t[t], pr_t[t], mx_t[t]);
  int touched = 0, mx = 0; long tot = 0;
  for (int j = 0; j < L.n; ++j) if (colcnt[j]) { ++touched; mx = std::max(mx, colcnt[j]); tot += colcnt[j]; }
  std::printf("n %d touched %d contributions %ld max/col %d\n", L.n, touched, tot, mx);
  return 0;
}

// The composers' encoding bounds over every streamed block (layout.h kFloatDivMax, GsSeg int16 positions):
// out[0..2] per GsClass: streamed (0/1); out[3..5]: its largest positions per instant (Lsum, GsGeo::Li);
// out[6]: the largest CSR range of any FsBlock or GsBlock; out[7]: FDISC streamed
extern "C" int emu_stream_limits(const towr_problem_desc_t* d, int64_t* out) {
  Layout L; std::string e;
  if (build_layout(*d, L, e)) return -1;
  int64_t nv = 0;
  for (int c = 0; c < GS_COUNT; ++c) {
    out[c] = L.gstream[c];
    int64_t li = 0;
    for (const GsGeo& g : L.gs_geo) if (g.cls == c) li = std::max<int64_t>(li, g.Li);
    out[3 + c] = li;
    for (const GsBlock& bl : L.gs_blocks[c]) nv = std::max<int64_t>(nv, bl.nv);
  }
  for (const FsBlock& fb : L.fs_blocks) nv = std::max<int64_t>(nv, fb.nv);
  out[6] = nv;
  out[7] = L.fstream;
  return 0;
}

// the small kinds' staged x (Layout::misc_xspan): out = {spans, 16-byte units staged, units of all of x}
extern "C" int emu_misc_xspan(const towr_problem_desc_t* d, int64_t* out) {
  Layout L; std::string e;
  if (build_layout(*d, L, e)) return -1;
  int64_t units = 0;
  for (size_t k = 1; k < L.misc_xspan.size(); k += 2) units += L.misc_xspan[k];
  out[0] = (int64_t)L.misc_xspan.size() / 2;
  out[1] = units;
  out[2] = (L.n + 1) / 2;
  return 0;
}

// layout statistics per item type (tiles, lanes used, candidates per wave, values per tile)
extern "C" int emu_stats(const towr_problem_desc_t* d) {
  Layout L; std::string e;
  if (build_layout(*d, L, e)) return -1;
  std::printf("fs tables: fs_t %zu fs_tmpl %zu fs_ws %zu fs_blocks %zu (bytes %zu)\n", L.fs_t.size(), L.fs_tmpl.size(), L.fs_ws.size(),
              L.fs_blocks.size(), 8 * L.fs_t.size() + 4 * L.fs_tmpl.size() + 4 * L.fs_ws.size() + sizeof(FsBlock) * L.fs_blocks.size() + 12 * L.fs_t.size());
  std::printf("fstream %d blocks %zu tmpl_max %d | gstream rom %d (%zu blocks) dyn %d (%zu blocks) tq %d (%zu blocks)\n", (int)L.fstream,
              L.fs_blocks.size(), L.fs_tmpl_max, (int)L.gstream[GS_ROM], L.gs_blocks[GS_ROM].size(), (int)L.gstream[GS_DYN],
              L.gs_blocks[GS_DYN].size(), (int)L.gstream[GS_TQ], L.gs_blocks[GS_TQ].size());
  std::printf("n %d m %d nnz %lld nodecol %zu | gait tables: spl %zu pinfo %zu pcols %zu pact %zu sched %zu\n", L.n, L.m,
              (long long)L.nnz, L.nodecol.size(), L.spl.size(), L.pinfo.size(), L.pcols.size(), L.pact.size(), L.sched.size());
  {
    auto a16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    int phs = 0;
    for (const SchedInfo& si : L.sched) phs = std::max(phs, (int)si.n_phases);
    const size_t tabs = a16(sizeof(SplineMeta) * L.spl.size()) + a16(sizeof(SchedInfo) * L.sched.size()) + a16(sizeof(PolyPhase) * L.pinfo.size()) +
                        a16(sizeof(int32_t) * L.pact.size()) + a16(sizeof(PhaseCol) * L.pcols.size());
    std::printf("record staging bytes: x %zu nodecol %zu tables %zu (spl %zu pinfo %zu pact %zu pcols %zu) timings %zu | state euler %zu rv %zu\n",
                8 * (size_t)((L.n + 2) & ~1), 16 * ((L.nodecol.size() + 3) / 4), tabs, sizeof(SplineMeta) * L.spl.size(),
                sizeof(PolyPhase) * L.pinfo.size(), sizeof(int32_t) * L.pact.size(), sizeof(PhaseCol) * L.pcols.size(),
                8 * (2 * L.pinfo.size() + L.sched.size() * phs), sizeof(DynEulerState), sizeof(DynRvState));
  }
  for (int cls = 0; cls < GS_COUNT; ++cls) {
    if (!L.gstream[cls]) continue;
    long nv = 0; int maxnv = 0;
    for (const GsBlock& bl : L.gs_blocks[cls]) { nv += bl.nv; maxnv = std::max(maxnv, bl.nv); }
    std::printf("gstream %d: instants %zu blocks %zu nmax %d geo_max {%d %d %d %d} values %ld max/block %d\n", cls, L.gs_inst[cls].size(),
                L.gs_blocks[cls].size(), L.gs_nmax[cls], L.gs_geo_max[cls][0], L.gs_geo_max[cls][1], L.gs_geo_max[cls][2],
                L.gs_geo_max[cls][3], nv, maxnv);
  }
  for (int t = 0; t < IT_COUNT; ++t) {
    int nt = L.type_tile0[t + 1] - L.type_tile0[t];
    if (!nt) continue;
    long used = 0, lanes = 0, candw = 0, cand = 0; int maxv = 0;
    for (int ti = L.type_tile0[t]; ti < L.type_tile0[t + 1]; ++ti) {
      const TileDesc& td = L.tiles[ti];
      maxv = std::max(maxv, td.v1 - td.v0);
      for (int w = td.i0; w < td.i1; w += 64) {
        int mc = 0;
        for (int l = w; l < std::min(w + 64, td.i1); ++l) {
          ++lanes;
          if (L.items[l].type != IT_NONE) { ++used; mc = std::max(mc, L.items[l].ncand); cand += L.items[l].ncand; }
        }
        candw += mc;
      }
    }
    std::printf("type %d: tiles %d block %d lanes %ld used %ld maxvals %d cand %ld sum_wave_maxcand %ld lds %d\n", t, nt,
                L.type_block[t], lanes, used, maxv, cand, candw, L.type_lds[t]);
  }
  return 0;
}

// LDS bank-conflict degree of the tile emission (ds_write_b64: 4 groups of 16 lanes, bank pair =
// double position mod 16): per item type, LDS cycles spent / conflict-free cycles, with the
// position map `swz` applied (0 = identity, 1 = the kernel's XOR swizzle)
extern "C" int emu_conflicts(const towr_problem_desc_t* d, int swz) {
  Layout L; std::string e;
  if (build_layout(*d, L, e)) return -1;
  for (int t = 0; t < IT_COUNT; ++t) {
    long cyc = 0, ideal = 0, wc[4] = {0, 0, 0, 0}, wi[4] = {0, 0, 0, 0};
    for (int ti = L.type_tile0[t]; ti < L.type_tile0[t + 1]; ++ti) {
      const TileDesc& td = L.tiles[ti];
      const int block = td.i1 - td.i0;
      for (int w = 0; w < block; w += 64) {
        int maxc = 0;
        for (int l = w; l < w + 64 && l < block; ++l)
          if (L.items[td.i0 + l].type != IT_NONE) maxc = std::max(maxc, L.items[td.i0 + l].ncand);
        for (int j = 0; j < maxc; ++j)
          for (int g = 0; g < 4; ++g) {
            int cnt[16] = {0}; bool any = false;
            for (int l = w + 16 * g; l < w + 16 * g + 16 && l < block; ++l) {
              const ItemDesc& it = L.items[td.i0 + l];
              if (it.type == IT_NONE || j >= it.ncand) continue;
              int pos = slot_pick(L.slot_groups[it.slot + (size_t)(j / 8) * block], j % 8);
              if (swz == 1 && pos < td.v1 - td.v0) { const int q = pos + (td.v0 & 1); pos = q ^ (((q >> 5) & 15) << 1); }
              if (swz == 2 && pos < td.v1 - td.v0) { const int q = pos + (td.v0 & 1); pos = q ^ (((q >> 4) & 7) << 1); }
              if (swz == 3 && pos < td.v1 - td.v0) { const int q = pos + (td.v0 & 1); pos = q ^ ((((q >> 4) ^ (q >> 7)) & 7) << 1); }
              cnt[pos & 15]++; any = true;
            }
            if (!any) continue;
            int m = 0; for (int q = 0; q < 16; ++q) m = std::max(m, cnt[q]);
            cyc += m; ideal += 1;
            if (w / 64 < 4) { wc[w / 64] += m; wi[w / 64] += 1; }
          }
      }
    }
    if (ideal) std::printf("type %d: lds write cycles %ld conflict-free %ld (x%.2f)  per wave %ld/%ld %ld/%ld %ld/%ld %ld/%ld\n", t, cyc, ideal,
                           (double)cyc / ideal, wc[0], wi[0], wc[1], wi[1], wc[2], wi[2], wc[3], wi[3]);
  }
  return 0;
}

// trajectory rows through engine_math.h's traj_row (host instantiation)
extern "C" int emu_traj(const towr_problem_desc_t* d, const double* x, double dt, double* out, int max_rows) {
  Layout L; std::string e;
  if (build_layout(*d, L, e)) return -1;
  std::vector<double> pd((size_t)TOWR_MAX_EE * TOWR_MAX_PHASES, 0.0);
  std::vector<int32_t> pn(TOWR_MAX_EE, 0), pc(TOWR_MAX_EE, 0);
  for (int ee = 0; ee < d->robot.n_ee; ++ee) {
    pn[ee] = d->n_phases[ee]; pc[ee] = d->contact_at_start[ee] != 0;
    for (int q = 0; q < d->n_phases[ee]; ++q) pd[(size_t)ee * TOWR_MAX_PHASES + q] = d->phase_durations[ee][q];
  }
  TrajPhases ph{pd.data(), pn.data(), pc.data()};
  Ctx c{};
  c.x = x; c.nodecol = L.nodecol.data(); c.spl = L.spl.data(); c.dur = L.dur.data();
  c.ter = &L.terrain; c.rb = L.rb; c.fdisc_motion = L.fdisc_motion;
  c.gait = L.gait; c.pinfo = L.pinfo.data(); c.pcols = L.pcols.data(); c.sched = L.sched.data();
  c.eelin = L.eelin.data(); c.rotvec = L.rotvec;
  double T = 0.0;
  for (int i = 0; i < L.spl[0].n_polys; ++i) T += L.dur[L.spl[0].dur_off + i];
  const int cols = traj_cols(L.rb.n_ee);
  int k = 0;
  for (double t = 0.0; t <= T + 1e-9; t += dt, ++k)
    if (k < max_rows) traj_row(c, ph, t, out + (size_t)k * cols, 1);
  return k;
}

// The product tables of build_jprod (Layout::jp_chunks, jp_rseg, jp_cseg, jp_cidx, jp_empty_rows, jp_row) as plain
// arrays. sizes (10): chunks, row segments, column segments, empty rows, jp_long, kJpChunk, nnz, m, n, kGnBlock. An output that
// is null is skipped (a first call with all of them null gives the sizes to allocate). chunks: {rs0, rns, rnl, cs0,
// cns, cnl} per chunk; rseg / cseg: {out, q0, len, flags} per segment; cidx: kJpChunk entries per chunk.
// emu_jp_tables_ex: the same for a description with side data, and a tenth size: kGnBlock (the block of
// towr_gn_direction_kernel, by which the tests classify that kernel's branches without a constant of their own).
extern "C" int emu_jp_tables_ex(const towr_problem_desc_t* d, int n_data, const towr_data_t* data, int64_t* sizes, int32_t* chunks,
                                int32_t* rseg, int32_t* cseg, uint16_t* cidx, int32_t* empty_rows, int32_t* row) {
  Layout L; std::string e;
  if (build_layout_ex(*d, n_data, data, L, e)) return -1;
  const int64_t sz[10] = {(int64_t)L.jp_chunks.size(), (int64_t)L.jp_rseg.size(), (int64_t)L.jp_cseg.size(),
                          (int64_t)L.jp_empty_rows.size(), L.jp_long, kJpChunk, L.nnz, L.m, L.n, kGnBlock};
  for (int i = 0; i < 10; ++i) sizes[i] = sz[i];
  if (chunks)
    for (size_t c = 0; c < L.jp_chunks.size(); ++c) {
      const JpChunk& ch = L.jp_chunks[c];
      const int32_t v[6] = {ch.rs0, ch.rns, ch.rnl, ch.cs0, ch.cns, ch.cnl};
      for (int i = 0; i < 6; ++i) chunks[6 * c + i] = v[i];
    }
  auto segs = [](const std::vector<JpSeg>& from, int32_t* to) {
    for (size_t k = 0; to && k < from.size(); ++k) {
      to[4 * k] = from[k].out; to[4 * k + 1] = from[k].q0; to[4 * k + 2] = from[k].len; to[4 * k + 3] = from[k].flags;
    }
  };
  segs(L.jp_rseg, rseg);
  segs(L.jp_cseg, cseg);
  if (cidx) std::copy(L.jp_cidx.begin(), L.jp_cidx.end(), cidx);
  if (empty_rows) std::copy(L.jp_empty_rows.begin(), L.jp_empty_rows.end(), empty_rows);
  if (row) std::copy(L.jp_row.begin(), L.jp_row.end(), row);
  return 0;
}
extern "C" int emu_jp_tables(const towr_problem_desc_t* d, int64_t* sizes, int32_t* chunks, int32_t* rseg, int32_t* cseg,
                             uint16_t* cidx, int32_t* empty_rows, int32_t* row) {
  return emu_jp_tables_ex(d, 0, nullptr, sizes, chunks, rseg, cseg, cidx, empty_rows, row);
}

// The two product kernels of jprod.hip for one problem, as a host walk of the same tables in the same order, so that
// every output is the kernel's own tree of additions: the product is rounded into the chunk's tile before it is
// summed; a short segment is summed by one lane in ascending order; a long one by 64 lanes (lane l: entries l,
// l + 64, ... in order), then the __shfl_down tree with offsets 32..1 (lane 0's value); a row cut by a chunk boundary
// goes through the two-slot carry picked by the chunk's parity; a column's chunk sums join its running sum in chunk
// order; `accumulate` leaves a column without entries alone. V (nnz), P, Z0 (n), LAM (m) -> Y (m: J P), Z (n: J^T LAM),
// Za (n: Z0 + J^T LAM). The tile starts as NaN and so do the carries: a segment that reads an entry its chunk did not
// write, or a carry that was not handed on, shows in the output. No contraction anywhere below: the kernels cannot
// fuse a product with the sum either, since the product goes through LDS.
#pragma clang fp contract(off)
namespace {
double jp_seg_sum(const JpSeg& s, const double* tile, const uint16_t* cidx, bool wave) {
  const int q0 = cidx ? (s.q0 & (kJpChunk - 1)) : s.q0;
  double lane[64];
  const int lanes = wave ? 64 : 1;
  for (int l = 0; l < lanes; ++l) {
    double acc = 0.0;
    for (int i = l; i < s.len; i += lanes) acc += tile[cidx ? cidx[q0 + i] : q0 + i];
    lane[l] = acc;
  }
  if (wave)
    for (int o = 32; o > 0; o >>= 1)
      for (int l = 0; l < o; ++l) lane[l] += lane[l + o];
  return lane[0];
}
}
extern "C" int emu_jac_products_ex(const towr_problem_desc_t* d, int n_data, const towr_data_t* data, const double* V,
                                   const double* P, const double* LAM, const double* Z0, double* Y, double* Z, double* Za) {
  Layout L; std::string e;
  if (build_layout_ex(*d, n_data, data, L, e)) return -1;
  const int n_chunks = (int)L.jp_chunks.size();
  std::vector<double> tile((size_t)kJpChunk, std::nan("")), zacc((size_t)L.n, 0.0);
  double carry[2] = {std::nan(""), std::nan("")};
  for (int32_t r : L.jp_empty_rows) Y[r] = 0.0;
  for (int ci = 0; ci < n_chunks; ++ci) {   // towr_jac_vec_kernel
    const int64_t k0 = (int64_t)ci * kJpChunk, k1 = std::min<int64_t>(L.nnz, k0 + kJpChunk);
    const JpChunk& ch = L.jp_chunks[ci];
    for (int64_t k = k0; k < k1; ++k) tile[(size_t)(k - k0)] = V[k] * P[L.col[k]];
    for (int q = 0; q < ch.rns + ch.rnl; ++q) {
      const JpSeg& s = L.jp_rseg[ch.rs0 + q];
      double sum = jp_seg_sum(s, tile.data(), nullptr, q >= ch.rns);
      if (s.flags & 1) sum = carry[(ci & 1) ^ 1] + sum;
      if (s.flags & 2) carry[ci & 1] = sum;
      else Y[s.out] = sum;
    }
  }
  std::fill(tile.begin(), tile.end(), std::nan(""));
  for (int ci = 0; ci < n_chunks; ++ci) {   // towr_jac_tvec_kernel
    const int64_t k0 = (int64_t)ci * kJpChunk, k1 = std::min<int64_t>(L.nnz, k0 + kJpChunk);
    const JpChunk& ch = L.jp_chunks[ci];
    for (int64_t k = k0; k < k1; ++k) tile[(size_t)(k - k0)] = V[k] * LAM[L.jp_row[k]];
    const uint16_t* cidx = L.jp_cidx.data() + k0;
    for (int q = 0; q < ch.cns + ch.cnl; ++q) {
      const JpSeg& s = L.jp_cseg[ch.cs0 + q];
      zacc[s.out] += jp_seg_sum(s, tile.data(), cidx, q >= ch.cns);
    }
  }
  for (int j = 0; j < L.n; ++j) {
    Z[j] = zacc[j];
    Za[j] = Z0[j];
    if (L.col_ptr[j + 1] != L.col_ptr[j]) Za[j] += zacc[j];
  }
  return 0;
}
extern "C" int emu_jac_products(const towr_problem_desc_t* d, const double* V, const double* P, const double* LAM,
                                const double* Z0, double* Y, double* Z, double* Za) {
  return emu_jac_products_ex(d, 0, nullptr, V, P, LAM, Z0, Y, Z, Za);
}

// towr_gn_direction_kernel (jprod.hip) for one problem, operation for operation: the held rule, act (a NaN is active),
// and per CG step t = act .* (J p) through the row segments with their carries (t = 0 on empty rows), z = J^T t through
// the column segments into running sums in chunk order, hp = rho z + mu p on the free columns, the dot products,
// al = rr / pHp, the updates of D, r and p, and the stop tests in the kernel's order and form; then D on the held
// columns (everywhere when no step completed), the slope and the six SUM entries. Every dot product is the kernel's
// tree: lane l's partial over its columns l, l + kGnBlock, ... in order from 0.0, the 64-lane __shfl_down tree of
// each wave (offsets 32..1, lane 0's value), the waves' partials added in wave order. X null: every column is free
// (XL / XU are not read). The tile is refilled with NaN before every chunk of every pass and the carries before every
// pass: a segment that reads what its chunk did not write, or a carry not handed on, shows as NaN in D.
// Returns 0; -1: the layout failed; -2: n is past the kernel's held mask (kGnMaxN).
namespace {
double gn_block_sum(const std::vector<double>& lane) {   // lane: kGnBlock partials
  double part[kGnBlock / 64];
  for (int w = 0; w < kGnBlock / 64; ++w) {
    double v[64];
    for (int l = 0; l < 64; ++l) v[l] = lane[(size_t)w * 64 + l];
    for (int o = 32; o > 0; o >>= 1)
      for (int l = 0; l < o; ++l) v[l] += v[l + o];
    part[w] = v[0];
  }
  double t = part[0];
  for (int w = 1; w < kGnBlock / 64; ++w) t += part[w];
  return t;
}
}
extern "C" int emu_gn_direction_ex(const towr_problem_desc_t* d, int n_data, const towr_data_t* data, const double* V,
                                   const double* LAMP, const double* GR, const double* X, const double* XL, const double* XU,
                                   double rho, double mu, double tol, int ncg, double* D, double* SUM) {
  Layout L; std::string e;
  if (build_layout_ex(*d, n_data, data, L, e)) return -1;
  if (L.n > kGnMaxN) return -2;
  const int n = L.n, m = L.m, n_chunks = (int)L.jp_chunks.size();
  const double nan = std::nan("");
  std::vector<double> p((size_t)n), r((size_t)n), z((size_t)n), t((size_t)m, nan), tile((size_t)kJpChunk), lane((size_t)kGnBlock);
  std::vector<uint8_t> held((size_t)n, 0), act((size_t)m);
  const double tol2 = tol * tol;
  // term(j, acc) on lane tid's columns in the lane's order (acc: its partial), then the block's tree
  auto lane_sums = [&](auto&& term) {
    for (int tid = 0; tid < kGnBlock; ++tid) {
      double acc = 0.0;
      for (int j = tid; j < n; j += kGnBlock) term(j, acc);
      lane[(size_t)tid] = acc;
    }
    return gn_block_sum(lane);
  };

  for (int j = 0; j < n; ++j) {
    const double g = GR[j];
    bool h = false;
    if (X) {
      const double x = X[j], l = XL[j], u = XU[j];
      const bool has_l = l > -kSideInf, has_u = u < kSideInf;
      h = (has_l && x <= l && g > 0.0) || (has_u && x >= u && g < 0.0) || (has_l && has_u && l == u);
    }
    held[(size_t)j] = h;
    p[(size_t)j] = r[(size_t)j] = h ? 0.0 : g;
  }
  const double bb = lane_sums([&](int j, double& acc) { if (!held[(size_t)j]) acc += GR[j] * GR[j]; });
  const double nheld = lane_sums([&](int j, double& acc) { if (held[(size_t)j]) acc += 1.0; });
  for (int i = 0; i < m; ++i) act[(size_t)i] = LAMP[i] != 0.0;
  for (int32_t i : L.jp_empty_rows) t[(size_t)i] = 0.0;

  double rr = bb;
  int steps = 0, code = 0;
  if (bb == 0.0) code = 3;
  else {
    for (int it = 0; it < ncg; ++it) {
      if (rr <= tol2 * bb) { code = 1; break; }
      std::fill(z.begin(), z.end(), 0.0);
      double carry[2] = {nan, nan};
      for (int ci = 0; ci < n_chunks; ++ci) {   // gn_jp_pass
        const int64_t k0 = (int64_t)ci * kJpChunk, k1 = std::min<int64_t>(L.nnz, k0 + kJpChunk);
        const JpChunk& ch = L.jp_chunks[(size_t)ci];
        std::fill(tile.begin(), tile.end(), nan);
        for (int64_t k = k0; k < k1; ++k) tile[(size_t)(k - k0)] = V[k] * p[(size_t)L.col[(size_t)k]];
        for (int q = 0; q < ch.rns + ch.rnl; ++q) {
          const JpSeg& s = L.jp_rseg[(size_t)(ch.rs0 + q)];
          double sum = jp_seg_sum(s, tile.data(), nullptr, q >= ch.rns);
          if (s.flags & 1) sum = carry[(ci & 1) ^ 1] + sum;
          if (s.flags & 2) carry[ci & 1] = sum;
          else t[(size_t)s.out] = (act[(size_t)s.out] ? 1.0 : 0.0) * sum;
        }
      }
      for (int ci = 0; ci < n_chunks; ++ci) {   // gn_jtt_pass
        const int64_t k0 = (int64_t)ci * kJpChunk, k1 = std::min<int64_t>(L.nnz, k0 + kJpChunk);
        const JpChunk& ch = L.jp_chunks[(size_t)ci];
        std::fill(tile.begin(), tile.end(), nan);
        for (int64_t k = k0; k < k1; ++k) tile[(size_t)(k - k0)] = V[k] * t[(size_t)L.jp_row[(size_t)k]];
        const uint16_t* cidx = L.jp_cidx.data() + k0;
        for (int q = 0; q < ch.cns + ch.cnl; ++q) {
          const JpSeg& s = L.jp_cseg[(size_t)(ch.cs0 + q)];
          z[(size_t)s.out] += jp_seg_sum(s, tile.data(), cidx, q >= ch.cns);
        }
      }
      const double php = lane_sums([&](int j, double& acc) {
        double hp = 0.0;
        if (!held[(size_t)j]) {
          const double pj = p[(size_t)j];
          hp = rho * z[(size_t)j] + mu * pj;
          acc += pj * hp;
        }
        z[(size_t)j] = hp;
      });
      if (!(php > 0.0)) { code = 2; break; }
      const double al = rr / php;
      const double rn = lane_sums([&](int j, double& acc) {
        if (held[(size_t)j]) return;
        const double d0 = steps ? D[j] : 0.0;
        D[j] = d0 + al * p[(size_t)j];
        const double rj = r[(size_t)j] - al * z[(size_t)j];
        r[(size_t)j] = rj;
        acc += rj * rj;
      });
      const double beta = rn / rr;
      for (int j = 0; j < n; ++j)
        if (!held[(size_t)j]) p[(size_t)j] = r[(size_t)j] + beta * p[(size_t)j];
      rr = rn;
      ++steps;
    }
  }
  const double slope = lane_sums([&](int j, double& acc) {
    const double g = GR[j];
    double dj = g;
    if (steps && !held[(size_t)j]) dj = D[j];
    else D[j] = g;
    acc += g * dj;
  });
  SUM[0] = (double)steps; SUM[1] = bb; SUM[2] = rr; SUM[3] = slope; SUM[4] = nheld; SUM[5] = (double)code;
  return 0;
}
#pragma clang fp contract(fast)

// whether every polynomial's active-window PhaseCols (pact window, then up to kGsAct entries: n, ids, derivs) coincide
// over the three dimensions, per spline (experiment aid: the record composers' window sums per dimension)
extern "C" int emu_window_dims(const towr_problem_desc_t* d) {
  Layout L; std::string e;
  if (build_layout(*d, L, e)) return -1;
  for (size_t s = 0; s < L.spl.size(); ++s) {
    const SplineMeta& m = L.spl[s];
    if (m.ee < 0) continue;
    int same = 1;
    for (int p = 0; p < m.n_polys && same; ++p) {
      int a[3], z[3];
      for (int k = 0; k < 3; ++k) { a[k] = L.pact[m.pact_off + 2 * (k * m.n_polys + p)]; z[k] = L.pact[m.pact_off + 2 * (k * m.n_polys + p) + 1]; }
      for (int k = 1; k < 3 && same; ++k) {
        if (z[k] - a[k] != z[0] - a[0]) { same = 0; break; }
        for (int q = 0; q < kGsAct && a[0] + q <= z[0]; ++q) {
          const PhaseCol& c0 = L.pcols[m.pcol_off[0] + a[0] + q];
          const PhaseCol& ck = L.pcols[m.pcol_off[k] + a[k] + q];
          if (c0.n != ck.n) { same = 0; break; }
          for (int j = 0; j < c0.n; ++j) if (c0.id[j] != ck.id[j] || c0.deriv[j] != ck.deriv[j]) same = 0;
        }
      }
    }
    std::printf("spline %zu ee %d: dims coincide %d\n", s, m.ee, same);
  }
  return 0;
}
