// auglag.hip — the batched solver-step entry points of the C-ABI (include/towr_gpu.h), what a device-resident
// augmented-Lagrangian loop calls between evaluations: Jacobian products (J p, J^T lam), constraint residuals and
// multiplier updates, the projected step, the L-BFGS history and direction, the Gauss-Newton direction (CG, or direct
// with its ordering and envelope found here on the host), and the
// fused sequences of these behind an evaluation, and the solve driver that runs those sequences in rounds and compacts the
// frozen problems out of the batch between them. Host code only: the kernels live in jprod.hip, resid.hip, step.hip and lbfgs.hip, their argument
// structs in layout.h. The evaluator (towr_gpu.hip) is used through handle.h alone: launch, launch_cost,
// batch_terrain, bind and the scratch helpers.
//
// Every entry point checks its arguments first (before bind: a layout-only handle still answers them), puts the
// caller's operands into the kernel's argument struct (layout.h; they lead it, in the C signature's order) and hands
// that to a launcher, which adds what the handle owns.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "handle.h"

using namespace tg;
using namespace tg::host;

void towr_gpu_handle_s::AugLag::release() {
  for (void* p : d_jp) if (p) (void)hipFree(p);
  for (void* p : d_gf) if (p) (void)hipFree(p);
  for (void* p : d_gt) if (p) (void)hipFree(p);
  void* rest[] = {d_pv, d_set_row0, d_blo, d_bup, d_rg, d_rl, d_set_col0, d_xlo, d_xup, d_sd, d_sf, d_pr};
  for (void* p : rest) if (p) (void)hipFree(p);
  if (h_head) (void)hipHostFree(h_head);
}

namespace {

// ---- padding and chunking -------------------------------------------------------------------------------------------
// leading dimension of a scratch matrix with k columns: rows on 128-byte boundaries
int64_t ld16(int64_t k) { return std::max<int64_t>(16, (k + 15) & ~int64_t(15)); }

// Problems per chunk of a fused entry's values scratch (d_pv): towr_gpu_set_products_chunk, or automatic.
// Automatic chunk: measured, a chunk sized to the Infinity Cache (128 MiB of values) gains nothing — the
// fused call at chunk = B costs what the three separate calls cost — and every further chunk costs its launch
// sequence and an underfilled chip (ANYmal gait, B = 1024: 18.8 ms in 15 chunks vs 2.6 ms in one). So the chunk is
// as large as a 2 GiB scratch allows (the footprint bound), cut into equal parts.
int chunk_plan(towr_gpu_handle h, int B) {
  constexpr int64_t kAutoBytes = int64_t(2) << 30;
  const int64_t cap = std::max<int64_t>(1, kAutoBytes / (8 * ld16(h->L.nnz)));
  const int64_t parts = (B + cap - 1) / cap;
  return (int)std::min<int64_t>(B, h->al.products_chunk > 0 ? h->al.products_chunk : (B + parts - 1) / parts);
}

// row c0 of an optional operand (NULL stays NULL)
template <class T>
T* row_at(T* p, int c0, int64_t ld) { return p ? p + (int64_t)c0 * ld : nullptr; }

// ---- device tables --------------------------------------------------------------------------------------------------
// Tables uploaded together on the first call that needs them (towr_gpu_create and the single-problem callbacks never
// pay for them; synchronous copies: that first call is not asynchronous). add() uploads one unless an earlier one
// failed; commit() stores the device pointers where they belong, or frees them all if any upload failed.
struct Uploads {
  towr_gpu_handle h;
  int rc = TOWR_OK;
  std::vector<std::pair<const void**, void*>> made;   // (where it belongs, the device copy)
  template <class T, class U>
  void add(U** dst, const std::vector<T>& src) {   // U: T or const T
    T* d = nullptr;
    if (rc == TOWR_OK) rc = upload(h, &d, src);
    if (d) made.emplace_back((const void**)dst, d);
  }
  int commit() {
    for (auto& m : made) if (rc) (void)hipFree(m.second); else *m.first = m.second;
    return rc;
  }
};

int products_ready(towr_gpu_handle h) {
  towr_gpu_handle_s::AugLag& al = h->al;
  if (al.jp_ready) return TOWR_OK;
  const Layout& L = h->L;
  const size_t lv = jp_vec_lds(L.n, L.m), lt = jp_tvec_lds(L.n, L.m);
  if (std::max(lv, lt) > kLdsMax) return fail(h, TOWR_ERR_UNSUPPORTED, "problem too large for the product kernels' LDS");
  if ((lv > 64 * 1024 && hipFuncSetAttribute(jp_vec_kernel(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lv) != hipSuccess) ||
      (lt > 64 * 1024 && hipFuncSetAttribute(jp_tvec_kernel(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lt) != hipSuccess))
    return fail(h, TOWR_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
  const std::vector<int32_t> cp32(L.col_ptr.begin(), L.col_ptr.end());
  Uploads u{h};
  JpArgs a{};
  u.add(&a.col, L.col); u.add(&a.row, L.jp_row); u.add(&a.cidx, L.jp_cidx); u.add(&a.rseg, L.jp_rseg); u.add(&a.cseg, L.jp_cseg);
  u.add(&a.chunks, L.jp_chunks); u.add(&a.empty_rows, L.jp_empty_rows); u.add(&a.col_ptr, cp32);
  if (int rc = u.commit()) return rc;
  a.nnz = L.nnz; a.n = L.n; a.m = L.m;
  a.n_chunks = (int32_t)L.jp_chunks.size(); a.n_empty = (int32_t)L.jp_empty_rows.size();
  for (size_t i = 0; i < u.made.size(); ++i) al.d_jp[i] = u.made[i].second;
  al.jp = a;
  al.jp_ready = true;
  return TOWR_OK;
}

// the GN direction kernel: the product tables, its dynamic LDS within the workgroup's (the static reduction buffers and
// the runtime's own share beside it: 1 KiB kept free) and the limit raised past the default 64 KiB where it needs more
int gn_fits(towr_gpu_handle h) {
  if (h->L.n > kGnMaxN || gn_direction_lds(h->L.n, h->L.m) + 1024 > kLdsMax)
    return fail(h, TOWR_ERR_UNSUPPORTED, "problem too large for the GN direction kernel's LDS");
  return TOWR_OK;
}
int gn_ready(towr_gpu_handle h) {
  if (int rc = products_ready(h)) return rc;
  towr_gpu_handle_s::AugLag& al = h->al;
  if (al.gn_ready) return TOWR_OK;
  if (int rc = gn_fits(h)) return rc;
  const size_t lds = gn_direction_lds(h->L.n, h->L.m);
  for (const void* k : {gn_direction_kernel(), gn_direction_pc_kernel()})
    if (lds > 64 * 1024 && hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return fail(h, TOWR_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
  al.gn_ready = true;
  return TOWR_OK;
}

// ---- the direct GN direction's symbolic phase (towr_gpu_gn_factor_info) ------------------------------------------------
// The ordering is reverse Cuthill-McKee on the graph of J^T J (two columns are adjacent when a row holds both): per
// connected component, components taken in the order of their (degree, index)-smallest column, a breadth-first search
// that appends a node's unvisited neighbours by ascending (degree, index); the whole sequence reversed. Two start rules
// are run — the component's (degree, index)-smallest column itself, and the George-Liu pseudo-peripheral node found
// from it (repeat: the (degree, index)-smallest node of the last level of the search from the current node, while the
// depth grows) — and the ordering with the smaller envelope is kept (the pseudo-peripheral one on a tie). Everything is
// a function of the pattern alone.
using Adjacency = std::vector<std::vector<int32_t>>;

Adjacency jtj_adjacency(const Layout& L) {
  Adjacency adj(L.n);
  std::vector<int32_t> mark(L.n, -1);
  for (int j = 0; j < L.n; ++j) {
    mark[j] = j;
    for (int64_t p = L.col_ptr[j]; p < L.col_ptr[j + 1]; ++p) {
      const int i = L.csc_row[p];
      for (int64_t e = L.row_ptr[i]; e < L.row_ptr[i + 1]; ++e) {
        const int k = L.col[e];
        if (mark[k] != j) { mark[k] = j; adj[j].push_back(k); }
      }
    }
    std::sort(adj[j].begin(), adj[j].end());
  }
  return adj;
}

// (degree, index) order
struct ByDegree {
  const Adjacency& adj;
  bool operator()(int32_t u, int32_t v) const {
    return adj[u].size() != adj[v].size() ? adj[u].size() < adj[v].size() : u < v;
  }
};

int32_t pseudo_peripheral(const Adjacency& adj, int32_t s, std::vector<int32_t>& dist, std::vector<int32_t>& queue) {
  const ByDegree less{adj};
  int depth = -1;
  for (;;) {
    queue.assign(1, s);
    dist[s] = 0;
    for (size_t head = 0; head < queue.size(); ++head)
      for (int32_t v : adj[queue[head]])
        if (dist[v] < 0) { dist[v] = dist[queue[head]] + 1; queue.push_back(v); }
    const int d = dist[queue.back()];
    int32_t cand = queue.back();
    for (int32_t v : queue)
      if (dist[v] == d && less(v, cand)) cand = v;
    for (int32_t v : queue) dist[v] = -1;
    if (d <= depth || cand == s) return s;
    depth = d;
    s = cand;
  }
}

// order[q] = the column at permuted position q
std::vector<int32_t> reverse_cuthill_mckee(const Adjacency& adj, bool peripheral) {
  const int n = (int)adj.size();
  const ByDegree less{adj};
  std::vector<int32_t> by_degree(n), order, dist(n, -1), queue;
  for (int j = 0; j < n; ++j) by_degree[j] = j;
  std::sort(by_degree.begin(), by_degree.end(), less);
  std::vector<char> seen(n, 0);
  order.reserve(n);
  for (int32_t s : by_degree) {
    if (seen[s]) continue;
    if (peripheral) s = pseudo_peripheral(adj, s, dist, queue);
    size_t head = order.size();
    order.push_back(s);
    seen[s] = 1;
    for (; head < order.size(); ++head) {
      const size_t a0 = order.size();
      for (int32_t v : adj[order[head]])
        if (!seen[v]) { seen[v] = 1; order.push_back(v); }
      std::sort(order.begin() + a0, order.end(), less);
    }
  }
  std::reverse(order.begin(), order.end());
  return order;
}

// pos and first of an ordering; returns the envelope (entries of the lower triangle with the diagonal)
int64_t envelope_of(const Adjacency& adj, const std::vector<int32_t>& order, std::vector<int32_t>& pos, std::vector<int32_t>& first) {
  const int n = (int)adj.size();
  pos.assign(n, 0);
  first.assign(n, 0);
  for (int q = 0; q < n; ++q) pos[order[q]] = q;
  int64_t env = 0;
  for (int q = 0; q < n; ++q) {
    int32_t f = q;
    for (int32_t v : adj[order[q]]) f = std::min(f, pos[v]);
    first[q] = f;
    env += q - f + 1;
  }
  return env;
}

// the host tables of the direct direction, once per handle (a layout-only handle too)
void gn_factor_tables(towr_gpu_handle h) {
  towr_gpu_handle_s::AugLag& al = h->al;
  if (al.gf_built) return;
  const int n = h->L.n;
  const Adjacency adj = jtj_adjacency(h->L);
  std::vector<int32_t> pos, first;
  al.gf_inv = reverse_cuthill_mckee(adj, true);
  al.gf_env = envelope_of(adj, al.gf_inv, al.gf_pos, al.gf_first);
  const std::vector<int32_t> plain = reverse_cuthill_mckee(adj, false);
  if (envelope_of(adj, plain, pos, first) < al.gf_env) {
    al.gf_inv = plain;
    al.gf_env = envelope_of(adj, plain, al.gf_pos, al.gf_first);
  }
  al.gf_last.assign(n, 0);
  al.gf_row_off.assign(n + 1, 0);
  al.gf_width = 0;
  int64_t off = 0;
  for (int q = 0; q < n; ++q) {
    const int32_t f = al.gf_first[q];
    al.gf_width = std::max(al.gf_width, q - f);
    al.gf_last[q] = q;
    for (int c = f; c < q; ++c) al.gf_last[c] = q;   // (q ascending: the last writer is the largest row)
    al.gf_row_off[q] = (int32_t)std::min<int64_t>(off, INT32_MAX);
    off += q - f + 1;
  }
  al.gf_row_off[n] = (int32_t)std::min<int64_t>(off, INT32_MAX);
  al.gf_built = true;
}

// the direct direction's kernel: its offsets are 32-bit and its per-column state and pivot rows live in LDS (1 KiB kept
// free beside it, as for the CG kernel)
int gn_direct_fits(towr_gpu_handle h) {
  gn_factor_tables(h);
  if (h->al.gf_env > INT32_MAX || gn_direct_lds(h->L.n, h->L.m, h->al.gf_width) + 1024 > kLdsMax)
    return fail(h, TOWR_ERR_UNSUPPORTED, "problem too large for the direct GN direction (envelope >= 2^31 entries, or its LDS)");
  return TOWR_OK;
}
int gn_direct_ready(towr_gpu_handle h) {
  if (int rc = products_ready(h)) return rc;
  towr_gpu_handle_s::AugLag& al = h->al;
  if (al.gnd_ready) return TOWR_OK;
  if (int rc = gn_direct_fits(h)) return rc;
  const size_t lds = gn_direct_lds(h->L.n, h->L.m, al.gf_width);
  if (lds > 64 * 1024 && hipFuncSetAttribute(gn_direct_kernel(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return fail(h, TOWR_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
  Uploads u{h};
  const int32_t* d[7] = {};
  u.add(&d[0], al.gf_pos); u.add(&d[1], al.gf_inv); u.add(&d[2], al.gf_first); u.add(&d[3], al.gf_last); u.add(&d[4], al.gf_row_off);
  u.add(&d[5], h->L.csc_row); u.add(&d[6], h->L.csc_index);
  if (int rc = u.commit()) return rc;
  for (int i = 0; i < 7; ++i) al.d_gf[i] = const_cast<int32_t*>(d[i]);
  al.gnd_ready = true;
  return TOWR_OK;
}

// ---- the tiled direct direction's symbolic phase (towr_gpu_gn_tile_info) -------------------------------------------------
// The 16 x 16 tile envelope of the ordering above: block row I stores the tiles bfirst[I] .. I. A block envelope has no
// fill outside itself, so this is the whole symbolic phase. Once per handle (a layout-only handle too).
void gn_tile_tables(towr_gpu_handle h) {
  gn_factor_tables(h);
  towr_gpu_handle_s::AugLag& al = h->al;
  if (al.gt_built) return;
  const int n = h->L.n, nt = (n + kGnTile - 1) / kGnTile;
  al.gt_bfirst.assign(nt, 0);
  al.gt_tile_off.assign(nt + 1, 0);
  std::vector<std::vector<int32_t>> below(nt);   // per block column the block rows under its diagonal tile
  int64_t off = 0;
  for (int I = 0; I < nt; ++I) {
    int32_t bf = I;
    for (int q = kGnTile * I; q < std::min(n, kGnTile * (I + 1)); ++q) bf = std::min(bf, al.gf_first[q] / kGnTile);
    al.gt_bfirst[I] = bf;
    al.gt_tile_off[I] = (int32_t)std::min<int64_t>(off, INT32_MAX);
    off += I - bf + 1;
    for (int K = bf; K < I; ++K) below[K].push_back(I);   // (I ascending)
  }
  al.gt_tile_off[nt] = (int32_t)std::min<int64_t>(off, INT32_MAX);
  al.gt_tiles = off;
  al.gt_col_ptr.assign(nt + 1, 0);
  al.gt_col_rows.clear();
  for (int J = 0; J < nt; ++J) {
    al.gt_col_ptr[J] = (int32_t)al.gt_col_rows.size();
    al.gt_col_rows.insert(al.gt_col_rows.end(), below[J].begin(), below[J].end());
  }
  al.gt_col_ptr[nt] = (int32_t)al.gt_col_rows.size();
  al.gt_terms = 0;   // one per row and pair of its columns, the diagonal included
  for (int i = 0; i < h->L.m; ++i) {
    const int64_t len = h->L.row_ptr[i + 1] - h->L.row_ptr[i];
    al.gt_terms += len * (len + 1) / 2;
  }
  al.gt_built = true;
}

// The assembly's terms (layout.h GnAsmTerm), for the upload: per stored entry (q, c), c <= q, the rows of J that hold
// both columns, ascending, with the two CSR entries — column inv[q]'s first, as the direct kernel multiplies them.
void gn_tile_assembly(towr_gpu_handle h, std::vector<int32_t>& ptr, std::vector<GnAsmTerm>& terms) {
  const Layout& L = h->L;
  const towr_gpu_handle_s::AugLag& al = h->al;
  auto slot = [&](int q, int c) {
    const int I = q / kGnTile, K = c / kGnTile;
    return 256 * (al.gt_tile_off[I] + K - al.gt_bfirst[I]) + kGnTile * (c % kGnTile) + q % kGnTile;
  };
  ptr.assign((size_t)(256 * al.gt_tiles + 1), 0);
  std::vector<int32_t> fill;
  for (int pass = 0; pass < 2; ++pass) {
    for (int i = 0; i < L.m; ++i)
      for (int64_t x = L.row_ptr[i]; x < L.row_ptr[i + 1]; ++x)
        for (int64_t y = L.row_ptr[i]; y < L.row_ptr[i + 1]; ++y) {
          const int q = al.gf_pos[L.col[x]], c = al.gf_pos[L.col[y]];
          if (c > q) continue;
          const int e = slot(q, c);
          if (pass == 0) ++ptr[e + 1];
          else terms[fill[e]++] = GnAsmTerm{(int32_t)x, (int32_t)y, i};
        }
    if (pass == 0) {
      for (size_t e = 1; e < ptr.size(); ++e) ptr[e] += ptr[e - 1];
      fill.assign(ptr.begin(), ptr.end() - 1);
      terms.resize((size_t)ptr.back());
    }
  }
}

// the tiled kernel: its offsets into a workspace row are 32-bit; its LDS holds per-column state only
int gn_tiled_fits(towr_gpu_handle h) {
  gn_tile_tables(h);
  if (256 * h->al.gt_tiles > INT32_MAX || h->al.gt_terms > INT32_MAX || gn_tiled_lds(h->L.n, h->L.m) + 1024 > kLdsMax)
    return fail(h, TOWR_ERR_UNSUPPORTED, "problem too large for the tiled GN direction (256 tiles or the assembly's terms >= 2^31, or its LDS)");
  return TOWR_OK;
}
int gn_tiled_ready(towr_gpu_handle h) {
  if (int rc = products_ready(h)) return rc;
  towr_gpu_handle_s::AugLag& al = h->al;
  if (al.gnt_ready) return TOWR_OK;
  if (int rc = gn_tiled_fits(h)) return rc;
  const size_t lds = gn_tiled_lds(h->L.n, h->L.m);
  if (lds > 64 * 1024 && hipFuncSetAttribute(gn_tiled_kernel(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return fail(h, TOWR_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
  std::vector<int32_t> asm_ptr;
  std::vector<GnAsmTerm> asm_terms;
  gn_tile_assembly(h, asm_ptr, asm_terms);
  Uploads u{h};
  const int32_t* d[7] = {};
  const GnAsmTerm* dt = nullptr;
  u.add(&d[0], al.gt_bfirst); u.add(&d[1], al.gt_tile_off); u.add(&d[2], al.gt_col_ptr); u.add(&d[3], al.gt_col_rows);
  u.add(&d[4], al.gf_pos); u.add(&d[5], al.gf_inv); u.add(&d[6], asm_ptr); u.add(&dt, asm_terms);
  if (int rc = u.commit()) return rc;
  for (int i = 0; i < 7; ++i) al.d_gt[i] = const_cast<int32_t*>(d[i]);
  al.d_gt[7] = const_cast<GnAsmTerm*>(dt);
  al.gnt_ready = true;
  return TOWR_OK;
}

// the residual kernel's tables: the sets' row ranges and, when every set's bounds are known, the description bounds
int residual_ready(towr_gpu_handle h) {
  towr_gpu_handle_s::AugLag& al = h->al;
  if (al.res_ready) return TOWR_OK;
  const Layout& L = h->L;
  std::vector<int32_t> row0;
  for (const ConsInfo& c : L.cons) row0.push_back(c.row0);
  row0.push_back(L.m);
  Uploads u{h};
  u.add(&al.d_set_row0, row0);
  if (L.bounds_err.empty()) { u.add(&al.d_blo, L.g_lower); u.add(&al.d_bup, L.g_upper); }
  if (int rc = u.commit()) return rc;
  al.res_ready = true;
  return TOWR_OK;
}

// the step kernel's tables: the variable sets' column ranges and the description's variable bounds
int step_ready(towr_gpu_handle h) {
  towr_gpu_handle_s::AugLag& al = h->al;
  if (al.step_ready) return TOWR_OK;
  const Layout& L = h->L;
  std::vector<int32_t> col0;
  for (const VarSetInfo& v : L.varsets) col0.push_back(v.col0);
  col0.push_back(L.n);
  Uploads u{h};
  u.add(&al.d_set_col0, col0); u.add(&al.d_xlo, L.x_lower); u.add(&al.d_xup, L.x_upper);
  if (int rc = u.commit()) return rc;
  al.step_ready = true;
  return TOWR_OK;
}

// ---- argument checks (before anything runs) ------------------------------------------------------------------------
// optional bounds (lo, up), `pair` in messages: both or neither; ldb is 0 (one row for every problem) or >= dim (`d`)
int box_args(towr_gpu_handle h, const double* lo, const double* up, int64_t ldb, int64_t dim, const char* pair, const char* d) {
  if ((lo == nullptr) != (up == nullptr)) return fail(h, TOWR_ERR_INVALID, std::string("only one of ") + pair + " given");
  if (lo && ldb != 0 && ldb < dim) return fail(h, TOWR_ERR_INVALID, std::string("ldb must be 0 (shared bounds) or >= ") + d);
  return TOWR_OK;
}

// the residual stage's operands (G is the entry's own business). lamp: the multiplier update runs — always in the
// fused entries, where a NULL LAMP only keeps lam+ in handle scratch
int residual_args(towr_gpu_handle h, const ResArgs& a, bool lamp) {
  const Layout& L = h->L;
  if (!a.SUM) return fail(h, TOWR_ERR_INVALID, "null SUM");
  if (a.lds < 4 + (int64_t)L.cons.size()) return fail(h, TOWR_ERR_INVALID, "lds smaller than 4 + n_constraints");
  if (int rc = box_args(h, a.GL, a.GU, a.ldb, L.m, "GL / GU", "m")) return rc;
  if (!a.GL && !L.bounds_err.empty()) return fail(h, TOWR_ERR_INVALID, L.bounds_err);
  if (lamp && !a.RHO && !(a.rho > 0)) return fail(h, TOWR_ERR_INVALID, "rho must be > 0 with LAMP");
  if (a.LAMP && a.ldlp < L.m) return fail(h, TOWR_ERR_INVALID, "leading dimension of LAMP smaller than m");
  if (lamp && a.LAM && a.ldl < L.m) return fail(h, TOWR_ERR_INVALID, "leading dimension of LAM smaller than m");
  return TOWR_OK;
}

// the step stage's operands (X, D and their leading dimensions are the entry's own business)
int step_args(towr_gpu_handle h, const StepArgs& a) {
  const Layout& L = h->L;
  if (!a.SUM) return fail(h, TOWR_ERR_INVALID, "null SUM");
  if (a.lds < 5 + (int64_t)L.varsets.size()) return fail(h, TOWR_ERR_INVALID, "lds smaller than 5 + n_varsets");
  if (int rc = box_args(h, a.XL, a.XU, a.ldb, L.n, "XL / XU", "n")) return rc;
  if (!a.ALPHA && a.alpha != a.alpha) return fail(h, TOWR_ERR_INVALID, "alpha is NaN");
  if (a.XP && a.ldxp < L.n) return fail(h, TOWR_ERR_INVALID, "leading dimension of XP smaller than n");
  return TOWR_OK;
}

// the history and summary of an L-BFGS stage (a: LbfgsUpdateArgs, lds_min 6, or LbfgsDirArgs, 5)
template <class Args>
int lbfgs_args(towr_gpu_handle h, const Args& a, int64_t lds_min) {
  if (!a.HS || !a.HY || !a.HMETA) return fail(h, TOWR_ERR_INVALID, "null HS, HY or HMETA");
  if (!a.SUM) return fail(h, TOWR_ERR_INVALID, "null SUM");
  if (a.mem < 1 || a.mem > TOWR_LBFGS_MAX_MEM) return fail(h, TOWR_ERR_INVALID, "mem outside 1..TOWR_LBFGS_MAX_MEM");
  if (a.ldh < h->L.n) return fail(h, TOWR_ERR_INVALID, "ldh smaller than n");
  if (a.lds < lds_min) return fail(h, TOWR_ERR_INVALID, lds_min == 6 ? "lds smaller than 6" : "lds smaller than 5");
  return TOWR_OK;
}
// the kernels' per-column state lives in LDS: the handle's n must fit (after bind: a layout-only handle has answered)
int lbfgs_fits(towr_gpu_handle h) {
  if (std::max(lbfgs_update_lds(h->L.n), lbfgs_direction_lds(h->L.n)) > kLbfgsMaxLds)
    return fail(h, TOWR_ERR_UNSUPPORTED, "n too large for the L-BFGS kernels' LDS");
  return TOWR_OK;
}

// the CG parameters of a GN direction (towr_gn_params_t) and where its outputs go
int gn_params(towr_gpu_handle h, const towr_gn_params_t* gn, const double* D, const double* SUM, int64_t lds) {
  if (!gn) return fail(h, TOWR_ERR_INVALID, "null gn params");
  if (gn->ncg < 1) return fail(h, TOWR_ERR_INVALID, "gn: ncg must be >= 1");
  if (!(gn->mu >= 0) || !(gn->tol >= 0)) return fail(h, TOWR_ERR_INVALID, "gn: mu or tol is negative or NaN");
  if (!D || !SUM) return fail(h, TOWR_ERR_INVALID, "null GN direction or summary (D / SUM, DC / GSUM)");
  if (lds < 6) return fail(h, TOWR_ERR_INVALID, "leading dimension of the GN summary smaller than 6");
  return TOWR_OK;
}

// [p, p + (B - 1) ld + len) and [q, ...) share a byte (B rows each; a NULL or B < 1 shares nothing)
bool rows_overlap(int B, const double* p, int64_t ldp, int64_t lenp, const double* q, int64_t ldq, int64_t lenq) {
  if (!p || !q || B < 1) return false;
  const double *pe = p + (int64_t)(B - 1) * ldp + lenp, *qe = q + (int64_t)(B - 1) * ldq + lenq;
  return p < qe && q < pe;
}

// the preconditioned entries' own arguments, behind gn_params: the choice, the M rows and the two summary entries more
int gn_pc_params(towr_gpu_handle h, int32_t precond, const double* PC, int64_t ldpc, int64_t lds) {
  if (precond != TOWR_GN_PC_NONE && precond != TOWR_GN_PC_JACOBI)
    return fail(h, TOWR_ERR_INVALID, "gn: precond outside {TOWR_GN_PC_NONE, TOWR_GN_PC_JACOBI}");
  if (precond == TOWR_GN_PC_JACOBI && !PC) return fail(h, TOWR_ERR_INVALID, "gn: null PC with TOWR_GN_PC_JACOBI");
  if (PC && ldpc < h->L.n) return fail(h, TOWR_ERR_INVALID, "gn: leading dimension of PC (ldpc) smaller than n");
  if (lds < 8) return fail(h, TOWR_ERR_INVALID, "leading dimension of the GN summary smaller than 8");
  return TOWR_OK;
}

// the direct direction's own arguments: of gn only the damping is read; where its outputs go; the caller's workspace
// (problem b of a call uses row b mod wrows)
// (tiled: the tiled direction's row of 256 doubles per stored tile instead of the envelope)
struct GnWorkspace { double* W; int64_t ldw; int32_t wrows; bool tiled = false; };
int64_t ws_used(towr_gpu_handle h, const GnWorkspace& ws) { return ws.tiled ? 256 * h->al.gt_tiles : h->al.gf_env; }
int gn_direct_params(towr_gpu_handle h, const towr_gn_params_t* gn, const double* D, const double* SUM, int64_t lds, const GnWorkspace& ws) {
  if (!gn) return fail(h, TOWR_ERR_INVALID, "null gn params");
  if (!(gn->mu >= 0)) return fail(h, TOWR_ERR_INVALID, "gn: mu is negative or NaN");
  if (!D || !SUM) return fail(h, TOWR_ERR_INVALID, "null GN direction or summary (D / SUM, DC / GSUM)");
  if (lds < 8) return fail(h, TOWR_ERR_INVALID, "leading dimension of the GN summary smaller than 8");
  if (!ws.W) return fail(h, TOWR_ERR_INVALID, "gn: null workspace W");
  if (ws.wrows < 1) return fail(h, TOWR_ERR_INVALID, "gn: wrows must be >= 1");
  if (ws.tiled) gn_tile_tables(h); else gn_factor_tables(h);
  if (ws.ldw < ws_used(h, ws))
    return fail(h, TOWR_ERR_INVALID, ws.tiled ? "gn: ldw smaller than ldw_min (towr_gpu_gn_tile_info)"
                                              : "gn: ldw smaller than ldw_min (towr_gpu_gn_factor_info)");
  return TOWR_OK;
}
// a workspace row in use shares a byte with [q, q + (B - 1) ld + len)
bool ws_overlap(towr_gpu_handle h, int B, const GnWorkspace& ws, const double* q, int64_t ldq, int64_t lenq) {
  if (!q || B < 1) return false;
  const double* we = ws.W + (std::min<int64_t>(B, ws.wrows) - 1) * ws.ldw + ws_used(h, ws);
  const double* qe = q + (int64_t)(B - 1) * ldq + lenq;
  return ws.W < qe && q < we;
}

// ---- the resident loop's parameters and state (towr_alsolve_params_t / towr_alsolve_state_t) ---------------------------
int alsolve_params(towr_gpu_handle h, const towr_alsolve_params_t* p) {
  if (!p) return fail(h, TOWR_ERR_INVALID, "null params");
  auto in01 = [](double v) { return v > 0 && v < 1; };     // (a NaN fails every test below)
  auto in0c1 = [](double v) { return v > 0 && v <= 1; };
  if (p->mem < 1 || p->mem > TOWR_LBFGS_MAX_MEM) return fail(h, TOWR_ERR_INVALID, "params: mem outside 1..TOWR_LBFGS_MAX_MEM");
  if (p->max_inner < 1 || p->max_outer < 1) return fail(h, TOWR_ERR_INVALID, "params: max_inner and max_outer must be >= 1");
  if (!in01(p->c1) || !in01(p->shrink)) return fail(h, TOWR_ERR_INVALID, "params: c1 and shrink must lie in (0, 1)");
  if (!(p->alpha_min > 0) || !(p->alpha0 >= p->alpha_min)) return fail(h, TOWR_ERR_INVALID, "params: alpha0 >= alpha_min > 0 required");
  if (!(p->curv_eps >= 0)) return fail(h, TOWR_ERR_INVALID, "params: curv_eps is negative or NaN");
  if (!(p->rho0 > 0) || !(p->rho_grow >= 1) || !(p->rho_max >= p->rho0))
    return fail(h, TOWR_ERR_INVALID, "params: rho0 > 0, rho_grow >= 1 and rho_max >= rho0 required");
  if (!in0c1(p->eta0) || !in0c1(p->eta_shrink) || !(p->eta_star > 0))
    return fail(h, TOWR_ERR_INVALID, "params: eta0 and eta_shrink in (0, 1] and eta_star > 0 required");
  if (!in0c1(p->omega0) || !in0c1(p->omega_shrink) || !(p->omega_star > 0))
    return fail(h, TOWR_ERR_INVALID, "params: omega0 and omega_shrink in (0, 1] and omega_star > 0 required");
  return TOWR_OK;
}

// the stop rule's parameters (towr_alsolve_stop_t)
int alsolve_stop_params(towr_gpu_handle h, const towr_alsolve_stop_t* sp) {
  if (!sp) return fail(h, TOWR_ERR_INVALID, "null stop");
  if (!(sp->acc_eta >= 0) || !(sp->acc_omega >= 0) || !(sp->infeas_rho >= 0))   // (a NaN fails every test)
    return fail(h, TOWR_ERR_INVALID, "stop: acc_eta, acc_omega or infeas_rho is negative or NaN");
  if (sp->acc_iters < 0) return fail(h, TOWR_ERR_INVALID, "stop: acc_iters is negative");
  if (!(sp->infeas_keep > 0 && sp->infeas_keep <= 1)) return fail(h, TOWR_ERR_INVALID, "stop: infeas_keep outside (0, 1]");
  return TOWR_OK;
}

// the state fields an entry uses: kAlLs the line search's, kAlOuter the outer update's, kAlInit the initialisation's;
// kAlStop the stop rule's; the iteration uses every field
enum : unsigned { kAlLs = 1, kAlOuter = 2, kAlInit = 4, kAlAll = 8, kAlStop = 16 };
int alsolve_state(towr_gpu_handle h, const towr_alsolve_state_t* s, unsigned use) {
  if (!s) return fail(h, TOWR_ERR_INVALID, "null state");
  const Layout& L = h->L;
  const bool all = use & kAlAll, ls = all || (use & kAlLs), ou = all || (use & kAlOuter), in = all || (use & kAlInit);
  if (!s->ISTATE || !s->SCAL || !s->HMETA || !s->ALPHA) return fail(h, TOWR_ERR_INVALID, "state: null ISTATE, SCAL, HMETA or ALPHA");
  if (s->ldsc < 8) return fail(h, TOWR_ERR_INVALID, "state: ldsc smaller than 8");
  if ((ls || in) && (!s->X || !s->XC)) return fail(h, TOWR_ERR_INVALID, "state: null X or XC");
  if (ls && (!s->GR || !s->GRC)) return fail(h, TOWR_ERR_INVALID, "state: null GR or GRC");
  if ((in || all) && !s->D) return fail(h, TOWR_ERR_INVALID, "state: null D");
  if ((ls || in) && s->ldx < L.n) return fail(h, TOWR_ERR_INVALID, "state: ldx smaller than n");
  if ((ou || in || (use & kAlStop)) && !s->RHO) return fail(h, TOWR_ERR_INVALID, "state: null RHO");
  if (ou && (!s->LAM || !s->LAMP)) return fail(h, TOWR_ERR_INVALID, "state: null LAM or LAMP");
  if (ou && s->ldl < L.m) return fail(h, TOWR_ERR_INVALID, "state: ldl smaller than m");
  if (ls) {
    if (!s->HS || !s->HY) return fail(h, TOWR_ERR_INVALID, "state: null HS or HY");
    if (s->ldh < L.n) return fail(h, TOWR_ERR_INVALID, "state: ldh smaller than n");
    if (!s->FC || !s->RSUM || !s->USUM || !s->LSUM) return fail(h, TOWR_ERR_INVALID, "state: null FC, RSUM, USUM or LSUM");
    if (s->ldrs < 4 || s->ldus < 6 || s->ldls < 8) return fail(h, TOWR_ERR_INVALID, "state: ldrs < 4, ldus < 6 or ldls < 8");
  }
  if (all) {
    if (!s->SSUM || !s->DSUM) return fail(h, TOWR_ERR_INVALID, "state: null SSUM or DSUM");
    if (s->ldrs < 4 + (int64_t)L.cons.size()) return fail(h, TOWR_ERR_INVALID, "state: ldrs smaller than 4 + n_constraints");
    if (s->ldss < 5 + (int64_t)L.varsets.size()) return fail(h, TOWR_ERR_INVALID, "state: ldss smaller than 5 + n_varsets");
    if (s->ldds < 5) return fail(h, TOWR_ERR_INVALID, "state: ldds smaller than 5");
  }
  return TOWR_OK;
}

// ---- launchers: one block per problem; the caller's operands in `a`, the handle's tables and sizes added here ----------
// one product's operands: Y = J p (Vec = P, Out = Y) or Z (+)= J^T lam (Vec = LAM, Out = Z)
JpArgs product(const double* V, int64_t ldv, const double* vec, int64_t ldvec, double* out, int64_t ldo, int accumulate) {
  JpArgs a{V, ldv, vec, ldvec, out, ldo};
  a.accumulate = accumulate;
  return a;
}
int launch_product(towr_gpu_handle h, bool tvec, int B, const JpArgs& call, hipStream_t s) {
  JpArgs a = h->al.jp;   // the tables (products_ready)
  a.V = call.V; a.ldv = call.ldv; a.Vec = call.Vec; a.ldvec = call.ldvec; a.Out = call.Out; a.ldo = call.ldo;
  a.accumulate = call.accumulate;
  const size_t lds = tvec ? jp_tvec_lds(a.n, a.m) : jp_vec_lds(a.n, a.m);
  void* args[] = {&a};
  HIPCHK(h, launch_kernel(tvec ? jp_tvec_kernel() : jp_vec_kernel(), dim3((unsigned)B), dim3(kJpBlock), args, lds, s));
  return TOWR_OK;
}

// (GL NULL: the handle's bounds, one row; without LAMP only the violation summary: LAM and rho are not used)
int launch_residual(towr_gpu_handle h, int B, ResArgs a, hipStream_t s) {
  if (!a.GL) { a.GL = h->al.d_blo; a.GU = h->al.d_bup; a.ldb = 0; }
  if (!a.LAMP) { a.LAM = nullptr; a.rho = 1.0; a.RHO = nullptr; }
  a.set_row0 = h->al.d_set_row0; a.m = h->L.m; a.n_sets = (int32_t)h->L.cons.size();
  void* args[] = {&a};
  HIPCHK(h, launch_kernel(res_kernel(), dim3((unsigned)B), dim3(kResBlock), args, 0, s));
  return TOWR_OK;
}

// (XL NULL: the handle's bounds, one row)
int launch_step(towr_gpu_handle h, int B, StepArgs a, hipStream_t s) {
  if (!a.XL) { a.XL = h->al.d_xlo; a.XU = h->al.d_xup; a.ldb = 0; }
  a.set_col0 = h->al.d_set_col0; a.n = h->L.n; a.n_sets = (int32_t)h->L.varsets.size();
  void* args[] = {&a};
  HIPCHK(h, launch_kernel(step_kernel(), dim3((unsigned)B), dim3(kStepBlock), args, 0, s));
  return TOWR_OK;
}

int launch_lbfgs_update(towr_gpu_handle h, int B, LbfgsUpdateArgs a, hipStream_t s) {
  a.n = h->L.n;
  void* args[] = {&a};
  HIPCHK(h, launch_kernel(lbfgs_update_kernel(), dim3((unsigned)B), dim3(kLbfgsBlock), args, (size_t)lbfgs_update_lds(a.n), s));
  return TOWR_OK;
}

// (XL NULL: the handle's bounds, one row — with X, after step_ready)
int launch_lbfgs_direction(towr_gpu_handle h, int B, LbfgsDirArgs a, hipStream_t s) {
  if (!a.XL) { a.XL = h->al.d_xlo; a.XU = h->al.d_xup; a.ldb = 0; }
  a.n = h->L.n;
  void* args[] = {&a};
  HIPCHK(h, launch_kernel(lbfgs_direction_kernel(), dim3((unsigned)B), dim3(kLbfgsBlock), args, (size_t)lbfgs_direction_lds(a.n), s));
  return TOWR_OK;
}

// (XL NULL: the handle's bounds, one row — with X, after step_ready; after gn_ready; a.PC: the preconditioned kernel)
int launch_gn(towr_gpu_handle h, int B, GnArgs a, hipStream_t s) {
  if (a.X && !a.XL) { a.XL = h->al.d_xlo; a.XU = h->al.d_xup; a.ldb = 0; }
  a.jp = h->al.jp;   // the tables (products_ready)
  void* args[] = {&a};
  HIPCHK(h, launch_kernel(a.PC ? gn_direction_pc_kernel() : gn_direction_kernel(), dim3((unsigned)B), dim3(kGnBlock), args,
                          gn_direction_lds(a.jp.n, a.jp.m), s));
  return TOWR_OK;
}

// (XL NULL: the handle's bounds, one row — with X, after step_ready; after gn_direct_ready.) ceil(B / wrows) launches in
// sequence: problem b of launch l is block b - l wrows and owns workspace row b mod wrows.
int launch_gn_direct(towr_gpu_handle h, int B, GnDirectArgs a, int wrows, hipStream_t s) {
  towr_gpu_handle_s::AugLag& al = h->al;
  if (a.X && !a.XL) { a.XL = al.d_xlo; a.XU = al.d_xup; a.ldb = 0; }
  const int32_t* const* t = reinterpret_cast<const int32_t* const*>(al.d_gf);
  a.pos = t[0]; a.inv = t[1]; a.first = t[2]; a.last = t[3]; a.row_off = t[4]; a.csc_row = t[5]; a.csc_index = t[6];
  a.col_ptr = al.jp.col_ptr;
  a.n = h->L.n; a.m = h->L.m; a.env = (int32_t)al.gf_env; a.width = al.gf_width;
  const size_t lds = gn_direct_lds(a.n, a.m, a.width);
  const int step = std::min(wrows, B);
  for (int c0 = 0; c0 < B; c0 += step) {
    GnDirectArgs g = a;
    g.V = a.V + (int64_t)c0 * a.ldv; g.LAMP = a.LAMP + (int64_t)c0 * a.ldlp; g.RHO = row_at(a.RHO, c0, 1);
    g.X = row_at(a.X, c0, a.ldx); g.GR = a.GR + (int64_t)c0 * a.ldgr;
    g.XL = row_at(a.XL, c0, a.ldb); g.XU = row_at(a.XU, c0, a.ldb);
    g.RUN = row_at(a.RUN, c0, a.run_stride);
    g.D = a.D + (int64_t)c0 * a.ldd; g.SUM = a.SUM + (int64_t)c0 * a.lds;
    void* args[] = {&g};
    HIPCHK(h, launch_kernel(gn_direct_kernel(), dim3((unsigned)std::min(step, B - c0)), dim3(kGnBlock), args, lds, s));
  }
  return TOWR_OK;
}

// the tiled direction: launch_gn_direct's launches and rows (after gn_tiled_ready)
int launch_gn_tiled(towr_gpu_handle h, int B, GnTiledArgs a, int wrows, hipStream_t s) {
  towr_gpu_handle_s::AugLag& al = h->al;
  if (a.X && !a.XL) { a.XL = al.d_xlo; a.XU = al.d_xup; a.ldb = 0; }
  const int32_t* const* t = reinterpret_cast<const int32_t* const*>(al.d_gt);
  a.bfirst = t[0]; a.tile_off = t[1]; a.tcol_ptr = t[2]; a.tcol_rows = t[3];
  a.pos = t[4]; a.inv = t[5]; a.asm_ptr = t[6]; a.asm_terms = reinterpret_cast<const GnAsmTerm*>(al.d_gt[7]);
  a.n = h->L.n; a.m = h->L.m; a.nt = (int32_t)al.gt_bfirst.size(); a.tiles = (int32_t)al.gt_tiles;
  const size_t lds = gn_tiled_lds(a.n, a.m);
  const int step = std::min(wrows, B);
  for (int c0 = 0; c0 < B; c0 += step) {
    GnTiledArgs g = a;
    g.V = a.V + (int64_t)c0 * a.ldv; g.LAMP = a.LAMP + (int64_t)c0 * a.ldlp; g.RHO = row_at(a.RHO, c0, 1);
    g.X = row_at(a.X, c0, a.ldx); g.GR = a.GR + (int64_t)c0 * a.ldgr;
    g.XL = row_at(a.XL, c0, a.ldb); g.XU = row_at(a.XU, c0, a.ldb);
    g.RUN = row_at(a.RUN, c0, a.run_stride);
    g.D = a.D + (int64_t)c0 * a.ldd; g.SUM = a.SUM + (int64_t)c0 * a.lds;
    void* args[] = {&g};
    HIPCHK(h, launch_kernel(gn_tiled_kernel(), dim3((unsigned)std::min(step, B - c0)), dim3(kGnBlock), args, lds, s));
  }
  return TOWR_OK;
}

int launch_gn_select(towr_gpu_handle h, int B, const towr_alsolve_state_t& st, const double* DC, hipStream_t s) {
  GnSelectArgs a{st.ISTATE, DC, st.ldx, st.GR, st.ldx, st.D, st.ldx, h->L.n, 0};
  void* args[] = {&a};
  HIPCHK(h, launch_kernel(gn_select_kernel(), dim3((unsigned)B), dim3(kLbfgsBlock), args, 0, s));
  return TOWR_OK;
}

// (XL NULL: the handle's bounds, one row — after step_ready)
int launch_linesearch(towr_gpu_handle h, int B, const towr_alsolve_params_t& p, const towr_alsolve_state_t& st, const double* XL,
                      const double* XU, int64_t ldb, hipStream_t s) {
  LineSearchArgs a{st, XL, XU, ldb, p.c1, p.shrink, p.alpha0, p.alpha_min, p.curv_eps, h->L.n, p.mem};
  if (!a.XL) { a.XL = h->al.d_xlo; a.XU = h->al.d_xup; a.ldb = 0; }
  void* args[] = {&a};
  HIPCHK(h, launch_kernel(linesearch_kernel(), dim3((unsigned)B), dim3(kLbfgsBlock), args, (size_t)lbfgs_update_lds(a.n), s));
  return TOWR_OK;
}

int launch_outer(towr_gpu_handle h, int B, const towr_alsolve_params_t& p, const towr_alsolve_state_t& st, hipStream_t s) {
  OuterArgs a{st, p, h->L.m};
  void* args[] = {&a};
  HIPCHK(h, launch_kernel(alsolve_outer_kernel(), dim3((unsigned)B), dim3(kLbfgsBlock), args, 0, s));
  return TOWR_OK;
}

// the stop rule: one thread per problem
int launch_stop(towr_gpu_handle h, int B, const towr_alsolve_params_t& p, const towr_alsolve_stop_t& sp,
                const towr_alsolve_state_t& st, hipStream_t s) {
  StopArgs a{st.ISTATE, st.SCAL, st.ldsc, st.ALPHA, st.RHO, sp, p.max_inner, B};
  void* args[] = {&a};
  HIPCHK(h, launch_kernel(alsolve_stop_kernel(), dim3((unsigned)((B + kLbfgsBlock - 1) / kLbfgsBlock)), dim3(kLbfgsBlock), args, 0, s));
  return TOWR_OK;
}

// the verdict stage on rows [c0, c0 + B) of the whole batch's operands in `whole` (n: the handle's)
int launch_verdict(towr_gpu_handle h, int B, const VerdictArgs& whole, int c0, hipStream_t s) {
  VerdictArgs a = whole;
  a.X += (int64_t)c0 * a.ldx; a.GR += (int64_t)c0 * a.ldx; a.XC += (int64_t)c0 * a.ldx;
  a.FC += c0; a.SCAL += (int64_t)c0 * a.ldsc; a.ISTATE += 4 * (int64_t)c0; a.RSUM += (int64_t)c0 * a.ldrs;
  a.VERDICT += c0; a.NDIR = row_at(a.NDIR, c0, 1);
  a.n = h->L.n;
  void* args[] = {&a};
  HIPCHK(h, launch_kernel(alsolve_verdict_kernel(), dim3((unsigned)B), dim3(kLbfgsBlock), args, 0, s));
  return TOWR_OK;
}

// ---- fused calls ----------------------------------------------------------------------------------------------------
// the stream and terrains of a fused call
struct Batch {
  hipStream_t s;
  const towr_terrain_t* ter;
  int per;
  const towr_terrain_t* terrain_at(int c0) const { return per ? ter + c0 : ter; }
};

// What the fused entries share behind bind: the batch terrains, nothing to do for B = 0, the tables the call needs
// (`ready`), then body(batch) holding the handle's scratch on the caller's stream — acquired once the tables are ready,
// released on every path behind that (also after a failure: what was queued still orders the scratch); the first code
// that is not TOWR_OK is the answer. A call that needs no table uses none of this file's scratch: its body runs as it is.
using Ready = int (*)(towr_gpu_handle);
// `ter` (the solve driver): the per-problem terrains of this call's rows in the handle's place.
template <class Body>
int fused(towr_gpu_handle h, int B, void* stream, std::initializer_list<Ready> ready, Body body,
          const towr_terrain_t* ter = nullptr) {
  Batch b{reinterpret_cast<hipStream_t>(stream), ter, ter ? 1 : 0};
  if (!ter)
    if (int rc = batch_terrain(h, B, false, &b.ter, &b.per)) return rc;
  if (B == 0) return TOWR_OK;
  if (ready.size() == 0) return body(b);
  for (Ready r : ready)
    if (int rc = r(h)) return rc;
  if (int rc = scratch_acquire(h, b.s)) return rc;
  const int rc = body(b);
  const int rr = scratch_release(h, b.s);
  return rc ? rc : rr;
}

// The chunks of towr_gpu_eval_auglag_batch_device, shared by the two step entries (inside fused()): per chunk of
// problems the evaluation at e.X (values into d_pv, never d_v, so the kept Jacobian survives), the residual kernel on
// that g and the J^T product with lam+ into z.Out, back to back on the caller's stream. e.G / r.LAMP NULL: g / lam+
// stay in handle scratch (d_rg / d_rl). e, r and z hold the whole batch's operands (r.G, z.V and z.Vec are not used); a
// chunk launches with its rows of them. With gn (the resident GN loop): behind a chunk's product, while its values are
// still in d_pv, the GN direction at (e.X, z.Out) with that lam+ and rho into the chunk's rows of gn->D / gn->SUM (of gn
// the bounds, RUN, D, SUM and the CG parameters are used); with gd the direct direction in its place (of gd the bounds,
// RUN, D, SUM, the workspace and mu); with gt the tiled direct direction, as gd. With vd (the lazy GN loop; vd holds the
// whole batch's operands): behind a chunk's product the verdict stage on the chunk's rows, and the chunk's direction runs
// with RUN = those rows of vd->VERDICT, run_stride 1, in place of the caller's RUN.
struct EvalStage { const double* X; int64_t ldx; double* G; int64_t ldg; };
int auglag_chunks(towr_gpu_handle h, int B, const EvalStage& e, const ResArgs& r, const JpArgs& z, const Batch& b,
                  const GnArgs* gn = nullptr, const GnDirectArgs* gd = nullptr, int wrows = 0, const GnTiledArgs* gt = nullptr,
                  const VerdictArgs* vd = nullptr) {
  towr_gpu_handle_s::AugLag& al = h->al;
  const int64_t ldv = ld16(h->L.nnz), ldr = ld16(h->L.m);
  const int C = chunk_plan(h, B);
  int rc = scratch_grow(h, &al.d_pv, &al.pv_cap, C, ldv);
  if (rc == TOWR_OK && !e.G) rc = scratch_grow(h, &al.d_rg, &al.rg_cap, C, ldr);
  if (rc == TOWR_OK && !r.LAMP) rc = scratch_grow(h, &al.d_rl, &al.rl_cap, C, ldr);
  for (int c0 = 0; c0 < B && rc == TOWR_OK; c0 += C) {
    const int cb = std::min(C, B - c0);
    double* g = e.G ? e.G + (int64_t)c0 * e.ldg : al.d_rg;
    ResArgs a = r;
    a.G = g; a.ldg = e.G ? e.ldg : ldr;
    if (r.LAMP) a.LAMP = r.LAMP + (int64_t)c0 * r.ldlp; else { a.LAMP = al.d_rl; a.ldlp = ldr; }
    a.GL = row_at(r.GL, c0, r.ldb); a.GU = row_at(r.GU, c0, r.ldb); a.LAM = row_at(r.LAM, c0, r.ldl);
    a.SUM = r.SUM + (int64_t)c0 * r.lds;
    a.RHO = row_at(r.RHO, c0, 1);
    rc = launch(h, cb, e.X + (int64_t)c0 * e.ldx, e.ldx, g, a.ldg, al.d_pv, ldv, 1, 1, b.s, b.terrain_at(c0), b.per, -1);
    if (rc == TOWR_OK) rc = launch_residual(h, cb, a, b.s);
    if (rc == TOWR_OK)
      rc = launch_product(h, true, cb, product(al.d_pv, ldv, a.LAMP, a.ldlp, z.Out + (int64_t)c0 * z.ldo, z.ldo, z.accumulate), b.s);
    if (rc == TOWR_OK && vd) rc = launch_verdict(h, cb, *vd, c0, b.s);
    if (rc == TOWR_OK && gn) {
      GnArgs g = *gn;
      g.V = al.d_pv; g.ldv = ldv;
      g.LAMP = a.LAMP; g.ldlp = a.ldlp;
      g.RHO = a.RHO; g.rho = r.rho;
      g.X = e.X + (int64_t)c0 * e.ldx; g.ldx = e.ldx;
      g.GR = z.Out + (int64_t)c0 * z.ldo; g.ldgr = z.ldo;
      g.XL = row_at(gn->XL, c0, gn->ldb); g.XU = row_at(gn->XU, c0, gn->ldb);
      g.RUN = row_at(gn->RUN, c0, gn->run_stride);
      if (vd) { g.RUN = vd->VERDICT + c0; g.run_stride = 1; }
      g.D = gn->D + (int64_t)c0 * gn->ldd;
      g.SUM = gn->SUM + (int64_t)c0 * gn->lds;
      if (gn->PC) g.PC = gn->PC + (int64_t)c0 * gn->ldpc;
      rc = launch_gn(h, cb, g, b.s);
    }
    if (rc == TOWR_OK && gd) {   // (the direct direction: wrows applies within the chunk)
      GnDirectArgs g = *gd;
      g.V = al.d_pv; g.ldv = ldv;
      g.LAMP = a.LAMP; g.ldlp = a.ldlp;
      g.RHO = a.RHO; g.rho = r.rho;
      g.X = e.X + (int64_t)c0 * e.ldx; g.ldx = e.ldx;
      g.GR = z.Out + (int64_t)c0 * z.ldo; g.ldgr = z.ldo;
      g.XL = row_at(gd->XL, c0, gd->ldb); g.XU = row_at(gd->XU, c0, gd->ldb);
      g.RUN = row_at(gd->RUN, c0, gd->run_stride);
      if (vd) { g.RUN = vd->VERDICT + c0; g.run_stride = 1; }
      g.D = gd->D + (int64_t)c0 * gd->ldd;
      g.SUM = gd->SUM + (int64_t)c0 * gd->lds;
      rc = launch_gn_direct(h, cb, g, wrows, b.s);
    }
    if (rc == TOWR_OK && gt) {   // (the tiled direction, as gd)
      GnTiledArgs g = *gt;
      g.V = al.d_pv; g.ldv = ldv;
      g.LAMP = a.LAMP; g.ldlp = a.ldlp;
      g.RHO = a.RHO; g.rho = r.rho;
      g.X = e.X + (int64_t)c0 * e.ldx; g.ldx = e.ldx;
      g.GR = z.Out + (int64_t)c0 * z.ldo; g.ldgr = z.ldo;
      g.XL = row_at(gt->XL, c0, gt->ldb); g.XU = row_at(gt->XU, c0, gt->ldb);
      g.RUN = row_at(gt->RUN, c0, gt->run_stride);
      if (vd) { g.RUN = vd->VERDICT + c0; g.run_stride = 1; }
      g.D = gt->D + (int64_t)c0 * gt->ldd;
      g.SUM = gt->SUM + (int64_t)c0 * gt->lds;
      rc = launch_gn_tiled(h, cb, g, wrows, b.s);
    }
  }
  return rc;
}

// the probe stage's own arguments (towr_alsolve_probe_t and its summary)
int probe_args(towr_gpu_handle h, const towr_alsolve_probe_t* probe, const double* PSUM, int64_t ldps) {
  if (!probe) return fail(h, TOWR_ERR_INVALID, "null probe");
  if (probe->trials < 1 || probe->trials > TOWR_PROBE_MAX) return fail(h, TOWR_ERR_INVALID, "probe: trials outside 1..TOWR_PROBE_MAX");
  if (!PSUM) return fail(h, TOWR_ERR_INVALID, "probe: null PSUM");
  if (ldps < 8) return fail(h, TOWR_ERR_INVALID, "probe: ldps smaller than 8");
  return TOWR_OK;
}

// The probe stage on the caller's stream (inside fused(), after residual_ready and step_ready): T + 1 launches of the
// probe kernel and, between two of them, f (the f-only objective launch), g (the g-only evaluation) and the residual
// kernel at the candidates. The candidates, f, g, lam+ and the residual summaries of the whole batch live in handle
// scratch (d_sd, d_sf, d_rg, d_rl, d_pr); the iteration behind the stage reuses d_rg with its own rows.
int probe_stage(towr_gpu_handle h, int B, const towr_alsolve_params_t& p, int T, const towr_alsolve_state_t& st, const double* GL,
                const double* GU, int64_t ldgb, const double* XL, const double* XU, int64_t ldxb, double* PSUM, int64_t ldps,
                const Batch& b) {
  towr_gpu_handle_s::AugLag& al = h->al;
  const int64_t ldn = ld16(h->L.n), ldr = ld16(h->L.m), ldq = ld16(4 + (int64_t)h->L.cons.size());
  int rc = scratch_grow(h, &al.d_sd, &al.sd_cap, B, ldn);
  if (rc == TOWR_OK) rc = scratch_grow(h, &al.d_sf, &al.sf_cap, B, 1);
  if (rc == TOWR_OK) rc = scratch_grow(h, &al.d_rg, &al.rg_cap, B, ldr);
  if (rc == TOWR_OK) rc = scratch_grow(h, &al.d_rl, &al.rl_cap, B, ldr);
  if (rc == TOWR_OK) rc = scratch_grow(h, &al.d_pr, &al.pr_cap, B, ldq);
  if (rc != TOWR_OK) return rc;
  ProbeArgs a{st, XL, XU, ldxb, al.d_sd, ldn, al.d_sf, al.d_pr, ldq, PSUM, ldps, p.c1, p.shrink, p.alpha_min, h->L.n, 0, T, 0};
  if (!a.XL) { a.XL = al.d_xlo; a.XU = al.d_xup; a.ldb = 0; }
  ResArgs r{al.d_rg, ldr, GL, GU, ldgb, st.LAM, st.ldl, al.d_rl, ldr, al.d_pr, ldq};
  r.rho = 1.0;
  r.RHO = st.RHO;
  for (int t = 0; t <= T && rc == TOWR_OK; ++t) {
    a.t = t;
    void* args[] = {&a};
    HIPCHK(h, launch_kernel(alsolve_probe_kernel(), dim3((unsigned)B), dim3(kLbfgsBlock), args, 0, b.s));
    if (t == T) break;
    rc = launch_cost(h, B, al.d_sd, ldn, al.d_sf, nullptr, 0, b.s, b.ter, b.per);
    if (rc == TOWR_OK) rc = launch(h, B, al.d_sd, ldn, al.d_rg, ldr, nullptr, 0, 1, 0, b.s, b.ter, b.per, -1);
    if (rc == TOWR_OK) rc = launch_residual(h, B, r, b.s);
  }
  return rc;
}

}  // namespace

// =================================================================================================
// C-ABI
// =================================================================================================
extern "C" {

// ---- Jacobian products (jprod.hip) ----------------------------------------------------------------------------
int towr_gpu_jac_csc(towr_gpu_handle h, int64_t* col_ptr, int32_t* row, int32_t* csr_index) {
  if (!h || !col_ptr || !row || !csr_index) return fail(h, TOWR_ERR_INVALID, "null argument");
  const Layout& L = h->L;
  std::memcpy(col_ptr, L.col_ptr.data(), sizeof(int64_t) * L.col_ptr.size());
  if (L.nnz) {
    std::memcpy(row, L.csc_row.data(), sizeof(int32_t) * L.csc_row.size());
    std::memcpy(csr_index, L.csc_index.data(), sizeof(int32_t) * L.csc_index.size());
  }
  return TOWR_OK;
}

int towr_gpu_jac_vec_batch_device(towr_gpu_handle h, int32_t B, const double* V, int64_t ldv, const double* P, int64_t ldp,
                                  double* Y, int64_t ldy, void* stream) {
  if (!h || B < 0 || !V || !P || !Y) return fail(h, TOWR_ERR_INVALID, "bad argument (null pointer or B < 0)");
  const Layout& L = h->L;
  if (ldv < L.nnz || ldp < L.n || ldy < L.m) return fail(h, TOWR_ERR_INVALID, "leading dimension smaller than nnz (V) / n (P) / m (Y)");
  if (int rc = bind(h)) return rc;
  if (B == 0) return TOWR_OK;
  if (int rc = products_ready(h)) return rc;
  return launch_product(h, false, B, product(V, ldv, P, ldp, Y, ldy, 0), reinterpret_cast<hipStream_t>(stream));
}

int towr_gpu_jac_tvec_batch_device(towr_gpu_handle h, int32_t B, const double* V, int64_t ldv, const double* LAM, int64_t ldl,
                                   double* Z, int64_t ldz, int32_t accumulate, void* stream) {
  if (!h || B < 0 || !V || !LAM || !Z) return fail(h, TOWR_ERR_INVALID, "bad argument (null pointer or B < 0)");
  const Layout& L = h->L;
  if (ldv < L.nnz || ldl < L.m || ldz < L.n) return fail(h, TOWR_ERR_INVALID, "leading dimension smaller than nnz (V) / m (LAM) / n (Z)");
  if (int rc = bind(h)) return rc;
  if (B == 0) return TOWR_OK;
  if (int rc = products_ready(h)) return rc;
  return launch_product(h, true, B, product(V, ldv, LAM, ldl, Z, ldz, accumulate != 0), reinterpret_cast<hipStream_t>(stream));
}

int towr_gpu_set_products_chunk(towr_gpu_handle h, int32_t problems) {
  if (!h || problems < 0) return fail(h, TOWR_ERR_INVALID, "bad argument");
  h->al.products_chunk = problems;
  return TOWR_OK;
}

// The values of `chunk` problems at a time in the handle's own scratch (d_pv, ordered across streams like the other
// scratch: fused()), each chunk evaluated by the batch launch sequence and consumed by the product kernels behind it
// on the caller's stream. Without LAM and P there are no values to keep: the plain evaluation of g.
int towr_gpu_eval_products_batch_device(towr_gpu_handle h, int32_t B, const double* X, int64_t ldx, double* G, int64_t ldg,
                                        const double* LAM, int64_t ldl, double* Z, int64_t ldz, int32_t accumulate,
                                        const double* P, int64_t ldp, double* Y, int64_t ldy, void* stream) {
  if (!h || B < 0 || !X) return fail(h, TOWR_ERR_INVALID, "bad argument (null X or B < 0)");
  const Layout& L = h->L;
  if ((Z && !LAM) || (Y && !P)) return fail(h, TOWR_ERR_INVALID, "Z given without LAM, or Y without P");
  if ((LAM && !Z) || (P && !Y)) return fail(h, TOWR_ERR_INVALID, "LAM given without Z, or P without Y");
  if (ldx < L.n || (G && ldg < L.m) || (LAM && (ldl < L.m || ldz < L.n)) || (P && (ldp < L.n || ldy < L.m)))
    return fail(h, TOWR_ERR_INVALID, "leading dimension smaller than n (X, P, Z) / m (G, LAM, Y)");
  if (int rc = bind(h)) return rc;
  const bool want_v = LAM || P;
  auto none = std::initializer_list<Ready>{};
  return fused(h, B, stream, want_v ? std::initializer_list<Ready>{products_ready} : none, [&](const Batch& b) -> int {
    if (!want_v) return G ? launch(h, B, X, ldx, G, ldg, nullptr, 0, 1, 0, b.s, b.ter, b.per, -1) : TOWR_OK;
    towr_gpu_handle_s::AugLag& al = h->al;
    const int64_t ldv = ld16(L.nnz);
    const int C = chunk_plan(h, B);
    int rc = scratch_grow(h, &al.d_pv, &al.pv_cap, C, ldv);
    for (int c0 = 0; c0 < B && rc == TOWR_OK; c0 += C) {
      const int cb = std::min(C, B - c0);
      rc = launch(h, cb, X + (int64_t)c0 * ldx, ldx, row_at(G, c0, ldg), ldg, al.d_pv, ldv, G != nullptr, 1, b.s, b.terrain_at(c0),
                  b.per, -1);
      if (rc == TOWR_OK && LAM)
        rc = launch_product(h, true, cb, product(al.d_pv, ldv, LAM + (int64_t)c0 * ldl, ldl, Z + (int64_t)c0 * ldz, ldz, accumulate != 0),
                            b.s);
      if (rc == TOWR_OK && P)
        rc = launch_product(h, false, cb, product(al.d_pv, ldv, P + (int64_t)c0 * ldp, ldp, Y + (int64_t)c0 * ldy, ldy, 0), b.s);
    }
    return rc;
  });
}

// ---- residuals (resid.hip) ---------------------------------------------------------------------------------------
int towr_gpu_residual_batch_device(towr_gpu_handle h, int32_t B, const double* G, int64_t ldg, const double* GL, const double* GU,
                                   int64_t ldb, const double* LAM, int64_t ldl, double rho, double* LAMP, int64_t ldlp,
                                   double* SUM, int64_t lds, void* stream) {
  if (!h || B < 0 || !G) return fail(h, TOWR_ERR_INVALID, "bad argument (null G or B < 0)");
  if (ldg < h->L.m) return fail(h, TOWR_ERR_INVALID, "leading dimension of G smaller than m");
  ResArgs a{G, ldg, GL, GU, ldb, LAM, ldl, LAMP, ldlp, SUM, lds};
  a.rho = rho;
  if (int rc = residual_args(h, a, LAMP != nullptr)) return rc;
  if (int rc = bind(h)) return rc;
  if (B == 0) return TOWR_OK;
  if (int rc = residual_ready(h)) return rc;
  return launch_residual(h, B, a, reinterpret_cast<hipStream_t>(stream));
}

// As towr_gpu_eval_products_batch_device: a chunk of problems at a time through the handle's scratch (the values in
// d_pv; g and lam+ in d_rg / d_rl when the caller does not want them), the three launches of a chunk back to back on
// the caller's stream (auglag_chunks).
int towr_gpu_eval_auglag_batch_device(towr_gpu_handle h, int32_t B, const double* X, int64_t ldx, const double* GL, const double* GU,
                                      int64_t ldb, const double* LAM, int64_t ldl, double rho, double* G, int64_t ldg,
                                      double* LAMP, int64_t ldlp, double* SUM, int64_t lds, double* Z, int64_t ldz,
                                      int32_t accumulate, void* stream) {
  if (!h || B < 0 || !X || !Z) return fail(h, TOWR_ERR_INVALID, "bad argument (null X or Z, or B < 0)");
  const Layout& L = h->L;
  if (ldx < L.n || ldz < L.n || (G && ldg < L.m)) return fail(h, TOWR_ERR_INVALID, "leading dimension smaller than n (X, Z) / m (G)");
  ResArgs r{nullptr, 0, GL, GU, ldb, LAM, ldl, LAMP, ldlp, SUM, lds};   // (G: the evaluation's, auglag_chunks)
  r.rho = rho;
  if (int rc = residual_args(h, r, true)) return rc;
  if (int rc = bind(h)) return rc;
  return fused(h, B, stream, {products_ready, residual_ready}, [&](const Batch& b) {
    return auglag_chunks(h, B, EvalStage{X, ldx, G, ldg}, r, product(nullptr, 0, nullptr, 0, Z, ldz, accumulate != 0), b);
  });
}

// ---- steps (step.hip) ----------------------------------------------------------------------------------------------
int towr_gpu_step_batch_device(towr_gpu_handle h, int32_t B, const double* X, int64_t ldx, const double* D, int64_t ldd,
                               const double* ALPHA, double alpha, const double* XL, const double* XU, int64_t ldb,
                               double* XP, int64_t ldxp, double* SUM, int64_t lds, void* stream) {
  if (!h || B < 0 || !X || !D) return fail(h, TOWR_ERR_INVALID, "bad argument (null X or D, or B < 0)");
  if (ldx < h->L.n || ldd < h->L.n) return fail(h, TOWR_ERR_INVALID, "leading dimension of X or D smaller than n");
  const StepArgs a{X, ldx, D, ldd, ALPHA, alpha, XL, XU, ldb, XP, ldxp, SUM, lds};
  if (int rc = step_args(h, a)) return rc;
  if (int rc = bind(h)) return rc;
  if (B == 0) return TOWR_OK;
  if (int rc = step_ready(h)) return rc;
  return launch_step(h, B, a, reinterpret_cast<hipStream_t>(stream));
}

// The gradient of the whole batch in handle scratch (d_sd: grad f from the cost launch, then + J^T lam+ per chunk of
// the auglag sequence), the step kernel behind it: what the three public calls launch, on the caller's stream.
int towr_gpu_auglag_step_batch_device(towr_gpu_handle h, int32_t B, const double* X, int64_t ldx, const double* GL, const double* GU,
                                      int64_t ldgb, const double* LAM, int64_t ldl, double rho, const double* ALPHA, double alpha,
                                      const double* XL, const double* XU, int64_t ldxb, double* F, double* G, int64_t ldg,
                                      double* LAMP, int64_t ldlp, double* RSUM, int64_t ldrs, double* XP, int64_t ldxp,
                                      double* SSUM, int64_t ldss, void* stream) {
  if (!h || B < 0 || !X || !XP) return fail(h, TOWR_ERR_INVALID, "bad argument (null X or XP, or B < 0)");
  const Layout& L = h->L;
  if (ldx < L.n || (G && ldg < L.m)) return fail(h, TOWR_ERR_INVALID, "leading dimension smaller than n (X) / m (G)");
  ResArgs r{nullptr, 0, GL, GU, ldgb, LAM, ldl, LAMP, ldlp, RSUM, ldrs};
  r.rho = rho;
  if (int rc = residual_args(h, r, true)) return rc;
  StepArgs st{X, ldx, nullptr, 0, ALPHA, alpha, XL, XU, ldxb, XP, ldxp, SSUM, ldss};   // (D: handle scratch, set below)
  if (int rc = step_args(h, st)) return rc;
  if (int rc = bind(h)) return rc;
  return fused(h, B, stream, {products_ready, residual_ready, step_ready}, [&](const Batch& b) {
    towr_gpu_handle_s::AugLag& al = h->al;
    const int64_t ldn = ld16(L.n);
    int rc = scratch_grow(h, &al.d_sd, &al.sd_cap, B, ldn);
    if (rc == TOWR_OK && !F) rc = scratch_grow(h, &al.d_sf, &al.sf_cap, B, 1);
    if (rc == TOWR_OK) rc = launch_cost(h, B, X, ldx, F ? F : al.d_sf, al.d_sd, ldn, b.s, b.ter, b.per);
    if (rc == TOWR_OK) rc = auglag_chunks(h, B, EvalStage{X, ldx, G, ldg}, r, product(nullptr, 0, nullptr, 0, al.d_sd, ldn, 1), b);
    st.D = al.d_sd; st.ldd = ldn;
    if (rc == TOWR_OK) rc = launch_step(h, B, st, b.s);
    return rc;
  });
}

// ---- L-BFGS (lbfgs.hip) --------------------------------------------------------------------------------------------
int towr_gpu_lbfgs_update_batch_device(towr_gpu_handle h, int32_t B, int32_t mem, const double* X, int64_t ldx, const double* XN,
                                       int64_t ldxn, const double* GR, int64_t ldgr, const double* GRN, int64_t ldgrn,
                                       double curv_eps, double* HS, double* HY, int64_t ldh, int32_t* HMETA, double* SUM,
                                       int64_t lds, void* stream) {
  if (!h || B < 0 || !X || !XN || !GR || !GRN) return fail(h, TOWR_ERR_INVALID, "bad argument (null X, XN, GR or GRN, or B < 0)");
  const int n = h->L.n;
  if (ldx < n || ldxn < n || ldgr < n || ldgrn < n) return fail(h, TOWR_ERR_INVALID, "leading dimension of X, XN, GR or GRN smaller than n");
  const LbfgsUpdateArgs a{X, ldx, XN, ldxn, GR, ldgr, GRN, ldgrn, HS, HY, ldh, HMETA, SUM, lds, curv_eps, 0, mem};
  if (int rc = lbfgs_args(h, a, 6)) return rc;
  if (!(curv_eps >= 0)) return fail(h, TOWR_ERR_INVALID, "curv_eps is negative or NaN");
  if (int rc = bind(h)) return rc;
  if (int rc = lbfgs_fits(h)) return rc;
  if (B == 0) return TOWR_OK;
  return launch_lbfgs_update(h, B, a, reinterpret_cast<hipStream_t>(stream));
}

int towr_gpu_lbfgs_direction_batch_device(towr_gpu_handle h, int32_t B, int32_t mem, const double* X, int64_t ldx, const double* GR,
                                          int64_t ldgr, const double* XL, const double* XU, int64_t ldb, const double* HS,
                                          const double* HY, int64_t ldh, const int32_t* HMETA, double* D, int64_t ldd, double* SUM,
                                          int64_t lds, void* stream) {
  if (!h || B < 0 || !GR || !D) return fail(h, TOWR_ERR_INVALID, "bad argument (null GR or D, or B < 0)");
  const int n = h->L.n;
  if ((X && ldx < n) || ldgr < n || ldd < n) return fail(h, TOWR_ERR_INVALID, "leading dimension of X, GR or D smaller than n");
  const LbfgsDirArgs a{X, ldx, GR, ldgr, XL, XU, ldb, HS, HY, ldh, HMETA, D, ldd, SUM, lds, 0, mem};
  if (int rc = lbfgs_args(h, a, 5)) return rc;
  if (int rc = box_args(h, XL, XU, ldb, n, "XL / XU", "n")) return rc;
  if (int rc = bind(h)) return rc;
  if (int rc = lbfgs_fits(h)) return rc;
  if (B == 0) return TOWR_OK;
  if (X && !XL)
    if (int rc = step_ready(h)) return rc;
  return launch_lbfgs_direction(h, B, a, reinterpret_cast<hipStream_t>(stream));
}

// The gradient of the augmented Lagrangian in the caller's GR (grad f from the cost launch, then + J^T lam+ per chunk of
// the auglag sequence; g and lam+ in handle scratch), the history update with (XPREV -> X, GRPREV -> GR), the
// direction in handle scratch (d_sd) and the step kernel behind it: what the five public calls launch, on the
// caller's stream.
int towr_gpu_auglag_lbfgs_step_batch_device(towr_gpu_handle h, int32_t B, int32_t mem, const double* X, int64_t ldx,
                                            const double* XPREV, int64_t ldxprev, const double* GRPREV, int64_t ldgrprev,
                                            const double* GL, const double* GU, int64_t ldgb, const double* LAM, int64_t ldl,
                                            double rho, const double* ALPHA, double alpha, const double* XL, const double* XU,
                                            int64_t ldxb, double curv_eps, double* HS, double* HY, int64_t ldh, int32_t* HMETA,
                                            double* F, double* GR, int64_t ldgr, double* RSUM, int64_t ldrs, double* USUM,
                                            int64_t ldus, double* DSUM, int64_t ldds, double* XP, int64_t ldxp, double* SSUM,
                                            int64_t ldss, void* stream) {
  if (!h || B < 0 || !X || !XP || !GR) return fail(h, TOWR_ERR_INVALID, "bad argument (null X, XP or GR, or B < 0)");
  const Layout& L = h->L;
  if (ldx < L.n || ldgr < L.n) return fail(h, TOWR_ERR_INVALID, "leading dimension of X or GR smaller than n");
  if ((XPREV == nullptr) != (GRPREV == nullptr)) return fail(h, TOWR_ERR_INVALID, "only one of XPREV / GRPREV given");
  if (XPREV && (ldxprev < L.n || ldgrprev < L.n)) return fail(h, TOWR_ERR_INVALID, "leading dimension of XPREV or GRPREV smaller than n");
  ResArgs r{nullptr, 0, GL, GU, ldgb, LAM, ldl, nullptr, 0, RSUM, ldrs};   // (g and lam+ stay in handle scratch)
  r.rho = rho;
  if (int rc = residual_args(h, r, true)) return rc;
  // the pair (X - XPREV, GR - GRPREV)
  const LbfgsUpdateArgs up{XPREV, ldxprev, X, ldx, GRPREV, ldgrprev, GR, ldgr, HS, HY, ldh, HMETA, USUM, ldus, curv_eps, 0, mem};
  if (XPREV)
    if (int rc = lbfgs_args(h, up, 6)) return rc;
  if (!(curv_eps >= 0)) return fail(h, TOWR_ERR_INVALID, "curv_eps is negative or NaN");   // (also without XPREV)
  LbfgsDirArgs dir{X, ldx, GR, ldgr, XL, XU, ldxb, HS, HY, ldh, HMETA, nullptr, 0, DSUM, ldds, 0, mem};   // (D: as st.D)
  if (int rc = lbfgs_args(h, dir, 5)) return rc;
  StepArgs st{X, ldx, nullptr, 0, ALPHA, alpha, XL, XU, ldxb, XP, ldxp, SSUM, ldss};   // (D: handle scratch, set below)
  if (int rc = step_args(h, st)) return rc;
  if (int rc = bind(h)) return rc;
  if (int rc = lbfgs_fits(h)) return rc;
  return fused(h, B, stream, {products_ready, residual_ready, step_ready}, [&](const Batch& b) {
    towr_gpu_handle_s::AugLag& al = h->al;
    const int64_t ldn = ld16(L.n);
    int rc = scratch_grow(h, &al.d_sd, &al.sd_cap, B, ldn);
    if (rc == TOWR_OK && !F) rc = scratch_grow(h, &al.d_sf, &al.sf_cap, B, 1);
    if (rc == TOWR_OK) rc = launch_cost(h, B, X, ldx, F ? F : al.d_sf, GR, ldgr, b.s, b.ter, b.per);
    if (rc == TOWR_OK) rc = auglag_chunks(h, B, EvalStage{X, ldx, nullptr, 0}, r, product(nullptr, 0, nullptr, 0, GR, ldgr, 1), b);
    if (rc == TOWR_OK && XPREV) rc = launch_lbfgs_update(h, B, up, b.s);
    dir.D = al.d_sd; dir.ldd = ldn;
    if (rc == TOWR_OK) rc = launch_lbfgs_direction(h, B, dir, b.s);
    st.D = al.d_sd; st.ldd = ldn;
    if (rc == TOWR_OK) rc = launch_step(h, B, st, b.s);
    return rc;
  });
}

// ---- the resident loop (lbfgs.hip: the line search, the outer update, the initialisation) ---------------------------
int towr_gpu_linesearch_batch_device(towr_gpu_handle h, int32_t B, const towr_alsolve_params_t* params,
                                     const towr_alsolve_state_t* state, const double* XL, const double* XU, int64_t ldxb,
                                     void* stream) {
  if (!h || B < 0) return fail(h, TOWR_ERR_INVALID, "bad argument (B < 0)");
  if (int rc = alsolve_params(h, params)) return rc;
  if (int rc = alsolve_state(h, state, kAlLs)) return rc;
  if (int rc = box_args(h, XL, XU, ldxb, h->L.n, "XL / XU", "n")) return rc;
  if (int rc = bind(h)) return rc;
  if (int rc = lbfgs_fits(h)) return rc;
  if (B == 0) return TOWR_OK;
  if (!XL)
    if (int rc = step_ready(h)) return rc;
  return launch_linesearch(h, B, *params, *state, XL, XU, ldxb, reinterpret_cast<hipStream_t>(stream));
}

int towr_gpu_auglag_outer_batch_device(towr_gpu_handle h, int32_t B, const towr_alsolve_params_t* params,
                                       const towr_alsolve_state_t* state, void* stream) {
  if (!h || B < 0) return fail(h, TOWR_ERR_INVALID, "bad argument (B < 0)");
  if (int rc = alsolve_params(h, params)) return rc;
  if (int rc = alsolve_state(h, state, kAlOuter)) return rc;
  if (int rc = bind(h)) return rc;
  if (B == 0) return TOWR_OK;
  return launch_outer(h, B, *params, *state, reinterpret_cast<hipStream_t>(stream));
}

int towr_gpu_alsolve_stop_batch_device(towr_gpu_handle h, int32_t B, const towr_alsolve_params_t* params,
                                       const towr_alsolve_stop_t* stop, const towr_alsolve_state_t* state, void* stream) {
  if (!h || B < 0) return fail(h, TOWR_ERR_INVALID, "bad argument (B < 0)");
  if (int rc = alsolve_params(h, params)) return rc;
  if (int rc = alsolve_stop_params(h, stop)) return rc;
  if (int rc = alsolve_state(h, state, kAlStop)) return rc;
  if (int rc = bind(h)) return rc;
  if (B == 0) return TOWR_OK;
  return launch_stop(h, B, *params, *stop, *state, reinterpret_cast<hipStream_t>(stream));
}

// what the iteration refuses (the initialisation answers the same arguments, so a loop fails at its first call)
static int alsolve_args(towr_gpu_handle h, int32_t B, const towr_alsolve_params_t* params, const towr_alsolve_state_t* state,
                        const double* GL, const double* GU, int64_t ldgb, const double* XL, const double* XU, int64_t ldxb) {
  if (!h || B < 0) return fail(h, TOWR_ERR_INVALID, "bad argument (B < 0)");
  if (int rc = alsolve_params(h, params)) return rc;
  if (int rc = alsolve_state(h, state, kAlAll)) return rc;
  if (int rc = box_args(h, GL, GU, ldgb, h->L.m, "GL / GU", "m")) return rc;
  if (!GL && !h->L.bounds_err.empty()) return fail(h, TOWR_ERR_INVALID, h->L.bounds_err);
  return box_args(h, XL, XU, ldxb, h->L.n, "XL / XU", "n");
}

// the initialisation's launch on the B rows of `st` (behind its checks and bind; the queued solve runs it per admission)
static int launch_alsolve_init(towr_gpu_handle h, int B, const towr_alsolve_params_t& p, const towr_alsolve_state_t& st,
                               const double* XL, const double* XU, int64_t ldxb, hipStream_t s) {
  if (B == 0) return TOWR_OK;
  if (!XL)
    if (int rc = step_ready(h)) return rc;
  AlInitArgs a{st, XL, XU, ldxb, p.rho0, p.eta0, p.omega0, h->L.n};
  if (!a.XL) { a.XL = h->al.d_xlo; a.XU = h->al.d_xup; a.ldb = 0; }
  void* args[] = {&a};
  HIPCHK(h, launch_kernel(alsolve_init_kernel(), dim3((unsigned)B), dim3(kLbfgsBlock), args, 0, s));
  return TOWR_OK;
}

int towr_gpu_alsolve_init_batch_device(towr_gpu_handle h, int32_t B, const towr_alsolve_params_t* params,
                                       const towr_alsolve_state_t* state, const double* XL, const double* XU, int64_t ldxb,
                                       void* stream) {
  if (int rc = alsolve_args(h, B, params, state, nullptr, nullptr, 0, XL, XU, ldxb)) return rc;
  if (int rc = bind(h)) return rc;
  if (int rc = lbfgs_fits(h)) return rc;
  return launch_alsolve_init(h, B, *params, *state, XL, XU, ldxb, reinterpret_cast<hipStream_t>(stream));
}

// Per iteration what the six public calls launch, on the caller's stream: the cost launch at XC (FC, GRC), the auglag
// chunks with the per-problem RHO accumulated onto GRC (g in handle scratch), the line search, the outer update, the
// direction of the problems whose flag bit 1 is set (RUN = the flags) and the step.
// (ter: fused()'s, the solve driver's permuted terrains; stop: the stop rule between the line search and the outer update;
// probe: the probe stage in front of every iteration, PSUM / ldps its summary)
static int alsolve_lbfgs_iterate(towr_gpu_handle h, int32_t B, int32_t iters, const towr_alsolve_params_t* params,
                                 const towr_alsolve_state_t* state, const double* GL, const double* GU, int64_t ldgb,
                                 const double* XL, const double* XU, int64_t ldxb, void* stream,
                                 const towr_terrain_t* ter = nullptr, const towr_alsolve_stop_t* stop = nullptr,
                                 const towr_alsolve_probe_t* probe = nullptr, double* PSUM = nullptr, int64_t ldps = 0) {
  if (int rc = alsolve_args(h, B, params, state, GL, GU, ldgb, XL, XU, ldxb)) return rc;
  if (stop)
    if (int rc = alsolve_stop_params(h, stop)) return rc;
  if (probe)
    if (int rc = probe_args(h, probe, PSUM, ldps)) return rc;
  if (iters < 0) return fail(h, TOWR_ERR_INVALID, "iters is negative");
  const towr_alsolve_state_t& st = *state;
  ResArgs r{nullptr, 0, GL, GU, ldgb, st.LAM, st.ldl, st.LAMP, st.ldl, st.RSUM, st.ldrs};
  r.rho = 1.0;
  r.RHO = st.RHO;
  LbfgsDirArgs dir{st.X, st.ldx, st.GR, st.ldx, XL, XU, ldxb, st.HS, st.HY, st.ldh, st.HMETA, st.D, st.ldx, st.DSUM, st.ldds, 0,
                   params->mem};
  dir.RUN = st.ISTATE + 1;
  dir.run_stride = 4;
  const StepArgs step{st.X, st.ldx, st.D, st.ldx, st.ALPHA, 0.0, XL, XU, ldxb, st.XC, st.ldx, st.SSUM, st.ldss};
  if (int rc = bind(h)) return rc;
  if (int rc = lbfgs_fits(h)) return rc;
  if (iters == 0) return TOWR_OK;
  return fused(h, B, stream, {products_ready, residual_ready, step_ready}, [&](const Batch& b) {
    int rc = TOWR_OK;
    for (int it = 0; it < iters && rc == TOWR_OK; ++it) {
      if (probe) rc = probe_stage(h, B, *params, probe->trials, st, GL, GU, ldgb, XL, XU, ldxb, PSUM, ldps, b);
      if (rc == TOWR_OK) rc = launch_cost(h, B, st.XC, st.ldx, st.FC, st.GRC, st.ldx, b.s, b.ter, b.per);
      if (rc == TOWR_OK)
        rc = auglag_chunks(h, B, EvalStage{st.XC, st.ldx, nullptr, 0}, r, product(nullptr, 0, nullptr, 0, st.GRC, st.ldx, 1), b);
      if (rc == TOWR_OK) rc = launch_linesearch(h, B, *params, st, XL, XU, ldxb, b.s);
      if (rc == TOWR_OK && stop) rc = launch_stop(h, B, *params, *stop, st, b.s);
      if (rc == TOWR_OK) rc = launch_outer(h, B, *params, st, b.s);
      if (rc == TOWR_OK) rc = launch_lbfgs_direction(h, B, dir, b.s);
      if (rc == TOWR_OK) rc = launch_step(h, B, step, b.s);
    }
    return rc;
  }, ter);
}

int towr_gpu_alsolve_probe_batch_device(towr_gpu_handle h, int32_t B, const towr_alsolve_params_t* params,
                                        const towr_alsolve_probe_t* probe, const towr_alsolve_state_t* state, const double* GL,
                                        const double* GU, int64_t ldgb, const double* XL, const double* XU, int64_t ldxb,
                                        double* PSUM, int64_t ldps, void* stream) {
  if (int rc = alsolve_args(h, B, params, state, GL, GU, ldgb, XL, XU, ldxb)) return rc;
  if (int rc = probe_args(h, probe, PSUM, ldps)) return rc;
  if (int rc = bind(h)) return rc;
  if (int rc = lbfgs_fits(h)) return rc;
  return fused(h, B, stream, {residual_ready, step_ready}, [&](const Batch& b) {
    return probe_stage(h, B, *params, probe->trials, *state, GL, GU, ldgb, XL, XU, ldxb, PSUM, ldps, b);
  });
}

int towr_gpu_alsolve_iterate_batch_device(towr_gpu_handle h, int32_t B, int32_t iters, const towr_alsolve_params_t* params,
                                          const towr_alsolve_state_t* state, const double* GL, const double* GU, int64_t ldgb,
                                          const double* XL, const double* XU, int64_t ldxb, void* stream) {
  return alsolve_lbfgs_iterate(h, B, iters, params, state, GL, GU, ldgb, XL, XU, ldxb, stream);
}

// ---- the Gauss-Newton direction (jprod.hip) and the resident loop that uses it ------------------------------------------
// both direction entries; PC NULL: the plain recursion (pc: the preconditioned entry's checks run)
static int gn_direction(towr_gpu_handle h, int32_t B, const towr_gn_params_t* gn, const double* V, int64_t ldv,
                        const double* LAMP, int64_t ldlp, const double* RHO, double rho, const double* X, int64_t ldx,
                        const double* GR, int64_t ldgr, const double* XL, const double* XU, int64_t ldb, const int32_t* RUN,
                        int32_t run_stride, double* D, int64_t ldd, double* SUM, int64_t lds, bool pc, int32_t precond, double* PC,
                        int64_t ldpc, void* stream) {
  if (!h || B < 0 || !V || !LAMP || !GR) return fail(h, TOWR_ERR_INVALID, "bad argument (null V, LAMP or GR, or B < 0)");
  if (int rc = gn_params(h, gn, D, SUM, lds)) return rc;
  const Layout& L = h->L;
  if (pc) {
    if (int rc = gn_pc_params(h, precond, PC, ldpc, lds)) return rc;
    if (precond != TOWR_GN_PC_JACOBI) PC = nullptr;
    if (rows_overlap(B, PC, ldpc, L.n, D, ldd, L.n) || rows_overlap(B, PC, ldpc, L.n, GR, ldgr, L.n) ||
        rows_overlap(B, PC, ldpc, L.n, X, ldx, L.n) || rows_overlap(B, PC, ldpc, L.n, V, ldv, L.nnz) ||
        rows_overlap(B, PC, ldpc, L.n, LAMP, ldlp, L.m))
      return fail(h, TOWR_ERR_INVALID, "gn: PC overlaps V, LAMP, X, GR or D");
  }
  if (!RHO && !(rho > 0)) return fail(h, TOWR_ERR_INVALID, "rho must be > 0 without RHO");
  if (ldv < L.nnz || ldlp < L.m || (X && ldx < L.n) || ldgr < L.n || ldd < L.n)
    return fail(h, TOWR_ERR_INVALID, "leading dimension smaller than nnz (V) / m (LAMP) / n (X, GR, D)");
  if (int rc = box_args(h, XL, XU, ldb, L.n, "XL / XU", "n")) return rc;
  if (int rc = bind(h)) return rc;
  if (int rc = gn_fits(h)) return rc;
  if (B == 0) return TOWR_OK;
  if (int rc = gn_ready(h)) return rc;
  if (X && !XL)
    if (int rc = step_ready(h)) return rc;
  GnArgs a{V, ldv, LAMP, ldlp, RHO, rho, X, ldx, GR, ldgr, XL, XU, ldb, RUN, run_stride, D, ldd, SUM, lds, gn->mu, gn->tol, gn->ncg, 0};
  a.PC = PC; a.ldpc = ldpc;
  return launch_gn(h, B, a, reinterpret_cast<hipStream_t>(stream));
}

int towr_gpu_gn_direction_batch_device(towr_gpu_handle h, int32_t B, const towr_gn_params_t* gn, const double* V, int64_t ldv,
                                       const double* LAMP, int64_t ldlp, const double* RHO, double rho, const double* X,
                                       int64_t ldx, const double* GR, int64_t ldgr, const double* XL, const double* XU,
                                       int64_t ldb, const int32_t* RUN, int32_t run_stride, double* D, int64_t ldd, double* SUM,
                                       int64_t lds, void* stream) {
  return gn_direction(h, B, gn, V, ldv, LAMP, ldlp, RHO, rho, X, ldx, GR, ldgr, XL, XU, ldb, RUN, run_stride, D, ldd, SUM, lds,
                      false, TOWR_GN_PC_NONE, nullptr, 0, stream);
}

int towr_gpu_gn_direction_pc_batch_device(towr_gpu_handle h, int32_t B, const towr_gn_params_t* gn, int32_t precond,
                                          const double* V, int64_t ldv, const double* LAMP, int64_t ldlp, const double* RHO,
                                          double rho, const double* X, int64_t ldx, const double* GR, int64_t ldgr,
                                          const double* XL, const double* XU, int64_t ldb, const int32_t* RUN, int32_t run_stride,
                                          double* D, int64_t ldd, double* SUM, int64_t lds, double* PC, int64_t ldpc,
                                          void* stream) {
  return gn_direction(h, B, gn, V, ldv, LAMP, ldlp, RHO, rho, X, ldx, GR, ldgr, XL, XU, ldb, RUN, run_stride, D, ldd, SUM, lds,
                      true, precond, PC, ldpc, stream);
}

// Per iteration what the public calls launch, on the caller's stream: the cost launch at XC (FC, GRC), the auglag chunks
// with the per-problem RHO accumulated onto GRC and, per chunk, the GN direction at (XC, GRC) into DC on the values still
// in handle scratch (RUN = the phases: frozen problems are skipped), the line search, the outer update, the select
// (D <- DC or GR by the flags) and the step. (stop, probe: as above; lazy: the verdict stage in every chunk, whose words
// are the direction's RUN)
static int alsolve_gn_iterate(towr_gpu_handle h, int32_t B, int32_t iters, const towr_alsolve_params_t* params,
                              const towr_alsolve_state_t* state, const towr_gn_params_t* gn, double* DC, double* GSUM,
                              int64_t ldgs, bool pc, int32_t precond, double* PC, const double* GL, const double* GU, int64_t ldgb,
                              const double* XL, const double* XU, int64_t ldxb, void* stream, const GnWorkspace* ws = nullptr,
                              const towr_terrain_t* ter = nullptr,   // (ter: fused()'s)
                              const towr_alsolve_stop_t* stop = nullptr,
                              const towr_alsolve_probe_t* probe = nullptr, double* PSUM = nullptr, int64_t ldps = 0,
                              const towr_alsolve_lazy_t* lazy = nullptr) {
  if (int rc = alsolve_args(h, B, params, state, GL, GU, ldgb, XL, XU, ldxb)) return rc;
  if (stop)
    if (int rc = alsolve_stop_params(h, stop)) return rc;
  if (probe)
    if (int rc = probe_args(h, probe, PSUM, ldps)) return rc;
  if (lazy && !lazy->VERDICT) return fail(h, TOWR_ERR_INVALID, "lazy: null VERDICT");
  if (iters < 0) return fail(h, TOWR_ERR_INVALID, "iters is negative");
  if (int rc = ws ? gn_direct_params(h, gn, DC, GSUM, ldgs, *ws) : gn_params(h, gn, DC, GSUM, ldgs)) return rc;
  const towr_alsolve_state_t& st = *state;
  if (ws) {
    const int64_t n = h->L.n;
    if (ws_overlap(h, B, *ws, DC, st.ldx, n) || ws_overlap(h, B, *ws, st.XC, st.ldx, n) || ws_overlap(h, B, *ws, st.GRC, st.ldx, n) ||
        ws_overlap(h, B, *ws, st.LAMP, st.ldl, h->L.m) || ws_overlap(h, B, *ws, GSUM, ldgs, 8))
      return fail(h, TOWR_ERR_INVALID, "gn: W overlaps LAMP, XC, GRC, DC or GSUM");
  }
  if (pc) {
    if (int rc = gn_pc_params(h, precond, PC, st.ldx, ldgs)) return rc;
    if (precond != TOWR_GN_PC_JACOBI) PC = nullptr;
    const int64_t n = h->L.n;
    if (rows_overlap(B, PC, st.ldx, n, DC, st.ldx, n) || rows_overlap(B, PC, st.ldx, n, st.XC, st.ldx, n) ||
        rows_overlap(B, PC, st.ldx, n, st.GRC, st.ldx, n) || rows_overlap(B, PC, st.ldx, n, st.LAMP, st.ldl, h->L.m))
      return fail(h, TOWR_ERR_INVALID, "gn: PC overlaps LAMP, XC, GRC or DC");
  }
  ResArgs r{nullptr, 0, GL, GU, ldgb, st.LAM, st.ldl, st.LAMP, st.ldl, st.RSUM, st.ldrs};
  r.rho = 1.0;
  r.RHO = st.RHO;
  GnArgs g{};   // (V, LAMP, RHO, X and GR: the chunk's, auglag_chunks)
  g.XL = XL; g.XU = XU; g.ldb = ldxb;
  g.RUN = st.ISTATE; g.run_stride = 4;
  g.D = DC; g.ldd = st.ldx; g.SUM = GSUM; g.lds = ldgs;
  g.PC = PC; g.ldpc = st.ldx;
  g.mu = gn->mu; g.tol = gn->tol; g.ncg = gn->ncg;
  GnDirectArgs gd{};   // (as g, for the direct direction)
  gd.XL = XL; gd.XU = XU; gd.ldb = ldxb;
  gd.RUN = st.ISTATE; gd.run_stride = 4;
  gd.D = DC; gd.ldd = st.ldx; gd.SUM = GSUM; gd.lds = ldgs;
  gd.mu = gn->mu;
  if (ws) { gd.W = ws->W; gd.ldw = ws->ldw; }
  GnTiledArgs gt{};   // (as gd, for the tiled direction)
  gt.XL = XL; gt.XU = XU; gt.ldb = ldxb;
  gt.RUN = st.ISTATE; gt.run_stride = 4;
  gt.D = DC; gt.ldd = st.ldx; gt.SUM = GSUM; gt.lds = ldgs;
  gt.mu = gn->mu;
  if (ws) { gt.W = ws->W; gt.ldw = ws->ldw; }
  const bool tiled = ws && ws->tiled;
  const StepArgs step{st.X, st.ldx, st.D, st.ldx, st.ALPHA, 0.0, XL, XU, ldxb, st.XC, st.ldx, st.SSUM, st.ldss};
  VerdictArgs vd{st.X, st.GR, st.XC, st.ldx, st.FC, st.SCAL, st.ldsc, st.ISTATE, st.RSUM, st.ldrs};
  if (lazy) { vd.VERDICT = lazy->VERDICT; vd.NDIR = lazy->NDIR; vd.c1 = params->c1; }
  if (int rc = bind(h)) return rc;
  if (int rc = lbfgs_fits(h)) return rc;
  if (int rc = tiled ? gn_tiled_fits(h) : ws ? gn_direct_fits(h) : gn_fits(h)) return rc;
  if (iters == 0) return TOWR_OK;
  return fused(h, B, stream, {tiled ? gn_tiled_ready : ws ? gn_direct_ready : gn_ready, residual_ready, step_ready}, [&](const Batch& b) {
    int rc = TOWR_OK;
    for (int it = 0; it < iters && rc == TOWR_OK; ++it) {
      if (probe) rc = probe_stage(h, B, *params, probe->trials, st, GL, GU, ldgb, XL, XU, ldxb, PSUM, ldps, b);
      if (rc == TOWR_OK) rc = launch_cost(h, B, st.XC, st.ldx, st.FC, st.GRC, st.ldx, b.s, b.ter, b.per);
      if (rc == TOWR_OK)
        rc = auglag_chunks(h, B, EvalStage{st.XC, st.ldx, nullptr, 0}, r, product(nullptr, 0, nullptr, 0, st.GRC, st.ldx, 1), b,
                           ws ? nullptr : &g, ws && !tiled ? &gd : nullptr, ws ? ws->wrows : 0, tiled ? &gt : nullptr,
                           lazy ? &vd : nullptr);
      if (rc == TOWR_OK) rc = launch_linesearch(h, B, *params, st, XL, XU, ldxb, b.s);
      if (rc == TOWR_OK && stop) rc = launch_stop(h, B, *params, *stop, st, b.s);
      if (rc == TOWR_OK) rc = launch_outer(h, B, *params, st, b.s);
      if (rc == TOWR_OK) rc = launch_gn_select(h, B, st, DC, b.s);
      if (rc == TOWR_OK) rc = launch_step(h, B, step, b.s);
    }
    return rc;
  }, ter);
}

int towr_gpu_alsolve_gn_iterate_batch_device(towr_gpu_handle h, int32_t B, int32_t iters, const towr_alsolve_params_t* params,
                                             const towr_alsolve_state_t* state, const towr_gn_params_t* gn, double* DC,
                                             double* GSUM, int64_t ldgs, const double* GL, const double* GU, int64_t ldgb,
                                             const double* XL, const double* XU, int64_t ldxb, void* stream) {
  return alsolve_gn_iterate(h, B, iters, params, state, gn, DC, GSUM, ldgs, false, TOWR_GN_PC_NONE, nullptr, GL, GU, ldgb, XL, XU,
                            ldxb, stream);
}

int towr_gpu_alsolve_gn_pc_iterate_batch_device(towr_gpu_handle h, int32_t B, int32_t iters, const towr_alsolve_params_t* params,
                                                const towr_alsolve_state_t* state, const towr_gn_params_t* gn, int32_t precond,
                                                double* DC, double* GSUM, int64_t ldgs, double* PC, const double* GL,
                                                const double* GU, int64_t ldgb, const double* XL, const double* XU, int64_t ldxb,
                                                void* stream) {
  return alsolve_gn_iterate(h, B, iters, params, state, gn, DC, GSUM, ldgs, true, precond, PC, GL, GU, ldgb, XL, XU, ldxb, stream);
}

// ---- the direct Gauss-Newton direction (jprod.hip): envelope Cholesky of rho (J^T W J)_ff + mu I -----------------------
int towr_gpu_gn_factor_info(towr_gpu_handle h, int32_t* ordering, int32_t* pos, int32_t* first, int64_t* envelope,
                            int64_t* bandwidth, int64_t* ldw_min) {
  if (!h) return fail(h, TOWR_ERR_INVALID, "null handle");
  gn_factor_tables(h);
  const towr_gpu_handle_s::AugLag& al = h->al;
  if (ordering) *ordering = TOWR_GN_ORDER_RCM;
  if (pos && h->L.n) std::memcpy(pos, al.gf_pos.data(), sizeof(int32_t) * al.gf_pos.size());
  if (first && h->L.n) std::memcpy(first, al.gf_first.data(), sizeof(int32_t) * al.gf_first.size());
  if (envelope) *envelope = al.gf_env;
  if (bandwidth) *bandwidth = al.gf_width;
  if (ldw_min) *ldw_min = al.gf_env;
  return TOWR_OK;
}

int towr_gpu_gn_direction_direct_batch_device(towr_gpu_handle h, int32_t B, const towr_gn_params_t* gn, const double* V,
                                              int64_t ldv, const double* LAMP, int64_t ldlp, const double* RHO, double rho,
                                              const double* X, int64_t ldx, const double* GR, int64_t ldgr, const double* XL,
                                              const double* XU, int64_t ldb, const int32_t* RUN, int32_t run_stride, double* D,
                                              int64_t ldd, double* SUM, int64_t lds, double* W, int64_t ldw, int32_t wrows,
                                              void* stream) {
  if (!h || B < 0 || !V || !LAMP || !GR) return fail(h, TOWR_ERR_INVALID, "bad argument (null V, LAMP or GR, or B < 0)");
  const GnWorkspace ws{W, ldw, wrows};
  if (int rc = gn_direct_params(h, gn, D, SUM, lds, ws)) return rc;
  const Layout& L = h->L;
  if (ws_overlap(h, B, ws, V, ldv, L.nnz) || ws_overlap(h, B, ws, LAMP, ldlp, L.m) || ws_overlap(h, B, ws, X, ldx, L.n) ||
      ws_overlap(h, B, ws, GR, ldgr, L.n) || ws_overlap(h, B, ws, D, ldd, L.n) || ws_overlap(h, B, ws, SUM, lds, 8))
    return fail(h, TOWR_ERR_INVALID, "gn: W overlaps V, LAMP, X, GR, D or SUM");
  if (!RHO && !(rho > 0)) return fail(h, TOWR_ERR_INVALID, "rho must be > 0 without RHO");
  if (ldv < L.nnz || ldlp < L.m || (X && ldx < L.n) || ldgr < L.n || ldd < L.n)
    return fail(h, TOWR_ERR_INVALID, "leading dimension smaller than nnz (V) / m (LAMP) / n (X, GR, D)");
  if (int rc = box_args(h, XL, XU, ldb, L.n, "XL / XU", "n")) return rc;
  if (int rc = bind(h)) return rc;
  if (int rc = gn_direct_fits(h)) return rc;
  if (B == 0) return TOWR_OK;
  if (int rc = gn_direct_ready(h)) return rc;
  if (X && !XL)
    if (int rc = step_ready(h)) return rc;
  GnDirectArgs a{V, ldv, LAMP, ldlp, RHO, rho, X, ldx, GR, ldgr, XL, XU, ldb, RUN, run_stride, D, ldd, SUM, lds, W, ldw, gn->mu};
  return launch_gn_direct(h, B, a, wrows, reinterpret_cast<hipStream_t>(stream));
}

int towr_gpu_alsolve_gn_direct_iterate_batch_device(towr_gpu_handle h, int32_t B, int32_t iters, const towr_alsolve_params_t* params,
                                                    const towr_alsolve_state_t* state, const towr_gn_params_t* gn, double* DC,
                                                    double* GSUM, int64_t ldgs, double* W, int64_t ldw, int32_t wrows,
                                                    const double* GL, const double* GU, int64_t ldgb, const double* XL,
                                                    const double* XU, int64_t ldxb, void* stream) {
  const GnWorkspace ws{W, ldw, wrows};
  return alsolve_gn_iterate(h, B, iters, params, state, gn, DC, GSUM, ldgs, false, TOWR_GN_PC_NONE, nullptr, GL, GU, ldgb, XL, XU,
                            ldxb, stream, &ws);
}

// ---- the tiled direct Gauss-Newton direction (jprod.hip): block Cholesky on the 16 x 16 tile envelope ---------------------
int towr_gpu_gn_tile_info(towr_gpu_handle h, int32_t* tile, int32_t* nt, int32_t* bfirst, int64_t* tiles, int64_t* ldw_min) {
  if (!h) return fail(h, TOWR_ERR_INVALID, "null handle");
  gn_tile_tables(h);
  const towr_gpu_handle_s::AugLag& al = h->al;
  if (tile) *tile = TOWR_GN_TILE;
  if (nt) *nt = (int32_t)al.gt_bfirst.size();
  if (bfirst && !al.gt_bfirst.empty()) std::memcpy(bfirst, al.gt_bfirst.data(), sizeof(int32_t) * al.gt_bfirst.size());
  if (tiles) *tiles = al.gt_tiles;
  if (ldw_min) *ldw_min = 256 * al.gt_tiles;
  return TOWR_OK;
}

int towr_gpu_gn_direction_tiled_batch_device(towr_gpu_handle h, int32_t B, const towr_gn_params_t* gn, const double* V,
                                             int64_t ldv, const double* LAMP, int64_t ldlp, const double* RHO, double rho,
                                             const double* X, int64_t ldx, const double* GR, int64_t ldgr, const double* XL,
                                             const double* XU, int64_t ldb, const int32_t* RUN, int32_t run_stride, double* D,
                                             int64_t ldd, double* SUM, int64_t lds, double* W, int64_t ldw, int32_t wrows,
                                             void* stream) {
  if (!h || B < 0 || !V || !LAMP || !GR) return fail(h, TOWR_ERR_INVALID, "bad argument (null V, LAMP or GR, or B < 0)");
  const GnWorkspace ws{W, ldw, wrows, true};
  if (int rc = gn_direct_params(h, gn, D, SUM, lds, ws)) return rc;
  const Layout& L = h->L;
  if (ws_overlap(h, B, ws, V, ldv, L.nnz) || ws_overlap(h, B, ws, LAMP, ldlp, L.m) || ws_overlap(h, B, ws, X, ldx, L.n) ||
      ws_overlap(h, B, ws, GR, ldgr, L.n) || ws_overlap(h, B, ws, D, ldd, L.n) || ws_overlap(h, B, ws, SUM, lds, 8))
    return fail(h, TOWR_ERR_INVALID, "gn: W overlaps V, LAMP, X, GR, D or SUM");
  if (!RHO && !(rho > 0)) return fail(h, TOWR_ERR_INVALID, "rho must be > 0 without RHO");
  if (ldv < L.nnz || ldlp < L.m || (X && ldx < L.n) || ldgr < L.n || ldd < L.n)
    return fail(h, TOWR_ERR_INVALID, "leading dimension smaller than nnz (V) / m (LAMP) / n (X, GR, D)");
  if (int rc = box_args(h, XL, XU, ldb, L.n, "XL / XU", "n")) return rc;
  if (int rc = bind(h)) return rc;
  if (int rc = gn_tiled_fits(h)) return rc;
  if (B == 0) return TOWR_OK;
  if (int rc = gn_tiled_ready(h)) return rc;
  if (X && !XL)
    if (int rc = step_ready(h)) return rc;
  GnTiledArgs a{V, ldv, LAMP, ldlp, RHO, rho, X, ldx, GR, ldgr, XL, XU, ldb, RUN, run_stride, D, ldd, SUM, lds, W, ldw, gn->mu};
  return launch_gn_tiled(h, B, a, wrows, reinterpret_cast<hipStream_t>(stream));
}

int towr_gpu_alsolve_gn_tiled_iterate_batch_device(towr_gpu_handle h, int32_t B, int32_t iters, const towr_alsolve_params_t* params,
                                                   const towr_alsolve_state_t* state, const towr_gn_params_t* gn, double* DC,
                                                   double* GSUM, int64_t ldgs, double* W, int64_t ldw, int32_t wrows,
                                                   const double* GL, const double* GU, int64_t ldgb, const double* XL,
                                                   const double* XU, int64_t ldxb, void* stream) {
  const GnWorkspace ws{W, ldw, wrows, true};
  return alsolve_gn_iterate(h, B, iters, params, state, gn, DC, GSUM, ldgs, false, TOWR_GN_PC_NONE, nullptr, GL, GU, ldgb, XL, XU,
                            ldxb, stream, &ws);
}

// ---- the lazy GN loop: the line search's verdict ahead of the direction (lbfgs.hip) -------------------------------------
int towr_gpu_alsolve_verdict_batch_device(towr_gpu_handle h, int32_t B, const towr_alsolve_params_t* params,
                                          const towr_alsolve_state_t* state, int32_t* VERDICT, int32_t* NDIR, void* stream) {
  if (!h || B < 0) return fail(h, TOWR_ERR_INVALID, "bad argument (B < 0)");
  if (int rc = alsolve_params(h, params)) return rc;
  if (!state) return fail(h, TOWR_ERR_INVALID, "null state");
  if (!VERDICT) return fail(h, TOWR_ERR_INVALID, "verdict: null VERDICT");
  const towr_alsolve_state_t& st = *state;   // (of the state only what the test reads)
  if (!st.X || !st.GR || !st.XC) return fail(h, TOWR_ERR_INVALID, "state: null X, GR or XC");
  if (!st.FC || !st.SCAL || !st.ISTATE || !st.RSUM) return fail(h, TOWR_ERR_INVALID, "state: null FC, SCAL, ISTATE or RSUM");
  if (st.ldx < h->L.n) return fail(h, TOWR_ERR_INVALID, "state: ldx smaller than n");
  if (st.ldsc < 8) return fail(h, TOWR_ERR_INVALID, "state: ldsc smaller than 8");
  if (st.ldrs < 4) return fail(h, TOWR_ERR_INVALID, "state: ldrs smaller than 4");
  if (int rc = bind(h)) return rc;
  if (int rc = lbfgs_fits(h)) return rc;
  if (B == 0) return TOWR_OK;
  VerdictArgs a{st.X, st.GR, st.XC, st.ldx, st.FC, st.SCAL, st.ldsc, st.ISTATE, st.RSUM, st.ldrs, VERDICT, NDIR, params->c1};
  return launch_verdict(h, B, a, 0, reinterpret_cast<hipStream_t>(stream));
}

int towr_gpu_alsolve_gn_lazy_iterate_batch_device(towr_gpu_handle h, int32_t B, int32_t iters, int32_t method,
                                                  const towr_alsolve_params_t* params, const towr_alsolve_state_t* state,
                                                  const towr_solve_dir_t* dir, const towr_alsolve_lazy_t* lazy, const double* GL,
                                                  const double* GU, int64_t ldgb, const double* XL, const double* XU,
                                                  int64_t ldxb, void* stream) {
  if (!h) return fail(h, TOWR_ERR_INVALID, "null handle");
  if (!dir) return fail(h, TOWR_ERR_INVALID, "lazy: null dir");
  if (method < TOWR_SOLVE_GN || method > TOWR_SOLVE_GN_TILED)
    return fail(h, TOWR_ERR_INVALID, "lazy: method outside TOWR_SOLVE_GN..TOWR_SOLVE_GN_TILED (L-BFGS has no direction at the candidate)");
  if (!lazy) return fail(h, TOWR_ERR_INVALID, "null lazy");
  const bool pc = method == TOWR_SOLVE_GN_PC;
  const GnWorkspace ws{dir->W, dir->ldw, dir->wrows, method == TOWR_SOLVE_GN_TILED};
  return alsolve_gn_iterate(h, B, iters, params, state, dir->gn, dir->DC, dir->GSUM, dir->ldgs, pc,
                            pc ? dir->precond : (int32_t)TOWR_GN_PC_NONE, pc ? dir->PC : nullptr, GL, GU, ldgb, XL, XU, ldxb, stream,
                            method >= TOWR_SOLVE_GN_DIRECT ? &ws : nullptr, nullptr, nullptr, nullptr, nullptr, 0, lazy);
}

// ---- a solve to completion: rounds of the resident loop, frozen problems compacted out (lbfgs.hip) ---------------------
// what the swap refuses of its descriptors
static int swap_rows_args(towr_gpu_handle h, int32_t n_arrays, const towr_rows_t* arrays) {
  if (n_arrays < 0 || n_arrays > TOWR_SWAP_MAX_ARRAYS) return fail(h, TOWR_ERR_INVALID, "swap: n_arrays outside 0..TOWR_SWAP_MAX_ARRAYS");
  if (n_arrays > 0 && !arrays) return fail(h, TOWR_ERR_INVALID, "swap: null arrays");
  for (int k = 0; k < n_arrays; ++k) {
    const towr_rows_t& r = arrays[k];
    if (!r.base || (reinterpret_cast<uintptr_t>(r.base) & 3)) return fail(h, TOWR_ERR_INVALID, "swap: array " + std::to_string(k) + ": base is NULL or not a multiple of 4");
    if (r.row_bytes <= 0 || (r.row_bytes & 3)) return fail(h, TOWR_ERR_INVALID, "swap: array " + std::to_string(k) + ": row_bytes is not a positive multiple of 4");
    if (r.ld_bytes <= 0 || (r.ld_bytes & 3)) return fail(h, TOWR_ERR_INVALID, "swap: array " + std::to_string(k) + ": ld_bytes is not a positive multiple of 4");
    if (r.ld_bytes < r.row_bytes) return fail(h, TOWR_ERR_INVALID, "swap: array " + std::to_string(k) + ": ld_bytes smaller than row_bytes");
    for (int j = 0; j < k; ++j) {
      const char *p = static_cast<const char*>(arrays[j].base), *q = static_cast<const char*>(r.base);
      if (p < q + r.row_bytes && q < p + arrays[j].row_bytes)
        return fail(h, TOWR_ERR_INVALID, "swap: arrays " + std::to_string(j) + " and " + std::to_string(k) + " overlap");
    }
  }
  return TOWR_OK;
}

static int launch_partition(towr_gpu_handle h, int B, const int32_t* ISTATE, int32_t* HEAD, int32_t* PAIRS, hipStream_t s) {
  PartitionArgs a{ISTATE, HEAD, PAIRS, B, 0};
  void* args[] = {&a};
  HIPCHK(h, launch_kernel(alsolve_partition_kernel(), dim3(1), dim3(kLbfgsBlock), args, 0, s));
  return TOWR_OK;
}

// (NP NULL: `pairs` is the count; else the grid's pairs. After swap_rows_args.)
static int launch_swap_rows(towr_gpu_handle h, const int32_t* NP, int pairs, const int32_t* PAIRS, int n_arrays,
                            const towr_rows_t* arrays, hipStream_t s) {
  if (pairs == 0 || n_arrays == 0) return TOWR_OK;
  SwapRowsArgs a{};
  a.NP = NP; a.PAIRS = PAIRS; a.npairs = pairs; a.n_arrays = n_arrays;
  for (int k = 0; k < n_arrays; ++k) a.rows[k] = SwapRows{static_cast<char*>(arrays[k].base), arrays[k].ld_bytes, arrays[k].row_bytes};
  void* args[] = {&a};
  HIPCHK(h, launch_kernel(alsolve_swap_rows_kernel(), dim3((unsigned)pairs, (unsigned)n_arrays), dim3(kLbfgsBlock), args, 0, s));
  return TOWR_OK;
}

// what the move refuses of its descriptor pairs (the swap's rules for either side; a pair shares one row length)
static int move_rows_args(towr_gpu_handle h, int32_t n_arrays, const towr_rows_t* slot, const towr_rows_t* out) {
  if (n_arrays < 0 || n_arrays > TOWR_MOVE_MAX_ARRAYS) return fail(h, TOWR_ERR_INVALID, "move: n_arrays outside 0..TOWR_MOVE_MAX_ARRAYS");
  if (n_arrays > 0 && (!slot || !out)) return fail(h, TOWR_ERR_INVALID, "move: null slot or out descriptors");
  for (int k = 0; k < n_arrays; ++k) {
    const std::string pair = "move: pair " + std::to_string(k) + ": ";
    if (slot[k].row_bytes != out[k].row_bytes) return fail(h, TOWR_ERR_INVALID, pair + "the two row_bytes differ");
    if (slot[k].row_bytes <= 0 || (slot[k].row_bytes & 3)) return fail(h, TOWR_ERR_INVALID, pair + "row_bytes is not a positive multiple of 4");
    for (const towr_rows_t* r : {&slot[k], &out[k]}) {
      if (!r->base || (reinterpret_cast<uintptr_t>(r->base) & 3)) return fail(h, TOWR_ERR_INVALID, pair + "base is NULL or not a multiple of 4");
      if (r->ld_bytes <= 0 || (r->ld_bytes & 3)) return fail(h, TOWR_ERR_INVALID, pair + "ld_bytes is not a positive multiple of 4");
      if (r->ld_bytes < r->row_bytes) return fail(h, TOWR_ERR_INVALID, pair + "ld_bytes smaller than row_bytes");
    }
  }
  return TOWR_OK;
}

// (add: AGE += add before the compare; after the entry's checks)
static int launch_retire_key(towr_gpu_handle h, int B, const int32_t* ISTATE, int32_t* AGE, int32_t* KEY, int add, int max_age,
                             hipStream_t s) {
  if (B == 0) return TOWR_OK;
  RetireKeyArgs a{ISTATE, AGE, KEY, B, add, max_age, 0};
  void* args[] = {&a};
  HIPCHK(h, launch_kernel(alsolve_retire_key_kernel(), dim3((unsigned)((B + kLbfgsBlock - 1) / kLbfgsBlock)), dim3(kLbfgsBlock), args, 0, s));
  return TOWR_OK;
}

// (after move_rows_args)
static int launch_move_rows(towr_gpu_handle h, const int32_t* ID, int r0, int count, int n_arrays, const towr_rows_t* slot,
                            const towr_rows_t* out, bool reverse, hipStream_t s) {
  if (count == 0 || n_arrays == 0) return TOWR_OK;
  MoveRowsArgs a{};
  a.ID = ID; a.r0 = r0; a.count = count; a.n_arrays = n_arrays; a.reverse = reverse ? 1 : 0;
  for (int k = 0; k < n_arrays; ++k)
    a.rows[k] = MoveRows{static_cast<char*>(slot[k].base), slot[k].ld_bytes, static_cast<char*>(out[k].base), out[k].ld_bytes,
                         slot[k].row_bytes};
  void* args[] = {&a};
  HIPCHK(h, launch_kernel(alsolve_move_rows_kernel(), dim3((unsigned)count, (unsigned)n_arrays), dim3(kLbfgsBlock), args, 0, s));
  return TOWR_OK;
}

int towr_gpu_alsolve_retire_key_batch_device(towr_gpu_handle h, int32_t B, const int32_t* ISTATE, int32_t* AGE, int32_t add,
                                             int32_t max_age, int32_t* KEY, void* stream) {
  if (!h || B < 0 || !ISTATE || !AGE || !KEY) return fail(h, TOWR_ERR_INVALID, "bad argument (null ISTATE, AGE or KEY, or B < 0)");
  if (add < 0) return fail(h, TOWR_ERR_INVALID, "retire key: add is negative");
  if (int rc = bind(h)) return rc;
  return launch_retire_key(h, B, ISTATE, AGE, KEY, add, max_age, reinterpret_cast<hipStream_t>(stream));
}

int towr_gpu_alsolve_move_rows_batch_device(towr_gpu_handle h, const int32_t* ID, int32_t r0, int32_t count, int32_t n_arrays,
                                            const towr_rows_t* slot, const towr_rows_t* out, int32_t reverse, void* stream) {
  if (!h || !ID) return fail(h, TOWR_ERR_INVALID, "bad argument (null ID)");
  if (r0 < 0 || count < 0) return fail(h, TOWR_ERR_INVALID, "move: negative r0 or count");
  if (reverse != 0 && reverse != 1) return fail(h, TOWR_ERR_INVALID, "move: reverse outside {0, 1}");
  if (int rc = move_rows_args(h, n_arrays, slot, out)) return rc;
  if (int rc = bind(h)) return rc;
  return launch_move_rows(h, ID, r0, count, n_arrays, slot, out, reverse == 1, reinterpret_cast<hipStream_t>(stream));
}

int towr_gpu_alsolve_partition_batch_device(towr_gpu_handle h, int32_t B, const int32_t* ISTATE, int32_t* HEAD, int32_t* PAIRS,
                                            void* stream) {
  if (!h || B < 0 || !ISTATE || !HEAD || !PAIRS) return fail(h, TOWR_ERR_INVALID, "bad argument (null ISTATE, HEAD or PAIRS, or B < 0)");
  if (int rc = bind(h)) return rc;
  return launch_partition(h, B, ISTATE, HEAD, PAIRS, reinterpret_cast<hipStream_t>(stream));   // (B = 0: HEAD = 0)
}

int towr_gpu_alsolve_swap_rows_batch_device(towr_gpu_handle h, const int32_t* NP, int32_t npairs, int32_t max_pairs,
                                            const int32_t* PAIRS, int32_t n_arrays, const towr_rows_t* arrays, void* stream) {
  if (!h || !PAIRS) return fail(h, TOWR_ERR_INVALID, "bad argument (null PAIRS)");
  if (NP ? max_pairs < 0 : npairs < 0) return fail(h, TOWR_ERR_INVALID, "swap: negative pair count (npairs without NP, max_pairs with it)");
  if (int rc = swap_rows_args(h, n_arrays, arrays)) return rc;
  if (int rc = bind(h)) return rc;
  return launch_swap_rows(h, NP, NP ? max_pairs : npairs, PAIRS, n_arrays, arrays, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"

// The per-problem rows of the state and of the method's direction (towr_gpu.h lists them with their used widths), in the
// order both solve drivers exchange them: add(base, ld_bytes, row_bytes).
template <class Add>
static void solve_state_rows(const Layout& L, const towr_alsolve_params_t& par, const towr_alsolve_state_t& st,
                             const towr_solve_dir_t& dir, int method, Add add) {
  for (double* p : {st.X, st.GR, st.XC, st.GRC, st.D}) add(p, 8 * st.ldx, 8 * (int64_t)L.n);
  for (double* p : {st.LAM, st.LAMP}) add(p, 8 * st.ldl, 8 * (int64_t)L.m);
  for (double* p : {st.HS, st.HY}) add(p, 8 * par.mem * st.ldh, 8 * ((par.mem - 1) * st.ldh + L.n));
  add(st.HMETA, 8, 8);
  for (double* p : {st.ALPHA, st.RHO, st.FC}) add(p, 8, 8);
  add(st.SCAL, 8 * st.ldsc, 64);
  add(st.ISTATE, 16, 16);
  add(st.RSUM, 8 * st.ldrs, 8 * (4 + (int64_t)L.cons.size()));
  add(st.SSUM, 8 * st.ldss, 8 * (5 + (int64_t)L.varsets.size()));
  add(st.DSUM, 8 * st.ldds, 40);
  add(st.USUM, 8 * st.ldus, 48);
  add(st.LSUM, 8 * st.ldls, 64);
  if (method != TOWR_SOLVE_LBFGS) {
    add(dir.DC, 8 * st.ldx, 8 * (int64_t)L.n);
    add(dir.GSUM, 8 * dir.ldgs, method == TOWR_SOLVE_GN ? 48 : 64);
  }
}

// the four solve entries; stop NULL: the plain loop and the plain report; probe NULL: no probe stage (PSUM is not read);
// lazy NULL: the method's iterate entry as it is, else the lazy GN iteration (NDIR among the exchanged rows)
static int alsolve_solve(towr_gpu_handle h, int32_t B, const towr_solve_opts_t* opts, const towr_alsolve_params_t* params,
                         const towr_alsolve_stop_t* stop, const towr_alsolve_state_t* state, const towr_solve_dir_t* dir,
                         double* GL, double* GU, int64_t ldgb, double* XL, double* XU, int64_t ldxb, int32_t* LOG,
                         towr_solve_report_t* report, void* stream, const towr_alsolve_probe_t* probe = nullptr,
                         double* PSUM = nullptr, int64_t ldps = 0, const towr_alsolve_lazy_t* lazy = nullptr) {
  if (!h) return fail(h, TOWR_ERR_INVALID, "null handle");
  if (!opts || !dir || !LOG || !report) return fail(h, TOWR_ERR_INVALID, "solve: null opts, dir, LOG or report");
  if (opts->method < TOWR_SOLVE_LBFGS || opts->method > TOWR_SOLVE_GN_TILED) return fail(h, TOWR_ERR_INVALID, "solve: method outside 0..4");
  if (lazy && opts->method == TOWR_SOLVE_LBFGS) return fail(h, TOWR_ERR_INVALID, "solve: lazy needs a GN method (L-BFGS has no direction at the candidate)");
  if (opts->max_iters < 0) return fail(h, TOWR_ERR_INVALID, "solve: max_iters is negative");
  if (opts->check_every < 1) return fail(h, TOWR_ERR_INVALID, "solve: check_every must be >= 1");
  if (opts->compact != 0 && opts->compact != 1) return fail(h, TOWR_ERR_INVALID, "solve: compact outside {0, 1}");
  const int method = opts->method;
  const bool gn = method != TOWR_SOLVE_LBFGS, compact = opts->compact == 1;
  const GnWorkspace ws{dir->W, dir->ldw, dir->wrows, method == TOWR_SOLVE_GN_TILED};
  // `iters` iterations of the method's iterate entry on rows [0, Bc): its own checks and launches (iters = 0: the checks)
  auto iterate = [&](int Bc, int iters, const towr_terrain_t* ter) -> int {
    if (!gn) return alsolve_lbfgs_iterate(h, Bc, iters, params, state, GL, GU, ldgb, XL, XU, ldxb, stream, ter, stop, probe, PSUM, ldps);
    const bool pc = method == TOWR_SOLVE_GN_PC;
    return alsolve_gn_iterate(h, Bc, iters, params, state, dir->gn, dir->DC, dir->GSUM, dir->ldgs, pc,
                              pc ? dir->precond : (int32_t)TOWR_GN_PC_NONE, pc ? dir->PC : nullptr, GL, GU, ldgb, XL, XU, ldxb, stream,
                              method >= TOWR_SOLVE_GN_DIRECT ? &ws : nullptr, ter, stop, probe, PSUM, ldps, lazy);
  };
  // the iterate entry's refusals, TOWR_ERR_NO_DEVICE and TOWR_ERR_UNSUPPORTED (it binds the handle); nothing is queued.
  // Its argument checks come first: with another code they have passed, and this entry's own follow before that code
  const int pre = iterate(B, 0, nullptr);
  if (pre == TOWR_ERR_INVALID) return pre;
  if (h->d_bterrain && h->bterrain_n != B)
    return fail(h, TOWR_ERR_INVALID, "batch terrains are set for " + std::to_string(h->bterrain_n) + " problems, the call has " +
                                         std::to_string(B));
  // the per-problem arrays (towr_gpu.h): what a round's swap exchanges
  const Layout& L = h->L;
  const towr_alsolve_state_t& st = *state;
  towr_rows_t rows[TOWR_SWAP_MAX_ARRAYS];
  int nr = 0;
  auto add = [&](void* base, int64_t ld_bytes, int64_t row_bytes) {   // (n or m = 0: nothing to exchange)
    if (row_bytes > 0) rows[nr++] = towr_rows_t{base, ld_bytes, row_bytes};
  };
  solve_state_rows(L, *params, st, *dir, method, add);
  if (lazy && lazy->NDIR) add(lazy->NDIR, 4, 4);   // (VERDICT is rewritten by every iteration: not exchanged)
  if (GL && ldgb > 0) for (double* p : {GL, GU}) add(p, 8 * ldgb, 8 * (int64_t)L.m);
  if (XL && ldxb > 0) for (double* p : {XL, XU}) add(p, 8 * ldxb, 8 * (int64_t)L.n);
  if (int rc = swap_rows_args(h, nr, rows)) return rc;
  if (pre != TOWR_OK) return pre;

  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  towr_gpu_handle_s::AugLag& al = h->al;
  if (!al.h_head) HIPCHK(h, hipHostMalloc(reinterpret_cast<void**>(&al.h_head), 8 * sizeof(int32_t), hipHostMallocDefault));
  towr_terrain_t* ter = nullptr;   // the private copy of the batch terrains, exchanged with the rest
  if (h->d_bterrain && B > 0 && opts->max_iters > 0) {
    HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&ter), sizeof(towr_terrain_t) * (size_t)B));
    if (hipMemcpyAsync(ter, h->d_bterrain, sizeof(towr_terrain_t) * (size_t)B, hipMemcpyDeviceToDevice, s) != hipSuccess) {
      (void)hipFree(ter);
      return fail(h, TOWR_ERR_HIP, "solve: copying the batch terrains failed");
    }
    static_assert(sizeof(towr_terrain_t) % 8 == 0, "a terrain is exchanged as 8-byte words");
    add(ter, sizeof(towr_terrain_t), sizeof(towr_terrain_t));
  }
  // HEAD to the host behind everything queued so far
  auto head_sync = [&]() -> int {
    HIPCHK(h, hipMemcpyAsync(al.h_head, LOG, 8 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return TOWR_OK;
  };

  int32_t* pairs = LOG + 8;
  std::vector<std::pair<int64_t, int>> swaps;   // per round that moved rows: (its first pair in the log, its pairs)
  int64_t used = 0, problem_iters = 0;
  int rounds = 0, iters_run = 0, Bcur = B, rc = TOWR_OK;
  bool lost = false;   // a swap was queued whose pair count never reached the host
  while (rc == TOWR_OK && iters_run < opts->max_iters && Bcur > 0) {
    const int k = std::min(opts->check_every, opts->max_iters - iters_run);
    rc = iterate(Bcur, k, ter);
    if (rc == TOWR_OK) rc = launch_partition(h, Bcur, st.ISTATE, LOG, pairs + 2 * used, s);
    if (rc == TOWR_OK && compact) rc = launch_swap_rows(h, LOG + 1, Bcur / 2, pairs + 2 * used, nr, rows, s);
    if (rc == TOWR_OK && (rc = head_sync()) != TOWR_OK) lost = compact;
    if (rc != TOWR_OK) break;
    ++rounds;
    iters_run += k;
    problem_iters += (int64_t)Bcur * k;
    const int na = al.h_head[0], np = al.h_head[1];
    if (compact) {
      if (np > 0) swaps.emplace_back(used, np);
      used += np;
      Bcur = na;
    }
    if (na == 0) break;
  }
  // back to the caller's order: the rounds' swaps again, the last first
  int rb = TOWR_OK;
  for (auto it = swaps.rbegin(); it != swaps.rend() && rb == TOWR_OK; ++it)
    rb = launch_swap_rows(h, nullptr, it->second, pairs + 2 * it->first, nr, rows, s);
  if (rb == TOWR_OK) rb = launch_partition(h, B, st.ISTATE, LOG, pairs, s);
  if (rb == TOWR_OK) rb = head_sync();
  else (void)hipStreamSynchronize(s);
  if (ter) (void)hipFree(ter);
  if (rc != TOWR_OK) {
    if (rb != TOWR_OK || lost) return fail(h, rc, "solve: a round failed and so did putting the rows back: the row order is unspecified");
    return rc;
  }
  if (rb != TOWR_OK) return fail(h, rb, "solve: putting the rows back failed: the row order is unspecified");
  report->rounds = rounds;
  report->iters_run = iters_run;
  report->problem_iters = problem_iters;
  for (int k = 0; k < 6; ++k) report->n_phase[k] = al.h_head[2 + k];
  report->reserved[0] = report->reserved[1] = 0;
  if (stop && B > 0) {   // the two new words among "any other word": counted on the host from the phase words
    std::vector<int32_t> is(4 * (size_t)B);
    HIPCHK(h, hipMemcpyAsync(is.data(), st.ISTATE, sizeof(int32_t) * is.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    for (int b = 0; b < B; ++b) {
      if (is[4 * (size_t)b] == kAlAcceptable) ++report->reserved[0];
      if (is[4 * (size_t)b] == kAlInfeasible) ++report->reserved[1];
    }
  }
  return TOWR_OK;
}

// ---- a queue of problems through the resident solve's slots ----------------------------------------------------------------
// the state's rows from row r on
static towr_alsolve_state_t state_from_row(const towr_alsolve_state_t& s, int r, int mem) {
  towr_alsolve_state_t o = s;
  const int64_t b = r;
  for (double** p : {&o.X, &o.GR, &o.XC, &o.GRC, &o.D}) *p += b * s.ldx;
  for (double** p : {&o.LAM, &o.LAMP}) *p += b * s.ldl;
  for (double** p : {&o.HS, &o.HY}) *p += b * mem * s.ldh;
  o.HMETA += 2 * b;
  for (double** p : {&o.ALPHA, &o.RHO, &o.FC}) *p += b;
  o.SCAL += b * s.ldsc;
  o.ISTATE += 4 * b;
  o.RSUM += b * s.ldrs;
  o.SSUM += b * s.ldss;
  o.DSUM += b * s.ldds;
  o.USUM += b * s.ldus;
  o.LSUM += b * s.ldls;
  return o;
}

// Rounds of admit / iterate / key, partition and swap / one host look / retire (towr_gpu.h). The frozen and the expired
// rows are swapped behind the live ones in every round and moved out from there; the variant that retires in place and
// admits into the holes was not built.
static int alsolve_solve_queue(towr_gpu_handle h, int32_t B, const towr_solve_opts_t* opts, const towr_alsolve_params_t* params,
                               const towr_alsolve_stop_t* stop, const towr_alsolve_state_t* state, const towr_solve_dir_t* dir,
                               const towr_solve_queue_t* queue, int32_t* LOG, towr_solve_report_t* report, void* stream) {
  if (!h) return fail(h, TOWR_ERR_INVALID, "null handle");
  if (!opts || !dir || !queue || !LOG || !report) return fail(h, TOWR_ERR_INVALID, "queue: null opts, dir, queue, LOG or report");
  if (opts->method < TOWR_SOLVE_LBFGS || opts->method > TOWR_SOLVE_GN_TILED) return fail(h, TOWR_ERR_INVALID, "queue: method outside 0..4");
  if (opts->check_every < 1) return fail(h, TOWR_ERR_INVALID, "queue: check_every must be >= 1");
  if (opts->max_iters < 1 || opts->max_iters % opts->check_every != 0)
    return fail(h, TOWR_ERR_INVALID, "queue: max_iters must be a positive multiple of check_every");
  if (opts->compact != 0 && opts->compact != 1) return fail(h, TOWR_ERR_INVALID, "queue: compact outside {0, 1} (it is not read)");
  const towr_solve_queue_t& q = *queue;
  const int N = q.N, K = opts->check_every, M = opts->max_iters, method = opts->method;
  if (N < 0) return fail(h, TOWR_ERR_INVALID, "queue: N is negative");
  if (N > 0 && B < 1) return fail(h, TOWR_ERR_INVALID, "queue: N problems need B >= 1 slots");
  const int64_t n = h->L.n, m = h->L.m;
  if (N > 0 && (!q.X0 || !q.ID || !q.AGE || !q.KEY || !q.X_OUT || (!q.LAM_OUT && m > 0) || !q.RHO_OUT || !q.SCAL_OUT || !q.ISTATE_OUT || !q.ITERS_OUT))
    return fail(h, TOWR_ERR_INVALID, "queue: null X0, ID, AGE, KEY, X_OUT, LAM_OUT, RHO_OUT, SCAL_OUT, ISTATE_OUT or ITERS_OUT");
  if (N > 0 && (q.ldx0 < n || q.ldxo < n)) return fail(h, TOWR_ERR_INVALID, "queue: ldx0 or ldxo below n");
  if (N > 0 && ((q.LAM0 && q.ldl0 < m) || q.ldlo < m)) return fail(h, TOWR_ERR_INVALID, "queue: ldl0 or ldlo below m");
  if (int rc = box_args(h, q.GL, q.GU, q.ldgb, m, "queue: GL / GU", "m")) return rc;
  if (int rc = box_args(h, q.XL, q.XU, q.ldxb, n, "queue: XL / XU", "n")) return rc;
  const bool per_g = q.GL && q.ldgb > 0, per_x = q.XL && q.ldxb > 0;
  if (per_g && (!q.GLW || !q.GUW || q.ldgw < m)) return fail(h, TOWR_ERR_INVALID, "queue: per-problem GL / GU need the work rows GLW, GUW (ldgw >= m)");
  if (per_x && (!q.XLW || !q.XUW || q.ldxw < n)) return fail(h, TOWR_ERR_INVALID, "queue: per-problem XL / XU need the work rows XLW, XUW (ldxw >= n)");
  // the bounds the launches see: the slot-side work rows, or the shared row / the handle's as they are
  double* GL = per_g ? q.GLW : const_cast<double*>(q.GL);
  double* GU = per_g ? q.GUW : const_cast<double*>(q.GU);
  double* XL = per_x ? q.XLW : const_cast<double*>(q.XL);
  double* XU = per_x ? q.XUW : const_cast<double*>(q.XU);
  const int64_t ldgb = per_g ? q.ldgw : 0, ldxb = per_x ? q.ldxw : 0;
  const bool gn = method != TOWR_SOLVE_LBFGS;
  const GnWorkspace ws{dir->W, dir->ldw, dir->wrows, method == TOWR_SOLVE_GN_TILED};
  auto iterate = [&](int Bc, int iters, const towr_terrain_t* ter) -> int {   // (alsolve_solve's)
    if (!gn) return alsolve_lbfgs_iterate(h, Bc, iters, params, state, GL, GU, ldgb, XL, XU, ldxb, stream, ter, stop);
    const bool pc = method == TOWR_SOLVE_GN_PC;
    return alsolve_gn_iterate(h, Bc, iters, params, state, dir->gn, dir->DC, dir->GSUM, dir->ldgs, pc,
                              pc ? dir->precond : (int32_t)TOWR_GN_PC_NONE, pc ? dir->PC : nullptr, GL, GU, ldgb, XL, XU, ldxb, stream,
                              method >= TOWR_SOLVE_GN_DIRECT ? &ws : nullptr, ter, stop);
  };
  // the iterate entry's refusals for B slots (iters = 0 queues nothing and does not look at the batch terrains' count)
  const int pre = iterate(B, 0, nullptr);
  if (pre == TOWR_ERR_INVALID) return pre;
  if (h->d_bterrain && h->bterrain_n != N)
    return fail(h, TOWR_ERR_INVALID, "batch terrains are set for " + std::to_string(h->bterrain_n) + " problems, the queue holds " +
                                         std::to_string(N));
  if (N == 0) {   // (an empty queue names no arrays)
    if (pre != TOWR_OK) return pre;
    *report = towr_solve_report_t{};
    return TOWR_OK;
  }
  const Layout& L = h->L;
  const towr_alsolve_state_t& st = *state;
  towr_rows_t rows[TOWR_SWAP_MAX_ARRAYS + 8];
  int nr = 0;
  auto add = [&](void* base, int64_t ld_bytes, int64_t row_bytes) {
    if (row_bytes > 0 && nr < TOWR_SWAP_MAX_ARRAYS + 8) rows[nr++] = towr_rows_t{base, ld_bytes, row_bytes};
  };
  solve_state_rows(L, *params, st, *dir, method, add);
  add(q.ID, 4, 4);
  add(q.AGE, 4, 4);
  if (per_g) for (double* p : {GL, GU}) add(p, 8 * ldgb, 8 * m);
  if (per_x) for (double* p : {XL, XU}) add(p, 8 * ldxb, 8 * n);
  const int ter_rows = h->d_bterrain ? 1 : 0;
  if (nr + ter_rows > TOWR_SWAP_MAX_ARRAYS) return fail(h, TOWR_ERR_INVALID, "queue: more per-problem arrays than TOWR_SWAP_MAX_ARRAYS");
  if (int rc = swap_rows_args(h, nr, rows)) return rc;
  // the moves: what admission gathers by ID (the queue's side is only read) and what retirement scatters
  towr_rows_t in_slot[TOWR_MOVE_MAX_ARRAYS], in_src[TOWR_MOVE_MAX_ARRAYS], out_slot[TOWR_MOVE_MAX_ARRAYS], out_dst[TOWR_MOVE_MAX_ARRAYS];
  int n_in = 0, n_out = 0;
  auto admit = [&](void* slot, int64_t slot_ld, const void* src, int64_t src_ld, int64_t row_bytes) {
    if (row_bytes <= 0) return;
    in_slot[n_in] = towr_rows_t{slot, slot_ld, row_bytes};
    in_src[n_in++] = towr_rows_t{const_cast<void*>(src), src_ld, row_bytes};
  };
  auto retire = [&](void* slot, int64_t slot_ld, void* dst, int64_t dst_ld, int64_t row_bytes) {
    if (row_bytes <= 0) return;
    out_slot[n_out] = towr_rows_t{slot, slot_ld, row_bytes};
    out_dst[n_out++] = towr_rows_t{dst, dst_ld, row_bytes};
  };
  admit(st.X, 8 * st.ldx, q.X0, 8 * q.ldx0, 8 * n);
  if (q.LAM0) admit(st.LAM, 8 * st.ldl, q.LAM0, 8 * q.ldl0, 8 * m);
  if (per_g) { admit(GL, 8 * ldgb, q.GL, 8 * q.ldgb, 8 * m); admit(GU, 8 * ldgb, q.GU, 8 * q.ldgb, 8 * m); }
  if (per_x) { admit(XL, 8 * ldxb, q.XL, 8 * q.ldxb, 8 * n); admit(XU, 8 * ldxb, q.XU, 8 * q.ldxb, 8 * n); }
  retire(st.X, 8 * st.ldx, q.X_OUT, 8 * q.ldxo, 8 * n);
  retire(st.LAM, 8 * st.ldl, q.LAM_OUT, 8 * q.ldlo, 8 * m);
  retire(st.RHO, 8, q.RHO_OUT, 8, 8);
  retire(st.SCAL, 8 * st.ldsc, q.SCAL_OUT, 64, 64);
  retire(st.ISTATE, 16, q.ISTATE_OUT, 16, 16);
  retire(q.AGE, 4, q.ITERS_OUT, 4, 4);
  if (int rc = move_rows_args(h, n_in, in_slot, in_src)) return rc;
  if (int rc = move_rows_args(h, n_out, out_slot, out_dst)) return rc;
  if (pre != TOWR_OK) return pre;

  *report = towr_solve_report_t{};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  towr_gpu_handle_s::AugLag& al = h->al;
  if (!al.h_head) HIPCHK(h, hipHostMalloc(reinterpret_cast<void**>(&al.h_head), 8 * sizeof(int32_t), hipHostMallocDefault));
  towr_terrain_t* ter = nullptr;   // the slots' terrains: gathered at admission, exchanged with the rows
  if (h->d_bterrain) {
    HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&ter), sizeof(towr_terrain_t) * (size_t)B));
    static_assert(sizeof(towr_terrain_t) % 8 == 0, "a terrain is moved as 8-byte words");
    add(ter, sizeof(towr_terrain_t), sizeof(towr_terrain_t));
    admit(ter, sizeof(towr_terrain_t), h->d_bterrain, sizeof(towr_terrain_t), sizeof(towr_terrain_t));
  }
  std::vector<int32_t> ids((size_t)N);   // (pageable: the copies below are staged before they return)
  for (int i = 0; i < N; ++i) ids[(size_t)i] = i;
  auto hip = [&](hipError_t e, const char* what) -> int {
    return e == hipSuccess ? TOWR_OK : fail(h, TOWR_ERR_HIP, std::string("queue: ") + what + " failed: " + hipGetErrorString(e));
  };

  int32_t* pairs = LOG + 8;
  int64_t problem_iters = 0;
  int rounds = 0, Bcur = 0, next = 0, rc = TOWR_OK;
  while (rc == TOWR_OK) {
    const int c = std::min(B - Bcur, N - next);
    if (c > 0) {   // admit problems next .. next + c - 1 into rows [Bcur, Bcur + c)
      rc = hip(hipMemcpyAsync(q.ID + Bcur, ids.data() + next, sizeof(int32_t) * (size_t)c, hipMemcpyHostToDevice, s), "writing ID");
      if (rc == TOWR_OK) rc = hip(hipMemsetAsync(q.AGE + Bcur, 0, sizeof(int32_t) * (size_t)c, s), "clearing AGE");
      if (rc == TOWR_OK && !q.LAM0 && m > 0)
        rc = hip(hipMemset2DAsync(st.LAM + (int64_t)Bcur * st.ldl, 8 * (size_t)st.ldl, 0, 8 * (size_t)m, (size_t)c, s), "clearing LAM");
      if (rc == TOWR_OK) rc = launch_move_rows(h, q.ID, Bcur, c, n_in, in_slot, in_src, true, s);
      if (rc == TOWR_OK)
        rc = launch_alsolve_init(h, c, *params, state_from_row(st, Bcur, params->mem), row_at(XL, Bcur, ldxb), row_at(XU, Bcur, ldxb),
                                 ldxb, s);
      if (rc != TOWR_OK) break;
      Bcur += c;
      next += c;
    }
    if (Bcur == 0) break;   // (next == N)
    rc = iterate(Bcur, K, ter);
    if (rc == TOWR_OK) rc = launch_retire_key(h, Bcur, st.ISTATE, q.AGE, q.KEY, K, M, s);
    if (rc == TOWR_OK) rc = launch_partition(h, Bcur, q.KEY, LOG, pairs, s);
    if (rc == TOWR_OK) rc = launch_swap_rows(h, LOG + 1, Bcur / 2, pairs, nr, rows, s);
    if (rc == TOWR_OK) rc = hip(hipMemcpyAsync(al.h_head, LOG, 8 * sizeof(int32_t), hipMemcpyDeviceToHost, s), "copying HEAD");
    if (rc == TOWR_OK) rc = hip(hipStreamSynchronize(s), "the round's synchronisation");
    if (rc != TOWR_OK) break;
    ++rounds;
    problem_iters += (int64_t)Bcur * K;
    const int na = al.h_head[0];
    rc = launch_move_rows(h, q.ID, na, Bcur - na, n_out, out_slot, out_dst, false, s);   // rows [na, Bcur) leave
    Bcur = na;
  }
  std::vector<int32_t> is(4 * (size_t)N);
  if (rc == TOWR_OK) rc = hip(hipMemcpyAsync(is.data(), q.ISTATE_OUT, sizeof(int32_t) * is.size(), hipMemcpyDeviceToHost, s), "copying ISTATE_OUT");
  const hipError_t es = hipStreamSynchronize(s);   // (on every path: nothing of this call is in flight at return)
  if (ter) (void)hipFree(ter);
  if (rc != TOWR_OK) return rc;
  if (int r2 = hip(es, "the last synchronisation")) return r2;
  report->rounds = rounds;
  report->iters_run = K * rounds;
  report->problem_iters = problem_iters;
  for (int i = 0; i < N; ++i) {
    const int32_t p = is[4 * (size_t)i];
    ++report->n_phase[p >= 0 && p <= 4 ? p : 5];
    if (stop && p == kAlAcceptable) ++report->reserved[0];
    if (stop && p == kAlInfeasible) ++report->reserved[1];
  }
  return TOWR_OK;
}

extern "C" {

int towr_gpu_alsolve_solve_queue_batch_device(towr_gpu_handle h, int32_t B, const towr_solve_opts_t* opts,
                                              const towr_alsolve_params_t* params, const towr_alsolve_stop_t* stop,
                                              const towr_alsolve_state_t* state, const towr_solve_dir_t* dir,
                                              const towr_solve_queue_t* queue, int32_t* LOG, towr_solve_report_t* report,
                                              void* stream) {
  return alsolve_solve_queue(h, B, opts, params, stop, state, dir, queue, LOG, report, stream);
}

int towr_gpu_alsolve_solve_batch_device(towr_gpu_handle h, int32_t B, const towr_solve_opts_t* opts,
                                        const towr_alsolve_params_t* params, const towr_alsolve_state_t* state,
                                        const towr_solve_dir_t* dir, double* GL, double* GU, int64_t ldgb, double* XL, double* XU,
                                        int64_t ldxb, int32_t* LOG, towr_solve_report_t* report, void* stream) {
  return alsolve_solve(h, B, opts, params, nullptr, state, dir, GL, GU, ldgb, XL, XU, ldxb, LOG, report, stream);
}

int towr_gpu_alsolve_solve_ex_batch_device(towr_gpu_handle h, int32_t B, const towr_solve_opts_t* opts,
                                           const towr_alsolve_params_t* params, const towr_alsolve_stop_t* stop,
                                           const towr_alsolve_state_t* state, const towr_solve_dir_t* dir, double* GL, double* GU,
                                           int64_t ldgb, double* XL, double* XU, int64_t ldxb, int32_t* LOG,
                                           towr_solve_report_t* report, void* stream) {
  return alsolve_solve(h, B, opts, params, stop, state, dir, GL, GU, ldgb, XL, XU, ldxb, LOG, report, stream);
}

int towr_gpu_alsolve_solve_probe_batch_device(towr_gpu_handle h, int32_t B, const towr_solve_opts_t* opts,
                                              const towr_alsolve_params_t* params, const towr_alsolve_stop_t* stop,
                                              const towr_alsolve_probe_t* probe, const towr_alsolve_state_t* state,
                                              const towr_solve_dir_t* dir, double* GL, double* GU, int64_t ldgb, double* XL,
                                              double* XU, int64_t ldxb, double* PSUM, int64_t ldps, int32_t* LOG,
                                              towr_solve_report_t* report, void* stream) {
  return alsolve_solve(h, B, opts, params, stop, state, dir, GL, GU, ldgb, XL, XU, ldxb, LOG, report, stream, probe, PSUM, ldps);
}

int towr_gpu_alsolve_solve_lazy_batch_device(towr_gpu_handle h, int32_t B, const towr_solve_opts_t* opts,
                                             const towr_alsolve_params_t* params, const towr_alsolve_stop_t* stop,
                                             const towr_alsolve_probe_t* probe, const towr_alsolve_state_t* state,
                                             const towr_solve_dir_t* dir, double* GL, double* GU, int64_t ldgb, double* XL,
                                             double* XU, int64_t ldxb, double* PSUM, int64_t ldps, int32_t* LOG,
                                             towr_solve_report_t* report, const towr_alsolve_lazy_t* lazy, void* stream) {
  return alsolve_solve(h, B, opts, params, stop, state, dir, GL, GU, ldgb, XL, XU, ldxb, LOG, report, stream, probe, PSUM, ldps,
                       lazy);
}

}  // extern "C"
