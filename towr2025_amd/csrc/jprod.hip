// jprod.hip — batched Jacobian-vector products on the evaluated CSR values (towr_gpu_jac_vec_batch_device,
// towr_gpu_jac_tvec_batch_device): Y_b = J_b p_b and Z_b (+)= J_b^T lam_b for B problems that share one pattern.
//
// One block per problem. The block keeps the problem's vector in LDS (p: n doubles, lam: m doubles) and walks the
// value array in chunks of kJpChunk consecutive CSR entries (layout.h JpChunk): every lane loads its entries of the
// chunk (coalesced, each value read once, the next chunk's loads in flight while this one is summed), multiplies by
// its vector element and puts the product in the chunk's LDS tile. Then every output with entries in the chunk sums
// its segment of the tile: one lane in ascending order, or one wave for a segment of jp_long entries or more (lane l
// takes entries l, l + 64, ... in order, then a fixed shuffle tree).
//   J p:    segments are row spans; the row cut by a chunk boundary hands its partial on through a carry in LDS;
//   J^T l:  segments are the chunk's columns, read through its by-column list (staged in LDS, rows ascending);
//           the chunk's partial is added to the column's running sum in LDS, chunks in ascending order.
// Every output element is one fixed tree of IEEE additions over exactly its own entries — no atomics, nothing that
// depends on B, the block's place in the grid, the stream or timing — so the bits are a function of the problem alone.
// Behind them: the Gauss-Newton direction (towr_gpu_gn_direction_batch_device, and its Jacobi-preconditioned form
// towr_gpu_gn_direction_pc_batch_device), a whole CG solve per block on the same walk and trees; and the direct
// direction (towr_gpu_gn_direction_direct_batch_device), an envelope Cholesky solve of the same system per block.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "consumer_common.h"
#include "layout.h"

namespace tg {
namespace {

constexpr int kJpPer = kJpChunk / kJpBlock;   // entries per lane and chunk
static_assert(kJpChunk % kJpBlock == 0 && kJpChunk <= 65536, "chunk-local positions are uint16");
static_assert(kJpChunk == 8 * kJpBlock, "a lane stages 8 by-column positions (16 bytes) per chunk");

extern __shared__ __attribute__((aligned(16))) double jp_lds[];

// lane 0 of the wave gets the sum in a fixed order (the other lanes' results are not used)
__device__ inline double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// the sum of segment s of the tile: by the calling lane (WAVE = false) or by its wave (result in lane 0)
template <bool WAVE, bool INDIRECT>
__device__ inline double seg_sum(const JpSeg& s, const double* tile, const uint16_t* cidx) {
  const int q0 = INDIRECT ? (s.q0 & (kJpChunk - 1)) : s.q0;
  double acc = 0.0;
  for (int i = WAVE ? (int)(threadIdx.x & 63) : 0; i < s.len; i += WAVE ? 64 : 1) acc += tile[INDIRECT ? cidx[q0 + i] : q0 + i];
  return WAVE ? wave_sum(acc) : acc;
}

__global__ void __launch_bounds__(kJpBlock) towr_jac_vec_kernel(JpArgs a) {
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  double* p = jp_lds;                       // n (padded to a 16-byte multiple)
  double* tile = p + ((a.n + 1) & ~1);      // kJpChunk products
  double* carry = tile + kJpChunk;          // 2: the row cut by the end of an even / odd chunk
  const double* Vb = a.V + b * a.ldv;
  double* Yb = a.Out + b * a.ldo;
  for (int j = tid; j < a.n; j += kJpBlock) p[j] = a.Vec[b * a.ldvec + j];
  for (int i = tid; i < a.n_empty; i += kJpBlock) Yb[a.empty_rows[i]] = 0.0;
  double v[kJpPer];
  int32_t c[kJpPer];
#pragma unroll
  for (int i = 0; i < kJpPer; ++i) {
    const int64_t k = (int64_t)i * kJpBlock + tid;
    v[i] = 0.0; c[i] = 0;
    if (k < a.nnz) { v[i] = __builtin_nontemporal_load(Vb + k); c[i] = a.col[k]; }
  }
  __syncthreads();
  for (int ci = 0; ci < a.n_chunks; ++ci) {
    const int64_t k0 = (int64_t)ci * kJpChunk;
    const JpChunk ch = a.chunks[ci];
#pragma unroll
    for (int i = 0; i < kJpPer; ++i)
      if (k0 + i * kJpBlock + tid < a.nnz) tile[i * kJpBlock + tid] = v[i] * p[c[i]];
#pragma unroll
    for (int i = 0; i < kJpPer; ++i) {   // the next chunk's values, in flight during the sums below
      const int64_t k = k0 + kJpChunk + (int64_t)i * kJpBlock + tid;
      if (k < a.nnz) { v[i] = __builtin_nontemporal_load(Vb + k); c[i] = a.col[k]; }
    }
    __syncthreads();
    auto finish = [&](const JpSeg& s, double sum) {
      if (s.flags & 1) sum = carry[(ci & 1) ^ 1] + sum;
      if (s.flags & 2) carry[ci & 1] = sum;
      else Yb[s.out] = sum;
    };
    for (int q = tid; q < ch.rns; q += kJpBlock) {
      const JpSeg s = a.rseg[ch.rs0 + q];
      finish(s, seg_sum<false, false>(s, tile, nullptr));
    }
    for (int q = tid >> 6; q < ch.rnl; q += kJpBlock / 64) {
      const JpSeg s = a.rseg[ch.rs0 + ch.rns + q];
      const double sum = seg_sum<true, false>(s, tile, nullptr);
      if ((tid & 63) == 0) finish(s, sum);
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kJpBlock) towr_jac_tvec_kernel(JpArgs a) {
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  double* lam = jp_lds;                        // m (padded)
  double* zacc = lam + ((a.m + 1) & ~1);       // n (padded): the columns' running sums
  double* tile = zacc + ((a.n + 1) & ~1);      // kJpChunk products
  uint16_t* cidx = reinterpret_cast<uint16_t*>(tile + kJpChunk);   // the chunk's by-column list
  const double* Vb = a.V + b * a.ldv;
  double* Zb = a.Out + b * a.ldo;
  for (int i = tid; i < a.m; i += kJpBlock) lam[i] = a.Vec[b * a.ldvec + i];
  for (int j = tid; j < a.n; j += kJpBlock) zacc[j] = 0.0;
  double v[kJpPer];
  int32_t r[kJpPer];
  uint4 cx = make_uint4(0, 0, 0, 0);
#pragma unroll
  for (int i = 0; i < kJpPer; ++i) {
    const int64_t k = (int64_t)i * kJpBlock + tid;
    v[i] = 0.0; r[i] = 0;
    if (k < a.nnz) { v[i] = __builtin_nontemporal_load(Vb + k); r[i] = a.row[k]; }
  }
  if (a.n_chunks > 0) cx = reinterpret_cast<const uint4*>(a.cidx)[tid];   // (the table is padded to whole chunks)
  __syncthreads();
  for (int ci = 0; ci < a.n_chunks; ++ci) {
    const int64_t k0 = (int64_t)ci * kJpChunk;
    const JpChunk ch = a.chunks[ci];
#pragma unroll
    for (int i = 0; i < kJpPer; ++i)
      if (k0 + i * kJpBlock + tid < a.nnz) tile[i * kJpBlock + tid] = v[i] * lam[r[i]];
    reinterpret_cast<uint4*>(cidx)[tid] = cx;
#pragma unroll
    for (int i = 0; i < kJpPer; ++i) {
      const int64_t k = k0 + kJpChunk + (int64_t)i * kJpBlock + tid;
      if (k < a.nnz) { v[i] = __builtin_nontemporal_load(Vb + k); r[i] = a.row[k]; }
    }
    if (ci + 1 < a.n_chunks) cx = reinterpret_cast<const uint4*>(a.cidx + k0 + kJpChunk)[tid];
    __syncthreads();
    for (int q = tid; q < ch.cns; q += kJpBlock) {
      const JpSeg s = a.cseg[ch.cs0 + q];
      zacc[s.out] += seg_sum<false, true>(s, tile, cidx);
    }
    for (int q = tid >> 6; q < ch.cnl; q += kJpBlock / 64) {
      const JpSeg s = a.cseg[ch.cs0 + ch.cns + q];
      const double sum = seg_sum<true, true>(s, tile, cidx);
      if ((tid & 63) == 0) zacc[s.out] += sum;
    }
    __syncthreads();
  }
  // (after the loop's last barrier, or the one before it when there is no chunk)
  for (int j = tid; j < a.n; j += kJpBlock) {
    if (!a.accumulate) Zb[j] = zacc[j];
    else if (a.col_ptr[j + 1] != a.col_ptr[j]) Zb[j] += zacc[j];   // a column without entries keeps its bits
  }
}

// ---- the Gauss-Newton direction (towr_gpu_gn_direction_batch_device) ---------------------------------------------------
// One block of kGnBlock threads per problem (twice the product kernels': the vectors' LDS admits two blocks per CU, and
// 16 waves hide the walk better than 8) stays resident for the whole CG solve on H = rho (J^T W J)_ff + mu I.
// Every step is the J p pass
// and the J^T t pass of the two kernels above over the problem's values — the same chunk walk, tiles, carries and segment
// trees — with the vectors kept in LDS between the passes instead of going through global memory: the first pass
// brings the values from HBM, the later ones find them in the caches (plain loads here, not non-temporal ones).
// Lane l owns columns l, l + kGnBlock, ... for everything that is per column (the held bit, p, r, Hp, d in the D row),
// so those updates need no barrier among themselves; a barrier stands between an update of p and the next J p pass.
// The dot products are block_sums of lbfgs.hip: the lane's partial in column order, a fixed shuffle tree, the waves'
// partials added in wave order by one lane, the scalar broadcast through LDS — every lane takes the stop decisions on
// the same bits. Contraction is off: every product and sum is the plain IEEE expression the header states.
constexpr int kGnPer = kJpChunk / kGnBlock;   // entries per lane and chunk
constexpr int kGnWaves = kGnBlock / 64;
static_assert(kJpChunk % kGnBlock == 0 && (sizeof(uint16_t) * kJpChunk / kGnBlock == 8 || sizeof(uint16_t) * kJpChunk / kGnBlock == 16),
              "a lane stages 4 or 8 by-column positions per chunk");
using GnCx = std::conditional<kGnPer == 4, uint2, uint4>::type;   // the lane's share of a chunk's by-column list

template <int K>
__device__ inline void gn_block_sums(double (&v)[K], double (*s_part)[kGnWaves], double* s_bc, int tid) {
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += __shfl_down(v[k], o, 64);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) s_part[k][tid >> 6] = v[k];
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      double t = s_part[k][0];
      for (int w = 1; w < kGnWaves; ++w) t += s_part[k][w];
      s_bc[k] = t;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = s_bc[k];
}

// A block runs few at a time per CU (its LDS), so the walk's dependent table loads are not hidden by other blocks as
// in the product kernels: the chunk descriptors are read two chunks ahead and lane tid's first short segment and its
// wave's first long one a chunk ahead (the sums and their order are unchanged).
struct GnSegs { JpSeg s, l; };
__device__ inline GnSegs gn_fetch(const JpSeg* seg, int s0, int ns, int nl, int tid) {
  GnSegs f{};
  if (tid < ns) f.s = seg[s0 + tid];
  if ((tid >> 6) < nl) f.l = seg[s0 + ns + (tid >> 6)];
  return f;
}

// t = w .* (J p): towr_jac_vec_kernel's walk with p in LDS and the row's sum scaled by its weight into t (LDS). The
// caller's barrier stands before it (p complete, the tile free); it ends behind its own last barrier.
__device__ inline void gn_jp_pass(const JpArgs& a, const double* Vb, const double* p, double* tile, double* carry, double* t,
                                  const uint8_t* act, int tid) {
#pragma clang fp contract(off)
  double v[kGnPer];
  int32_t c[kGnPer];
#pragma unroll
  for (int i = 0; i < kGnPer; ++i) {
    const int64_t k = (int64_t)i * kGnBlock + tid;
    v[i] = 0.0; c[i] = 0;
    if (k < a.nnz) { v[i] = Vb[k]; c[i] = a.col[k]; }
  }
  const JpChunk none{};
  JpChunk ch = a.n_chunks > 0 ? a.chunks[0] : none, nx = a.n_chunks > 1 ? a.chunks[1] : none;
  GnSegs cur = gn_fetch(a.rseg, ch.rs0, ch.rns, ch.rnl, tid);
  for (int ci = 0; ci < a.n_chunks; ++ci) {
    const int64_t k0 = (int64_t)ci * kJpChunk;
#pragma unroll
    for (int i = 0; i < kGnPer; ++i)
      if (k0 + i * kGnBlock + tid < a.nnz) tile[i * kGnBlock + tid] = v[i] * p[c[i]];
#pragma unroll
    for (int i = 0; i < kGnPer; ++i) {
      const int64_t k = k0 + kJpChunk + (int64_t)i * kGnBlock + tid;
      if (k < a.nnz) { v[i] = Vb[k]; c[i] = a.col[k]; }
    }
    const JpChunk n2 = ci + 2 < a.n_chunks ? a.chunks[ci + 2] : none;
    const GnSegs nxt = gn_fetch(a.rseg, nx.rs0, nx.rns, nx.rnl, tid);   // (no chunk: no segments, nothing is read)
    __syncthreads();
    auto finish = [&](const JpSeg& s, double sum) {
      if (s.flags & 1) sum = carry[(ci & 1) ^ 1] + sum;
      if (s.flags & 2) carry[ci & 1] = sum;
      else t[s.out] = (act[s.out] ? 1.0 : 0.0) * sum;
    };
    for (int q = tid; q < ch.rns; q += kGnBlock) {
      const JpSeg s = q == tid ? cur.s : a.rseg[ch.rs0 + q];
      finish(s, seg_sum<false, false>(s, tile, nullptr));
    }
    for (int q = tid >> 6; q < ch.rnl; q += kGnBlock / 64) {
      const JpSeg s = q == (tid >> 6) ? cur.l : a.rseg[ch.rs0 + ch.rns + q];
      const double sum = seg_sum<true, false>(s, tile, nullptr);
      if ((tid & 63) == 0) finish(s, sum);
    }
    __syncthreads();
    ch = nx; nx = n2; cur = nxt;
  }
}

// z += J^T t: towr_jac_tvec_kernel's walk with t and the columns' running sums z in LDS (z zeroed by the caller, before
// a barrier). Ends behind its own last barrier. DIAG: the same walk with the tile filled by w_i * (v * v) (w from act;
// t is not read): z += diag(J^T W J), on the sums towr_jac_tvec_kernel would form on the squared values.
template <bool DIAG>
__device__ inline void gn_jtt_pass(const JpArgs& a, const double* Vb, const double* t, double* z, double* tile, uint16_t* cidx,
                                   const uint8_t* act, int tid) {
#pragma clang fp contract(off)
  double v[kGnPer];
  int32_t r[kGnPer];
  GnCx cx{};
#pragma unroll
  for (int i = 0; i < kGnPer; ++i) {
    const int64_t k = (int64_t)i * kGnBlock + tid;
    v[i] = 0.0; r[i] = 0;
    if (k < a.nnz) { v[i] = Vb[k]; r[i] = a.row[k]; }
  }
  if (a.n_chunks > 0) cx = reinterpret_cast<const GnCx*>(a.cidx)[tid];
  const JpChunk none{};
  JpChunk ch = a.n_chunks > 0 ? a.chunks[0] : none, nx = a.n_chunks > 1 ? a.chunks[1] : none;
  GnSegs cur = gn_fetch(a.cseg, ch.cs0, ch.cns, ch.cnl, tid);
  for (int ci = 0; ci < a.n_chunks; ++ci) {
    const int64_t k0 = (int64_t)ci * kJpChunk;
#pragma unroll
    for (int i = 0; i < kGnPer; ++i)
      if (k0 + i * kGnBlock + tid < a.nnz) {
        if (DIAG) tile[i * kGnBlock + tid] = (act[r[i]] ? 1.0 : 0.0) * (v[i] * v[i]);
        else tile[i * kGnBlock + tid] = v[i] * t[r[i]];
      }
    reinterpret_cast<GnCx*>(cidx)[tid] = cx;
#pragma unroll
    for (int i = 0; i < kGnPer; ++i) {
      const int64_t k = k0 + kJpChunk + (int64_t)i * kGnBlock + tid;
      if (k < a.nnz) { v[i] = Vb[k]; r[i] = a.row[k]; }
    }
    if (ci + 1 < a.n_chunks) cx = reinterpret_cast<const GnCx*>(a.cidx + k0 + kJpChunk)[tid];
    const JpChunk n2 = ci + 2 < a.n_chunks ? a.chunks[ci + 2] : none;
    const GnSegs nxt = gn_fetch(a.cseg, nx.cs0, nx.cns, nx.cnl, tid);
    __syncthreads();
    for (int q = tid; q < ch.cns; q += kGnBlock) {
      const JpSeg s = q == tid ? cur.s : a.cseg[ch.cs0 + q];
      z[s.out] += seg_sum<false, true>(s, tile, cidx);
    }
    for (int q = tid >> 6; q < ch.cnl; q += kGnBlock / 64) {
      const JpSeg s = q == (tid >> 6) ? cur.l : a.cseg[ch.cs0 + ch.cns + q];
      const double sum = seg_sum<true, true>(s, tile, cidx);
      if ((tid & 63) == 0) z[s.out] += sum;
    }
    __syncthreads();
    ch = nx; nx = n2; cur = nxt;
  }
}

// PCG: the Jacobi-preconditioned recursion of towr_gpu_gn_direction_pc_batch_device. M = rho diag(J^T W J) + mu (1.0
// where that is exactly 0) lives in the problem's PC row as d lives in D: the lane that owns a column writes and reads
// it. z = r ./ M is formed where r is updated and kept in the column accumulator (free between the passes) for the
// update of p behind the sums; rn and rzn share one block_sums, so a step has the barriers of the plain one.
template <bool PCG>
__device__ __forceinline__ void gn_direction_body(const GnArgs& a) {
#pragma clang fp contract(off)
  __shared__ double s_part[2][kGnWaves], s_bc[2];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  if (a.RUN && a.RUN[b * a.run_stride] >= 2) return;   // (block-uniform: before any barrier)
  const JpArgs& T = a.jp;
  const int n = T.n, m = T.m;
  const int n2 = (n + 1) & ~1, m2 = (m + 1) & ~1;
  double* p = jp_lds;                 // n (padded): 0 on held columns
  double* r = p + n2;                 // n
  double* z = r + n2;                 // n: the columns' running sums of J^T t, then H p
  double* t = z + n2;                 // m
  double* tile = t + m2;              // kJpChunk products
  double* carry = tile + kJpChunk;    // 2
  uint16_t* cidx = reinterpret_cast<uint16_t*>(carry + 2);   // the chunk's by-column list (16-byte aligned)
  uint8_t* act = reinterpret_cast<uint8_t*>(cidx + kJpChunk);   // m: the row is active (w = 1)
  const double* Vb = a.V + b * a.ldv;
  const double* Gb = a.GR + b * a.ldgr;
  const double* LPb = a.LAMP + b * a.ldlp;
  double* Db = a.D + b * a.ldd;
  double* PCb = PCG ? a.PC + b * a.ldpc : nullptr;
  const double rho = a.RHO ? a.RHO[b] : a.rho;
  const double mu = a.mu;
  const double tol2 = a.tol * a.tol;

  // the held mask (bit k: the lane's k-th column), r = p = g on free columns, bb = sum_free g^2
  unsigned held = 0u;
  double v2[2] = {0.0, 0.0};   // bb, the held count (integers below 2^53: exact in any order)
  {
    const double* Xb = a.X ? a.X + b * a.ldx : nullptr;
    const double* Lb = a.X ? a.XL + b * a.ldb : nullptr;
    const double* Ub = a.X ? a.XU + b * a.ldb : nullptr;
    int k = 0;
    for (int j = tid; j < n; j += kGnBlock, ++k) {
      const double g = Gb[j];
      bool h = false;
      if (Xb) {
        const double x = Xb[j], l = Lb[j], u = Ub[j];
        const bool has_l = l > -kSideInf, has_u = u < kSideInf;
        h = (has_l && x <= l && g > 0.0) || (has_u && x >= u && g < 0.0) || (has_l && has_u && l == u);
      }
      if (h) {
        held |= 1u << k;
        v2[1] += 1.0;
        p[j] = 0.0;
        r[j] = 0.0;
      } else {
        v2[0] += g * g;
        p[j] = g;
        r[j] = g;
      }
      if (PCG) z[j] = 0.0;
    }
  }
  for (int i = tid; i < m; i += kGnBlock) act[i] = LPb[i] != 0.0;   // (a NaN is active)
  for (int i = tid; i < T.n_empty; i += kGnBlock) t[T.empty_rows[i]] = 0.0;   // rows without entries: never written again
  gn_block_sums<2>(v2, s_part, s_bc, tid);   // (its barriers: p, act and t are complete)
  const double bb = v2[0], nheld = v2[1];

  // the diagonal on the J^T t walk, M into the PC row, z = r ./ M, p = z, rz = sum_free r z
  double rz = 0.0, nzero = 0.0;
  if (PCG) {
    gn_jtt_pass<true>(T, Vb, nullptr, z, tile, cidx, act, tid);
    double v3[2] = {0.0, 0.0};   // rz, the replaced count (exact)
    int k = 0;
    for (int j = tid; j < n; j += kGnBlock, ++k) {
      if ((held >> k) & 1u) { PCb[j] = 0.0; continue; }
      double mj = rho * z[j] + mu;
      if (mj == 0.0) { mj = 1.0; v3[1] += 1.0; }
      PCb[j] = mj;
      const double rj = r[j], zj = rj / mj;
      p[j] = zj;
      v3[0] += rj * zj;
    }
    gn_block_sums<2>(v3, s_part, s_bc, tid);   // (its barriers: p is complete)
    rz = v3[0]; nzero = v3[1];
  }

  double rr = bb;
  int steps = 0, code = 0;
  if (bb == 0.0) code = 3;
  else {
    for (int it = 0; it < a.ncg; ++it) {
      if (rr <= tol2 * bb) { code = 1; break; }   // (a NaN goes on to the curvature test, which ends on it)
      for (int j = tid; j < n; j += kGnBlock) z[j] = 0.0;
      gn_jp_pass(T, Vb, p, tile, carry, t, act, tid);
      __syncthreads();   // (also without a chunk: z is zero before the sums below)
      gn_jtt_pass<false>(T, Vb, t, z, tile, cidx, act, tid);
      double s1[1] = {0.0};   // sum_free p Hp
      int k = 0;
      for (int j = tid; j < n; j += kGnBlock, ++k) {
        double hp = 0.0;
        if (!((held >> k) & 1u)) {
          const double pj = p[j];
          hp = rho * z[j] + mu * pj;
          s1[0] += pj * hp;
        }
        z[j] = hp;
      }
      gn_block_sums<1>(s1, s_part, s_bc, tid);
      if (!(s1[0] > 0.0)) { code = 2; break; }   // (a NaN anywhere ends here)
      const double al = (PCG ? rz : rr) / s1[0];
      double s2[PCG ? 2 : 1] = {};   // sum_free r r (and sum_free r z)
      k = 0;
      for (int j = tid; j < n; j += kGnBlock, ++k) {
        if ((held >> k) & 1u) continue;
        const double d0 = steps ? Db[j] : 0.0;
        Db[j] = d0 + al * p[j];
        const double rj = r[j] - al * z[j];
        r[j] = rj;
        s2[0] += rj * rj;
        if (PCG) {
          const double zj = rj / PCb[j];
          z[j] = zj;
          s2[PCG ? 1 : 0] += rj * zj;
        }
      }
      gn_block_sums<PCG ? 2 : 1>(s2, s_part, s_bc, tid);
      const double beta = PCG ? s2[PCG ? 1 : 0] / rz : s2[0] / rr;
      k = 0;
      for (int j = tid; j < n; j += kGnBlock, ++k)
        if (!((held >> k) & 1u)) p[j] = (PCG ? z[j] : r[j]) + beta * p[j];
      if (PCG) rz = s2[PCG ? 1 : 0];
      rr = s2[0];
      ++steps;
      __syncthreads();   // p is complete before the next pass reads it
    }
  }

  // D on the held columns (or everywhere when no step completed) and the slope sum g D over all columns
  double w[1] = {0.0};
  {
    int k = 0;
    for (int j = tid; j < n; j += kGnBlock, ++k) {
      const double g = Gb[j];
      double d = g;
      if (steps && !((held >> k) & 1u)) d = Db[j];
      else Db[j] = g;
      w[0] += g * d;
    }
  }
  gn_block_sums<1>(w, s_part, s_bc, tid);
  if (tid == 0) {
    double* Sb = a.SUM + b * a.lds;
    Sb[0] = (double)steps;
    Sb[1] = bb;
    Sb[2] = rr;
    Sb[3] = w[0];
    Sb[4] = nheld;
    Sb[5] = (double)code;
    if (PCG) { Sb[6] = rz; Sb[7] = nzero; }
  }
}

__global__ void __launch_bounds__(kGnBlock) towr_gn_direction_kernel(GnArgs a) { gn_direction_body<false>(a); }
__global__ void __launch_bounds__(kGnBlock) towr_gn_direction_pc_kernel(GnArgs a) { gn_direction_body<true>(a); }

// ---- the direct Gauss-Newton direction (towr_gpu_gn_direction_direct_batch_device) -----------------------------------
// One block of kGnBlock threads per problem, resident for the assembly, the factorisation and both solves. L lives in
// the problem's workspace row in global memory (the envelope in permuted order, row by row, the diagonal last in its
// row); per permuted column the running sums (sum_k L_qk^2, sum_k L_qk y_k), y and the diagonal of L live in LDS.
//   assembly: one lane per envelope entry merges the two columns' sorted by-column row lists, rows ascending;
//   factorisation, columns ascending: the pivot row's segment is staged in LDS (double-buffered: the segment of column
//   c + 1 is staged during column c, its last entry put there by the lane that computes it), every lane forms the pivot
//   and y_c on the same bits, lanes are spread over the rows r > c whose envelope reaches c; one barrier per column.
//   The forward solve rides on it (y_c is known when column c starts; the lane of row r adds L_rc y_c to the row's sum);
//   the backward solve, columns descending: d_c on the same bits in every lane, lanes spread over row c of L (contiguous
//   in the workspace), each adding L_ck d_c to the running sum of column k; one barrier per column.
// Every sum has one fixed order (ascending k in the factorisation and the forward solve, descending row in the backward
// solve, ascending row in the assembly), so the stop decision (the first pivot that is not > 0) is block-uniform.
__global__ void __launch_bounds__(kGnBlock) towr_gn_direct_kernel(GnDirectArgs a) {
#pragma clang fp contract(off)
  __shared__ double s_part[2][kGnWaves], s_bc[2];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  if (a.RUN && a.RUN[b * a.run_stride] >= 2) return;   // (block-uniform: before any barrier)
  const int n = a.n, m = a.m;
  const int n2 = (n + 1) & ~1, w2 = (a.width + 2) & ~1;
  double* dsum = jp_lds;          // n: sum_k L_qk^2 so far; in the backward solve sum_r L_rq d_r so far
  double* zacc = dsum + n2;       // n: sum_k L_qk y_k so far
  double* y = zacc + n2;          // n
  double* diag = y + n2;          // n: L_qq
  double* seg = diag + n2;        // 2 w2: the pivot rows of an even / odd column
  uint8_t* act = reinterpret_cast<uint8_t*>(seg + 2 * w2);   // m: the row is active (w = 1)
  uint8_t* heldq = act + ((m + 15) & ~15);                    // n: the column at permuted position q is held
  const double* Vb = a.V + b * a.ldv;
  const double* Gb = a.GR + b * a.ldgr;
  const double* LPb = a.LAMP + b * a.ldlp;
  double* Db = a.D + b * a.ldd;
  double* Lb = a.W + b * a.ldw;
  const double rho = a.RHO ? a.RHO[b] : a.rho;
  const double mu = a.mu;

  // the held columns (lbfgs.hip's rule) by permuted position, bb = sum_free g^2
  double v2[2] = {0.0, 0.0};   // bb, the held count (exact)
  {
    const double* Xb = a.X ? a.X + b * a.ldx : nullptr;
    const double* Lo = a.X ? a.XL + b * a.ldb : nullptr;
    const double* Up = a.X ? a.XU + b * a.ldb : nullptr;
    for (int j = tid; j < n; j += kGnBlock) {
      const double g = Gb[j];
      bool h = false;
      if (Xb) {
        const double x = Xb[j], l = Lo[j], u = Up[j];
        const bool has_l = l > -kSideInf, has_u = u < kSideInf;
        h = (has_l && x <= l && g > 0.0) || (has_u && x >= u && g < 0.0) || (has_l && has_u && l == u);
      }
      heldq[a.pos[j]] = h;
      if (h) v2[1] += 1.0;
      else v2[0] += g * g;
      dsum[j] = 0.0;
      zacc[j] = 0.0;
    }
  }
  for (int i = tid; i < m; i += kGnBlock) act[i] = LPb[i] != 0.0;   // (a NaN is active)
  gn_block_sums<2>(v2, s_part, s_bc, tid);   // (its barriers: heldq, act and the running sums are complete)
  const double bb = v2[0], nheld = v2[1];

  int code = 1, bcol = -1;
  double pmin = __builtin_inf(), pmax = 0.0;
  if (bb == 0.0) code = 3;
  else {
    // assembly: entry e of the envelope is (q, c), c <= q; lane tid takes e = tid, tid + kGnBlock, ...
    int q = 0;
    for (int e = tid; e < a.env; e += kGnBlock) {
      while (a.row_off[q + 1] <= e) ++q;
      const int c = a.first[q] + (e - a.row_off[q]);
      double val;
      if (heldq[q] | heldq[c]) val = q == c ? 1.0 : 0.0;
      else {
        const int j = a.inv[q], k = a.inv[c];
        int pa = a.col_ptr[j], pb = a.col_ptr[k];
        const int ea = a.col_ptr[j + 1], eb = a.col_ptr[k + 1];
        double acc = 0.0;
        bool any = false;
        if (pa < ea && pb < eb) {
          int ra = a.csc_row[pa], rb = a.csc_row[pb];
          for (;;) {
            if (ra == rb) {
              const double t = Vb[a.csc_index[pa]] * Vb[a.csc_index[pb]];
              acc += (act[ra] ? 1.0 : 0.0) * t;
              any = true;
              ++pa; ++pb;
              if (pa >= ea || pb >= eb) break;
              ra = a.csc_row[pa]; rb = a.csc_row[pb];
            } else if (ra < rb) {
              if (++pa >= ea) break;
              ra = a.csc_row[pa];
            } else {
              if (++pb >= eb) break;
              rb = a.csc_row[pb];
            }
          }
        }
        if (q == c) val = rho * acc + mu;
        else val = any ? rho * acc : 0.0;   // (no shared row: +0.0 as it stands)
      }
      Lb[e] = val;
    }
    __syncthreads();

    // factorisation and forward solve, columns ascending
    for (int c = 0; c < n; ++c) {
      const double* buf = seg + (c & 1) * w2;
      double* nbuf = seg + ((c + 1) & 1) * w2;
      const int f = a.first[c];
      const double piv = Lb[a.row_off[c + 1] - 1] - dsum[c];
      if (!(piv > 0.0)) { code = 2; bcol = c; break; }   // (a NaN too; block-uniform, before this column's barrier)
      if (!heldq[c]) {
        if (piv < pmin) pmin = piv;
        if (piv > pmax) pmax = piv;
      }
      const double lcc = __builtin_sqrt(piv);
      const double yc = (Gb[a.inv[c]] - zacc[c]) / lcc;
      if (tid == 0) { diag[c] = lcc; y[c] = yc; }
      int f1 = 0;
      if (c + 1 < n) {   // the next pivot row's entries left of c are final: stage them
        f1 = a.first[c + 1];
        const double* Ln = Lb + a.row_off[c + 1] - f1;
        for (int k = f1 + tid; k < c; k += kGnBlock) nbuf[k - f1] = Ln[k];
      }
      const int lastc = a.last[c];
      for (int r = c + 1 + tid; r <= lastc; r += kGnBlock) {
        const int fr = a.first[r];
        if (fr > c) continue;
        double* Lr = Lb + a.row_off[r] - fr;   // Lr[k] = L_rk
        double s = 0.0;
        for (int k = fr > f ? fr : f; k < c; ++k) s += Lr[k] * buf[k - f];
        const double l = (Lr[c] - s) / lcc;
        Lr[c] = l;
        dsum[r] += l * l;
        zacc[r] += l * yc;
        if (r == c + 1) nbuf[c - f1] = l;
      }
      __syncthreads();
    }

    // backward solve, columns descending: d_c = (y_c - sum_{r > c} L_rc d_r) / L_cc, the sum in descending r
    if (code == 1) {
      for (int j = tid; j < n; j += kGnBlock) dsum[j] = 0.0;
      __syncthreads();
      for (int c = n - 1; c >= 0; --c) {
        const double dc = (y[c] - dsum[c]) / diag[c];
        const int f = a.first[c];
        const double* Lc = Lb + a.row_off[c] - f;
        for (int k = f + tid; k < c; k += kGnBlock) dsum[k] += Lc[k] * dc;
        if (tid == 0 && !heldq[c]) Db[a.inv[c]] = dc;
        __syncthreads();
      }
    }
  }

  // D on the held columns (or everywhere unless solved) and the slope sum g D over all columns
  double w[1] = {0.0};
  for (int j = tid; j < n; j += kGnBlock) {
    const double g = Gb[j];
    double d = g;
    if (code == 1 && !heldq[a.pos[j]]) d = Db[j];
    else Db[j] = g;
    w[0] += g * d;
  }
  gn_block_sums<1>(w, s_part, s_bc, tid);
  if (tid == 0) {
    double* Sb = a.SUM + b * a.lds;
    Sb[0] = code == 1 ? 1.0 : 0.0;
    Sb[1] = bb;
    Sb[2] = pmin == __builtin_inf() ? 0.0 : pmin;
    Sb[3] = w[0];
    Sb[4] = nheld;
    Sb[5] = (double)code;
    Sb[6] = pmax;
    Sb[7] = (double)bcol;
  }
}

// ---- the tiled direct Gauss-Newton direction (towr_gpu_gn_direction_tiled_batch_device) ------------------------------
// The direct direction's system, held rule and summary, factorised as a block Cholesky on 16 x 16 tiles inside the tile
// envelope (layout.h GnTiledArgs: the tiles block row by block row in the workspace row, a tile column-major, so that
// lane l of a wave reads double 64 kk + l of a tile as its operand of the kk-th v_mfma_f64_16x16x4_f64 of a tile product
// and holds doubles 64 i + l of the result tile in its accumulator: every tile access of a wave is 512 contiguous bytes).
//   assembly: one lane per stored entry sums the entry's terms — the rows the direct kernel's merge of the two columns'
//   lists finds, in its order, listed once per handle (GnAsmTerm), so the loads of a sum do not depend on one another;
//   factorisation, left-looking by block column J, two barriers per block column:
//     wave 0 forms H_JJ - sum_K L_JK L_JK^T, takes the tile's rows into registers (lane r: row r) and factorises it
//     unblocked by shuffles, the forward solve of the block's 16 unknowns riding on it (sum_K L_JK y_K is formed on the
//     operands the tile products load); waves 1 .. 7 form H_IJ - sum_K L_IK L_JK^T for the rows I > J that reach J, a
//     tile per wave at a time; barrier; the stop decision on a word of LDS every lane reads; one lane per row of the
//     panel solves it against L_JJ^T (in LDS); barrier;
//   backward solve, block columns descending: wave 0 solves L_JJ^T d_J = y_J - acc_J by shuffles; barrier; one lane per
//   column of block row J's tiles adds L_JK^T d_J to acc_K; barrier.
// The summation order is the header's (towr_gpu_gn_direction_tiled_batch_device); nothing depends on B, the block's
// place, the stream or timing.
typedef double gn_v4f64 __attribute__((ext_vector_type(4)));

// acc - A B^T on two tiles' operands of this lane (a: the tile that gives the result's columns, b: its rows)
__device__ __forceinline__ gn_v4f64 gn_tile_msub(gn_v4f64 acc, const double (&va)[4], const double (&vb)[4]) {
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-va[kk], vb[kk], acc, 0, 0, 0);
  return acc;
}

// (4 waves per SIMD asked for: within 128 registers two blocks share a CU)
__global__ void __launch_bounds__(kGnBlock, 4) towr_gn_tiled_kernel(GnTiledArgs a) {
#pragma clang fp contract(off)
  __shared__ double s_part[2][kGnWaves], s_bc[2];
  __shared__ int s_bad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  if (a.RUN && a.RUN[b * a.run_stride] >= 2) return;   // (block-uniform: before any barrier)
  const int n = a.n, m = a.m, nt = a.nt, np = kGnTile * nt;
  double* y = jp_lds;            // 16 nt: g~ by permuted position, then y, then d~ (0 in the padding)
  double* bacc = y + np;         // 16 nt: the backward solve's sum_r L_rq d_r so far
  double* sL = bacc + np;        // 256: L_JJ, column-major
  uint8_t* act = reinterpret_cast<uint8_t*>(sL + 256);   // m: the row is active (w = 1)
  uint8_t* heldq = act + ((m + 15) & ~15);                // 16 nt: 1 held, 0 free, 2 padding
  const double* Vb = a.V + b * a.ldv;
  const double* Gb = a.GR + b * a.ldgr;
  const double* LPb = a.LAMP + b * a.ldlp;
  double* Db = a.D + b * a.ldd;
  double* Lb = a.W + b * a.ldw;
  const double rho = a.RHO ? a.RHO[b] : a.rho;
  const double mu = a.mu;

  // the held columns (lbfgs.hip's rule) by permuted position, bb = sum_free g^2 (the direct kernel's sums)
  double v2[2] = {0.0, 0.0};   // bb, the held count (exact)
  {
    const double* Xb = a.X ? a.X + b * a.ldx : nullptr;
    const double* Lo = a.X ? a.XL + b * a.ldb : nullptr;
    const double* Up = a.X ? a.XU + b * a.ldb : nullptr;
    for (int j = tid; j < n; j += kGnBlock) {
      const double g = Gb[j];
      bool h = false;
      if (Xb) {
        const double x = Xb[j], l = Lo[j], u = Up[j];
        const bool has_l = l > -kSideInf, has_u = u < kSideInf;
        h = (has_l && x <= l && g > 0.0) || (has_u && x >= u && g < 0.0) || (has_l && has_u && l == u);
      }
      const int q = a.pos[j];
      heldq[q] = h;
      y[q] = g;
      bacc[q] = 0.0;
      if (h) v2[1] += 1.0;
      else v2[0] += g * g;
    }
    for (int q = n + tid; q < np; q += kGnBlock) { heldq[q] = 2; y[q] = 0.0; bacc[q] = 0.0; }
  }
  for (int i = tid; i < m; i += kGnBlock) act[i] = LPb[i] != 0.0;   // (a NaN is active)
  gn_block_sums<2>(v2, s_part, s_bc, tid);   // (its barriers: heldq, act, y and bacc are complete)
  const double bb = v2[0], nheld = v2[1];

  int code = 1, bcol = -1;
  double pmin = __builtin_inf(), pmax = 0.0;   // (kept by wave 0, every lane of it on the same bits)
  if (bb == 0.0) code = 3;
  else {
    // assembly: stored entry e is entry (r, c) = (e & 15, (e >> 4) & 15) of stored tile e >> 8
    {
      int I = 0;
      const int total = 256 * a.tiles;
      for (int e = tid; e < total; e += kGnBlock) {
        const int t = e >> 8;
        while (a.tile_off[I + 1] <= t) ++I;
        const int q = kGnTile * I + (e & 15), c = kGnTile * (a.bfirst[I] + (t - a.tile_off[I])) + ((e >> 4) & 15);
        double val;
        if (c > q) val = 0.0;   // (above the diagonal: not read for a result)
        else if (heldq[q] | heldq[c]) val = q == c ? 1.0 : 0.0;
        else {
          const int p0 = a.asm_ptr[e], p1 = a.asm_ptr[e + 1];
          double acc = 0.0;
          for (int p = p0; p < p1; ++p) {
            const GnAsmTerm t = a.asm_terms[p];
            const double vv = Vb[t.a] * Vb[t.b];
            acc += (act[t.row] ? 1.0 : 0.0) * vv;
          }
          if (q == c) val = rho * acc + mu;
          else val = p1 > p0 ? rho * acc : 0.0;   // (no shared row: +0.0 as it stands)
        }
        Lb[e] = val;
      }
    }
    __syncthreads();

    // factorisation and forward solve, block columns ascending
    for (int J = 0; J < nt; ++J) {
      const int bfJ = a.bfirst[J];
      double* rowJ = Lb + 256 * a.tile_off[J];   // tile (J, K) at rowJ + 256 (K - bfJ)
      const int cp0 = a.tcol_ptr[J], cnt = a.tcol_ptr[J + 1] - cp0;
      if (wave == 0) {
        double* T = rowJ + 256 * (J - bfJ);
        gn_v4f64 acc;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = T[64 * i + lane];
        double s = 0.0;   // this lane's share of sum_K L_JK y_K for row lane & 15: the k = 4 kk + (lane >> 4)
        for (int K = bfJ; K < J; ++K) {
          const double* A = rowJ + 256 * (K - bfJ);
          double va[4];
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) va[kk] = A[64 * kk + lane];
          acc = gn_tile_msub(acc, va, va);
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) s += va[kk] * y[kGnTile * K + 4 * kk + (lane >> 4)];
        }
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        // row r = lane & 15 of the tile into registers: entry (r, c) is accumulator c >> 2 of lane r + 16 (c & 3)
        const int r = lane & 15;
        double row[kGnTile];
#pragma unroll
        for (int c = 0; c < kGnTile; ++c) row[c] = __shfl(acc[c >> 2], r + 16 * (c & 3), 64);
        double t = y[kGnTile * J + r] - s;
        int badk = -1;
#pragma unroll
        for (int k = 0; k < kGnTile; ++k) {
          __builtin_amdgcn_sched_barrier(0);   // (one step's shuffles at a time: the rows stay in registers)
          if (badk < 0) {   // (wave-uniform)
            const double piv = __shfl(row[k], k, 64);
            if (!(piv > 0.0)) badk = k;   // (a NaN too)
            else {
              if (!heldq[kGnTile * J + k]) {
                if (piv < pmin) pmin = piv;
                if (piv > pmax) pmax = piv;
              }
              const double l = __builtin_sqrt(piv);
              row[k] = r == k ? l : row[k] / l;
              const double yk = __shfl(t, k, 64) / l;
              if (r == k) t = yk;
              else if (r > k) t -= row[k] * yk;
#pragma unroll
              for (int c = k + 1; c < kGnTile; ++c) row[c] -= row[k] * __shfl(row[k], c, 64);
            }
          }
        }
        if (lane < kGnTile) {
#pragma unroll
          for (int c = 0; c < kGnTile; ++c) {
            const double v = c <= r ? row[c] : 0.0;
            sL[kGnTile * c + r] = v;
            T[kGnTile * c + r] = v;
          }
          y[kGnTile * J + r] = t;
        }
        if (lane == 0) s_bad = badk;
      } else {
        for (int i = wave - 1; i < cnt; i += kGnWaves - 1) {
          const int I = a.tcol_rows[cp0 + i];
          const int bfI = a.bfirst[I];
          double* rowI = Lb + 256 * a.tile_off[I];
          double* T = rowI + 256 * (J - bfI);
          gn_v4f64 acc;
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] = T[64 * k + lane];
          for (int K = bfI > bfJ ? bfI : bfJ; K < J; ++K) {
            const double* A = rowJ + 256 * (K - bfJ);
            const double* Bt = rowI + 256 * (K - bfI);
            double va[4], vb[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) { va[kk] = A[64 * kk + lane]; vb[kk] = Bt[64 * kk + lane]; }
            acc = gn_tile_msub(acc, va, vb);
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) T[64 * k + lane] = acc[k];
        }
      }
      __syncthreads();
      const int bad = s_bad;   // (block-uniform: written before the barrier, next after the one below)
      if (bad >= 0) { code = 2; bcol = kGnTile * J + bad; break; }
      // the panel: row p & 15 of tile p >> 4 of the block column, X L_JJ^T = A by columns ascending
      for (int p = tid; p < kGnTile * cnt; p += kGnBlock) {
        const int I = a.tcol_rows[cp0 + (p >> 4)];
        double* T = Lb + 256 * (a.tile_off[I] + J - a.bfirst[I]) + (p & 15);
        double x[kGnTile];
#pragma unroll
        for (int c = 0; c < kGnTile; ++c) x[c] = T[kGnTile * c];
#pragma unroll
        for (int c = 0; c < kGnTile; ++c) {
          __builtin_amdgcn_sched_barrier(0);   // (one column's reads of L_JJ at a time)
          double s = x[c];
#pragma unroll
          for (int k = 0; k < c; ++k) s -= x[k] * sL[kGnTile * k + c];
          x[c] = s / sL[(kGnTile + 1) * c];
        }
#pragma unroll
        for (int c = 0; c < kGnTile; ++c) T[kGnTile * c] = x[c];
      }
      __syncthreads();
    }

    // backward solve, block columns descending
    if (code == 1) {
      for (int J = nt - 1; J >= 0; --J) {
        const int bfJ = a.bfirst[J];
        const double* rowJ = Lb + 256 * a.tile_off[J];
        if (wave == 0) {
          const int c = lane & 15;
          const double* T = rowJ + 256 * (J - bfJ) + kGnTile * c;   // column c of L_JJ
          double col[kGnTile];
#pragma unroll
          for (int k = 0; k < kGnTile; ++k) col[k] = T[k];
          double t = y[kGnTile * J + c] - bacc[kGnTile * J + c];
#pragma unroll
          for (int k = kGnTile - 1; k >= 0; --k) {
            __builtin_amdgcn_sched_barrier(0);
            const double dk = __shfl(t, k, 64) / __shfl(col[k], k, 64);
            if (c == k) t = dk;
            else if (c < k) t -= col[k] * dk;
          }
          if (lane < kGnTile) {
            const int q = kGnTile * J + c;
            y[q] = t;
            if (q < n && !heldq[q]) Db[a.inv[q]] = t;
          }
        }
        __syncthreads();
        for (int p = tid; p < kGnTile * (J - bfJ); p += kGnBlock) {   // column p & 15 of tile (J, bfJ + (p >> 4))
          const double* T = rowJ + kGnTile * p;
          double s = 0.0;
#pragma unroll
          for (int r = kGnTile - 1; r >= 0; --r) s += T[r] * y[kGnTile * J + r];
          bacc[kGnTile * bfJ + p] += s;
        }
        __syncthreads();
      }
    }
  }

  // D on the held columns (or everywhere unless solved) and the slope sum g D over all columns
  double w[1] = {0.0};
  for (int j = tid; j < n; j += kGnBlock) {
    const double g = Gb[j];
    double d = g;
    if (code == 1 && heldq[a.pos[j]] == 0) d = Db[j];
    else Db[j] = g;
    w[0] += g * d;
  }
  gn_block_sums<1>(w, s_part, s_bc, tid);
  if (tid == 0) {
    double* Sb = a.SUM + b * a.lds;
    Sb[0] = code == 1 ? 1.0 : 0.0;
    Sb[1] = bb;
    Sb[2] = pmin == __builtin_inf() ? 0.0 : pmin;
    Sb[3] = w[0];
    Sb[4] = nheld;
    Sb[5] = (double)code;
    Sb[6] = pmax;
    Sb[7] = (double)bcol;
  }
}

}  // namespace

size_t gn_tiled_lds(int n, int m) {
  const size_t np = (size_t)kGnTile * ((n + kGnTile - 1) / kGnTile);
  return sizeof(double) * (2 * np + 256) + (size_t)((m + 15) & ~15) + np;
}
const void* gn_tiled_kernel() { return reinterpret_cast<const void*>(&towr_gn_tiled_kernel); }

size_t gn_direct_lds(int n, int m, int width) {
  return sizeof(double) * (size_t)(4 * ((n + 1) & ~1) + 2 * ((width + 2) & ~1)) + (size_t)((m + 15) & ~15) + (size_t)((n + 15) & ~15);
}
const void* gn_direct_kernel() { return reinterpret_cast<const void*>(&towr_gn_direct_kernel); }

size_t gn_direction_lds(int n, int m) {
  return sizeof(double) * (size_t)(3 * ((n + 1) & ~1) + ((m + 1) & ~1) + kJpChunk + 2) + sizeof(uint16_t) * kJpChunk +
         (size_t)((m + 15) & ~15);
}
const void* gn_direction_kernel() { return reinterpret_cast<const void*>(&towr_gn_direction_kernel); }
const void* gn_direction_pc_kernel() { return reinterpret_cast<const void*>(&towr_gn_direction_pc_kernel); }

size_t jp_vec_lds(int n, int m) { return sizeof(double) * (size_t)(((n + 1) & ~1) + kJpChunk + 2); }
size_t jp_tvec_lds(int n, int m) {
  return sizeof(double) * (size_t)(((m + 1) & ~1) + ((n + 1) & ~1) + kJpChunk) + sizeof(uint16_t) * kJpChunk;
}
const void* jp_vec_kernel() { return reinterpret_cast<const void*>(&towr_jac_vec_kernel); }
const void* jp_tvec_kernel() { return reinterpret_cast<const void*>(&towr_jac_tvec_kernel); }

}  // namespace tg
