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
#include <hip/hip_runtime.h>

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

}  // namespace

size_t jp_vec_lds(int n, int m) { return sizeof(double) * (size_t)(((n + 1) & ~1) + kJpChunk + 2); }
size_t jp_tvec_lds(int n, int m) {
  return sizeof(double) * (size_t)(((m + 1) & ~1) + ((n + 1) & ~1) + kJpChunk) + sizeof(uint16_t) * kJpChunk;
}
const void* jp_vec_kernel() { return reinterpret_cast<const void*>(&towr_jac_vec_kernel); }
const void* jp_tvec_kernel() { return reinterpret_cast<const void*>(&towr_jac_tvec_kernel); }

}  // namespace tg
