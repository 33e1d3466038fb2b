// resid.hip — batched constraint residuals (towr_gpu_residual_batch_device): per problem, the violation of G against
// the bounds (GL, GU) summarised (max, sum, arg max, per constraint set) and, with LAMP, the augmented Lagrangian's
// multiplier update lam+ = rho (t - clamp(t)), t = g + lam / rho, and its penalty term phi.
//
// One block of kResBlock threads per problem. Lane l takes rows l, l + kResBlock, ... in ascending order, kResUnroll
// of them in flight at a time: G, LAM and LAMP stream coalesced (8 bytes per lane, 512 per wave instruction) and are
// read or written once; the bounds (shared by the batch when ldb = 0) and the sets' row ranges stay cache-resident.
//   sums ([1] sum v, [3] phi): the lane's partial in row order, a fixed __shfl_down tree over the wave, then the
//     waves' partials added in wave order by one lane — one tree per output, no floating-point atomics;
//   maxima: a violation is >= +0.0 or NaN, and NaN is made the canonical quiet NaN, so the values order as their
//     bit patterns read as unsigned integers, NaN above everything. [0] / [2] reduce (bits, row) keys — larger bits
//     win, equal bits the lower row — and the per-set maxima are integer maxima in LDS: exact and order-free.
// Nothing depends on B, the block's place in the grid, the stream or timing: the bits are a function of the problem.
#include <hip/hip_runtime.h>

#include "consumer_common.h"
#include "layout.h"

namespace tg {
namespace {

constexpr int kResUnroll = 4;
constexpr int kResWaves = kResBlock / 64;

__global__ void __launch_bounds__(kResBlock) towr_residual_kernel(ResArgs a) {
  __shared__ int32_t s_row0[TOWR_MAX_CONSTRAINTS + 1];
  __shared__ unsigned long long s_setmax[TOWR_MAX_CONSTRAINTS];
  __shared__ double s_sum[kResWaves], s_phi[kResWaves];
  __shared__ unsigned long long s_key[kResWaves];
  __shared__ int32_t s_arg[kResWaves];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int m = a.m;
  const double* Gb = a.G + b * a.ldg;
  const double* Lb = a.GL + b * a.ldb;
  const double* Ub = a.GU + b * a.ldb;
  const double* LAMb = a.LAM ? a.LAM + b * a.ldl : nullptr;
  double* LPb = a.LAMP ? a.LAMP + b * a.ldlp : nullptr;
  const double rho = a.RHO ? a.RHO[b] : a.rho;   // (RHO: the resident loop's per-problem penalty, auglag.hip)
  for (int s = tid; s <= a.n_sets; s += kResBlock) s_row0[s] = a.set_row0[s];
  for (int s = tid; s < a.n_sets; s += kResBlock) s_setmax[s] = 0ull;
  __syncthreads();

  double sum = 0.0, phi = 0.0;
  unsigned long long key = 0ull;   // the lane's largest violation (bits) and its first row
  int arg = -1;
  int set = 0;                     // the set of the lane's current row (rows ascend, so it only moves forward)
  unsigned long long setmax = 0ull;
  for (int i0 = tid; i0 < m; i0 += kResBlock * kResUnroll) {
    double g[kResUnroll], l[kResUnroll], u[kResUnroll], lam[kResUnroll];
#pragma unroll
    for (int k = 0; k < kResUnroll; ++k) {
      const int i = i0 + k * kResBlock;
      g[k] = 0.0; l[k] = 0.0; u[k] = 0.0; lam[k] = 0.0;
      if (i < m) {
        g[k] = __builtin_nontemporal_load(Gb + i);
        l[k] = Lb[i];
        u[k] = Ub[i];
        if (LAMb) lam[k] = __builtin_nontemporal_load(LAMb + i);
      }
    }
#pragma unroll
    for (int k = 0; k < kResUnroll; ++k) {
      const int i = i0 + k * kResBlock;
      if (i >= m) break;
      const bool has_l = l[k] > -kSideInf, has_u = u[k] < kSideInf;
      double v = 0.0;
      if (has_l && l[k] - g[k] > v) v = l[k] - g[k];
      if (has_u && g[k] - u[k] > v) v = g[k] - u[k];
      if (g[k] != g[k]) v = g[k];   // (the comparisons above drop a NaN)
      sum += v;
      const unsigned long long vb = v_bits(v);
      if (vb > key) { key = vb; arg = i; }
      if (i >= s_row0[set + 1]) {
        if (setmax) atomicMax(&s_setmax[set], setmax);
        setmax = 0ull;
        do ++set; while (i >= s_row0[set + 1]);
      }
      if (vb > setmax) setmax = vb;
      if (LPb) {
        const double t = g[k] + lam[k] / rho;
        double c = t;
        if (has_l && c < l[k]) c = l[k];
        if (has_u && c > u[k]) c = u[k];
        const double r = t - c;
        __builtin_nontemporal_store(rho * r, LPb + i);
        phi += 0.5 * rho * r * r - 0.5 * lam[k] * lam[k] / rho;
      }
    }
  }
  if (setmax) atomicMax(&s_setmax[set], setmax);

  // the wave's tree (lane 0 holds the result), then the waves in order
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_down(sum, o, 64);
    phi += __shfl_down(phi, o, 64);
    const unsigned long long ok = __shfl_down(key, o, 64);
    const int oa = __shfl_down(arg, o, 64);
    if (ok > key || (ok == key && ok != 0ull && oa < arg)) { key = ok; arg = oa; }
  }
  if ((tid & 63) == 0) {
    s_sum[tid >> 6] = sum; s_phi[tid >> 6] = phi; s_key[tid >> 6] = key; s_arg[tid >> 6] = arg;
  }
  __syncthreads();
  double* Sb = a.SUM + b * a.lds;
  if (tid == 0) {
    for (int w = 1; w < kResWaves; ++w) {
      sum += s_sum[w];
      phi += s_phi[w];
      if (s_key[w] > key || (s_key[w] == key && key != 0ull && s_arg[w] < arg)) { key = s_key[w]; arg = s_arg[w]; }
    }
    Sb[0] = __longlong_as_double((long long)key);
    Sb[1] = sum;
    Sb[2] = key ? (double)arg : -1.0;
    Sb[3] = LPb ? phi : 0.0;
  }
  for (int s = tid; s < a.n_sets; s += kResBlock) Sb[4 + s] = __longlong_as_double((long long)s_setmax[s]);
}

}  // namespace

const void* res_kernel() { return reinterpret_cast<const void*>(&towr_residual_kernel); }

}  // namespace tg
