// step.hip — the batched projected step (towr_gpu_step_batch_device): per problem XP = P_[XL, XU](X - a D) and the
// summary of the projected step s = XP - X: max |s|, sum s^2, sum d s, the columns on a bound, how far X is outside
// its box, and max |s| per variable set.
//
// The shape of resid.hip. One block of kStepBlock threads per problem. Lane l takes columns l, l + kStepBlock, ... in
// ascending order, kStepUnroll of them in flight at a time: X, D and XP stream coalesced (8 bytes per lane, 512 per
// wave instruction) and are read or written once; the bounds (shared by the batch when ldb = 0) and the sets' column
// ranges stay cache-resident.
//   sums ([1] sum s^2, [2] sum d s): the lane's partial in column order, a fixed __shfl_down tree over the wave, then
//     the waves' partials added in wave order by one lane — one tree per output, no floating-point atomics;
//   maxima ([0], [4], per set): the values are >= +0.0 or NaN, and NaN is made the canonical quiet NaN, so they order
//     as their bit patterns read as unsigned integers, NaN above everything: integer maxima, exact and order-free;
//   [3] is an integer count, exact in any order.
// t = x - a d is a rounded product then a rounded subtraction: contraction is off for the whole kernel, so every
// output is the plain IEEE expression the header states. Nothing depends on B, the block's place in the grid, the
// stream or timing: the bits are a function of the problem.
#include <hip/hip_runtime.h>

#include "consumer_common.h"
#include "layout.h"

namespace tg {
namespace {

#ifndef TOWR_STEP_UNROLL   // (experiment builds: -DTOWR_STEP_UNROLL. Measured on MI355X, ANYmal trot B = 4096 / stairs gait-opt
                           // B = 1024, ms per call: 4 0.0325 / 0.0132, 8 0.0382-0.0390 / 0.0130-0.0135)
#define TOWR_STEP_UNROLL 4
#endif
constexpr int kStepUnroll = TOWR_STEP_UNROLL;
constexpr int kStepWaves = kStepBlock / 64;

__global__ void __launch_bounds__(kStepBlock) towr_proj_step_kernel(StepArgs a) {
#pragma clang fp contract(off)
  __shared__ int32_t s_col0[TOWR_MAX_VARSETS + 1];
  __shared__ unsigned long long s_setmax[TOWR_MAX_VARSETS];
  __shared__ double s_sq[kStepWaves], s_ds[kStepWaves];
  __shared__ unsigned long long s_smax[kStepWaves], s_out[kStepWaves];
  __shared__ int32_t s_cnt[kStepWaves];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int n = a.n;
  const double* Xb = a.X + b * a.ldx;
  const double* Db = a.D + b * a.ldd;
  const double* Lb = a.XL + b * a.ldb;
  const double* Ub = a.XU + b * a.ldb;
  double* XPb = a.XP ? a.XP + b * a.ldxp : nullptr;
  const double al = a.ALPHA ? a.ALPHA[b] : a.alpha;
  for (int s = tid; s <= a.n_sets; s += kStepBlock) s_col0[s] = a.set_col0[s];
  for (int s = tid; s < a.n_sets; s += kStepBlock) s_setmax[s] = 0ull;
  __syncthreads();

  double sq = 0.0, ds = 0.0;
  unsigned long long smax = 0ull, out = 0ull;   // the lane's largest |s| and largest distance outside the box (bits)
  int cnt = 0;
  int set = 0;                                  // the set of the lane's current column (columns ascend)
  unsigned long long setmax = 0ull;
  for (int j0 = tid; j0 < n; j0 += kStepBlock * kStepUnroll) {
    double x[kStepUnroll], d[kStepUnroll], l[kStepUnroll], u[kStepUnroll];
#pragma unroll
    for (int k = 0; k < kStepUnroll; ++k) {
      const int j = j0 + k * kStepBlock;
      x[k] = 0.0; d[k] = 0.0; l[k] = 0.0; u[k] = 0.0;
      if (j < n) {
        x[k] = __builtin_nontemporal_load(Xb + j);
        d[k] = __builtin_nontemporal_load(Db + j);
        l[k] = Lb[j];
        u[k] = Ub[j];
      }
    }
#pragma unroll
    for (int k = 0; k < kStepUnroll; ++k) {
      const int j = j0 + k * kStepBlock;
      if (j >= n) break;
      const bool has_l = l[k] > -kSideInf, has_u = u[k] < kSideInf;
      const double ad = al * d[k];
      const double t = x[k] - ad;
      double xp = t;                     // (the comparisons drop a NaN: xp stays NaN)
      if (has_l && xp < l[k]) xp = l[k];
      if (has_u && xp > u[k]) xp = u[k];
      if (XPb) __builtin_nontemporal_store(xp, XPb + j);
      const double s = xp - x[k];
      sq += s * s;
      ds += d[k] * s;
      if ((has_l && xp == l[k]) || (has_u && xp == u[k])) ++cnt;
      double o = 0.0;
      if (has_l && l[k] - x[k] > o) o = l[k] - x[k];
      if (has_u && x[k] - u[k] > o) o = x[k] - u[k];
      const unsigned long long ob = v_bits(o);
      if (ob > out) out = ob;
      const unsigned long long sb = v_bits(fabs(s));
      if (sb > smax) smax = sb;
      if (j >= s_col0[set + 1]) {
        if (setmax) atomicMax(&s_setmax[set], setmax);
        setmax = 0ull;
        do ++set; while (j >= s_col0[set + 1]);
      }
      if (sb > setmax) setmax = sb;
    }
  }
  if (setmax) atomicMax(&s_setmax[set], setmax);

  // the wave's tree (lane 0 holds the result), then the waves in order
  for (int o = 32; o > 0; o >>= 1) {
    sq += __shfl_down(sq, o, 64);
    ds += __shfl_down(ds, o, 64);
    cnt += __shfl_down(cnt, o, 64);
    const unsigned long long om = __shfl_down(smax, o, 64);
    if (om > smax) smax = om;
    const unsigned long long oo = __shfl_down(out, o, 64);
    if (oo > out) out = oo;
  }
  if ((tid & 63) == 0) {
    s_sq[tid >> 6] = sq; s_ds[tid >> 6] = ds; s_cnt[tid >> 6] = cnt; s_smax[tid >> 6] = smax; s_out[tid >> 6] = out;
  }
  __syncthreads();
  double* Sb = a.SUM + b * a.lds;
  if (tid == 0) {
    for (int w = 1; w < kStepWaves; ++w) {
      sq += s_sq[w];
      ds += s_ds[w];
      cnt += s_cnt[w];
      if (s_smax[w] > smax) smax = s_smax[w];
      if (s_out[w] > out) out = s_out[w];
    }
    Sb[0] = __longlong_as_double((long long)smax);
    Sb[1] = sq;
    Sb[2] = ds;
    Sb[3] = (double)cnt;
    Sb[4] = __longlong_as_double((long long)out);
  }
  for (int s = tid; s < a.n_sets; s += kStepBlock) Sb[5 + s] = __longlong_as_double((long long)s_setmax[s]);
}

}  // namespace

const void* step_kernel() { return reinterpret_cast<const void*>(&towr_proj_step_kernel); }

}  // namespace tg
