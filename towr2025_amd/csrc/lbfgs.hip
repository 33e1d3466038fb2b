// lbfgs.hip — the batched L-BFGS kernels: the per-problem ring of (s, y) pairs (towr_gpu_lbfgs_update_batch_device)
// and the two-loop recursion on the free columns (towr_gpu_lbfgs_direction_batch_device); and the kernels of the
// resident AL loop built on them (the line search, the probe stage in front of it, the verdict stage of the lazy GN loop,
// the outer update, the stop rule, the state's initialisation; at the end), with the two kernels of the compacting
// solve behind those (the partition plan and the row swap) and the two of the queued solve (the retire key and the row move by index).
//
// The shape of resid.hip and step.hip. One block of kLbfgsBlock threads per problem. Lane l takes columns l,
// l + kLbfgsBlock, ... in ascending order in every pass, so a column belongs to one lane for the whole kernel: the
// per-column state in LDS (s and y of the update; q / r and the pair's row kept for the in-place update of the
// direction) is lane-private and needs no barrier, and the held mask is a bit per column in a lane register. The rows
// stream coalesced (8 bytes per lane, 512 per wave instruction).
//   update:    one pass over X, XN, GR, GRN forms s and y once (into LDS) and the three sums; the decision is taken on
//              the sums; only then the slot and HMETA are written, from LDS. A rejected problem writes SUM alone.
//   direction: a pair costs one pass over (s_k, y_k) in the first loop — it forms sum s y, sum s q and sum y y, with
//              y_k kept in LDS for q -= a y — and one more in the second (sum y r, s_k kept for r += (a - beta) s).
//   sums: the lane's partial in column order, a fixed __shfl_down tree over the wave, the waves' partials added in wave
//     order by one lane and the scalar broadcast through LDS behind a barrier: every lane takes the accept / used
//     decisions on the same bits. No floating-point atomics.
// Contraction is off: every product and sum is the plain IEEE expression the header states. Nothing depends on B, the
// block's place in the grid, the stream or timing: the bits are a function of the problem.
#include <hip/hip_runtime.h>

#include "consumer_common.h"
#include "layout.h"

namespace tg {
namespace {

constexpr int kLbfgsWaves = kLbfgsBlock / 64;
static_assert(kLbfgsMaxLds / 16 <= 32 * kLbfgsBlock, "the held mask is one 32-bit word per lane");
static_assert(TOWR_LBFGS_MAX_MEM < 32, "the used pairs are one 32-bit mask");

// v[k] <- the block's sum of v[k], the same bits in every lane (two barriers; s_part / s_bc may be reused at once)
template <int K>
__device__ inline void block_sums(double (&v)[K], double (*s_part)[kLbfgsWaves], double* s_bc, int tid) {
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
      for (int w = 1; w < kLbfgsWaves; ++w) t += s_part[k][w];
      s_bc[k] = t;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = s_bc[k];
}

__global__ void __launch_bounds__(kLbfgsBlock) towr_lbfgs_update_kernel(LbfgsUpdateArgs a) {
#pragma clang fp contract(off)
  extern __shared__ double s_dyn[];
  __shared__ double s_part[3][kLbfgsWaves], s_bc[3];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int n = a.n, mem = a.mem;
  double* s_s = s_dyn;
  double* s_y = s_dyn + n;
  const double* Xb = a.X + b * a.ldx;
  const double* XNb = a.XN + b * a.ldxn;
  const double* Gb = a.GR + b * a.ldgr;
  const double* GNb = a.GRN + b * a.ldgrn;
  int count = a.HMETA[2 * b], next = a.HMETA[2 * b + 1];   // (read by every lane before the sums' barriers)
  if (count < 0 || count > mem || next < 0 || next >= mem) count = next = 0;

  double v[3] = {0.0, 0.0, 0.0};   // sum s y, sum s s, sum y y
#pragma unroll 4
  for (int j = tid; j < n; j += kLbfgsBlock) {
    const double s = XNb[j] - Xb[j];
    const double y = GNb[j] - Gb[j];
    s_s[j] = s;
    s_y[j] = y;
    v[0] += s * y;
    v[1] += s * s;
    v[2] += y * y;
  }
  block_sums<3>(v, s_part, s_bc, tid);
  const bool accept = v[0] > a.curv_eps * v[2];   // (a NaN anywhere: false)
  if (accept) {
    double* S = a.HS + (b * mem + next) * a.ldh;
    double* Y = a.HY + (b * mem + next) * a.ldh;
#pragma unroll 4
    for (int j = tid; j < n; j += kLbfgsBlock) {
      S[j] = s_s[j];
      Y[j] = s_y[j];
    }
  }
  if (tid == 0) {
    const int cnt = accept ? (count < mem ? count + 1 : mem) : count;
    if (accept) {
      a.HMETA[2 * b] = cnt;
      a.HMETA[2 * b + 1] = next + 1 < mem ? next + 1 : 0;
    }
    double* Sb = a.SUM + b * a.lds;
    Sb[0] = v[0];
    Sb[1] = v[1];
    Sb[2] = v[2];
    Sb[3] = accept ? 1.0 : 0.0;
    Sb[4] = (double)cnt;
    Sb[5] = accept ? (double)next : -1.0;
  }
}

// The line search of the resident AL loop (towr_gpu.h): the update kernel's pass with one more sum (gs = sum GR s), the
// accept test on the broadcast sums, the pair offered from LDS as above, then — when a base is accepted — one pass
// that copies XC / GRC over X / GR and takes pg on the new base. The phase, the meta and the scalars are read by every
// lane at entry; lane 0 writes them behind the last barrier of the path taken.
__global__ void __launch_bounds__(kLbfgsBlock) towr_linesearch_kernel(LineSearchArgs a) {
#pragma clang fp contract(off)
  extern __shared__ double s_dyn[];
  __shared__ double s_part[4][kLbfgsWaves], s_bc[4];
  __shared__ unsigned long long s_pg[kLbfgsWaves];
  const towr_alsolve_state_t& st = a.st;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int n = a.n, mem = a.mem;
  int32_t* IS = st.ISTATE + 4 * b;
  double* Lb = st.LSUM + b * st.ldls;
  const int phase = IS[0];
  if (phase != kAlRestart && phase != kAlSearch) {   // frozen (or garbage): nothing but the flags and the code
    if (tid == 0) {
      IS[1] = 0;
      Lb[0] = 0.0;
    }
    return;
  }
  double* s_s = s_dyn;
  double* s_y = s_dyn + n;
  double* Xb = st.X + b * st.ldx;
  double* Gb = st.GR + b * st.ldx;
  const double* XCb = st.XC + b * st.ldx;
  const double* GCb = st.GRC + b * st.ldx;
  double* Sc = st.SCAL + b * st.ldsc;
  int count = st.HMETA[2 * b], next = st.HMETA[2 * b + 1];
  if (count < 0 || count > mem || next < 0 || next >= mem) count = next = 0;
  const int inner = IS[2];
  const double fc = st.FC[b], viol = st.RSUM[b * st.ldrs];
  const double mc = fc + st.RSUM[b * st.ldrs + 3];
  const double m0 = Sc[0], pg_old = Sc[1], alpha = st.ALPHA[b];

  double v[4] = {0.0, 0.0, 0.0, 0.0};   // sum s y, sum s s, sum y y, sum gr s
  bool take = true, store = false;      // a base is accepted; the pair goes to its slot
  if (phase == kAlSearch) {
#pragma unroll 4
    for (int j = tid; j < n; j += kLbfgsBlock) {
      const double g = Gb[j];
      const double s = XCb[j] - Xb[j];
      const double y = GCb[j] - g;
      s_s[j] = s;
      s_y[j] = y;
      v[0] += s * y;
      v[1] += s * s;
      v[2] += y * y;
      v[3] += g * s;
    }
    block_sums<4>(v, s_part, s_bc, tid);
    const double c1gs = a.c1 * v[3];
    take = v[3] <= 0.0 && mc <= m0 + c1gs;   // (a NaN anywhere: false)
    store = take && v[0] > a.curv_eps * v[2];
    if (store) {
      double* S = st.HS + (b * mem + next) * st.ldh;
      double* Y = st.HY + (b * mem + next) * st.ldh;
#pragma unroll 4
      for (int j = tid; j < n; j += kLbfgsBlock) {
        S[j] = s_s[j];
        Y[j] = s_y[j];
      }
    }
  }

  unsigned long long pg = 0ull;
  if (take) {   // X <- XC, GR <- GRC and pg there (the step kernel's expression with a = 1)
    const double* Lo = a.XL + b * a.ldb;
    const double* Up = a.XU + b * a.ldb;
#pragma unroll 4
    for (int j = tid; j < n; j += kLbfgsBlock) {
      const double x = XCb[j], g = GCb[j], l = Lo[j], u = Up[j];
      Xb[j] = x;
      Gb[j] = g;
      const bool has_l = l > -kSideInf, has_u = u < kSideInf;
      const double ad = 1.0 * g;
      double xp = x - ad;
      if (has_l && xp < l) xp = l;
      if (has_u && xp > u) xp = u;
      const unsigned long long sb = v_bits(fabs(xp - x));
      if (sb > pg) pg = sb;
    }
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long om = __shfl_down(pg, o, 64);
      if (om > pg) pg = om;
    }
    if ((tid & 63) == 0) s_pg[tid >> 6] = pg;
    __syncthreads();
  }
  if (tid != 0) return;

  int code, flags = 0;
  if (take) {
    for (int w = 1; w < kLbfgsWaves; ++w)
      if (s_pg[w] > pg) pg = s_pg[w];
    if (phase == kAlRestart) {
      st.HMETA[2 * b] = 0;
      st.HMETA[2 * b + 1] = 0;
      IS[0] = kAlSearch;
      code = 1;
      flags = 1 | 2 | 4;
    } else {
      const int cnt = store ? (count < mem ? count + 1 : mem) : count;
      if (store) {
        st.HMETA[2 * b] = cnt;
        st.HMETA[2 * b + 1] = next + 1 < mem ? next + 1 : 0;
      }
      double* Ub = st.USUM + b * st.ldus;
      Ub[0] = v[0];
      Ub[1] = v[1];
      Ub[2] = v[2];
      Ub[3] = store ? 1.0 : 0.0;
      Ub[4] = (double)cnt;
      Ub[5] = store ? (double)next : -1.0;
      code = 2;
      flags = 1 | 2;
    }
    Sc[0] = mc;
    Sc[1] = __longlong_as_double((long long)pg);
    Sc[4] = viol;
    Sc[5] = fc;
    st.ALPHA[b] = a.alpha0;
  } else {
    const double t = alpha * a.shrink;
    if (t >= a.alpha_min) {
      st.ALPHA[b] = t;
      code = 3;
    } else if (count > 0) {
      st.HMETA[2 * b] = 0;
      st.HMETA[2 * b + 1] = 0;
      st.ALPHA[b] = a.alpha0;
      flags = 2 | 4;
      code = 4;
    } else {
      IS[0] = kAlStalled;
      st.ALPHA[b] = 0.0;
      code = 5;
    }
  }
  IS[1] = flags;
  IS[2] = inner + 1;
  Lb[0] = (double)code;
  Lb[1] = v[3];
  Lb[2] = mc;
  Lb[3] = m0;
  Lb[4] = v[0];
  Lb[5] = v[2];
  Lb[6] = store ? 1.0 : 0.0;
  Lb[7] = take ? __longlong_as_double((long long)pg) : pg_old;
}

// The probe stage of the resident AL loop (towr_gpu.h, towr_gpu_alsolve_probe_batch_device): launch t of T + 1. Between
// two launches the host side evaluates f and phi at the candidates in XT (an f-only objective launch, a g-only
// evaluation, the residual kernel). Launch t, for a SEARCH problem that no earlier launch decided (PSUM[0] == 0):
//   folds trial t - 1: MC = F + RS[3], the line search's test on it and on the gs that launch t - 1 left in PSUM[5];
//   passed, or a_t is below alpha_min: the stage ends at a_{t-1} (code 1 / 3); else t == T: it ends at the untested a_T
//     (code 2); else the candidate of trial t goes into XT and its gs into PSUM[5].
// Ending writes XC = P(X - a D) with the step kernel's expression (the bits trial t* left in XT), gs on the line search's
// tree (block_sums: the lane's partial in column order), ALPHA, inner and the summary. The lengths are recomputed from
// ALPHA by t rounded products; every lane reads ALPHA, inner and PSUM before the sums' barriers, lane 0 writes them behind.
// A problem that is not in SEARCH gets PSUM[0] = 0 and, in XT, a copy of X for the evaluations between the launches.
__global__ void __launch_bounds__(kLbfgsBlock) towr_alsolve_probe_kernel(ProbeArgs a) {
#pragma clang fp contract(off)
  __shared__ double s_part[1][kLbfgsWaves], s_bc[1];
  const towr_alsolve_state_t& st = a.st;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int n = a.n, t = a.t;
  int32_t* IS = st.ISTATE + 4 * b;
  double* Pb = a.PSUM + b * a.ldps;
  double* XTb = a.XT + b * a.ldxt;
  const double* Xb = st.X + b * st.ldx;
  if (IS[0] != kAlSearch) {   // (block-uniform: before any barrier)
    if (t == 0) {
#pragma unroll 4
      for (int j = tid; j < n; j += kLbfgsBlock) XTb[j] = Xb[j];
      if (tid == 0) Pb[0] = 0.0;
    }
    return;
  }
  if (t > 0 && Pb[0] != 0.0) return;   // decided by an earlier launch (every lane reads the same word; no launch writes it meanwhile)
  const double gs_prev = t > 0 ? Pb[5] : 0.0;
  const int inner = IS[2];
  const double m0 = st.SCAL[b * st.ldsc];
  double prev = 0.0, cur = st.ALPHA[b];   // a_{t-1}, a_t
  for (int k = 0; k < t; ++k) {
    prev = cur;
    cur = cur * a.shrink;
  }
  const bool cur_ok = t == 0 || cur >= a.alpha_min;   // (a NaN: false; the lengths before it were valid, or t - 1 had ended the stage)
  double mc = __longlong_as_double(0x7ff8000000000000ll);
  bool pass = false;
  if (t > 0) {
    mc = a.F[b] + a.RS[b * a.ldrs + 3];
    const double c1gs = a.c1 * gs_prev;
    pass = gs_prev <= 0.0 && mc <= m0 + c1gs;   // (a NaN anywhere: false)
  }
  int code = 0, tstar = 0;
  double al = cur;
  if (pass || !cur_ok) {
    code = pass ? 1 : 3;
    tstar = t - 1;
    al = prev;
  } else if (t == a.T) {
    code = 2;
    tstar = t;
    mc = __longlong_as_double(0x7ff8000000000000ll);
  }
  double* Ob = code ? st.XC + b * st.ldx : XTb;
  const double* Db = st.D + b * st.ldx;
  const double* Gb = st.GR + b * st.ldx;
  const double* Lo = a.XL + b * a.ldb;
  const double* Up = a.XU + b * a.ldb;
  double v[1] = {0.0};   // sum gr s
#pragma unroll 4
  for (int j = tid; j < n; j += kLbfgsBlock) {
    const double x = Xb[j], d = Db[j], l = Lo[j], u = Up[j], g = Gb[j];
    const bool has_l = l > -kSideInf, has_u = u < kSideInf;
    const double ad = al * d;
    double xp = x - ad;   // (the comparisons drop a NaN: xp stays NaN)
    if (has_l && xp < l) xp = l;
    if (has_u && xp > u) xp = u;
    Ob[j] = xp;
    const double s = xp - x;
    v[0] += g * s;
  }
  block_sums<1>(v, s_part, s_bc, tid);
  if (tid != 0) return;
  if (!code) {
    Pb[0] = 0.0;
    Pb[5] = v[0];
    return;
  }
  st.ALPHA[b] = al;
  IS[2] = inner + tstar;
  Pb[0] = (double)code;
  Pb[1] = (double)tstar;
  Pb[2] = (double)(code == 2 ? t : tstar + 1);
  Pb[3] = al;
  Pb[4] = mc;
  Pb[5] = v[0];
  Pb[6] = 0.0;
  Pb[7] = 0.0;
}

// The verdict stage of the lazy GN loop (towr_gpu.h, towr_gpu_alsolve_verdict_batch_device): the line search's accept
// test restated ahead of the direction, on the operands the line search will find (the stage writes none of them).
// RESTART: 0 (the line search always takes a RESTART candidate); SEARCH: gs = sum GR (XC - X) on the tree of the line
// search's v[3] (block_sums: the lane's partial in column order), mc = FC + RSUM[3], the test on the broadcast sum; any
// other word: 2. The words are a RUN mask for the direction kernels (run_stride 1). The phase is read by every lane at
// entry; lane 0 writes VERDICT and counts the zeros in NDIR behind the sums' barriers.
__global__ void __launch_bounds__(kLbfgsBlock) towr_alsolve_verdict_kernel(VerdictArgs a) {
#pragma clang fp contract(off)
  __shared__ double s_part[1][kLbfgsWaves], s_bc[1];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int n = a.n;
  const int phase = a.ISTATE[4 * b];
  int word = 2;
  if (phase == kAlRestart) {
    word = 0;
  } else if (phase == kAlSearch) {   // (block-uniform: every lane reaches the sums' barriers)
    const double* Xb = a.X + b * a.ldx;
    const double* Gb = a.GR + b * a.ldx;
    const double* XCb = a.XC + b * a.ldx;
    const double mc = a.FC[b] + a.RSUM[b * a.ldrs + 3];
    const double m0 = a.SCAL[b * a.ldsc];
    double v[1] = {0.0};   // sum gr s
#pragma unroll 4
    for (int j = tid; j < n; j += kLbfgsBlock) {
      const double g = Gb[j];
      const double s = XCb[j] - Xb[j];
      v[0] += g * s;
    }
    block_sums<1>(v, s_part, s_bc, tid);
    const double c1gs = a.c1 * v[0];
    const bool take = v[0] <= 0.0 && mc <= m0 + c1gs;   // (a NaN anywhere: false)
    word = take ? 0 : 2;
  }
  if (tid != 0) return;
  a.VERDICT[b] = word;
  if (word == 0 && a.NDIR) a.NDIR[b] = a.NDIR[b] + 1;
}

__global__ void __launch_bounds__(kLbfgsBlock) towr_lbfgs_direction_kernel(LbfgsDirArgs a) {
#pragma clang fp contract(off)
  extern __shared__ double s_dyn[];
  __shared__ double s_part[3][kLbfgsWaves], s_bc[3];
  __shared__ double s_alpha[TOWR_LBFGS_MAX_MEM], s_c[TOWR_LBFGS_MAX_MEM];   // a_i and c_i of the used pairs, by i - 1
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  if (a.RUN && !(a.RUN[b * a.run_stride] & 2)) return;   // (block-uniform: before any barrier)
  const int n = a.n, mem = a.mem;
  double* s_q = s_dyn;       // q, then r; a held column keeps g
  double* s_v = s_dyn + n;   // the pair's y (first loop) or s (second loop)
  const double* Gb = a.GR + b * a.ldgr;
  const double* HSb = a.HS + b * mem * a.ldh;
  const double* HYb = a.HY + b * mem * a.ldh;
  int count = a.HMETA[2 * b], next = a.HMETA[2 * b + 1];
  if (count < 0 || count > mem || next < 0 || next >= mem) count = next = 0;

  // q = g, the held mask (bit k: the lane's k-th column) and sum_free g^2
  unsigned held = 0u;
  double nheld = 0.0, gg = 0.0;
  if (a.X) {
    const double* Xb = a.X + b * a.ldx;
    const double* Lb = a.XL + b * a.ldb;
    const double* Ub = a.XU + b * a.ldb;
    int k = 0;
#pragma unroll 4
    for (int j = tid; j < n; j += kLbfgsBlock, ++k) {
      const double g = Gb[j], x = Xb[j], l = Lb[j], u = Ub[j];
      const bool has_l = l > -kSideInf, has_u = u < kSideInf;
      const bool h = (has_l && x <= l && g > 0.0) || (has_u && x >= u && g < 0.0) || (has_l && has_u && l == u);
      if (h) {
        held |= 1u << k;
        nheld += 1.0;
      } else {
        gg += g * g;
      }
      s_q[j] = g;
    }
  } else {
#pragma unroll 4
    for (int j = tid; j < n; j += kLbfgsBlock) {
      const double g = Gb[j];
      gg += g * g;
      s_q[j] = g;
    }
  }

  // first loop, newest to oldest
  unsigned used = 0u;
  int nused = 0;
  double gamma = 1.0;
  for (int i = 1; i <= count; ++i) {
    const int slot = next - i < 0 ? next - i + mem : next - i;
    const double* S = HSb + (int64_t)slot * a.ldh;
    const double* Y = HYb + (int64_t)slot * a.ldh;
    double v[3] = {0.0, 0.0, 0.0};   // sum_free s y, sum_free s q, sum_free y y
    int k = 0;
#pragma unroll 4
    for (int j = tid; j < n; j += kLbfgsBlock, ++k) {
      const double s = S[j], y = Y[j];
      s_v[j] = y;
      if (!((held >> k) & 1u)) {
        v[0] += s * y;
        v[1] += s * s_q[j];
        v[2] += y * y;
      }
    }
    block_sums<3>(v, s_part, s_bc, tid);
    if (v[0] > 0.0) {   // (a NaN c_i: unused)
      const double al = v[1] / v[0];
      if (!used) gamma = v[0] / v[2];
      used |= 1u << i;
      ++nused;
      if (tid == 0) {
        s_alpha[i - 1] = al;
        s_c[i - 1] = v[0];
      }
      k = 0;
      for (int j = tid; j < n; j += kLbfgsBlock, ++k)
        if (!((held >> k) & 1u)) s_q[j] = s_q[j] - al * s_v[j];
    }
  }

  // r = gamma q (no pair used: r = q, bit for bit)
  if (used) {
    int k = 0;
    for (int j = tid; j < n; j += kLbfgsBlock, ++k)
      if (!((held >> k) & 1u)) s_q[j] = gamma * s_q[j];
  }

  // second loop, the used pairs oldest to newest
  for (int i = count; i >= 1; --i) {
    if (!((used >> i) & 1u)) continue;
    const int slot = next - i < 0 ? next - i + mem : next - i;
    const double* S = HSb + (int64_t)slot * a.ldh;
    const double* Y = HYb + (int64_t)slot * a.ldh;
    double v[1] = {0.0};   // sum_free y r
    int k = 0;
#pragma unroll 4
    for (int j = tid; j < n; j += kLbfgsBlock, ++k) {
      const double s = S[j], y = Y[j];
      s_v[j] = s;
      if (!((held >> k) & 1u)) v[0] += y * s_q[j];
    }
    block_sums<1>(v, s_part, s_bc, tid);   // (its barriers also order tid 0's s_alpha / s_c before the reads below)
    const double beta = v[0] / s_c[i - 1];
    const double co = s_alpha[i - 1] - beta;
    k = 0;
    for (int j = tid; j < n; j += kLbfgsBlock, ++k)
      if (!((held >> k) & 1u)) s_q[j] = s_q[j] + co * s_v[j];
  }

  // D and the slope sum g D over all columns
  double* Db = a.D + b * a.ldd;
  double w[3] = {0.0, gg, nheld};   // (the held count: integers below 2^53, exact in any order)
#pragma unroll 4
  for (int j = tid; j < n; j += kLbfgsBlock) {
    const double d = s_q[j], g = Gb[j];
    Db[j] = d;
    w[0] += g * d;
  }
  block_sums<3>(w, s_part, s_bc, tid);
  if (tid == 0) {
    double* Sb = a.SUM + b * a.lds;
    Sb[0] = (double)nused;
    Sb[1] = gamma;
    Sb[2] = w[0];
    Sb[3] = w[2];
    Sb[4] = w[1];
  }
}

// The outer update and the initialisation of the resident AL loop (towr_gpu.h). One block per problem, lane l on rows /
// columns l, l + kLbfgsBlock, ..., the rows streamed once (non-temporal). There are no sums: every output is a copy, one
// rounded product or a comparison.
//   outer: every lane reads the problem's phase, flags, counter and scalars and takes the same decisions on them; a
//          problem the update does not act on returns before anything is written. Only the multiplier update moves a
//          row (LAM <- LAMP); the scalars are written by lane 0 behind a barrier, once every lane has read them.
//   init:  XC = the caller's X clamped to the sides that count, D = 0, the scalars by lane 0.
__global__ void __launch_bounds__(kLbfgsBlock) towr_alsolve_outer_kernel(OuterArgs a) {
#pragma clang fp contract(off)
  const towr_alsolve_state_t& st = a.st;
  const towr_alsolve_params_t& pr = a.pr;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  int32_t* IS = st.ISTATE + 4 * b;
  double* Sc = st.SCAL + b * st.ldsc;
  const int phase = IS[0], flags = IS[1], inner = IS[2], outer = IS[3];
  const double pg = Sc[1], eta = Sc[2], omega = Sc[3], viol = Sc[4];
  if (phase != kAlSearch || !(flags & 1) || !(pg <= omega || inner >= pr.max_inner)) return;
  const bool converged = viol <= eta && viol <= pr.eta_star && pg <= pr.omega_star;
  const bool feasible = viol <= eta;   // (a NaN viol: the penalty grows)
  if (!converged && feasible) {
    const double* LPb = st.LAMP + b * st.ldl;
    double* LAMb = st.LAM + b * st.ldl;
#pragma unroll 4
    for (int i = tid; i < a.m; i += kLbfgsBlock) __builtin_nontemporal_store(__builtin_nontemporal_load(LPb + i), LAMb + i);
  }
  __syncthreads();   // every lane has read the scalars
  if (tid != 0) return;
  st.ALPHA[b] = 0.0;
  IS[1] = 0;
  if (converged) {
    IS[0] = kAlConverged;
    return;
  }
  if (feasible) {
    const double te = eta * pr.eta_shrink, to = omega * pr.omega_shrink;
    Sc[2] = te > pr.eta_star ? te : pr.eta_star;
    Sc[3] = to > pr.omega_star ? to : pr.omega_star;
  } else {
    const double tr = st.RHO[b] * pr.rho_grow;
    st.RHO[b] = tr < pr.rho_max ? tr : pr.rho_max;
  }
  IS[3] = outer + 1;
  IS[2] = 0;
  st.HMETA[2 * b] = 0;
  st.HMETA[2 * b + 1] = 0;
  IS[0] = outer + 1 >= pr.max_outer ? kAlMaxed : kAlRestart;
}

// The stop rule of the resident AL loop (towr_gpu.h, towr_gpu_alsolve_stop_batch_device), between the line search and
// the outer update. One thread per problem: it reads the problem's four state words, five scalars and RHO and takes
// every decision on them; a problem that is not in SEARCH returns before anything is written. IEEE comparisons and one
// rounded product; every test is written so that a NaN operand makes it false on the stopping side (`within` false
// resets the run, `!(viol <= eta)` is the outer update's own "not feasible", the three tests of `stuck` are false).
__global__ void __launch_bounds__(kLbfgsBlock) towr_alsolve_stop_kernel(StopArgs a) {
#pragma clang fp contract(off)
  const int64_t b = (int64_t)blockIdx.x * kLbfgsBlock + threadIdx.x;
  if (b >= a.B) return;
  int32_t* IS = a.ISTATE + 4 * b;
  if (IS[0] != kAlSearch) return;
  double* Sc = a.SCAL + b * a.ldsc;
  const int flags = IS[1], inner = IS[2];
  const double pg = Sc[1], eta = Sc[2], omega = Sc[3], viol = Sc[4];
  const towr_alsolve_stop_t& sp = a.sp;
  if (sp.acc_iters > 0) {
    const bool within = viol <= sp.acc_eta && pg <= sp.acc_omega;
    const double run = within ? Sc[6] + 1.0 : 0.0;
    Sc[6] = run;
    if (run >= (double)sp.acc_iters) {
      IS[0] = kAlAcceptable;
      IS[1] = 0;
      a.ALPHA[b] = 0.0;
      return;
    }
  }
  const bool grow = (flags & 1) && (pg <= omega || inner >= a.max_inner) && !(viol <= eta);
  if (!grow) return;
  const double last = Sc[7];
  const double keep = sp.infeas_keep * last;
  const bool stuck = last > 0.0 && viol >= keep && a.RHO[b] >= sp.infeas_rho;
  if (stuck) {
    IS[0] = kAlInfeasible;
    IS[1] = 0;
    a.ALPHA[b] = 0.0;
  } else {
    Sc[7] = viol;
  }
}

__global__ void __launch_bounds__(kLbfgsBlock) towr_alsolve_init_kernel(AlInitArgs a) {
#pragma clang fp contract(off)
  const towr_alsolve_state_t& st = a.st;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const double* Xb = st.X + b * st.ldx;
  const double* Lo = a.XL + b * a.ldb;
  const double* Up = a.XU + b * a.ldb;
  double* XCb = st.XC + b * st.ldx;
  double* Db = st.D + b * st.ldx;
#pragma unroll 4
  for (int j = tid; j < a.n; j += kLbfgsBlock) {
    const double l = Lo[j], u = Up[j];
    double x = __builtin_nontemporal_load(Xb + j);
    if (l > -kSideInf && x < l) x = l;   // (the comparisons drop a NaN: x stays NaN)
    if (u < kSideInf && x > u) x = u;
    __builtin_nontemporal_store(x, XCb + j);
    __builtin_nontemporal_store(0.0, Db + j);
  }
  if (tid != 0) return;
  int32_t* IS = st.ISTATE + 4 * b;
  IS[0] = kAlRestart;
  IS[1] = 0;
  IS[2] = 0;
  IS[3] = 0;
  st.HMETA[2 * b] = 0;
  st.HMETA[2 * b + 1] = 0;
  st.RHO[b] = a.rho0;
  st.ALPHA[b] = 0.0;
  double* Sc = st.SCAL + b * st.ldsc;
  for (int k = 0; k < 8; ++k) Sc[k] = 0.0;
  Sc[2] = a.eta0;
  Sc[3] = a.omega0;
}

// The select of the resident GN loop (towr_gpu_alsolve_gn_iterate_batch_device): by the flags the line search wrote,
// D <- DC when a base was accepted (bit 0), else D <- GR when the history was reset (bit 2: the steepest-descent retry),
// else nothing. Copies only; every lane reads the flags, which no kernel writes meanwhile.
__global__ void __launch_bounds__(kLbfgsBlock) towr_gn_select_kernel(GnSelectArgs a) {
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int flags = a.ISTATE[4 * b + 1];
  if (!(flags & (1 | 4))) return;
  const double* Sb = (flags & 1) ? a.DC + b * a.lddc : a.GR + b * a.ldgr;
  double* Db = a.D + b * a.ldd;
#pragma unroll 4
  for (int j = tid; j < a.n; j += kLbfgsBlock) Db[j] = Sb[j];
}

// The partition plan of the compacting solve (towr_gpu_alsolve_partition_batch_device). One block. A row is active iff
// its phase word is 0 or 1. The first pass counts the six classes of phase words (a ballot per class and stride, the
// waves' counts added through LDS): na = the active rows. The second pass walks the rows again in strides of the block
// and ranks the frozen rows in [0, na) and the active rows in [na, B), each in ascending row order: a lane's rank is the
// running count of the strides before, the counts of the waves before it in this stride and the set bits below it in its
// wave's ballot. Integer counts only: the result is a function of the phase words. Rank r < np <= B / 2 writes
// PAIRS[2 r] (frozen) or PAIRS[2 r + 1] (active); nothing else of PAIRS is written.
__global__ void __launch_bounds__(kLbfgsBlock) towr_alsolve_partition_kernel(PartitionArgs a) {
  __shared__ int32_t s_cnt[kLbfgsWaves][6];
  __shared__ int32_t s_tot[2][kLbfgsWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int B = a.B;
  int32_t cnt[6] = {0, 0, 0, 0, 0, 0};
  for (int base = 0; base < B; base += kLbfgsBlock) {   // (a uniform trip count: every lane takes every ballot)
    const int i = base + tid;
    int cls = -1;
    if (i < B) {
      const int32_t p = a.ISTATE[4 * (int64_t)i];
      cls = (p >= 0 && p <= 4) ? p : 5;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) cnt[k] += __popcll(__ballot(cls == k));
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) s_cnt[wave][k] = cnt[k];
  }
  __syncthreads();
  int32_t tot[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    tot[k] = 0;
    for (int w = 0; w < kLbfgsWaves; ++w) tot[k] += s_cnt[w][k];
  }
  const int na = tot[0] + tot[1];
  int32_t run_f = 0, run_a = 0;   // frozen rows ranked so far in [0, na), active rows in [na, B): the same in every lane
  for (int base = 0; base < B; base += kLbfgsBlock) {
    const int i = base + tid;
    bool act = false;
    if (i < B) {
      const int32_t p = a.ISTATE[4 * (int64_t)i];
      act = p == kAlRestart || p == kAlSearch;
    }
    const bool f = i < na && !act;           // (na <= B)
    const bool g = i >= na && i < B && act;
    const unsigned long long mf = __ballot(f), mg = __ballot(g);
    if (lane == 0) {
      s_tot[0][wave] = __popcll(mf);
      s_tot[1][wave] = __popcll(mg);
    }
    __syncthreads();
    int32_t off_f = run_f, off_a = run_a;
    for (int w = 0; w < kLbfgsWaves; ++w) {
      const int32_t tf = s_tot[0][w], ta = s_tot[1][w];
      if (w < wave) { off_f += tf; off_a += ta; }
      run_f += tf;
      run_a += ta;
    }
    if (f) a.PAIRS[2 * (int64_t)(off_f + __popcll(mf & below))] = i;
    if (g) a.PAIRS[2 * (int64_t)(off_a + __popcll(mg & below)) + 1] = i;
    __syncthreads();   // s_tot is rewritten by the next stride
  }
  if (tid == 0) {
    a.HEAD[0] = na;
    a.HEAD[1] = run_f;   // (== run_a: [0, na) lacks as many active rows as [na, B) holds)
#pragma unroll
    for (int k = 0; k < 6; ++k) a.HEAD[2 + k] = tot[k];
  }
}

// The row swap of the compacting solve (towr_gpu_alsolve_swap_rows_batch_device): block (i, k) exchanges bytes
// [0, row_bytes) of rows PAIRS[2 i] and PAIRS[2 i + 1] of array k; blocks beyond the pair count (read from NP[0] when
// given) exit. A lane reads its word of both rows into registers, then writes both; a word belongs to one lane and the
// pairs are disjoint, so no two lanes of the grid touch the same byte. 8 bytes per lane where the array's base, leading
// dimension and row length allow, else 4; coalesced.
template <class T>
__device__ inline void swap_words(char* p, char* q, int64_t bytes, int tid) {
  T* u = reinterpret_cast<T*>(p);
  T* v = reinterpret_cast<T*>(q);
  const int64_t nw = bytes / (int64_t)sizeof(T);
#pragma unroll 4
  for (int64_t j = tid; j < nw; j += kLbfgsBlock) {
    const T x = u[j], y = v[j];
    u[j] = y;
    v[j] = x;
  }
}

__global__ void __launch_bounds__(kLbfgsBlock) towr_alsolve_swap_rows_kernel(SwapRowsArgs a) {
  const int i = blockIdx.x;
  int count = a.npairs;
  if (a.NP) {
    count = a.NP[0];
    if (count > a.npairs) count = a.npairs;   // (npairs: the grid's pairs, max_pairs)
  }
  if (i >= count) return;
  const int32_t f = a.PAIRS[2 * (int64_t)i], g = a.PAIRS[2 * (int64_t)i + 1];
  if (f < 0 || g < 0 || f == g) return;   // (never from the partition)
  const SwapRows& r = a.rows[blockIdx.y];
  char* p = r.base + (int64_t)f * r.ld_bytes;
  char* q = r.base + (int64_t)g * r.ld_bytes;
  if (((reinterpret_cast<uintptr_t>(r.base) | (uintptr_t)r.ld_bytes | (uintptr_t)r.row_bytes) & 7) == 0)
    swap_words<unsigned long long>(p, q, r.row_bytes, threadIdx.x);
  else
    swap_words<uint32_t>(p, q, r.row_bytes, threadIdx.x);
}

// The retire key of the queued solve (towr_gpu_alsolve_retire_key_batch_device): one thread per row. A row leaves its
// slot when it is frozen (the partition's rule on its phase word) or when it has run out of budget: the key of an active
// row whose age has reached max_age is 7, a word the partition counts as frozen; every other row's key is its phase
// word. ISTATE is not written, so an expired problem keeps its RESTART / SEARCH word. add > 0: AGE[b] += add first (the
// round's iterations). Integer compares only. Of a KEY row only word 0 is written.
__global__ void __launch_bounds__(kLbfgsBlock) towr_alsolve_retire_key_kernel(RetireKeyArgs a) {
  const int64_t b = (int64_t)blockIdx.x * kLbfgsBlock + threadIdx.x;
  if (b >= a.B) return;
  int32_t age = a.AGE[b];
  if (a.add != 0) {
    age += a.add;
    a.AGE[b] = age;
  }
  const int32_t p = a.ISTATE[4 * b];
  const bool act = p == kAlRestart || p == kAlSearch;
  a.KEY[4 * b] = (act && age >= a.max_age) ? 7 : p;
}

// The row move of the queued solve (towr_gpu_alsolve_move_rows_batch_device): block (i, k), i < count, copies bytes
// [0, row_bytes) of row r0 + i of slot[k] to row ID[r0 + i] of out[k], or with `reverse` from there into the slot row. A
// negative ID skips its row. A word belongs to one lane; the IDs of one call are distinct, so no two blocks write the same
// byte. 8 bytes per lane where both bases, both leading dimensions and the row length allow, else 4; coalesced.
template <class T>
__device__ inline void copy_words(const char* src, char* dst, int64_t bytes, int tid) {
  const T* u = reinterpret_cast<const T*>(src);
  T* v = reinterpret_cast<T*>(dst);
  const int64_t nw = bytes / (int64_t)sizeof(T);
#pragma unroll 4
  for (int64_t j = tid; j < nw; j += kLbfgsBlock) v[j] = u[j];
}

__global__ void __launch_bounds__(kLbfgsBlock) towr_alsolve_move_rows_kernel(MoveRowsArgs a) {
  const int i = blockIdx.x;
  if (i >= a.count) return;
  const int64_t row = (int64_t)a.r0 + i;
  const int32_t id = a.ID[row];
  if (id < 0) return;
  const MoveRows& r = a.rows[blockIdx.y];
  char* p = r.slot + row * r.slot_ld;
  char* q = r.out + (int64_t)id * r.out_ld;
  const char* src = a.reverse ? q : p;
  char* dst = a.reverse ? p : q;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(r.slot) | reinterpret_cast<uintptr_t>(r.out) | (uintptr_t)r.slot_ld |
                         (uintptr_t)r.out_ld | (uintptr_t)r.row_bytes;
  if ((bits & 7) == 0)
    copy_words<unsigned long long>(src, dst, r.row_bytes, threadIdx.x);
  else
    copy_words<uint32_t>(src, dst, r.row_bytes, threadIdx.x);
}

}  // namespace

const void* alsolve_partition_kernel() { return reinterpret_cast<const void*>(&towr_alsolve_partition_kernel); }
const void* alsolve_swap_rows_kernel() { return reinterpret_cast<const void*>(&towr_alsolve_swap_rows_kernel); }
const void* alsolve_retire_key_kernel() { return reinterpret_cast<const void*>(&towr_alsolve_retire_key_kernel); }
const void* alsolve_move_rows_kernel() { return reinterpret_cast<const void*>(&towr_alsolve_move_rows_kernel); }
const void* gn_select_kernel() { return reinterpret_cast<const void*>(&towr_gn_select_kernel); }
const void* lbfgs_update_kernel() { return reinterpret_cast<const void*>(&towr_lbfgs_update_kernel); }
const void* lbfgs_direction_kernel() { return reinterpret_cast<const void*>(&towr_lbfgs_direction_kernel); }
const void* alsolve_probe_kernel() { return reinterpret_cast<const void*>(&towr_alsolve_probe_kernel); }
const void* alsolve_verdict_kernel() { return reinterpret_cast<const void*>(&towr_alsolve_verdict_kernel); }
const void* linesearch_kernel() { return reinterpret_cast<const void*>(&towr_linesearch_kernel); }
const void* alsolve_outer_kernel() { return reinterpret_cast<const void*>(&towr_alsolve_outer_kernel); }
const void* alsolve_stop_kernel() { return reinterpret_cast<const void*>(&towr_alsolve_stop_kernel); }
const void* alsolve_init_kernel() { return reinterpret_cast<const void*>(&towr_alsolve_init_kernel); }

}  // namespace tg
