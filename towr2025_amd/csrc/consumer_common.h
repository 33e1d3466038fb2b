// consumer_common.h — device-side constants and helpers shared by the solver-step kernels (resid.hip, step.hip,
// lbfgs.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace tg {

constexpr double kSideInf = 1e19;   // IPOPT's nlp_lower / upper_bound_inf: a side beyond it does not count
constexpr unsigned long long kNanBits = 0x7ff8000000000000ull;   // the canonical quiet NaN

// v >= +0.0 or NaN as a key that orders like the value, NaN (made canonical) above everything
__device__ inline unsigned long long v_bits(double v) { return v != v ? kNanBits : (unsigned long long)__double_as_longlong(v); }

}  // namespace tg
