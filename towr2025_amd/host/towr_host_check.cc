// towr_host_check — C++ host driver over the C-ABI, used by the tests (tests/test_cpp_host.py).
// It builds a BASELINE configuration through the C++ NlpFormulation mirror, creates the engine and
// walks the IPOPT callback sequence of one iteration:
//   get_nlp_info -> eval_jac_g(structure) -> eval_f(x, new_x = true) -> eval_grad_f(x, false)
//   -> eval_g(x, false) -> eval_jac_g(x, false)
// and dumps everything to a binary file:
//   desc bytes | n m (int32) nnz (int64) | x0[n] | iRow[nnz] jCol[nnz] | (device >= 0) g[m] values[nnz] f grad[n]
// and (device >= 0) the trajectory of x0 sampled at 0.01 s as SaveTrajectoryToCSV writes it, to <out.bin>.csv
// usage: towr_host_check <anymal|anymal_costs|anymal_rotvec|anymal_gait|biped|biped_next|hopper> <out.bin> [device (default -1: layout only)]
//        towr_host_check <cfg> --zerocopy [device] [timed iterations]
//   the zero-copy Jacobian of NlpCallbacks (towr_gpu.hpp) against the engine's own evaluation, bit for bit: IPOPT's
//   values array stable across calls (TNLPAdapter's jac_g_), g before J and J before g, a values array that moves
//   between calls, and the array after finalize_solution; then per-iteration timings (eval_g + eval_jac_g through the
//   callbacks, and eval_jac_g alone) against the cached path (one fused evaluation into the page-locked cache + the
//   nnz-value copy into IPOPT's array). Prints one line "zerocopy ok ..." or fails with a message.
//        towr_host_check <cfg> --products [device] [problems]
//   evaluates a batch of the configuration on the device, applies J p and J^T lam there (separate calls and the fused
//   entry) and compares them with a host loop over the CSR pattern; prints "products ok ... largest |err|/bound x"
//   and exits non-zero when a bound is exceeded.
//        towr_host_check <cfg> --bounds [relaxed dims, e.g. 2 or 0,2]
//   prints the C++ mirror's TOWR_DATA_BOUNDS entries ("data <constraint> <count> <values...>") and, from a layout-only
//   engine created with them, the constraint bounds ("row <i> <lower> <upper>"), every double as %.17g.
//        towr_host_check <cfg> --varbounds [plain|rich] [device (default -1: layout only)]
//   prints the C++ mirror's TOWR_DATA_VAR_BOUNDS entries ("data <variable set> <count> <values...>") and, from an
//   engine created with them, the variable bounds ("col <j> <lower> <upper>"), every double as %.17g.
//        towr_host_check <cfg> --residual [device] [problems]
//   evaluates a batch on the device, runs the residual kernel (the handle's bounds, random multipliers) and the fused
//   merit-and-gradient entry, and compares them with a host loop over the bounds; prints "residual ok ..." and exits
//   non-zero on a mismatch.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "nlp_formulation.hpp"
#include "towr_gpu.hpp"

using namespace towr_gpu;

namespace {

double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v.empty() ? 0.0 : v[v.size() / 2];
}

int zerocopy_check(const towr_problem_desc_t& d, int device, int iters) {
  Engine e(d, device);
  const int n = e.GetNumberOfOptimizationVariables(), m = e.GetNumberOfConstraints();
  const int nnz = (int)e.GetNumberOfJacobianNonzeros();
  const std::vector<double> x0 = e.GetVariableValues();
  std::vector<std::vector<double>> xs;
  for (int k = 0; k < 3; ++k) {   // x0 and two deterministic perturbations
    std::vector<double> x = x0;
    for (int i = 0; i < n; ++i) x[i] += 0.01 * k * std::sin(0.37 * i + k);
    xs.push_back(x);
  }
  std::vector<std::vector<double>> gr(3, std::vector<double>(m)), vr(3, std::vector<double>(nnz));
  for (int k = 0; k < 3; ++k) e.EvalConstraintsAndJacobian(xs[k].data(), gr[k].data(), vr[k].data());   // the engine's own (staged) evaluation
  auto same = [&](const std::vector<double>& a, const std::vector<double>& b, const char* what, int k) {
    if (std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) != 0) {
      std::fprintf(stderr, "zerocopy: %s differs at x %d\n", what, k);
      return false;
    }
    return true;
  };
  NlpCallbacks nlp(e);
  std::vector<double> g(m), jac_g(nnz);   // IPOPT's TNLPAdapter arrays: allocated once per solve
  for (int rep = 0; rep < 2; ++rep)
    for (int k = 0; k < 3; ++k) {
      std::fill(jac_g.begin(), jac_g.end(), NAN);
      bool ok;
      if (rep == 0) ok = nlp.eval_g(n, xs[k].data(), true, m, g.data()) && nlp.eval_jac_g(n, xs[k].data(), false, m, nnz, nullptr, nullptr, jac_g.data());
      else ok = nlp.eval_jac_g(n, xs[k].data(), true, m, nnz, nullptr, nullptr, jac_g.data()) && nlp.eval_g(n, xs[k].data(), false, m, g.data());
      if (!ok) { std::fprintf(stderr, "zerocopy: callback failed: %s\n", towr_gpu_last_error(e.handle())); return 1; }
      if (!same(g, gr[k], rep ? "g (J first)" : "g", k) || !same(jac_g, vr[k], rep ? "values (J first)" : "values", k)) return 1;
      // (a small Jacobian is copied from the page-locked cache when g came first: no registration then)
      if (!nlp.values_zero_copy() && !(nlp.small_jacobian() && rep == 0)) {
        std::fprintf(stderr, "zerocopy: IPOPT's array was not registered\n");
        return 1;
      }
    }
  if (nlp.values_registrations() != 1) { std::fprintf(stderr, "zerocopy: %d registrations of a stable array\n", nlp.values_registrations()); return 1; }
  for (int k = 0; k < 3; ++k) {   // a values array that moves between calls
    std::vector<double> moved(nnz, NAN);
    if (!nlp.eval_g(n, xs[k].data(), true, m, g.data()) || !nlp.eval_jac_g(n, xs[k].data(), false, m, nnz, nullptr, nullptr, moved.data())) return 1;
    if (!same(moved, vr[k], "values (moved array)", k)) return 1;
    nlp.finalize_solution();   // (the vector is freed next: release its registration first)
  }
  const int want_reg = nlp.small_jacobian() ? 1 : 4;   // (g first: a small Jacobian is copied from the cache)
  if (nlp.values_registrations() != want_reg) {
    std::fprintf(stderr, "zerocopy: %d registrations, expected %d\n", nlp.values_registrations(), want_reg);
    return 1;
  }
  // timings: IPOPT's per-iteration pair through the callbacks, against the cached path of round 4 (one fused
  // evaluation into page-locked g / values caches, then both copied into IPOPT's arrays)
  using clk = std::chrono::steady_clock;
  auto us = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
  std::vector<double> t_pair, t_jac, t_old, t_oldjac;
  std::vector<double> cg(m), cv(nnz);
  const bool pg = e.RegisterHost(cg.data(), cg.size() * sizeof(double)) == TOWR_OK;
  const bool pv = e.RegisterHost(cv.data(), cv.size() * sizeof(double)) == TOWR_OK;
  for (int it = 0; it < iters + 10; ++it) {
    const double* x = xs[it % 3].data();
    auto t0 = clk::now();
    nlp.eval_g(n, x, true, m, g.data());
    auto t1 = clk::now();
    nlp.eval_jac_g(n, x, false, m, nnz, nullptr, nullptr, jac_g.data());
    auto t2 = clk::now();
    e.EvalConstraintsAndJacobian(x, cg.data(), cv.data());
    std::copy(cg.begin(), cg.end(), g.begin());
    auto t3 = clk::now();
    std::copy(cv.begin(), cv.end(), jac_g.begin());
    auto t4 = clk::now();
    if (it >= 10) { t_pair.push_back(us(t0, t2)); t_jac.push_back(us(t1, t2)); t_old.push_back(us(t2, t4)); t_oldjac.push_back(us(t3, t4)); }
  }
  if (pg) e.UnregisterHost(cg.data());
  if (pv) e.UnregisterHost(cv.data());
  std::printf("zerocopy ok n=%d m=%d nnz=%d iters=%d path %s pair_us %.1f jac_us %.1f cached_pair_us %.1f cached_copy_us %.1f\n", n,
              m, nnz, iters, nlp.small_jacobian() ? "cached" : "device-kept", median(t_pair), median(t_jac), median(t_old), median(t_oldjac));
  return 0;
}

// --products: a batch of B perturbations of x0 evaluated on the device, both products applied there (the separate
// calls and the fused entry, which must agree bit for bit), compared with a host loop over towr_gpu_jac_csr in long
// double under the a-priori bound 2 gamma_k S (k terms, S = sum |v| |vec|, gamma_k = k u / (1 - k u), u = 2^-53).
struct DevBuf {
  double* p = nullptr;
  size_t n = 0;
  explicit DevBuf(size_t doubles) : n(doubles) { if (hipMalloc(reinterpret_cast<void**>(&p), sizeof(double) * std::max<size_t>(n, 1)) != hipSuccess) p = nullptr; }
  ~DevBuf() { if (p) (void)hipFree(p); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  bool put(const std::vector<double>& h) { return p && hipMemcpy(p, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice) == hipSuccess; }
  bool get(std::vector<double>& h) const { h.resize(n); return p && hipMemcpy(h.data(), p, sizeof(double) * n, hipMemcpyDeviceToHost) == hipSuccess; }
};

int products_check(const towr_problem_desc_t& d, int device, int B) {
  Engine e(d, device);
  const int n = e.GetNumberOfOptimizationVariables(), m = e.GetNumberOfConstraints();
  const int64_t nnz = e.GetNumberOfJacobianNonzeros();
  std::vector<int64_t> rp((size_t)m + 1), cp((size_t)n + 1);
  std::vector<int32_t> col((size_t)nnz), crow((size_t)nnz), cidx((size_t)nnz);
  e.GetJacobianCsr(rp.data(), col.data());
  e.GetJacobianCsc(cp.data(), crow.data(), cidx.data());
  const std::vector<double> x0 = e.GetVariableValues();
  std::vector<double> X((size_t)B * n), P((size_t)B * n), LAM((size_t)B * m);
  for (int b = 0; b < B; ++b) {
    for (int i = 0; i < n; ++i) { X[(size_t)b * n + i] = x0[i] + 0.01 * (b + 1) * std::sin(0.37 * i + b); P[(size_t)b * n + i] = std::cos(1.3 * i + 0.7 * b); }
    for (int i = 0; i < m; ++i) LAM[(size_t)b * m + i] = std::sin(0.9 * i + 1.1 * b) * (1 + i % 3);
  }
  DevBuf dX(X.size()), dP(P.size()), dL(LAM.size()), dG((size_t)B * m), dV((size_t)B * nnz), dY((size_t)B * m), dZ((size_t)B * n),
      dG2((size_t)B * m), dY2((size_t)B * m), dZ2((size_t)B * n);
  if (!dX.put(X) || !dP.put(P) || !dL.put(LAM) || !dG.p || !dV.p || !dY.p || !dZ.p || !dG2.p || !dY2.p || !dZ2.p) {
    std::fprintf(stderr, "products: device allocation failed\n");
    return 1;
  }
  e.SetProductsChunk(3);
  if (e.EvalBatchDevice(B, dX.p, n, dG.p, m, dV.p, nnz, nullptr) || e.JacVecBatchDevice(B, dV.p, nnz, dP.p, n, dY.p, m, nullptr) ||
      e.JacTVecBatchDevice(B, dV.p, nnz, dL.p, m, dZ.p, n, false, nullptr) ||
      e.EvalProductsBatchDevice(B, dX.p, n, dG2.p, m, dL.p, m, dZ2.p, n, false, dP.p, n, dY2.p, m, nullptr) ||
      hipDeviceSynchronize() != hipSuccess) {
    std::fprintf(stderr, "products: %s\n", towr_gpu_last_error(e.handle()));
    return 1;
  }
  std::vector<double> G, V, Y, Z, G2, Y2, Z2;
  if (!dG.get(G) || !dV.get(V) || !dY.get(Y) || !dZ.get(Z) || !dG2.get(G2) || !dY2.get(Y2) || !dZ2.get(Z2)) return 1;
  auto same = [](const std::vector<double>& a, const std::vector<double>& b) { return std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0; };
  if (!same(G, G2) || !same(Y, Y2) || !same(Z, Z2)) { std::fprintf(stderr, "products: the fused entry differs from the separate calls\n"); return 1; }
  const long double u = std::ldexp(1.0L, -53);
  double worst = 0.0;
  auto judge = [&](double got, long double ref, long double S, int64_t k) {
    if (k == 0) { if (got != 0.0) worst = INFINITY; return; }
    const long double bound = 2 * (k * u / (1 - k * u)) * S;
    const long double err = std::fabs((long double)got - ref);
    worst = std::max(worst, bound > 0 ? (double)(err / bound) : (err > 0 ? (double)INFINITY : 0.0));
  };
  for (int b = 0; b < B; ++b) {
    const double *v = V.data() + (size_t)b * nnz, *p = P.data() + (size_t)b * n, *l = LAM.data() + (size_t)b * m;
    for (int r = 0; r < m; ++r) {
      long double s = 0, S = 0;
      for (int64_t k = rp[r]; k < rp[r + 1]; ++k) { const long double t = (long double)v[k] * p[col[k]]; s += t; S += std::fabs(t); }
      judge(Y[(size_t)b * m + r], s, S, rp[r + 1] - rp[r]);
    }
    for (int j = 0; j < n; ++j) {
      long double s = 0, S = 0;
      for (int64_t q = cp[j]; q < cp[j + 1]; ++q) { const long double t = (long double)v[cidx[q]] * l[crow[q]]; s += t; S += std::fabs(t); }
      judge(Z[(size_t)b * n + j], s, S, cp[j + 1] - cp[j]);
    }
  }
  std::printf("products %s n=%d m=%d nnz=%lld B=%d largest |err|/bound %.3f\n", worst <= 1.0 ? "ok" : "FAILED", n, m, (long long)nnz, B, worst);
  return worst <= 1.0 ? 0 : 1;
}

std::vector<towr_data_t> as_side_data(const std::vector<BoundsEntry>& bd) {
  std::vector<towr_data_t> out;
  for (const BoundsEntry& e : bd) out.push_back(towr_data_t{TOWR_DATA_BOUNDS, e.index, (int64_t)e.values.size(), e.values.data()});
  return out;
}

int bounds_dump(const NlpFormulation& f) {
  const std::vector<BoundsEntry> bd = f.BoundsData();
  for (const BoundsEntry& e : bd) {
    std::printf("data %d %zu", e.index, e.values.size());
    for (double v : e.values) std::printf(" %.17g", v);
    std::printf("\n");
  }
  Engine e(f.MakeDesc(), -1, as_side_data(bd));
  const int m = e.GetNumberOfConstraints();
  std::vector<double> lo(m), up(m);
  e.GetConstraintBounds(lo.data(), up.data());
  for (int i = 0; i < m; ++i) std::printf("row %d %.17g %.17g\n", i, lo[i], up[i]);
  return 0;
}

// --varbounds: the variable-bound knobs of the variant set on `f` (the same values as tests/test_var_bounds.py):
//   plain  stance tracking off: the start / goal bounds of nlp_formulation.cc:136-151, 234-235, 279-280, 309-340;
//   rich   stance-position tracking on every foot, stance-rpy tracking on foot 0, the base pitch pinned, the final
//          base z free, an exact base-linear waypoint and a toleranced base-angular one.
int varbounds_dump(NlpFormulation f, const std::string& variant, int device) {
  Parameters& P = f.params_;
  if (variant == "rich") {
    P.constrain_base_pitch_ = true;
    P.base_pitch_target_ = 0.05;
    P.bounds_final_lin_pos_ = {0, 1};
    P.base_lin_waypoints_.push_back({0.52, 0, {2}, {0.0, 0.0, 0.5}, {0.0, 0.0, 0.0}});
    P.base_ang_waypoints_.push_back({0.25, 1, {0, 2}, {0.1, 0.0, -0.1}, {0.05, 0.0, 0.025}});
    for (int ee = 0; ee < P.GetEECount(); ++ee) {
      std::vector<std::array<double, 3>> pos;
      for (int k = 0; k < (int)P.ee_phase_durations_[ee].size(); ++k) pos.push_back({0.125 * k + 0.0625 * ee, -0.25 * ee, 0.0});
      P.ee_stance_position_.push_back(pos);
    }
    P.ee_stance_rpy_.push_back({});
    for (int k = 0; k < (int)P.ee_phase_durations_[0].size(); ++k) P.ee_stance_rpy_[0].push_back({0.0, 0.03125 * k, 0.5});
  } else {
    P.enable_stance_tracking = false;
  }
  const std::vector<BoundsEntry> vb = f.VarBoundsData();
  std::vector<towr_data_t> data;
  for (const BoundsEntry& e : vb) {
    std::printf("data %d %zu", e.index, e.values.size());
    for (double v : e.values) std::printf(" %.17g", v);
    std::printf("\n");
    data.push_back(towr_data_t{TOWR_DATA_VAR_BOUNDS, e.index, (int64_t)e.values.size(), e.values.data()});
  }
  Engine e(f.MakeDesc(), device, data);
  const int n = e.GetNumberOfOptimizationVariables();
  std::vector<double> lo(n), up(n), lo2(n), up2(n);
  e.GetVariableBounds(lo.data(), up.data());
  e.GetVariableBoundsWith(data, lo2.data(), up2.data());
  if (lo != lo2 || up != up2) { std::fprintf(stderr, "varbounds: GetVariableBoundsWith differs from GetVariableBounds\n"); return 1; }
  for (int j = 0; j < n; ++j) std::printf("col %d %.17g %.17g\n", j, lo[j], up[j]);
  return 0;
}

// --residual: B perturbations of x0; the residual kernel's outputs against a host loop: the maxima, the arg max and the
// per-set maxima bit for bit, the two sums under 2 gamma_m S (+ 8 u S for phi's per-term roundings), lam+ within
// 8 u rho (|g| + |lam| / rho + |c|); then the fused entry against the separate calls, bit for bit.
int residual_check(const NlpFormulation& f, int device, int B) {
  const std::vector<BoundsEntry> bd = f.BoundsData();
  const towr_problem_desc_t d = f.MakeDesc();
  Engine e(d, device, as_side_data(bd));
  const int n = e.GetNumberOfOptimizationVariables(), m = e.GetNumberOfConstraints(), ns = d.n_constraints, lds = 4 + ns;
  const int64_t nnz = e.GetNumberOfJacobianNonzeros();
  std::vector<double> lo(m), up(m);
  e.GetConstraintBounds(lo.data(), up.data());
  std::vector<int32_t> row0(ns + 1, m);
  for (int s = 0; s < ns; ++s) { int32_t k, ee, rows; e.GetConstraintInfo(s, &k, &ee, &row0[s], &rows); }
  const std::vector<double> x0 = e.GetVariableValues();
  const double rho = 10.0;
  std::vector<double> X((size_t)B * n), LAM((size_t)B * m);
  for (int b = 0; b < B; ++b) {
    for (int i = 0; i < n; ++i) X[(size_t)b * n + i] = x0[i] + 0.01 * b * std::sin(0.37 * i + b);
    for (int i = 0; i < m; ++i) LAM[(size_t)b * m + i] = std::sin(0.9 * i + 1.1 * b) * (1 + i % 3);
  }
  DevBuf dX(X.size()), dL(LAM.size()), dG((size_t)B * m), dV((size_t)B * nnz), dLP((size_t)B * m), dS((size_t)B * lds), dZ((size_t)B * n),
      dG2((size_t)B * m), dLP2((size_t)B * m), dS2((size_t)B * lds), dZ2((size_t)B * n);
  if (!dX.put(X) || !dL.put(LAM) || !dG.p || !dV.p || !dLP.p || !dS.p || !dZ.p || !dG2.p || !dLP2.p || !dS2.p || !dZ2.p) {
    std::fprintf(stderr, "residual: device allocation failed\n");
    return 1;
  }
  e.SetProductsChunk(3);
  if (e.EvalBatchDevice(B, dX.p, n, dG.p, m, dV.p, nnz, nullptr) ||
      e.ResidualBatchDevice(B, dG.p, m, nullptr, nullptr, 0, dL.p, m, rho, dLP.p, m, dS.p, lds, nullptr) ||
      e.JacTVecBatchDevice(B, dV.p, nnz, dLP.p, m, dZ.p, n, false, nullptr) ||
      e.EvalAuglagBatchDevice(B, dX.p, n, nullptr, nullptr, 0, dL.p, m, rho, dG2.p, m, dLP2.p, m, dS2.p, lds, dZ2.p, n, false, nullptr) ||
      hipDeviceSynchronize() != hipSuccess) {
    std::fprintf(stderr, "residual: %s\n", towr_gpu_last_error(e.handle()));
    return 1;
  }
  std::vector<double> G, LP, S, Z, G2, LP2, S2, Z2;
  if (!dG.get(G) || !dLP.get(LP) || !dS.get(S) || !dZ.get(Z) || !dG2.get(G2) || !dLP2.get(LP2) || !dS2.get(S2) || !dZ2.get(Z2)) return 1;
  auto same = [](const std::vector<double>& a, const std::vector<double>& b) { return std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0; };
  if (!same(G, G2) || !same(LP, LP2) || !same(S, S2) || !same(Z, Z2)) { std::fprintf(stderr, "residual: the fused entry differs from the separate calls\n"); return 1; }
  const long double u = std::ldexp(1.0L, -53), gam = 2 * (m * u / (1 - m * u));
  int bad = 0;
  double worst = 0.0;
  for (int b = 0; b < B; ++b) {
    const double *g = G.data() + (size_t)b * m, *lam = LAM.data() + (size_t)b * m, *lp = LP.data() + (size_t)b * m, *sm = S.data() + (size_t)b * lds;
    std::vector<double> smax(ns, 0.0);
    double vmax = 0.0, arg = -1.0;
    long double sv = 0, phi = 0, aphi = 0;
    int set = 0;
    for (int i = 0; i < m; ++i) {
      while (i >= row0[set + 1]) ++set;
      const bool hl = lo[i] > -1e19, hu = up[i] < 1e19;
      double v = 0.0;
      if (hl && lo[i] - g[i] > v) v = lo[i] - g[i];
      if (hu && g[i] - up[i] > v) v = g[i] - up[i];
      if (v > vmax) { vmax = v; arg = i; }
      smax[set] = std::max(smax[set], v);
      sv += v;
      const double t = g[i] + lam[i] / rho;
      double c = t;
      if (hl && c < lo[i]) c = lo[i];
      if (hu && c > up[i]) c = up[i];
      const double r = t - c;
      const long double term = 0.5L * rho * r * r - 0.5L * lam[i] * lam[i] / rho;
      phi += term; aphi += std::fabs(term);
      const double tol = 8 * (double)u * rho * (std::fabs(g[i]) + std::fabs(lam[i]) / rho + std::fabs(c));
      if (!(std::fabs(lp[i] - rho * r) <= tol)) ++bad;
    }
    if (std::memcmp(&sm[0], &vmax, 8) || sm[2] != arg) ++bad;
    for (int s = 0; s < ns; ++s) if (std::memcmp(&sm[4 + s], &smax[s], 8)) ++bad;
    const long double e1 = std::fabs((long double)sm[1] - sv), b1 = gam * sv;
    const long double e3 = std::fabs((long double)sm[3] - phi), b3 = (gam + 8 * u) * aphi;
    if (!(e1 <= b1) || !(e3 <= b3)) ++bad;
    if (b1 > 0) worst = std::max(worst, (double)(e1 / b1));
    if (b3 > 0) worst = std::max(worst, (double)(e3 / b3));
  }
  std::printf("residual %s n=%d m=%d sets=%d B=%d mismatches %d largest sum |err|/bound %.3f\n", bad ? "FAILED" : "ok", n, m, ns, B, bad, worst);
  return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s <anymal|biped|hopper> <out.bin> [device]\n", argv[0]); return 2; }
  const std::string cfg = argv[1];
  const int device = argc > 3 ? std::atoi(argv[3]) : -1;
  const bool zc = std::string(argv[2]) == "--zerocopy", pr = std::string(argv[2]) == "--products";
  const bool bo = std::string(argv[2]) == "--bounds", rs = std::string(argv[2]) == "--residual";
  NlpFormulation f = (cfg == "anymal" || cfg == "anymal_costs" || cfg == "anymal_rotvec" || cfg == "anymal_gait") ? AnymalTrot()
                     : (cfg == "biped" || cfg == "biped_next") ? BipedWalk() : MonopedHopper();
  if (cfg == "anymal_gait") {   // BASELINE configs[3]: stairs, phase-duration optimisation
    f.terrain_ = HeightMap::MakeTerrain(HeightMap::StairsID);
    f.params_.OptimizePhaseDurations();
  }
  if (cfg == "biped_next") {   // SURVEY §8(f) kinds: Torque, TerrainHard, EELinear (tests/configs.py)
    f.params_.constraints_.push_back(Parameters::Torque);
    f.params_.constraints_.push_back(Parameters::TerrainHard);
    Parameters::EELinearConstraintDef a, b;
    a.terms = {{0, 1, 1.0}, {1, 1, 1.0}};
    a.tolerance = 0.5;
    b.terms = {{0, 2, 0.5}, {1, 0, -1.0}, {0, 2, 0.5}};
    b.target = 1; b.deriv = 1; b.tolerance = 1.0; b.dt = 0.05;
    f.params_.ee_linear_constraints_ = {a, b};
  }
  if (cfg == "anymal_rotvec") f.params_.angular_rep_ = Parameters::RotationVector;
  if (cfg == "anymal_costs") {   // every cost kind (tests/configs.py _with_costs)
    f.params_.costs_ = {{Parameters::ForcesCostID, 1e-3}, {Parameters::EEMotionCostID, 0.5},
                        {Parameters::EnergyCostID, 1e-4}, {Parameters::AngMomCostID, 0.1}};
    f.params_.enable_swing_ee_base_pos_tracking = true;
  }
  try {
    if (bo) {
      for (const char* q = argc > 3 ? argv[3] : ""; *q; ++q)
        if (*q >= '0' && *q <= '2') f.params_.rom_swing_relax_dims_.push_back(*q - '0');
      return bounds_dump(f);
    }
    if (std::string(argv[2]) == "--varbounds") return varbounds_dump(f, argc > 3 ? argv[3] : "plain", argc > 4 ? std::atoi(argv[4]) : -1);
    if (rs) return residual_check(f, device < 0 ? 0 : device, argc > 4 ? std::max(1, std::atoi(argv[4])) : 5);
    const towr_problem_desc_t d = f.MakeDesc();
    if (zc) return zerocopy_check(d, device < 0 ? 0 : device, argc > 4 ? std::atoi(argv[4]) : 200);
    if (pr) return products_check(d, device < 0 ? 0 : device, argc > 4 ? std::max(1, std::atoi(argv[4])) : 7);
    Engine e(d, device);
    NlpCallbacks nlp(e);
    int n = 0, m = 0, nnz = 0;
    nlp.get_nlp_info(n, m, nnz);
    std::vector<double> x = e.GetVariableValues();
    std::vector<int> iRow(nnz), jCol(nnz);
    if (!nlp.eval_jac_g(n, x.data(), true, m, nnz, iRow.data(), jCol.data(), nullptr)) { std::fprintf(stderr, "structure failed\n"); return 1; }
    FILE* fp = std::fopen(argv[2], "wb");
    if (!fp) return 1;
    std::fwrite(&d, sizeof(d), 1, fp);
    const int32_t nm[2] = {n, m};
    const int64_t nz = nnz;
    std::fwrite(nm, sizeof(nm), 1, fp);
    std::fwrite(&nz, sizeof(nz), 1, fp);
    std::fwrite(x.data(), sizeof(double), x.size(), fp);
    std::fwrite(iRow.data(), sizeof(int), iRow.size(), fp);
    std::fwrite(jCol.data(), sizeof(int), jCol.size(), fp);
    if (device >= 0) {
      std::vector<double> g(m), v(nnz), grad(n);
      double obj = 0.0;
      if (!nlp.eval_f(n, x.data(), true, obj) || !nlp.eval_grad_f(n, x.data(), false, grad.data()) ||
          !nlp.eval_g(n, x.data(), false, m, g.data()) ||
          !nlp.eval_jac_g(n, x.data(), false, m, nnz, nullptr, nullptr, v.data())) {
        std::fprintf(stderr, "evaluation failed: %s\n", towr_gpu_last_error(e.handle()));
        std::fclose(fp);
        return 1;
      }
      std::fwrite(g.data(), sizeof(double), g.size(), fp);
      std::fwrite(v.data(), sizeof(double), v.size(), fp);
      std::fwrite(&obj, sizeof(double), 1, fp);
      std::fwrite(grad.data(), sizeof(double), grad.size(), fp);
      // the trajectory export of x (SaveTrajectoryToCSV), to <out>.csv
      if (!SaveTrajectoryToCSV(e, x.data(), std::string(argv[2]) + ".csv", 0.01)) { std::fprintf(stderr, "csv export failed\n"); return 1; }
    }
    std::fclose(fp);
    std::printf("%s: n=%d m=%d nnz=%d%s\n", cfg.c_str(), n, m, nnz, device >= 0 ? " (evaluated on the GPU)" : " (layout only)");
  } catch (const std::exception& ex) {
    std::fprintf(stderr, "error: %s\n", ex.what());
    return 1;
  }
  return 0;
}
