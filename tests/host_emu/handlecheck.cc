// TEST INFRASTRUCTURE ONLY — AddressSanitizer / UndefinedBehaviorSanitizer / LeakSanitizer driver of the handle's
// lifetimes (tests/test_sanitizers.py): the real library's host code (towr_gpu.hip, auglag.hip, layout.hip built with
// the sanitizers, the kernel files plain) through the C-ABI, without a GPU. Every handle is layout-only (device -1),
// and one creation with device 0 walks the failure path behind the layout and the fusion setup: the process hides
// the GPUs from itself, so that path is the same on a machine that has one. Input: the problem file format of
// sancheck.cc. Built by `make sanitize`.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/towr_gpu.h"

namespace {
int g_line = 0;
#define CHECK(cond)                                                                                          \
  do {                                                                                                       \
    if (!(cond)) { std::fprintf(stderr, "handlecheck.cc:%d: %s\n  last error: %s\n", __LINE__, #cond, towr_gpu_last_error(nullptr)); return __LINE__; } \
    g_line = __LINE__;                                                                                       \
  } while (0)

// every accessor a layout-only handle answers, the refusals of the entry points that need a device, and the
// null-argument refusals
int exercise(towr_gpu_handle h, const towr_problem_desc_t& d) {
  int32_t n = 0, m = 0;
  int64_t nnz = 0;
  CHECK(towr_gpu_sizes(h, &n, &m, &nnz) == TOWR_OK && n > 0 && m >= 0 && nnz >= 0);
  CHECK(towr_gpu_sizes(nullptr, &n, &m, &nnz) == TOWR_ERR_INVALID);
  std::vector<int32_t> ir((size_t)nnz + 1), jc((size_t)nnz + 1), col((size_t)nnz + 1), row((size_t)nnz + 1), cidx((size_t)nnz + 1);
  std::vector<int64_t> rp((size_t)m + 1), cp((size_t)n + 1);
  CHECK(towr_gpu_jac_structure(h, ir.data(), jc.data()) == TOWR_OK);
  CHECK(towr_gpu_jac_structure(h, nullptr, jc.data()) == TOWR_ERR_INVALID);
  CHECK(towr_gpu_jac_csr(h, rp.data(), col.data()) == TOWR_OK && rp[(size_t)m] == nnz);
  CHECK(towr_gpu_jac_csr(h, nullptr, col.data()) == TOWR_ERR_INVALID);
  CHECK(towr_gpu_jac_csc(h, cp.data(), row.data(), cidx.data()) == TOWR_OK && cp[(size_t)n] == nnz);
  std::vector<double> x((size_t)n), lo((size_t)std::max(n, m) + 1), up((size_t)std::max(n, m) + 1);
  CHECK(towr_gpu_initial_x(h, x.data()) == TOWR_OK);
  CHECK(towr_gpu_initial_x(h, nullptr) == TOWR_ERR_INVALID);
  CHECK(towr_gpu_initial_x_for(h, &d.init, &d.terrain, x.data()) == TOWR_OK);
  CHECK(towr_gpu_initial_x_for(h, nullptr, &d.terrain, x.data()) == TOWR_ERR_INVALID);
  for (int32_t i = 0; i < d.n_constraints; ++i) {
    int32_t kind = -1, ee = 0, r0 = -1, rows = -1;
    CHECK(towr_gpu_constraint_info(h, i, &kind, &ee, &r0, &rows) == TOWR_OK && kind == d.constraints[i].kind && r0 >= 0 && r0 + rows <= m);
  }
  CHECK(towr_gpu_constraint_info(h, d.n_constraints, nullptr, nullptr, nullptr, nullptr) == TOWR_ERR_INVALID);
  for (int32_t i = 0; i < d.n_varsets; ++i) {
    int32_t kind = -1, ee = 0, c0 = -1, cnt = -1;
    CHECK(towr_gpu_varset_info(h, i, &kind, &ee, &c0, &cnt) == TOWR_OK && c0 >= 0 && c0 + cnt <= n);
  }
  CHECK(towr_gpu_varset_info(h, -1, nullptr, nullptr, nullptr, nullptr) == TOWR_ERR_INVALID);
  // (a description with an EELinear or LinearEquality set and no TOWR_DATA_BOUNDS entry is refused by name)
  const int rb = towr_gpu_constraint_bounds(h, lo.data(), up.data());
  CHECK(rb == TOWR_OK || (rb == TOWR_ERR_INVALID && towr_gpu_last_error(h)[0] != 0));
  CHECK(towr_gpu_constraint_bounds_for(h, &d.init, &d.terrain, lo.data(), up.data()) == rb);
  CHECK(towr_gpu_constraint_bounds(h, nullptr, up.data()) == TOWR_ERR_INVALID);
  CHECK(towr_gpu_variable_bounds(h, lo.data(), up.data()) == TOWR_OK);
  CHECK(towr_gpu_variable_bounds_with(h, 0, nullptr, lo.data(), up.data()) == TOWR_OK);
  CHECK(towr_gpu_variable_bounds(h, lo.data(), nullptr) == TOWR_ERR_INVALID);
  for (int32_t k = 0; k < towr_gpu_num_kernels(); ++k) {
    const char* name = nullptr;
    int32_t nt = -1;
    int64_t bytes = -1;
    CHECK(towr_gpu_kernel_info(h, k, &name, &nt, &bytes) == TOWR_OK && name && nt >= 0 && bytes >= 0);
  }
  CHECK(towr_gpu_kernel_info(h, towr_gpu_num_kernels(), nullptr, nullptr, nullptr) == TOWR_ERR_INVALID);
  for (int32_t k = 0; k < towr_gpu_num_kernels() - 2; ++k) CHECK(towr_gpu_kernel_path(h, k) >= -1);
  std::vector<int32_t> launches(16);
  const int nl = towr_gpu_step_launches(h, launches.data(), (int32_t)launches.size());
  CHECK(nl >= 1 && nl <= (int)launches.size() && towr_gpu_step_launches(h, nullptr, 0) == nl);
  int32_t ns = 0, ncols = 0;
  CHECK(towr_gpu_trajectory_size(h, 0.05, &ns, &ncols) == TOWR_OK && ns > 0 && ncols > 0);
  CHECK(towr_gpu_trajectory_size(h, 0.0, &ns, &ncols) == TOWR_ERR_INVALID);
  int64_t outside = -1;
  CHECK(towr_gpu_pattern_outside(h, x.data(), &outside) == TOWR_OK && outside >= 0);
  CHECK(towr_gpu_algorithmic_bytes_per_call(h) > 0);
  CHECK(towr_gpu_set_products_chunk(h, 0) == TOWR_OK);
  CHECK(towr_gpu_set_cost_grid(h, 3) == TOWR_OK && towr_gpu_cost_grid(h, 0) == 3 && towr_gpu_cost_grid(h, 1) == 3);
  CHECK(towr_gpu_set_cost_grid(h, -1) == TOWR_ERR_INVALID && towr_gpu_cost_grid(h, 1) == 3);
  CHECK(towr_gpu_set_cost_grid(h, 0) == TOWR_OK && towr_gpu_cost_grid(h, 1) == 1);

  // what needs a device is refused, and the handle stays whole
  std::vector<double> g((size_t)m + 1), v((size_t)nnz + 1), tr((size_t)ns * ncols);
  double f = 0.0;
  CHECK(towr_gpu_eval_g(h, x.data(), g.data()) == TOWR_ERR_NO_DEVICE);
  CHECK(std::strstr(towr_gpu_last_error(h), "layout-only") != nullptr);
  CHECK(towr_gpu_eval_jac_values(h, x.data(), v.data()) == TOWR_ERR_NO_DEVICE);
  CHECK(towr_gpu_eval_g_jac(h, x.data(), g.data(), v.data()) == TOWR_ERR_NO_DEVICE);
  CHECK(towr_gpu_eval_g_keep_jac(h, x.data(), g.data()) == TOWR_ERR_NO_DEVICE);
  CHECK(towr_gpu_eval_jac_values_kept(h, x.data(), v.data()) == TOWR_ERR_NO_DEVICE);
  CHECK(towr_gpu_eval_f(h, x.data(), &f) == TOWR_ERR_NO_DEVICE);
  CHECK(towr_gpu_eval_grad_f(h, x.data(), lo.data()) == TOWR_ERR_NO_DEVICE);
  CHECK(towr_gpu_eval_batch(h, 1, x.data(), g.data(), v.data()) == TOWR_ERR_NO_DEVICE);
  CHECK(towr_gpu_eval_batch_device(h, 1, x.data(), n, g.data(), m, v.data(), nnz, 1, 1, nullptr) == TOWR_ERR_NO_DEVICE);
  CHECK(towr_gpu_eval_cost_batch_device(h, 1, x.data(), n, &f, nullptr, 0, nullptr) == TOWR_ERR_NO_DEVICE);
  CHECK(towr_gpu_sample_trajectory(h, x.data(), 0.05, tr.data()) == TOWR_ERR_NO_DEVICE);
  CHECK(towr_gpu_jac_vec_batch_device(h, 1, v.data(), nnz, x.data(), n, g.data(), m, nullptr) == TOWR_ERR_NO_DEVICE);
  CHECK(towr_gpu_set_batch_terrain(h, 1, &d.terrain) == TOWR_ERR_NO_DEVICE);
  CHECK(towr_gpu_register_host(h, x.data(), (int64_t)(sizeof(double) * x.size())) == TOWR_ERR_NO_DEVICE);
  CHECK(towr_gpu_unregister_host(h, x.data()) == TOWR_ERR_INVALID);   // (was never registered)
  CHECK(towr_gpu_eval_g(h, nullptr, g.data()) == TOWR_ERR_INVALID);
  CHECK(towr_gpu_eval_batch(h, -1, x.data(), g.data(), v.data()) == TOWR_ERR_INVALID);
  CHECK(towr_gpu_register_host(h, nullptr, 8) == TOWR_ERR_INVALID);
  CHECK(towr_gpu_sizes(h, &n, &m, &nnz) == TOWR_OK);
  return 0;
}

int run(const towr_problem_desc_t& d, const std::vector<towr_data_t>& data) {
  const int32_t nd = (int32_t)data.size();
  towr_gpu_handle h = nullptr;
  CHECK(towr_gpu_create_ex(nullptr, 0, nullptr, -1, &h) == TOWR_ERR_INVALID);
  CHECK(towr_gpu_create_ex(&d, nd, data.data(), -1, nullptr) == TOWR_ERR_INVALID);
  CHECK(towr_gpu_create_ex(&d, 1, nullptr, -1, &h) == TOWR_ERR_INVALID && h == nullptr);
  CHECK(towr_gpu_destroy(nullptr) == TOWR_OK);

  // a layout-only handle: the accessors, the refusals, destruction (with a SoftConstraint term: the child handle too)
  CHECK(towr_gpu_create_ex(&d, nd, data.data(), -1, &h) == TOWR_OK && h != nullptr);
  if (int rc = exercise(h, d)) return rc;
  CHECK(towr_gpu_destroy(h) == TOWR_OK);

  // device 0 with no GPU in sight: the failure path behind the layout, the fusion setup and the soft child
  h = reinterpret_cast<towr_gpu_handle>(&h);
  const int rdev = towr_gpu_create_ex(&d, nd, data.data(), 0, &h);
  if (rdev == TOWR_OK) {   // (a GPU the process could not hide from itself: nothing to check on this path)
    CHECK(towr_gpu_destroy(h) == TOWR_OK);
  } else {
    CHECK(rdev == TOWR_ERR_NO_DEVICE && h == nullptr && std::strstr(towr_gpu_last_error(nullptr), "no HIP device") != nullptr);
  }

  // SoftConstraint terms: the bounds entry missing, then with a wrong count — refused with the child already built
  for (int32_t i = 0; i < nd; ++i) {
    if (data[(size_t)i].kind != TOWR_DATA_SOFT_BOUNDS) continue;
    std::vector<towr_data_t> without(data);
    without.erase(without.begin() + i);
    std::vector<towr_data_t> wrong(data);
    wrong[(size_t)i].count -= 1;
    for (const std::vector<towr_data_t>* bad : {&without, &wrong}) {
      h = reinterpret_cast<towr_gpu_handle>(&h);
      CHECK(towr_gpu_create_ex(&d, (int32_t)bad->size(), bad->data(), -1, &h) == TOWR_ERR_INVALID && h == nullptr);
      const std::string msg = towr_gpu_last_error(nullptr);
      CHECK(msg == "SoftConstraint term " + std::to_string(data[(size_t)i].index) +
                       ": bounds (side data TOWR_DATA_SOFT_BOUNDS, lower then upper) missing or not 2 x the set's rows");
    }
  }
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s problem.bin\n", argv[0]); return 2; }
  // lifetimes of the host code are what is checked: the process never opens a GPU, also where one is present
  setenv("HIP_VISIBLE_DEVICES", "-1", 1);
  setenv("ROCR_VISIBLE_DEVICES", "-1", 1);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  towr_problem_desc_t d;
  int32_t nd = 0;
  if (std::fread(&d, sizeof d, 1, f) != 1 || std::fread(&nd, 4, 1, f) != 1 || nd < 0 || nd > 64) return 3;
  std::vector<towr_data_t> data((size_t)nd);
  std::vector<std::vector<double>> keep((size_t)nd);
  for (int i = 0; i < nd; ++i) {
    if (std::fread(&data[i].kind, 4, 1, f) != 1 || std::fread(&data[i].index, 4, 1, f) != 1 || std::fread(&data[i].count, 8, 1, f) != 1) return 3;
    keep[i].resize((size_t)data[i].count);
    if (data[i].count && std::fread(keep[i].data(), sizeof(double), (size_t)data[i].count, f) != (size_t)data[i].count) return 3;
    data[i].data = keep[i].data();
  }
  std::fclose(f);
  if (int rc = run(d, data)) return rc > 255 ? 1 : rc;
  std::printf("ok handles (last check line %d)\n", g_line);
  return 0;
}
