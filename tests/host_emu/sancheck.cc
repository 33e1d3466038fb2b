// TEST INFRASTRUCTURE ONLY — AddressSanitizer / UndefinedBehaviorSanitizer driver of the engine's host
// code (tests/test_sanitizers.py): the layout builder (towr2025_amd/csrc/layout.hip: variable maps, time
// grids, structure pass, CSR, tiles, slot tables, streaming tables, cost items) and the host instantiation
// of engine_math.h through the emulation (emu.hip), built host-only with the sanitizers. Input: the
// problem file format of oracle/sancheck.c. Built by `make sanitize`.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../towr2025_amd/csrc/layout.h"

extern "C" int emu_eval_ex(const towr_problem_desc_t* d, int n_data, const towr_data_t* data, const double* x, double* g,
                           double* v, char* err, int errlen);
extern "C" int emu_cost(const towr_problem_desc_t* d, const double* x, double* f, double* grad, char* err, int errlen);
extern "C" int emu_traj(const towr_problem_desc_t* d, const double* x, double dt, double* out, int max_rows);
extern "C" int emu_jac_products_ex(const towr_problem_desc_t* d, int n_data, const towr_data_t* data, const double* V,
                                   const double* P, const double* LAM, const double* Z0, double* Y, double* Z, double* Za);
extern "C" int emu_gn_direction_ex(const towr_problem_desc_t* d, int n_data, const towr_data_t* data, const double* V,
                                   const double* LAMP, const double* GR, const double* X, const double* XL, const double* XU,
                                   double rho, double mu, double tol, int ncg, double* D, double* SUM);

extern "C" int emu_tile_bounds_ex(const towr_problem_desc_t* d, int n_data, const towr_data_t* data, int64_t* out, char* err, int errlen);

extern "C" void emu_limb_sum(const double* v, int k, long long limbs[3], int* bad, double* value);

// The limb arithmetic (CostLimbEmit, limb_of, limb_value) on the boundary list of tests/test_costs.py, each entry
// alone, then all accepted ones together and 2047 of the largest accepted magnitude, in exactly sized heap buffers
// (shifts by the exponent are where undefined behaviour would hide). Returns 0 when every flag and sum is as expected.
static int limb_boundaries() {
  const double inf = std::numeric_limits<double>::infinity(), top = std::nextafter(0x1p65, 0.0);
  const double ok[] = {0x1p-60, -0x1p-60, std::nextafter(0x1p-60, 0.0), 0x1p-61, 4.9e-324, -2.2e-308, 0.0, -0.0,
                       top, -top, 0x1p-18, -0x1p24, 1.0, -3.5e-7, 0x1p64, 0x1p-19 - 0x1p-60};
  const double refused[] = {0x1p65, -0x1p65, inf, -inf, std::nan(""), 1e30, 1.7e308};
  for (double x : ok) {
    std::vector<double> v(1, x);
    std::vector<long long> l(3);
    int bad = -1; double val = 0.0;
    emu_limb_sum(v.data(), 1, l.data(), &bad, &val);
    if (bad != 0) return 1;
    if (std::fabs(x) >= 0x1p-60 && !(std::fabs(val - x) <= 0x1p-60)) return 2;
    if (std::fabs(x) < 0x1p-60 && (l[0] || l[1] || l[2] || val != 0.0)) return 3;
  }
  for (double x : refused) {
    std::vector<double> v(1, x);
    std::vector<long long> l(3);
    int bad = -1; double val = 0.0;
    emu_limb_sum(v.data(), 1, l.data(), &bad, &val);
    if (bad != 1 || l[0] || l[1] || l[2]) return 4;
  }
  std::vector<double> all(ok, ok + sizeof ok / sizeof ok[0]);
  std::vector<long long> l(3);
  int bad = -1; double val = 0.0;
  emu_limb_sum(all.data(), (int)all.size(), l.data(), &bad, &val);
  if (bad != 0) return 5;
  std::vector<double> many(2047, top);
  emu_limb_sum(many.data(), (int)many.size(), l.data(), &bad, &val);
  const long long lim = 1ll << 53;
  if (bad != 0 || l[0] >= lim || l[1] >= lim || l[2] >= lim || l[0] < 0 || l[1] < 0 || l[2] <= 0) return 6;
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s problem.bin\n", argv[0]); return 2; }
  if (int rc = limb_boundaries()) { std::fprintf(stderr, "limb boundaries: check %d\n", rc); return 8; }
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
  tg::Layout L;
  std::string err;
  if (int rc = tg::build_layout_ex(d, nd, data.data(), L, err)) { std::fprintf(stderr, "layout: %s\n", err.c_str()); return 4; }
  std::vector<double> x = L.x0, g((size_t)L.m + 1), v((size_t)L.nnz + 1), grad((size_t)L.n);
  char e[256];
  if (emu_eval_ex(&d, nd, data.data(), x.data(), g.data(), v.data(), e, sizeof e)) { std::fprintf(stderr, "emu: %s\n", e); return 5; }
  double fv = 0.0;
  if (d.n_costs && nd == 0 && emu_cost(&d, x.data(), &fv, grad.data(), e, sizeof e)) { std::fprintf(stderr, "cost: %s\n", e); return 6; }
  const int rows = emu_traj(&d, x.data(), 0.05, nullptr, 0);
  std::vector<double> tr((size_t)(rows > 0 ? rows : 1) * (19 + 25 * d.robot.n_ee));
  emu_traj(&d, x.data(), 0.05, tr.data(), rows);
  // the product tables' walk (build_jprod's chunks, segments and by-column lists) on the values above, in
  // exactly-sized buffers: P = x, LAM = g, Z0 = x
  std::vector<double> vx(v.begin(), v.begin() + (size_t)L.nnz), lam(g.begin(), g.begin() + (size_t)L.m);
  std::vector<double> y((size_t)L.m), z((size_t)L.n), za((size_t)L.n);
  if (emu_jac_products_ex(&d, nd, data.data(), vx.data(), x.data(), lam.data(), x.data(), y.data(), z.data(), za.data())) {
    std::fprintf(stderr, "products: layout\n");
    return 7;
  }
  // the GN direction's walk (emu_gn_direction_ex) on the same values, two CG steps, in exactly-sized buffers:
  // LAMP = g, GR = x, the layout's variable bounds at X = x when it has them (else every column free)
  {
    const bool vb = L.x_lower.size() == (size_t)L.n && L.x_upper.size() == (size_t)L.n;
    std::vector<double> dir((size_t)L.n), sum(6);
    if (emu_gn_direction_ex(&d, nd, data.data(), vx.data(), lam.data(), x.data(), vb ? x.data() : nullptr,
                            vb ? L.x_lower.data() : nullptr, vb ? L.x_upper.data() : nullptr, 10.0, 1e-3, 0.0, 2, dir.data(), sum.data())) {
      std::fprintf(stderr, "gn direction: layout\n");
      return 9;
    }
  }
  // the tile tables' walk (emu_tile_bounds_ex: every lane's slot groups, positions, dummy slots and LDS regions as the
  // emitters address them; its hit counters and Dynamic scratch are exactly sized), eight counts and a message
  {
    std::vector<int64_t> counts(8);
    std::vector<char> msg(256);
    if (int rc = emu_tile_bounds_ex(&d, nd, data.data(), counts.data(), msg.data(), (int)msg.size())) {
      std::fprintf(stderr, "tile bounds: check %d: %s\n", rc, msg.data());
      return 10;
    }
    if (counts[5] != L.nnz) { std::fprintf(stderr, "tile bounds: the tiles cover %lld of %lld values\n", (long long)counts[5], (long long)L.nnz); return 10; }
  }
  std::printf("ok n=%d m=%d nnz=%lld\n", L.n, L.m, (long long)L.nnz);
  return 0;
}
