// traj_eval_asan.cpp -- stand-alone driver of the host-only trajectory evaluation (csrc/lslam_traj.hip, plain C++), for a
// sanitizer run on the CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ the-cooper-mapper_amd/csrc/lslam_traj.hip
//       tools/cpp/traj_eval_asan.cpp -o traj_eval_asan && ./traj_eval_asan       (one command line)
// Covers empty inputs, single samples, the all-gated case, the collinear and the too-short alignment, and a general case whose
// planted transform must come back.  Prints "traj_eval ok" and exits 0, or says what failed and exits 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lslam_c.h"

namespace lslam {
static std::string g_error;
void set_error(const char *msg) { g_error = msg; }  // the library's lives in lslam_api.hip
}  // namespace lslam

static int fails = 0;
#define CHECK(cond)                                             \
  do {                                                          \
    if (!(cond)) {                                              \
      std::printf("FAILED %s (line %d)\n", #cond, __LINE__);    \
      ++fails;                                                  \
    }                                                           \
  } while (0)

int main() {
  lslam_traj_params P;
  std::memset(&P, 0xA5, sizeof(P));
  lslam_traj_default_params(&P);
  CHECK(P.gate == 10.0 && P.align == 0 && P.reserved[0] == 0 && P.reserved[2] == 0);
  lslam_traj_stats st;

  // empty inputs, with and without alignment
  P.align = 1;
  CHECK(lslam_traj_eval(nullptr, nullptr, 0, nullptr, nullptr, 0, &P, &st) == LSLAM_OK);
  CHECK(st.n_used == 0 && st.n_gated == 0 && std::isnan(st.mean[0]) && std::isnan(st.var[3]) && st.max[3] == 0.0 && st.aligned == 0);
  const double t1[1] = {1.0}, p1[3] = {1.0, 2.0, 3.0}, r1[3] = {1.5, 2.0, 3.0};
  CHECK(lslam_traj_eval(t1, p1, 1, nullptr, nullptr, 0, &P, &st) == LSLAM_OK && st.n_used == 0);
  CHECK(lslam_traj_eval(nullptr, nullptr, 0, t1, r1, 1, nullptr, &st) == LSLAM_OK && st.n_used == 0);
  // refusals
  CHECK(lslam_traj_eval(t1, p1, 1, t1, r1, 1, &P, nullptr) == LSLAM_ERR_INVALID);
  CHECK(lslam_traj_eval(nullptr, p1, 1, t1, r1, 1, &P, &st) == LSLAM_ERR_INVALID);
  lslam_traj_params bad = P;
  bad.gate = -1.0;
  CHECK(lslam_traj_eval(t1, p1, 1, t1, r1, 1, &bad, &st) == LSLAM_ERR_INVALID && lslam::g_error.find("gate") != std::string::npos);
  // single samples
  CHECK(lslam_traj_eval(t1, p1, 1, t1, r1, 1, &P, &st) == LSLAM_OK);
  CHECK(st.n_used == 1 && st.mean[0] == 0.5 && st.mean[3] == 0.5 && std::isnan(st.var[0]) && st.mean_dt == 0.0 && st.aligned == 0 &&
        std::isnan(st.ate_rmse) && st.T_align[0] == 1.0 && st.T_align[15] == 1.0 && st.T_align[3] == 0.0);

  // a general case: estimates = a rotation about z and a shift of the references
  const int n = 50;
  std::vector<double> ts(n), ref(3 * n), est(3 * n), far(3 * n), line_e(3 * n), line_r(3 * n);
  const double c = std::cos(0.3), s = std::sin(0.3);
  for (int i = 0; i < n; ++i) {
    ts[i] = 0.1 * i;
    const double x = 0.5 * i, y = 3.0 * std::sin(0.2 * i), z = 0.01 * i * i;
    ref[3 * i] = x; ref[3 * i + 1] = y; ref[3 * i + 2] = z;
    est[3 * i] = c * x - s * y + 1.0; est[3 * i + 1] = s * x + c * y - 2.0; est[3 * i + 2] = z + 0.5;
    for (int k = 0; k < 3; ++k) far[3 * i + k] = ref[3 * i + k] + 100.0;
    line_e[3 * i] = 1.0 * i; line_e[3 * i + 1] = 2.0 * i; line_e[3 * i + 2] = -0.5 * i;
    for (int k = 0; k < 3; ++k) line_r[3 * i + k] = line_e[3 * i + k] + 1.0 + k;
  }
  P.gate = 0.0;
  CHECK(lslam_traj_eval(ts.data(), est.data(), n, ts.data(), ref.data(), n, &P, &st) == LSLAM_OK);
  CHECK(st.n_used == n && st.aligned == 1 && st.ate_rmse < 1e-9);
  CHECK(std::fabs(st.T_align[0] - c) < 1e-12 && std::fabs(st.T_align[1] - s) < 1e-12 && std::fabs(st.T_align[4] + s) < 1e-12);
  // all gated: the maxima still move
  P.gate = 10.0;
  CHECK(lslam_traj_eval(ts.data(), far.data(), n, ts.data(), ref.data(), n, &P, &st) == LSLAM_OK);
  CHECK(st.n_used == 0 && st.n_gated == n && st.max[3] > 100.0 && std::isnan(st.mean[3]) && st.aligned == 0);
  // collinear pairs and two pairs: no alignment
  P.gate = 0.0;
  CHECK(lslam_traj_eval(ts.data(), line_e.data(), n, ts.data(), line_r.data(), n, &P, &st) == LSLAM_OK);
  CHECK(st.n_used == n && st.aligned == 0 && std::isnan(st.ate_rmse));
  CHECK(lslam_traj_eval(ts.data(), est.data(), 2, ts.data(), ref.data(), 2, &P, &st) == LSLAM_OK && st.n_used == 2 && st.aligned == 0);
  // estimates outside the references' span, references outside the estimates'
  CHECK(lslam_traj_eval(ts.data() + 40, est.data() + 120, 10, ts.data(), ref.data(), 5, &P, &st) == LSLAM_OK && st.n_used == 10);

  if (fails) return 1;
  std::printf("traj_eval ok\n");
  return 0;
}
