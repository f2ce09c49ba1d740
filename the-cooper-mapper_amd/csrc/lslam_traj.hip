// lslam_traj.hip -- trajectory evaluation (include/lslam_c.h lslam_traj_*): map_evaluation/Evaluation.cpp:39-150 on arrays, and
// a rigidly aligned ATE the reference does not have.  Host code in fp64, plain C++: nothing here includes or calls HIP, so the
// file also compiles with a host compiler alone (tools/cpp/traj_eval_asan.cpp builds it that way under the sanitizers).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/lslam_c.h"

namespace lslam {
void set_error(const char *msg);  // lslam_api.hip (a stand-alone build supplies its own)
}

namespace {

// cyclic Jacobi on a symmetric 3x3 matrix: a <- diagonal, v <- eigenvector columns
void jacobi3(double a[3][3], double v[3][3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    const double off = std::fabs(a[0][1]) + std::fabs(a[0][2]) + std::fabs(a[1][2]);
    if (off == 0.0) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (a[p][q] == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
        const double root = std::sqrt(theta * theta + 1.0);
        const double t = theta >= 0.0 ? 1.0 / (theta + root) : -1.0 / (root - theta);
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        const int r = 3 - p - q;
        const double h = t * a[p][q];
        a[p][p] -= h;
        a[q][q] += h;
        a[p][q] = a[q][p] = 0.0;
        const double rp = c * a[r][p] - s * a[r][q], rq = s * a[r][p] + c * a[r][q];
        a[r][p] = a[p][r] = rp;
        a[r][q] = a[q][r] = rq;
        for (int k = 0; k < 3; ++k) {
          const double x = c * v[k][p] - s * v[k][q], y = s * v[k][p] + c * v[k][q];
          v[k][p] = x;
          v[k][q] = y;
        }
      }
  }
}

void cross3(const double a[3], const double b[3], double o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
bool normalise3(double a[3]) {
  const double n = std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
  if (!(n > 0.0) || !std::isfinite(n)) return false;
  for (int k = 0; k < 3; ++k) a[k] /= n;
  return true;
}

// Kabsch: R, t minimising sum |R e + t - r|^2 over the m pairs; false when the pairs do not fix a rotation
bool rigid_align(const std::vector<double> &e, const std::vector<double> &r, size_t m, double R[3][3], double t[3]) {
  if (m < 3) return false;
  double ce[3] = {0, 0, 0}, cr[3] = {0, 0, 0};
  for (size_t i = 0; i < m; ++i)
    for (int k = 0; k < 3; ++k) { ce[k] += e[3 * i + k]; cr[k] += r[3 * i + k]; }
  for (int k = 0; k < 3; ++k) { ce[k] /= (double)m; cr[k] /= (double)m; }
  double H[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};  // sum (e - ce)(r - cr)^T
  for (size_t i = 0; i < m; ++i)
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) H[a][b] += (e[3 * i + a] - ce[a]) * (r[3 * i + b] - cr[b]);
  // H = U S V^T: V and S^2 from H^T H, U's first two columns from H V / S, the third columns by cross products -- both bases
  // right-handed, so R = V U^T is a rotation (what the reflection case's diag(1, 1, -1) does)
  double A[3][3], V[3][3];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) A[a][b] = (H[0][a] * H[0][b] + H[1][a] * H[1][b]) + H[2][a] * H[2][b];
  jacobi3(A, V);
  int o[3] = {0, 1, 2};  // descending eigenvalues
  for (int a = 0; a < 2; ++a)
    for (int b = a + 1; b < 3; ++b)
      if (A[o[b]][o[b]] > A[o[a]][o[a]]) { const int x = o[a]; o[a] = o[b]; o[b] = x; }
  const double l0 = A[o[0]][o[0]], l1 = A[o[1]][o[1]];
  if (!(l0 > 0.0) || !std::isfinite(l0) || !(l1 > 1e-12 * l0)) return false;  // s1 <= 1e-6 s0: collinear
  double v[3][3], u[3][3];  // rows: the vectors
  for (int c = 0; c < 2; ++c) {
    for (int k = 0; k < 3; ++k) v[c][k] = V[k][o[c]];
    for (int k = 0; k < 3; ++k) u[c][k] = (H[k][0] * v[c][0] + H[k][1] * v[c][1]) + H[k][2] * v[c][2];
  }
  if (!normalise3(u[0])) return false;
  const double d = (u[1][0] * u[0][0] + u[1][1] * u[0][1]) + u[1][2] * u[0][2];
  for (int k = 0; k < 3; ++k) u[1][k] -= d * u[0][k];
  if (!normalise3(u[1])) return false;
  cross3(u[0], u[1], u[2]);
  cross3(v[0], v[1], v[2]);
  if (!normalise3(v[2])) return false;
  // H = sum_c s_c u_c v_c^T with u in the estimates' space: the rotation takes u_c to v_c
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) R[a][b] = (v[0][a] * u[0][b] + v[1][a] * u[1][b]) + v[2][a] * u[2][b];
  for (int a = 0; a < 3; ++a) t[a] = cr[a] - ((R[a][0] * ce[0] + R[a][1] * ce[1]) + R[a][2] * ce[2]);
  return true;
}

int bad(const char *what) {
  lslam::set_error(what);
  return LSLAM_ERR_INVALID;
}

}  // namespace

extern "C" {

void lslam_traj_default_params(lslam_traj_params *p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->gate = 10.0;  // Evaluation.cpp:64
  p->align = 0;
}
size_t lslam_sizeof_traj_params(void) { return sizeof(lslam_traj_params); }
size_t lslam_sizeof_traj_stats(void) { return sizeof(lslam_traj_stats); }

int lslam_traj_eval(const double *est_stamp, const double *est_xyz, size_t n_est, const double *ref_stamp, const double *ref_xyz,
                    size_t n_ref, const lslam_traj_params *params, lslam_traj_stats *stats) {
  lslam_traj_params P;
  lslam_traj_default_params(&P);
  if (params) P = *params;
  if (!stats) return bad("lslam_traj_eval: null stats");
  if ((n_est && (!est_stamp || !est_xyz)) || (n_ref && (!ref_stamp || !ref_xyz))) return bad("lslam_traj_eval: null array with samples");
  if (!(P.gate >= 0.0) || !std::isfinite(P.gate)) return bad("lslam_traj_eval: gate must be finite and >= 0 (0: no gate)");
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  std::memset(stats, 0, sizeof(*stats));
  std::vector<double> diff[4], dts, ue, ur;
  double mx[4] = {0.0, 0.0, 0.0, 0.0};
  int64_t gated = 0;
  for (size_t i = 0; i < n_est && n_ref; ++i) {
    const double now = est_stamp[i];
    double dt = -1.0;
    size_t cor = 0;
    for (size_t k = 0, j = n_ref - 1; k < n_ref; ++k, --j) {  // :44-51, from the newest sample backwards
      if (k == 0 || dt > std::fabs(now - ref_stamp[j])) {
        dt = std::fabs(now - ref_stamp[j]);
        cor = j;
      } else {
        break;
      }
    }
    const double dx = std::fabs(est_xyz[3 * i] - ref_xyz[3 * cor]), dy = std::fabs(est_xyz[3 * i + 1] - ref_xyz[3 * cor + 1]),
                 dz = std::fabs(est_xyz[3 * i + 2] - ref_xyz[3 * cor + 2]);
    const double dist = std::sqrt((dx * dx + dy * dy) + dz * dz);
    const double d4[4] = {dx, dy, dz, dist};
    for (int c = 0; c < 4; ++c) mx[c] = std::fmax(mx[c], d4[c]);  // :59-62, before the gate
    if (P.gate == 0.0 || dist <= P.gate) {
      for (int c = 0; c < 4; ++c) diff[c].push_back(d4[c]);
      dts.push_back(dt);
      for (int c = 0; c < 3; ++c) { ue.push_back(est_xyz[3 * i + c]); ur.push_back(ref_xyz[3 * cor + c]); }
    } else {
      ++gated;
    }
  }
  const size_t num = dts.size();
  stats->n_used = (int64_t)num;
  stats->n_gated = gated;
  for (int c = 0; c < 4; ++c) {
    stats->max[c] = mx[c];
    double mean = 0.0;
    for (size_t i = 0; i < num; ++i) mean += diff[c][i];
    mean = num ? mean / (double)num : qnan;
    double var = 0.0;
    for (size_t i = 0; i < num; ++i) var += (diff[c][i] - mean) * (diff[c][i] - mean);
    stats->mean[c] = mean;
    stats->var[c] = num >= 2 ? var / (double)(num - 1) : qnan;
  }
  double mdt = 0.0;
  for (size_t i = 0; i < num; ++i) mdt += dts[i];
  stats->mean_dt = num ? mdt / (double)num : qnan;
  stats->aligned = 0;
  stats->ate_rmse = qnan;
  for (int k = 0; k < 4; ++k) stats->T_align[5 * k] = 1.0;
  double R[3][3], t[3];
  if (P.align && rigid_align(ue, ur, num, R, t)) {
    double ss = 0.0;
    for (size_t i = 0; i < num; ++i) {
      double e2 = 0.0;
      for (int a = 0; a < 3; ++a) {
        const double w = (((R[a][0] * ue[3 * i] + R[a][1] * ue[3 * i + 1]) + R[a][2] * ue[3 * i + 2]) + t[a]) - ur[3 * i + a];
        e2 += w * w;
      }
      ss += e2;
    }
    stats->aligned = 1;
    stats->ate_rmse = std::sqrt(ss / (double)num);
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) stats->T_align[4 * a + b] = R[a][b];
      stats->T_align[4 * a + 3] = t[a];
    }
  }
  return LSLAM_OK;
}

}  // extern "C"
