// C++ drop-in check of the marginal covariances of SolverG2OT (include/lslam_solver_g2o.hpp) over the C ABI: marginals (with
// and without cross blocks), relativeCovariances, marginalStats, and the exception for a vertex out of range.
// argv[1]: a graph written by the test as text: "n_vertices n_edges ref max_iters", then per vertex 16 doubles (the 4x4 estimate,
// row-major), per edge "i j", 36 doubles (its information matrix) and 16 doubles (the relative pose), then "n_q" and the queried
// vertices.  The first vertex is fixed.  Prints what the test compares with the Python mirror on the same numbers:
//   COV <k> <36 doubles>        marginals(vertices)             CROSS <a> <b> <36 doubles>   ... its cross blocks
//   REL <k> <36 doubles>        relativeCovariances(ref, vertices)
//   STATS <columns> <panels> <iters_max> <coarse_used>           of the relativeCovariances call
//   REFUSED <1 if a vertex out of range threw and left the output vector as it was>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>

#include "lslam_solver_g2o.hpp"

struct Iso {
  double m[16];
  struct M { double *m; double &operator()(int r, int c) { return m[r * 4 + c]; } };
  M matrix() { return M{m}; }
  Iso() { for (int i = 0; i < 16; ++i) m[i] = (i % 5 == 0) ? 1.0 : 0.0; }
};
struct Mat6 { double v[36]; double operator()(int r, int c) const { return v[r * 6 + c]; } };
typedef pose_graph::SolverG2OT<Iso, Mat6> Solver;

static bool read_n(FILE *f, double *out, int n) {
  for (int k = 0; k < n; ++k)
    if (std::fscanf(f, "%lf", &out[k]) != 1) return false;
  return true;
}

static void print36(const double *b) {
  for (int k = 0; k < 36; ++k) std::printf(" %.17g", b[k]);
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int nv = 0, ne = 0, ref = 0, max_iters = 0;
  if (std::fscanf(f, "%d %d %d %d", &nv, &ne, &ref, &max_iters) != 4) return 2;
  try {
    Solver solver;
    std::vector<Solver::VertexSE3 *> v;
    if (nv == 0) {  // (no graph given: one vertex, so that the backend is asked for)
      Iso T;
      v.push_back(solver.add_se3_node(T));
    }
    for (int k = 0; k < nv; ++k) {
      Iso T;
      if (!read_n(f, T.m, 16)) return 2;
      v.push_back(solver.add_se3_node(T));
    }
    for (int k = 0; k < ne; ++k) {
      int i = 0, j = 0;
      Mat6 w;
      Iso Z;
      if (std::fscanf(f, "%d %d", &i, &j) != 2 || !read_n(f, w.v, 36) || !read_n(f, Z.m, 16)) return 2;
      solver.add_se3_edge(v[(size_t)i], v[(size_t)j], Z, w);
    }
    int nq = 0;
    std::vector<int> q;
    if (nv > 0 && std::fscanf(f, "%d", &nq) != 1) return 2;
    for (int k = 0; k < nq; ++k) {
      int x = 0;
      if (std::fscanf(f, "%d", &x) != 1) return 2;
      q.push_back(x);
    }
    if (nv == 0) q.push_back(0);
    std::fclose(f);
    lslam_pg_marginal_opts o = Solver::defaultMarginalOpts();
    o.max_iters = max_iters;
    std::vector<double> cov, cross, rel;
    solver.marginals(q, cov, &cross, &o);
    const size_t n = q.size();
    for (size_t k = 0; k < n; ++k) { std::printf("COV %zu", k); print36(&cov[k * 36]); }
    for (size_t a = 0; a < n; ++a)
      for (size_t b = 0; b < n; ++b) { std::printf("CROSS %zu %zu", a, b); print36(&cross[(a * n + b) * 36]); }
    solver.relativeCovariances(ref, q, rel, &o);
    for (size_t k = 0; k < n; ++k) { std::printf("REL %zu", k); print36(&rel[k * 36]); }
    const lslam_pg_marginal_stats &st = solver.marginalStats();
    std::printf("STATS %d %d %d %d\n", st.columns, st.panels, st.iters_max, st.coarse_used);
    int refused = 0;
    std::vector<double> keep(3, -7.25);
    try {
      std::vector<int> bad(1, (int)v.size());
      solver.marginals(bad, keep);
    } catch (const std::runtime_error &) {
      refused = keep.size() == 3 && keep[0] == -7.25;
    }
    std::printf("REFUSED %d\n", refused);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
