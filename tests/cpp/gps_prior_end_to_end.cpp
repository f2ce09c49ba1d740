// C++ drop-in check of the unary constraints of SolverG2OT (include/lslam_solver_g2o.hpp) over the C ABI:
// add_se3_prior_xyz_edge / add_se3_prior_quat_edge / add_se3_prior_pose_edge, add_robust_kernel on a prior, priorWeights,
// setFixFirstNode and a save / load round trip.
// argv[1]: a graph written by the test as text: "n_vertices n_edges n_priors fix_first", then per vertex 16 doubles (the 4x4
// estimate, row-major), per edge "i j", 36 doubles (its information matrix) and 16 doubles (the relative pose), per prior
// "vertex form kernel size" -- form 0: 3 doubles (xyz) and a 3x3 information; form 1: a 4x4 pose and a 6x6 information;
// form 2: 4 doubles (quaternion x y z w) and a 3x3 information -- kernel "NONE" / "Huber" / "Cauchy" / "DCS" with its size.
// argv[2]: where to save the optimised graph.  Prints what the test compares with the Python mirror on the same numbers:
//   ITER <LM iterations>   CHI2 <final chi2>
//   PWEIGHT <prior> <weight>              priorWeights()
//   POS <vertex> <x> <y> <z>              the optimised positions
//   LOADED <vertices> <priors>            a second solver after load(argv[2])
//   LITER <LM iterations>   LPOS <vertex> <x> <y> <z>    ... optimised again (kernels are not part of the file)
//   REFUSED <1 if an unknown kernel type and a missing prior were refused>
// argv[3] (optional): a drive for pose_graph::Graph (include/lslam_loop_closure.hpp) with its GPS switch on: "n sigma_xy sigma_z
// kernel size", then per frame 16 doubles (the odometry pose) and 3 doubles (the UTM fix).  Every frame goes through
// add_frame(..., utm_coord, nullptr) and one optimize(); no loops (an empty loop_source).  Prints
//   GPASS <frame> <priors in the solver> <1 if the graph frame has been moved onto the fixes>
//   GORIGIN <x> <y> <z>                    utm_origin
//   GWEIGHT <fix> <weight>                 gpsWeights()
//   GPOS <keyframe> <x> <y> <z>            the keyframes' estimates
//   GTF <16 doubles>                       tf_odom2graph
//   GOFF <1 if the same frames without the switch added no prior and left the first vertex's estimate the odometry's>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <vector>

#include "lslam_loop_closure.hpp"
#include "lslam_solver_g2o.hpp"

struct Iso {
  double m[16];
  struct M { double *m; double &operator()(int r, int c) { return m[r * 4 + c]; } };
  M matrix() { return M{m}; }
  Iso() { for (int i = 0; i < 16; ++i) m[i] = (i % 5 == 0) ? 1.0 : 0.0; }
};
struct Mat6 { double v[36]; double operator()(int r, int c) const { return v[r * 6 + c]; } };
struct Mat3 { double v[9]; double operator()(int r, int c) const { return v[r * 3 + c]; } };
struct Vec3 { double v[3]; double operator()(int i) const { return v[i]; } };
struct Quat {
  double q[4];
  double x() const { return q[0]; }
  double y() const { return q[1]; }
  double z() const { return q[2]; }
  double w() const { return q[3]; }
};
typedef pose_graph::SolverG2OT<Iso, Mat6> Solver;

static bool read_n(FILE *f, double *out, int n) {
  for (int k = 0; k < n; ++k)
    if (std::fscanf(f, "%lf", &out[k]) != 1) return false;
  return true;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int nv = 0, ne = 0, np = 0, fix_first = 1;
  if (std::fscanf(f, "%d %d %d %d", &nv, &ne, &np, &fix_first) != 4) return 2;
  try {
    Solver solver;
    solver.setFixFirstNode(fix_first != 0);
    std::vector<Solver::VertexSE3 *> v;
    std::vector<Solver::EdgeSE3Prior *> priors;
    if (nv == 0) {  // (no graph given: one vertex with one prior, so that the backend is asked for)
      Iso T;
      v.push_back(solver.add_se3_node(T));
      const Vec3 z = {{1.0, 2.0, 3.0}};
      const Mat3 w = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};
      priors.push_back(solver.add_se3_prior_xyz_edge(v[0], z, w));
    }
    for (int k = 0; k < nv; ++k) {
      Iso T;
      if (!read_n(f, T.m, 16)) return 2;
      v.push_back(solver.add_se3_node(T));
    }
    for (int e = 0; e < ne; ++e) {
      int i = 0, j = 0;
      Mat6 info;
      Iso Z;
      if (std::fscanf(f, "%d %d", &i, &j) != 2 || !read_n(f, info.v, 36) || !read_n(f, Z.m, 16)) return 2;
      solver.add_se3_edge(v[(size_t)i], v[(size_t)j], Z, info);
    }
    for (int p = 0; p < np; ++p) {
      int vertex = 0, form = 0;
      char kernel[32];
      double size = 1.0;
      if (std::fscanf(f, "%d %d %31s %lf", &vertex, &form, kernel, &size) != 4) return 2;
      Solver::EdgeSE3Prior *pr = nullptr;
      if (form == 0) {
        Vec3 z;
        Mat3 w;
        if (!read_n(f, z.v, 3) || !read_n(f, w.v, 9)) return 2;
        pr = solver.add_se3_prior_xyz_edge(v[(size_t)vertex], z, w);
      } else if (form == 1) {
        Iso Z;
        Mat6 w;
        if (!read_n(f, Z.m, 16) || !read_n(f, w.v, 36)) return 2;
        pr = solver.add_se3_prior_pose_edge(v[(size_t)vertex], Z, w);
      } else {
        Quat q;
        Mat3 w;
        if (!read_n(f, q.q, 4) || !read_n(f, w.v, 9)) return 2;
        pr = solver.add_se3_prior_quat_edge(v[(size_t)vertex], q, w);
      }
      if (std::string(kernel) != "NONE") solver.add_robust_kernel(pr, kernel, size);
      priors.push_back(pr);
    }
    std::fclose(f);
    solver.optimize();
    std::printf("ITER %d\nCHI2 %.17g\n", solver.lastStats().iterations, solver.lastStats().chi2_final);
    const std::vector<double> w = solver.priorWeights();
    for (size_t k = 0; k < w.size(); ++k) std::printf("PWEIGHT %zu %.17g\n", k, w[k]);
    for (size_t k = 0; k < v.size(); ++k) {
      Iso T = v[k]->estimate();
      std::printf("POS %zu %.17g %.17g %.17g\n", k, T.m[3], T.m[7], T.m[11]);
    }
    bool refused = false;
    try {
      solver.add_robust_kernel(priors[0], "Tukey", 1.0);
    } catch (const std::invalid_argument &) {
      refused = true;
    }
    try {
      Solver::EdgeSE3Prior none{(int)priors.size()};
      solver.add_robust_kernel(&none, "Huber", 1.0);
      refused = false;
    } catch (const std::invalid_argument &) {
    }
    solver.save(argv[2]);
    Solver again;
    again.load(argv[2]);
    std::printf("LOADED %d %zu\n", again.is_first ? 0 : nv, again.numPriors());
    again.optimize();
    std::printf("LITER %d\n", again.lastStats().iterations);
    for (int k = 0; k < nv; ++k) {
      Solver::VertexSE3 vk{k, &again};
      Iso T = vk.estimate();
      std::printf("LPOS %d %.17g %.17g %.17g\n", k, T.m[3], T.m[7], T.m[11]);
    }
    std::printf("REFUSED %d\n", refused ? 1 : 0);
    if (argc > 3) {
      FILE *gf = std::fopen(argv[3], "r");
      int n = 0;
      double sxy = 0.0, sz = 0.0, ksize = 1.0;
      char kname[32];
      if (!gf || std::fscanf(gf, "%d %lf %lf %31s %lf", &n, &sxy, &sz, kname, &ksize) != 5) return 2;
      lslam_ctx *ctx = nullptr;
      if (lslam_ctx_create(0, &ctx) != LSLAM_OK) {
        std::fprintf(stderr, "backend unavailable: %s\n", lslam_last_error());
        return 1;
      }
      {
        pose_graph::Graph graph(ctx), off(ctx);
        graph.gps_sigma_xy = sxy;
        graph.gps_sigma_z = sz;
        graph.gps_robust_kernel = kname;
        graph.gps_robust_kernel_size = ksize;
        const auto no_loops = [](const std::vector<pose_graph::KeyFrame::Ptr> &, const std::deque<pose_graph::KeyFrame::Ptr> &,
                                 std::vector<pose_graph::Loop::Ptr> &) {};
        graph.loop_source = no_loops;
        off.loop_source = no_loops;
        const std::vector<float> none;
        pose_graph::Mat4d first;
        for (int k = 0; k < n; ++k) {
          pose_graph::Mat4d odom;
          double fix[3];
          if (!read_n(gf, odom.m, 16) || !read_n(gf, fix, 3)) return 2;
          if (k == 0) first = odom;
          if (!graph.add_frame(odom, none, none, fix, nullptr) || !off.add_frame(odom, none, none, fix, nullptr)) {
            std::fprintf(stderr, "frame %d was not taken as a keyframe\n", k);
            return 1;
          }
          if (graph.optimize(1000) < 0 || off.optimize(1000) < 0) {
            std::fprintf(stderr, "Graph::optimize failed: %s %s\n", graph.lastError().c_str(), off.lastError().c_str());
            return 1;
          }
          std::printf("GPASS %d %zu %d\n", k, graph.numPriors(), graph.gps_aligned ? 1 : 0);
        }
        std::fclose(gf);
        std::printf("GORIGIN %.17g %.17g %.17g\n", graph.utm_origin[0], graph.utm_origin[1], graph.utm_origin[2]);
        const std::vector<double> &gw = graph.gpsWeights();
        for (size_t k = 0; k < gw.size(); ++k) std::printf("GWEIGHT %zu %.17g\n", k, gw[k]);
        for (size_t k = 0; k < graph.keyframes.size(); ++k)
          std::printf("GPOS %zu %.17g %.17g %.17g\n", k, graph.keyframes[k]->estimate(0, 3), graph.keyframes[k]->estimate(1, 3),
                      graph.keyframes[k]->estimate(2, 3));
        std::printf("GTF");
        for (int q = 0; q < 16; ++q) std::printf(" %.17g", graph.tf_odom2graph.m[q]);
        bool same = off.numPriors() == 0 && !off.gps_aligned && !off.has_utm_origin && off.gpsWeights().empty();
        for (int q = 0; q < 16 && !off.keyframes.empty(); ++q) same = same && off.keyframes[0]->estimate.m[q] == first.m[q];
        std::printf("\nGOFF %d\n", same ? 1 : 0);
      }
      lslam_ctx_destroy(ctx);
    }
  } catch (const std::exception &ex) {
    std::fprintf(stderr, "backend unavailable: %s\n", ex.what());
    return 1;
  }
  return 0;
}
