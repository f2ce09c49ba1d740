// C++ drop-in check of the robust-kernel additions: SolverG2OT::add_robust_kernel / edgeWeights (include/lslam_solver_g2o.hpp)
// and Graph::loop_robust_kernel / loop_robust_kernel_size / loopWeights (include/lslam_loop_closure.hpp) over the C ABI.
// Reads a graph written by the test as text: "n_vertices n_edges", then per vertex 16 doubles (the 4x4 estimate, row-major),
// then per edge "i j is_loop", 6 doubles (the diagonal of its information matrix) and 16 doubles (the relative pose).
// argv[2]: kernel type put on every loop edge ("NONE", "Huber", "Cauchy", "DCS"), argv[3]: its size.  Prints what the test
// compares with the Python mirror driven with the same matrices:
//   ITER <LM iterations>
//   WEIGHT <edge index> <weight>            one line per loop edge
//   POS <vertex> <x> <y> <z>                the optimised positions
// then the same graph through pose_graph::Graph: the vertices' 4x4 as odometry frames (add_frame), the loop edges handed
// over through Graph::loop_source, loop_robust_kernel / loop_robust_kernel_size set, one optimize():
//   GITER <LM iterations>   GLOOPS <loops found>
//   GWEIGHT <loop index> <weight>           Graph::loopWeights(), aligned with Graph::loops
//   GPOS <keyframe> <x> <y> <z>             the keyframes' estimates
//   REFUSED <1 if an unknown kernel type was refused by both mirrors>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <exception>
#include <memory>
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
typedef pose_graph::SolverG2OT<Iso, Mat6> Solver;

static bool read_iso(FILE *f, Iso &T) {
  for (int k = 0; k < 16; ++k)
    if (std::fscanf(f, "%lf", &T.m[k]) != 1) return false;
  return true;
}

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  const std::string kernel = argv[2];
  const double size = std::atof(argv[3]);
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int nv = 0, ne = 0;
  if (std::fscanf(f, "%d %d", &nv, &ne) != 2) return 2;
  try {
    Solver solver;
    std::vector<Solver::VertexSE3 *> v;
    std::vector<int> loop_edges;
    std::vector<Iso> frames, loop_rel;
    std::vector<int> loop_i, loop_j;
    if (nv == 0) {  // (no graph given: one vertex, so that the backend is asked for)
      Iso T;
      v.push_back(solver.add_se3_node(T));
    }
    for (int k = 0; k < nv; ++k) {
      Iso T;
      if (!read_iso(f, T)) return 2;
      v.push_back(solver.add_se3_node(T));
      frames.push_back(T);
    }
    for (int e = 0; e < ne; ++e) {
      int i = 0, j = 0, is_loop = 0;
      Mat6 info{};
      Iso Z;
      if (std::fscanf(f, "%d %d %d", &i, &j, &is_loop) != 3) return 2;
      for (int k = 0; k < 6; ++k)
        if (std::fscanf(f, "%lf", &info.v[k * 7]) != 1) return 2;
      if (!read_iso(f, Z)) return 2;
      Solver::EdgeSE3 *edge = solver.add_se3_edge(v[(size_t)i], v[(size_t)j], Z, info);
      if (is_loop) {
        solver.add_robust_kernel(edge, kernel, size);
        loop_edges.push_back(edge->index);
        loop_i.push_back(i);
        loop_j.push_back(j);
        loop_rel.push_back(Z);
      }
    }
    std::fclose(f);
    solver.optimize();
    std::printf("ITER %d\n", solver.lastStats().iterations);
    const std::vector<double> w = solver.edgeWeights();
    for (size_t k = 0; k < loop_edges.size(); ++k) std::printf("WEIGHT %d %.17g\n", loop_edges[k], w[(size_t)loop_edges[k]]);
    for (size_t k = 0; k < v.size(); ++k) {
      Iso T = v[k]->estimate();
      std::printf("POS %d %.17g %.17g %.17g\n", (int)k, T.m[3], T.m[7], T.m[11]);
    }
    bool refused = false;
    if (ne > 0) {
      Solver::EdgeSE3 first{0};
      try {
        solver.add_robust_kernel(&first, "Tukey", 1.0);
      } catch (const std::invalid_argument &) {
        refused = true;
      }
    }
    // the Graph mirror: its switches exist, an empty graph has no loops and no weights, an unknown kernel type is an error
    lslam_ctx *ctx = nullptr;
    if (lslam_ctx_create(0, &ctx) != LSLAM_OK) {
      std::fprintf(stderr, "backend unavailable: %s\n", lslam_last_error());
      return 1;
    }
    {
      pose_graph::Graph graph(ctx);
      graph.loop_robust_kernel = kernel;
      graph.loop_robust_kernel_size = size;
      const bool empty_ok = graph.optimize() == 0 && graph.loopWeights().empty() && graph.loops.empty();
      graph.loop_robust_kernel = "Tukey";
      refused = refused && empty_ok && graph.optimize() == -1;
      graph.loop_robust_kernel = "DCS";
      graph.loop_robust_kernel_size = 0.0;
      refused = refused && graph.optimize() == -1;
    }
    if (!frames.empty()) {  // the scenario through Graph, its loops through the seam
      pose_graph::Graph graph(ctx, 0, (int)frames.size());
      graph.loop_robust_kernel = kernel;
      graph.loop_robust_kernel_size = size;
      const std::vector<float> none;
      for (size_t k = 0; k < frames.size(); ++k) {
        pose_graph::Mat4d odom;
        for (int q = 0; q < 16; ++q) odom.m[q] = frames[k].m[q];
        if (!graph.add_frame(odom, none, none)) {
          std::fprintf(stderr, "frame %zu was not taken as a keyframe\n", k);
          return 1;
        }
      }
      graph.loop_source = [&](const std::vector<pose_graph::KeyFrame::Ptr> &old, const std::deque<pose_graph::KeyFrame::Ptr> &fresh,
                              std::vector<pose_graph::Loop::Ptr> &out) {
        if (!old.empty()) return;  // everything is new in the one pass this program makes
        for (size_t k = 0; k < loop_rel.size(); ++k) {
          pose_graph::Loop::Ptr lp = std::make_shared<pose_graph::Loop>();
          lp->key1 = fresh[(size_t)loop_i[k]];
          lp->key2 = fresh[(size_t)loop_j[k]];
          for (int q = 0; q < 16; ++q) lp->relative_pose.m[q] = loop_rel[k].m[q];
          out.push_back(lp);
        }
      };
      const int found = graph.optimize(1000);
      if (found < 0) {
        std::fprintf(stderr, "Graph::optimize failed: %s\n", graph.lastError().c_str());
        return 1;
      }
      std::printf("GITER %d\nGLOOPS %d\n", graph.last_iterations, found);
      const std::vector<double> &gw = graph.loopWeights();
      for (size_t k = 0; k < gw.size(); ++k) std::printf("GWEIGHT %zu %.17g\n", k, gw[k]);
      for (size_t k = 0; k < graph.keyframes.size(); ++k)
        std::printf("GPOS %zu %.17g %.17g %.17g\n", k, graph.keyframes[k]->estimate(0, 3), graph.keyframes[k]->estimate(1, 3),
                    graph.keyframes[k]->estimate(2, 3));
    }
    lslam_ctx_destroy(ctx);
    std::printf("REFUSED %d\n", refused ? 1 : 0);
  } catch (const std::exception &ex) {
    std::fprintf(stderr, "backend unavailable: %s\n", ex.what());
    return 1;
  }
  return 0;
}
