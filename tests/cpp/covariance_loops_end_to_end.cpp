// C++ drop-in check of the covariance-gated loop search of include/lslam_loop_closure.hpp (Graph::loop_search = "covariance",
// LoopDetector::find_covariance_candidates, Loop::mahalanobis, Graph::loopConsistency) over the C ABI, on a RESIDENT graph.
// argv[1]: the frame stream of tests/cpp/loop_closure_end_to_end.cpp (16 doubles odometry pose, then corner and surf clouds as
// uint32 count + count x {x,y,z,intensity} floats); argv[2]: accum_distance_thresh; argv[3]: "covariance" or "NONE";
// argv[4]: max_iters of the covariance calls; argv[5]: the shift [m] of the deliberately wrong relative pose; argv[6..11]
// (optional): the six diagonal entries of Graph::odometry_information; argv[12] (optional): rel_tol of the covariance calls.
// Drives Graph::add_frame / Graph::optimize per frame and prints what the test compares with the Python mirror:
//   GATE <keyframes so far> <candidate node> <d2>     every candidate the gate looked at, pass by pass
//   LOOP <key1 node> <key2 node> <mahalanobis>         every loop found
//   WRONG <d2>                                         loopConsistency of the first loop's pose shifted along z, asked right after it was found
//   LOOPS <n> KEYFRAMES <n>      KF <i> <x> <y> <z>    the estimates at the end
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "lslam_loop_closure.hpp"

static bool read_cloud(FILE *f, std::vector<float> &c) {
  uint32_t n = 0;
  if (std::fread(&n, 4, 1, f) != 1) return false;
  c.resize(4 * (size_t)n);
  return n == 0 || std::fread(c.data(), 16, n, f) == n;
}

int main(int argc, char **argv) {
  if (argc < 6) return 2;
  lslam_ctx *ctx = nullptr;
  if (lslam_ctx_create(0, &ctx) != LSLAM_OK) {
    std::fprintf(stderr, "backend unavailable: %s\n", lslam_last_error());
    return 1;
  }
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  {
    pose_graph::Graph g(ctx, 0, 10, true);
    g.loop_detector.accum_distance_thresh = std::atof(argv[2]);
    g.loop_search = argv[3];
    g.covariance_opts.max_iters = std::atoi(argv[4]);
    const double shift = std::atof(argv[5]);
    for (int k = 0; k < 6 && argc >= 12; ++k) g.odometry_information[k] = std::atof(argv[6 + k]);
    if (argc >= 13) g.covariance_opts.rel_tol = std::atof(argv[12]);
    int n_loops = 0;
    bool wrong_done = false;
    pose_graph::Mat4d odom;
    std::vector<float> corner, surf;
    while (std::fread(odom.m, sizeof(double), 16, f) == 16 && read_cloud(f, corner) && read_cloud(f, surf)) {
      if (!g.add_frame(odom, corner, surf)) continue;
      const size_t before = g.loops.size();
      const int found = g.optimize(20);
      if (found < 0) {
        std::fprintf(stderr, "optimize failed: %s\n", g.lastError().c_str());
        return 1;
      }
      for (const auto &gt : g.loop_detector.last_gate) std::printf("GATE %zu %d %.17g\n", g.keyframes.size(), gt.node, gt.d2);
      g.loop_detector.last_gate.clear();
      for (size_t k = before; k < g.loops.size(); ++k) {
        const auto &lp = g.loops[k];
        std::printf("LOOP %d %d %.17g\n", lp->key1->node, lp->key2->node, lp->has_mahalanobis ? lp->mahalanobis : -1.0);
        if (!wrong_done && lp->has_mahalanobis) {
          pose_graph::Mat4d Z = lp->relative_pose;
          Z(2, 3) += shift;  // along z: across the drift of the test's scenario
          double d2 = 0.0;
          if (!g.loopConsistency(lp->key1, lp->key2, Z, &d2)) {
            std::fprintf(stderr, "loopConsistency failed: %s\n", g.lastError().c_str());
            return 1;
          }
          std::printf("WRONG %.17g\n", d2);
          wrong_done = true;
        }
      }
      n_loops += found;
    }
    std::fclose(f);
    std::printf("LOOPS %d KEYFRAMES %zu\n", n_loops, g.keyframes.size());
    for (size_t i = 0; i < g.keyframes.size(); ++i)
      std::printf("KF %zu %.17g %.17g %.17g\n", i, g.keyframes[i]->estimate(0, 3), g.keyframes[i]->estimate(1, 3),
                  g.keyframes[i]->estimate(2, 3));
  }
  lslam_ctx_destroy(ctx);
  return 0;
}
