// C++ drop-in check of the edge-information additions: pose_graph::Graph::edge_information / range_sigma / edgeInformations /
// informationMatrices (include/lslam_loop_closure.hpp) over the C ABI (lslam_keyframe_edge_information).
// Reads the keyframes the test wrote as text: "n_keyframes range_sigma", then per keyframe 16 doubles (the odometry pose,
// row-major), "n_corner" and 4 floats per point, "n_surf" and 4 floats per point; then "n_loops" and per loop "i j" and 16
// doubles (the measured pose of keyframe j in keyframe i's frame).  Drives a resident Graph with edge_information = "hessian"
// through one optimize(), the loops handed over through Graph::loop_source with keyframe i as their reference, and prints what
// the test compares with the Python mirror driven with the same keyframes, bit for bit:
//   EDGES <edges>   ITER <LM iterations>
//   INFO <edge> <n_rows> <36 doubles as hex floats>       Graph::informationMatrices()
//   POS <keyframe> <x> <y> <z>
//   REFUSED <1 if the option's misuse was refused: an unknown value, no range_sigma, a graph that is not resident>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <memory>
#include <string>
#include <vector>

#include "lslam_loop_closure.hpp"

static bool read_mat(FILE *f, pose_graph::Mat4d &T) {
  for (int k = 0; k < 16; ++k)
    if (std::fscanf(f, "%lf", &T.m[k]) != 1) return false;
  return true;
}
static bool read_cloud(FILE *f, std::vector<float> &c) {
  long n = 0;
  if (std::fscanf(f, "%ld", &n) != 1 || n < 0) return false;
  c.resize(4 * (size_t)n);
  for (size_t k = 0; k < c.size(); ++k)
    if (std::fscanf(f, "%f", &c[k]) != 1) return false;
  return true;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n_kf = 0, n_loops = 0;
  double sigma = 0.0;
  if (std::fscanf(f, "%d %lf", &n_kf, &sigma) != 2) return 2;
  std::vector<pose_graph::Mat4d> odom((size_t)n_kf), loop_rel;
  std::vector<std::vector<float> > corner((size_t)n_kf), surf((size_t)n_kf);
  std::vector<int> loop_i, loop_j;
  for (int k = 0; k < n_kf; ++k)
    if (!read_mat(f, odom[(size_t)k]) || !read_cloud(f, corner[(size_t)k]) || !read_cloud(f, surf[(size_t)k])) return 2;
  if (std::fscanf(f, "%d", &n_loops) != 1) return 2;
  for (int k = 0; k < n_loops; ++k) {
    int i = 0, j = 0;
    pose_graph::Mat4d Z;
    if (std::fscanf(f, "%d %d", &i, &j) != 2 || !read_mat(f, Z)) return 2;
    loop_i.push_back(i);
    loop_j.push_back(j);
    loop_rel.push_back(Z);
  }
  std::fclose(f);
  lslam_ctx *ctx = nullptr;
  if (lslam_ctx_create(0, &ctx) != LSLAM_OK) {
    std::fprintf(stderr, "backend unavailable (no CPU fallback): %s\n", lslam_last_error());
    return 1;
  }
  bool refused = true;
  {
    pose_graph::Graph host(ctx);  // not resident; (the options are checked before anything is added)
    host.edge_information = "hessian";
    host.range_sigma = 0.02;
    refused = refused && host.optimize() == -1;
    pose_graph::Graph g(ctx, 0, 10, true);
    g.edge_information = "hessian";  // no range_sigma
    refused = refused && g.optimize() == -1;
    g.range_sigma = 0.02;
    g.edge_information = "identity";
    refused = refused && g.optimize() == -1 && g.edgeInformations().empty();
  }
  int rc = 0;
  {
    pose_graph::Graph graph(ctx, 0, n_kf > 0 ? n_kf : 1, true);
    graph.edge_information = "hessian";
    graph.range_sigma = sigma;
    for (int k = 0; k < n_kf; ++k)
      if (!graph.add_frame(odom[(size_t)k], corner[(size_t)k], surf[(size_t)k])) {
        std::fprintf(stderr, "frame %d was not taken as a keyframe: %s\n", k, graph.lastError().c_str());
        return 1;
      }
    graph.loop_source = [&](const std::vector<pose_graph::KeyFrame::Ptr> &old, const std::deque<pose_graph::KeyFrame::Ptr> &fresh,
                            std::vector<pose_graph::Loop::Ptr> &out) {
      if (!old.empty()) return;  // everything is new in the one pass this program makes
      static const float EYE[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
      for (size_t k = 0; k < loop_rel.size(); ++k) {
        pose_graph::Loop::Ptr lp = std::make_shared<pose_graph::Loop>();
        lp->key1 = fresh[(size_t)loop_i[k]];
        lp->key2 = fresh[(size_t)loop_j[k]];
        lp->relative_pose = loop_rel[k];
        lp->ref_ids.assign(1, lp->key1->store_id);
        lp->rel_T.assign(EYE, EYE + 16);
        out.push_back(lp);
      }
    };
    const int found = graph.optimize(1000);
    if (found < 0) {
      std::fprintf(stderr, "Graph::optimize failed: %s\n", graph.lastError().c_str());
      rc = 1;
    } else {
      const std::vector<double> &info = graph.informationMatrices();
      const std::vector<lslam_edge_info> &ei = graph.edgeInformations();
      std::printf("EDGES %zu\nITER %d\n", info.size() / 36, graph.last_iterations);
      for (size_t e = 0; e < info.size() / 36 && e < ei.size(); ++e) {
        std::printf("INFO %zu %d", e, (int)ei[e].n_rows);
        for (int k = 0; k < 36; ++k) std::printf(" %a", info[36 * e + (size_t)k]);
        std::printf("\n");
      }
      for (size_t k = 0; k < graph.keyframes.size(); ++k)
        std::printf("POS %zu %.17g %.17g %.17g\n", k, graph.keyframes[k]->estimate(0, 3), graph.keyframes[k]->estimate(1, 3),
                    graph.keyframes[k]->estimate(2, 3));
    }
  }
  lslam_ctx_destroy(ctx);
  std::printf("REFUSED %d\n", refused ? 1 : 0);
  return rc;
}
