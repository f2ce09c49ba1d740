// C++ drop-in check of the plane priors of SolverG2OT (include/lslam_solver_g2o.hpp) over the C ABI: add_se3_prior_plane_edge
// (against a given world plane and against the floor z = 0), add_robust_kernel on a plane prior, planePriorWeights and a
// save / load round trip.
// argv[1]: a graph written by the test as text: "n_vertices n_edges n_planes fix_first", then per vertex 16 doubles (the 4x4
// estimate, row-major), per edge "i j", 36 doubles (its information matrix) and 16 doubles (the relative pose), per plane prior
// "vertex default_world kernel size", 4 doubles (the measured plane), 4 doubles (the world plane; not passed on when
// default_world is 1) and a 3x3 information -- kernel "NONE" / "Huber" / "Cauchy" / "DCS" with its size.
// argv[2]: where to save the optimised graph.  Prints what the test compares with the Python mirror on the same numbers:
//   ITER <LM iterations>   CHI2 <final chi2>
//   QWEIGHT <plane prior> <weight>        planePriorWeights()
//   POS <vertex> <x> <y> <z>              the optimised positions
//   LOADED <vertices> <plane priors>      a second solver after load(argv[2])
//   LITER <LM iterations>   LPOS <vertex> <x> <y> <z>    ... optimised again (kernels are not part of the file)
//   REFUSED <1 if an unknown kernel type and a missing plane prior were refused>
// With argv[1] = "--graph": argv[2] is a drive for pose_graph::Graph (include/lslam_loop_closure.hpp) with its floor switch on:
// "n sigma_normal sigma_distance kernel size resident n_hypotheses min_inliers max_iterations", the 6 diagonal entries of the
// odometry information, then per frame 16 doubles (the odometry pose), the number of surface points and their x y z.  Every frame
// goes through add_frame and one optimize(max_iterations); no loops (an empty loop_source); resident = 1: the clouds live in the graph's
// KeyframeStore and one KeyframeStore::floorDetect call per pass finds the floors.  Prints
//   FPASS <frame> <plane priors in the solver> <LM iterations of the pass>
//   FNOTFOUND <keyframe> <LSLAM_FLOOR_* status>      floorsNotFound
//   FCOEFF <keyframe> <nx> <ny> <nz> <d>             the accepted floors, in plane-prior order
//   FWEIGHT <plane prior> <weight>                   floorWeights()
//   FREJECTED <keyframe>                             rejectedFloors()
//   FPOS <keyframe> <x> <y> <z>                      the keyframes' estimates
//   FMOVED <cloud bytes the store moved after the keyframes' own uploads, -1 without a store>
//   FOFF <1 if the same frames without the switch added no plane prior, looked for no floor and never ran the solver>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <vector>

#include <cstring>

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
struct Vec4 { double v[4]; double operator()(int i) const { return v[i]; } };
typedef pose_graph::SolverG2OT<Iso, Mat6> Solver;

static bool read_n(FILE *f, double *out, int n) {
  for (int k = 0; k < n; ++k)
    if (std::fscanf(f, "%lf", &out[k]) != 1) return false;
  return true;
}

static int drive_graph(const char *path) {
  FILE *gf = std::fopen(path, "r");
  int n = 0, resident = 0, n_hyp = 0, min_inliers = 0, max_iterations = 0;
  double sn = 0.0, sd = 0.0, ksize = 1.0, oinfo[6];
  char kname[32];
  if (!gf || std::fscanf(gf, "%d %lf %lf %31s %lf %d %d %d %d", &n, &sn, &sd, kname, &ksize, &resident, &n_hyp, &min_inliers, &max_iterations) != 9 ||
      !read_n(gf, oinfo, 6))
    return 2;
  lslam_ctx *ctx = nullptr;
  if (lslam_ctx_create(0, &ctx) != LSLAM_OK) {
    std::fprintf(stderr, "backend unavailable: %s\n", lslam_last_error());
    return 1;
  }
  int rc = 0;
  {
    pose_graph::Graph graph(ctx, 0, 10, resident != 0), off(ctx, 0, 10, resident != 0);
    graph.floor_sigma_normal = sn;
    graph.floor_sigma_distance = sd;
    graph.floor_robust_kernel = kname;
    graph.floor_robust_kernel_size = ksize;
    graph.floor_params.n_hypotheses = n_hyp;
    graph.floor_params.min_inliers = min_inliers;
    for (int k = 0; k < 6; ++k) graph.odometry_information[k] = off.odometry_information[k] = oinfo[k];
    const auto no_loops = [](const std::vector<pose_graph::KeyFrame::Ptr> &, const std::deque<pose_graph::KeyFrame::Ptr> &,
                             std::vector<pose_graph::Loop::Ptr> &) {};
    graph.loop_source = no_loops;
    off.loop_source = no_loops;
    const std::vector<float> none;
    unsigned long long uploaded = 0;
    bool off_quiet = true;
    for (int k = 0; k < n && rc == 0; ++k) {
      pose_graph::Mat4d odom;
      int m = 0;
      if (!read_n(gf, odom.m, 16) || std::fscanf(gf, "%d", &m) != 1 || m < 0) return 2;
      std::vector<float> surf((size_t)m * 4, 0.0f);
      for (int i = 0; i < m; ++i) {
        double p[3];
        if (!read_n(gf, p, 3)) return 2;
        for (int c = 0; c < 3; ++c) surf[(size_t)i * 4 + c] = (float)p[c];
      }
      uploaded += (unsigned long long)m * 16;
      if (!graph.add_frame(odom, none, surf) || !off.add_frame(odom, none, surf)) {
        std::fprintf(stderr, "frame %d was not taken as a keyframe\n", k);
        rc = 1;
        break;
      }
      if (graph.optimize(max_iterations) < 0 || off.optimize(max_iterations) < 0) {
        std::fprintf(stderr, "Graph::optimize failed: %s %s\n", graph.lastError().c_str(), off.lastError().c_str());
        rc = 1;
        break;
      }
      off_quiet = off_quiet && off.last_iterations == 0;
      std::printf("FPASS %d %zu %d\n", k, graph.numPlanePriors(), graph.last_iterations);
    }
    std::fclose(gf);
    if (rc == 0) {
      for (const auto &kf : graph.floorsNotFound) std::printf("FNOTFOUND %d %d\n", kf->node, kf->floor_status);
      for (const auto &kf : graph.floors)
        std::printf("FCOEFF %d %.17g %.17g %.17g %.17g\n", kf->node, kf->floor_coeffs[0], kf->floor_coeffs[1], kf->floor_coeffs[2], kf->floor_coeffs[3]);
      const std::vector<double> &w = graph.floorWeights();
      for (size_t k = 0; k < w.size(); ++k) std::printf("FWEIGHT %zu %.17g\n", k, w[k]);
      for (const auto &kf : graph.rejectedFloors()) std::printf("FREJECTED %d\n", kf->node);
      for (size_t k = 0; k < graph.keyframes.size(); ++k)
        std::printf("FPOS %zu %.17g %.17g %.17g\n", k, graph.keyframes[k]->estimate(0, 3), graph.keyframes[k]->estimate(1, 3),
                    graph.keyframes[k]->estimate(2, 3));
      long long moved = -1;
      if (graph.store) {
        lslam_kfs_stats st;
        if (graph.store->info(st)) moved = (long long)(st.cloud_bytes_uploaded - uploaded) + (long long)st.cloud_bytes_downloaded;
      }
      std::printf("FMOVED %lld\n", moved);
      bool quiet = off_quiet && off.numPlanePriors() == 0 && off.floors.empty() && off.floorsNotFound.empty() && off.floorWeights().empty();
      for (const auto &kf : off.keyframes) quiet = quiet && !kf->has_floor_coeffs && kf->floor_status == -1;
      std::printf("FOFF %d\n", quiet ? 1 : 0);
    }
  }
  lslam_ctx_destroy(ctx);
  return rc;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  if (std::strcmp(argv[1], "--graph") == 0) return drive_graph(argv[2]);
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int nv = 0, ne = 0, nq = 0, fix_first = 1;
  if (std::fscanf(f, "%d %d %d %d", &nv, &ne, &nq, &fix_first) != 4) return 2;
  try {
    Solver solver;
    solver.setFixFirstNode(fix_first != 0);
    std::vector<Solver::VertexSE3 *> vs;
    for (int k = 0; k < nv; ++k) {
      Iso T;
      if (!read_n(f, T.m, 16)) return 2;
      vs.push_back(solver.add_se3_node(T));
    }
    for (int k = 0; k < ne; ++k) {
      int i, j;
      Mat6 w;
      Iso T;
      if (std::fscanf(f, "%d %d", &i, &j) != 2 || !read_n(f, w.v, 36) || !read_n(f, T.m, 16)) return 2;
      solver.add_se3_edge(vs[(size_t)i], vs[(size_t)j], T, w);
    }
    std::vector<Solver::EdgeSE3Plane *> planes;
    for (int k = 0; k < nq; ++k) {
      int v, default_world;
      char kernel[32];
      double size;
      Vec4 meas, world;
      Mat3 w;
      if (std::fscanf(f, "%d %d %31s %lf", &v, &default_world, kernel, &size) != 4 || !read_n(f, meas.v, 4) || !read_n(f, world.v, 4) ||
          !read_n(f, w.v, 9))
        return 2;
      Solver::EdgeSE3Plane *p = default_world ? solver.add_se3_prior_plane_edge(vs[(size_t)v], meas, w)
                                              : solver.add_se3_prior_plane_edge(vs[(size_t)v], meas, w, world);
      if (std::string(kernel) != "NONE") solver.add_robust_kernel(p, kernel, size);
      planes.push_back(p);
    }
    std::fclose(f);
    int refused = 0;
    try {
      solver.add_robust_kernel(planes[0], "Tukey", 1.0);
    } catch (const std::invalid_argument &) {
      ++refused;
    }
    try {
      solver.add_robust_kernel(static_cast<Solver::EdgeSE3Plane *>(nullptr), "Huber", 1.0);
    } catch (const std::invalid_argument &) {
      ++refused;
    }
    solver.optimize();
    std::printf("ITER %d\nCHI2 %.17g\n", solver.lastStats().iterations, solver.lastStats().chi2_final);
    const std::vector<double> w = solver.planePriorWeights();
    for (size_t k = 0; k < w.size(); ++k) std::printf("QWEIGHT %zu %.17g\n", k, w[k]);
    for (int k = 0; k < nv; ++k) {
      Iso T = vs[(size_t)k]->estimate();
      std::printf("POS %d %.17g %.17g %.17g\n", k, T.m[3], T.m[7], T.m[11]);
    }
    solver.save(argv[2]);
    Solver again;
    again.load(argv[2]);
    std::printf("LOADED %d %zu\n", again.is_first ? 0 : nv, again.numPlanePriors());
    again.optimize();
    std::printf("LITER %d\n", again.lastStats().iterations);
    for (int k = 0; k < nv; ++k) {
      Solver::VertexSE3 vk{k, &again};
      Iso T = vk.estimate();
      std::printf("LPOS %d %.17g %.17g %.17g\n", k, T.m[3], T.m[7], T.m[11]);
    }
    std::printf("REFUSED %d\n", refused == 2 ? 1 : 0);
  } catch (const std::exception &e) {
    std::fprintf(stderr, "floor_prior_end_to_end: %s\n", e.what());
    return 1;
  }
  return 0;
}
