// C++ drop-in check of the map-quality mirrors (include/lslam_loop_closure.hpp: KeyframeStore::mapQuality, Graph::mapQuality,
// trajectoryEval; include/lslam_feature_map.hpp: FeatureMap::quality) over the C ABI.
// argv[1]: the keyframes, binary: uint32 n, then per keyframe 16 doubles (the odometry pose, row-major 4x4), 16 doubles (the
// estimate), uint32 n_corner and its {x, y, z, intensity} floats, uint32 n_surf and its floats.  Every frame goes through
// add_frame of a resident and of a host graph and is handed its estimate.  Prints what the test compares with the Python
// mirrors on the same numbers, integers in decimal and doubles as hexadecimal floats:
//   Q <what> <n_query> <n_defined> <n_sparse> <sum_entropy_q32> <sum_plane_var_q30> <sum_neighbors> <max_neighbors> <MME> <MPV> <mean k>
//     what: RES_EST / RES_ODOM (the resident graph), HOST_EST / HOST_ODOM (the host graph), STORE_CORNER (the store's member, corner
//     clouds at the estimates), FMAP_CORNER / FMAP_SURF (a cube map that holds keyframe 0's clouds at its estimate)
//   TRAJ <n_used> <n_gated> <mean dist> <max dist> <aligned> <ate_rmse>    estimate against odometry positions, stamps 0, 1, 2, ...
//   MOVED <cloud bytes the store moved after the keyframes' own uploads>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "lslam_feature_map.hpp"
#include "lslam_loop_closure.hpp"

struct Point {
  float x, y, z, intensity;
};
struct Cloud {
  std::vector<Point> points;
  void clear() { points.clear(); }
};
struct Iso {
  struct M {
    float m[16];
    float operator()(int r, int c) const { return m[4 * r + c]; }
  } mat;
  M &matrix() { return mat; }
};

static bool read_cloud(FILE *f, std::vector<float> &out) {
  unsigned n = 0;
  if (std::fread(&n, 4, 1, f) != 1) return false;
  out.resize((size_t)n * 4);
  return n == 0 || std::fread(out.data(), 16, n, f) == n;
}
static void print_q(const char *what, const lslam_mapq_stats &s) {
  std::printf("Q %s %lld %lld %lld %lld %lld %lld %lld %a %a %a\n", what, (long long)s.n_query, (long long)s.n_defined, (long long)s.n_sparse,
              (long long)s.sum_entropy_q32, (long long)s.sum_plane_var_q30, (long long)s.sum_neighbors, (long long)s.max_neighbors,
              s.mean_entropy, s.mean_plane_variance, s.mean_neighbors);
}
static Cloud to_cloud(const std::vector<float> &v) {
  Cloud c;
  for (size_t i = 0; i + 3 < v.size(); i += 4) c.points.push_back(Point{v[i], v[i + 1], v[i + 2], v[i + 3]});
  return c;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  unsigned n = 0;
  if (!f || std::fread(&n, 4, 1, f) != 1) return 2;
  lslam_ctx *ctx = nullptr;
  if (lslam_ctx_create(0, &ctx) != LSLAM_OK) {
    std::fprintf(stderr, "backend unavailable: %s\n", lslam_last_error());
    return 1;
  }
  int rc = 0;
  {
    pose_graph::Graph resident(ctx, 0, 10, true), host(ctx, 0, 10, false);
    std::vector<pose_graph::KeyFrame::Ptr> kr, kh;
    std::vector<double> stamps, est_xyz, odom_xyz;
    std::vector<float> corner0, surf0;
    pose_graph::Mat4d est0;
    unsigned long long uploaded = 0;
    for (unsigned k = 0; k < n; ++k) {
      pose_graph::Mat4d odom, est;
      std::vector<float> corner, surf;
      if (std::fread(odom.m, 8, 16, f) != 16 || std::fread(est.m, 8, 16, f) != 16 || !read_cloud(f, corner) || !read_cloud(f, surf)) return 2;
      uploaded += (unsigned long long)(corner.size() + surf.size()) * 4;
      pose_graph::KeyFrame::Ptr a = resident.add_frame(odom, corner, surf), b = host.add_frame(odom, corner, surf);
      if (!a || !b) {
        std::fprintf(stderr, "frame %u was not taken as a keyframe: %s\n", k, resident.lastError().c_str());
        rc = 1;
        break;
      }
      a->estimate = est;
      b->estimate = est;
      kr.push_back(a);
      kh.push_back(b);
      stamps.push_back((double)k);
      for (int d = 0; d < 3; ++d) { est_xyz.push_back(est.m[4 * d + 3]); odom_xyz.push_back(odom.m[4 * d + 3]); }
      if (k == 0) { corner0 = corner; surf0 = surf; est0 = est; }
    }
    std::fclose(f);
    lslam_mapq_params P;
    lslam_mapq_default_params(&P);
    lslam_mapq_stats st;
    if (rc == 0) {
      const struct { const char *what; pose_graph::Graph *g; std::vector<pose_graph::KeyFrame::Ptr> *k; bool odom; } runs[4] = {
          {"RES_EST", &resident, &kr, false}, {"RES_ODOM", &resident, &kr, true}, {"HOST_EST", &host, &kh, false}, {"HOST_ODOM", &host, &kh, true}};
      for (const auto &r : runs) {
        if (!r.g->mapQuality(r.odom, 1, &P, st, r.k)) {
          std::fprintf(stderr, "Graph::mapQuality: %s\n", r.g->lastError().c_str());
          rc = 1;
          break;
        }
        print_q(r.what, st);
      }
    }
    if (rc == 0) {
      std::vector<int32_t> ids;
      std::vector<float> poses;
      for (const auto &kf : kr) {
        float T[16];
        pose_graph::to_float16(kf->estimate, T);
        ids.push_back(kf->store_id);
        poses.insert(poses.end(), T, T + 16);
      }
      P.radius = 0.5f;
      P.min_neighbors = 3;
      lslam_kfs_stats ks;
      if (!resident.store->mapQuality(ids, poses, 0, &P, st) || !resident.store->info(ks)) {
        std::fprintf(stderr, "KeyframeStore::mapQuality: %s\n", resident.store->lastError().c_str());
        rc = 1;
      } else {
        print_q("STORE_CORNER", st);
        std::printf("MOVED %lld\n", (long long)(ks.cloud_bytes_uploaded - uploaded) + (long long)ks.cloud_bytes_downloaded);
      }
    }
    if (rc == 0 && n) {
      try {
        lidar_slam::FeatureMap<Point, Cloud> fm(ctx);
        fm.update(Point{0.0f, 0.0f, 0.0f, 0.0f});
        Iso T;
        pose_graph::to_float16(est0, T.mat.m);
        fm.addFeatureCloud(to_cloud(corner0), to_cloud(surf0), T);
        print_q("FMAP_CORNER", fm.quality(0, &P));
        print_q("FMAP_SURF", fm.quality());
      } catch (const std::exception &e) {
        std::fprintf(stderr, "FeatureMap: %s\n", e.what());
        rc = 1;
      }
    }
    if (rc == 0) {
      lslam_traj_params tp;
      lslam_traj_default_params(&tp);
      tp.align = 1;
      lslam_traj_stats ts;
      if (!pose_graph::trajectoryEval(stamps, est_xyz, stamps, odom_xyz, &tp, ts)) {
        std::fprintf(stderr, "trajectoryEval: %s\n", lslam_last_error());
        rc = 1;
      } else {
        std::printf("TRAJ %lld %lld %a %a %d %a\n", (long long)ts.n_used, (long long)ts.n_gated, ts.mean[3], ts.max[3], (int)ts.aligned, ts.ate_rmse);
      }
    }
  }
  lslam_ctx_destroy(ctx);
  return rc;
}
