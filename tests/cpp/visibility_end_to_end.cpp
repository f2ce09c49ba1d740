// C++ drop-in check of the visibility filter of pose_graph::Graph and KeyframeStore (include/lslam_loop_closure.hpp) over the C
// ABI: a resident Graph with remove_dynamic on rebuilds its final map without the points other keyframes looked through.
// argv[1]: the keyframes, binary: uint32 n, then per keyframe 16 doubles (the odometry pose, row-major 4x4), uint32 n_corner and
// its {x, y, z, intensity} floats, uint32 n_surf and its floats.  argv[2]: up_axis.  Every frame goes through add_frame, then one
// optimize (no loops: an empty loop_source), then getFinalFeatureMap(bootstrap = true) with 21 x 11 x 21 cubes.  Prints what the
// test compares with the Python mirror on the same numbers:
//   ADDED <keyframes added> <keyframes>
//   REMOVED <keyframe> <corner points left out> <surf points left out>      removedPoints
//   VOTES <keyframe> <points with a free vote> <points with a hit vote> <dynamic points>
//                                       KeyframeStore::vis_votes of all keyframes on the keyframe's surf cloud, read as graph points
//   IMAGE <keyframe> <finite pixels>    KeyframeStore::vis_range_image
//   MOVED <cloud bytes the store moved after the keyframes' own uploads and the VOTES line's downloads>
//   OFF <1 if the same frames without the switch left removedPoints empty>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <string>
#include <vector>

#include "lslam_loop_closure.hpp"

static bool read_cloud(FILE *f, std::vector<float> &out) {
  unsigned n = 0;
  if (std::fread(&n, 4, 1, f) != 1) return false;
  out.resize((size_t)n * 4);
  return n == 0 || std::fread(out.data(), 16, n, f) == n;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
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
    pose_graph::Graph graph(ctx, 0, 10, true), off(ctx, 0, 10, true);
    graph.remove_dynamic = true;
    graph.dynamic_params.up_axis = std::atoi(argv[2]);
    const auto no_loops = [](const std::vector<pose_graph::KeyFrame::Ptr> &, const std::deque<pose_graph::KeyFrame::Ptr> &,
                             std::vector<pose_graph::Loop::Ptr> &) {};
    graph.loop_source = no_loops;
    off.loop_source = no_loops;
    unsigned long long uploaded = 0;
    for (unsigned k = 0; k < n && rc == 0; ++k) {
      pose_graph::Mat4d odom;
      std::vector<float> corner, surf;
      if (std::fread(odom.m, 8, 16, f) != 16 || !read_cloud(f, corner) || !read_cloud(f, surf)) return 2;
      uploaded += (unsigned long long)(corner.size() + surf.size()) * 4;
      if (!graph.add_frame(odom, corner, surf) || !off.add_frame(odom, corner, surf)) {
        std::fprintf(stderr, "frame %u was not taken as a keyframe\n", k);
        rc = 1;
      }
    }
    std::fclose(f);
    if (rc == 0 && (graph.optimize() < 0 || off.optimize() < 0)) {
      std::fprintf(stderr, "Graph::optimize failed: %s %s\n", graph.lastError().c_str(), off.lastError().c_str());
      rc = 1;
    }
    if (rc == 0) {
      std::vector<char> matched;
      std::vector<pose_graph::Mat4d> poses;
      const int added = graph.getFinalFeatureMap(ctx, "", true, matched, poses, nullptr, 21, 11, 21);
      const int added_off = off.getFinalFeatureMap(ctx, "", true, matched, poses, nullptr, 21, 11, 21);
      if (added < 0 || added_off < 0) {
        std::fprintf(stderr, "Graph::getFinalFeatureMap failed: %s %s\n", graph.lastError().c_str(), off.lastError().c_str());
        rc = 1;
      } else {
        std::printf("ADDED %d %zu\n", added, graph.keyframes.size());
        for (size_t k = 0; k < graph.removedPoints.size(); ++k)
          std::printf("REMOVED %zu %zu %zu\n", k, graph.removedPoints[k].first, graph.removedPoints[k].second);
        std::printf("OFF %d\n", off.removedPoints.empty() && added_off == added ? 1 : 0);
      }
    }
    if (rc == 0) {
      pose_graph::KeyframeStore &store = *graph.store;
      std::vector<int32_t> ids;
      std::vector<float> poses;
      for (const auto &kf : graph.keyframes) {
        float P[16];
        pose_graph::to_float16(kf->estimate, P);
        ids.push_back(kf->store_id);
        poses.insert(poses.end(), P, P + 16);
      }
      unsigned long long downloaded = 0;
      for (size_t k = 0; k < graph.keyframes.size() && rc == 0; ++k) {
        std::vector<float> surf, img;
        std::vector<uint32_t> votes;
        if (!store.get(graph.keyframes[k]->store_id, 1, surf) || !store.vis_votes(ids, poses, surf, votes) ||
            !store.vis_range_image(graph.keyframes[k]->store_id, img)) {
          std::fprintf(stderr, "KeyframeStore: %s\n", store.lastError().c_str());
          rc = 1;
          break;
        }
        downloaded += (unsigned long long)surf.size() * 4;
        size_t n_free = 0, n_hit = 0, n_dyn = 0, n_pix = 0;
        for (uint32_t w : votes) {
          const uint32_t fr = w & 0xffffu, hi = w >> 16;
          n_free += fr > 0;
          n_hit += hi > 0;
          n_dyn += fr >= (uint32_t)graph.dynamic_params.min_free_votes && fr > hi;
        }
        for (float v : img) n_pix += std::isfinite(v) ? 1 : 0;
        std::printf("VOTES %zu %zu %zu %zu\nIMAGE %zu %zu\n", k, n_free, n_hit, n_dyn, k, n_pix);
      }
      lslam_kfs_stats st;
      if (rc == 0 && store.info(st))
        std::printf("MOVED %lld\n", (long long)(st.cloud_bytes_uploaded - uploaded) + (long long)(st.cloud_bytes_downloaded - downloaded));
    }
  }
  lslam_ctx_destroy(ctx);
  return rc;
}
