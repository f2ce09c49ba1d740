// C++ drop-in check of the occupancy grid's mirrors (include/lslam_loop_closure.hpp) over the C ABI: KeyframeStore::occFitBounds /
// occSetup / occIntegrate / occCounts / occValues / occInfo / occClear and saveMap.
// argv[1]: a drive written by the test as text: "n up_axis resolution min_range max_range fit width height origin_a origin_b",
// then per keyframe 16 floats (the pose, row-major), "n_corner n_surf" and the points' x y z, corner cloud first.  fit = 1: the
// bounds are fitted to the poses, the four numbers after it are ignored.
// argv[2]: the stem saveMap writes <stem>.pgm / <stem>.yaml to.  argv[3]: the counts, width * height uint32, as a binary file.
// Prints what the test compares with the Python path on the same numbers:
//   GRID <width> <height> <origin_a> <origin_b>
//   RAYS <cast> <dropped> <obstacle> <ground> <keyframes integrated>
//   TWICE <1 if a second integration of every keyframe doubled every count, and clear zeroed them>
//   REFUSED <1 if a pose count that does not match the ids and an id out of range were refused>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "lslam_loop_closure.hpp"

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  lslam_ctx *ctx = nullptr;
  if (lslam_ctx_create(0, &ctx) != LSLAM_OK) {
    std::fprintf(stderr, "backend unavailable: %s\n", lslam_last_error());
    return 1;
  }
  int rc = 0;
  {
    FILE *f = std::fopen(argv[1], "r");
    int n = 0, fit = 0;
    lslam_occ_params p;
    lslam_occ_default_params(&p);
    if (!f || std::fscanf(f, "%d %d %f %f %f %d %d %d %lf %lf", &n, &p.up_axis, &p.resolution, &p.min_range, &p.max_range, &fit, &p.width,
                          &p.height, &p.origin[0], &p.origin[1]) != 10)
      return 2;
    pose_graph::KeyframeStore store(ctx, 0, 0, 4096);
    std::vector<int32_t> ids;
    std::vector<float> poses;
    for (int k = 0; k < n; ++k) {
      float v;
      for (int e = 0; e < 16; ++e) {
        if (std::fscanf(f, "%f", &v) != 1) return 2;
        poses.push_back(v);
      }
      int nc = 0, ns = 0;
      if (std::fscanf(f, "%d %d", &nc, &ns) != 2) return 2;
      std::vector<float> cloud[2];
      for (int t = 0; t < 2; ++t)
        for (int i = 0; i < (t ? ns : nc); ++i) {
          float x, y, z;
          if (std::fscanf(f, "%f %f %f", &x, &y, &z) != 3) return 2;
          cloud[t].insert(cloud[t].end(), {x, y, z, 0.0f});
        }
      const int id = store.add(cloud[0], cloud[1]);
      if (id < 0) { std::fprintf(stderr, "add: %s\n", store.lastError().c_str()); return 3; }
      ids.push_back(id);
    }
    std::fclose(f);
    std::vector<uint32_t> counts, twice, cleared;
    std::vector<int8_t> values;
    lslam_occ_stats st;
    bool ok = (!fit || store.occFitBounds(poses, p)) && store.occSetup(p) && store.occIntegrate(ids, poses) && store.occCounts(counts) &&
              store.occValues(values) && store.occInfo(st);
    if (!ok) { std::fprintf(stderr, "occupancy: %s\n", store.lastError().c_str()); return 3; }
    std::printf("GRID %d %d %.17g %.17g\n", st.params.width, st.params.height, st.params.origin[0], st.params.origin[1]);
    std::printf("RAYS %lld %lld %lld %lld %d\n", (long long)st.rays_cast, (long long)st.rays_dropped, (long long)st.rays_obstacle,
                (long long)st.rays_ground, st.n_integrated);
    if (!pose_graph::saveMap(argv[2], values, st.params)) { std::fprintf(stderr, "saveMap failed\n"); return 3; }
    FILE *o = std::fopen(argv[3], "wb");
    if (!o || std::fwrite(counts.data(), sizeof(uint32_t), counts.size(), o) != counts.size() || std::fclose(o) != 0) return 3;
    // refusals leave the grid alone
    std::vector<float> short_poses(poses.begin(), poses.end() - 16);
    std::vector<int32_t> bad_ids(ids);
    bad_ids.back() = n;
    const bool refused = !store.occIntegrate(ids, short_poses) && !store.occIntegrate(bad_ids, poses) && store.occCounts(twice) && twice == counts;
    std::printf("REFUSED %d\n", refused ? 1 : 0);
    ok = store.occIntegrate(ids, poses) && store.occCounts(twice) && store.occClear() && store.occCounts(cleared);
    bool doubled = ok && twice.size() == counts.size();
    for (size_t i = 0; doubled && i < counts.size(); ++i) doubled = twice[i] == 2 * counts[i] && cleared[i] == 0;
    std::printf("TWICE %d\n", doubled ? 1 : 0);
  }
  lslam_ctx_destroy(ctx);
  return rc;
}
