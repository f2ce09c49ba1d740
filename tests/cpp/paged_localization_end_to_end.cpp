// C++ drop-in check of the paged localisation mirrors through the C ABI: lidar_slam::LaserLocalization with setDynamicMode /
// setupFilesDirectory (include/lslam_pipeline.hpp) and lidar_slam::DynamicFeatureMap (include/lslam_dynamic_feature_map.hpp)
// over a map saved with saveCloudToFiles (lslam_fmap_save) and converted with convertIndexFile.
// argv: session file, map directory, the saved map's origin ox oy oz, the window W H D, cube size, valid distance.
// The session: 16 floats start pose, then records of {int64 stamp, 16 floats odometry pose, uint32 nc, nc x {x,y,z,w}, uint32 ns,
// ns x {x,y,z,w}}.  One "SWEEP" line per record with the flags, the match's counters, the pose and the velocity; then a "MAP"
// line from DynamicFeatureMap at the first record's position.  The test compares them with the Python run (same ABI calls).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "lslam_dynamic_feature_map.hpp"
#include "lslam_pipeline.hpp"
#include "lslam_scan_match.hpp"

static bool read_cloud(FILE *f, std::vector<float> &out) {
  uint32_t n = 0;
  if (std::fread(&n, 4, 1, f) != 1) return false;
  out.resize((size_t)n * 4);
  return n == 0 || std::fread(&out[0], 16, n, f) == n;
}

int main(int argc, char **argv) {
  if (argc < 11) return 2;
  lidar_slam::ScanMatch sm(10);  // owns the context; never throws
  if (!sm.ok()) {
    std::fprintf(stderr, "backend unavailable: %s\n", sm.initError().c_str());
    return 1;
  }
  const std::string dir(argv[2]);
  const int W = std::atoi(argv[6]), H = std::atoi(argv[7]), D = std::atoi(argv[8]);
  const float cube = (float)std::atof(argv[9]), valid = (float)std::atof(argv[10]);
  if (!lidar_slam::DynamicFeatureMap::convertIndexFile(dir + "/index.txt", std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]),
                                                       dir + "/index2.txt")) {
    std::fprintf(stderr, "index not converted: %s\n", lslam_last_error());
    return 1;
  }
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  float start[16];
  if (std::fread(start, 4, 16, f) != 16) return 2;
  lidar_slam::LaserLocalization localization(sm.context(), W, H, D);
  if (!localization.ok()) {
    std::fprintf(stderr, "node unavailable: %s\n", localization.lastError().c_str());
    return 1;
  }
  if (localization.setupFilesDirectory(dir)) return 3;  // refused while the dynamic mode is off
  if (!localization.setupWorldCubeSize(cube) || !localization.setupLidarValidDistance(valid) || !localization.setDynamicMode(true) ||
      !localization.setupFilesDirectory(dir) || !localization.handleInitialPose(start)) {
    std::fprintf(stderr, "paged map not opened: %s\n", localization.lastError().c_str());
    return 1;
  }
  std::vector<float> corner, surf, corner0, surf0;
  float odom[16], first[3] = {0, 0, 0};
  int64_t stamp = 0;
  int sweep = 0;
  while (std::fread(&stamp, 8, 1, f) == 1) {
    if (std::fread(odom, 4, 16, f) != 16 || !read_cloud(f, corner) || !read_cloud(f, surf)) return 2;
    if (sweep == 0) {
      corner0 = corner;
      surf0 = surf;
      first[0] = odom[3]; first[1] = odom[7]; first[2] = odom[11];
    }
    if (!localization.process(corner, surf, odom, stamp)) {
      std::fprintf(stderr, "localisation failed: %s\n", localization.lastError().c_str());
      return 1;
    }
    const lslam_stats &st = localization.lastStats();
    lslam_loc_window_stats w;
    if (!localization.windowInfo(&w)) return 1;
    std::printf("SWEEP %d %d %d %d %d %d %d %d %d %d %d", sweep, localization.flags(), st.status, st.iterations, st.n_line, st.n_plane, st.n_rows,
                w.centre[0], w.centre[1], w.centre[2], (int)w.files_read_total);
    for (int k = 0; k < 16; ++k) std::printf(" %a", (double)localization.lidarMapped()[k]);
    for (int k = 0; k < 3; ++k) std::printf(" %a", (double)localization.velocity()[k]);
    std::printf("\n");
    ++sweep;
  }
  std::fclose(f);
  lidar_slam::DynamicFeatureMap map(sm.context(), W, H, D);
  std::vector<float> sc, ss;
  float pose[6] = {0.f, 0.f, 0.f, first[0], first[1], first[2]};
  int lines = 0, planes = 0;
  if (!map.ok() || !map.setupFilterSize(1.0f, 1.0f, 0.6f) || !map.setupWorldCubeSize(cube) || !map.setupLidarValidDistance(valid) ||
      !map.setupLidarFov(20.0f, 20.0f) || !map.setupFilesDirectory(dir) || !map.update(first) || !map.getSurroundFeature(sc, ss)) {
    std::fprintf(stderr, "DynamicFeatureMap failed: %s\n", map.lastError().c_str());
    return 1;
  }
  pose[2] = 0.3f;
  const bool converged = map.scanMatchScan(corner0, surf0, pose, lines, planes);
  std::printf("MAP %d %d %d %d %d %d", (int)(sc.size() / 4), (int)(ss.size() / 4), converged ? 1 : 0, lines, planes, map.lastStats().iterations);
  for (int k = 0; k < 6; ++k) std::printf(" %a", (double)pose[k]);
  std::printf("\n");
  std::printf("OK sweeps %d\n", sweep);
  return 0;
}
