// C++ drop-in check of include/lslam_pipeline.hpp's LaserLocalization mirror through the C ABI: registration -> odometry ->
// localisation over a loaded map.  argv: a session file written by the test -- records of a uint32 tag 2 = cloud {int64 stamp,
// uint32 count, count x {x,y,z,w} floats} -- the directory of a map saved with saveCloudToFiles (lslam_fmap_save) and the three
// cube-grid dimensions.  Every cloud goes through MultiScanRegistration::process, LaserOdometry::processFeatureSet and
// LaserLocalization::process (the odometry node's last clouds and _Tsum); one "SWEEP" line per cloud with the flags, the
// match's counters, the pose and the velocity, which the test compares with the Python mirrors (same ABI calls: same bits).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lslam_pipeline.hpp"
#include "lslam_scan_match.hpp"

struct RawPoint {
  float x, y, z, w;
};
struct RawCloud {
  std::vector<RawPoint> points;
};

int main(int argc, char **argv) {
  if (argc < 6) return 2;
  lidar_slam::ScanMatch sm(10);  // owns the context; never throws
  if (!sm.ok()) {
    std::fprintf(stderr, "backend unavailable: %s\n", sm.initError().c_str());
    return 1;
  }
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  lidar_slam::MultiScanRegistration registration(sm.context());
  lidar_slam::LaserOdometry odometry(sm.context());
  lidar_slam::LaserLocalization localization(sm.context(), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]));
  if (!registration.ok() || !localization.ok()) {
    std::fprintf(stderr, "node unavailable: %s%s\n", registration.lastError().c_str(), localization.lastError().c_str());
    return 1;
  }
  if (!localization.loadMap(argv[2])) {
    std::fprintf(stderr, "map not loaded: %s\n", localization.lastError().c_str());
    return 1;
  }
  const float start[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  RawCloud cloud;
  uint32_t tag = 0;
  int sweep = 0;
  while (std::fread(&tag, 4, 1, f) == 1) {
    int64_t stamp = 0;
    uint32_t n = 0;
    if (tag != 2 || std::fread(&stamp, 8, 1, f) != 1 || std::fread(&n, 4, 1, f) != 1) return 2;
    cloud.points.resize(n);
    if (n && std::fread(&cloud.points[0], sizeof(RawPoint), n, f) != n) return 2;
    if (!registration.process(cloud, stamp)) {
      std::fprintf(stderr, "registration failed: %s\n", registration.lastError().c_str());
      return 1;
    }
    odometry.processFeatureSet(registration.featureSet());
    if (!odometry.lastError().empty()) {
      std::fprintf(stderr, "odometry failed: %s\n", odometry.lastError().c_str());
      return 1;
    }
    if (sweep == 1 && !localization.handleInitialPose(start)) return 1;  // the first sweep arrives before the initial pose: dropped
    const bool done = localization.process(odometry.lastCornerCloud(), odometry.lastSurfaceCloud(), odometry.Tsum(), stamp);
    if (!done && !localization.dropped()) {
      std::fprintf(stderr, "localisation failed: %s\n", localization.lastError().c_str());
      return 1;
    }
    const lslam_stats &st = localization.lastStats();
    std::printf("SWEEP %d %d %d %d %d %d %d", sweep, localization.flags(), done ? st.status : -100, done ? st.iterations : 0,
                done ? st.n_line : 0, done ? st.n_plane : 0, done ? st.n_rows : 0);
    for (int k = 0; k < 16; ++k) std::printf(" %a", (double)localization.lidarMapped()[k]);
    for (int k = 0; k < 3; ++k) std::printf(" %a", (double)localization.velocity()[k]);
    std::printf("\n");
    ++sweep;
  }
  std::fclose(f);
  std::printf("OK sweeps %d\n", sweep);
  return 0;
}
