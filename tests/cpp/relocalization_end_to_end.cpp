// C++ drop-in check of LaserLocalization::relocalize (include/lslam_pipeline.hpp) through the C ABI.  argv[1]: a file written by
// the test -- six arrays, each a uint32 count of floats followed by the floats: map corner, map surf, sweep corner, sweep surf
// (packed {x, y, z, w}), rotations (angle triplets), positions -- then the three cube-grid dimensions, the voxel edge and whether
// the rotation indices wrap.  The node gets the map, no initial pose: a sweep is dropped, relocalize(apply) finds the pose, the
// next sweep is processed.  One "RELOC" line and one "SWEEP" line, which the test compares with the Python mirror's run (same ABI
// calls: same bits).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lslam_pipeline.hpp"
#include "lslam_scan_match.hpp"

static bool read_array(FILE *f, std::vector<float> &out) {
  uint32_t n = 0;
  if (std::fread(&n, 4, 1, f) != 1) return false;
  out.resize(n);
  return n == 0 || std::fread(&out[0], sizeof(float), n, f) == n;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  lidar_slam::ScanMatch sm(10);  // owns the context; never throws
  if (!sm.ok()) {
    std::fprintf(stderr, "backend unavailable: %s\n", sm.initError().c_str());
    return 1;
  }
  if (argc < 7) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<float> a[6];
  for (int k = 0; k < 6; ++k)
    if (!read_array(f, a[k])) return 2;
  std::fclose(f);
  lidar_slam::LaserLocalization localization(sm.context(), std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
  if (!localization.ok() || !localization.setMap(a[0], a[1], false)) {
    std::fprintf(stderr, "node unavailable: %s\n", localization.lastError().c_str());
    return 1;
  }
  const float odom[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  if (localization.process(a[2], a[3], odom, 1000000000) || !localization.dropped()) return 3;  // no pose yet: dropped
  lslam_reloc_opts opts;
  std::memset(&opts, 0, sizeof(opts));
  opts.voxel = (float)std::atof(argv[5]);
  opts.rot_cyclic = std::atoi(argv[6]);
  opts.apply = 1;
  if (!localization.relocalize(a[2], a[3], a[4], a[5], &opts)) {
    std::fprintf(stderr, "not relocalised: status %d %s\n", localization.relocStatus(), localization.lastError().c_str());
    return 1;
  }
  const lslam_reloc_result &r = localization.relocResult();
  std::printf("RELOC %d %d %d %d %a", r.accepted, r.winner, r.runner_up, r.n_candidates, (double)r.fraction);
  for (int k = 0; k < 16; ++k) std::printf(" %a", (double)r.T[k]);
  std::printf("\n");
  if (!localization.process(a[2], a[3], odom, 1200000000)) {
    std::fprintf(stderr, "localisation failed: %s\n", localization.lastError().c_str());
    return 1;
  }
  std::printf("SWEEP %d", localization.flags());
  for (int k = 0; k < 16; ++k) std::printf(" %a", (double)localization.lidarMapped()[k]);
  std::printf("\n");
  return 0;
}
