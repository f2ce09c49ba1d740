// C++ drop-in check of include/lslam_pipeline.hpp's LaserMappingLocal / LocalFeatureMap mirrors through the C ABI.  Reads the
// corner / surf clouds and the odometry pose of N consecutive sweeps from a file written by the test (per sweep: uint32 count +
// count x {x,y,z,intensity} floats, twice, then 16 floats), feeds them through LaserMappingLocal::process and prints one "POSE"
// line per sweep, which the test compares with the Python mirror (same ABI calls: same bits).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lslam_pipeline.hpp"
#include "lslam_scan_match.hpp"

static bool read_cloud(FILE *f, std::vector<float> &c) {
  uint32_t n = 0;
  if (std::fread(&n, 4, 1, f) != 1) return false;
  c.resize(4 * (size_t)n);
  return n == 0 || std::fread(c.data(), 16, n, f) == n;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  lidar_slam::ScanMatch sm(10);  // owns the context; never throws
  if (!sm.ok()) {
    std::fprintf(stderr, "backend unavailable: %s\n", sm.initError().c_str());
    return 1;
  }
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  lidar_slam::LaserMappingLocal mapping(sm.context(), 1.0f, 1.0f, 30.0, 1u << 18, 64);
  std::vector<float> corner, surf, sc, ss;
  float odom[16];
  int sweep = 0;
  while (read_cloud(f, corner) && read_cloud(f, surf) && std::fread(odom, 4, 16, f) == 16) {
    if (!mapping.process(corner, surf, odom)) {
      std::fprintf(stderr, "mapping failed: %s\n", mapping.lastError().c_str());
      return 1;
    }
    mapping.featureMap().clean();
    if (!mapping.featureMap().getSurroundFeature(sc, ss)) return 1;
    const float *T = mapping.lidarMapped();
    std::printf("POSE %d", sweep);
    for (int i = 0; i < 12; ++i) std::printf(" %a", (double)T[i]);
    std::printf(" %zu %zu\n", sc.size() / 4, ss.size() / 4);
    ++sweep;
  }
  std::fclose(f);
  std::printf("OK sweeps %d\n", sweep);
  return 0;
}
