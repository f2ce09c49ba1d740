// C++ drop-in check of include/lslam_pipeline.hpp's OrganisedScanRegistration mirror through the C ABI.  Reads organised sweeps
// and IMU messages from a file written by the test -- records of a uint32 tag: 1 = IMU {int64 stamp, double roll, pitch, yaw,
// double acceleration[3]}, 2 = cloud {int64 stamp, uint32 height, uint32 width, height x width points of 32 bytes: {x, y, z}
// floats, the ring as a uint16 at byte 26} -- feeds them through OrganisedScanRegistration::handleIMUMessage / process and
// LaserOdometry::processFeatureSet and prints one "SWEEP" line per cloud (with a checksum of laserCloud's cloud and ranges),
// which the test compares with the Python mirrors (same ABI calls: same bits).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lslam_pipeline.hpp"
#include "lslam_scan_match.hpp"

struct PointXYZIT {  // the reference's driver point: 32 bytes, ring at 26
  float x, y, z, pad;
  float intensity;
  float timestamp;
  uint16_t pad2;
  uint16_t ring;
  float pad3;
};
static_assert(sizeof(PointXYZIT) == 32, "the file's point");
struct OrganisedCloud {
  uint32_t height, width;
  std::vector<PointXYZIT> points;
};

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  lidar_slam::ScanMatch sm(10);  // owns the context; never throws
  if (!sm.ok()) {
    std::fprintf(stderr, "backend unavailable: %s\n", sm.initError().c_str());
    return 1;
  }
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  lidar_slam::OrganisedScanRegistration registration(sm.context());
  lidar_slam::LaserOdometry odometry(sm.context());
  if (!registration.ok()) {
    std::fprintf(stderr, "registration unavailable: %s\n", registration.lastError().c_str());
    return 1;
  }
  OrganisedCloud cloud;
  uint32_t tag = 0;
  int sweep = 0;
  while (std::fread(&tag, 4, 1, f) == 1) {
    int64_t stamp = 0;
    if (std::fread(&stamp, 8, 1, f) != 1) return 2;
    if (tag == 1) {
      double v[6];
      if (std::fread(v, 8, 6, f) != 6) return 2;
      if (!registration.handleIMUMessage(stamp, v[0], v[1], v[2], v + 3)) {
        std::fprintf(stderr, "IMU message refused: %s\n", registration.lastError().c_str());
        return 1;
      }
      continue;
    }
    if (std::fread(&cloud.height, 4, 1, f) != 1 || std::fread(&cloud.width, 4, 1, f) != 1) return 2;
    const size_t n = (size_t)cloud.height * cloud.width;
    cloud.points.resize(n);
    if (n && std::fread(&cloud.points[0], sizeof(PointXYZIT), n, f) != n) return 2;
    if (!registration.process(cloud, stamp)) {
      std::fprintf(stderr, "registration failed: %s\n", registration.lastError().c_str());
      return 1;
    }
    const bool matched = odometry.processFeatureSet(registration.featureSet());
    if (!odometry.lastError().empty()) {
      std::fprintf(stderr, "odometry failed: %s\n", odometry.lastError().c_str());
      return 1;
    }
    std::printf("SWEEP %d %d %d", sweep, registration.hasIMUData() ? 1 : 0, matched ? 1 : 0);
    for (int k = 0; k < 4; ++k) std::printf(" %zu", registration.counts()[k]);
    for (int k = 0; k < 12; ++k) std::printf(" %a", (double)registration.imuTrans()[k]);
    for (int k = 0; k < 6; ++k) std::printf(" %a", (double)odometry.transform()[k]);
    // the registered cloud and the ranges, into vectors the mirror sizes itself: a checksum of the bits
    std::vector<float> registered;
    std::vector<int32_t> ranges;
    if (!registration.laserCloud(registered, &ranges)) {
      std::fprintf(stderr, "laserCloud failed: %s\n", registration.lastError().c_str());
      return 1;
    }
    uint64_t sum = 1469598103934665603ull;  // FNV-1a over the cloud's words, then the ranges
    for (size_t k = 0; k < registered.size(); ++k) {
      uint32_t w;
      std::memcpy(&w, &registered[k], 4);
      sum = (sum ^ w) * 1099511628211ull;
    }
    for (size_t k = 0; k < ranges.size(); ++k) sum = (sum ^ (uint32_t)ranges[k]) * 1099511628211ull;
    std::printf(" %zu %zu %llx\n", registered.size() / 4, ranges.size() / 2, (unsigned long long)sum);
    ++sweep;
  }
  std::fclose(f);
  std::printf("OK sweeps %d\n", sweep);
  return 0;
}
