// lslam_dynamic_feature_map.hpp -- header-only mirror of lidar_slam::DynamicFeatureMap (util/DynamicFeatureMap.h) on the paged
// mode of the device-resident localisation node (lslam_pmap_*, include/lslam_c.h): a window of W x H x D cubes addressed by
// global cube index follows the sensor; update() reads, filters and gives a kd-tree to exactly the cubes that enter it.
//
// Clouds are packed {x, y, z, intensity} floats; a pose is the Twist rot_x rot_y rot_z pos_x pos_y pos_z.  Defaults are those of
// DynamicFeatureMap.h:76-90: 21 x 11 x 21 cubes of 50 m, valid distance 100 m, leaves 0.2 / 0.4 / 0.6.
// Not mirrored: addFeatureCloud / testAddFeatureCloud / downsizeValidCloud (LaserMatcher.cpp:350 never adds in dynamic mode),
// saveCloudToFiles (its body is commented out), getFullMap (gated on cubes nothing fills), getLocIdxCloud.
#ifndef LSLAM_DYNAMIC_FEATURE_MAP_HPP
#define LSLAM_DYNAMIC_FEATURE_MAP_HPP

#include <cstring>
#include <string>
#include <vector>

#include "lslam_c.h"

namespace lidar_slam {

class DynamicFeatureMap {
public:
  explicit DynamicFeatureMap(lslam_ctx *ctx, int cubeWidth = 21, int cubeHeight = 11, int cubeDepth = 21) : _loc(nullptr) {
    std::memset(&_last, 0, sizeof(_last));
    if (lslam_abi_version() != LSLAM_ABI_VERSION || lslam_sizeof_stats() != sizeof(lslam_stats)) {
      _err = "liblslam_hip was built from another include/lslam_c.h than this program (ABI version / struct sizes differ)";
      return;
    }
    if (lslam_loc_create(ctx, cubeWidth, cubeHeight, cubeDepth, &_loc) != LSLAM_OK) {
      _loc = nullptr;
      _err = lslam_last_error();
      return;
    }
    lslam_loc_setup_map_filter_size(_loc, 0.2f, 0.4f);
    lslam_loc_setup_world_cube_size(_loc, 50.0f);
    lslam_loc_setup_lidar_valid_distance(_loc, 100.0f);
  }
  ~DynamicFeatureMap() { lslam_loc_destroy(_loc); }
  DynamicFeatureMap(const DynamicFeatureMap &) = delete;
  DynamicFeatureMap &operator=(const DynamicFeatureMap &) = delete;
  bool ok() const { return _loc != nullptr; }

  // (the third leaf is getFullMap's, which is not built)
  bool setupFilterSize(float corner, float surf, float /*map*/ = 0.6f) { return check(lslam_loc_setup_map_filter_size(_loc, corner, surf)); }
  bool setupScanFilterSize(float corner, float surf) { return check(lslam_loc_setup_scan_filter_size(_loc, corner, surf)); }
  bool setupWorldCubeSize(float size) { return check(lslam_loc_setup_world_cube_size(_loc, size)); }
  bool setupLidarValidDistance(float dist) { return check(lslam_loc_setup_lidar_valid_distance(_loc, dist)); }
  // accepted and ignored: InVerticalFov computes the angles and decides by distance alone
  bool setupLidarFov(float /*maxUpDegree*/, float /*maxDownDegree*/) { return _loc != nullptr; }
  bool setupFilesDirectory(const std::string &filePath) { return check(lslam_pmap_open(_loc, filePath.c_str())); }
  bool setupPagedCapacity(size_t maxPointsPerType) { return check(lslam_pmap_setup_capacity(_loc, maxPointsPerType)); }
  // convertIndexFile writes "index2.txt" into the working directory in the reference; here the output is named
  static bool convertIndexFile(const std::string &filePath, int x, int y, int z, const std::string &outPath = "index2.txt") {
    return lslam_index_convert(filePath.c_str(), x, y, z, outPath.c_str()) == LSLAM_OK;
  }

  // update(sensorGlo, sensorUpDir): the up direction decides nothing in the reference and is ignored
  bool update(const float sensorGlo[3], const float * /*sensorUpDir*/ = nullptr) { return check(lslam_pmap_update(_loc, sensorGlo)); }
  bool stage(const float pos[3]) { return check(lslam_pmap_stage(_loc, pos)); }
  bool getSurroundFeature(std::vector<float> &surroundCorner, std::vector<float> &surroundSurf) {
    size_t nc = 0, ns = 0;
    if (!check(lslam_pmap_get_surround(_loc, nullptr, 0, &nc, nullptr, 0, &ns))) return false;
    surroundCorner.assign(4 * nc + 4, 0.0f);
    surroundSurf.assign(4 * ns + 4, 0.0f);
    const bool good = check(lslam_pmap_get_surround(_loc, surroundCorner.data(), nc, &nc, surroundSurf.data(), ns, &ns));
    surroundCorner.resize(4 * nc);
    surroundSurf.resize(4 * ns);
    return good;
  }
  // scanMatchScan(CornerCloud, SurfCloud, transformf): true when the loop converged; transformf is written back in every case.
  // The window is updated at transformf's translation and the clouds go through the node's scan filters first (lslam_loc_match
  // is prepareFeatureFrame + optimizeTransform; leaves 1.0 / 1.0 unless setupScanFilterSize says otherwise).
  bool scanMatchScan(const std::vector<float> &cornerCloud, const std::vector<float> &surfCloud, float transformf[6]) {
    if (!_loc) return false;
    const int rc = lslam_loc_match(_loc, cornerCloud.data(), cornerCloud.size() / 4, surfCloud.data(), surfCloud.size() / 4, 16, transformf, &_last);
    if (rc < 0) _err = lslam_last_error();
    return rc == LSLAM_OK;
  }
  // the overload that also reports the match counts (DynamicFeatureMap.h: scanMatchScan(..., line_match_count, plane_match_count))
  bool scanMatchScan(const std::vector<float> &cornerCloud, const std::vector<float> &surfCloud, float transformf[6], int &lineMatchCount,
                     int &planeMatchCount) {
    const bool good = scanMatchScan(cornerCloud, surfCloud, transformf);
    lineMatchCount = _last.n_line;
    planeMatchCount = _last.n_plane;
    return good;
  }
  bool windowInfo(lslam_loc_window_stats *out) { return check(lslam_pmap_window_info(_loc, out)); }
  const lslam_stats &lastStats() const { return _last; }
  const std::string &lastError() const { return _err; }
  lslam_loc *handle() { return _loc; }

private:
  bool check(int rc) {
    if (rc < 0) _err = lslam_last_error();
    return rc >= 0;
  }
  lslam_loc *_loc;
  lslam_stats _last;
  std::string _err;
};

}  // namespace lidar_slam
#endif  // LSLAM_DYNAMIC_FEATURE_MAP_HPP
