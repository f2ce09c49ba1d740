// lslam_survey_map.hpp -- the reference's featureExtracter executable (io_module/feature_extracter.cpp:43-130) as a class over
// the C ABI (lslam_survey_*, include/lslam_c.h): a dense survey cloud becomes the corner / surf cube map that
// LaserLocalization::loadMap opens.  C++11, header only; never throws: ok() / lastError() report.
//
//   lidar_slam::FeatureExtracter fx(ctx);          // params() holds the reference's literals; change them before extract
//   if (fx.extract(cloud.points) && fx.saveCloudToFiles(dir)) localization.loadMap(dir);
//
// The result stays on the device between extract and saveCloudToFiles / getFeatureClouds; a second extract replaces it.
#pragma once

#include <cstddef>
#include <string>
#include <vector>

#include "lslam_c.h"

namespace lidar_slam {

class FeatureExtracter {
public:
  explicit FeatureExtracter(lslam_ctx *ctx) : _ctx(ctx), _map(nullptr) {
    lslam_survey_default_params(&_params);
    if (lslam_abi_version() != LSLAM_ABI_VERSION)
      _err = "liblslam_hip was built from another include/lslam_c.h than this program (ABI version differs)";
  }
  ~FeatureExtracter() { lslam_survey_destroy(_map); }
  FeatureExtracter(const FeatureExtracter &) = delete;
  FeatureExtracter &operator=(const FeatureExtracter &) = delete;
  bool ok() const { return _ctx != nullptr && _err.empty(); }
  lslam_survey_params &params() { return _params; }
  // points: any record type that starts with float x, y, z (pcl::PointXYZ, PointXYZI, ...)
  template <class PointT>
  bool extract(const std::vector<PointT> &points) {
    return extract(points.empty() ? nullptr : &points[0], points.size(), sizeof(PointT));
  }
  bool extract(const void *cloud, size_t n, size_t strideBytes) {
    drop();
    return check(lslam_survey_extract(_ctx, cloud, n, strideBytes, &_params, &_map));
  }
  // pcl::io::loadPCDFile of the executable's argv[1] (DATA ascii or binary)
  bool extractFile(const std::string &pcdPath) {
    drop();
    return check(lslam_survey_extract_file(_ctx, pcdPath.c_str(), &_params, &_map));
  }
  bool stats(lslam_survey_stats *out) { return check(lslam_survey_info(_map, out)); }
  // packed {x, y, z, intensity = 0}, axes permuted as the reference does
  bool getFeatureClouds(std::vector<float> &corner, std::vector<float> &surf) {
    lslam_survey_stats st;
    if (!stats(&st)) return false;
    corner.resize((size_t)st.n_corner * 4);
    surf.resize((size_t)st.n_surf * 4);
    return check(lslam_survey_get(_map, corner.empty() ? nullptr : &corner[0], (size_t)st.n_corner, surf.empty() ? nullptr : &surf[0],
                                  (size_t)st.n_surf));
  }
  // _featureCloud.saveCloudToFiles(): index.txt and <count>.pcd
  bool saveCloudToFiles(const std::string &directory) { return check(lslam_survey_save(_map, directory.c_str())); }
  const std::string &lastError() const { return _err; }
  lslam_survey *handle() { return _map; }

private:
  void drop() {
    lslam_survey_destroy(_map);
    _map = nullptr;
  }
  bool check(int rc) {
    if (rc != LSLAM_OK) _err = lslam_last_error();
    return rc == LSLAM_OK;
  }
  lslam_ctx *_ctx;
  lslam_survey *_map;
  lslam_survey_params _params;
  std::string _err;
};

}  // namespace lidar_slam
