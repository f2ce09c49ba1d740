// lslam_pipeline.hpp -- header-only C++ mirrors of the per-sweep state machines either side of the
// scan-match hot path, over the C ABI (lslam_c.h):
//
//   lidar_slam::MultiScanRegistration    odometry/MultiScanRegistration.cpp:78-200 on ScanRegistration.cpp:89-188, :684-707
//                                        (handleIMUMessage, handleCloudMessage, process: the registration node, lslam_sreg_*)
//   lidar_slam::OrganisedScanRegistration  odometry/OrganizedScanRegistration.cpp:82-150: the same node for a height x width cloud
//                                        whose points carry their ring (lslam_oreg_*)
//   lidar_slam::LaserOdometry::process   /root/reference/L_SLAM/src/odometry/LaserOdometry.cpp:288-326
//                                        (+ scanMatch :328-647 = lslam_odometry_match, transformToEnd
//                                        :156-168 = lslam_transform_to_end, transformUpdate :649-653)
//   lidar_slam::LaserMapping::process    odometry/LaserMapping.cpp:39-59 over LaserMatcher
//                                        (odometry/LaserMatcher.cpp:289-354: prepareFeatureFrame,
//                                        prepareFeatureSurround, optimizeTransform, transformMerge /
//                                        transformUpdate, featureMapUpdate)
//   lidar_slam::LaserMappingLocal::process  odometry/LaserMappingLocal.cpp:39-83: the same matcher over the sliding window of
//                                        recent frames, io_module/LocalFeatureMap.h (lidar_slam::LocalFeatureMap below)
//   lidar_slam::LaserLocalization::process  odometry/LaserLocalization.cpp:140-188: localisation over a prebuilt map, the node
//                                        resident on the device (lslam_loc_*)
//
// ROS plumbing (topics, time-stamp matching, tf, frame skipping) is the host program's.  Clouds are any
// type with `.points` (std::vector-like) of points with float x, y, z and `intensity` (= ring + relTime);
// sizeof(point) is the stride, the intensity is read where the member lies.  Poses are row-major 4x4
// float arrays (Eigen::Isometry3f::matrix() transposed into row order by the caller's adapter).
// Like the reference's nodes these objects never throw; a backend failure makes process() return false
// and leaves the message in lastError().
#pragma once

#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "lslam_c.h"

namespace lidar_slam {

namespace detail {
// pack a cloud into {x, y, z, intensity} floats (the layout every lslam_* cloud entry point accepts with stride 16)
template <typename Cloud>
inline void pack_xyzi(const Cloud &c, std::vector<float> &out) {
  out.resize(4 * c.points.size());
  for (size_t i = 0; i < c.points.size(); ++i) {
    out[4 * i] = c.points[i].x;
    out[4 * i + 1] = c.points[i].y;
    out[4 * i + 2] = c.points[i].z;
    out[4 * i + 3] = c.points[i].intensity;
  }
}
inline void mat_mul4(const float A[16], const float B[16], float C[16]) {
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      float s = 0.f;
      for (int k = 0; k < 4; ++k) s += A[r * 4 + k] * B[k * 4 + c];
      C[r * 4 + c] = s;
    }
}
inline void identity4(float T[16]) {
  std::memset(T, 0, 16 * sizeof(float));
  T[0] = T[5] = T[10] = T[15] = 1.f;
}
}  // namespace detail

// MultiScanRegistration (the first node of the sweep chain): raw driver cloud in, the sweep's four feature lists in HBM out --
// ring and relTime, the IMU de-skew, the grouping by ring and the feature extraction on the device behind one wait
// (lslam_sreg_*, include/lslam_c.h).  The ROS side stays the host program's: handleIMUMessage takes the stamp in nanoseconds
// and the roll / pitch / yaw tf's getRPY gave, handleCloudMessage / process the cloud (any type with `.points` of points with
// float x, y, z first) and its stamp.  featureSet() is what LaserOdometry::processFeatureSet takes.
class MultiScanRegistration {
public:
  explicit MultiScanRegistration(lslam_ctx *ctx, float lowerBound = -15.f, float upperBound = 15.f, int nScanRings = 16,
                                 float scanPeriod = 0.1f, const lslam_reg_params *config = nullptr, int imuHistorySize = 200)
      : _sr(nullptr), _fs(nullptr), _nScanRings(nScanRings), _systemDelay(SYSTEM_DELAY), _cloudReceiveCount(0) {
    std::memset(_imuTrans, 0, sizeof(_imuTrans));
    std::memset(_counts, 0, sizeof(_counts));
    std::memset(&_stats, 0, sizeof(_stats));
    if (lslam_abi_version() != LSLAM_ABI_VERSION || lslam_sizeof_opts() != sizeof(lslam_opts) || lslam_sizeof_stats() != sizeof(lslam_stats)) {
      _err = "liblslam_hip was built from another include/lslam_c.h than this program (ABI version / struct sizes differ)";
      return;
    }
    if (lslam_sreg_create(ctx, config, lowerBound, upperBound, nScanRings, scanPeriod, imuHistorySize, &_sr) != LSLAM_OK ||
        lslam_fset_create(ctx, &_fs) != LSLAM_OK)
      _err = lslam_last_error();
  }
  ~MultiScanRegistration() {
    if (_sr) lslam_sreg_destroy(_sr);
    if (_fs) lslam_fset_destroy(_fs);
  }
  MultiScanRegistration(const MultiScanRegistration &) = delete;
  MultiScanRegistration &operator=(const MultiScanRegistration &) = delete;
  enum { SYSTEM_DELAY = 2 };  // the first clouds of a session are skipped (MultiScanRegistration.cpp:82-85)
  bool ok() const { return _sr && _fs; }
  // ScanRegistration::handleIMUMessage after getRPY; false for a stamp that is not later than the previous one
  bool handleIMUMessage(int64_t stampNs, double roll, double pitch, double yaw, const double linearAcceleration[3]) {
    if (!ok()) return false;
    return lslam_sreg_imu_push(_sr, stampNs, roll, pitch, yaw, linearAcceleration) == LSLAM_OK || fail();
  }
  bool hasIMUData() const {
    int32_t n = 0;
    return _sr && lslam_sreg_imu_info(_sr, &n, nullptr, nullptr) == LSLAM_OK && n > 0;
  }
  // false while the system delay lasts (nothing processed) and on a backend error
  template <typename Cloud>
  bool handleCloudMessage(const Cloud &laserCloudIn, int64_t stampNs) {
    ++_cloudReceiveCount;
    if (_systemDelay > 0) {
      --_systemDelay;
      return false;
    }
    return process(laserCloudIn, stampNs);
  }
  template <typename Cloud>
  bool process(const Cloud &laserCloudIn, int64_t scanTimeNs) {
    if (!ok()) return false;
    const size_t n = laserCloudIn.points.size();
    const void *p = n ? static_cast<const void *>(&laserCloudIn.points[0]) : nullptr;
    if (lslam_sreg_process(_sr, p, n, sizeof(laserCloudIn.points[0]), scanTimeNs, _fs, _counts, _imuTrans, &_stats) < 0) return fail();
    return true;
  }
  lslam_fset *featureSet() const { return _fs; }  // /laser_cloud_sharp, _less_sharp, _flat, _less_flat, in HBM
  const size_t *counts() const { return _counts; }
  const float *imuTrans() const { return _imuTrans; }  // /imu_trans: four points {x, y, z}
  // /velodyne_cloud_2 on request: packed {x', y', z', ring + relTime}; ranges (optional): resized to nScanRings x {first, last}
  bool laserCloud(std::vector<float> &cloud, std::vector<int32_t> *ranges = nullptr) {
    if (!ok()) return false;
    cloud.resize(4 * _stats.n_points);
    if (ranges) ranges->assign(2 * (size_t)(_nScanRings > 0 ? _nScanRings : 0), 0);
    size_t n = 0;
    if (lslam_sreg_cloud(_sr, cloud.data(), _stats.n_points, &n, ranges ? ranges->data() : nullptr) < 0) {
      cloud.clear();
      return fail();
    }
    cloud.resize(4 * n);
    return true;
  }
  const lslam_sreg_stats &nodeStats() const { return _stats; }
  long cloudReceiveCount() const { return _cloudReceiveCount; }
  const std::string &lastError() const { return _err; }

private:
  bool fail() {
    _err = lslam_last_error();
    return false;
  }
  lslam_sreg *_sr;
  lslam_fset *_fs;
  int _nScanRings;
  int _systemDelay;
  long _cloudReceiveCount;
  size_t _counts[4];
  float _imuTrans[12];
  lslam_sreg_stats _stats;
  std::string _err;
};

// OrganisedScanRegistration: the registration node for an organised cloud (the reference's Pandar / Ouster front end) -- any
// type with `.height`, `.width` and `.points` (row-major, height * width of them) whose points have float x, y, z first and a
// uint16_t member `ring`; sizeof(point) is the stride and the ring is read where the member lies.  Validity, relTime from the
// column, ring + relTime, the rows concatenated, the ranges and the extraction run on the device behind one wait (lslam_oreg_*,
// include/lslam_c.h).  As in the reference an IMU that has been heard changes /imu_trans only: the points are not de-skewed.
class OrganisedScanRegistration {
public:
  explicit OrganisedScanRegistration(lslam_ctx *ctx, float scanPeriod = 0.1f, float blindRadius = 2.5f,
                                     const lslam_reg_params *config = nullptr, int imuHistorySize = 200)
      : _og(nullptr), _fs(nullptr), _height(0), _systemDelay(SYSTEM_DELAY), _cloudReceiveCount(0) {
    std::memset(_imuTrans, 0, sizeof(_imuTrans));
    std::memset(_counts, 0, sizeof(_counts));
    std::memset(&_stats, 0, sizeof(_stats));
    if (lslam_abi_version() != LSLAM_ABI_VERSION || lslam_sizeof_opts() != sizeof(lslam_opts) || lslam_sizeof_stats() != sizeof(lslam_stats)) {
      _err = "liblslam_hip was built from another include/lslam_c.h than this program (ABI version / struct sizes differ)";
      return;
    }
    if (lslam_oreg_create(ctx, config, scanPeriod, blindRadius, imuHistorySize, &_og) != LSLAM_OK || lslam_fset_create(ctx, &_fs) != LSLAM_OK)
      _err = lslam_last_error();
  }
  ~OrganisedScanRegistration() {
    if (_og) lslam_oreg_destroy(_og);
    if (_fs) lslam_fset_destroy(_fs);
  }
  OrganisedScanRegistration(const OrganisedScanRegistration &) = delete;
  OrganisedScanRegistration &operator=(const OrganisedScanRegistration &) = delete;
  enum { SYSTEM_DELAY = 2 };  // the first clouds of a session are skipped (OrganizedScanRegistration.cpp:62-65)
  bool ok() const { return _og && _fs; }
  // ScanRegistration::handleIMUMessage after getRPY; false for a stamp that is not later than the previous one
  bool handleIMUMessage(int64_t stampNs, double roll, double pitch, double yaw, const double linearAcceleration[3]) {
    if (!ok()) return false;
    return lslam_oreg_imu_push(_og, stampNs, roll, pitch, yaw, linearAcceleration) == LSLAM_OK || fail();
  }
  bool hasIMUData() const {
    int32_t n = 0;
    return _og && lslam_oreg_imu_info(_og, &n, nullptr, nullptr) == LSLAM_OK && n > 0;
  }
  // false while the system delay lasts (nothing processed) and on a backend error
  template <typename Cloud>
  bool handleCloudMessage(const Cloud &laserCloudIn, int64_t stampNs) {
    ++_cloudReceiveCount;
    if (_systemDelay > 0) {
      --_systemDelay;
      return false;
    }
    return process(laserCloudIn, stampNs);
  }
  template <typename Cloud>
  bool process(const Cloud &laserCloudIn, int64_t scanTimeNs) {
    if (!ok()) return false;
    const size_t h = laserCloudIn.height, w = laserCloudIn.width;
    if (laserCloudIn.points.size() != h * w) {
      _err = "OrganisedScanRegistration::process: the cloud is not height x width";
      return false;
    }
    const void *p = nullptr;
    size_t ringOffset = 0;
    if (h && w) {
      p = static_cast<const void *>(&laserCloudIn.points[0]);
      ringOffset = (size_t)(reinterpret_cast<const char *>(&laserCloudIn.points[0].ring) - static_cast<const char *>(p));
    }
    if (lslam_oreg_process(_og, p, h, w, sizeof(laserCloudIn.points[0]), ringOffset, scanTimeNs, _fs, _counts, _imuTrans, &_stats) < 0)
      return fail();
    _height = h;
    return true;
  }
  lslam_fset *featureSet() const { return _fs; }  // /laser_cloud_sharp, _less_sharp, _flat, _less_flat, in HBM
  const size_t *counts() const { return _counts; }
  const float *imuTrans() const { return _imuTrans; }  // /imu_trans: four points {x, y, z}
  // /velodyne_cloud_2 on request: packed {x, y, z, ring + relTime}; ranges (optional): resized to height x {first, last}
  bool laserCloud(std::vector<float> &cloud, std::vector<int32_t> *ranges = nullptr) {
    if (!ok()) return false;
    cloud.resize(4 * _stats.n_points);
    if (ranges) ranges->assign(2 * _height, 0);
    size_t n = 0;
    if (lslam_oreg_cloud(_og, cloud.data(), _stats.n_points, &n, ranges ? ranges->data() : nullptr) < 0) {
      cloud.clear();
      return fail();
    }
    cloud.resize(4 * n);
    return true;
  }
  const lslam_oreg_stats &nodeStats() const { return _stats; }
  long cloudReceiveCount() const { return _cloudReceiveCount; }
  const std::string &lastError() const { return _err; }

private:
  bool fail() {
    _err = lslam_last_error();
    return false;
  }
  lslam_oreg *_og;
  lslam_fset *_fs;
  size_t _height;
  int _systemDelay;
  long _cloudReceiveCount;
  size_t _counts[4];
  float _imuTrans[12];
  lslam_oreg_stats _stats;
  std::string _err;
};

// LaserOdometry (variant B, BASELINE configs[0]): first sweep initialises the "last" clouds; afterwards
// scanMatch against them with the persistent _transform as the initial guess, _Tsum = _Tsum * transform,
// transformToEnd of the less-sharp / less-flat clouds, which become the next "last" clouds
// (LaserOdometry.cpp:288-326).  The node's state lives in HBM (lslam_odom, include/lslam_c.h): the last clouds and
// their search grids never leave the device; process() takes the sweep's four clouds from the host (one upload),
// processFeatureSet() takes them where lslam_extract_features_dev left them.
class LaserOdometry {
public:
  explicit LaserOdometry(lslam_ctx *ctx, int maxIterations = 25, float deltaTAbort = 0.1f, float deltaRAbort = 0.1f)
      : _ctx(ctx), _od(nullptr), _fs(nullptr), _matched(false) {
    std::memset(_transform, 0, sizeof(_transform));
    detail::identity4(_Tsum);
    std::memset(&_last, 0, sizeof(_last));
    std::memset(&_ostats, 0, sizeof(_ostats));
    if (lslam_odom_create(ctx, maxIterations, deltaTAbort, deltaRAbort, &_od) != LSLAM_OK ||
        lslam_fset_create(ctx, &_fs) != LSLAM_OK)
      _err = lslam_last_error();
  }
  ~LaserOdometry() {
    if (_od) lslam_odom_destroy(_od);
    if (_fs) lslam_fset_destroy(_fs);
  }
  LaserOdometry(const LaserOdometry &) = delete;
  LaserOdometry &operator=(const LaserOdometry &) = delete;
  // LaserOdometry.cpp:288-326.  Returns false for the first sweep (nothing to match against) and on a backend
  // error; Tsum() is the accumulated sweep-to-sweep motion, lastCornerCloud()/lastSurfaceCloud() the clouds the
  // mapping node receives (/laser_cloud_corner_last, /laser_cloud_surf_last), packed {x,y,z,intensity}.
  template <typename Cloud>
  bool process(const Cloud &cornerPointsSharp, const Cloud &cornerPointsLessSharp, const Cloud &surfPointsFlat,
               const Cloud &surfPointsLessFlat) {
    if (!_od || !_fs) return false;
    std::vector<float> sharp, less_sharp, flat, less_flat;
    detail::pack_xyzi(cornerPointsSharp, sharp);
    detail::pack_xyzi(cornerPointsLessSharp, less_sharp);
    detail::pack_xyzi(surfPointsFlat, flat);
    detail::pack_xyzi(surfPointsLessFlat, less_flat);
    if (lslam_fset_upload(_ctx, _fs, sharp.data(), sharp.size() / 4, less_sharp.data(), less_sharp.size() / 4, flat.data(),
                          flat.size() / 4, less_flat.data(), less_flat.size() / 4, 16) < 0)
      return fail();
    return processFeatureSet(_fs);
  }
  // the same on a feature set that is in HBM already
  bool processFeatureSet(lslam_fset *fs) {
    if (!_od) return false;
    size_t n[4];
    if (lslam_fset_counts(fs, n) < 0) return fail();
    _lastCorner.resize(4 * n[1]);
    _lastSurf.resize(4 * n[3]);
    const uint64_t before = _ostats.sweeps;
    const int st = lslam_odom_process(_od, fs, _transform, _Tsum, &_last, &_ostats, _lastCorner.data(), n[1], _lastSurf.data(), n[3]);
    if (st < 0) return fail();
    _matched = _ostats.matched != 0;
    return before != 0;  // the first sweep only initialises (:295-303)
  }
  const float *Tsum() const { return _Tsum; }
  const float *transform() const { return _transform; }
  const std::vector<float> &lastCornerCloud() const { return _lastCorner; }
  const std::vector<float> &lastSurfaceCloud() const { return _lastSurf; }
  const lslam_stats &lastStats() const { return _last; }
  const lslam_odom_stats &nodeStats() const { return _ostats; }
  bool matched() const { return _matched; }  // false: the last clouds were too small to match against (:337)
  const std::string &lastError() const { return _err; }

private:
  bool fail() {
    _err = lslam_last_error();
    return false;
  }
  lslam_ctx *_ctx;
  lslam_odom *_od;
  lslam_fset *_fs;
  bool _matched;
  float _transform[6];  // _transform: sweep-to-sweep motion, kept as the next initial guess
  float _Tsum[16];      // _Tsum
  std::vector<float> _lastCorner, _lastSurf;
  lslam_stats _last;
  lslam_odom_stats _ostats;
  std::string _err;
};

namespace detail {
// LaserMatcher (LaserMatcher.cpp:80-116, 289-347): the per-sweep steps the mapping nodes share -- transformMerge (odometry
// prior), VoxelGrid of the frame's feature clouds, scanMatchScan with thresholds 0.1 / 0.1 and the score gate off (its return
// value is ignored, :327-331), transformUpdate.  A node puts its map container's two steps between them.
class LaserMatcherSteps {
public:
  const float *lidarMapped() const { return _lidarMappedNew; }
  const lslam_stats &lastStats() const { return _last; }
  const std::string &lastError() const { return _err; }

protected:
  LaserMatcherSteps(lslam_ctx *ctx, float filterCorner, float filterSurf) : _ctx(ctx), _filterCorner(filterCorner), _filterSurf(filterSurf) {
    lslam_default_opts(&_opts);
    _opts.delta_t_abort = 0.1f;  // _scan_match.setConvergeThreshold(0.1, 0.1), LaserMatcher.cpp:94
    _opts.delta_r_abort = 0.1f;
    _opts.use_score = 0;         // setUseCore(false), :95
    identity4(_lidarOdomLast);
    identity4(_lidarMappedLast);
    identity4(_lidarMappedNew);
    std::memset(&_last, 0, sizeof(_last));
  }
  // transformMerge, :333-340, and prepareFeatureFrame, :289-301
  bool mergeAndPrepareFrame(const std::vector<float> &cornerLast, const std::vector<float> &surfLast, const float lidarOdomNew[16]) {
    lslam_transform_associate(_lidarOdomLast, lidarOdomNew, _lidarMappedLast, _lidarMappedNew);
    if (_filterCorner == _filterSurf) {  // the reference's defaults: both clouds in one pass (lslam_voxel_grid2: same bits)
      _cornerDS.resize(cornerLast.size() + 4);
      _surfDS.resize(surfLast.size() + 4);
      size_t nc2 = 0, ns2 = 0;
      if (lslam_voxel_grid2(_ctx, cornerLast.data(), cornerLast.size() / 4, surfLast.data(), surfLast.size() / 4, 16, _filterCorner,
                            _cornerDS.data(), cornerLast.size() / 4, &nc2, _surfDS.data(), surfLast.size() / 4, &ns2) < 0)
        return fail();
      _cornerDS.resize(4 * nc2);
      _surfDS.resize(4 * ns2);
    } else if (!downsize(cornerLast, _filterCorner, _cornerDS) || !downsize(surfLast, _filterSurf, _surfDS)) {
      return fail();
    }
    return true;
  }
  // optimizeTransform, :327-331, against the context's map (nc / ns: the sizes of the surround that became it), and
  // transformUpdate, :342-347
  bool optimizeAndUpdate(size_t nc, size_t ns, const float lidarOdomNew[16]) {
    if (nc || ns) {
      float pose[6];
      lslam_isometry_to_pose(_lidarMappedNew, pose);
      const int st = lslam_scanmatch_scan(_ctx, _cornerDS.data(), _cornerDS.size() / 4, _surfDS.data(), _surfDS.size() / 4, 16, pose,
                                          &_opts, &_last);
      if (st < 0) return fail();
      if (st != LSLAM_TOO_FEW_REF) lslam_pose_to_isometry(pose, _lidarMappedNew);  // ScanMatch.cpp:57-61 leaves the pose untouched
    }
    std::memcpy(_lidarMappedLast, _lidarMappedNew, sizeof(_lidarMappedNew));
    std::memcpy(_lidarOdomLast, lidarOdomNew, sizeof(_lidarOdomLast));
    return true;
  }
  bool downsize(const std::vector<float> &in, float leaf, std::vector<float> &out) {
    out.resize(in.size() + 4);
    size_t n = 0;
    const int st = lslam_voxel_grid(_ctx, in.data(), in.size() / 4, 16, leaf, out.data(), in.size() / 4, &n);
    out.resize(4 * n);
    return st >= 0;
  }
  bool fail() {
    _err = lslam_last_error();
    return false;
  }
  lslam_ctx *_ctx;
  float _filterCorner, _filterSurf;
  lslam_opts _opts;
  float _lidarOdomLast[16], _lidarMappedLast[16], _lidarMappedNew[16];
  std::vector<float> _cornerDS, _surfDS;
  lslam_stats _last;
  std::string _err;
};
}  // namespace detail

// LaserMapping (BASELINE configs[1]): LaserMatcher's steps over the cube grid -- FeatureMap::update + surround -> the context's
// map (device) before the match, addFeatureCloud after it.
class LaserMapping : public detail::LaserMatcherSteps {
public:
  // LaserMatcher.cpp:80-116 defaults (filter 1.0 / 1.0, map filters 1.0 / 1.0 / 2.0, 121 x 121 x 11 cubes)
  explicit LaserMapping(lslam_ctx *ctx, int cubeX = 121, int cubeY = 121, int cubeZ = 11, float filterCorner = 1.0f,
                        float filterSurf = 1.0f, float mapFilterCorner = 1.0f, float mapFilterSurf = 1.0f, float mapFilter = 2.0f)
      : detail::LaserMatcherSteps(ctx, filterCorner, filterSurf), _fm(nullptr) {
    if (lslam_fmap_create(ctx, cubeX, cubeY, cubeZ, &_fm) != LSLAM_OK) {
      _fm = nullptr;
      _err = lslam_last_error();
    } else {
      lslam_fmap_setup_filter_size(_fm, mapFilterCorner, mapFilterSurf, mapFilter);
      // the per-frame surround map is searched through its cell grids; its kd-trees are built only if a frame needs them
      // (lslam_map_defer_trees) -- same poses either way
      lslam_map_defer_trees(ctx, 1);
    }
  }
  ~LaserMapping() { lslam_fmap_destroy(_fm); }
  LaserMapping(const LaserMapping &) = delete;
  LaserMapping &operator=(const LaserMapping &) = delete;

  // cornerLast / surfLast: the odometry node's last clouds, packed {x,y,z,intensity} (LaserOdometry::lastCornerCloud());
  // lidarOdomNew: its _Tsum (row-major 4x4).  Returns false on a backend error; lidarMapped() is the sweep's pose in the map.
  bool process(const std::vector<float> &cornerLast, const std::vector<float> &surfLast, const float lidarOdomNew[16]) {
    if (!_fm) return false;
    if (!mergeAndPrepareFrame(cornerLast, surfLast, lidarOdomNew)) return false;
    // prepareFeatureSurround, :303-325
    const float pos[3] = {_lidarMappedNew[3], _lidarMappedNew[7], _lidarMappedNew[11]};
    if (lslam_fmap_update(_fm, pos) < 0) return fail();
    size_t nc = 0, ns = 0;
    if (lslam_fmap_surround_to_map_counts(_fm, &nc, &ns) < 0) return fail();  // the surround becomes the context's map
    if (!optimizeAndUpdate(nc, ns, lidarOdomNew)) return false;
    // featureMapUpdate, :349-354.  -DLSLAM_MAPPING_DEFER_ADD: enqueued, not waited for (lslam_fmap_add_feature_cloud_begin) -- the
    // map's rebuild then runs while the node takes up its next sweep and the next call on the map waits and commits first.  It pays
    // where the host idles between two sweeps (the Python mirror: 0.91 -> 0.82 ms per frame); with three nodes on three threads
    // it does not (the device is the limit there) and the chain fell into its slow mode more often (tools/node_threads_ab.py)
#ifdef LSLAM_MAPPING_DEFER_ADD
    if (lslam_fmap_add_feature_cloud_begin(_fm, _cornerDS.data(), _cornerDS.size() / 4, _surfDS.data(), _surfDS.size() / 4, 16,
                                           _lidarMappedNew) < 0)
      return fail();
#else
    if (lslam_fmap_add_feature_cloud(_fm, _cornerDS.data(), _cornerDS.size() / 4, _surfDS.data(), _surfDS.size() / 4, 16, _lidarMappedNew) < 0)
      return fail();
#endif
    return true;
  }
  lslam_fmap *featureMap() { return _fm; }

private:
  lslam_fmap *_fm;
};

// LocalFeatureMap<PointT> (io_module/LocalFeatureMap.h) over lslam_lmap_*: the frames of the last `queue distance` metres of
// path in HBM.  Clouds are packed {x, y, z, intensity} floats; tf is a row-major 4x4.
class LocalFeatureMap {
public:
  explicit LocalFeatureMap(lslam_ctx *ctx, size_t maxPointsPerType = 0, int maxFrames = 0, int flags = 0) : _lm(nullptr) {
    if (lslam_lmap_create(ctx, maxPointsPerType, maxFrames, flags, &_lm) != LSLAM_OK) {
      _lm = nullptr;
      _err = lslam_last_error();
    }
  }
  ~LocalFeatureMap() { lslam_lmap_destroy(_lm); }
  LocalFeatureMap(const LocalFeatureMap &) = delete;
  LocalFeatureMap &operator=(const LocalFeatureMap &) = delete;
  bool valid() const { return _lm != nullptr; }
  bool setupQueueDistance(double metres) { return check(lslam_lmap_setup_queue_distance(_lm, metres)); }
  // (not in the reference, whose leaves are fixed at 0.2 / 0.4; refused once a frame has been added)
  bool setupFilterSize(float corner, float surf) { return check(lslam_lmap_setup_filter_size(_lm, corner, surf)); }
  // LocalFeatureMap.h:62-69 behind LaserMappingLocal.cpp:68-83: the clouds are transformed by tf, pushed; clean() runs
  bool addDataFrame(const std::vector<float> &cornerDS, const std::vector<float> &surfDS, const float tf[16]) {
    return check(lslam_lmap_add_data_frame(_lm, cornerDS.data(), cornerDS.size() / 4, surfDS.data(), surfDS.size() / 4, 16, tf));
  }
  // :84-99, to the host
  bool getSurroundFeature(std::vector<float> &surroundCorner, std::vector<float> &surroundSurf) {
    size_t nc = 0, ns = 0;
    if (!check(lslam_lmap_get_surround(_lm, nullptr, 0, &nc, nullptr, 0, &ns))) return false;
    surroundCorner.resize(4 * nc + 4);
    surroundSurf.resize(4 * ns + 4);
    if (!check(lslam_lmap_get_surround(_lm, surroundCorner.data(), nc, &nc, surroundSurf.data(), ns, &ns))) return false;
    surroundCorner.resize(4 * nc);
    surroundSurf.resize(4 * ns);
    return true;
  }
  // ... or as the scan matcher's map, without leaving the device
  bool surroundToMap(size_t *nCorner, size_t *nSurf) { return check(lslam_lmap_surround_to_map_counts(_lm, nCorner, nSurf)); }
  // :70-82 -- nothing to do: addDataFrame cleans, as the reference's does (n frames behind the threshold -> n + 1 erased)
  void clean() {}
  bool clear() { return check(lslam_lmap_clear(_lm)); }
  const std::string &lastError() const { return _err; }
  lslam_lmap *handle() { return _lm; }

private:
  bool check(int rc) {
    if (rc < 0) _err = lslam_last_error();
    return rc >= 0;
  }
  lslam_lmap *_lm;
  std::string _err;
};

// LaserMappingLocal (odometry/LaserMappingLocal.cpp:39-83): LaserMatcher's steps over the sliding window -- its filtered
// surround becomes the context's map before the match (prepareFeatureSurround, :61-66), the sweep's downsampled clouds are
// added at the new map pose after it (featureMapUpdate, :68-83).
class LaserMappingLocal : public detail::LaserMatcherSteps {
public:
  explicit LaserMappingLocal(lslam_ctx *ctx, float filterCorner = 1.0f, float filterSurf = 1.0f, double queueDistance = 30.0,
                             size_t maxPointsPerType = 0, int maxFrames = 0, int flags = 0)
      : detail::LaserMatcherSteps(ctx, filterCorner, filterSurf), _map(ctx, maxPointsPerType, maxFrames, flags) {
    if (!_map.valid()) {
      _err = _map.lastError();
    } else {
      _map.setupQueueDistance(queueDistance);
      lslam_map_defer_trees(ctx, 1);  // (as LaserMapping: the per-sweep map is searched through its cell grids)
    }
  }
  bool process(const std::vector<float> &cornerLast, const std::vector<float> &surfLast, const float lidarOdomNew[16]) {
    if (!_map.valid()) return false;
    if (!mergeAndPrepareFrame(cornerLast, surfLast, lidarOdomNew)) return false;
    size_t nc = 0, ns = 0;
    if (!_map.surroundToMap(&nc, &ns)) return failMap();
    if (!optimizeAndUpdate(nc, ns, lidarOdomNew)) return false;
    if (!_map.addDataFrame(_cornerDS, _surfDS, _lidarMappedNew)) return failMap();
    return true;
  }
  LocalFeatureMap &featureMap() { return _map; }

private:
  bool failMap() {
    _err = _map.lastError();
    return false;
  }
  LocalFeatureMap _map;
};

// LaserLocalization (odometry/LaserLocalization.cpp:140-188 over util/FeatureMap.h): the second operating mode -- a map built
// once and saved with saveCloudToFiles is loaded at init, every cube's kd-tree is built once, and each sweep is matched against
// it on the device behind one host wait (lslam_loc_*, include/lslam_c.h).  loadMap is _feature_map->loadCloudFromFiles,
// handleInitialPose the pose initialPoseHandler ends with (its ROS sign conventions are the host program's), process the
// sweep: transformMerge, prepareFeatureFrame, optimizeTransform, transformUpdate with its reset-after-match rule, the velocity.
// The UKF (imu_que) is the host program's: lidarMapped(), velocity() and the stamp are what imu_que.correct is handed.
class LaserLocalization {
public:
  explicit LaserLocalization(lslam_ctx *ctx, int cubeX = 121, int cubeY = 121, int cubeZ = 11, float filterCorner = 1.0f,
                             float filterSurf = 1.0f, float mapFilterCorner = 1.0f, float mapFilterSurf = 1.0f)
      : _loc(nullptr), _flags(0), _hasVelocity(false), _dynamic(false), _relocStatus(0) {
    detail::identity4(_lidarMappedNew);
    std::memset(_velocity, 0, sizeof(_velocity));
    std::memset(&_last, 0, sizeof(_last));
    std::memset(&_reloc, 0, sizeof(_reloc));
    if (lslam_abi_version() != LSLAM_ABI_VERSION || lslam_sizeof_opts() != sizeof(lslam_opts) || lslam_sizeof_stats() != sizeof(lslam_stats)) {
      _err = "liblslam_hip was built from another include/lslam_c.h than this program (ABI version / struct sizes differ)";
      return;
    }
    if (lslam_loc_create(ctx, cubeX, cubeY, cubeZ, &_loc) != LSLAM_OK) {
      _loc = nullptr;
      _err = lslam_last_error();
      return;
    }
    lslam_loc_setup_scan_filter_size(_loc, filterCorner, filterSurf);
    lslam_loc_setup_map_filter_size(_loc, mapFilterCorner, mapFilterSurf);
  }
  ~LaserLocalization() { lslam_loc_destroy(_loc); }
  LaserLocalization(const LaserLocalization &) = delete;
  LaserLocalization &operator=(const LaserLocalization &) = delete;
  bool ok() const { return _loc != nullptr; }
  bool setupWorldOrigin(int ox, int oy, int oz) { return check(lslam_loc_setup_world_origin(_loc, ox, oy, oz)); }
  bool setupWorldCubeSize(float size) { return check(lslam_loc_setup_world_cube_size(_loc, size)); }
  bool setupLidarValidDistance(float dist) { return check(lslam_loc_setup_lidar_valid_distance(_loc, dist)); }
  // init(): _feature_map->loadCloudFromFiles(map_file_path)
  bool loadMap(const std::string &directory) { return check(lslam_loc_load(_loc, directory.c_str())); }
  // ... or the map a mapping node of the same context has just built
  bool adoptMap(lslam_fmap *fm) { return check(lslam_loc_set_map_from_fmap(_loc, fm)); }
  // LaserMatcher's dynamicMode branch (LaserMatcher.cpp:100-104): the cubes become a window over the files of a directory
  // (index2.txt plus <count>.pcd) that follows the sensor; setupFilesDirectory reads the index and enters the mode
  bool setDynamicMode(bool on) {
    _dynamic = on;
    return true;
  }
  bool setupFilesDirectory(const std::string &directory) {
    if (!_dynamic) {
      _err = "setupFilesDirectory: the dynamic mode is off (setDynamicMode)";
      return false;
    }
    return check(lslam_pmap_open(_loc, directory.c_str()));
  }
  bool setupPagedCapacity(size_t maxPointsPerType) { return check(lslam_pmap_setup_capacity(_loc, maxPointsPerType)); }
  // between sweeps, with the host's predicted position: the cubes the next window would need are read ahead
  bool stage(const float pos[3]) { return check(lslam_pmap_stage(_loc, pos)); }
  bool windowInfo(lslam_loc_window_stats *out) { return check(lslam_pmap_window_info(_loc, out)); }
  bool handleInitialPose(const float T[16]) { return check(lslam_loc_set_initial_pose(_loc, T)); }
  // the map from host clouds (packed {x, y, z, intensity}); filter: every cube through the map filters, as loadMap does
  bool setMap(const std::vector<float> &corner, const std::vector<float> &surf, bool filter) {
    return check(lslam_loc_set_map(_loc, corner.data(), corner.size() / 4, surf.data(), surf.size() / 4, 16, filter ? 1 : 0));
  }
  // Global re-localisation (lslam_reloc_*, include/lslam_c.h): the pose of one sweep in the loaded map without an initial pose,
  // where the reference waits for a click in RViz or a GPS fix.  rotXyz: Twist angle triplets, posXyz: positions, every pair is
  // a hypothesis; opts may be null (the defaults).  true: accepted -- with opts->apply the node then holds the pose as after
  // handleInitialPose(relocResult().T).  false: relocStatus() says why (LSLAM_NOT_CONVERGED, LSLAM_TOO_FEW_MATCHES: the result is
  // filled in all the same; negative: a backend error, lastError()).
  bool relocalize(const std::vector<float> &corner, const std::vector<float> &surf, const std::vector<float> &rotXyz,
                  const std::vector<float> &posXyz, const lslam_reloc_opts *opts = nullptr) {
    if (!_loc) return false;
    _relocStatus = lslam_reloc_relocalize(_loc, corner.data(), corner.size() / 4, surf.data(), surf.size() / 4, 16, rotXyz.data(),
                                          rotXyz.size() / 3, posXyz.data(), posXyz.size() / 3, opts, &_reloc);
    if (_relocStatus < 0) _err = lslam_last_error();
    return _relocStatus == LSLAM_OK && _reloc.accepted != 0;
  }
  const lslam_reloc_result &relocResult() const { return _reloc; }
  int relocStatus() const { return _relocStatus; }
  // cornerLast / surfLast: packed {x, y, z, intensity}; lidarOdomNew: the odometry node's _Tsum.  false: a backend error, or the
  // sweep was dropped (dropped() says which); the match's own outcome (lastStats().status) never makes it false, as the
  // reference ignores scanMatchScan's result.
  bool process(const std::vector<float> &cornerLast, const std::vector<float> &surfLast, const float lidarOdomNew[16], int64_t stampNs) {
    if (!_loc) return false;
    return finish(lslam_loc_process(_loc, cornerLast.data(), cornerLast.size() / 4, surfLast.data(), surfLast.size() / 4, 16, lidarOdomNew,
                                    stampNs, _lidarMappedNew, _velocity, &_flags, &_last));
  }
  // the same for clouds in the context's device memory (lslam_odom_last_view)
  bool processDevice(const void *dCornerLast, size_t nCorner, const void *dSurfLast, size_t nSurf, const float lidarOdomNew[16],
                     int64_t stampNs) {
    if (!_loc) return false;
    return finish(lslam_loc_process_device(_loc, dCornerLast, nCorner, dSurfLast, nSurf, lidarOdomNew, stampNs, _lidarMappedNew, _velocity,
                                           &_flags, &_last));
  }
  const float *lidarMapped() const { return _lidarMappedNew; }
  const float *velocity() const { return _velocity; }
  bool hasVelocity() const { return _hasVelocity; }
  bool dropped() const { return (_flags & LSLAM_LOC_DROPPED) != 0; }
  int flags() const { return _flags; }
  const lslam_stats &lastStats() const { return _last; }
  const std::string &lastError() const { return _err; }
  lslam_loc *handle() { return _loc; }

private:
  bool check(int rc) {
    if (rc < 0) _err = lslam_last_error();
    return rc >= 0;
  }
  bool finish(int rc) {
    if (rc < 0) {
      _err = lslam_last_error();
      return false;
    }
    _hasVelocity = (_flags & LSLAM_LOC_HAS_VELOCITY) != 0;
    return (_flags & LSLAM_LOC_DROPPED) == 0;
  }
  lslam_loc *_loc;
  float _lidarMappedNew[16], _velocity[3];
  int32_t _flags;
  bool _hasVelocity, _dynamic;
  lslam_stats _last;
  lslam_reloc_result _reloc;
  int _relocStatus;
  std::string _err;
};

}  // namespace lidar_slam
