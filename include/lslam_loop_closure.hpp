// lslam_loop_closure.hpp -- header-only C++ mirrors of the loop-closure front end and the pose-graph node's
// bookkeeping over the C ABI (lslam_c.h):
//
//   pose_graph::LoopDetector      /root/reference/L_SLAM/src/pose_graph/loop_detector.hpp:50-280
//                                 (trajectory radius search + candidate gating on the host, coarse alignment =
//                                 lslam_icp_align, fine alignment = ScanMatch::scanMatchLocal on the device)
//   pose_graph::KeyframeUpdater   pose_graph/keyframe_updater.hpp:10-60
//   pose_graph::Graph             pose_graph/graph.cpp:230-385 (keyframe queue, odometry / loop edges with the
//                                 reference's information matrices, optimise when a loop was found, odom -> graph)
//
//   KeyframeStore                 RAII wrapper of lslam_kfs_*: the keyframes' clouds resident in HBM.  A Graph made with
//                                 resident = true owns one: add_frame uploads a keyframe's clouds once, LoopDetector and
//                                 getFinalFeatureMap then name them by id and no cloud crosses PCIe again.  Same ABI
//                                 kernels in the same order as the host-cloud path: same results.
//
// Not in the reference: KeyframeStore::sc_* (lslam_sc_*: scan-context descriptors over the store),
// LoopDetector::detect_appearance (loop candidates from what a keyframe looks like, verified by lslam_kfs_loop_match) and
// Graph's appearance_loops switch (off by default: nothing changes without it).
//
// ROS topics, threads and tf are the host program's.  Poses are row-major 4x4 doubles (Mat4d); clouds are packed
// {x, y, z, intensity} floats.  Nothing here throws; backend failures end up in lastError() and a false / empty
// result, the way the reference's nodes report a failed match.
//
// Three things of the reference are restated as they are, not as they were probably meant (the Python mirror
// the-cooper-mapper_amd/loop_closure.py documents the evidence): the radius handed to radiusSearch is compared
// with SQUARED distances (nanoflann_pcl.h:166-186), KdTreeFLANN::radiusSearch returns ONE result -- the nearest
// (nanoflann_pcl.h:173) --, and the trajectory is flattened with y = 0 (loop_detector.hpp:98,120).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "lslam_c.h"

namespace pose_graph {

struct Mat4d {
  double m[16];
  Mat4d() { std::memset(m, 0, sizeof(m)); m[0] = m[5] = m[10] = m[15] = 1.0; }
  double &operator()(int r, int c) { return m[r * 4 + c]; }
  double operator()(int r, int c) const { return m[r * 4 + c]; }
};
inline Mat4d operator*(const Mat4d &A, const Mat4d &B) {
  Mat4d C;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      double s = 0;
      for (int k = 0; k < 4; ++k) s += A(r, k) * B(k, c);
      C(r, c) = s;
    }
  return C;
}
inline Mat4d inverse(const Mat4d &T) {  // Eigen::Isometry3d::inverse(): [R^T | -R^T t]
  Mat4d I;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) I(r, c) = T(c, r);
    I(r, 3) = -(T(0, r) * T(0, 3) + T(1, r) * T(1, 3) + T(2, r) * T(2, 3));
  }
  return I;
}
inline void to_float16(const Mat4d &T, float out[16]) { for (int i = 0; i < 16; ++i) out[i] = (float)T.m[i]; }
inline Mat4d from_float16(const float in[16]) { Mat4d T; for (int i = 0; i < 16; ++i) T.m[i] = in[i]; return T; }

// 4x4 <-> g2o's {t, q_xyzw} (Eigen::Quaterniond(R))
inline void mat_to_pose7(const Mat4d &T, double p[7]) {
  p[0] = T(0, 3); p[1] = T(1, 3); p[2] = T(2, 3);
  const double tr = T(0, 0) + T(1, 1) + T(2, 2);
  double q[4];
  if (tr > 0) {
    double s = std::sqrt(tr + 1.0);
    q[3] = 0.5 * s;
    s = 0.5 / s;
    q[0] = (T(2, 1) - T(1, 2)) * s; q[1] = (T(0, 2) - T(2, 0)) * s; q[2] = (T(1, 0) - T(0, 1)) * s;
  } else {
    int i = 0;
    if (T(1, 1) > T(0, 0)) i = 1;
    if (T(2, 2) > T(i, i)) i = 2;
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    double s = std::sqrt(T(i, i) - T(j, j) - T(k, k) + 1.0);
    q[i] = 0.5 * s;
    s = 0.5 / s;
    q[3] = (T(k, j) - T(j, k)) * s;
    q[j] = (T(j, i) + T(i, j)) * s;
    q[k] = (T(k, i) + T(i, k)) * s;
  }
  p[3] = q[0]; p[4] = q[1]; p[5] = q[2]; p[6] = q[3];
}
inline Mat4d pose7_to_mat(const double p[7]) {
  const double x = p[3], y = p[4], z = p[5], w = p[6];
  Mat4d T;
  T(0, 0) = 1 - 2 * (y * y + z * z); T(0, 1) = 2 * (x * y - z * w);     T(0, 2) = 2 * (x * z + y * w);
  T(1, 0) = 2 * (x * y + z * w);     T(1, 1) = 1 - 2 * (x * x + z * z); T(1, 2) = 2 * (y * z - x * w);
  T(2, 0) = 2 * (x * z - y * w);     T(2, 1) = 2 * (y * z + x * w);     T(2, 2) = 1 - 2 * (x * x + y * y);
  T(0, 3) = p[0]; T(1, 3) = p[1]; T(2, 3) = p[2];
  return T;
}

// The occupancy grid as the stem.pgm / stem.yaml pair map_server loads (byte for byte what the Python occupancy.save_map writes):
// binary P5, row 0 the largest b, trinary as map_saver writes it -- value >= 65 -> 0, 0 <= value <= 19 -> 254, anything else,
// unknown included -> 205.  values: width * height, row-major with index j * width + i (KeyframeStore::occValues).
inline bool saveMap(const std::string &stem, const std::vector<int8_t> &values, const lslam_occ_params &params) {
  const size_t w = (size_t)params.width, h = (size_t)params.height;
  if (params.width < 1 || params.height < 1 || values.size() != w * h) return false;
  const std::string pgm = stem + ".pgm", yaml = stem + ".yaml";
  const size_t slash = pgm.find_last_of('/');
  const std::string base = slash == std::string::npos ? pgm : pgm.substr(slash + 1);
  FILE *f = std::fopen(pgm.c_str(), "wb");
  if (!f) return false;
  std::fprintf(f, "P5\n# CREATOR: lslam occupancy %.17g m/pix\n%zu %zu\n255\n", (double)params.resolution, w, h);
  std::vector<unsigned char> row(w);
  for (size_t r = 0; r < h; ++r) {
    const int8_t *v = &values[(h - 1 - r) * w];
    for (size_t i = 0; i < w; ++i) row[i] = v[i] >= 65 ? 0 : (v[i] >= 0 && v[i] <= 19 ? 254 : 205);
    std::fwrite(row.data(), 1, w, f);
  }
  if (std::fclose(f) != 0) return false;
  f = std::fopen(yaml.c_str(), "w");
  if (!f) return false;
  std::fprintf(f, "# map axes in the graph frame: %s; origin is the corner of cell (0, 0)\n",
               params.up_axis == 1 ? "a = +z, b = +x (y up)" : "a = +x, b = +y (z up)");
  std::fprintf(f, "image: %s\nresolution: %.17g\norigin: [%.17g, %.17g, 0.0]\n", base.c_str(), (double)params.resolution, params.origin[0],
               params.origin[1]);
  std::fprintf(f, "negate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n");
  return std::fclose(f) == 0;
}

// The keyframes' clouds in device memory (lslam_kfs_*).  Not copyable; the store may outlive its ctx (every call is then
// refused), the destructor frees it either way.
class KeyframeStore {
public:
  explicit KeyframeStore(lslam_ctx *ctx, size_t max_points_per_type = 0, int32_t max_keyframes = 0, size_t slab_points = 0) {
    if (lslam_kfs_create(ctx, max_points_per_type, max_keyframes, slab_points, &_h) != LSLAM_OK) _err = lslam_last_error();
  }
  ~KeyframeStore() { lslam_kfs_destroy(_h); }
  KeyframeStore(const KeyframeStore &) = delete;
  KeyframeStore &operator=(const KeyframeStore &) = delete;
  bool ok() const { return _h != nullptr; }
  lslam_kfs *handle() const { return _h; }
  // -> the keyframe's id, -1 when the add was refused (lastError says why)
  int add(const std::vector<float> &corner, const std::vector<float> &surf) {
    int32_t id = -1;
    if (lslam_kfs_add(_h, corner.data(), corner.size() / 4, surf.data(), surf.size() / 4, 16, &id) != LSLAM_OK) {
      _err = lslam_last_error();
      return -1;
    }
    return id;
  }
  bool get(int id, int which, std::vector<float> &out) {
    size_t n = 0;
    if (lslam_kfs_get(_h, id, which, nullptr, 0, &n) != LSLAM_OK) { _err = lslam_last_error(); return false; }
    out.resize(4 * n);
    if (lslam_kfs_get(_h, id, which, out.data(), n, &n) != LSLAM_OK) { _err = lslam_last_error(); return false; }
    return true;
  }
  bool info(lslam_kfs_stats &st) {
    if (lslam_kfs_info(_h, &st) == LSLAM_OK) return true;
    _err = lslam_last_error();
    return false;
  }
  bool clear() {
    if (lslam_kfs_clear(_h) == LSLAM_OK) return true;
    _err = lslam_last_error();
    return false;
  }
  // The floor of each named keyframe's SURFACE cloud, where it lies (lslam_floor_detect_keyframes: every keyframe through each
  // stage in one launch, no cloud moved); params == nullptr: the defaults.  results[k] belongs to ids[k].
  bool floorDetect(const std::vector<int32_t> &ids, const lslam_floor_params *params, std::vector<lslam_floor_result> &results) {
    results.assign(ids.size(), lslam_floor_result());
    if (lslam_floor_detect_keyframes(_h, (int32_t)ids.size(), ids.data(), params, results.data()) == LSLAM_OK) return true;
    _err = lslam_last_error();
    return false;
  }
  // ---- loop candidates by appearance: scan context (lslam_sc_*) ----
  // params == nullptr: the defaults.  Other parameters than those in force drop the descriptors held.
  bool sc_setup(const lslam_sc_params *params = nullptr) {
    if (lslam_sc_setup(_h, params) == LSLAM_OK) return true;
    _err = lslam_last_error();
    return false;
  }
  bool sc_info(lslam_sc_stats &st) {
    if (lslam_sc_info(_h, &st) == LSLAM_OK) return true;
    _err = lslam_last_error();
    return false;
  }
  // keyframe id's descriptor, n_ring x n_sector row-major (parity tap)
  bool sc_descriptor(int id, std::vector<float> &out) {
    lslam_sc_stats st;
    if (!sc_info(st)) return false;
    out.assign((size_t)std::max(st.params.n_ring, 1) * (size_t)std::max(st.params.n_sector, 1), 0.0f);
    if (lslam_sc_descriptor(_h, id, out.data()) == LSLAM_OK) return true;
    _err = lslam_last_error();
    return false;
  }
  // One list per query, best first (distance, then id), top_k entries apart in the outputs; n_out[q] of them are valid.
  // max_cand_id == nullptr: query_ids[q] - 1.
  bool sc_query(const std::vector<int32_t> &query_ids, const std::vector<int32_t> *max_cand_id, int top_k, std::vector<int32_t> &ids,
                std::vector<int32_t> &shifts, std::vector<float> &dists, std::vector<int32_t> &n_out) {
    const size_t nq = query_ids.size(), k = (size_t)std::max(top_k, 1);
    ids.assign(nq * k, -1);
    shifts.assign(nq * k, 0);
    dists.assign(nq * k, 1.0f);
    n_out.assign(nq, 0);
    if (max_cand_id && max_cand_id->size() != nq) { _err = "sc_query: one max_cand_id per query"; return false; }
    if (lslam_sc_query(_h, (int32_t)nq, query_ids.data(), max_cand_id ? max_cand_id->data() : nullptr, top_k, ids.data(),
                           shifts.data(), dists.data(), n_out.data()) == LSLAM_OK)
      return true;
    _err = lslam_last_error();
    return false;
  }
  // the query kernel's distance and shift of query_id against every keyframe (parity tap)
  bool sc_distances(int query_id, std::vector<float> &dists, std::vector<int32_t> &shifts) {
    lslam_kfs_stats st;
    if (!info(st)) return false;
    dists.assign((size_t)st.n_keyframes, 0.0f);
    shifts.assign((size_t)st.n_keyframes, 0);
    if (lslam_sc_distances(_h, query_id, dists.data(), shifts.data()) == LSLAM_OK) return true;
    _err = lslam_last_error();
    return false;
  }
  // ---- visibility votes: the final map without moving objects (lslam_vis_*) ----
  // params == nullptr: the defaults.  Other parameters than those in force drop the range images held.
  bool vis_setup(const lslam_vis_params *params = nullptr) {
    if (lslam_vis_setup(_h, params) == LSLAM_OK) return true;
    _err = lslam_last_error();
    return false;
  }
  bool vis_info(lslam_vis_stats &st) {
    if (lslam_vis_info(_h, &st) == LSLAM_OK) return true;
    _err = lslam_last_error();
    return false;
  }
  // keyframe id's range image, n_row x n_col row-major, +inf where nothing was seen (parity tap)
  bool vis_range_image(int id, std::vector<float> &out) {
    lslam_vis_stats st;
    if (!vis_info(st)) return false;
    out.assign((size_t)std::max(st.params.n_row, 1) * (size_t)std::max(st.params.n_col, 1), 0.0f);
    if (lslam_vis_range_image(_h, id, out.data()) == LSLAM_OK) return true;
    _err = lslam_last_error();
    return false;
  }
  // The votes of keyframes ids[k] at poses[16 k ..] (row-major 4x4 float, graph <- sensor) on host points {x, y, z, -}:
  // votes[i] = n_free | n_hit << 16.
  bool vis_votes(const std::vector<int32_t> &ids, const std::vector<float> &poses, const std::vector<float> &points,
                 std::vector<uint32_t> &votes) {
    votes.assign(points.size() / 4, 0u);
    if (poses.size() != 16 * ids.size()) { _err = "vis_votes: one 4x4 pose per id"; return false; }
    if (lslam_vis_votes(_h, (int32_t)ids.size(), ids.data(), poses.data(), points.data(), points.size() / 4, 16, votes.data()) == LSLAM_OK)
      return true;
    _err = lslam_last_error();
    return false;
  }
  // n points in the ctx's device memory, packed {x, y, z, -}: the ones that are not dynamic, in input order, into d_out (room
  // for n points); -> how many, -1 when refused.
  long vis_filter(const std::vector<int32_t> &ids, const std::vector<float> &poses, const float *d_xyzi, size_t n, float *d_out) {
    size_t kept = 0;
    if (poses.size() != 16 * ids.size()) { _err = "vis_filter: one 4x4 pose per id"; return -1; }
    if (lslam_vis_filter_device(_h, (int32_t)ids.size(), ids.data(), poses.data(), d_xyzi, n, d_out, &kept) == LSLAM_OK) return (long)kept;
    _err = lslam_last_error();
    return -1;
  }
  // lslam_kfs_add_to_fmap with the filter in front; removed[0 / 1]: the corner / surf points left out
  bool vis_add_to_fmap(int id, lslam_fmap *fm, const float T[16], const std::vector<int32_t> &ids, const std::vector<float> &poses,
                       size_t removed[2]) {
    if (poses.size() != 16 * ids.size()) { _err = "vis_add_to_fmap: one 4x4 pose per id"; return false; }
    if (lslam_vis_add_to_fmap(_h, id, fm, T, (int32_t)ids.size(), ids.data(), poses.data(), removed) == LSLAM_OK) return true;
    _err = lslam_last_error();
    return false;
  }
  // ---- 2D occupancy grid: ray-cast votes of the keyframes (lslam_occ_*) ----
  // width and height have no default: set them, or let occFitBounds.  Other parameters than those in force clear the grid.
  bool occSetup(const lslam_occ_params &params) {
    if (lslam_occ_setup(_h, &params) == LSLAM_OK) return true;
    _err = lslam_last_error();
    return false;
  }
  bool occInfo(lslam_occ_stats &st) {
    if (lslam_occ_info(_h, &st) == LSLAM_OK) return true;
    _err = lslam_last_error();
    return false;
  }
  bool occClear() {
    if (lslam_occ_clear(_h) == LSLAM_OK) return true;
    _err = lslam_last_error();
    return false;
  }
  // origin, width and height of `params` fitted to the poses' positions +- max_range (host only)
  bool occFitBounds(const std::vector<float> &poses, lslam_occ_params &params) {
    if (lslam_occ_fit_bounds((int32_t)(poses.size() / 16), poses.data(), &params) == LSLAM_OK) return true;
    _err = lslam_last_error();
    return false;
  }
  // The votes of keyframes ids[k] at poses[16 k ..] (row-major 4x4 float, graph <- sensor).  planes: empty (every keyframe uses
  // the fallback plane) or four doubles per id (lslam_floor_result.plane); plane_valid: empty or one flag per id, 0: the fallback.
  bool occIntegrate(const std::vector<int32_t> &ids, const std::vector<float> &poses, const std::vector<double> &planes = std::vector<double>(),
                    const std::vector<int32_t> &plane_valid = std::vector<int32_t>()) {
    if (poses.size() != 16 * ids.size() || (!planes.empty() && planes.size() != 4 * ids.size()) ||
        (!plane_valid.empty() && plane_valid.size() != ids.size())) {
      _err = "occIntegrate: one 4x4 pose per id, and no or one plane and flag per id";
      return false;
    }
    if (lslam_occ_integrate(_h, (int32_t)ids.size(), ids.data(), poses.data(), planes.empty() ? nullptr : planes.data(),
                            plane_valid.empty() || planes.empty() ? nullptr : plane_valid.data()) == LSLAM_OK)
      return true;
    _err = lslam_last_error();
    return false;
  }
  // n_free | n_hit << 16 per cell, row-major with index j * width + i
  bool occCounts(std::vector<uint32_t> &out) {
    lslam_occ_stats st;
    if (!occInfo(st)) return false;
    out.assign((size_t)std::max(st.params.width, 1) * (size_t)std::max(st.params.height, 1), 0u);
    if (lslam_occ_counts(_h, out.data()) == LSLAM_OK) return true;
    _err = lslam_last_error();
    return false;
  }
  // -1 unknown, else 0 .. 100
  bool occValues(std::vector<int8_t> &out) {
    lslam_occ_stats st;
    if (!occInfo(st)) return false;
    out.assign((size_t)std::max(st.params.width, 1) * (size_t)std::max(st.params.height, 1), (int8_t)-1);
    if (lslam_occ_values(_h, out.data()) == LSLAM_OK) return true;
    _err = lslam_last_error();
    return false;
  }
  // ---- map quality (lslam_mapq_keyframes) ----
  // Mean map entropy and mean plane variance of keyframes ids' clouds of one type (which: 0 corner, 1 surf) put together at
  // poses[16 k ..] (row-major 4x4 float, graph <- sensor): the score of a trajectory.  params == nullptr: the defaults.
  bool mapQuality(const std::vector<int32_t> &ids, const std::vector<float> &poses, int which, const lslam_mapq_params *params,
                  lslam_mapq_stats &stats) {
    if (poses.size() != 16 * ids.size()) { _err = "mapQuality: one 4x4 pose per id"; return false; }
    if (lslam_mapq_keyframes(_h, (int32_t)ids.size(), ids.data(), poses.data(), which, params, &stats) == LSLAM_OK) return true;
    _err = lslam_last_error();
    return false;
  }
  const std::string &lastError() const { return _err; }

private:
  lslam_kfs *_h = nullptr;
  std::string _err;
};

// lslam_traj_eval on vectors (map_evaluation/Evaluation.cpp's statistics, and the rigidly aligned ATE): est_xyz / ref_xyz hold
// three doubles per stamp, ref_stamp ascends.  params == nullptr: the defaults (gate 10 m, no alignment).  Host code: no device.
inline bool trajectoryEval(const std::vector<double> &est_stamp, const std::vector<double> &est_xyz, const std::vector<double> &ref_stamp,
                           const std::vector<double> &ref_xyz, const lslam_traj_params *params, lslam_traj_stats &stats) {
  if (est_xyz.size() != 3 * est_stamp.size() || ref_xyz.size() != 3 * ref_stamp.size()) return false;
  return lslam_traj_eval(est_stamp.data(), est_xyz.data(), est_stamp.size(), ref_stamp.data(), ref_xyz.data(), ref_stamp.size(), params,
                         &stats) == LSLAM_OK;
}

// pose_graph/keyframe.h
struct KeyFrame {
  typedef std::shared_ptr<KeyFrame> Ptr;
  Mat4d odom, estimate;          // odometry pose at insertion; node->estimate()
  double accum_distance = 0.0;
  std::vector<float> cornerCloud, surfCloud;  // {x,y,z,intensity} in the keyframe's own frame
  int node = -1;                 // vertex id in the solver
  int frame_id = 0;
  lslam_kfs *store = nullptr;    // the store that holds the clouds on the device (a resident Graph's), and the id there;
  int store_id = -1;             // cornerCloud / surfCloud are then empty unless the graph keeps host copies
  // keyframe.h:40-41's optional fields (boost::optional there): a projected GPS fix and an IMU orientation (x, y, z, w); used
  // only by a Graph with gps_sigma_xy / imu_orientation_sigma set.  gps_local = utm_coord - the graph's utm_origin (fp64).
  bool has_utm_coord = false, has_imu_quat = false, has_gps_local = false;
  double utm_coord[3] = {0.0, 0.0, 0.0}, imu_quat[4] = {0.0, 0.0, 0.0, 1.0}, gps_local[3] = {0.0, 0.0, 0.0};
  // the floor found in the surface cloud by a Graph with floor_sigma_normal / floor_sigma_distance set: (n, d) in the sensor
  // frame when has_floor_coeffs; floor_status is the detection's LSLAM_FLOOR_* (-1: not looked for)
  bool has_floor_coeffs = false;
  double floor_coeffs[4] = {0.0, 0.0, 0.0, 0.0};
  int floor_status = -1;
};

// loop_detector.hpp:18-48
struct Loop {
  typedef std::shared_ptr<Loop> Ptr;
  KeyFrame::Ptr key1, key2;
  Mat4d relative_pose;
  // the store ids and transforms (16 floats each) of the keyframes whose local clouds the verification matched against; empty
  // where the keyframes are not in a store -- what Graph::edge_information = "hessian" builds the edge's match Hessian from
  std::vector<int32_t> ref_ids;
  std::vector<float> rel_T;
  // Graph::loop_search = "covariance": e^T (Sigma_rel + Omega_loop^-1)^-1 e when the loop was found (has_mahalanobis)
  bool has_mahalanobis = false;
  double mahalanobis = 0.0;
};

// keyframe_updater.hpp:10-60
class KeyframeUpdater {
public:
  bool update(const Mat4d &pose) {
    if (is_first) {
      is_first = false;
      prev_keypose = pose;
      return true;
    }
    const Mat4d delta = inverse(prev_keypose) * pose;
    const double dx = std::sqrt(delta(0, 3) * delta(0, 3) + delta(1, 3) * delta(1, 3) + delta(2, 3) * delta(2, 3));
    const double c = std::min(1.0, std::max(-1.0, (delta(0, 0) + delta(1, 1) + delta(2, 2) - 1.0) / 2.0));
    const double da = std::acos(c);  // Eigen::AngleAxisd(R).angle()
    if (dx < keyframe_delta_trans && da < keyframe_delta_angle) return false;
    accum_distance += dx;
    prev_keypose = pose;
    frame_count++;
    return true;
  }
  double get_accum_distance() const { return accum_distance; }
  int get_unique_id() { return ++frame_id; }
  double keyframe_delta_trans = 0.25, keyframe_delta_angle = 0.05;

private:
  bool is_first = true;
  Mat4d prev_keypose;
  double accum_distance = 0.0;
  int frame_count = 0, frame_id = 0;
};

// ---- covariance gates (not in the reference): chi-square quantiles and the small dense algebra they need ---------------------
// the two tabulated values the defaults need; Wilson-Hilferty otherwise: k (1 - 2/(9k) + z_p sqrt(2/(9k)))^3
inline double normal_quantile(double p) {  // Acklam's rational approximation, then one Halley step on erfc: ~1e-15
  static const double a[6] = {-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02, 1.383577518672690e+02,
                              -3.066479806614716e+01, 2.506628277459239e+00};
  static const double b[5] = {-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02, 6.680131188771972e+01,
                              -1.328068155288572e+01};
  static const double c[6] = {-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00, -2.549732539343734e+00,
                              4.374664141464968e+00, 2.938163982698783e+00};
  static const double d[4] = {7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00, 3.754408661907416e+00};
  double x;
  if (p < 0.02425) {
    const double q = std::sqrt(-2.0 * std::log(p));
    x = (((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) / ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1.0);
  } else if (p > 1.0 - 0.02425) {
    const double q = std::sqrt(-2.0 * std::log(1.0 - p));
    x = -(((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) / ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1.0);
  } else {
    const double q = p - 0.5, r = q * q;
    x = (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q /
        (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1.0);
  }
  const double e = 0.5 * std::erfc(-x / std::sqrt(2.0)) - p;
  const double u = e * std::sqrt(2.0 * 3.141592653589793) * std::exp(x * x / 2.0);
  return x - u / (1.0 + x * u / 2.0);
}
inline double chi2_quantile_wh(double p, int k) {
  const double a = 2.0 / (9.0 * k);
  const double t = 1.0 - a + normal_quantile(p) * std::sqrt(a);
  return k * t * t * t;
}
inline double chi2_quantile(double p, int k) {
  if (p == 0.99 && k == 3) return 11.345;
  if (p == 0.99 && k == 6) return 16.812;
  return chi2_quantile_wh(p, k);
}
// largest eigenvalue of a symmetric 3x3 (row-major, stride `ld`), closed form
inline double sym3_lambda_max(const double *A, int ld) {
  const double a00 = A[0], a11 = A[ld + 1], a22 = A[2 * ld + 2], a01 = A[1], a02 = A[2], a12 = A[ld + 2];
  const double p1 = a01 * a01 + a02 * a02 + a12 * a12;
  if (p1 == 0.0) return std::max(a00, std::max(a11, a22));
  const double q = (a00 + a11 + a22) / 3.0;
  const double p2 = (a00 - q) * (a00 - q) + (a11 - q) * (a11 - q) + (a22 - q) * (a22 - q) + 2.0 * p1;
  const double p = std::sqrt(p2 / 6.0);
  const double b00 = (a00 - q) / p, b11 = (a11 - q) / p, b22 = (a22 - q) / p, b01 = a01 / p, b02 = a02 / p, b12 = a12 / p;
  const double det = b00 * (b11 * b22 - b12 * b12) - b01 * (b01 * b22 - b12 * b02) + b02 * (b01 * b12 - b11 * b02);
  const double r = std::min(1.0, std::max(-1.0, det / 2.0));
  return q + 2.0 * p * std::cos(std::acos(r) / 3.0);
}
// x^T S^-1 x for an n x n S (n <= 6), Gaussian elimination with partial pivoting; false when S is singular
inline bool quadratic_form_inv(const double *S, int n, const double *x, double *out) {
  double M[6][7];
  for (int r = 0; r < n; ++r) {
    for (int c = 0; c < n; ++c) M[r][c] = S[r * n + c];
    M[r][n] = x[r];
  }
  for (int p = 0; p < n; ++p) {
    int best = p;
    for (int r = p + 1; r < n; ++r)
      if (std::fabs(M[r][p]) > std::fabs(M[best][p])) best = r;
    if (!(std::fabs(M[best][p]) > 0.0)) return false;
    if (best != p)
      for (int c = 0; c <= n; ++c) std::swap(M[p][c], M[best][c]);
    for (int r = p + 1; r < n; ++r) {
      const double f = M[r][p] / M[p][p];
      for (int c = p; c <= n; ++c) M[r][c] -= f * M[p][c];
    }
  }
  double y[6];
  for (int r = n - 1; r >= 0; --r) {
    double s = M[r][n];
    for (int c = r + 1; c < n; ++c) s -= M[r][c] * y[c];
    y[r] = s / M[r][r];
  }
  double q = 0.0;
  for (int r = 0; r < n; ++r) q += x[r] * y[r];
  *out = q;
  return true;
}
// the solver's edge error of an edge (key1, key2) measured as Z at the given estimates: toVectorMQT(Z^-1 X1^-1 X2)
inline void edge_error6(const Mat4d &X1, const Mat4d &X2, const Mat4d &Z, double e[6]) {
  double p[7];
  mat_to_pose7(inverse(Z) * (inverse(X1) * X2), p);
  const double n = std::sqrt(p[3] * p[3] + p[4] * p[4] + p[5] * p[5] + p[6] * p[6]), s = p[6] < 0 ? -1.0 : 1.0;
  for (int k = 0; k < 3; ++k) {
    e[k] = p[k];
    e[3 + k] = s * p[3 + k] / n;
  }
}
// e^T (Sigma_rel + Omega^-1)^-1 e of a verified loop; Omega diagonal (the node's loop information)
inline bool loop_mahalanobis(const Mat4d &X1, const Mat4d &X2, const Mat4d &Z, const double sigma_rel[36], const double info_diag[6],
                             double *d2) {
  double e[6], S[36];
  edge_error6(X1, X2, Z, e);
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) S[r * 6 + c] = sigma_rel[r * 6 + c] + (r == c ? 1.0 / info_diag[r] : 0.0);
  return quadratic_form_inv(S, 6, e, d2);
}

class LoopDetector {
public:
  // loop_detector.hpp:55-63; `ctx` runs the coarse and the fine alignment
  explicit LoopDetector(lslam_ctx *ctx) : _ctx(ctx) { lslam_default_opts(&_opts); }

  double get_distance_thresh() const { return estimated_distance_thresh; }
  int get_loop_count() const { return loop_count; }
  const std::string &lastError() const { return _err; }

  // :66-87
  bool detect_nearest(const std::vector<KeyFrame::Ptr> &keyframes, const std::deque<KeyFrame::Ptr> &new_keyframes,
                      std::vector<Loop::Ptr> &detected_loops) {
    updateTrajectory(keyframes);
    bool loop_found = false;
    for (const auto &nk : new_keyframes) {
      std::vector<KeyFrame::Ptr> candidates;
      if (!find_nearest_candidates(keyframes, nk, candidates)) continue;
      Loop::Ptr loop = matching_nearest(candidates, nk);
      if (loop) {
        detected_loops.push_back(loop);
        loop_count++;
        loop_found = true;
      }
    }
    return loop_found;
  }

  // ---- not in the reference: candidates by appearance (lslam_sc_*) ----
  // The scan-context candidate list of one new keyframe, in its store's ids, best first: empty when the interval rule skips the
  // keyframe or no keyframe is accum_distance_thresh of travel behind it.  No gate on the estimated distance: that is the point.
  // false: a backend error (lastError()).
  bool appearance_candidates(const std::vector<KeyFrame::Ptr> &keyframes, const KeyFrame::Ptr &nk, std::vector<int32_t> &ids,
                             std::vector<int32_t> &shifts, std::vector<float> &dists) {
    ids.clear();
    shifts.clear();
    dists.clear();
    if (!nk->store) { _err = "detect_appearance: the new keyframe is not in a KeyframeStore"; return false; }
    if (nk->accum_distance - last_loop_accum_distance < last_loop_interval_thresh) return true;
    int32_t max_cand = -1;  // accumulated distance is monotone in the id: the eligible candidates are the ids up to one limit
    for (const auto &k : keyframes)
      if (k->store == nk->store && k->store_id < nk->store_id && k->store_id > max_cand &&
          nk->accum_distance - k->accum_distance >= accum_distance_thresh)
        max_cand = k->store_id;
    if (max_cand < 0) return true;
    lslam_sc_stats st;
    if (lslam_sc_info(nk->store, &st) < 0 || (!st.is_set && lslam_sc_setup(nk->store, nullptr) < 0)) {
      _err = lslam_last_error();
      return false;
    }
    const int32_t q = nk->store_id;
    int32_t n = 0;
    ids.assign((size_t)sc_top_k, -1);
    shifts.assign((size_t)sc_top_k, 0);
    dists.assign((size_t)sc_top_k, 1.0f);
    if (lslam_sc_query(nk->store, 1, &q, &max_cand, sc_top_k, ids.data(), shifts.data(), dists.data(), &n) < 0) {
      _err = lslam_last_error();
      ids.clear(); shifts.clear(); dists.clear();
      return false;
    }
    ids.resize((size_t)n);
    shifts.resize((size_t)n);
    dists.resize((size_t)n);
    return true;
  }

  // Loops found from what the new keyframes look like: per new keyframe the sc_top_k nearest scan-context descriptors among the
  // keyframes at least accum_distance_thresh of travel back; those below sc_distance_thresh are verified in list order by
  // lslam_kfs_loop_match (one candidate, started from the rotation the descriptor shift stands for); the first accepted one is
  // the Loop.  All keyframes involved are in one KeyframeStore on this detector's ctx.
  bool detect_appearance(const std::vector<KeyFrame::Ptr> &keyframes, const std::deque<KeyFrame::Ptr> &new_keyframes,
                         std::vector<Loop::Ptr> &detected_loops) {
    bool loop_found = false;
    for (const auto &nk : new_keyframes) {
      std::vector<int32_t> ids, shifts;
      std::vector<float> dists;
      if (!appearance_candidates(keyframes, nk, ids, shifts, dists) || ids.empty()) continue;
      lslam_sc_stats sc;
      if (lslam_sc_info(nk->store, &sc) < 0) { _err = lslam_last_error(); continue; }
      for (size_t i = 0; i < ids.size(); ++i) {
        if (!(dists[i] < (float)sc_distance_thresh)) break;  // the list is sorted
        KeyFrame::Ptr cand;
        for (const auto &k : keyframes)
          if (k->store == nk->store && k->store_id == ids[i]) { cand = k; break; }
        if (!cand) continue;
        float guess[16];
        sc_shift_guess(shifts[i], sc.params.n_sector, sc.params.up_axis, guess);
        float rel[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        int32_t stage = 0, its = 0;
        double fit = 0;
        lslam_stats st;
        if (lslam_kfs_loop_match(nk->store, 1, &ids[i], rel, nk->store_id, guess, 10, &_opts, &stage, &fit, &its, &st) < 0) {
          _err = lslam_last_error();
          continue;
        }
        if (stage != LSLAM_KFS_LOOP_ACCEPTED) continue;
        last_loop_accum_distance = nk->accum_distance;
        Loop::Ptr lp = std::make_shared<Loop>();
        lp->key1 = cand;
        lp->key2 = nk;
        lp->relative_pose = from_float16(guess);
        lp->ref_ids.assign(1, ids[i]);
        lp->rel_T.assign(rel, rel + 16);
        detected_loops.push_back(lp);
        loop_count++;
        loop_found = true;
        break;
      }
    }
    return loop_found;
  }

  // The pose of the query in the candidate's frame that a scan-context shift stands for: the rotation by shift * 2 pi / n_sector
  // about the up axis, zero translation (lslam_c.h, SHIFT) -- lslam_kfs_loop_match's guess.
  static void sc_shift_guess(int32_t shift, int32_t n_sector, int32_t up_axis, float T[16]) {
    const double psi = (double)shift * (6.283185307179586 / (double)n_sector);
    const float c = (float)std::cos(psi), s = (float)std::sin(psi);
    for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    if (up_axis == 1) { T[0] = c; T[2] = s; T[8] = -s; T[10] = c; }   // about +y: z -> x
    else { T[0] = c; T[1] = -s; T[4] = s; T[5] = c; }                 // about +z: x -> y
  }

  // :93-106
  void updateTrajectory(const std::vector<KeyFrame::Ptr> &keyframes) {
    _traj.resize(keyframes.size() * 3);
    for (size_t i = 0; i < keyframes.size(); ++i) {
      _traj[3 * i] = (float)keyframes[i]->estimate(0, 3);
      _traj[3 * i + 1] = 0.0f;
      _traj[3 * i + 2] = (float)keyframes[i]->estimate(2, 3);
    }
  }

  // :108-164
  bool find_nearest_candidates(const std::vector<KeyFrame::Ptr> &keyframes, const KeyFrame::Ptr &nk,
                               std::vector<KeyFrame::Ptr> &candidates) {
    if (nk->accum_distance - last_loop_accum_distance < last_loop_interval_thresh) return false;
    const float pos[3] = {(float)nk->estimate(0, 3), 0.0f, (float)nk->estimate(2, 3)};
    // KdTreeFLANN::radiusSearch(pos, 5.0): squared distances against 5.0, ONE result -- the nearest
    int best = -1;
    float best_d2 = 5.0f;
    for (size_t i = 0; i < _traj.size() / 3; ++i) {
      const float dx = _traj[3 * i] - pos[0], dy = _traj[3 * i + 1] - pos[1], dz = _traj[3 * i + 2] - pos[2];
      const float d2 = (dx * dx + dy * dy) + dz * dz;
      if (d2 < best_d2) { best_d2 = d2; best = (int)i; }
    }
    if (best < 0) return false;
    if (best_d2 >= estimated_distance_thresh) return false;
    const KeyFrame::Ptr &kf = keyframes[(size_t)best];
    if (nk->accum_distance - kf->accum_distance < accum_distance_thresh) return false;
    candidates.push_back(kf);
    return true;
  }

  // ---- not in the reference: candidates by pose uncertainty (lslam_pg_marginals / lslam_pg_relative_covariances) -------------
  // find_nearest_candidates with the fixed sqrt(5) m sphere replaced by one sized by the new keyframe's uncertainty and a
  // Mahalanobis gate per candidate; `pg` holds the keyframes' vertices (KeyFrame::node), the new one's included.
  //   1. radius = max(sqrt(5), sqrt(chi2_3(p) lambda_max(Sigma_nn,tt))) -- a HEURISTIC proxy: uncertainty against the gauge, not
  //      against each candidate; it only has to be generous
  //   2. the old keyframes inside it (this detector's trajectory: y zeroed, as the reference's search) that are
  //      accum_distance_thresh of travel back; the nearest max_candidates of them
  //   3. ONE lslam_pg_relative_covariances call gives their exact Sigma_rel; each is gated on d2 = v^T Sigma_rel,tt^-1 v <=
  //      chi2_3(p), v = R_j^T (t_j - t_new): the relative translation in the candidate's frame, the frame the translation block
  //      of Sigma_rel (an edge error's coordinates) is in
  //   4. survivors in order of d2; then the reference's grouping (5 m of accumulated distance around the first, at most 6)
  // last_gate: (node, d2) of everything step 3 looked at.  false: no candidate, or a backend error (lastError() is set then).
  struct Gated { int node; double d2; };
  std::vector<Gated> last_gate;
  bool find_covariance_candidates(const std::vector<KeyFrame::Ptr> &keyframes, const KeyFrame::Ptr &nk, lslam_pg *pg, double gate_prob,
                                  int max_candidates, const lslam_pg_marginal_opts *opts, std::vector<KeyFrame::Ptr> &candidates) {
    last_gate.clear();
    _err.clear();
    if (nk->accum_distance - last_loop_accum_distance < last_loop_interval_thresh) return false;
    const double chi2 = chi2_quantile(gate_prob, 3);
    double s_nn[36];
    const int32_t nn = nk->node;
    if (lslam_pg_marginals(pg, 1, &nn, opts, s_nn, nullptr, nullptr) < 0) {
      _err = lslam_pg_last_error();
      return false;
    }
    const double radius2 = std::max(5.0, chi2 * std::max(sym3_lambda_max(s_nn, 6), 0.0));
    const double pos[3] = {nk->estimate(0, 3), 0.0, nk->estimate(2, 3)};
    const size_t n = _traj.size() / 3;
    std::vector<double> d2(n);
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; ++i) {
      const double dx = (double)_traj[3 * i] - pos[0], dy = (double)_traj[3 * i + 1] - pos[1], dz = (double)_traj[3 * i + 2] - pos[2];
      d2[i] = dx * dx + dy * dy + dz * dz;
      order[i] = i;
    }
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return d2[a] < d2[b]; });
    std::vector<KeyFrame::Ptr> near;
    for (size_t k = 0; k < n; ++k) {
      if (!(d2[order[k]] < radius2) || (int)near.size() >= max_candidates) break;
      const KeyFrame::Ptr &kf = keyframes[order[k]];
      if (kf == nk || nk->accum_distance - kf->accum_distance < accum_distance_thresh) continue;
      near.push_back(kf);
    }
    if (near.empty()) return false;
    std::vector<int32_t> nodes;
    for (const auto &kf : near) nodes.push_back(kf->node);
    std::vector<double> s_rel(near.size() * 36);
    if (lslam_pg_relative_covariances(pg, nn, (int32_t)nodes.size(), nodes.data(), opts, s_rel.data(), nullptr) < 0) {
      _err = lslam_pg_last_error();
      return false;
    }
    struct Pass { double d2; size_t k; };
    std::vector<Pass> gated;
    for (size_t k = 0; k < near.size(); ++k) {
      const Mat4d &E = near[k]->estimate;
      const double t[3] = {E(0, 3) - nk->estimate(0, 3), E(1, 3) - nk->estimate(1, 3), E(2, 3) - nk->estimate(2, 3)};
      double v[3], S[9], m = 0.0;
      for (int r = 0; r < 3; ++r) {
        v[r] = E(0, r) * t[0] + E(1, r) * t[1] + E(2, r) * t[2];
        for (int c = 0; c < 3; ++c) S[r * 3 + c] = s_rel[k * 36 + r * 6 + c];
      }
      if (!quadratic_form_inv(S, 3, v, &m)) m = INFINITY;
      last_gate.push_back(Gated{near[k]->node, m});
      if (m <= chi2) gated.push_back(Pass{m, k});
    }
    std::stable_sort(gated.begin(), gated.end(), [](const Pass &a, const Pass &b) { return a.d2 < b.d2; });
    double candidate_dist = 0.0;
    for (const Pass &g : gated) {
      if (candidates.size() >= 6) break;
      const KeyFrame::Ptr &kf = near[g.k];
      if (candidates.empty()) candidate_dist = kf->accum_distance;
      else if (std::fabs(candidate_dist - kf->accum_distance) > 5.0) continue;
      candidates.push_back(kf);
    }
    return !candidates.empty();
  }
  // detect_nearest over find_covariance_candidates; false with lastError() set on a backend error
  bool detect_covariance(const std::vector<KeyFrame::Ptr> &keyframes, const std::deque<KeyFrame::Ptr> &new_keyframes, lslam_pg *pg,
                         double gate_prob, int max_candidates, const lslam_pg_marginal_opts *opts, std::vector<Loop::Ptr> &detected_loops) {
    updateTrajectory(keyframes);
    for (const auto &nk : new_keyframes) {
      std::vector<KeyFrame::Ptr> candidates;
      if (!find_covariance_candidates(keyframes, nk, pg, gate_prob, max_candidates, opts, candidates)) {
        if (!_err.empty()) return false;
        continue;
      }
      Loop::Ptr loop = matching_nearest(candidates, nk);
      if (loop) {
        detected_loops.push_back(loop);
        loop_count++;
      }
    }
    return true;
  }

  // :166-230
  Loop::Ptr matching_nearest(const std::vector<KeyFrame::Ptr> &candidates, const KeyFrame::Ptr &nk) {
    if (candidates.empty()) return nullptr;
    const Mat4d inv = inverse(candidates[0]->estimate);
    bool stored = nk->store != nullptr && candidates.size() <= 6;
    for (const auto &c : candidates) stored = stored && c->store == nk->store;
    if (stored) return matching_nearest_stored(candidates, nk, inv);
    std::vector<float> cornerLocal = candidates[0]->cornerCloud, surfLocal = candidates[0]->surfCloud;
    for (size_t i = 1; i < candidates.size(); ++i) {
      float rel[16];
      to_float16(inv * candidates[i]->estimate, rel);
      append_transformed(candidates[i]->cornerCloud, rel, cornerLocal);
      append_transformed(candidates[i]->surfCloud, rel, surfLocal);
    }
    float guess[16];
    to_float16(inv * nk->estimate, guess);
    // corseMatching, :232-255
    if (surfLocal.empty()) return nullptr;
    int32_t conv = 0, its = 0;
    double fit = 0;
    if (lslam_icp_align(_ctx, surfLocal.data(), surfLocal.size() / 4, nk->surfCloud.data(), nk->surfCloud.size() / 4, 16, guess, 10,
                        0.0, 0.0, &fit, &conv, &its) < 0) {
      _err = lslam_last_error();
      return nullptr;
    }
    if (!conv) return nullptr;
    // scan_match.scanMatchLocal(cornerLocal, surfLocal, corner, surf, guess2): VoxelGrid 0.2 / 0.4, then scanMatchScan
    std::vector<float> ds[4];
    const std::vector<float> *in[4] = {&cornerLocal, &surfLocal, &nk->cornerCloud, &nk->surfCloud};
    const float leaf[4] = {0.2f, 0.4f, 0.2f, 0.4f};
    for (int k = 0; k < 4; ++k) {
      ds[k].resize(in[k]->size() + 4);
      size_t n = 0;
      if (lslam_voxel_grid(_ctx, in[k]->data(), in[k]->size() / 4, 16, leaf[k], ds[k].data(), in[k]->size() / 4, &n) < 0) {
        _err = lslam_last_error();
        return nullptr;
      }
      ds[k].resize(4 * n);
    }
    float pose[6];
    lslam_isometry_to_pose(guess, pose);
    lslam_stats st;
    const int rc = lslam_scanmatch_full(_ctx, ds[0].data(), ds[0].size() / 4, ds[1].data(), ds[1].size() / 4, 16, ds[2].data(),
                                        ds[2].size() / 4, ds[3].data(), ds[3].size() / 4, 16, pose, &_opts, &st);
    if (rc < 0) _err = lslam_last_error();
    if (rc != LSLAM_OK) return nullptr;  // hasConverged == false
    lslam_pose_to_isometry(pose, guess);
    last_loop_accum_distance = nk->accum_distance;
    Loop::Ptr lp = std::make_shared<Loop>();
    lp->key1 = candidates[0];
    lp->key2 = nk;
    lp->relative_pose = from_float16(guess);
    return lp;
  }

  double estimated_distance_thresh = 25.0, accum_distance_thresh = 30.0, last_loop_interval_thresh = 3.0,
         fitness_score_thresh = 0.5;
  // detect_appearance.  0.2 is the upper end of the range the descriptor's authors use; not tuned on this project's data
  double sc_distance_thresh = 0.2;
  int sc_top_k = 4;

private:
  // the same for keyframes whose clouds are in a KeyframeStore: one call, no cloud crosses PCIe (lslam_kfs_loop_match)
  Loop::Ptr matching_nearest_stored(const std::vector<KeyFrame::Ptr> &candidates, const KeyFrame::Ptr &nk, const Mat4d &inv) {
    std::vector<int32_t> ids;
    std::vector<float> rel(16 * candidates.size());
    for (size_t i = 0; i < candidates.size(); ++i) {
      ids.push_back(candidates[i]->store_id);
      to_float16(inv * candidates[i]->estimate, &rel[16 * i]);
    }
    float guess[16];
    to_float16(inv * nk->estimate, guess);
    int32_t stage = 0, its = 0;
    double fit = 0;
    lslam_stats st;
    if (lslam_kfs_loop_match(nk->store, (int32_t)ids.size(), ids.data(), rel.data(), nk->store_id, guess, 10, &_opts, &stage, &fit,
                             &its, &st) < 0) {
      _err = lslam_last_error();
      return nullptr;
    }
    if (stage != LSLAM_KFS_LOOP_ACCEPTED) return nullptr;
    last_loop_accum_distance = nk->accum_distance;
    Loop::Ptr lp = std::make_shared<Loop>();
    lp->key1 = candidates[0];
    lp->key2 = nk;
    lp->relative_pose = from_float16(guess);
    lp->ref_ids = ids;
    lp->rel_T = rel;
    return lp;
  }
  static void append_transformed(const std::vector<float> &c, const float T[16], std::vector<float> &out) {
    for (size_t i = 0; i + 3 < c.size(); i += 4) {  // pcl::transformPointCloud, fp32
      const float x = c[i], y = c[i + 1], z = c[i + 2];
      out.push_back(((T[0] * x + T[1] * y) + T[2] * z) + T[3]);
      out.push_back(((T[4] * x + T[5] * y) + T[6] * z) + T[7]);
      out.push_back(((T[8] * x + T[9] * y) + T[10] * z) + T[11]);
      out.push_back(c[i + 3]);
    }
  }
  lslam_ctx *_ctx;
  lslam_opts _opts;
  std::vector<float> _traj;
  int loop_count = 0;
  double last_loop_accum_distance = 0.0;
  std::string _err;
};

// pose_graph::Graph (graph.cpp:230-385) with SolverG2O (solver_g2o.cpp:51-95) folded in: vertices / edges are
// kept on the host and handed to lslam_pg_* when an optimisation is due.
class Graph {
public:
  // resident: the keyframes' clouds live in a KeyframeStore on `ctx` (add_frame uploads them once); keep_host_clouds = false
  // then leaves KeyFrame::cornerCloud / surfCloud empty (KeyframeStore::get fetches a cloud when one is wanted)
  // appearance_loops (not in the reference; implies resident): optimize also runs LoopDetector::detect_appearance -- scan-context
  // candidates over the store, sc_params being lslam_sc_setup's (nullptr: the defaults) -- for the new keyframes for which
  // detect_nearest found no loop
  explicit Graph(lslam_ctx *ctx, int device = 0, int max_keyframes_per_update = 10, bool resident = false,
                 bool keep_host_clouds = true, bool appearance_loops = false, const lslam_sc_params *sc_params = nullptr)
      : loop_detector(ctx), _ctx(ctx), _device(device), _max_per_update(max_keyframes_per_update), _keep_host(keep_host_clouds),
        _appearance(appearance_loops) {
    lslam_floor_default_params(&floor_params);
    lslam_vis_default_params(&dynamic_params);
    lslam_occ_default_params(&occupancy_params);
    if (resident || appearance_loops) {
      store.reset(new KeyframeStore(ctx));
      if (!store->ok()) _err = store->lastError();
      else if (appearance_loops && !store->sc_setup(sc_params)) _err = store->lastError();
    }
  }

  // graph.cpp:230-246: returns the queued keyframe, or null when the pose did not move enough
  KeyFrame::Ptr add_frame(const Mat4d &odom, const std::vector<float> &corner, const std::vector<float> &surf) {
    if (!keyframe_updater.update(odom)) return nullptr;
    KeyFrame::Ptr kf = std::make_shared<KeyFrame>();
    kf->odom = odom;
    kf->accum_distance = keyframe_updater.get_accum_distance();
    if (store) {
      kf->store_id = store->add(corner, surf);
      if (kf->store_id < 0) {  // (a full store: the message names the limit)
        _err = store->lastError();
        return nullptr;
      }
      kf->store = store->handle();
    }
    if (!store || _keep_host) {
      kf->cornerCloud = corner;
      kf->surfCloud = surf;
    }
    kf->frame_id = keyframe_updater.get_unique_id();
    keyframe_queue.push_back(kf);
    return kf;
  }
  // ... with keyframe.h:40-41's optional fields: utm_coord[3] (x, y, z [m], projected -- what kf_fusion/fpdReceiver.cpp makes of
  // a fix) and imu_quat[4] (x, y, z, w); either may be null.  Stored on the keyframe; used only with gps_sigma_xy /
  // imu_orientation_sigma.
  KeyFrame::Ptr add_frame(const Mat4d &odom, const std::vector<float> &corner, const std::vector<float> &surf, const double *utm_coord,
                          const double *imu_quat) {
    KeyFrame::Ptr kf = add_frame(odom, corner, surf);
    if (!kf) return kf;
    if (utm_coord) {
      kf->has_utm_coord = true;
      for (int k = 0; k < 3; ++k) kf->utm_coord[k] = utm_coord[k];
    }
    if (imu_quat) {
      kf->has_imu_quat = true;
      for (int k = 0; k < 4; ++k) kf->imu_quat[k] = imu_quat[k];
    }
    return kf;
  }

  // one pass of the optimisation loop, graph.cpp:313-383: flush the queue (vertices + odometry edges), detect loops
  // among the new keyframes, add loop edges, optimise if a loop was found, update odom -> graph.
  // Returns the number of loops found (-1 on a backend error).
  int optimize(int max_iterations = 1000) {
    const int loop_kind = lslam_pg_kernel_from_name(loop_robust_kernel.c_str());
    if (loop_kind < 0) {  // both checked before anything is added: a refused kernel must not leave edges behind
      _err = "Graph: unknown loop_robust_kernel " + loop_robust_kernel + " (NONE, Huber, Cauchy, DCS)";
      return -1;
    }
    if (loop_kind != LSLAM_PG_KERNEL_NONE && !(std::isfinite(loop_robust_kernel_size) && loop_robust_kernel_size > 0.0)) {
      _err = "Graph: loop_robust_kernel_size must be finite and > 0";
      return -1;
    }
    const bool hessian = edge_information == "hessian";
    if (!hessian && edge_information != "NONE") {
      _err = "Graph: unknown edge_information " + edge_information + " (NONE, hessian)";
      return -1;
    }
    if (hessian && !(std::isfinite(range_sigma) && range_sigma > 0.0)) {
      _err = "Graph: edge_information = hessian needs range_sigma, the sensor's range noise [m]";
      return -1;
    }
    if (hessian && !store) {
      _err = "Graph: edge_information = hessian needs a resident graph";
      return -1;
    }
    const int gps_kind = lslam_pg_kernel_from_name(gps_robust_kernel.c_str());
    if (gps_kind < 0 || (gps_kind != LSLAM_PG_KERNEL_NONE && !(std::isfinite(gps_robust_kernel_size) && gps_robust_kernel_size > 0.0))) {
      _err = "Graph: gps_robust_kernel is NONE, Huber, Cauchy or DCS with a finite gps_robust_kernel_size > 0";
      return -1;
    }
    if (!(gps_sigma_xy >= 0.0 && gps_sigma_z >= 0.0 && std::isfinite(gps_sigma_xy) && std::isfinite(gps_sigma_z)) ||
        ((gps_sigma_xy > 0.0) != (gps_sigma_z > 0.0)) || !(imu_orientation_sigma >= 0.0) || !(gps_min_spread >= 0.0)) {
      _err = "Graph: gps_sigma_xy and gps_sigma_z [m] are set together, both > 0; imu_orientation_sigma [rad] and gps_min_spread [m] >= 0";
      return -1;
    }
    const int floor_kind = lslam_pg_kernel_from_name(floor_robust_kernel.c_str());
    if (floor_kind < 0 || (floor_kind != LSLAM_PG_KERNEL_NONE && !(std::isfinite(floor_robust_kernel_size) && floor_robust_kernel_size > 0.0))) {
      _err = "Graph: floor_robust_kernel is NONE, Huber, Cauchy or DCS with a finite floor_robust_kernel_size > 0";
      return -1;
    }
    if (!(floor_sigma_normal >= 0.0 && floor_sigma_distance >= 0.0 && std::isfinite(floor_sigma_normal) && std::isfinite(floor_sigma_distance)) ||
        ((floor_sigma_normal > 0.0) != (floor_sigma_distance > 0.0))) {
      _err = "Graph: floor_sigma_normal [rad] and floor_sigma_distance [m] are set together, both > 0";
      return -1;
    }
    const bool covariance = loop_search == "covariance";
    if (!covariance && loop_search != "NONE") {
      _err = "Graph: unknown loop_search " + loop_search + " (NONE, covariance)";
      return -1;
    }
    if (covariance && (!(loop_gate_prob > 0.0 && loop_gate_prob < 1.0) || loop_max_candidates < 1 ||
                       !(loop_consistency_prob >= 0.0 && loop_consistency_prob < 1.0))) {
      _err = "Graph: loop_gate_prob in (0, 1), loop_max_candidates >= 1, loop_consistency_prob in [0, 1) (0: record only)";
      return -1;
    }
    _edge_failed = false;
    const bool flushed = flush_keyframe_queue();
    if (_edge_failed) return -1;
    if (!flushed) return 0;
    std::vector<Loop::Ptr> found;
    std::deque<KeyFrame::Ptr> nk(new_keyframes.begin(), new_keyframes.end());
    struct PgGuard {  // the solver graph the covariances are asked of: the vertices and odometry edges just flushed included
      lslam_pg *pg;
      ~PgGuard() { lslam_pg_destroy(pg); }
    } cov{nullptr};
    if (covariance && !(cov.pg = make_pg())) return -1;
    if (loop_source) loop_source(keyframes, nk, found);
    else if (covariance) {
      if (!loop_detector.detect_covariance(keyframes, nk, cov.pg, loop_gate_prob, loop_max_candidates, &covariance_opts, found)) {
        _err = loop_detector.lastError();
        return -1;
      }
    } else loop_detector.detect_nearest(keyframes, nk, found);
    if (_appearance && !loop_source) {
      std::deque<KeyFrame::Ptr> open;
      for (const auto &k : nk) {
        bool closed = false;
        for (const auto &lp : found) closed = closed || lp->key2 == k;
        if (!closed) open.push_back(k);
      }
      loop_detector.detect_appearance(keyframes, open, found);
    }
    static const double LOOP_INFO[6] = {2, 2, 2, 2, 2, 2};  // graph.cpp:333-339
    if (covariance) {  // every loop, whichever detector found it: its Mahalanobis distance; dropped only when a probability is set
      std::vector<Loop::Ptr> keep;
      for (const auto &lp : found) {
        if (!loop_consistency(cov.pg, lp->key1, lp->key2, lp->relative_pose, &lp->mahalanobis)) return -1;
        lp->has_mahalanobis = true;
        if (loop_consistency_prob > 0.0 && lp->mahalanobis > chi2_quantile(loop_consistency_prob, 6)) _inconsistent.push_back(lp);
        else keep.push_back(lp);
      }
      found.swap(keep);
    }
    for (const auto &lp : found) {
      double full[36];
      if (hessian) {
        if (lp->ref_ids.empty()) {
          _err = "Graph: edge_information = hessian needs loops verified in the keyframe store";
          return -1;
        }
        if (!hessian_information(LOOP_INFO, lp->ref_ids, lp->rel_T, lp->key2->store_id, lp->relative_pose, full)) return -1;
      }
      _loop_edges.push_back((int)(_ij.size() / 2));
      add_edge(lp->key1->node, lp->key2->node, lp->relative_pose, LOOP_INFO, loop_kind, loop_robust_kernel_size, hessian ? full : nullptr);
    }
    loops.insert(loops.end(), found.begin(), found.end());
    keyframes.insert(keyframes.end(), new_keyframes.begin(), new_keyframes.end());
    const bool added_priors = add_priors(new_keyframes, gps_kind);
    bool added_floors = false;
    if (!add_floors(new_keyframes, floor_kind, &added_floors)) return -1;
    new_keyframes.clear();
    last_iterations = 0;
    if (!found.empty() || added_priors || added_floors) {
      if (!solve_graph(max_iterations, nullptr, nullptr)) return -1;
    }
    const KeyFrame::Ptr &last = keyframes.back();
    tf_odom2graph = last->estimate * inverse(last->odom);
    return (int)found.size();
  }

  // Graph::getFinalFeatureMap (graph.cpp:150-199; called by Graph::save, :106-147): the optimised keyframes rebuilt into a map
  // ONE AFTER THE OTHER -- keyframe k is matched against a map that already holds keyframes 0 .. k-1:
  //   feature_map2.update(estimate) -> getSurroundFeature -> VoxelGrid 0.2 / 0.3 of the keyframe's clouds -> scanMatchScan (a
  //   default ScanMatch) from the estimate -> addFeatureCloud with the refined estimate iff matched -> saveCloudToFiles(directory)
  // all on the device (lslam_fmap_*: the map never leaves HBM between keyframes).  matched[k] / poses[k]: per keyframe.
  // Quirk kept with bootstrap = false (the reference as written): the map starts empty, the first match returns false for want
  // of reference points (ScanMatch.cpp:57-61), nothing is added -- and so for every keyframe after it.  bootstrap = true adds a
  // keyframe WITHOUT a match while the surround holds fewer than the 50 / 100 points a match needs.  The caller destroys *map_out
  // (lslam_fmap_destroy); returns the number of keyframes added, -1 on a backend error.
  int getFinalFeatureMap(lslam_ctx *ctx, const std::string &directory, bool bootstrap, std::vector<char> &matched,
                         std::vector<Mat4d> &poses, lslam_fmap **map_out, int cubeWidth = 121, int cubeHeight = 111,
                         int cubeDepth = 121) {
    matched.clear();
    poses.clear();
    removedPoints.clear();
    if (remove_dynamic && (!store || ctx != _ctx)) {
      _err = "Graph: remove_dynamic needs a resident graph and the map on its context";
      return -1;
    }
    lslam_fmap *fm = nullptr;
    if (lslam_fmap_create(ctx, cubeWidth, cubeHeight, cubeDepth, &fm) != LSLAM_OK) return fail_final(nullptr);
    lslam_fmap_setup_filter_size(fm, 0.2f, 0.2f, 0.4f);
    lslam_opts opts;
    lslam_default_opts(&opts);  // lidar_slam::ScanMatch scan_match;
    int added = 0;
    std::vector<float> cc, cs;
    for (const auto &kf : keyframes) {
      float T[16];
      to_float16(kf->estimate, T);  // node->estimate().cast<float>()
      const float pos[3] = {T[3], T[7], T[11]};
      if (lslam_fmap_update(fm, pos) < 0) return fail_final(fm);
      size_t nc = 0, ns = 0;
      if (lslam_fmap_surround_counts(fm, &nc, &ns) < 0) return fail_final(fm);
      // a stored keyframe is filtered, matched and added where it is (lslam_kfs_scanmatch, lslam_kfs_add_to_fmap)
      const bool stored = kf->store != nullptr && ctx == _ctx;
      const size_t kc = kf->cornerCloud.size() / 4, ks = kf->surfCloud.size() / 4;
      size_t mc = 0, ms = 0;
      if (!stored) {
        cc.resize(4 * kc + 4);
        cs.resize(4 * ks + 4);
        if (lslam_voxel_grid(ctx, kf->cornerCloud.data(), kc, 16, 0.2f, cc.data(), kc, &mc) < 0) return fail_final(fm);
        if (lslam_voxel_grid(ctx, kf->surfCloud.data(), ks, 16, 0.3f, cs.data(), ks, &ms) < 0) return fail_final(fm);
      }
      bool ok = false;
      const bool enough = nc >= 50 && ns >= 100;
      if (enough) {
        if (lslam_fmap_surround_to_map(fm) < 0) return fail_final(fm);
        float pose[6];
        lslam_isometry_to_pose(T, pose);
        lslam_stats st;
        const int rc = stored ? lslam_kfs_scanmatch(kf->store, kf->store_id, 0.2f, 0.3f, pose, &opts, &st)
                              : lslam_scanmatch_scan(ctx, cc.data(), mc, cs.data(), ms, 16, pose, &opts, &st);
        if (rc < 0) return fail_final(fm);
        if (rc != LSLAM_TOO_FEW_REF) lslam_pose_to_isometry(pose, T);  // written back also when the match failed (:342-346)
        ok = rc == LSLAM_OK;
      }
      if (ok || (bootstrap && !enough)) {
        if ((stored ? add_stored(kf, fm, T, true)
                    : lslam_fmap_add_feature_cloud(fm, kf->cornerCloud.data(), kc, kf->surfCloud.data(), ks, 16, T)) < 0)
          return fail_final(fm);
        ++added;
      }
      matched.push_back(ok ? 1 : 0);
      poses.push_back(from_float16(T));
    }
    if (!directory.empty() && lslam_fmap_save(fm, directory.c_str()) < 0) return fail_final(fm);
    if (map_out) *map_out = fm;
    else lslam_fmap_destroy(fm);
    return added;
  }

  // Graph::save (graph.cpp:106-147) with the reference's hard-coded paths replaced by `directory` (which must exist, with its
  // subdirectories graph/ and graph2/: saveCloudToFiles writes into an existing directory): graph_before.g2o, a final
  // optimisation, graph_end.g2o, the keyframes' estimates and tf_odom2graph refreshed, the map of all keyframes at their
  // optimised poses (FeatureMap(121, 111, 121) with its default filter sizes: update + addFeatureCloud per keyframe, no match)
  // into directory/graph, traj_graph.pcd and traj_odom.pcd (ASCII; x y z intensity normal_x normal_y normal_z curvature =
  // translation, quaternion w, quaternion x y z of the float-cast rotation, index), then getFinalFeatureMap into directory/graph2.
  // With `occupancy` on, also directory/map.pgm and map.yaml (occupancyGrid, saveMap); off: nothing new is written.
  bool save(const std::string &directory, bool bootstrap = false, int max_iterations = 1000) {
    if (keyframes.empty()) { _err = "Graph::save: no keyframes"; return false; }
    if (remove_dynamic && !store) { _err = "Graph: remove_dynamic needs a resident graph"; return false; }
    // (the .g2o files carry no kernel: the text format has no place for one)
    const std::string before = directory + "/graph_before.g2o", end = directory + "/graph_end.g2o";
    if (!solve_graph(max_iterations, before.c_str(), end.c_str())) return false;
    tf_odom2graph = keyframes.back()->estimate * inverse(keyframes.back()->odom);
    lslam_fmap *fm = nullptr;
    if (lslam_fmap_create(_ctx, 121, 111, 121, &fm) != LSLAM_OK) return fail_final(nullptr) >= 0;
    for (const auto &kf : keyframes) {
      float T[16];
      to_float16(kf->estimate, T);
      const float pos[3] = {T[3], T[7], T[11]};
      if (lslam_fmap_update(fm, pos) < 0) return fail_final(fm) >= 0;
      if ((kf->store ? add_stored(kf, fm, T, false)
                     : lslam_fmap_add_feature_cloud(fm, kf->cornerCloud.data(), kf->cornerCloud.size() / 4, kf->surfCloud.data(),
                                                    kf->surfCloud.size() / 4, 16, T)) < 0)
        return fail_final(fm) >= 0;
    }
    if (lslam_fmap_save(fm, (directory + "/graph").c_str()) < 0) return fail_final(fm) >= 0;
    lslam_fmap_destroy(fm);
    if (!save_trajectory_cloud(directory + "/traj_graph.pcd", false) || !save_trajectory_cloud(directory + "/traj_odom.pcd", true)) {
      _err = "Graph::save: cannot write the trajectory clouds";
      return false;
    }
    std::vector<char> matched;
    std::vector<Mat4d> poses;
    if (getFinalFeatureMap(_ctx, directory + "/graph2", bootstrap, matched, poses, nullptr) < 0) return false;
    if (!occupancy) return true;
    std::vector<int8_t> values;
    std::vector<uint32_t> counts;
    lslam_occ_params p;
    if (!occupancyGrid(values, counts, p)) return false;
    if (!saveMap(directory + "/map", values, p)) { _err = "Graph::save: cannot write map.pgm / map.yaml"; return false; }
    return true;
  }

  LoopDetector loop_detector;
  KeyframeUpdater keyframe_updater;
  std::unique_ptr<KeyframeStore> store;  // resident graphs only
  std::vector<KeyFrame::Ptr> keyframes, new_keyframes;
  std::deque<KeyFrame::Ptr> keyframe_queue;
  std::vector<Loop::Ptr> loops;
  // A robust kernel on every LOOP edge added from now on (not in the reference, which includes g2o's robust-kernel headers and
  // uses none): "NONE" (default: every edge at full weight), "Huber", "Cauchy" or "DCS" with delta loop_robust_kernel_size;
  // semantics in lslam_c.h.  Odometry edges never carry one.  Huber is convex: it bounds a false loop's pull but cannot
  // reject it; Cauchy (0.1) and DCS (1) can.  Reporting only: nothing is removed from the graph.
  std::string loop_robust_kernel = "NONE";
  double loop_robust_kernel_size = 1.0;
  // Covariance-gated loops (not in the reference, whose search is a fixed sqrt(5) m sphere): "NONE" (default: nothing changes)
  // or "covariance" -- the candidates of a new keyframe are searched inside a radius sized by its pose uncertainty and gated on
  // the Mahalanobis distance of the relative translation at probability loop_gate_prob, the nearest loop_max_candidates at most
  // (LoopDetector::find_covariance_candidates; lslam_pg_marginals / lslam_pg_relative_covariances with covariance_opts).  Every
  // loop found by any detector then carries Loop::mahalanobis = e^T (Sigma_rel + Omega_loop^-1)^-1 e, e the edge error of the
  // verified relative pose at the current estimates; with loop_consistency_prob > 0 a loop whose value exceeds the chi-square
  // quantile with 6 degrees of freedom is dropped before it reaches the solver: inconsistentLoops().
  std::string loop_search = "NONE";
  double loop_gate_prob = 0.99;
  int loop_max_candidates = 32;
  double loop_consistency_prob = 0.0;
  lslam_pg_marginal_opts covariance_opts = {0.0, 0, -1};
  const std::vector<Loop::Ptr> &inconsistentLoops() const { return _inconsistent; }
  // Loop::mahalanobis of a (would-be) loop edge key1 -> key2 at the current estimates, both keyframes in the solver's arrays
  bool loopConsistency(const KeyFrame::Ptr &key1, const KeyFrame::Ptr &key2, const Mat4d &relative_pose, double *d2) {
    lslam_pg *pg = make_pg();
    if (!pg) return false;
    const bool ok = loop_consistency(pg, key1, key2, relative_pose, d2);
    lslam_pg_destroy(pg);
    return ok;
  }
  // the robust weight of every entry of `loops` after the last optimisation (all 1 without a kernel)
  const std::vector<double> &loopWeights() const { return _loop_weights; }
  // Data-driven edge information (not in the reference, whose InformationEstimator returns the identity): "NONE" (default:
  // graph.cpp's constants) or "hessian" -- every edge added from now on gets
  //   Omega = Omega_ref + H / max(sum_b2 / (n_rows - 6), range_sigma^2),        Omega_ref alone below 50 rows (ScanMatch.cpp:142)
  // with H, sum_b2, n_rows the fp64 match Hessian of the edge's two keyframes at its measurement (lslam_keyframe_edge_information:
  // odometry edges against the previous keyframe, loop edges against the keyframes their verification used; leaves 0.2 / 0.4 /
  // 0.2 / 0.4 as scanMatchLocal) and Omega_ref graph.cpp's constant for the edge type, a weak prior: Omega stays positive
  // definite, and a direction the match did not observe keeps exactly the reference's weight.  Needs a resident graph and
  // range_sigma [m], the range noise of the caller's sensor -- no default: the library does not guess it.
  std::string edge_information = "NONE";
  double range_sigma = 0.0;
  // the lslam_edge_info of every edge in edge order (edge_information = "hessian" only), and every edge's 6x6 information
  const std::vector<lslam_edge_info> &edgeInformations() const { return _edge_infos; }
  const std::vector<double> &informationMatrices() const { return _info; }
  // Where the loops come from, when set: called by optimize() instead of loop_detector's detect_nearest / detect_appearance
  // with (keyframes, new keyframes, loops out).  The counterpart of the Python Graph's loop_detector argument: a node that has
  // its own place recognition, or a test with prepared loops, hands them over here.
  std::function<void(const std::vector<KeyFrame::Ptr> &, const std::deque<KeyFrame::Ptr> &, std::vector<Loop::Ptr> &)> loop_source;
  // GPS fixes and IMU orientations as unary constraints (not in the reference, whose keyframes only carry the two fields;
  // lslam_pg_set_priors, semantics in lslam_c.h).  All off by default (0).
  //   gps_sigma_xy / gps_sigma_z [m]: the fixes handed to add_frame become XYZ priors with information diag(1/sxy^2, 1/sxy^2,
  //     1/sz^2) and gps_robust_kernel / gps_robust_kernel_size on each (multipath: "Cauchy" rejects an outlying fix).  No
  //     default: the library does not guess a receiver's noise.  utm_origin is the first keyframe fix, kept in fp64 on the host
  //     and subtracted before anything reaches the solver (UTM coordinates are ~1e6 m).
  //   GAUGE: the graph frame starts as the first lidar pose, not ENU; priors under a fixed, misaligned first vertex would bend
  //     the map.  Until the fixes span a plane -- the second singular value of the centred fix positions >= gps_min_spread
  //     (0: 10 * gps_sigma_xy) -- priors are queued and the first vertex stays fixed (the reference's behaviour); then the
  //     keyframe estimates and tf_odom2graph are moved by the rigid fit of estimate positions to fixes (lslam_debug_icp_fit),
  //     all queued priors are added and the solver runs with no fixed vertex from there on.
  //   imu_orientation_sigma [rad]: a keyframe's imu_quat (in the frame the fixes are in) becomes a POSE prior with a zero
  //     translation block and (2 / sigma)^2 on the quaternion vector; queued with the fixes when the GPS switch is on.
  // optimize() then runs the solver when a pass added loops OR priors.
  // Floor planes as plane priors (not in the reference, which only shows the intent: solver_g2o.h:61-65, :92, graph.cpp:321;
  // lslam_floor_detect*, lslam_pg_set_plane_priors, semantics in lslam_c.h).  Off by default (0).
  //   floor_sigma_normal [rad] / floor_sigma_distance [m]: on each pass the floor of every new keyframe's surface cloud is
  //     detected on the device with floor_params (the defaults unless changed) -- one KeyframeStore::floorDetect call over the
  //     store of a resident graph, one lslam_floor_detect per cloud otherwise.  An accepted floor becomes the keyframe's
  //     floor_coeffs and a plane prior against floor_world_plane -- the floor in the GRAPH frame, z = 0 by default; a graph frame
  //     that starts at the first sensor pose has its floor at (0, 0, 1, sensor_height) -- with information diag(1/sn^2, 1/sn^2,
  //     1/sd^2) and floor_robust_kernel / floor_robust_kernel_size.  A keyframe whose floor was not found adds nothing and is
  //     counted (floorsNotFound).  No default: the library does not guess the detection's noise.
  //   LIMIT: with the reference's constant odometry information (sigma about 1 m / 0.7 rad) bending the trajectory onto an
  //     outlying floor costs less than any kernel charges for rejecting it: a kernel rejects only when the edges are worth
  //     something -- odometry_information below, or edge_information = "hessian".
  // The final map without moving objects (not in the reference, whose addFeatureCloud only voxel-filters; lslam_vis_*, semantics in
  // lslam_c.h).  Off by default.  With remove_dynamic on a resident graph, getFinalFeatureMap and the unmatched map of save add a
  // keyframe through lslam_vis_add_to_fmap: its points, at the pose they are added with, are voted on by every keyframe, itself
  // included, whose optimised translation lies within 2 * max_range of its own, at its optimised estimate; what the votes call
  // dynamic -- a car that stood at a junction for two keyframes and drove off -- is left out.  dynamic_params: lslam_vis_setup's
  // (the defaults unless changed).  removedPoints: (corner, surf) points left out per keyframe getFinalFeatureMap added.
  bool remove_dynamic = false;
  lslam_vis_params dynamic_params;
  // The 2D occupancy grid of the keyframes' ray-cast votes (not in the reference; lslam_occ_*, semantics in lslam_c.h): with
  // `occupancy` on a resident graph, save also writes directory/map.pgm and map.yaml (saveMap).  occupancy_params: lslam_occ_setup's;
  // while width or height is 0 the bounds are fitted to the poses (lslam_occ_fit_bounds).  Off by default.
  bool occupancy = false;
  lslam_occ_params occupancy_params;
  // Clears the store's grid and integrates every keyframe at its optimised estimate (odom: at its odometry pose).  With `floor`
  // each keyframe's floor is detected where its cloud lies (floor_params, with the grid's up axis and sensor_height) and decides
  // what is an obstacle; a status other than OK falls back to (up axis, sensor_height).  params_out: the parameters in force.
  bool occupancyGrid(std::vector<int8_t> &values, std::vector<uint32_t> &counts, lslam_occ_params &params_out, bool odom = false,
                     bool floor = true) {
    if (!occupancy || !store) { _err = "Graph: occupancy needs the option on and a resident graph"; return false; }
    if (keyframes.empty()) { _err = "Graph::occupancyGrid: no keyframes"; return false; }
    std::vector<int32_t> ids;
    std::vector<float> poses(16 * keyframes.size());
    for (size_t k = 0; k < keyframes.size(); ++k) {
      if (keyframes[k]->store != store->handle()) { _err = "Graph::occupancyGrid: every keyframe must be in the graph's store"; return false; }
      to_float16(odom ? keyframes[k]->odom : keyframes[k]->estimate, &poses[16 * k]);
      ids.push_back(keyframes[k]->store_id);
    }
    lslam_occ_params p = occupancy_params;
    std::vector<double> planes;
    std::vector<int32_t> valid;
    bool good = (p.width > 0 && p.height > 0) || store->occFitBounds(poses, p);
    if (good && floor) {
      lslam_floor_params fp = floor_params;
      fp.up[0] = 0.0f, fp.up[1] = p.up_axis == 1 ? 1.0f : 0.0f, fp.up[2] = p.up_axis == 1 ? 0.0f : 1.0f;
      fp.sensor_height = p.sensor_height;
      std::vector<lslam_floor_result> res;
      good = store->floorDetect(ids, &fp, res);
      for (size_t k = 0; good && k < res.size(); ++k) {
        valid.push_back(res[k].status == LSLAM_FLOOR_OK ? 1 : 0);
        for (int e = 0; e < 4; ++e) planes.push_back(valid.back() ? res[k].plane[e] : 0.0);
      }
    }
    good = good && store->occSetup(p) && store->occClear() && store->occIntegrate(ids, poses, planes, valid) &&
           store->occValues(values) && store->occCounts(counts);
    if (!good) { _err = store->lastError(); return false; }
    params_out = p;
    return true;
  }
  std::vector<std::pair<size_t, size_t>> removedPoints;
  double floor_sigma_normal = 0.0, floor_sigma_distance = 0.0;
  lslam_floor_params floor_params;
  std::string floor_robust_kernel = "NONE";
  double floor_robust_kernel_size = 1.0;
  double floor_world_plane[4] = {0.0, 0.0, 1.0, 0.0};
  std::vector<KeyFrame::Ptr> floors;           // the keyframes whose floor became a plane prior, in plane-prior order
  std::vector<KeyFrame::Ptr> floorsNotFound;   // ... and those whose floor was not found (KeyFrame::floor_status says why)
  const std::vector<double> &floorWeights() const { return _floor_weights; }
  std::vector<KeyFrame::Ptr> rejectedFloors(double threshold = 0.1) const {
    std::vector<KeyFrame::Ptr> out;
    for (size_t k = 0; k < floors.size() && k < _floor_weights.size(); ++k)
      if (_floor_weights[k] < threshold) out.push_back(floors[k]);
    return out;
  }
  size_t numPlanePriors() const { return _qv.size(); }
  // The diagonal of every odometry edge's information over [translation, rotation]; the reference's constant (graph.cpp:279-288)
  // unless the caller knows its odometry better.
  double odometry_information[6] = {0.8, 0.4, 0.8, 1.0, 2.0, 1.0};
  double gps_sigma_xy = 0.0, gps_sigma_z = 0.0;
  std::string gps_robust_kernel = "NONE";
  double gps_robust_kernel_size = 1.0;
  double gps_min_spread = 0.0;
  double imu_orientation_sigma = 0.0;
  bool gps_aligned = false;
  bool has_utm_origin = false;
  double utm_origin[3] = {0.0, 0.0, 0.0};
  // the keyframe of every GPS prior in the solver; its robust weight after the last optimisation (all 1 without a kernel);
  // the keyframes whose fix has a weight below `threshold` (reporting only: nothing is removed)
  std::vector<KeyFrame::Ptr> gps_fixes;
  const std::vector<double> &gpsWeights() const { return _gps_weights; }
  std::vector<KeyFrame::Ptr> rejectedFixes(double threshold = 0.1) const {
    std::vector<KeyFrame::Ptr> out;
    for (size_t k = 0; k < gps_fixes.size() && k < _gps_weights.size(); ++k)
      if (_gps_weights[k] < threshold) out.push_back(gps_fixes[k]);
    return out;
  }
  size_t numPriors() const { return _pv.size(); }
  // the second singular value of the centred fix positions of the keyframes in the graph [m]: 0 on a line
  double gpsSpread() const {
    double S[18] = {0.0};
    for (const auto &kf : keyframes)
      if (kf->has_gps_local) accumulate_pair(S, kf->gps_local, kf->gps_local);
    if (S[0] < 3.0) return 0.0;
    double R[9], t[3], W[3];
    if (lslam_debug_icp_fit(S, R, t, W, nullptr) < 0) return 0.0;
    return std::sqrt(W[1] > 0.0 ? W[1] : 0.0);  // F^T F of the centred fixes F: its singular values are those of F, squared
  }
  // Mean map entropy and mean plane variance (lslam_mapq_*; not in the reference) of the keyframes' clouds of one type (which:
  // 0 corner, 1 surf) put together at their poses -- odom = false: the optimised estimates; true: the odometry poses they started
  // from -- so the two calls score what the optimisation did to the MAP, without ground truth: lower is crisper.  A resident
  // graph evaluates the clouds where they lie in the store; a host graph moves them on the host by the same fp32 formula and
  // uploads.  which_keyframes == nullptr: `keyframes`.  params == nullptr: the defaults.
  bool mapQuality(bool odom, int which, const lslam_mapq_params *params, lslam_mapq_stats &stats,
                  const std::vector<KeyFrame::Ptr> *which_keyframes = nullptr) {
    const std::vector<KeyFrame::Ptr> &every = which_keyframes ? *which_keyframes : keyframes;
    if (which < 0 || which > 1) { _err = "mapQuality: which is 0 (corner) or 1 (surf)"; return false; }
    std::vector<int32_t> ids;
    std::vector<float> poses(16 * every.size()), cloud;
    bool stored = (bool)store;
    for (size_t k = 0; k < every.size(); ++k) {
      to_float16(odom ? every[k]->odom : every[k]->estimate, &poses[16 * k]);
      stored = stored && every[k]->store == store->handle();
      ids.push_back(every[k]->store_id);
    }
    if (stored) {
      if (store->mapQuality(ids, poses, which, params, stats)) return true;
      _err = store->lastError();
      return false;
    }
    for (size_t k = 0; k < every.size(); ++k) {
      const std::vector<float> &c = which ? every[k]->surfCloud : every[k]->cornerCloud;
      const float *T = &poses[16 * k];
      for (size_t i = 0; i + 3 < c.size(); i += 4) {  // pcl::transformPointCloud, fp32
        const float x = c[i], y = c[i + 1], z = c[i + 2];
        cloud.push_back(((T[0] * x + T[1] * y) + T[2] * z) + T[3]);
        cloud.push_back(((T[4] * x + T[5] * y) + T[6] * z) + T[7]);
        cloud.push_back(((T[8] * x + T[9] * y) + T[10] * z) + T[11]);
      }
    }
    if (lslam_mapq_eval(_ctx, cloud.data(), cloud.size() / 3, 12, nullptr, 0, 0, params, &stats, nullptr, nullptr, nullptr) == LSLAM_OK)
      return true;
    _err = lslam_last_error();
    return false;
  }
  Mat4d tf_odom2graph;
  int last_iterations = 0;
  const std::string &lastError() const { return _err; }

private:
  // generateGraphTrajectoryCloud / generateOdomTrajectoryCloud + saveTrajectoryCloud
  bool save_trajectory_cloud(const std::string &path, bool odom) const {
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) return false;
    std::fprintf(f, "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity normal_x normal_y normal_z curvature\n"
                    "SIZE 4 4 4 4 4 4 4 4\nTYPE F F F F F F F F\nCOUNT 1 1 1 1 1 1 1 1\nWIDTH %zu\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\n"
                    "POINTS %zu\nDATA ascii\n", keyframes.size(), keyframes.size());
    for (size_t i = 0; i < keyframes.size(); ++i) {
      float Tf[16];
      to_float16(odom ? keyframes[i]->odom : keyframes[i]->estimate, Tf);
      double p7[7];
      mat_to_pose7(from_float16(Tf), p7);
      std::fprintf(f, "%.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", Tf[3], Tf[7], Tf[11], (float)p7[6], (float)p7[3], (float)p7[4],
                   (float)p7[5], (float)i);
    }
    return std::fclose(f) == 0;
  }
  int fail_final(lslam_fmap *fm) {
    _err = lslam_last_error();
    if (fm) lslam_fmap_destroy(fm);
    return -1;
  }
  // A stored keyframe's clouds into fm at T; with remove_dynamic through the visibility filter (voters: see remove_dynamic), the
  // points it left out appended to removedPoints when `record`.  -> the ABI's status.
  int add_stored(const KeyFrame::Ptr &kf, lslam_fmap *fm, const float T[16], bool record) {
    if (!remove_dynamic) return lslam_kfs_add_to_fmap(kf->store, kf->store_id, fm, T);
    int rc = lslam_vis_setup(kf->store, &dynamic_params);
    if (rc < 0) return rc;
    const double reach = 2.0 * (double)dynamic_params.max_range;
    std::vector<int32_t> ids;
    std::vector<float> poses;
    for (const auto &o : keyframes) {
      if (o->store != kf->store) continue;
      const double dx = o->estimate(0, 3) - kf->estimate(0, 3), dy = o->estimate(1, 3) - kf->estimate(1, 3),
                   dz = o->estimate(2, 3) - kf->estimate(2, 3);
      if (std::sqrt(dx * dx + dy * dy + dz * dz) > reach) continue;
      float P[16];
      to_float16(o->estimate, P);
      ids.push_back(o->store_id);
      poses.insert(poses.end(), P, P + 16);
    }
    size_t removed[2] = {0, 0};
    rc = lslam_vis_add_to_fmap(kf->store, kf->store_id, fm, T, (int32_t)ids.size(), ids.data(), poses.data(), removed);
    if (rc >= 0 && record) removedPoints.push_back(std::make_pair(removed[0], removed[1]));
    return rc;
  }
  static void accumulate_pair(double S[18], const double s[3], const double t[3]) {  // lslam_debug_icp_fit's sums
    S[0] += 1.0;
    for (int r = 0; r < 3; ++r) {
      S[2 + r] += s[r];
      S[5 + r] += t[r];
      for (int c = 0; c < 3; ++c) S[8 + r * 3 + c] += s[r] * t[c];
    }
  }
  // The priors of a pass's new keyframes: queued until the fixes span a plane, then added -- all of them, after the graph frame
  // has been moved onto the fixes.  -> whether any prior reached the solver.
  bool add_priors(const std::vector<KeyFrame::Ptr> &fresh, int gps_kind) {
    const bool gps = gps_sigma_xy > 0.0, imu = imu_orientation_sigma > 0.0;
    if (!gps && !imu) return false;
    for (const auto &kf : fresh) {
      if (gps && kf->has_utm_coord) {
        if (!has_utm_origin) {
          has_utm_origin = true;
          for (int k = 0; k < 3; ++k) utm_origin[k] = kf->utm_coord[k];
        }
        kf->has_gps_local = true;
        for (int k = 0; k < 3; ++k) kf->gps_local[k] = kf->utm_coord[k] - utm_origin[k];  // fp64, before anything reaches the solver
      }
      if (kf->has_gps_local || (imu && kf->has_imu_quat)) _prior_queue.push_back(kf);
    }
    if (gps && !gps_aligned && !align_to_fixes()) return false;
    bool added = false;
    for (const auto &kf : _prior_queue) {
      if (kf->has_gps_local) {
        double w[36] = {0.0};
        w[0] = w[7] = 1.0 / (gps_sigma_xy * gps_sigma_xy);
        w[14] = 1.0 / (gps_sigma_z * gps_sigma_z);
        const double z[7] = {kf->gps_local[0], kf->gps_local[1], kf->gps_local[2], 0.0, 0.0, 0.0, 1.0};
        _gps_priors.push_back((int)_pv.size());
        gps_fixes.push_back(kf);
        add_prior(kf->node, LSLAM_PG_PRIOR_XYZ, z, w, gps_kind, gps_robust_kernel_size);
        added = true;
      }
      if (imu && kf->has_imu_quat) {
        const double *q = kf->imu_quat;
        const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        const double z[7] = {0.0, 0.0, 0.0, q[0] / n, q[1] / n, q[2] / n, q[3] / n};
        double w[36] = {0.0};
        w[21] = w[28] = w[35] = (2.0 / imu_orientation_sigma) * (2.0 / imu_orientation_sigma);
        add_prior(kf->node, LSLAM_PG_PRIOR_POSE, z, w, LSLAM_PG_KERNEL_NONE, 1.0);
        added = true;
      }
    }
    _prior_queue.clear();
    return added;
  }
  // The floors of a pass's new keyframes: detected in one call over the store (resident) or per cloud; the accepted ones become
  // plane priors.  -> false on a backend error; *added: whether any reached the solver.
  bool add_floors(const std::vector<KeyFrame::Ptr> &fresh, int floor_kind, bool *added) {
    *added = false;
    if (!(floor_sigma_normal > 0.0) || fresh.empty()) return true;
    std::vector<lslam_floor_result> res(fresh.size());
    if (store) {
      std::vector<int32_t> ids;
      for (const auto &kf : fresh) ids.push_back(kf->store_id);
      if (!store->floorDetect(ids, &floor_params, res)) {
        _err = store->lastError();
        return false;
      }
    } else {
      for (size_t k = 0; k < fresh.size(); ++k)
        if (lslam_floor_detect(_ctx, fresh[k]->surfCloud.data(), fresh[k]->surfCloud.size() / 4, 16, &floor_params, &res[k]) < 0) {
          _err = lslam_last_error();
          return false;
        }
    }
    const double wn = 1.0 / (floor_sigma_normal * floor_sigma_normal), wd = 1.0 / (floor_sigma_distance * floor_sigma_distance);
    for (size_t k = 0; k < fresh.size(); ++k) {
      const KeyFrame::Ptr &kf = fresh[k];
      kf->floor_status = res[k].status;
      if (res[k].status != LSLAM_FLOOR_OK) {
        floorsNotFound.push_back(kf);
        continue;
      }
      kf->has_floor_coeffs = true;
      for (int c = 0; c < 4; ++c) kf->floor_coeffs[c] = res[k].plane[c];
      _qv.push_back(kf->node);
      _qworld.insert(_qworld.end(), floor_world_plane, floor_world_plane + 4);
      _qmeas.insert(_qmeas.end(), kf->floor_coeffs, kf->floor_coeffs + 4);
      const double w[9] = {wn, 0.0, 0.0, 0.0, wn, 0.0, 0.0, 0.0, wd};
      _qinfo.insert(_qinfo.end(), w, w + 9);
      _qkind.push_back(floor_kind);
      _qdelta.push_back(floor_robust_kernel_size);
      floors.push_back(kf);
      *added = true;
    }
    return true;
  }
  void add_prior(int v, int type, const double z[7], const double w[36], int kind, double delta) {
    _pv.push_back(v);
    _ptype.push_back(type);
    _pmeas.insert(_pmeas.end(), z, z + 7);
    _pinfo.insert(_pinfo.end(), w, w + 36);
    _pkind.push_back(kind);
    _pdelta.push_back(delta);
  }
  // Once the fixes span a plane: the rigid fit of the keyframes' estimate positions to their fixes moves every estimate and
  // tf_odom2graph, and no vertex is fixed from here on.  -> whether that has happened.
  bool align_to_fixes() {
    const double need = gps_min_spread > 0.0 ? gps_min_spread : 10.0 * gps_sigma_xy;
    if (!(gpsSpread() >= need)) return false;
    double S[18] = {0.0};
    for (const auto &kf : keyframes)
      if (kf->has_gps_local) {
        const double s[3] = {kf->estimate(0, 3), kf->estimate(1, 3), kf->estimate(2, 3)};
        accumulate_pair(S, s, kf->gps_local);
      }
    double R[9], t[3], W[3];
    if (lslam_debug_icp_fit(S, R, t, W, nullptr) < 0) return false;
    Mat4d T;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) T.m[r * 4 + c] = R[r * 3 + c];
      T.m[r * 4 + 3] = t[r];
    }
    for (auto &kf : keyframes) {
      kf->estimate = T * kf->estimate;
      mat_to_pose7(kf->estimate, &_poses[7 * (size_t)kf->node]);
    }
    tf_odom2graph = T * tf_odom2graph;
    gps_aligned = true;
    return true;
  }
  // graph.cpp:248-297
  bool flush_keyframe_queue() {
    if (keyframe_queue.empty()) return false;
    const Mat4d odom2map = tf_odom2graph;
    const int n = std::min<int>((int)keyframe_queue.size(), _max_per_update);
    const double *ODOM_INFO = odometry_information;  // graph.cpp:279-288 by default
    for (int i = 0; i < n; ++i) {
      KeyFrame::Ptr kf = keyframe_queue[(size_t)i];
      new_keyframes.push_back(kf);
      kf->estimate = odom2map * kf->odom;
      double p7[7];
      mat_to_pose7(kf->estimate, p7);
      kf->node = (int)(_poses.size() / 7);
      _poses.insert(_poses.end(), p7, p7 + 7);
      if (i == 0 && keyframes.empty()) continue;
      const KeyFrame::Ptr &prev = i == 0 ? keyframes.back() : keyframe_queue[(size_t)i - 1];
      const Mat4d relative = inverse(prev->odom) * kf->odom;
      double full[36];
      const bool hessian = edge_information == "hessian";
      if (hessian) {  // the previous keyframe is the reference, the edge's measurement the pose
        static const float EYE[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        if (!hessian_information(ODOM_INFO, std::vector<int32_t>(1, prev->store_id), std::vector<float>(EYE, EYE + 16), kf->store_id,
                                 relative, full))
          _edge_failed = true;
      }
      add_edge(prev->node, kf->node, relative, ODOM_INFO, LSLAM_PG_KERNEL_NONE, 1.0, hessian && !_edge_failed ? full : nullptr);
    }
    keyframe_queue.erase(keyframe_queue.begin(), keyframe_queue.begin() + n);
    return true;
  }
  // the graph as it stands through the solver: kernels on, [save,] optimise, [save,] estimates and loop weights back --
  // optimize() and save() share it
  bool solve_graph(int max_iterations, const char *g2o_before, const char *g2o_end) {
    lslam_pg *pg = nullptr;
    if (lslam_pg_create(_device, (int)(_poses.size() / 7), _poses.data(), (int)(_ij.size() / 2), _ij.data(), _meas.data(), _info.data(),
                        gps_aligned ? -1 : 0, &pg) != LSLAM_OK) {  // (aligned: the priors hold the gauge, no vertex is fixed)
      _err = lslam_pg_last_error();
      return false;
    }
    lslam_pg_stats st;
    int rc = apply_kernels(pg);
    if (rc >= 0 && !_pv.empty()) {
      bool any = false;
      for (size_t p = 0; p < _pkind.size(); ++p) any = any || _pkind[p] != LSLAM_PG_KERNEL_NONE;
      rc = lslam_pg_set_priors(pg, (int32_t)_pv.size(), _pv.data(), _ptype.data(), _pmeas.data(), _pinfo.data(),
                               any ? _pkind.data() : nullptr, any ? _pdelta.data() : nullptr);
    }
    if (rc >= 0 && !_qv.empty()) {
      bool any = false;
      for (size_t p = 0; p < _qkind.size(); ++p) any = any || _qkind[p] != LSLAM_PG_KERNEL_NONE;
      rc = lslam_pg_set_plane_priors(pg, (int32_t)_qv.size(), _qv.data(), _qworld.data(), _qmeas.data(), _qinfo.data(),
                                     any ? _qkind.data() : nullptr, any ? _qdelta.data() : nullptr);
    }
    if (rc >= 0 && g2o_before) rc = lslam_pg_save_g2o(pg, g2o_before);
    if (rc >= 0) rc = lslam_pg_optimize(pg, max_iterations, &st);
    if (rc >= 0 && g2o_end) rc = lslam_pg_save_g2o(pg, g2o_end);
    if (rc >= 0) rc = lslam_pg_get_poses(pg, _poses.data());
    if (rc >= 0) rc = read_loop_weights(pg);
    if (rc >= 0 && !_pv.empty()) {
      std::vector<double> w(_pv.size());
      rc = lslam_pg_prior_robust(pg, nullptr, nullptr, nullptr, w.data());
      _gps_weights.clear();
      for (size_t k = 0; rc >= 0 && k < _gps_priors.size(); ++k) _gps_weights.push_back(w[(size_t)_gps_priors[k]]);
    }
    if (rc >= 0 && !_qv.empty()) {
      _floor_weights.assign(_qv.size(), 1.0);
      rc = lslam_pg_plane_prior_robust(pg, nullptr, nullptr, nullptr, _floor_weights.data());
    }
    lslam_pg_destroy(pg);
    if (rc < 0) {
      _err = lslam_pg_last_error();
      return false;
    }
    last_iterations = st.iterations;
    for (auto &kf : keyframes) kf->estimate = pose7_to_mat(&_poses[7 * (size_t)kf->node]);
    return true;
  }
  // the graph as it stands as a solver graph (kernels, priors, plane priors), for the covariance calls; null with _err set
  lslam_pg *make_pg() {
    lslam_pg *pg = nullptr;
    if (lslam_pg_create(_device, (int)(_poses.size() / 7), _poses.data(), (int)(_ij.size() / 2), _ij.data(), _meas.data(), _info.data(),
                        gps_aligned ? -1 : 0, &pg) != LSLAM_OK) {
      _err = lslam_pg_last_error();
      return nullptr;
    }
    int rc = apply_kernels(pg);
    if (rc >= 0 && !_pv.empty()) {
      bool any = false;
      for (size_t p = 0; p < _pkind.size(); ++p) any = any || _pkind[p] != LSLAM_PG_KERNEL_NONE;
      rc = lslam_pg_set_priors(pg, (int32_t)_pv.size(), _pv.data(), _ptype.data(), _pmeas.data(), _pinfo.data(),
                               any ? _pkind.data() : nullptr, any ? _pdelta.data() : nullptr);
    }
    if (rc >= 0 && !_qv.empty()) {
      bool any = false;
      for (size_t p = 0; p < _qkind.size(); ++p) any = any || _qkind[p] != LSLAM_PG_KERNEL_NONE;
      rc = lslam_pg_set_plane_priors(pg, (int32_t)_qv.size(), _qv.data(), _qworld.data(), _qmeas.data(), _qinfo.data(),
                                     any ? _qkind.data() : nullptr, any ? _qdelta.data() : nullptr);
    }
    if (rc < 0) {
      _err = lslam_pg_last_error();
      lslam_pg_destroy(pg);
      return nullptr;
    }
    return pg;
  }
  bool loop_consistency(lslam_pg *pg, const KeyFrame::Ptr &key1, const KeyFrame::Ptr &key2, const Mat4d &relative_pose, double *d2) {
    static const double LOOP_INFO[6] = {2, 2, 2, 2, 2, 2};
    double s_rel[36];
    const int32_t j = key2->node;
    if (lslam_pg_relative_covariances(pg, key1->node, 1, &j, &covariance_opts, s_rel, nullptr) < 0) {
      _err = lslam_pg_last_error();
      return false;
    }
    if (!loop_mahalanobis(key1->estimate, key2->estimate, relative_pose, s_rel, LOOP_INFO, d2)) {
      _err = "Graph: the loop's covariance is singular";
      return false;
    }
    return true;
  }
  std::vector<Loop::Ptr> _inconsistent;
  int apply_kernels(lslam_pg *pg) {
    bool any = false;
    for (size_t e = 0; e < _kind.size(); ++e) any = any || _kind[e] != LSLAM_PG_KERNEL_NONE;
    return any ? lslam_pg_set_robust_kernels(pg, _kind.data(), _delta.data()) : LSLAM_OK;
  }
  int read_loop_weights(lslam_pg *pg) {
    std::vector<double> w(_ij.size() / 2);
    const int rc = lslam_pg_edge_robust(pg, nullptr, nullptr, nullptr, w.data());
    if (rc < 0) return rc;
    _loop_weights.clear();
    for (size_t k = 0; k < _loop_edges.size(); ++k) _loop_weights.push_back(w[(size_t)_loop_edges[k]]);
    return LSLAM_OK;
  }
  // One edge's information under edge_information = "hessian" (the formula at that member; sums that are not finite -- a scan
  // point exactly on its line is a 0 / 0 in the reference's coefficient -- count as no match); its lslam_edge_info is kept.
  bool hessian_information(const double diag_ref[6], const std::vector<int32_t> &ref_ids, const std::vector<float> &rel_T, int new_id,
                           const Mat4d &T, double out[36]) {
    float Tf[16];
    to_float16(T, Tf);
    lslam_edge_info ei;
    if (lslam_keyframe_edge_information(store->handle(), (int32_t)ref_ids.size(), ref_ids.data(), rel_T.data(), new_id, Tf, 0.2f, 0.4f, 0.2f,
                                   0.4f, &ei) < 0) {
      _err = lslam_last_error();
      return false;
    }
    _edge_infos.push_back(ei);
    bool use = ei.n_rows >= 50 && std::isfinite(ei.sum_b2);
    for (int k = 0; k < 36; ++k) use = use && std::isfinite(ei.H[k]);
    const double s2 = use ? std::max(ei.sum_b2 / (double)(ei.n_rows - 6), range_sigma * range_sigma) : 1.0;
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) {
        const double ref = r == c ? diag_ref[r] : 0.0;
        out[r * 6 + c] = use ? ref + ei.H[r * 6 + c] / s2 : ref;
      }
    return true;
  }
  void add_edge(int a, int b, const Mat4d &rel, const double diag_info[6], int kind = LSLAM_PG_KERNEL_NONE, double delta = 1.0,
                const double *full_info = nullptr) {
    _kind.push_back(kind);
    _delta.push_back(delta);
    _ij.push_back(a);
    _ij.push_back(b);
    double p7[7];
    mat_to_pose7(rel, p7);
    _meas.insert(_meas.end(), p7, p7 + 7);
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) _info.push_back(full_info ? full_info[r * 6 + c] : (r == c ? diag_info[r] : 0.0));
  }
  lslam_ctx *_ctx;
  int _device, _max_per_update;
  bool _keep_host, _appearance;
  std::vector<double> _poses, _meas, _info;
  std::vector<int32_t> _ij;
  std::vector<int32_t> _kind;  // per edge: LSLAM_PG_KERNEL_* and its delta
  std::vector<double> _delta;
  std::vector<int> _loop_edges;  // edge index of every entry of `loops`
  std::vector<double> _loop_weights;
  std::vector<lslam_edge_info> _edge_infos;
  bool _edge_failed = false;
  // unary constraints: vertex, LSLAM_PG_PRIOR_*, measurement, information, kernel; the keyframes whose priors wait for the
  // alignment; the prior index of every entry of gps_fixes and its weight
  std::vector<int32_t> _pv, _ptype, _pkind;
  std::vector<double> _pmeas, _pinfo, _pdelta;
  std::vector<KeyFrame::Ptr> _prior_queue;
  std::vector<int> _gps_priors;
  std::vector<double> _gps_weights;
  // plane priors: vertex, world plane, measured plane, 3x3 information, kernel; the weight of every entry of `floors`
  std::vector<int32_t> _qv, _qkind;
  std::vector<double> _qworld, _qmeas, _qinfo, _qdelta, _floor_weights;
  std::string _err;
};

}  // namespace pose_graph
