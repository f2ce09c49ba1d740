// lslam_kfs_impl.hpp -- the keyframe store's state, shared by the files that implement lslam_kfs_* entry points: lslam_kfs.hip
// (the clouds and the pose-graph steps that read them) and lslam_sc.hip (the scan-context descriptors over them).  Host side only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdio>
#include <memory>
#include <vector>

#include "lslam_internal.hpp"

namespace lslam {

struct Slab {
  DevBuf<float4> buf;
  size_t used = 0;
};
struct KeyframeClouds {
  float4 *p[2];
  size_t n[2];
  float lo[2][3], hi[2][3];  // getMinMax3D of each cloud (not read for an empty one)
};

// What the describe kernel reads per keyframe (uploaded for the keyframes that have no descriptor yet)
struct ScJob {
  const float4 *p[2];
  uint32_t n[2];
};

// Scan-context state of a store (lslam_sc_*, lslam_sc.hip).  Empty -- no allocation -- until lslam_sc_setup.
// Keyframe i's record lives in slab i / SC_SLAB_KEYFRAMES at (i % SC_SLAB_KEYFRAMES) * stride floats: the raw maxima D[ring][sector],
// then the query form -- the columns divided by their norms, [ring][sector], and one more row of 1.0 / 0.0: the column's norm is > 0.
// A slab is never moved or freed before drop(), so records stay where the describe kernel wrote them.
struct ScState {
  static constexpr size_t SC_SLAB_KEYFRAMES = 1024;
  bool set = false;
  lslam_sc_params params{};
  float ring_scale = 0.0f;      // (float)n_ring / max_range
  double sector_scale = 0.0;    // n_sector / (2 pi)
  size_t stride = 0;            // floats per keyframe record: (2 * n_ring + 1) * n_sector
  size_t described = 0;         // keyframes 0 .. described-1 have their record
  std::vector<std::unique_ptr<DevBuf<float>>> slabs;
  DevBuf<float *> d_slabs;      // the slabs' base pointers, for the kernels
  size_t slabs_uploaded = 0;
  PinBuf<ScJob> h_jobs;
  DevBuf<ScJob> d_jobs;
  // a query call's scratch: ids and limits up, tile lists, the merged lists down
  PinBuf<int32_t> h_io;
  DevBuf<int32_t> d_in, d_out, d_tile_shift;
  DevBuf<uint64_t> d_tile_key;
  DevBuf<float> d_tap;
  int64_t describe_launches = 0, query_launches = 0;

  size_t bytes_held() const {
    size_t b = 0;
    for (const auto &s : slabs) b += s->cap * sizeof(float);
    return b;
  }
  // the descriptors go (their slabs are freed); parameters, scratch and counters stay.  The caller has waited for the stream.
  void drop() {
    slabs.clear();
    slabs_uploaded = 0;
    described = 0;
  }
};

// Floor detection (lslam_floor.hip): what its kernels read per cloud of a call, what the host reads back per cloud, and the
// scratch of a call.  A context owns one (CTX_SLOT_FLOOR: the single-cloud entry points), a store owns one
// (lslam_floor_detect_keyframes); each is freed with its owner.
constexpr int FLOOR_NSUM = 11;
struct FloorJob {
  const float4 *pts;
  uint32_t n;
  uint32_t cand_base;  // the cloud's slice of d_cand_idx / d_cand_pts: [cand_base, cand_base + n)
  uint32_t tile_base;  // ... of the per-tile arrays: its ceil(n / 1024) tiles
  uint32_t pad;
};
struct FloorOut {
  int32_t K, best, best_count, pad;
  double sums[FLOOR_NSUM];
};
struct FloorPlane {
  float4 p32;     // the plane the inlier test reads
  double p64[4];  // ... and the one distances are taken from
};
struct FloorScratch {
  PinBuf<FloorJob> h_jobs;
  DevBuf<FloorJob> d_jobs;
  DevBuf<int32_t> d_tile_cnt, d_tile_off, d_cand_idx, d_triples, d_hstat, d_counts;
  DevBuf<float4> d_cand_pts, d_planes, d_cloud;
  PinBuf<float4> h_cloud;  // staging of lslam_floor_detect's host cloud
  DevBuf<double> d_partials;
  DevBuf<FloorOut> d_out;
  PinBuf<FloorOut> h_out;
  DevBuf<FloorPlane> d_cur;
  PinBuf<FloorPlane> h_cur;
  bool tap_valid = false;  // the lists of the last call's first cloud are there (lslam_debug_floor_hypotheses)
  int32_t tap_K = 0, tap_H = 0;
  // the shape of the last call's scoring launch, and a second set of counters (lslam_debug_floor_score: the kernel alone, timed)
  int32_t last_clouds = 0, last_H = 0;
  uint32_t last_tiles = 0;
  float last_thr = 0.0f;
  DevBuf<int32_t> d_counts_again;
};

// Visibility votes (lslam_vis_*, lslam_vis.hip): a coarse range image per keyframe and the scratch of a vote / filter call.
// Empty -- no allocation -- until lslam_vis_setup.  Keyframe i's image (n_row * n_col floats) lives in slab i / slab_kf at
// (i % slab_kf) * stride floats; a slab is never moved or freed before drop(), so images stay where they were built.
struct VisJob {
  const float4 *p[2];
  uint32_t n[2];
  float *img;
};
struct VisState {
  bool set = false;
  lslam_vis_params params{};
  double el0 = 0.0, row_scale = 0.0, col_scale = 0.0;  // fov_down in rad, n_row / fov in rad, n_col / (2 pi): fp64, host
  size_t stride = 0;    // floats per image
  size_t slab_kf = 0;   // images per slab
  size_t imaged = 0;    // keyframes 0 .. imaged-1 have their image
  std::vector<std::unique_ptr<DevBuf<float>>> slabs;
  PinBuf<VisJob> h_jobs;
  DevBuf<VisJob> d_jobs;
  // a call's scratch: per voter {image, inverse pose} up, the query points, the votes, the compaction's counts
  PinBuf<float> h_in;
  DevBuf<float> d_inv;
  DevBuf<const float *> d_img;
  PinBuf<const float *> h_img;
  DevBuf<float4> d_pts, d_keep[2];
  PinBuf<float4> h_pts;
  DevBuf<uint32_t> d_votes, d_votes_again, d_block;
  PinBuf<uint32_t> h_votes, h_count;
  int64_t image_launches = 0, vote_launches = 0;
  // the shape of the last lslam_vis_votes call (lslam_debug_vis_votes: the vote kernel alone, timed)
  size_t last_n = 0;
  int32_t last_ids = 0;

  float *image(size_t id) const { return slabs[id / slab_kf]->p + (id % slab_kf) * stride; }
  size_t bytes_held() const {
    size_t b = 0;
    for (const auto &s : slabs) b += s->cap * sizeof(float);
    return b;
  }
  // the images go (their slabs are freed); parameters, scratch and counters stay.  The caller has waited for the stream.
  void drop() {
    slabs.clear();
    imaged = 0;
    last_n = 0;
    last_ids = 0;
  }
};

// Occupancy grid (lslam_occ_*, lslam_occ.hip): the counts and values of one grid and the scratch of an integration.  Empty -- no
// allocation -- until lslam_occ_setup; the grid itself is allocated (zeroed) by the first call that needs it.
struct OccJob {  // what the ray and merge kernels read per keyframe of a call
  const float4 *p[2];
  uint32_t n[2];
  float T[12];       // the pose's first three rows
  float plane[4];
  int32_t ax, ay;    // the ray origin in fixed point (read only when a_ok)
  int32_t a_ok;      // 0: the origin lies outside the fixed-point range, every ray of the keyframe is dropped
  int32_t wi0, wj0;  // the window's first cell ...
  int32_t ww, wh;    // ... and its size in cells (0 x 0: the keyframe cannot touch the grid)
  uint32_t words;    // uint32 per bit plane: ceil(ww * wh / 32)
  uint64_t plane_at; // the HIT plane's first word in the chunk's scratch; the FREE plane follows it
};
struct OccState {
  bool set = false;
  lslam_occ_params params{};
  double scale = 0.0;  // 256 / resolution: fp64, host
  int32_t n_integrated = 0;
  bool values_stale = true;
  DevBuf<uint32_t> d_counts;
  DevBuf<int8_t> d_values;
  // an integration's scratch: the jobs up, the bit planes of one chunk, the four ray counters
  PinBuf<OccJob> h_jobs;
  DevBuf<OccJob> d_jobs;
  DevBuf<uint32_t> d_planes, d_planes_again;
  DevBuf<unsigned long long> d_stats, d_stats_again;  // [1] dropped, [2] obstacle, [3] ground, [4] cells outside their window
  PinBuf<unsigned long long> h_stats;
  int64_t rays[4] = {0, 0, 0, 0};  // cast, dropped, obstacle, ground since the last clear
  int64_t ray_launches = 0, merge_launches = 0, value_launches = 0;
  int32_t last_ids = 0;  // the jobs of the last integration are in d_jobs (lslam_debug_occ_integrate)

  size_t cells() const { return (size_t)params.width * (size_t)params.height; }
  bool held() const { return d_counts.p != nullptr; }
  size_t grid_bytes() const { return d_counts.cap * sizeof(uint32_t) + d_values.cap; }
  size_t scratch_bytes() const { return (d_planes.cap + d_planes_again.cap) * sizeof(uint32_t); }
  void zero_tallies() {
    n_integrated = 0;
    values_stale = true;
    rays[0] = rays[1] = rays[2] = rays[3] = 0;
  }
  // the grid and its scratch go; parameters and launch counters stay.  The caller has waited for the stream.
  void drop() {
    d_counts.release();
    d_values.release();
    d_planes.release();
    d_planes_again.release();
    zero_tallies();
    last_ids = 0;
  }
};

}  // namespace lslam

struct lslam_kfs {
  lslam_ctx *ctx = nullptr;
  hipStream_t stream = nullptr;
  size_t max_points = 0, slab_points = 0;
  int32_t max_keyframes = 0;
  std::vector<std::unique_ptr<lslam::Slab>> slabs;
  std::vector<lslam::KeyframeClouds> kfs;
  size_t total[2] = {0, 0};
  size_t held_points = 0;
  uint64_t bytes_up = 0, bytes_down = 0;
  lslam::PinBuf<float4> h_stage;
  lslam::DevBuf<uint32_t> d_box;  // [12] grid_bbox2's scratch
  // loop match: the assembled clouds, their {x, y, z, index} forms, the four filtered clouds
  lslam::DevBuf<float4> local[2], indexed[2], filt[4];
  size_t n_local[2] = {0, 0};
  lslam::ScState sc;
  lslam::FloorScratch floor;
  lslam::VisState vis;
  lslam::OccState occ;
};

namespace lslam {

inline int check_kfs(lslam_kfs *k, const char *what) {
  if (!k) {
    char b[160];
    snprintf(b, sizeof(b), "%s: null keyframe store", what);
    set_error(b);
    return LSLAM_ERR_INVALID;
  }
  if (!ctx_alive(k->ctx)) {
    set_error("keyframe store: its ctx was destroyed");
    return LSLAM_ERR_INVALID;
  }
  LSLAM_TRY(hipSetDevice(ctx_device(k->ctx)));
  return LSLAM_OK;
}

// lslam_kfs.hip: the named keyframes' clouds of one type, each moved by its pose, as one device cloud (lslam_mapq_keyframes)
int kfs_gather_posed(lslam_kfs *k, int32_t n_ids, const int32_t *ids, const float *poses16, int which, DevBuf<float4> &out, size_t *total_out);

inline int check_id(const lslam_kfs *k, const char *what, int32_t id) {
  if (id < 0 || (size_t)id >= k->kfs.size()) {
    char b[200];
    snprintf(b, sizeof(b), "%s: keyframe id %d out of range (the store holds %zu)", what, id, k->kfs.size());
    set_error(b);
    return LSLAM_ERR_INVALID;
  }
  return LSLAM_OK;
}

}  // namespace lslam
