// lslam_kfs.hip -- the keyframe store: the corner and surface clouds of pose_graph::Graph's keyframes (pose_graph/keyframe.h)
// in HBM, and the steps of the pose-graph node that read them there -- LoopDetector::matching_nearest
// (pose_graph/loop_detector.hpp:166-255) and Graph::getFinalFeatureMap's per-keyframe work (pose_graph/graph.cpp:150-199).
//
// Layout: slabs of float4 {x, y, z, intensity}, each a DevBuf of its own.  A cloud is placed behind the last cloud of the
// newest slab when it fits there, otherwise in a new slab; a cloud larger than a slab gets a slab of exactly its size.  A cloud
// never straddles slabs and a slab is never moved or freed before clear / destroy, so the device pointers lslam_kfs_view hands
// out stay valid and growing the store copies nothing.  The host keeps the table {pointer, count, bounding box} per keyframe
// and type; ids are 0, 1, 2, ... in order of insertion (the order of the reference's `keyframes` vector).
//
// No new arithmetic: the consumers run the kernels of the host-pointer entry points (lslam_icp_align, lslam_voxel_grid,
// lslam_map_set + lslam_scanmatch_scan, lslam_fmap_add_feature_cloud) in their order through the device-input forms of
// lslam_internal.hpp; what is new is kfs_gather_kernel, the candidates' clouds in the frame of the first candidate.
#include "../../include/lslam_c.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "lslam_internal.hpp"
#include "lslam_kfs_impl.hpp"

namespace {

constexpr size_t KFS_DEFAULT_SLAB = (size_t)1 << 20;     // 16 MiB: ~300 VLP-16 keyframes' surface clouds
constexpr size_t KFS_DEFAULT_POINTS = (size_t)1 << 26;   // per type: 1 GiB, taken slab by slab as the store grows
constexpr size_t KFS_MAX_POINTS = (size_t)1 << 30;
constexpr int32_t KFS_DEFAULT_KEYFRAMES = 1 << 16;
constexpr int KFS_MAX_CAND = 6;  // loop_detector.hpp:141

// The candidates' clouds of one feature type as ONE cloud in candidate 0's frame (loop_detector.hpp:166-200): candidate 0's
// points as they are -- a copy of the bits, -0.0 and NaN intensities included (a product with the identity would change
// both) -- candidates 1 .. n-1 through rigid_transform_point with their rel_k, appended in candidate order.
struct GatherArgs {
  const float4 *src[KFS_MAX_CAND];
  int32_t off[KFS_MAX_CAND + 1];  // candidate k's first output point; off[n_cand]: the total
  int32_t n_cand;
  float T[KFS_MAX_CAND][12];      // rows of [R | t] (T[0] is not read)
  float4 *out;
};
__global__ __launch_bounds__(256) void kfs_gather_kernel(const GatherArgs a) {
  const int first = (int)blockIdx.x * 256;
  const int i = first + (int)threadIdx.x;
  int k = 0;  // the candidate of the workgroup's first point (uniform), then a step or two per lane where a workgroup straddles
  while (k + 1 < a.n_cand && a.off[k + 1] <= first) ++k;
  if (i >= a.off[a.n_cand]) return;
  while (a.off[k + 1] <= i) ++k;  // (i < off[n_cand]: ends at k < n_cand; empty candidates are stepped over)
  const float4 p = a.src[k][i - a.off[k]];  // one 16-byte load and store per lane, consecutive lanes consecutive points
  a.out[i] = k == 0 ? p : lslam::rigid_transform_point(a.T[k], p);
}

// {x, y, z, intensity} -> {x, y, z, bitcast(index)}: what the map set reads (lslam_map_set packs a host cloud the same way)
__global__ __launch_bounds__(256) void kfs_index_kernel(const float4 *in, int n, float4 *out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float4 p = in[i];
  p.w = __builtin_bit_cast(float, (uint32_t)i);
  out[i] = p;
}

using lslam::check_kfs;
using lslam::check_id;
using lslam::Slab;
using lslam::KeyframeClouds;

// Room for two clouds.  Nothing is committed: the caller commits (slab `used` counters) once the points are there; slabs
// opened here are dropped again by rollback().
struct Placement {
  float4 *p[2] = {nullptr, nullptr};
  size_t slab[2] = {0, 0};
  size_t slabs_before = 0;
};
int place(lslam_kfs *k, const size_t n[2], Placement *pl) {
  pl->slabs_before = k->slabs.size();
  size_t pending_used = 0;  // of the newest slab, by cloud 0 of this add
  size_t pending_slab = (size_t)-1;
  for (int t = 0; t < 2; ++t) {
    if (!n[t]) continue;
    Slab *last = k->slabs.empty() ? nullptr : k->slabs.back().get();
    const size_t last_used = last ? last->used + (pending_slab == k->slabs.size() - 1 ? pending_used : 0) : 0;
    if (n[t] <= k->slab_points && last && last->buf.cap >= k->slab_points && last_used + n[t] <= last->buf.cap) {
      pl->p[t] = last->buf.p + last_used;
      pl->slab[t] = k->slabs.size() - 1;
      pending_slab = pl->slab[t];
      pending_used = last_used - last->used + n[t];
      continue;
    }
    std::unique_ptr<Slab> s(new Slab());
    const size_t want = n[t] > k->slab_points ? n[t] : k->slab_points;
    const hipError_t e = s->buf.alloc(want);
    if (e != hipSuccess) {
      char b[200];
      snprintf(b, sizeof(b), "keyframe store: a slab of %zu points could not be allocated: %s", want, hipGetErrorString(e));
      lslam::set_error(b);
      k->slabs.resize(pl->slabs_before);
      return LSLAM_ERR_HIP;
    }
    k->slabs.push_back(std::move(s));
    pl->p[t] = k->slabs.back()->buf.p;
    pl->slab[t] = k->slabs.size() - 1;
    pending_slab = pl->slab[t];
    pending_used = n[t];
  }
  return LSLAM_OK;
}
void rollback(lslam_kfs *k, const Placement &pl) { k->slabs.resize(pl.slabs_before); }

int add_impl(lslam_kfs *k, const void *corner, size_t n_corner, const void *surf, size_t n_surf, size_t stride_bytes, bool host,
             int32_t *id_out) {
  const char *what = host ? "lslam_kfs_add" : "lslam_kfs_add_device";
  if (id_out) *id_out = -1;
  int rc = check_kfs(k, what);
  if (rc) return rc;
  if ((n_corner && !corner) || (n_surf && !surf) || (host && (stride_bytes < 16 || (stride_bytes & 3)))) {
    lslam::set_error("keyframe store add: null cloud with points, or a stride under 16 bytes");
    return LSLAM_ERR_INVALID;
  }
  const void *src[2] = {corner, surf};
  const size_t n[2] = {n_corner, n_surf};
  if (k->kfs.size() + 1 > (size_t)k->max_keyframes) {
    char b[200];
    snprintf(b, sizeof(b), "%s: the store would hold %zu keyframes, max_keyframes is %d", what, k->kfs.size() + 1, k->max_keyframes);
    lslam::set_error(b);
    return LSLAM_ERR_INVALID;
  }
  for (int t = 0; t < 2; ++t)
    if (k->total[t] + n[t] > k->max_points) {
      char b[240];
      snprintf(b, sizeof(b), "%s: the store would hold %zu %s points, max_points_per_type is %zu", what, k->total[t] + n[t],
               t ? "surf" : "corner", k->max_points);
      lslam::set_error(b);
      return LSLAM_ERR_INVALID;
    }
  hipStream_t s = k->stream;
  if (host) LSLAM_TRY(k->h_stage.reserve(n[0] + n[1]));
  Placement pl;
  rc = place(k, n, &pl);
  if (rc) return rc;
  size_t at = 0;
  hipError_t e = hipSuccess;
  for (int t = 0; t < 2 && e == hipSuccess; ++t) {
    if (!n[t]) continue;
    if (host) {
      float4 *h = k->h_stage.p + at;
      const char *p = static_cast<const char *>(src[t]);
      if (stride_bytes == 16) {
        std::memcpy(h, p, n[t] * sizeof(float4));
      } else {  // pcl::PointXYZI: {x, y, z} at 0, the intensity at byte 16 when the point has it
        for (size_t i = 0; i < n[t]; ++i) {
          float v[3], w = 0.0f;
          std::memcpy(v, p + i * stride_bytes, 12);
          if (stride_bytes >= 20) std::memcpy(&w, p + i * stride_bytes + 16, 4);
          h[i] = make_float4(v[0], v[1], v[2], w);
        }
      }
      e = hipMemcpyAsync(pl.p[t], h, n[t] * sizeof(float4), hipMemcpyHostToDevice, s);
      at += n[t];
    } else {
      e = hipMemcpyAsync(pl.p[t], src[t], n[t] * sizeof(float4), hipMemcpyDeviceToDevice, s);
    }
  }
  // both clouds' boxes behind the copies: ONE wait for the uploads and the boxes (the filters of the consumers start from them)
  KeyframeClouds kc{};
  if (e == hipSuccess) {
    const float4 *bp[2] = {pl.p[0], pl.p[1]};
    const int bn[2] = {(int)n[0], (int)n[1]};
    e = lslam::grid_bbox2(bp, bn, k->d_box.p, kc.lo, kc.hi, s);
  }
  if (e != hipSuccess) {
    char b[200];
    snprintf(b, sizeof(b), "%s: copying the clouds failed: %s", what, hipGetErrorString(e));
    lslam::set_error(b);
    (void)hipStreamSynchronize(s);
    rollback(k, pl);
    return LSLAM_ERR_HIP;
  }
  for (int t = 0; t < 2; ++t) {
    kc.p[t] = pl.p[t];
    kc.n[t] = n[t];
    if (n[t]) k->slabs[pl.slab[t]]->used += n[t];
    k->total[t] += n[t];
  }
  for (size_t i = pl.slabs_before; i < k->slabs.size(); ++i) k->held_points += k->slabs[i]->buf.cap;
  if (host) k->bytes_up += (uint64_t)(n[0] + n[1]) * sizeof(float4);
  k->kfs.push_back(kc);
  if (id_out) *id_out = (int32_t)k->kfs.size() - 1;
  return LSLAM_OK;
}

// The candidates' local clouds into k->local[0 / 1]; enqueued, not waited for.
int assemble(lslam_kfs *k, const char *what, int32_t n_cand, const int32_t *ids, const float *rel_T) {
  if (n_cand < 1 || n_cand > KFS_MAX_CAND || !ids || (n_cand > 1 && !rel_T)) {
    char b[200];
    snprintf(b, sizeof(b), "%s: between 1 and %d candidates, with their ids and transforms", what, KFS_MAX_CAND);
    lslam::set_error(b);
    return LSLAM_ERR_INVALID;
  }
  for (int c = 0; c < n_cand; ++c) {
    const int rc = check_id(k, what, ids[c]);
    if (rc) return rc;
  }
  for (int t = 0; t < 2; ++t) {
    GatherArgs a{};
    size_t total = 0;
    for (int c = 0; c < n_cand; ++c) {
      const KeyframeClouds &kc = k->kfs[(size_t)ids[c]];
      a.src[c] = kc.p[t];
      a.off[c] = (int32_t)total;
      total += kc.n[t];
      if (total > (size_t)INT32_MAX) {
        lslam::set_error("keyframe store: the candidates' clouds hold more than 2^31 points");
        return LSLAM_ERR_INVALID;
      }
      if (c) std::memcpy(a.T[c], rel_T + 16 * (size_t)c, 12 * sizeof(float));
    }
    a.off[n_cand] = (int32_t)total;
    a.n_cand = n_cand;
    k->n_local[t] = total;
    if (!total) continue;
    LSLAM_TRY(k->local[t].reserve(total));
    a.out = k->local[t].p;
    hipLaunchKernelGGL(kfs_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, k->stream, a);
    LSLAM_TRY(hipGetLastError());
  }
  return LSLAM_OK;
}

int index_cloud(lslam_kfs *k, const float4 *in, size_t n, lslam::DevBuf<float4> &out) {
  LSLAM_TRY(out.reserve(n ? n : 1));
  if (!n) return LSLAM_OK;
  hipLaunchKernelGGL(kfs_index_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, k->stream, in, (int)n, out.p);
  LSLAM_TRY(hipGetLastError());
  return LSLAM_OK;
}

}  // namespace

namespace lslam {

// The named keyframes' clouds of one type, EVERY one moved by its pose (row-major 4x4 fp32 each), appended in the order named
// into out (reserved here) -> *total points.  kfs_gather_kernel leaves its candidate 0 as it is, so each launch runs with an
// empty candidate 0 and up to KFS_MAX_CAND - 1 keyframes behind it; enqueued on the store's stream, not waited for.  The ids
// have been checked by the caller.
int kfs_gather_posed(lslam_kfs *k, int32_t n_ids, const int32_t *ids, const float *poses16, int which, DevBuf<float4> &out, size_t *total_out) {
  size_t total = 0;
  for (int32_t c = 0; c < n_ids; ++c) total += k->kfs[(size_t)ids[c]].n[which];
  *total_out = total;
  if (total > (size_t)INT32_MAX) {
    lslam::set_error("keyframe store: the named keyframes' clouds hold more than 2^31 points");
    return LSLAM_ERR_INVALID;
  }
  LSLAM_TRY(out.reserve(total ? total : 1));
  size_t base = 0;
  for (int32_t c0 = 0; c0 < n_ids; c0 += KFS_MAX_CAND - 1) {
    const int m = n_ids - c0 < KFS_MAX_CAND - 1 ? n_ids - c0 : KFS_MAX_CAND - 1;
    GatherArgs a{};
    size_t chunk = 0;
    a.src[0] = nullptr;
    a.off[0] = 0;
    for (int j = 0; j < m; ++j) {
      const KeyframeClouds &kc = k->kfs[(size_t)ids[c0 + j]];
      a.src[j + 1] = kc.p[which];
      a.off[j + 1] = (int32_t)chunk;
      chunk += kc.n[which];
      std::memcpy(a.T[j + 1], poses16 + 16 * (size_t)(c0 + j), 12 * sizeof(float));
    }
    a.off[m + 1] = (int32_t)chunk;
    a.n_cand = m + 1;
    a.out = out.p + base;
    base += chunk;
    if (!chunk) continue;
    hipLaunchKernelGGL(kfs_gather_kernel, dim3((unsigned)((chunk + 255) / 256)), dim3(256), 0, k->stream, a);
    LSLAM_TRY(hipGetLastError());
  }
  return LSLAM_OK;
}

}  // namespace lslam

extern "C" {

int lslam_kfs_create(lslam_ctx *ctx, size_t max_points_per_type, int32_t max_keyframes, size_t slab_points, lslam_kfs **out) {
  if (out) *out = nullptr;
  if (!ctx || !lslam::ctx_alive(ctx) || !out) {
    lslam::set_error("lslam_kfs_create: null ctx or null out");
    return LSLAM_ERR_INVALID;
  }
  if (max_keyframes < 0 || max_points_per_type > KFS_MAX_POINTS || slab_points > KFS_MAX_POINTS) {
    lslam::set_error("lslam_kfs_create: negative max_keyframes, or max_points_per_type / slab_points above 2^30");
    return LSLAM_ERR_INVALID;
  }
  LSLAM_TRY(hipSetDevice(lslam::ctx_device(ctx)));
  lslam_kfs *k = new lslam_kfs();
  k->ctx = ctx;
  k->stream = lslam::ctx_stream(ctx);
  k->max_points = max_points_per_type ? max_points_per_type : KFS_DEFAULT_POINTS;
  k->max_keyframes = max_keyframes ? max_keyframes : KFS_DEFAULT_KEYFRAMES;
  k->slab_points = slab_points ? slab_points : KFS_DEFAULT_SLAB;
  const hipError_t e = k->d_box.alloc(12);
  if (e != hipSuccess) {
    lslam::set_error("lslam_kfs_create: allocation failed");
    delete k;
    return LSLAM_ERR_HIP;
  }
  *out = k;
  return LSLAM_OK;
}

void lslam_kfs_destroy(lslam_kfs *k) {
  if (!k) return;
  if (lslam::ctx_alive(k->ctx)) {  // (a store may outlive its ctx: the ctx waited for its streams when it went)
    (void)hipSetDevice(lslam::ctx_device(k->ctx));
    (void)hipStreamSynchronize(k->stream);
  }
  delete k;
}

int lslam_kfs_clear(lslam_kfs *k) {
  const int rc = check_kfs(k, "lslam_kfs_clear");
  if (rc) return rc;
  LSLAM_TRY(hipStreamSynchronize(k->stream));
  k->kfs.clear();
  k->slabs.clear();
  k->total[0] = k->total[1] = 0;
  k->held_points = 0;
  k->n_local[0] = k->n_local[1] = 0;
  k->sc.drop();  // the descriptors go with the keyframes; the scan-context parameters stay
  k->vis.drop();  // ... and so do the range images; the visibility parameters stay
  k->occ.drop();  // ... and the occupancy grid, which was built from these keyframes; its parameters stay
  return LSLAM_OK;
}

int lslam_kfs_add(lslam_kfs *k, const void *corner, size_t n_corner, const void *surf, size_t n_surf, size_t stride_bytes, int32_t *id) {
  return add_impl(k, corner, n_corner, surf, n_surf, stride_bytes, true, id);
}

int lslam_kfs_add_device(lslam_kfs *k, const void *d_corner, size_t n_corner, const void *d_surf, size_t n_surf, int32_t *id) {
  return add_impl(k, d_corner, n_corner, d_surf, n_surf, sizeof(float4), false, id);
}

int lslam_kfs_counts(lslam_kfs *k, int32_t id, size_t *n_corner, size_t *n_surf) {
  if (n_corner) *n_corner = 0;
  if (n_surf) *n_surf = 0;
  int rc = check_kfs(k, "lslam_kfs_counts");
  if (rc) return rc;
  rc = check_id(k, "lslam_kfs_counts", id);
  if (rc) return rc;
  if (n_corner) *n_corner = k->kfs[(size_t)id].n[0];
  if (n_surf) *n_surf = k->kfs[(size_t)id].n[1];
  return LSLAM_OK;
}

int lslam_kfs_get(lslam_kfs *k, int32_t id, int32_t which, float *out_xyzi, size_t cap, size_t *n_out) {
  if (n_out) *n_out = 0;
  int rc = check_kfs(k, "lslam_kfs_get");
  if (rc) return rc;
  rc = check_id(k, "lslam_kfs_get", id);
  if (rc) return rc;
  if (which < 0 || which > 1) {
    lslam::set_error("lslam_kfs_get: which is 0 (corner) or 1 (surf)");
    return LSLAM_ERR_INVALID;
  }
  const KeyframeClouds &kc = k->kfs[(size_t)id];
  const size_t n = kc.n[which];
  if (n_out) *n_out = n;
  if (!out_xyzi) return LSLAM_OK;  // the count only
  if (n > cap) {
    lslam::set_error("lslam_kfs_get: output buffer too small");
    return LSLAM_ERR_INVALID;
  }
  if (n) {
    LSLAM_TRY(hipMemcpyAsync(out_xyzi, kc.p[which], n * sizeof(float4), hipMemcpyDeviceToHost, k->stream));
    LSLAM_TRY(hipStreamSynchronize(k->stream));
    k->bytes_down += (uint64_t)n * sizeof(float4);
  }
  return LSLAM_OK;
}

int lslam_kfs_view(lslam_kfs *k, int32_t id, const float **d_corner, size_t *n_corner, const float **d_surf, size_t *n_surf) {
  if (d_corner) *d_corner = nullptr;
  if (d_surf) *d_surf = nullptr;
  if (n_corner) *n_corner = 0;
  if (n_surf) *n_surf = 0;
  int rc = check_kfs(k, "lslam_kfs_view");
  if (rc) return rc;
  rc = check_id(k, "lslam_kfs_view", id);
  if (rc) return rc;
  const KeyframeClouds &kc = k->kfs[(size_t)id];
  if (d_corner) *d_corner = reinterpret_cast<const float *>(kc.p[0]);
  if (d_surf) *d_surf = reinterpret_cast<const float *>(kc.p[1]);
  if (n_corner) *n_corner = kc.n[0];
  if (n_surf) *n_surf = kc.n[1];
  return LSLAM_OK;
}

int lslam_kfs_info(lslam_kfs *k, lslam_kfs_stats *stats) {
  if (stats) std::memset(stats, 0, sizeof(*stats));
  const int rc = check_kfs(k, "lslam_kfs_info");
  if (rc) return rc;
  if (!stats) {
    lslam::set_error("lslam_kfs_info: null stats");
    return LSLAM_ERR_INVALID;
  }
  stats->n_keyframes = (int64_t)k->kfs.size();
  stats->n_points[0] = k->total[0];
  stats->n_points[1] = k->total[1];
  stats->n_slabs = (int64_t)k->slabs.size();
  stats->bytes_held = (uint64_t)k->held_points * sizeof(float4);
  stats->cloud_bytes_uploaded = k->bytes_up;
  stats->cloud_bytes_downloaded = k->bytes_down;
  return LSLAM_OK;
}

int lslam_kfs_debug_local_clouds(lslam_kfs *k, int32_t n_cand, const int32_t *ids, const float *rel_T, float *corner_out, size_t cap_c,
                                 size_t *n_c, float *surf_out, size_t cap_s, size_t *n_s) {
  if (n_c) *n_c = 0;
  if (n_s) *n_s = 0;
  int rc = check_kfs(k, "lslam_kfs_debug_local_clouds");
  if (rc) return rc;
  rc = assemble(k, "lslam_kfs_debug_local_clouds", n_cand, ids, rel_T);
  if (rc) {
    (void)hipStreamSynchronize(k->stream);
    return rc;
  }
  if (n_c) *n_c = k->n_local[0];
  if (n_s) *n_s = k->n_local[1];
  float *dst[2] = {corner_out, surf_out};
  const size_t cap[2] = {cap_c, cap_s};
  for (int t = 0; t < 2; ++t) {
    if (!dst[t]) continue;  // the count only
    if (k->n_local[t] > cap[t]) {
      (void)hipStreamSynchronize(k->stream);
      lslam::set_error("lslam_kfs_debug_local_clouds: output buffer too small");
      return LSLAM_ERR_INVALID;
    }
    if (k->n_local[t]) {
      LSLAM_TRY(hipMemcpyAsync(dst[t], k->local[t].p, k->n_local[t] * sizeof(float4), hipMemcpyDeviceToHost, k->stream));
      k->bytes_down += (uint64_t)k->n_local[t] * sizeof(float4);
    }
  }
  LSLAM_TRY(hipStreamSynchronize(k->stream));
  return LSLAM_OK;
}

int lslam_kfs_loop_match(lslam_kfs *k, int32_t n_cand, const int32_t *ids, const float *rel_T, int32_t new_id, float guess[16],
                         int32_t icp_max_iterations, const lslam_opts *opts, int32_t *stage, double *fitness, int32_t *icp_iterations,
                         lslam_stats *stats) {
  if (stage) *stage = LSLAM_KFS_EMPTY_REFERENCE;
  if (fitness) *fitness = 0.0;
  if (icp_iterations) *icp_iterations = 0;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  int rc = check_kfs(k, "lslam_kfs_loop_match");
  if (rc) return rc;
  if (!guess) {
    lslam::set_error("lslam_kfs_loop_match: null guess");
    return LSLAM_ERR_INVALID;
  }
  rc = check_id(k, "lslam_kfs_loop_match", new_id);
  if (rc) return rc;
  rc = assemble(k, "lslam_kfs_loop_match", n_cand, ids, rel_T);
  if (rc) {
    (void)hipStreamSynchronize(k->stream);
    return rc;
  }
  const KeyframeClouds nk = k->kfs[(size_t)new_id];
  if (k->n_local[1] == 0) {  // corseMatching, loop_detector.hpp:233-235
    LSLAM_TRY(hipStreamSynchronize(k->stream));
    return LSLAM_OK;
  }
  // ---- corseMatching: ICP of the new keyframe's surface cloud onto the candidates' (lslam_icp_align) -------------------------
  rc = index_cloud(k, k->local[1].p, k->n_local[1], k->indexed[1]);
  if (rc) return rc;
  int32_t converged = 0;
  rc = lslam::icp_align_device(k->ctx, k->indexed[1].p, k->n_local[1], nk.p[1], nk.n[1], guess, icp_max_iterations, 0.0, 0.0, fitness,
                               &converged, icp_iterations);
  if (rc) return rc;
  if (stage) *stage = LSLAM_KFS_ICP_REJECTED;
  if (!converged) return LSLAM_OK;
  // ---- scanMatchLocal (ScanMatch.cpp:362-398): VoxelGrid 0.2 / 0.4 / 0.2 / 0.4, then scanMatchScan -----------------------------
  float lo[2][3], hi[2][3];
  {
    const float4 *bp[2] = {k->local[0].p, k->local[1].p};
    const int bn[2] = {(int)k->n_local[0], (int)k->n_local[1]};
    LSLAM_TRY(lslam::grid_bbox2(bp, bn, k->d_box.p, lo, hi, k->stream));
  }
  const float4 *in[4] = {k->local[0].p, k->local[1].p, nk.p[0], nk.p[1]};
  const size_t n_in[4] = {k->n_local[0], k->n_local[1], nk.n[0], nk.n[1]};
  const float *blo[4] = {lo[0], lo[1], nk.lo[0], nk.lo[1]}, *bhi[4] = {hi[0], hi[1], nk.hi[0], nk.hi[1]};
  const float leaf[4] = {0.2f, 0.4f, 0.2f, 0.4f};  // ScanMatch.cpp:29-30
  size_t m[4] = {0, 0, 0, 0};
  for (int c = 0; c < 4; ++c) {
    LSLAM_TRY(k->filt[c].reserve(n_in[c] ? n_in[c] : 1));
    rc = lslam::voxel_grid_device(k->ctx, in[c], n_in[c], blo[c], bhi[c], leaf[c], k->filt[c].p, &m[c]);
    if (rc) {
      (void)hipStreamSynchronize(k->stream);
      return rc;
    }
  }
  if (stage) *stage = LSLAM_KFS_MATCH_FAILED;
  if (m[0] < 50 || m[1] < 100) {  // ScanMatch.cpp:57-61, before the trees are built (lslam_scanmatch_full)
    LSLAM_TRY(hipStreamSynchronize(k->stream));
    if (stats) stats->status = LSLAM_TOO_FEW_REF;
    float tw[6];  // the mirrors hand the pose over as a twist and take it back as an isometry, also when nothing ran
    lslam_isometry_to_pose(guess, tw);
    lslam_pose_to_isometry(tw, guess);
    return LSLAM_OK;
  }
  for (int t = 0; t < 2; ++t) {
    rc = index_cloud(k, k->filt[t].p, m[t], k->indexed[t]);
    if (rc) return rc;
  }
  rc = lslam::map_set_device(k->ctx, k->indexed[0].p, m[0], k->indexed[1].p, m[1]);
  if (rc) return rc;
  float pose[6];
  lslam_isometry_to_pose(guess, pose);
  lslam_stats local;
  lslam_stats *st = stats ? stats : &local;
  rc = lslam::scanmatch_scan_device(k->ctx, k->filt[2].p, m[2], k->filt[3].p, m[3], pose, opts, st);
  if (rc < 0) return rc;
  lslam_pose_to_isometry(pose, guess);  // written back also when the match failed (ScanMatch.cpp:342-346)
  if (rc == LSLAM_OK && stage) *stage = LSLAM_KFS_LOOP_ACCEPTED;
  return LSLAM_OK;
}

int lslam_keyframe_edge_information(lslam_kfs *k, int32_t n_ref, const int32_t *ref_ids, const float *rel_T, int32_t new_id,
                               const float T[16], float leaf_ref_corner, float leaf_ref_surf, float leaf_corner, float leaf_surf,
                               lslam_edge_info *out) {
  if (out) std::memset(out, 0, sizeof(*out));
  if (!k || !out || !T) {
    lslam::set_error("lslam_keyframe_edge_information: null store, pose or out");
    return LSLAM_ERR_INVALID;
  }
  const float leaf[4] = {leaf_ref_corner, leaf_ref_surf, leaf_corner, leaf_surf};
  for (int c = 0; c < 4; ++c)
    if (!(leaf[c] > 0.0f)) {
      lslam::set_error("lslam_keyframe_edge_information: a leaf that is not positive");
      return LSLAM_ERR_INVALID;
    }
  int rc = check_kfs(k, "lslam_keyframe_edge_information");
  if (rc) return rc;
  rc = check_id(k, "lslam_keyframe_edge_information", new_id);
  if (rc) return rc;
  rc = assemble(k, "lslam_keyframe_edge_information", n_ref, ref_ids, rel_T);
  if (rc) {
    (void)hipStreamSynchronize(k->stream);
    return rc;
  }
  const KeyframeClouds nk = k->kfs[(size_t)new_id];
  // ---- the reference and the scan as lslam_kfs_loop_match's scanMatchLocal makes them ----------------------------------------
  float lo[2][3], hi[2][3];
  {
    const float4 *bp[2] = {k->local[0].p, k->local[1].p};
    const int bn[2] = {(int)k->n_local[0], (int)k->n_local[1]};
    LSLAM_TRY(lslam::grid_bbox2(bp, bn, k->d_box.p, lo, hi, k->stream));
  }
  const float4 *in[4] = {k->local[0].p, k->local[1].p, nk.p[0], nk.p[1]};
  const size_t n_in[4] = {k->n_local[0], k->n_local[1], nk.n[0], nk.n[1]};
  const float *blo[4] = {lo[0], lo[1], nk.lo[0], nk.lo[1]}, *bhi[4] = {hi[0], hi[1], nk.hi[0], nk.hi[1]};
  size_t m[4] = {0, 0, 0, 0};
  for (int c = 0; c < 4; ++c) {
    LSLAM_TRY(k->filt[c].reserve(n_in[c] ? n_in[c] : 1));
    rc = lslam::voxel_grid_device(k->ctx, in[c], n_in[c], blo[c], bhi[c], leaf[c], k->filt[c].p, &m[c]);
    if (rc) {
      (void)hipStreamSynchronize(k->stream);
      return rc;
    }
  }
  if (m[0] == 0 || m[1] == 0) {  // nothing to match against: *out stays zero
    LSLAM_TRY(hipStreamSynchronize(k->stream));
    return LSLAM_OK;
  }
  for (int t = 0; t < 2; ++t) {
    rc = index_cloud(k, k->filt[t].p, m[t], k->indexed[t]);
    if (rc) return rc;
  }
  rc = lslam::map_set_device(k->ctx, k->indexed[0].p, m[0], k->indexed[1].p, m[1]);
  if (rc) return rc;
  rc = lslam::scan_set_device(k->ctx, k->filt[2].p, m[2], k->filt[3].p, m[3]);
  if (rc) return rc;
  float pose[6];
  lslam_isometry_to_pose(T, pose);
  return lslam_match_information(k->ctx, pose, LSLAM_SEARCH_AUTO, out);
}

int lslam_kfs_scanmatch(lslam_kfs *k, int32_t id, float leaf_corner, float leaf_surf, float pose[6], const lslam_opts *opts,
                        lslam_stats *stats) {
  if (stats) std::memset(stats, 0, sizeof(*stats));
  int rc = check_kfs(k, "lslam_kfs_scanmatch");
  if (rc) return rc;
  rc = check_id(k, "lslam_kfs_scanmatch", id);
  if (rc) return rc;
  if (!pose || !(leaf_corner > 0.0f) || !(leaf_surf > 0.0f)) {
    lslam::set_error("lslam_kfs_scanmatch: null pose, or a leaf that is not positive");
    return LSLAM_ERR_INVALID;
  }
  const KeyframeClouds kc = k->kfs[(size_t)id];
  const float leaf[2] = {leaf_corner, leaf_surf};
  size_t m[2] = {0, 0};
  for (int t = 0; t < 2; ++t) {
    LSLAM_TRY(k->filt[2 + t].reserve(kc.n[t] ? kc.n[t] : 1));
    rc = lslam::voxel_grid_device(k->ctx, kc.p[t], kc.n[t], kc.lo[t], kc.hi[t], leaf[t], k->filt[2 + t].p, &m[t]);
    if (rc) {
      (void)hipStreamSynchronize(k->stream);
      return rc;
    }
  }
  return lslam::scanmatch_scan_device(k->ctx, k->filt[2].p, m[0], k->filt[3].p, m[1], pose, opts, stats);
}

int lslam_kfs_add_to_fmap(lslam_kfs *k, int32_t id, lslam_fmap *fm, const float T[16]) {
  int rc = check_kfs(k, "lslam_kfs_add_to_fmap");
  if (rc) return rc;
  rc = check_id(k, "lslam_kfs_add_to_fmap", id);
  if (rc) return rc;
  if (!fm || !T) {
    lslam::set_error("lslam_kfs_add_to_fmap: null feature map or null pose");
    return LSLAM_ERR_INVALID;
  }
  const KeyframeClouds &kc = k->kfs[(size_t)id];
  return lslam::fmap_add_feature_cloud_device(fm, kc.p[0], kc.n[0], kc.p[1], kc.n[1], T);
}

}  // extern "C"
