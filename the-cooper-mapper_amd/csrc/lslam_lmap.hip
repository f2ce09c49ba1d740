// lslam_lmap.hip -- the sliding-window local map in HBM: io_module/LocalFeatureMap.h (addDataFrame, clean, getSurroundFeature)
// with FrameUpdater.hpp's path length, the map container of odometry/LaserMappingLocal.cpp.
//
// Layout: per feature type ONE ring of float4 {x, y, z, intensity} holding the live frames' transformed clouds back to back in
// queue order (oldest first, inside a frame in the frame's order); the host keeps the table of frames {first, count, accum,
// box} and all of FrameUpdater / clean() in double -- a dozen flops per frame.  An eviction moves the ring's head: whole frames
// leave from the front, nothing is copied.  The surround is pcl::VoxelGrid over the concatenation of the window, per type with
// its own leaf, produced in one of two ways (a creation flag; same bits):
//   (a) LSLAM_LMAP_REFILTER: the live points are gathered out of the ring (wrap-around handled there) and filtered by
//       voxel_filter_segments as ONE segment -- min_b, the "leaf too small" guard and the sort of everything, every sweep;
//   (b) LSLAM_LMAP_KEY_ORDERED: besides the ring, each type's points are kept in (absolute voxel of the type's leaf, arrival)
//       order.  Voxels are cut at absolute multiples of the leaf, so neither the grouping nor the (z, y, x) output order depends
//       on min_b, and a type has one leaf for its whole life: the order never goes stale.  A sweep sorts only the points that
//       arrived since the last one and merges them in behind their equals (lslam_fmap.hip's run_pipeline, n_sorted path:
//       voxel_filter_window), an eviction is a stable compaction by frame sequence, the centroid pass runs over the whole array.
//       The window's extent -- guard, min_b, key width -- comes from the frames' boxes on the host, every sweep.  When the guard
//       fires (the filter hands the input back in ARRIVAL order) or the key does not fit, the sweep takes (a); when the device
//       finds the order broken, the array is rebuilt from the ring by a sort of everything.
// The filtered clouds become the context's map through map_set_device with their boxes: one wait per surround, both types.
//
// The one place this container differs from the reference: LocalFeatureMap's queue grows without bound (a sensor that stands
// still never advances accum_distance, so nothing is ever erased); HBM cannot.  create() takes max_points per type and
// max_frames, and an add whose result would exceed either is refused with LSLAM_ERR_INVALID and changes nothing.
#include "../../include/lslam_c.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>

#include "lslam_internal.hpp"
#include "lslam_pointgrid_dev.hpp"

namespace {

constexpr size_t LM_MAX_POINTS = (size_t)1 << 24;      // per type (the compaction's block offsets are summed per block)
constexpr size_t LM_DEFAULT_POINTS = (size_t)1 << 20;  // 30 m at 0.1 m per sweep: 300 frames x ~1000 corner / ~2500 surf points
constexpr int32_t LM_DEFAULT_FRAMES = 4096;
constexpr int LM_TILE = 1024;  // elements per workgroup of the compaction (4 rounds of 256)

// One frame's two clouds, both types in one launch (workgroups [0, nb0) work on type 0): p' = R p + t with the operation order of
// fm_transform_kernel (pcl::transformPointCloud, transform_utils.h:601-614), into the staging of the add, and the clouds' boxes.
struct TransformArgs {
  const float4 *in[2];
  float4 *out[2];
  int n[2];
  int nb0;
  uint32_t *res;  // [2][8]
};
__global__ __launch_bounds__(256) void lm_transform_kernel(const TransformArgs a, const lslam::Rigid12 Tm) {
  const int t = (int)blockIdx.x >= a.nb0 ? 1 : 0;
  const int i = ((int)blockIdx.x - (t ? a.nb0 : 0)) * 256 + (int)threadIdx.x;
  const bool in = i < a.n[t];
  uint32_t mm[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  if (in) {
    const float4 q = lslam::rigid_transform_point(Tm.m, a.in[t][i]);
    a.out[t][i] = q;
    lslam::box_add(mm, q);
  }
  lslam::box_reduce(mm, in, a.res + 8 * t + 1);
}

// The commit of an add: the staged frame goes to the tail of its ring (wrapping) and, for the key-ordered window, behind the
// points that wait to be merged in, with the frame's sequence number.
struct AppendArgs {
  const float4 *in[2];
  float4 *ring[2];
  float4 *xs[2];     // null: no key-ordered array
  uint32_t *xq[2];
  int n[2];
  int nb0;
  uint32_t tail[2];  // ring position of the frame's first point
  uint32_t nx[2];    // entries of xs before the frame
  uint32_t cap;
  uint32_t seq;
};
__global__ __launch_bounds__(256) void lm_append_kernel(const AppendArgs a) {
  const int t = (int)blockIdx.x >= a.nb0 ? 1 : 0;
  const int i = ((int)blockIdx.x - (t ? a.nb0 : 0)) * 256 + (int)threadIdx.x;
  if (i >= a.n[t]) return;
  const float4 p = a.in[t][i];
  uint32_t r = a.tail[t] + (uint32_t)i;  // tail < cap, i < cap <= 2^24
  if (r >= a.cap) r -= a.cap;
  a.ring[t][r] = p;
  if (a.xs[t]) {
    const uint32_t x = a.nx[t] + (uint32_t)i;
    if (x < a.cap) {
      a.xs[t][x] = p;
      a.xq[t][x] = a.seq;
    }
  }
}

// the live points of a ring, in queue order, as one array
__global__ __launch_bounds__(256) void lm_gather_kernel(const float4 *ring, uint32_t cap, uint32_t head, int n, float4 *out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t r = head + (uint32_t)i;
  if (r >= cap) r -= cap;
  out[i] = ring[r];
}

// The filtered cloud as the map wants it -- {x, y, z, bitcast(index)} -- with its bounding box.  The number of points is on the
// device (or in pinned memory) when this runs: *n_ptr, clamped to the buffers' size.  res[0] = points, res[1..6] the box.
__global__ __launch_bounds__(256) void lm_index_box_kernel(const float4 *filt, const uint32_t *n_ptr, uint32_t cap, float4 *map_pts,
                                                           uint32_t *res) {
  const uint32_t n = min(*n_ptr, cap);
  if (blockIdx.x == 0 && threadIdx.x == 0) res[0] = n;
  uint32_t mm[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  bool any = false;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    float4 p = filt[i];
    lslam::box_add(mm, p);
    p.w = __builtin_bit_cast(float, i);
    map_pts[i] = p;
    any = true;
  }
  lslam::box_reduce(mm, any, res + 1);
}

// Eviction from the key-ordered array: a stable compaction of the entries whose frame is still in the queue (seq >= min_seq).
// Pass 1: live entries per tile of LM_TILE.
__global__ __launch_bounds__(256) void lm_live_count_kernel(const uint32_t *xq, int n, uint32_t min_seq, int32_t *tile_count) {
  const int base = blockIdx.x * LM_TILE;
  int c = 0;
#pragma unroll
  for (int r = 0; r < LM_TILE / 256; ++r) {
    const int i = base + r * 256 + (int)threadIdx.x;
    c += (i < n && xq[i] >= min_seq) ? 1 : 0;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
  __shared__ int part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_count[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}
// Pass 2: every workgroup sums the tiles before its own (a few thousand words at most: no scan launch between the passes), then
// places its live entries in order -- ballot prefix inside a wavefront, the four wavefronts' counts through LDS.
__global__ __launch_bounds__(256) void lm_compact_kernel(const float4 *xs, const uint32_t *xq, int n, uint32_t min_seq,
                                                         const int32_t *tile_count, float4 *xs_out, uint32_t *xq_out, uint32_t cap) {
  __shared__ int part[4];
  __shared__ int wave_n[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int before = 0;
  for (int b = (int)threadIdx.x; b < (int)blockIdx.x; b += 256) before += tile_count[b];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) before += __shfl_xor(before, d, 64);
  if (lane == 0) part[wave] = before;
  __syncthreads();
  int offset = part[0] + part[1] + part[2] + part[3];
  const int base = blockIdx.x * LM_TILE;
  for (int r = 0; r < LM_TILE / 256; ++r) {
    const int i = base + r * 256 + (int)threadIdx.x;
    const bool live = i < n && xq[i] >= min_seq;
    const unsigned long long m = __ballot(live);
    __syncthreads();  // (wave_n of the previous round has been read)
    if (lane == 0) wave_n[wave] = __popcll(m);
    __syncthreads();
    int w_before = 0;
    for (int w = 0; w < wave; ++w) w_before += wave_n[w];
    const int round_total = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
    if (live) {
      const uint32_t dst = (uint32_t)(offset + w_before + __popcll(m & ((1ull << lane) - 1ull)));
      if (dst < cap) {
        xs_out[dst] = xs[i];
        xq_out[dst] = xq[i];
      }
    }
    offset += round_total;
  }
}

// the key-ordered array after a merge: entry j is the input's entry order[j]
__global__ __launch_bounds__(256) void lm_permute_kernel(const float4 *xs, const uint32_t *xq, const uint32_t *order, int n, float4 *xs_out,
                                                         uint32_t *xq_out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const uint32_t i = min(order[j], (uint32_t)(n - 1));  // (a merge whose prefix was not in order leaves no permutation: the result is discarded)
  xs_out[j] = xs[i];
  xq_out[j] = xq[i];
}

struct LFrame {
  uint64_t first[2];  // absolute ring counters (position = counter % cap)
  uint32_t count[2];
  double accum;       // DataFrame::accum_distance
  uint32_t seq;
  float lo[2][3], hi[2][3];  // the transformed clouds' boxes
};

}  // namespace

struct lslam_lmap {
  lslam_ctx *ctx = nullptr;
  hipStream_t stream = nullptr;
  int32_t flags = 0;
  bool key_ordered = false, always_resort = false;
  size_t cap = 0;
  int32_t max_frames = 0;
  double queue_distance = 30.0;       // LocalFeatureMap.h: queue_distance_threshold
  float leaf[2] = {0.2f, 0.4f};       // LocalFeatureMap.h:29-33
  // FrameUpdater
  bool is_first = true;
  double prev[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  double accum = 0.0;
  std::deque<LFrame> frames;
  uint32_t next_seq = 0;
  int64_t evicted = 0;
  bool has_frames_ever = false;  // the leaves are fixed from the first frame on
  // rings
  lslam::DevBuf<float4> ring[2];
  uint64_t head[2] = {0, 0}, tail[2] = {0, 0};
  size_t live[2] = {0, 0};
  // add staging
  lslam::PinBuf<float4> h_stage[2];
  lslam::DevBuf<float4> d_raw[2], d_tf[2];
  // surround
  lslam::DevBuf<float4> gath[2], filt[2], mapp[2];
  lslam::DevBuf<int32_t> seg[2], oseg[2];  // zeros (one segment) / the filter's segment output
  lslam::DevBuf<uint32_t> d_res;  // [2][8] add boxes, [2][8] surround counts and boxes
  lslam::PinBuf<uint32_t> h_pin;  // pinned: [2][4] done words, [2][8] add boxes, [2][8] surround results
  bool sur_valid = false;
  size_t n_sur[2] = {0, 0};
  float sur_lo[2][3], sur_hi[2][3];
  // key-ordered window
  lslam::DevBuf<float4> xs[2], xs_alt[2];
  lslam::DevBuf<uint32_t> xq[2], xq_alt[2];
  lslam::DevBuf<int32_t> tile_count;
  size_t nx[2] = {0, 0}, nx_sorted[2] = {0, 0};  // entries of xs / of its prefix that is in key order (evicted ones included until compacted)
  uint32_t pend_seq[2] = {0, 0};                 // frames from this sequence number on are behind the prefix
  bool x_valid[2] = {true, true}, x_dead[2] = {false, false};
  lslam::WindowFilter *wf[2] = {nullptr, nullptr};
  int64_t n_merged = 0, n_resorted = 0, n_refiltered = 0;
};

namespace {

uint32_t *done_words(lslam_lmap *lm, int t) { return lm->h_pin.p + 4 * t; }
uint32_t *h_addbox(lslam_lmap *lm) { return lm->h_pin.p + 8; }
uint32_t *h_surres(lslam_lmap *lm) { return lm->h_pin.p + 24; }

int check_lm(lslam_lmap *lm, const char *what) {
  if (!lm) {
    char b[160];
    snprintf(b, sizeof(b), "%s: null local map", what);
    lslam::set_error(b);
    return LSLAM_ERR_INVALID;
  }
  if (!lslam::ctx_alive(lm->ctx)) {
    lslam::set_error("local map: its ctx was destroyed");
    return LSLAM_ERR_INVALID;
  }
  LSLAM_TRY(hipSetDevice(lslam::ctx_device(lm->ctx)));
  return LSLAM_OK;
}

void free_all(lslam_lmap *lm) {  // what no member's destructor releases
  for (int t = 0; t < 2; ++t) {
    lslam::window_filter_destroy(lm->wf[t]);
    lm->wf[t] = nullptr;
  }
}

void reset_state(lslam_lmap *lm) {  // LocalFeatureMap as constructed (the leaves and the queue distance stay)
  lm->is_first = true;
  lm->accum = 0.0;
  lm->frames.clear();
  lm->evicted = 0;
  lm->has_frames_ever = false;
  for (int t = 0; t < 2; ++t) {
    lm->head[t] = lm->tail[t] = 0;
    lm->live[t] = 0;
    lm->nx[t] = lm->nx_sorted[t] = 0;
    lm->pend_seq[t] = lm->next_seq;
    lm->x_valid[t] = true;
    lm->x_dead[t] = false;
  }
  lm->sur_valid = false;
}

int reserve_stage(lslam_lmap *lm, int t, size_t n, bool host) {
  LSLAM_TRY(lm->d_raw[t].reserve(n));
  LSLAM_TRY(lm->d_tf[t].reserve(n));
  if (host) LSLAM_TRY(lm->h_stage[t].reserve(n));
  return LSLAM_OK;
}

// a HIP error in the middle of an add or a surround: the device side is of unknown content -- the container is emptied, which
// is a state of its own right (never half a frame)
int fail_reset(lslam_lmap *lm, int rc) {
  reset_state(lm);
  return rc;
}

// addDataFrame: host = the clouds are in host memory (stride_bytes apart), else packed float4 in the context's device memory
int add_impl(lslam_lmap *lm, const void *corner, size_t n_corner, const void *surf, size_t n_surf, size_t stride_bytes,
             const float T_map[16], bool host) {
  int rc = check_lm(lm, "lslam_lmap_add_data_frame");
  if (rc) return rc;
  if (!T_map || (n_corner && !corner) || (n_surf && !surf) || (host && (stride_bytes < 16 || (stride_bytes & 3)))) {
    lslam::set_error("lslam_lmap_add_data_frame: null cloud with points, null pose, or a stride under 16 bytes");
    return LSLAM_ERR_INVALID;
  }
  const void *src[2] = {corner, surf};
  const size_t n_new[2] = {n_corner, n_surf};
  // ---- FrameUpdater::update + clean(), on copies: nothing is committed before the frame's points are staged --------------
  double P[12];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) P[4 * r + c] = (double)T_map[4 * r + c];  // frame->odom = pose.cast<double>()
  double accum = lm->accum;
  if (!lm->is_first) {
    // (prev^-1 * pose).translation() of two isometries: R_prev^T t + (-(R_prev^T t_prev)), products summed left to right
    const double *Q = lm->prev;
    double d[3];
    for (int k = 0; k < 3; ++k) {
      const double a = (Q[k] * P[3] + Q[4 + k] * P[7]) + Q[8 + k] * P[11];
      const double b = (Q[k] * Q[3] + Q[4 + k] * Q[7]) + Q[8 + k] * Q[11];
      d[k] = a + (-b);
    }
    accum += std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
  }
  size_t n_del = 0;  // clean(): the frames at the front with accum <= current - threshold (the new frame never is one) ...
  for (const LFrame &f : lm->frames) {
    if (f.accum > accum - lm->queue_distance) break;
    ++n_del;
  }
  const size_t size_pushed = lm->frames.size() + 1;
  const size_t n_erase = n_del > 0 ? n_del + 1 : 0;  // ... and ONE MORE is erased (LocalFeatureMap.h:80-81)
  const bool survives = n_erase < size_pushed;         // a step beyond the threshold takes the new frame with the rest
  size_t live_after[2] = {lm->live[0], lm->live[1]};
  for (size_t k = 0; k < std::min(n_erase, lm->frames.size()); ++k)
    for (int t = 0; t < 2; ++t) live_after[t] -= lm->frames[k].count[t];
  if (survives) {
    if (size_pushed - n_erase > (size_t)lm->max_frames) {
      char b[200];
      snprintf(b, sizeof(b), "lslam_lmap_add_data_frame: the window would hold %zu frames, max_frames is %d", size_pushed - n_erase, lm->max_frames);
      lslam::set_error(b);
      return LSLAM_ERR_INVALID;
    }
    for (int t = 0; t < 2; ++t)
      if (live_after[t] + n_new[t] > lm->cap) {
        char b[240];
        snprintf(b, sizeof(b), "lslam_lmap_add_data_frame: the window would hold %zu %s points, max_points_per_type is %zu",
                 live_after[t] + n_new[t], t ? "surf" : "corner", lm->cap);
        lslam::set_error(b);
        return LSLAM_ERR_INVALID;
      }
  }
  hipStream_t s = lm->stream;
  LFrame fr{};
  if (survives && (n_new[0] || n_new[1])) {
    // ---- stage: upload (both types), transform, boxes; ONE wait -------------------------------------------------------------
    TransformArgs ta{};
    for (int t = 0; t < 2; ++t) {
      rc = reserve_stage(lm, t, n_new[t], host);
      if (rc) return rc;
      if (host && n_new[t]) {
        float4 *h = lm->h_stage[t].p;
        const char *p = static_cast<const char *>(src[t]);
        if (stride_bytes == 16) {
          std::memcpy(h, p, n_new[t] * sizeof(float4));
        } else {  // pcl::PointXYZI: {x, y, z} at 0, the intensity at byte 16 when the point has it
          for (size_t i = 0; i < n_new[t]; ++i) {
            float v[3], w = 0.0f;
            std::memcpy(v, p + i * stride_bytes, 12);
            if (stride_bytes >= 20) std::memcpy(&w, p + i * stride_bytes + 16, 4);
            h[i] = make_float4(v[0], v[1], v[2], w);
          }
        }
        LSLAM_TRY(hipMemcpyAsync(lm->d_raw[t].p, h, n_new[t] * sizeof(float4), hipMemcpyHostToDevice, s));
      }
      ta.in[t] = host ? lm->d_raw[t].p : static_cast<const float4 *>(src[t]);
      ta.out[t] = lm->d_tf[t].p;
      ta.n[t] = (int)n_new[t];
    }
    ta.nb0 = (int)((n_new[0] + 255) / 256);
    ta.res = lm->d_res.p;
    lslam::Rigid12 Tm;
    for (int k = 0; k < 12; ++k) Tm.m[k] = T_map[k];
    LSLAM_TRY(hipMemsetAsync(lm->d_res.p, 0, 16 * sizeof(uint32_t), s));
    hipLaunchKernelGGL(lm_transform_kernel, dim3((unsigned)(ta.nb0 + (int)((n_new[1] + 255) / 256))), dim3(256), 0, s, ta, Tm);
    LSLAM_TRY(hipGetLastError());
    LSLAM_TRY(hipMemcpyAsync(h_addbox(lm), lm->d_res.p, 16 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    LSLAM_TRY(hipStreamSynchronize(s));
    for (int t = 0; t < 2; ++t)
      for (int a = 0; a < 3; ++a) {
        fr.lo[t][a] = n_new[t] ? lslam::ordered_back(~h_addbox(lm)[8 * t + 1 + a]) : INFINITY;
        fr.hi[t][a] = n_new[t] ? lslam::ordered_back(h_addbox(lm)[8 * t + 4 + a]) : -INFINITY;
        if (n_new[t] && !(std::isfinite(fr.lo[t][a]) && std::isfinite(fr.hi[t][a]))) {
          lslam::set_error("lslam_lmap_add_data_frame: a transformed point is not finite");
          return LSLAM_ERR_INVALID;
        }
      }
  } else {
    for (int t = 0; t < 2; ++t)
      for (int a = 0; a < 3; ++a) { fr.lo[t][a] = INFINITY; fr.hi[t][a] = -INFINITY; }
  }
  // ---- commit ---------------------------------------------------------------------------------------------------------------
  lm->is_first = false;
  std::memcpy(lm->prev, P, sizeof(P));
  lm->accum = accum;
  lm->has_frames_ever = true;
  lm->sur_valid = false;
  const uint32_t seq = lm->next_seq++;
  for (size_t k = 0; k < std::min(n_erase, size_pushed - 1); ++k) {
    const LFrame &f = lm->frames.front();
    for (int t = 0; t < 2; ++t) {
      lm->head[t] += f.count[t];
      lm->live[t] -= f.count[t];
      if (f.count[t]) lm->x_dead[t] = true;
    }
    lm->frames.pop_front();
  }
  lm->evicted += (int64_t)n_erase;
  if (!survives || lm->frames.empty()) {  // nothing of the old window is left: the rings and the ordered arrays start over
    for (int t = 0; t < 2; ++t) {
      lm->head[t] = lm->tail[t] = 0;
      lm->live[t] = 0;
      lm->nx[t] = lm->nx_sorted[t] = 0;
      lm->pend_seq[t] = seq;
      lm->x_valid[t] = true;
      lm->x_dead[t] = false;
    }
  }
  if (!survives) return LSLAM_OK;
  if (lm->key_ordered)
    for (int t = 0; t < 2; ++t)
      if (lm->x_valid[t] && lm->nx[t] + n_new[t] > lm->cap) {
        // the ordered array is full of evicted entries: it is rebuilt from the ring at the next surround instead
        lm->x_valid[t] = false;
      }
  if (n_new[0] || n_new[1]) {
    AppendArgs aa{};
    for (int t = 0; t < 2; ++t) {
      aa.in[t] = lm->d_tf[t].p;
      aa.ring[t] = lm->ring[t].p;
      const bool x = lm->key_ordered && lm->x_valid[t];
      aa.xs[t] = x ? lm->xs[t].p : nullptr;
      aa.xq[t] = x ? lm->xq[t].p : nullptr;
      aa.n[t] = (int)n_new[t];
      aa.tail[t] = (uint32_t)(lm->tail[t] % lm->cap);
      aa.nx[t] = (uint32_t)lm->nx[t];
    }
    aa.nb0 = (int)((n_new[0] + 255) / 256);
    aa.cap = (uint32_t)lm->cap;
    aa.seq = seq;
    hipLaunchKernelGGL(lm_append_kernel, dim3((unsigned)(aa.nb0 + (int)((n_new[1] + 255) / 256))), dim3(256), 0, s, aa);
    if (hipGetLastError() != hipSuccess) {
      lslam::set_error("lslam_lmap_add_data_frame: the append launch failed; the window was emptied");
      return fail_reset(lm, LSLAM_ERR_HIP);
    }
  }
  fr.accum = accum;
  fr.seq = seq;
  for (int t = 0; t < 2; ++t) {
    fr.first[t] = lm->tail[t];
    fr.count[t] = (uint32_t)n_new[t];
    lm->tail[t] += n_new[t];
    lm->live[t] += n_new[t];
    if (lm->key_ordered && lm->x_valid[t]) lm->nx[t] += n_new[t];
  }
  lm->frames.push_back(fr);
  return LSLAM_OK;
}

// the window's extent of type t, from the frames' boxes
void window_box(const lslam_lmap *lm, int t, float mn[3], float mx[3]) {
  for (int a = 0; a < 3; ++a) { mn[a] = INFINITY; mx[a] = -INFINITY; }
  for (const LFrame &f : lm->frames)
    if (f.count[t])
      for (int a = 0; a < 3; ++a) {
        mn[a] = f.lo[t][a] < mn[a] ? f.lo[t][a] : mn[a];
        mx[a] = f.hi[t][a] > mx[a] ? f.hi[t][a] : mx[a];
      }
}

int index_box(lslam_lmap *lm, int t, const uint32_t *n_ptr) {
  const unsigned blocks = (unsigned)std::min<size_t>(512, (lm->live[t] + 255) / 256);
  hipLaunchKernelGGL(lm_index_box_kernel, dim3(blocks), dim3(256), 0, lm->stream, (const float4 *)lm->filt[t].p, n_ptr, (uint32_t)lm->cap,
                     lm->mapp[t].p, lm->d_res.p + 16 + 8 * t);
  LSLAM_TRY(hipGetLastError());
  return LSLAM_OK;
}

int gather_ring(lslam_lmap *lm, int t, float4 *out) {
  const int n = (int)lm->live[t];
  if (!n) return LSLAM_OK;
  hipLaunchKernelGGL(lm_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, lm->stream, (const float4 *)lm->ring[t].p,
                     (uint32_t)lm->cap, (uint32_t)(lm->head[t] % lm->cap), n, out);
  LSLAM_TRY(hipGetLastError());
  return LSLAM_OK;
}

// (a): gather + voxel_filter_segments over one segment.  wait: the filter's blocking form (the retry after a key-range error)
int refilter(lslam_lmap *lm, int t, bool wait) {
  int rc = gather_ring(lm, t, lm->gath[t].p);
  if (rc) return rc;
  size_t m = 0;
  uint32_t *done = done_words(lm, t);
  done[0] = done[1] = done[2] = 0;
  rc = lslam::voxel_filter_segments(lm->ctx, lm->gath[t].p, lm->seg[t].p, lm->live[t], 1, lm->leaf[t], lm->filt[t].p, lm->oseg[t].p, &m, true,
                                    wait ? nullptr : done);
  if (rc) return rc;
  if (wait) done[0] = (uint32_t)m;
  lm->n_refiltered++;
  return index_box(lm, t, done);
}

// (b): *took = false when this sweep cannot go through the ordered array (guard, key width): the caller takes (a)
int ordered_filter(lslam_lmap *lm, int t, bool *took) {
  *took = false;
  hipStream_t s = lm->stream;
  float mn[3], mx[3];
  window_box(lm, t, mn, mx);
  // what pcl::VoxelGrid::applyFilter (and lslam_voxel_grid) derive from the extent
  const float inv = 1.0f / lm->leaf[t];
  int32_t base0[3];
  double cells = 1.0, vol = 1.0;
  for (int d = 0; d < 3; ++d) {
    const float fl = std::floor(mn[d] * inv), fh = std::floor(mx[d] * inv), fe = (mx[d] - mn[d]) * inv;
    if (!(std::fabs(fl) < 1.0e9f && std::fabs(fh) < 1.0e9f && fe < 4.0e18f)) return LSLAM_OK;  // (a)'s business
    base0[d] = (int32_t)fl;
    const double c = (double)((int32_t)fh - base0[d] + 1);
    cells = c > cells ? c : cells;
    vol *= (double)((long long)fe + 1);
  }
  if (!(vol <= 2147483647.0)) return LSLAM_OK;  // "Leaf size is too small": the input comes back unfiltered, in arrival order
  int bits = 1;
  while ((double)(1ull << bits) < cells + 1.0) ++bits;
  if (3 * bits + 1 > 63) return LSLAM_OK;
  const uint32_t min_seq = lm->frames.front().seq;
  if (lm->always_resort) lm->x_valid[t] = false;
  if (!lm->x_valid[t]) {  // rebuild from the ring: everything is "new"
    int rc = gather_ring(lm, t, lm->xs[t].p);
    if (rc) return rc;
    size_t at = 0;
    for (const LFrame &f : lm->frames) {  // (the fall-back path: one fill per frame)
      if (f.count[t]) LSLAM_TRY(hipMemsetD32Async((hipDeviceptr_t)(lm->xq[t].p + at), (int)f.seq, f.count[t], s));
      at += f.count[t];
    }
    lm->nx[t] = lm->live[t];
    lm->nx_sorted[t] = 0;
    lm->x_dead[t] = false;
    lm->x_valid[t] = true;
  } else if (lm->x_dead[t] && lm->nx[t]) {  // evictions since the last sweep: stable compaction by frame sequence
    const int n = (int)lm->nx[t];
    const unsigned tiles = (unsigned)((n + LM_TILE - 1) / LM_TILE);
    hipLaunchKernelGGL(lm_live_count_kernel, dim3(tiles), dim3(256), 0, s, (const uint32_t *)lm->xq[t].p, n, min_seq, lm->tile_count.p);
    hipLaunchKernelGGL(lm_compact_kernel, dim3(tiles), dim3(256), 0, s, (const float4 *)lm->xs[t].p, (const uint32_t *)lm->xq[t].p, n, min_seq,
                       (const int32_t *)lm->tile_count.p, lm->xs_alt[t].p, lm->xq_alt[t].p, (uint32_t)lm->cap);
    LSLAM_TRY(hipGetLastError());
    std::swap(lm->xs[t], lm->xs_alt[t]);
    std::swap(lm->xq[t], lm->xq_alt[t]);
    size_t sorted_live = 0;
    for (const LFrame &f : lm->frames)
      if ((int32_t)(f.seq - lm->pend_seq[t]) < 0) sorted_live += f.count[t];
    lm->nx_sorted[t] = sorted_live;
    lm->nx[t] = lm->live[t];
    lm->x_dead[t] = false;
  }
  uint32_t *done = done_words(lm, t);
  done[0] = done[1] = done[2] = 0;
  const uint32_t *order = nullptr;
  int rc = lslam::voxel_filter_window(s, lm->wf[t], lm->xs[t].p, lm->nx_sorted[t], lm->nx[t], lm->leaf[t], base0, bits, lm->filt[t].p, done, &order);
  if (rc) return rc;
  if (lm->nx_sorted[t] > 0 && lm->nx_sorted[t] < lm->nx[t]) lm->n_merged++; else lm->n_resorted++;
  const int n = (int)lm->nx[t];
  hipLaunchKernelGGL(lm_permute_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float4 *)lm->xs[t].p, (const uint32_t *)lm->xq[t].p,
                     order, n, lm->xs_alt[t].p, lm->xq_alt[t].p);
  LSLAM_TRY(hipGetLastError());
  std::swap(lm->xs[t], lm->xs_alt[t]);
  std::swap(lm->xq[t], lm->xq_alt[t]);
  lm->nx_sorted[t] = lm->nx[t];
  lm->pend_seq[t] = lm->next_seq;
  *took = true;
  return index_box(lm, t, done);
}

// getSurroundFeature: both types filtered, counts and boxes on the host; ONE wait
int ensure_surround(lslam_lmap *lm) {
  if (lm->sur_valid) return LSLAM_OK;
  hipStream_t s = lm->stream;
  bool any = false, ordered[2] = {false, false};
  uint32_t *h = h_surres(lm);
  for (int k = 0; k < 16; ++k) h[k] = 0u;
  LSLAM_TRY(hipMemsetAsync(lm->d_res.p + 16, 0, 16 * sizeof(uint32_t), s));
  for (int t = 0; t < 2; ++t) {
    if (!lm->live[t]) continue;
    int rc = LSLAM_OK;
    if (lm->key_ordered) rc = ordered_filter(lm, t, &ordered[t]);
    if (!rc && !ordered[t]) rc = refilter(lm, t, false);
    if (rc) {  // (an argument-like error -- an extent no key can hold -- leaves the window as it was; a runtime error empties it)
      (void)hipStreamSynchronize(s);
      lm->x_valid[0] = lm->x_valid[1] = false;
      return rc == LSLAM_ERR_HIP ? fail_reset(lm, rc) : rc;
    }
    any = true;
  }
  if (any) {
    LSLAM_TRY(hipMemcpyAsync(h, lm->d_res.p + 16, 16 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    LSLAM_TRY(hipStreamSynchronize(s));
    for (int t = 0; t < 2; ++t) {
      if (!lm->live[t]) continue;
      const uint32_t *done = done_words(lm, t);
      if (done[1] || (ordered[t] && done[2])) {
        // the key did not hold the points after all, or the ordered array was not in order: the blocking full re-filter
        // decides, and the ordered array is rebuilt from the ring at the next sweep
        if (ordered[t]) lm->x_valid[t] = false;
        LSLAM_TRY(hipMemsetAsync(lm->d_res.p + 16 + 8 * t, 0, 8 * sizeof(uint32_t), s));
        const int rc = refilter(lm, t, true);
        if (rc) return rc == LSLAM_ERR_HIP ? fail_reset(lm, rc) : rc;
        LSLAM_TRY(hipMemcpyAsync(h + 8 * t, lm->d_res.p + 16 + 8 * t, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        LSLAM_TRY(hipStreamSynchronize(s));
      }
    }
  }
  for (int t = 0; t < 2; ++t) {
    lm->n_sur[t] = lm->live[t] ? h[8 * t] : 0;
    lslam::box_back(h + 8 * t + 1, lm->sur_lo[t], lm->sur_hi[t]);
  }
  lm->sur_valid = true;
  return LSLAM_OK;
}

}  // namespace

extern "C" {

int lslam_lmap_create(lslam_ctx *ctx, size_t max_points_per_type, int32_t max_frames, int32_t flags, lslam_lmap **out) {
  if (out) *out = nullptr;
  if (!ctx || !lslam::ctx_alive(ctx) || !out) {
    lslam::set_error("lslam_lmap_create: null ctx or null out");
    return LSLAM_ERR_INVALID;
  }
  const int32_t known = LSLAM_LMAP_REFILTER | LSLAM_LMAP_KEY_ORDERED | LSLAM_LMAP_ALWAYS_RESORT;
  if ((flags & ~known) || ((flags & LSLAM_LMAP_REFILTER) && (flags & (LSLAM_LMAP_KEY_ORDERED | LSLAM_LMAP_ALWAYS_RESORT))) || max_frames < 0 ||
      max_points_per_type > LM_MAX_POINTS) {
    lslam::set_error("lslam_lmap_create: unknown or contradictory flags, negative max_frames, or max_points_per_type above 2^24");
    return LSLAM_ERR_INVALID;
  }
  LSLAM_TRY(hipSetDevice(lslam::ctx_device(ctx)));
  lslam_lmap *lm = new lslam_lmap();
  lm->ctx = ctx;
  lm->stream = lslam::ctx_stream(ctx);
  lm->flags = flags;
  lm->always_resort = (flags & LSLAM_LMAP_ALWAYS_RESORT) != 0;
  lm->key_ordered = lm->always_resort || (flags & LSLAM_LMAP_KEY_ORDERED) != 0 || !(flags & LSLAM_LMAP_REFILTER);  // the default: see DESIGN
  lm->cap = max_points_per_type ? max_points_per_type : LM_DEFAULT_POINTS;
  lm->max_frames = max_frames ? max_frames : LM_DEFAULT_FRAMES;
  const size_t cap = lm->cap;
  hipError_t e = hipSuccess;
  for (int t = 0; t < 2 && e == hipSuccess; ++t) {
    if (e == hipSuccess) e = lm->ring[t].alloc(cap);
    if (e == hipSuccess) e = lm->gath[t].alloc(cap);
    if (e == hipSuccess) e = lm->filt[t].alloc(cap);
    if (e == hipSuccess) e = lm->mapp[t].alloc(cap);
    if (e == hipSuccess) e = lm->seg[t].alloc(cap);
    if (e == hipSuccess) e = lm->oseg[t].alloc(cap);
    if (e == hipSuccess) e = hipMemsetAsync(lm->seg[t].p, 0, cap * sizeof(int32_t), lm->stream);
    if (lm->key_ordered) {
      if (e == hipSuccess) e = lm->xs[t].alloc(cap);
      if (e == hipSuccess) e = lm->xs_alt[t].alloc(cap);
      if (e == hipSuccess) e = lm->xq[t].alloc(cap);
      if (e == hipSuccess) e = lm->xq_alt[t].alloc(cap);
      if (e == hipSuccess) lm->wf[t] = lslam::window_filter_create();
    }
  }
  if (e == hipSuccess) e = lm->d_res.alloc(32);
  if (e == hipSuccess && lm->key_ordered) e = lm->tile_count.alloc((cap + LM_TILE - 1) / LM_TILE);
  if (e == hipSuccess) e = lm->h_pin.alloc(40);
  if (e == hipSuccess) e = hipStreamSynchronize(lm->stream);
  if (e != hipSuccess) {
    char b[200];
    snprintf(b, sizeof(b), "lslam_lmap_create: allocation for %zu points per type failed: %s", cap, hipGetErrorString(e));
    lslam::set_error(b);
    free_all(lm);
    delete lm;
    return LSLAM_ERR_HIP;
  }
  std::memset(lm->h_pin.p, 0, 40 * sizeof(uint32_t));
  reset_state(lm);
  *out = lm;
  return LSLAM_OK;
}

void lslam_lmap_destroy(lslam_lmap *lm) {
  if (!lm) return;
  if (lslam::ctx_alive(lm->ctx)) {  // (a local map may outlive its ctx; its stream is then gone)
    (void)hipSetDevice(lslam::ctx_device(lm->ctx));
    (void)hipStreamSynchronize(lm->stream);
  }
  free_all(lm);
  delete lm;
}

int lslam_lmap_setup_queue_distance(lslam_lmap *lm, double metres) {
  const int rc = check_lm(lm, "lslam_lmap_setup_queue_distance");
  if (rc) return rc;
  if (!(metres > 0.0) || !std::isfinite(metres)) {
    lslam::set_error("lslam_lmap_setup_queue_distance: the distance must be positive and finite");
    return LSLAM_ERR_INVALID;
  }
  lm->queue_distance = metres;
  return LSLAM_OK;
}

int lslam_lmap_setup_filter_size(lslam_lmap *lm, float corner, float surf) {
  const int rc = check_lm(lm, "lslam_lmap_setup_filter_size");
  if (rc) return rc;
  if (!(corner > 0.0f) || !(surf > 0.0f) || !std::isfinite(corner) || !std::isfinite(surf)) {
    lslam::set_error("lslam_lmap_setup_filter_size: the leaves must be positive and finite");
    return LSLAM_ERR_INVALID;
  }
  if (lm->has_frames_ever) {
    lslam::set_error("lslam_lmap_setup_filter_size: the leaves are fixed once a frame has been added (the key-ordered window is sorted by them); "
                     "lslam_lmap_clear first");
    return LSLAM_ERR_INVALID;
  }
  lm->leaf[0] = corner;
  lm->leaf[1] = surf;
  return LSLAM_OK;
}

int lslam_lmap_add_data_frame(lslam_lmap *lm, const void *corner, size_t n_corner, const void *surf, size_t n_surf, size_t stride_bytes,
                              const float T_map[16]) {
  return add_impl(lm, corner, n_corner, surf, n_surf, stride_bytes, T_map, true);
}

int lslam_lmap_add_data_frame_device(lslam_lmap *lm, const void *d_corner, size_t n_corner, const void *d_surf, size_t n_surf,
                                     const float T_map[16]) {
  return add_impl(lm, d_corner, n_corner, d_surf, n_surf, sizeof(float4), T_map, false);
}

int lslam_lmap_surround_to_map_counts(lslam_lmap *lm, size_t *n_corner, size_t *n_surf) {
  if (n_corner) *n_corner = 0;
  if (n_surf) *n_surf = 0;
  int rc = check_lm(lm, "lslam_lmap_surround_to_map_counts");
  if (rc) return rc;
  rc = ensure_surround(lm);
  if (rc) return rc;
  if (n_corner) *n_corner = lm->n_sur[0];
  if (n_surf) *n_surf = lm->n_sur[1];
  if (lm->n_sur[0] == 0 && lm->n_sur[1] == 0) return lslam_map_set(lm->ctx, nullptr, 0, nullptr, 0, 16);
  return lslam::map_set_device(lm->ctx, lm->mapp[0].p, lm->n_sur[0], lm->mapp[1].p, lm->n_sur[1], lm->sur_lo, lm->sur_hi);
}

int lslam_lmap_get_surround(lslam_lmap *lm, float *corner_xyzi, size_t cap_c, size_t *n_c, float *surf_xyzi, size_t cap_s, size_t *n_s) {
  if (n_c) *n_c = 0;
  if (n_s) *n_s = 0;
  int rc = check_lm(lm, "lslam_lmap_get_surround");
  if (rc) return rc;
  rc = ensure_surround(lm);
  if (rc) return rc;
  if (n_c) *n_c = lm->n_sur[0];
  if (n_s) *n_s = lm->n_sur[1];
  float *dst[2] = {corner_xyzi, surf_xyzi};
  const size_t cap[2] = {cap_c, cap_s};
  bool any = false;
  for (int t = 0; t < 2; ++t) {
    if (!dst[t]) continue;  // counts only
    if (lm->n_sur[t] > cap[t]) {
      lslam::set_error("lslam_lmap_get_surround: output buffer too small");
      return LSLAM_ERR_INVALID;
    }
    if (lm->n_sur[t]) {
      LSLAM_TRY(hipMemcpyAsync(dst[t], lm->filt[t].p, lm->n_sur[t] * sizeof(float4), hipMemcpyDeviceToHost, lm->stream));
      any = true;
    }
  }
  if (any) LSLAM_TRY(hipStreamSynchronize(lm->stream));
  return LSLAM_OK;
}

int lslam_lmap_info(lslam_lmap *lm, int32_t *n_frames, double *accum_distance, size_t live_points[2], int64_t *frames_evicted) {
  const int rc = check_lm(lm, "lslam_lmap_info");
  if (rc) return rc;
  if (n_frames) *n_frames = (int32_t)lm->frames.size();
  if (accum_distance) *accum_distance = lm->accum;
  if (live_points) { live_points[0] = lm->live[0]; live_points[1] = lm->live[1]; }
  if (frames_evicted) *frames_evicted = lm->evicted;
  return LSLAM_OK;
}

int lslam_lmap_get_frames(lslam_lmap *lm, int32_t cap_frames, int32_t *n_frames, double *accum, int32_t *counts, float *corner_xyzi,
                          size_t cap_c, float *surf_xyzi, size_t cap_s) {
  if (n_frames) *n_frames = 0;
  int rc = check_lm(lm, "lslam_lmap_get_frames");
  if (rc) return rc;
  const size_t nf = lm->frames.size();
  if (n_frames) *n_frames = (int32_t)nf;
  if ((accum || counts) && (cap_frames < 0 || (size_t)cap_frames < nf)) {
    lslam::set_error("lslam_lmap_get_frames: frame tables too small");
    return LSLAM_ERR_INVALID;
  }
  if ((corner_xyzi && cap_c < lm->live[0]) || (surf_xyzi && cap_s < lm->live[1])) {
    lslam::set_error("lslam_lmap_get_frames: point buffer too small");
    return LSLAM_ERR_INVALID;
  }
  for (size_t k = 0; k < nf; ++k) {
    if (accum) accum[k] = lm->frames[k].accum;
    if (counts) { counts[2 * k] = (int32_t)lm->frames[k].count[0]; counts[2 * k + 1] = (int32_t)lm->frames[k].count[1]; }
  }
  float *dst[2] = {corner_xyzi, surf_xyzi};
  bool any = false;
  for (int t = 0; t < 2; ++t) {
    if (!dst[t] || !lm->live[t]) continue;
    rc = gather_ring(lm, t, lm->gath[t].p);
    if (rc) return rc;
    LSLAM_TRY(hipMemcpyAsync(dst[t], lm->gath[t].p, lm->live[t] * sizeof(float4), hipMemcpyDeviceToHost, lm->stream));
    any = true;
  }
  if (any) LSLAM_TRY(hipStreamSynchronize(lm->stream));
  return LSLAM_OK;
}

int lslam_lmap_stats(lslam_lmap *lm, int64_t *merged, int64_t *resorted, int64_t *refiltered) {
  const int rc = check_lm(lm, "lslam_lmap_stats");
  if (rc) return rc;
  if (merged) *merged = lm->n_merged;
  if (resorted) *resorted = lm->n_resorted;
  if (refiltered) *refiltered = lm->n_refiltered;
  return LSLAM_OK;
}

int lslam_lmap_clear(lslam_lmap *lm) {
  const int rc = check_lm(lm, "lslam_lmap_clear");
  if (rc) return rc;
  LSLAM_TRY(hipStreamSynchronize(lm->stream));
  reset_state(lm);
  return LSLAM_OK;
}

}  // extern "C"
