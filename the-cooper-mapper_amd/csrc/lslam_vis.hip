// lslam_vis.hip -- visibility votes over the keyframe store: a coarse range image per keyframe and, per query point, the count of
// keyframes that looked through the place where it is ("free") or saw a surface there ("hit") -- lslam_vis_* of
// include/lslam_c.h, whose comment is the specification; DESIGN 8g.  Not in the reference: its addFeatureCloud only voxel-filters.
//
// Kernels:
//   vis_fill_kernel     +inf into the images of the keyframes that are about to get one.
//   vis_image_kernel    grid (point tiles, keyframes).  One point per lane, corner cloud then surf cloud where they lie in the
//                       store's slabs; the pixel's range goes in with an integer atomic min on its bit pattern (ranges are > 0, so
//                       the orderings agree, and a minimum does not depend on arrival order).
//   vis_vote_kernel     grid (tiles of LSLAM_VIS_POINT_TILE query points, chunks of LSLAM_VIS_KF_CHUNK voters).  A lane keeps its
//                       point in registers for the whole chunk; the voter index is the same in every lane, so the inverse pose and
//                       the image pointer come through scalar loads; the fp32 range gate runs before any atan2; the window's pixels
//                       are read through L2 (an image is 23 KB at 16 x 360).  Votes accumulate in registers and leave through ONE
//                       integer atomicAdd of n_free | n_hit << 16 per point and chunk.
//   vis_count / _scan / _scatter_kernel   the stable compaction of the points that are not dynamic: per-workgroup counts, their
//                       exclusive scan by one workgroup, the scatter (rank inside a workgroup by ballot and popcount).
// Only integer min / add combine values across lanes: nothing depends on arrival order, two calls give the same bits.
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

using lslam::VisJob;
using lslam::VisState;
using lslam::check_id;
using lslam::check_kfs;

constexpr int VIS_BLOCK = 256;
constexpr int VIS_CHUNK = LSLAM_VIS_KF_CHUNK;
static_assert(LSLAM_VIS_POINT_TILE == VIS_BLOCK, "one query point per lane");
constexpr int32_t VIS_MAX_IDS = 65535;          // n_free and n_hit fit 16 bits each
constexpr size_t VIS_MAX_POINTS = 0x7fffffffu;  // of a call
constexpr size_t VIS_SLAB_FLOATS = (size_t)1 << 21;  // 8 MiB: 364 images of 16 x 360
constexpr uint32_t VIS_INF_BITS = 0x7f800000u;
constexpr double VIS_PI = 3.141592653589793, VIS_TWO_PI = 6.283185307179586;

struct VisShape {
  int32_t n_row, n_col, window, up_axis;
  float min_range, max_range, abs_margin, rel_margin;
  double el0, row_scale, col_scale;
};
struct VisMove {  // the query points' own transform (lslam_vis_add_to_fmap), rows of [R | t]
  float T[12];
  int32_t use;
};

// ((T0 x + T1 y) + T2 z) + T3 per row, every product and sum rounded on its own (lslam::rigid_transform_point's formula)
__device__ __forceinline__ void vis_move(const float *T, float x, float y, float z, float &ox, float &oy, float &oz) {
  ox = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[0], x), __fmul_rn(T[1], y)), __fmul_rn(T[2], z)), T[3]);
  oy = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[4], x), __fmul_rn(T[5], y)), __fmul_rn(T[6], z)), T[7]);
  oz = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[8], x), __fmul_rn(T[9], y)), __fmul_rn(T[10], z)), T[11]);
}

// The pixel of a point in a sensor frame (the header's PIXEL); false: not observable.  0 <= row < n_row, 0 <= col < n_col.
__device__ __forceinline__ bool vis_pixel(const VisShape &sh, float x, float y, float z, float &r, int &row, int &col) {
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
  const float a = sh.up_axis == 1 ? z : x, b = sh.up_axis == 1 ? x : y, h = sh.up_axis == 1 ? y : z;
  const float d2 = __fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b));
  r = sqrtf(__fadd_rn(d2, __fmul_rn(h, h)));
  if (!(r >= sh.min_range && r <= sh.max_range)) return false;  // the cheap gate (an overflowed r = inf included), before any atan2
  const float rho = sqrtf(d2);
  const double rowd = (atan2((double)h, (double)rho) - sh.el0) * sh.row_scale;
  if (!(rowd >= 0.0 && rowd < (double)sh.n_row)) return false;
  row = (int)rowd;
  double ang = atan2((double)b, (double)a);
  if (ang < 0.0) ang += VIS_TWO_PI;
  col = (int)(ang * sh.col_scale);  // (ang >= 0: col >= 0)
  if (col > sh.n_col - 1) col = sh.n_col - 1;
  return true;
}

__global__ __launch_bounds__(VIS_BLOCK) void vis_fill_kernel(const VisJob *jobs, size_t stride, size_t total) {
  for (size_t i = (size_t)blockIdx.x * VIS_BLOCK + threadIdx.x; i < total; i += (size_t)gridDim.x * VIS_BLOCK)
    reinterpret_cast<uint32_t *>(jobs[i / stride].img)[i % stride] = VIS_INF_BITS;  // (i / stride < the jobs of the launch)
}

__global__ __launch_bounds__(VIS_BLOCK) void vis_image_kernel(const VisJob *jobs, uint32_t n_jobs, const VisShape sh) {
  for (uint32_t j = blockIdx.y; j < n_jobs; j += gridDim.y) {
    const VisJob job = jobs[j];
    const uint32_t i = blockIdx.x * VIS_BLOCK + threadIdx.x;
    if (i >= job.n[0] + job.n[1]) continue;
    const float4 p = i < job.n[0] ? job.p[0][i] : job.p[1][i - job.n[0]];
    float r;
    int row, col;
    if (!vis_pixel(sh, p.x, p.y, p.z, r, row, col)) continue;
    atomicMin(reinterpret_cast<uint32_t *>(job.img) + (size_t)row * sh.n_col + col, __builtin_bit_cast(uint32_t, r));
  }
}

__global__ __launch_bounds__(VIS_BLOCK) void vis_vote_kernel(const float4 *__restrict__ pts, uint32_t n, const VisMove mv,
                                                              const float *__restrict__ inv, const float *const *__restrict__ imgs,
                                                              uint32_t n_ids, const VisShape sh, uint32_t *votes) {
  const uint32_t i = blockIdx.x * VIS_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t k0 = blockIdx.y * VIS_CHUNK, k1 = k0 + VIS_CHUNK < n_ids ? k0 + VIS_CHUNK : n_ids;
  float qx, qy, qz;
  {
    const float4 q = pts[i];
    qx = q.x, qy = q.y, qz = q.z;
    if (mv.use) vis_move(mv.T, q.x, q.y, q.z, qx, qy, qz);
  }
  const int W = sh.n_col, w = sh.window;
  uint32_t n_free = 0, n_hit = 0;
  for (uint32_t k = k0; k < k1; ++k) {  // k is the same in every lane: M and img are scalar loads
    const float *M = inv + 12 * (size_t)k;
    const float *img = imgs[k];
    float x, y, z, r;
    vis_move(M, qx, qy, qz, x, y, z);
    int row, col;
    if (!vis_pixel(sh, x, y, z, r, row, col)) continue;
    const float m = fmaxf(sh.abs_margin, __fmul_rn(sh.rel_margin, r));
    const float beyond = __fadd_rn(r, m);
    const bool centre = __builtin_bit_cast(uint32_t, img[(size_t)row * W + col]) != VIS_INF_BITS;
    bool all_beyond = true, hit = false;
    for (int dr = -w; dr <= w; ++dr) {
      const int rr = row + dr;
      if (rr < 0 || rr >= sh.n_row) continue;
      for (int dc = -w; dc <= w; ++dc) {
        int cc = col + dc;  // window <= 3 < n_col: one wrap is enough
        if (cc < 0) cc += W;
        else if (cc >= W) cc -= W;
        const float v = img[(size_t)rr * W + cc];  // (0 <= rr < n_row, 0 <= cc < n_col)
        if (__builtin_bit_cast(uint32_t, v) == VIS_INF_BITS) continue;
        all_beyond = all_beyond && v > beyond;
        hit = hit || fabsf(__fsub_rn(v, r)) <= m;
      }
    }
    n_free += (centre && all_beyond) ? 1u : 0u;
    n_hit += hit ? 1u : 0u;
  }
  const uint32_t word = n_free | (n_hit << 16);
  if (word) atomicAdd(&votes[i], word);
}

__device__ __forceinline__ bool vis_kept(uint32_t word, uint32_t min_free) {
  const uint32_t n_free = word & 0xffffu, n_hit = word >> 16;
  return !(n_free >= min_free && n_free > n_hit);
}

// rank of this lane among the workgroup's lanes with `keep`, and their number; every lane of the workgroup calls it
__device__ __forceinline__ uint32_t vis_block_rank(bool keep, uint32_t *total) {
  __shared__ uint32_t wave_sum[VIS_BLOCK / 64];
  const unsigned long long mask = __ballot(keep);
  const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
  const uint32_t below = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
  __syncthreads();  // (the previous use of wave_sum has been read)
  if (lane == 0) wave_sum[wv] = (uint32_t)__popcll(mask);
  __syncthreads();
  uint32_t off = 0, sum = 0;
  for (int j = 0; j < VIS_BLOCK / 64; ++j) {
    off += j < wv ? wave_sum[j] : 0u;
    sum += wave_sum[j];
  }
  *total = sum;
  return off + below;
}

__global__ __launch_bounds__(VIS_BLOCK) void vis_count_kernel(const uint32_t *votes, uint32_t n, uint32_t min_free, uint32_t *counts) {
  const uint32_t i = blockIdx.x * VIS_BLOCK + threadIdx.x;
  uint32_t total;
  (void)vis_block_rank(i < n && vis_kept(votes[i < n ? i : 0], min_free), &total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// counts[0 .. nb) -> their exclusive scan, counts[nb] = the total; one workgroup
__global__ __launch_bounds__(VIS_BLOCK) void vis_scan_kernel(uint32_t *counts, uint32_t nb) {
  __shared__ uint32_t s[VIS_BLOCK];
  __shared__ uint32_t carry;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (uint32_t base = 0; base < nb; base += VIS_BLOCK) {
    const uint32_t idx = base + tid;
    const uint32_t v = idx < nb ? counts[idx] : 0u;
    s[tid] = v;
    __syncthreads();
    for (uint32_t d = 1; d < VIS_BLOCK; d <<= 1) {
      const uint32_t t = tid >= d ? s[tid - d] : 0u;
      __syncthreads();
      s[tid] += t;
      __syncthreads();
    }
    const uint32_t before = carry, incl = s[tid];
    if (idx < nb) counts[idx] = before + incl - v;
    __syncthreads();
    if (tid == VIS_BLOCK - 1) carry = before + incl;
    __syncthreads();
  }
  if (tid == 0) counts[nb] = carry;
}

__global__ __launch_bounds__(VIS_BLOCK) void vis_scatter_kernel(const float4 *src, const uint32_t *votes, uint32_t n, uint32_t min_free,
                                                                 const uint32_t *offsets, float4 *out) {
  const uint32_t i = blockIdx.x * VIS_BLOCK + threadIdx.x;
  const bool keep = i < n && vis_kept(votes[i < n ? i : 0], min_free);
  uint32_t total;
  const uint32_t rank = vis_block_rank(keep, &total);
  if (keep) out[offsets[blockIdx.x] + rank] = src[i];  // (offset + rank < the kept points so far <= i: inside room for n)
}

int vis_ready(lslam_kfs *k, const char *what) {
  if (!k->vis.set) {
    char b[200];
    snprintf(b, sizeof(b), "%s: lslam_vis_setup was not called on this store", what);
    lslam::set_error(b);
    return LSLAM_ERR_INVALID;
  }
  return LSLAM_OK;
}

VisShape vis_shape(const VisState &v) {
  VisShape sh{};
  sh.n_row = v.params.n_row;
  sh.n_col = v.params.n_col;
  sh.window = v.params.window;
  sh.up_axis = v.params.up_axis;
  sh.min_range = v.params.min_range;
  sh.max_range = v.params.max_range;
  sh.abs_margin = v.params.abs_margin;
  sh.rel_margin = v.params.rel_margin;
  sh.el0 = v.el0;
  sh.row_scale = v.row_scale;
  sh.col_scale = v.col_scale;
  return sh;
}

// the voters of a call: everything that can be refused, before anything runs
int vis_check_voters(lslam_kfs *k, const char *what, int32_t n_ids, const int32_t *ids, const float *poses) {
  char b[240];
  if (n_ids < 0 || n_ids > VIS_MAX_IDS || (n_ids && (!ids || !poses))) {
    snprintf(b, sizeof(b), "%s: n_ids outside 0 .. %d, or null ids / poses", what, VIS_MAX_IDS);
    lslam::set_error(b);
    return LSLAM_ERR_INVALID;
  }
  for (int32_t i = 0; i < n_ids; ++i) {
    const int rc = check_id(k, what, ids[i]);
    if (rc) return rc;
    for (int e = 0; e < 12; ++e)
      if (!std::isfinite(poses[16 * (size_t)i + e])) {
        snprintf(b, sizeof(b), "%s: pose %d is not finite", what, i);
        lslam::set_error(b);
        return LSLAM_ERR_INVALID;
      }
  }
  return LSLAM_OK;
}

// Every keyframe without an image gets one, in one launch behind the fill (enqueued, not waited for).
int vis_images_pending(lslam_kfs *k) {
  VisState &v = k->vis;
  const size_t n = k->kfs.size();
  if (v.imaged >= n) return LSLAM_OK;
  const size_t want_slabs = (n + v.slab_kf - 1) / v.slab_kf;
  while (v.slabs.size() < want_slabs) {
    std::unique_ptr<lslam::DevBuf<float>> s(new lslam::DevBuf<float>());
    const hipError_t e = s->alloc(v.slab_kf * v.stride);
    if (e != hipSuccess) {
      char b[200];
      snprintf(b, sizeof(b), "visibility: an image slab could not be allocated: %s", hipGetErrorString(e));
      lslam::set_error(b);
      return LSLAM_ERR_HIP;
    }
    v.slabs.push_back(std::move(s));
  }
  const size_t m = n - v.imaged;
  LSLAM_TRY(v.h_jobs.reserve(m));
  LSLAM_TRY(v.d_jobs.reserve(m));
  size_t most = 1;
  for (size_t i = 0; i < m; ++i) {
    const lslam::KeyframeClouds &kc = k->kfs[v.imaged + i];
    VisJob j{};
    for (int t = 0; t < 2; ++t) {
      j.p[t] = kc.p[t];
      j.n[t] = (uint32_t)kc.n[t];
    }
    j.img = v.image(v.imaged + i);
    v.h_jobs.p[i] = j;
    if (kc.n[0] + kc.n[1] > most) most = kc.n[0] + kc.n[1];
  }
  LSLAM_TRY(hipMemcpyAsync(v.d_jobs.p, v.h_jobs.p, m * sizeof(VisJob), hipMemcpyHostToDevice, k->stream));
  const size_t total = m * v.stride;
  const size_t fill_blocks = (total + VIS_BLOCK - 1) / VIS_BLOCK;
  hipLaunchKernelGGL(vis_fill_kernel, dim3((unsigned)(fill_blocks < 65536 ? fill_blocks : 65536)), dim3(VIS_BLOCK), 0, k->stream,
                     v.d_jobs.p, v.stride, total);
  LSLAM_TRY(hipGetLastError());
  hipLaunchKernelGGL(vis_image_kernel, dim3((unsigned)((most + VIS_BLOCK - 1) / VIS_BLOCK), (unsigned)(m < 65535 ? m : 65535)),
                     dim3(VIS_BLOCK), 0, k->stream, v.d_jobs.p, (uint32_t)m, vis_shape(v));
  LSLAM_TRY(hipGetLastError());
  // (h_jobs is rewritten by the next build only: every caller waits for the stream before it returns)
  v.imaged = n;
  ++v.image_launches;
  return LSLAM_OK;
}

// The voters' images and inverse poses to the device (enqueued): (R^T, -R^T t) in fp64, rounded to fp32.
int vis_upload_voters(lslam_kfs *k, int32_t n_ids, const int32_t *ids, const float *poses) {
  VisState &v = k->vis;
  if (!n_ids) return LSLAM_OK;
  const size_t m = (size_t)n_ids;
  LSLAM_TRY(v.h_in.reserve(12 * m));
  LSLAM_TRY(v.d_inv.reserve(12 * m));
  LSLAM_TRY(v.h_img.reserve(m));
  LSLAM_TRY(v.d_img.reserve(m));
  for (size_t i = 0; i < m; ++i) {
    const float *T = poses + 16 * i;
    float *o = v.h_in.p + 12 * i;
    const double t0 = T[3], t1 = T[7], t2 = T[11];
    for (int j = 0; j < 3; ++j) {
      const double r0 = T[j], r1 = T[4 + j], r2 = T[8 + j];  // column j of R: row j of R^T
      o[4 * j + 0] = (float)r0;
      o[4 * j + 1] = (float)r1;
      o[4 * j + 2] = (float)r2;
      o[4 * j + 3] = (float)-((r0 * t0 + r1 * t1) + r2 * t2);
    }
    v.h_img.p[i] = v.image((size_t)ids[i]);
  }
  LSLAM_TRY(hipMemcpyAsync(v.d_inv.p, v.h_in.p, 12 * m * sizeof(float), hipMemcpyHostToDevice, k->stream));
  LSLAM_TRY(hipMemcpyAsync(v.d_img.p, v.h_img.p, m * sizeof(const float *), hipMemcpyHostToDevice, k->stream));
  return LSLAM_OK;
}

// votes[n] = 0, then the vote kernel (enqueued).  T: the query points' own transform, or nullptr.
int vis_launch_votes(lslam_kfs *k, const float4 *d_pts, size_t n, const float *T, int32_t n_ids, uint32_t *d_votes, bool counted) {
  VisState &v = k->vis;
  if (!n) return LSLAM_OK;
  LSLAM_TRY(hipMemsetAsync(d_votes, 0, n * sizeof(uint32_t), k->stream));
  if (!n_ids) return LSLAM_OK;
  VisMove mv{};
  if (T) {
    std::memcpy(mv.T, T, 12 * sizeof(float));
    mv.use = 1;
  }
  const dim3 grid((unsigned)((n + VIS_BLOCK - 1) / VIS_BLOCK), (unsigned)((n_ids + VIS_CHUNK - 1) / VIS_CHUNK));
  hipLaunchKernelGGL(vis_vote_kernel, grid, dim3(VIS_BLOCK), 0, k->stream, d_pts, (uint32_t)n, mv, v.d_inv.p, v.d_img.p, (uint32_t)n_ids,
                     vis_shape(v), d_votes);
  LSLAM_TRY(hipGetLastError());
  if (counted) ++v.vote_launches;
  return LSLAM_OK;
}

// The stable compaction of src's kept points into out (enqueued); the count lands in d_block[block_at + blocks].
int vis_launch_compact(lslam_kfs *k, const float4 *src, const uint32_t *d_votes, size_t n, size_t block_at, float4 *out) {
  VisState &v = k->vis;
  const uint32_t nb = (uint32_t)((n + VIS_BLOCK - 1) / VIS_BLOCK), min_free = (uint32_t)v.params.min_free_votes;
  uint32_t *counts = v.d_block.p + block_at;
  if (!nb) {
    LSLAM_TRY(hipMemsetAsync(counts, 0, sizeof(uint32_t), k->stream));
    return LSLAM_OK;
  }
  hipLaunchKernelGGL(vis_count_kernel, dim3(nb), dim3(VIS_BLOCK), 0, k->stream, d_votes, (uint32_t)n, min_free, counts);
  LSLAM_TRY(hipGetLastError());
  hipLaunchKernelGGL(vis_scan_kernel, dim3(1), dim3(VIS_BLOCK), 0, k->stream, counts, nb);
  LSLAM_TRY(hipGetLastError());
  hipLaunchKernelGGL(vis_scatter_kernel, dim3(nb), dim3(VIS_BLOCK), 0, k->stream, src, d_votes, (uint32_t)n, min_free, counts, out);
  LSLAM_TRY(hipGetLastError());
  return LSLAM_OK;
}

// an error after work was enqueued: the stream is drained before the caller gets its buffers back
int vis_fail(lslam_kfs *k, int rc) {
  (void)hipStreamSynchronize(k->stream);
  return rc;
}

int vis_entry(lslam_kfs *k, const char *what, int32_t n_ids, const int32_t *ids, const float *poses) {
  int rc = check_kfs(k, what);
  if (rc) return rc;
  rc = vis_ready(k, what);
  if (rc) return rc;
  return vis_check_voters(k, what, n_ids, ids, poses);
}

size_t vis_blocks(size_t n) { return (n + VIS_BLOCK - 1) / VIS_BLOCK; }

}  // namespace

extern "C" {

void lslam_vis_default_params(lslam_vis_params *p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->n_row = 16;
  p->n_col = 360;
  p->fov_down_deg = -16.0f;
  p->fov_up_deg = 16.0f;
  p->min_range = 1.0f;
  p->max_range = 80.0f;
  p->window = 1;
  p->abs_margin = 0.5f;
  p->rel_margin = 0.02f;
  p->min_free_votes = 2;
  p->up_axis = 1;
}

size_t lslam_sizeof_vis_params(void) { return sizeof(lslam_vis_params); }
size_t lslam_sizeof_vis_stats(void) { return sizeof(lslam_vis_stats); }

int lslam_vis_setup(lslam_kfs *k, const lslam_vis_params *params) {
  const int rc = check_kfs(k, "lslam_vis_setup");
  if (rc) return rc;
  lslam_vis_params p;
  lslam_vis_default_params(&p);
  if (params) p = *params;
  char b[240];
  b[0] = 0;
  if (p.n_row < 1 || p.n_row > 128) snprintf(b, sizeof(b), "lslam_vis_setup: n_row %d outside 1 .. 128", p.n_row);
  else if (p.n_col < 4 || p.n_col > 4096) snprintf(b, sizeof(b), "lslam_vis_setup: n_col %d outside 4 .. 4096", p.n_col);
  else if (!std::isfinite(p.fov_down_deg) || p.fov_down_deg < -90.0f || p.fov_down_deg > 90.0f)
    snprintf(b, sizeof(b), "lslam_vis_setup: fov_down_deg %g is not within [-90, 90]", (double)p.fov_down_deg);
  else if (!std::isfinite(p.fov_up_deg) || p.fov_up_deg < -90.0f || p.fov_up_deg > 90.0f || !(p.fov_down_deg < p.fov_up_deg))
    snprintf(b, sizeof(b), "lslam_vis_setup: fov_up_deg %g is not within (fov_down_deg, 90]", (double)p.fov_up_deg);
  else if (!(p.min_range > 0.0f) || !std::isfinite(p.min_range))
    snprintf(b, sizeof(b), "lslam_vis_setup: min_range %g is not a positive finite length", (double)p.min_range);
  else if (!(p.max_range > p.min_range) || !std::isfinite(p.max_range))
    snprintf(b, sizeof(b), "lslam_vis_setup: max_range %g is not a finite length above min_range", (double)p.max_range);
  else if (p.window < 0 || p.window > 3) snprintf(b, sizeof(b), "lslam_vis_setup: window %d outside 0 .. 3", p.window);
  else if (!(p.abs_margin >= 0.0f) || !std::isfinite(p.abs_margin))
    snprintf(b, sizeof(b), "lslam_vis_setup: abs_margin %g is negative or not finite", (double)p.abs_margin);
  else if (!(p.rel_margin >= 0.0f) || !std::isfinite(p.rel_margin))
    snprintf(b, sizeof(b), "lslam_vis_setup: rel_margin %g is negative or not finite", (double)p.rel_margin);
  else if (p.min_free_votes < 1) snprintf(b, sizeof(b), "lslam_vis_setup: min_free_votes %d below 1", p.min_free_votes);
  else if (p.up_axis != 1 && p.up_axis != 2) snprintf(b, sizeof(b), "lslam_vis_setup: up_axis %d is neither 1 (y up) nor 2 (z up)", p.up_axis);
  if (b[0]) {
    lslam::set_error(b);
    return LSLAM_ERR_INVALID;
  }
  VisState &v = k->vis;
  if (v.set && std::memcmp(&v.params, &p, sizeof(p)) == 0) return LSLAM_OK;
  LSLAM_TRY(hipStreamSynchronize(k->stream));
  v.drop();
  v.params = p;
  v.el0 = (double)p.fov_down_deg * VIS_PI / 180.0;
  v.row_scale = (double)p.n_row / (((double)p.fov_up_deg - (double)p.fov_down_deg) * VIS_PI / 180.0);
  v.col_scale = (double)p.n_col / VIS_TWO_PI;
  v.stride = (size_t)p.n_row * (size_t)p.n_col;
  v.slab_kf = VIS_SLAB_FLOATS / v.stride;
  if (v.slab_kf < 1) v.slab_kf = 1;
  if (v.slab_kf > 1024) v.slab_kf = 1024;
  v.set = true;
  return LSLAM_OK;
}

int lslam_vis_info(lslam_kfs *k, lslam_vis_stats *out) {
  if (out) std::memset(out, 0, sizeof(*out));
  const int rc = check_kfs(k, "lslam_vis_info");
  if (rc) return rc;
  if (!out) {
    lslam::set_error("lslam_vis_info: null out");
    return LSLAM_ERR_INVALID;
  }
  const VisState &v = k->vis;
  if (v.set) out->params = v.params;
  out->is_set = v.set ? 1 : 0;
  out->n_images = (int64_t)v.imaged;
  out->image_bytes = (uint64_t)v.bytes_held();
  out->image_launches = v.image_launches;
  out->vote_launches = v.vote_launches;
  return LSLAM_OK;
}

int lslam_vis_range_image(lslam_kfs *k, int32_t id, float *out) {
  int rc = check_kfs(k, "lslam_vis_range_image");
  if (rc) return rc;
  rc = vis_ready(k, "lslam_vis_range_image");
  if (rc) return rc;
  rc = check_id(k, "lslam_vis_range_image", id);
  if (rc) return rc;
  if (!out) {
    lslam::set_error("lslam_vis_range_image: null out");
    return LSLAM_ERR_INVALID;
  }
  rc = vis_images_pending(k);
  if (rc) return vis_fail(k, rc);
  VisState &v = k->vis;
  LSLAM_TRY(hipMemcpyAsync(out, v.image((size_t)id), v.stride * sizeof(float), hipMemcpyDeviceToHost, k->stream));
  LSLAM_TRY(hipStreamSynchronize(k->stream));
  return LSLAM_OK;
}

int lslam_vis_votes(lslam_kfs *k, int32_t n_ids, const int32_t *ids, const float *poses, const void *points, size_t n,
                    size_t stride_bytes, uint32_t *votes_out) {
  int rc = vis_entry(k, "lslam_vis_votes", n_ids, ids, poses);
  if (rc) return rc;
  if (n > VIS_MAX_POINTS || (n && (!points || !votes_out)) || stride_bytes < 16 || (stride_bytes & 3)) {
    lslam::set_error("lslam_vis_votes: more than 2^31 - 1 points, null points or votes, or a stride under 16 bytes");
    return LSLAM_ERR_INVALID;
  }
  VisState &v = k->vis;
  v.last_n = 0;
  if (!n) return LSLAM_OK;
  LSLAM_TRY(v.h_pts.reserve(n));
  LSLAM_TRY(v.d_pts.reserve(n));
  LSLAM_TRY(v.d_votes.reserve(n));
  LSLAM_TRY(v.h_votes.reserve(n));
  const char *src = static_cast<const char *>(points);
  for (size_t i = 0; i < n; ++i) {
    float c[3];
    std::memcpy(c, src + i * stride_bytes, 12);
    v.h_pts.p[i] = make_float4(c[0], c[1], c[2], 0.0f);
  }
  rc = vis_images_pending(k);
  if (rc) return vis_fail(k, rc);
  rc = vis_upload_voters(k, n_ids, ids, poses);
  if (rc) return vis_fail(k, rc);
  LSLAM_TRY(hipMemcpyAsync(v.d_pts.p, v.h_pts.p, n * sizeof(float4), hipMemcpyHostToDevice, k->stream));
  rc = vis_launch_votes(k, v.d_pts.p, n, nullptr, n_ids, v.d_votes.p, true);
  if (rc) return vis_fail(k, rc);
  LSLAM_TRY(hipMemcpyAsync(v.h_votes.p, v.d_votes.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, k->stream));
  LSLAM_TRY(hipStreamSynchronize(k->stream));
  std::memcpy(votes_out, v.h_votes.p, n * sizeof(uint32_t));
  v.last_n = n;
  v.last_ids = n_ids;
  return LSLAM_OK;
}

int lslam_vis_votes_device(lslam_kfs *k, int32_t n_ids, const int32_t *ids, const float *poses, const float *d_xyzi, size_t n,
                           uint32_t *d_votes) {
  int rc = vis_entry(k, "lslam_vis_votes_device", n_ids, ids, poses);
  if (rc) return rc;
  if (n > VIS_MAX_POINTS || (n && (!d_xyzi || !d_votes))) {
    lslam::set_error("lslam_vis_votes_device: more than 2^31 - 1 points, or null points or votes");
    return LSLAM_ERR_INVALID;
  }
  k->vis.last_n = 0;
  if (!n) return LSLAM_OK;
  rc = vis_images_pending(k);
  if (rc) return vis_fail(k, rc);
  rc = vis_upload_voters(k, n_ids, ids, poses);
  if (rc) return vis_fail(k, rc);
  rc = vis_launch_votes(k, reinterpret_cast<const float4 *>(d_xyzi), n, nullptr, n_ids, d_votes, true);
  if (rc) return vis_fail(k, rc);
  LSLAM_TRY(hipStreamSynchronize(k->stream));
  return LSLAM_OK;
}

int lslam_vis_filter_device(lslam_kfs *k, int32_t n_ids, const int32_t *ids, const float *poses, const float *d_xyzi, size_t n,
                            float *d_out, size_t *n_kept) {
  int rc = vis_entry(k, "lslam_vis_filter_device", n_ids, ids, poses);
  if (rc) return rc;
  if (n > VIS_MAX_POINTS || !n_kept || (n && (!d_xyzi || !d_out))) {
    lslam::set_error("lslam_vis_filter_device: more than 2^31 - 1 points, or null points, output or n_kept");
    return LSLAM_ERR_INVALID;
  }
  VisState &v = k->vis;
  v.last_n = 0;
  *n_kept = 0;
  if (!n) return LSLAM_OK;
  LSLAM_TRY(v.d_votes.reserve(n));
  LSLAM_TRY(v.d_block.reserve(vis_blocks(n) + 1));
  LSLAM_TRY(v.h_count.reserve(2));
  rc = vis_images_pending(k);
  if (rc) return vis_fail(k, rc);
  rc = vis_upload_voters(k, n_ids, ids, poses);
  if (rc) return vis_fail(k, rc);
  const float4 *src = reinterpret_cast<const float4 *>(d_xyzi);
  rc = vis_launch_votes(k, src, n, nullptr, n_ids, v.d_votes.p, true);
  if (rc) return vis_fail(k, rc);
  rc = vis_launch_compact(k, src, v.d_votes.p, n, 0, reinterpret_cast<float4 *>(d_out));
  if (rc) return vis_fail(k, rc);
  LSLAM_TRY(hipMemcpyAsync(v.h_count.p, v.d_block.p + vis_blocks(n), sizeof(uint32_t), hipMemcpyDeviceToHost, k->stream));
  LSLAM_TRY(hipStreamSynchronize(k->stream));
  *n_kept = v.h_count.p[0];
  return LSLAM_OK;
}

int lslam_vis_add_to_fmap(lslam_kfs *k, int32_t id, lslam_fmap *fm, const float T[16], int32_t n_ids, const int32_t *ids,
                          const float *poses, size_t n_removed[2]) {
  int rc = vis_entry(k, "lslam_vis_add_to_fmap", n_ids, ids, poses);
  if (rc) return rc;
  rc = check_id(k, "lslam_vis_add_to_fmap", id);
  if (rc) return rc;
  if (!fm || !T) {
    lslam::set_error("lslam_vis_add_to_fmap: null feature map or null pose");
    return LSLAM_ERR_INVALID;
  }
  VisState &v = k->vis;
  v.last_n = 0;
  const lslam::KeyframeClouds kc = k->kfs[(size_t)id];
  const size_t nb[2] = {vis_blocks(kc.n[0]), vis_blocks(kc.n[1])};
  LSLAM_TRY(v.d_votes.reserve(kc.n[0] + kc.n[1] ? kc.n[0] + kc.n[1] : 1));
  LSLAM_TRY(v.d_block.reserve(nb[0] + nb[1] + 2));
  LSLAM_TRY(v.h_count.reserve(2));
  for (int t = 0; t < 2; ++t) LSLAM_TRY(v.d_keep[t].reserve(kc.n[t] ? kc.n[t] : 1));
  rc = vis_images_pending(k);
  if (rc) return vis_fail(k, rc);
  rc = vis_upload_voters(k, n_ids, ids, poses);
  if (rc) return vis_fail(k, rc);
  const size_t block_at[2] = {0, nb[0] + 1}, vote_at[2] = {0, kc.n[0]};
  for (int t = 0; t < 2; ++t) {
    rc = vis_launch_votes(k, kc.p[t], kc.n[t], T, n_ids, v.d_votes.p + vote_at[t], true);
    if (rc) return vis_fail(k, rc);
    rc = vis_launch_compact(k, kc.p[t], v.d_votes.p + vote_at[t], kc.n[t], block_at[t], v.d_keep[t].p);
    if (rc) return vis_fail(k, rc);
    LSLAM_TRY(hipMemcpyAsync(v.h_count.p + t, v.d_block.p + block_at[t] + nb[t], sizeof(uint32_t), hipMemcpyDeviceToHost, k->stream));
  }
  LSLAM_TRY(hipStreamSynchronize(k->stream));  // the two counts; the feature map may run on another context's stream
  const size_t kept[2] = {v.h_count.p[0], v.h_count.p[1]};
  if (n_removed) {
    n_removed[0] = kc.n[0] - kept[0];
    n_removed[1] = kc.n[1] - kept[1];
  }
  return lslam::fmap_add_feature_cloud_device(fm, v.d_keep[0].p, kept[0], v.d_keep[1].p, kept[1], T);
}

int lslam_debug_vis_votes(lslam_kfs *k, int32_t launches) {
  int rc = check_kfs(k, "lslam_debug_vis_votes");
  if (rc) return rc;
  rc = vis_ready(k, "lslam_debug_vis_votes");
  if (rc) return rc;
  VisState &v = k->vis;
  if (!v.last_n || !v.last_ids || launches < 0) {
    lslam::set_error("lslam_debug_vis_votes: no lslam_vis_votes call with points and voters has run last, or negative launches");
    return LSLAM_ERR_INVALID;
  }
  LSLAM_TRY(v.d_votes_again.reserve(v.last_n));
  for (int32_t i = 0; i < launches; ++i) {
    rc = vis_launch_votes(k, v.d_pts.p, v.last_n, nullptr, v.last_ids, v.d_votes_again.p, false);
    if (rc) return vis_fail(k, rc);
  }
  return LSLAM_OK;
}

}  // extern "C"
