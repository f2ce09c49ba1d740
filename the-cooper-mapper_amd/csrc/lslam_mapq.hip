// lslam_mapq.hip -- map quality on the device (include/lslam_c.h lslam_mapq_*): per point the covariance of its fixed-radius
// neighbourhood, from it the entropy and the plane variance, and their exact means over a map (MME, MPV).  The header is the
// specification; tests/map_quality_ref.py restates it in numpy.
//
// Shape of the work.  The sums are integers (units of 2^-16 m), so any order of summation gives the same bits.
//   box_kernel / sg_key_kernel / radix sort /  both clouds sorted by the key of their cell in ONE grid over the surface's
//   sg_gather_kernel                            bounding box, cell = radius * (1 + 1/1024); non-finite points sort behind: the
//                                               sorted search grid of lslam_pointgrid_dev.hpp, shared with the survey extractor
//   mq_probe_kernel                            one lane per query, in cell order (neighbouring lanes walk the same rows): the
//                                               nine rows of three cells around the query, ten integer sums
//   mq_tail_kernel                             one lane per query: the fp64 covariance, the Jacobi sweeps, three logarithms;
//                                               per-workgroup integer partials
//   mq_final_kernel                            the partials to the six aggregates: no atomics anywhere
// MEASURED AND NOT SHIPPED: a wavefront per run of x-adjacent cells that finds its nine candidate rows once, stages them
// through LDS in tiles and splits the (query, candidate) tests over its lanes.  On the bench's voxel-filtered map (one or two
// points per cell) such a wavefront holds a handful of queries and its fixed cost decides: 663 / 403 / 215 us for 587 k points
// at r = 0.15 / 0.3 / 0.6 against 164 / 186 / 214 us of the survey extractor's lane-per-query kernel, so the lane-per-query
// probe is the one kernel here (DESIGN 8h has both sets of numbers).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/lslam_c.h"
#include "lslam_internal.hpp"
#include "lslam_jacobi_dev.hpp"
#include "lslam_kfs_impl.hpp"
#include "lslam_pointgrid_dev.hpp"

namespace {

using lslam::DevBuf;
using lslam::SGrid;

constexpr int MQ_BLOCK = 256;
constexpr size_t MQ_MAX_POINTS = (size_t)1 << 25;
constexpr double ENTROPY_CONST = 4.2568155996140185;  // 1.5 * ln(2 pi e)
constexpr int NSUM = 9;
constexpr int NAGG = 6;  // n_defined, n_sparse, sum_entropy_q32, sum_plane_var_q30, sum_neighbors, max_neighbors

inline dim3 blocks_for(size_t n) { return dim3((unsigned)((n + MQ_BLOCK - 1) / MQ_BLOCK)); }

// ---- the neighbourhood sums --------------------------------------------------------------------------------------------------
struct ProbeArgs {
  SGrid g;                // the finite surface points in cell order
  const float4 *qpts;     // [nq] finite queries in key order
  int nq;
  float r2;
  int32_t *count;         // [nq] per sorted query
  long long *sums;        // [NSUM][stride]
  size_t stride;
};
__device__ __forceinline__ long long shfl_xor_ll(long long v, int m) {
  const int lo = __shfl_xor((int)(v & 0xffffffffll), m, 64), hi = __shfl_xor((int)(v >> 32), m, 64);
  return (long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo);
}

__global__ __launch_bounds__(MQ_BLOCK) void mq_probe_kernel(const ProbeArgs a) {
  const int i = blockIdx.x * MQ_BLOCK + threadIdx.x;
  if (i >= a.nq) return;
  const float4 q = a.qpts[i];
  int k = 0;
  long long s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0, s6 = 0, s7 = 0, s8 = 0;
  lslam::sg_probe27(a.g, q, [&](const float4 &p) {
    const float dx = __fsub_rn(p.x, q.x), dy = __fsub_rn(p.y, q.y), dz = __fsub_rn(p.z, q.z);
    const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    if (!(d2 < a.r2)) return;
    const int X = (int)rint(((double)p.x - (double)q.x) * 65536.0), Y = (int)rint(((double)p.y - (double)q.y) * 65536.0),
              Z = (int)rint(((double)p.z - (double)q.z) * 65536.0);
    ++k;
    s0 += X; s1 += Y; s2 += Z;
    s3 += (long long)X * X; s4 += (long long)X * Y; s5 += (long long)X * Z;
    s6 += (long long)Y * Y; s7 += (long long)Y * Z; s8 += (long long)Z * Z;
  });
  a.count[i] = k;
  a.sums[i] = s0; a.sums[a.stride + i] = s1; a.sums[2 * a.stride + i] = s2;
  a.sums[3 * a.stride + i] = s3; a.sums[4 * a.stride + i] = s4; a.sums[5 * a.stride + i] = s5;
  a.sums[6 * a.stride + i] = s6; a.sums[7 * a.stride + i] = s7; a.sums[8 * a.stride + i] = s8;
}

// ---- the per-point tail ------------------------------------------------------------------------------------------------------
struct TailArgs {
  const float4 *qpts;    // [nq_all] sorted queries (w: the caller's index); the first nq are finite
  int nq, nq_all;
  const int32_t *count;
  const long long *sums;
  size_t stride;
  int min_neighbors;
  double lambda_floor;
  double *out_l3, *out_h;  // (or null) in the caller's order
  int32_t *out_count;      // (or null)
  long long *partials;     // [blocks][NAGG]
};
__global__ __launch_bounds__(MQ_BLOCK) void mq_tail_kernel(const TailArgs a) {
  __shared__ long long red[MQ_BLOCK / 64][NAGG];
  const int i = blockIdx.x * MQ_BLOCK + threadIdx.x;
  long long agg[NAGG] = {0, 0, 0, 0, 0, 0};
  if (i < a.nq_all) {
    const uint32_t at = __float_as_uint(a.qpts[i].w);
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    double l0 = qnan, l1 = qnan, l2 = qnan, h = qnan;
    const int k = i < a.nq ? a.count[i] : 0;
    if (i < a.nq && k < a.min_neighbors) agg[1] = 1;
    if (i < a.nq && k >= a.min_neighbors) {
      const double K = (double)k, c1 = 1.0 / 65536.0, c2 = 1.0 / 4294967296.0;
      const double sx = (double)a.sums[i] * c1, sy = (double)a.sums[a.stride + i] * c1, sz = (double)a.sums[2 * a.stride + i] * c1;
      const double sxx = (double)a.sums[3 * a.stride + i] * c2, sxy = (double)a.sums[4 * a.stride + i] * c2,
                   sxz = (double)a.sums[5 * a.stride + i] * c2, syy = (double)a.sums[6 * a.stride + i] * c2,
                   syz = (double)a.sums[7 * a.stride + i] * c2, szz = (double)a.sums[8 * a.stride + i] * c2;
      const double mx = sx / K, my = sy / K, mz = sz / K;
      double a00 = sxx / K - mx * mx, a01 = sxy / K - mx * my, a02 = sxz / K - mx * mz;
      double a11 = syy / K - my * my, a12 = syz / K - my * mz, a22 = szz / K - mz * mz;
      for (int it = 0; it < lslam::JACOBI_SWEEPS; ++it) {  // (the eigenvalues alone: no vectors)
        lslam::sv_rotate(a00, a11, a01, a02, a12);
        lslam::sv_rotate(a00, a22, a02, a01, a12);
        lslam::sv_rotate(a11, a22, a12, a01, a02);
      }
      l0 = a00; l1 = a11; l2 = a22;
      if (l1 < l0) { const double t = l0; l0 = l1; l1 = t; }
      if (l2 < l1) { const double t = l1; l1 = l2; l2 = t; }
      if (l1 < l0) { const double t = l0; l0 = l1; l1 = t; }
      const double f = a.lambda_floor;
      const double v = l0 > 0.0 ? l0 : 0.0;
      h = 0.5 * ((log(l0 < f ? f : l0) + log(l1 < f ? f : l1)) + log(l2 < f ? f : l2)) + ENTROPY_CONST;
      agg[0] = 1;
      agg[2] = __double2ll_rn(h * 4294967296.0);
      agg[3] = __double2ll_rn(v * 1073741824.0);
      agg[4] = k;
      agg[5] = k;
    }
    if (a.out_l3) { a.out_l3[3 * (size_t)at] = l0; a.out_l3[3 * (size_t)at + 1] = l1; a.out_l3[3 * (size_t)at + 2] = l2; }
    if (a.out_h) a.out_h[at] = h;
    if (a.out_count) a.out_count[at] = k;
  }
#pragma unroll
  for (int j = 0; j < NAGG; ++j)
    for (int m = 32; m > 0; m >>= 1) {
      const long long o = shfl_xor_ll(agg[j], m);
      agg[j] = j == 5 ? (o > agg[j] ? o : agg[j]) : agg[j] + o;
    }
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int j = 0; j < NAGG; ++j) red[threadIdx.x >> 6][j] = agg[j];
  __syncthreads();
  if (threadIdx.x < NAGG) {
    const int j = (int)threadIdx.x;
    long long t = red[0][j];
    for (int w = 1; w < MQ_BLOCK / 64; ++w) t = j == 5 ? (red[w][j] > t ? red[w][j] : t) : t + red[w][j];
    a.partials[(size_t)blockIdx.x * NAGG + j] = t;
  }
}
// one workgroup: partials[blocks][NAGG] -> out[NAGG]
__global__ __launch_bounds__(MQ_BLOCK) void mq_final_kernel(const long long *partials, int blocks, long long *out) {
  __shared__ long long red[MQ_BLOCK / 64][NAGG];
  long long agg[NAGG] = {0, 0, 0, 0, 0, 0};
  for (int b = (int)threadIdx.x; b < blocks; b += MQ_BLOCK)
#pragma unroll
    for (int j = 0; j < NAGG; ++j) {
      const long long o = partials[(size_t)b * NAGG + j];
      agg[j] = j == 5 ? (o > agg[j] ? o : agg[j]) : agg[j] + o;
    }
#pragma unroll
  for (int j = 0; j < NAGG; ++j)
    for (int m = 32; m > 0; m >>= 1) {
      const long long o = shfl_xor_ll(agg[j], m);
      agg[j] = j == 5 ? (o > agg[j] ? o : agg[j]) : agg[j] + o;
    }
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int j = 0; j < NAGG; ++j) red[threadIdx.x >> 6][j] = agg[j];
  __syncthreads();
  if (threadIdx.x < NAGG) {
    const int j = (int)threadIdx.x;
    long long t = red[0][j];
    for (int w = 1; w < MQ_BLOCK / 64; ++w) t = j == 5 ? (red[w][j] > t ? red[w][j] : t) : t + red[w][j];
    out[j] = t;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// One cloud's sort: keys and positions in, the sorted keys and the gathered points out
struct SortBuf {
  DevBuf<uint64_t> k0, k1;
  DevBuf<uint32_t> i0, i1;
  DevBuf<float4> sorted;
};
// The evaluation's scratch, kept in the context (CTX_SLOT_MAPQ) and freed by lslam_ctx_destroy
struct Scratch {
  DevBuf<char> tmp;
  SortBuf s, q;
  DevBuf<uint32_t> box;
  DevBuf<int32_t> count;
  DevBuf<long long> sums, partials, agg;
  // the host form's staging and outputs, the keyframe form's gathered cloud
  DevBuf<float4> up_s, up_q, gathered;
  DevBuf<double> l3, h;
  DevBuf<int32_t> ocount;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  ~Scratch() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

int bad(const char *what) {
  lslam::set_error(what);
  return LSLAM_ERR_INVALID;
}

int check_params(const lslam_mapq_params *params, lslam_mapq_params *P) {
  lslam_mapq_default_params(P);
  if (params) *P = *params;
  if (!std::isfinite(P->radius) || !(P->radius > 0.0f) || !(P->radius <= 8.0f)) return bad("map quality: radius must be finite and in (0, 8] m");
  if (P->min_neighbors < 3) return bad("map quality: min_neighbors must be at least 3");
  if (!std::isfinite(P->lambda_floor) || !(P->lambda_floor > 0.0)) return bad("map quality: lambda_floor must be finite and > 0");
  return LSLAM_OK;
}

void empty_stats(lslam_mapq_stats *st) {
  std::memset(st, 0, sizeof(*st));
  st->mean_entropy = st->mean_plane_variance = st->mean_neighbors = std::numeric_limits<double>::quiet_NaN();
}

int sort_cloud(Scratch &w, SortBuf &b, hipStream_t s, const float4 *pts, size_t n, const SGrid &g, uint64_t behind, int end_bit) {
  LSLAM_TRY(b.k0.reserve(n)); LSLAM_TRY(b.k1.reserve(n)); LSLAM_TRY(b.i0.reserve(n)); LSLAM_TRY(b.i1.reserve(n)); LSLAM_TRY(b.sorted.reserve(n));
  hipLaunchKernelGGL(lslam::sg_key_kernel<true>, lslam::sg_blocks(n), dim3(lslam::SG_BLOCK), 0, s, pts, (int)n, g, behind, b.k0.p, b.i0.p);
  LSLAM_TRY(lslam::sort_pairs(w.tmp, b.k0.p, b.k1.p, b.i0.p, b.i1.p, n, end_bit, s));
  hipLaunchKernelGGL(lslam::sg_gather_kernel<>, lslam::sg_blocks(n), dim3(lslam::SG_BLOCK), 0, s, pts, b.i1.p, (int)n, b.sorted.p);
  LSLAM_TRY(hipGetLastError());
  return LSLAM_OK;
}

// The evaluation on device clouds (d_queries null: the surface queries itself).  Outputs: device pointers or null.  Waits.
int run(lslam_ctx *ctx, const float4 *d_surface, size_t ns_all, const float4 *d_queries, size_t nq_all, const lslam_mapq_params &P,
        lslam_mapq_stats *st, double *d_l3, double *d_h, int32_t *d_count) {
  empty_stats(st);
  const bool self = d_queries == nullptr;
  if (self) nq_all = ns_all;
  st->n_query = (int64_t)nq_all;
  if (ns_all >= MQ_MAX_POINTS || nq_all >= MQ_MAX_POINTS) return bad("map quality: 2^25 or more points in a cloud");
  LSLAM_TRY(hipSetDevice(lslam::ctx_device(ctx)));
  hipStream_t s = lslam::ctx_stream(ctx);
  Scratch &w = *lslam::ctx_slot<Scratch>(ctx, lslam::CTX_SLOT_MAPQ);
  for (hipEvent_t &e : w.ev)
    if (!e) LSLAM_TRY(hipEventCreate(&e));
  if (!nq_all) return LSLAM_OK;
  // the surface's bounding box and the finite counts of both clouds: one wait
  uint32_t box[14] = {};  // per cloud: the six words of a box, the count
  LSLAM_TRY(w.box.reserve(14));
  LSLAM_TRY(hipMemcpyAsync(w.box.p, box, sizeof(box), hipMemcpyHostToDevice, s));
  if (ns_all) hipLaunchKernelGGL(lslam::box_kernel<true>, lslam::box_blocks((int)ns_all), dim3(lslam::BOX_BLOCK), 0, s, d_surface, (int)ns_all, w.box.p);
  if (!self) hipLaunchKernelGGL(lslam::box_kernel<true>, lslam::box_blocks((int)nq_all), dim3(lslam::BOX_BLOCK), 0, s, d_queries, (int)nq_all, w.box.p + 7);
  LSLAM_TRY(hipMemcpyAsync(box, w.box.p, sizeof(box), hipMemcpyDeviceToHost, s));
  LSLAM_TRY(hipStreamSynchronize(s));
  const size_t ns = box[6], nq = self ? ns : box[13];
  st->n_surface = (int64_t)ns;
  st->n_nonfinite = (int64_t)(nq_all - nq);
  float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {0.0f, 0.0f, 0.0f};  // (no finite surface point: one cell)
  if (ns) lslam::box_back(box, lo, hi);
  SGrid g{};
  uint64_t cells = 1;  // itself the key of the non-finite points
  int end_bit = 1;
  lslam::sg_shape(lo, hi, (double)P.radius * lslam::GRID_CELL_PAD, &g, &cells, &end_bit);
  // both clouds sorted by cell
  LSLAM_TRY(hipEventRecord(w.ev[0], s));
  if (ns_all) LSLAM_RC(sort_cloud(w, w.s, s, d_surface, ns_all, g, cells, end_bit));
  if (!self) LSLAM_RC(sort_cloud(w, w.q, s, d_queries, nq_all, g, cells, end_bit));
  SortBuf &qs = self ? w.s : w.q;
  LSLAM_TRY(hipEventRecord(w.ev[1], s));
  // the sums
  const size_t stride = nq ? nq : 1;
  LSLAM_TRY(w.count.reserve(stride)); LSLAM_TRY(w.sums.reserve((size_t)NSUM * stride));
  if (nq) {
    ProbeArgs a{};
    a.g = g;
    a.g.keys = w.s.k1.p;
    a.g.pts = w.s.sorted.p;
    a.g.n = (int)ns;
    a.qpts = qs.sorted.p;
    a.nq = (int)nq;
    a.r2 = (float)((double)P.radius * (double)P.radius);
    a.count = w.count.p;
    a.sums = w.sums.p;
    a.stride = stride;
    hipLaunchKernelGGL(mq_probe_kernel, blocks_for(nq), dim3(MQ_BLOCK), 0, s, a);
    LSLAM_TRY(hipGetLastError());
  }
  LSLAM_TRY(hipEventRecord(w.ev[2], s));
  // the tail and the aggregates
  const int blocks = (int)((nq_all + MQ_BLOCK - 1) / MQ_BLOCK);
  LSLAM_TRY(w.partials.reserve((size_t)blocks * NAGG)); LSLAM_TRY(w.agg.reserve(NAGG));
  TailArgs t{};
  t.qpts = qs.sorted.p;
  t.nq = (int)nq;
  t.nq_all = (int)nq_all;
  t.count = w.count.p;
  t.sums = w.sums.p;
  t.stride = stride;
  t.min_neighbors = P.min_neighbors;
  t.lambda_floor = P.lambda_floor;
  t.out_l3 = d_l3;
  t.out_h = d_h;
  t.out_count = d_count;
  t.partials = w.partials.p;
  hipLaunchKernelGGL(mq_tail_kernel, dim3(blocks), dim3(MQ_BLOCK), 0, s, t);
  hipLaunchKernelGGL(mq_final_kernel, dim3(1), dim3(MQ_BLOCK), 0, s, w.partials.p, blocks, w.agg.p);
  LSLAM_TRY(hipGetLastError());
  LSLAM_TRY(hipEventRecord(w.ev[3], s));
  long long agg[NAGG];
  LSLAM_TRY(hipMemcpyAsync(agg, w.agg.p, sizeof(agg), hipMemcpyDeviceToHost, s));
  LSLAM_TRY(hipStreamSynchronize(s));
  st->n_defined = agg[0];
  st->n_sparse = agg[1];
  st->sum_entropy_q32 = agg[2];
  st->sum_plane_var_q30 = agg[3];
  st->sum_neighbors = agg[4];
  st->max_neighbors = agg[5];
  if (agg[0] > 0) {
    const double nd = (double)agg[0];
    st->mean_entropy = ((double)agg[2] / 4294967296.0) / nd;
    st->mean_plane_variance = ((double)agg[3] / 1073741824.0) / nd;
    st->mean_neighbors = (double)agg[4] / nd;
  }
  float *ms[3] = {&st->ms_sort, &st->ms_kernel, &st->ms_reduce};
  for (int k = 0; k < 3; ++k) LSLAM_TRY(hipEventElapsedTime(ms[k], w.ev[k], w.ev[k + 1]));
  return LSLAM_OK;
}

int need_ctx(lslam_ctx *ctx, const char *what) {
  if (!ctx || !lslam::ctx_alive(ctx)) {
    lslam::set_error((std::string(what) + ": no context").c_str());
    return LSLAM_ERR_INVALID;
  }
  return LSLAM_OK;
}

bool stride_ok(size_t stride) { return stride >= 12 && (stride & 3) == 0; }

// host records {x, y, z, ...} -> packed float4 on the device
int upload(hipStream_t s, DevBuf<float4> &d, std::vector<float4> &h, const void *cloud, size_t n, size_t stride) {
  h.resize(n);
  const char *b = (const char *)cloud;
  for (size_t i = 0; i < n; ++i) {
    float v[3];
    std::memcpy(v, b + i * stride, 12);
    h[i] = make_float4(v[0], v[1], v[2], 0.0f);
  }
  LSLAM_TRY(d.reserve(n ? n : 1));
  if (n) LSLAM_TRY(hipMemcpyAsync(d.p, h.data(), n * sizeof(float4), hipMemcpyHostToDevice, s));
  return LSLAM_OK;
}

}  // namespace

extern "C" {

void lslam_mapq_default_params(lslam_mapq_params *p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->radius = 0.3f;
  p->min_neighbors = 5;
  p->lambda_floor = 1e-8;
}
size_t lslam_sizeof_mapq_params(void) { return sizeof(lslam_mapq_params); }
size_t lslam_sizeof_mapq_stats(void) { return sizeof(lslam_mapq_stats); }

int lslam_mapq_eval_device(lslam_ctx *ctx, const float *d_surface, size_t n, const float *d_queries, size_t nq, const lslam_mapq_params *params,
                           lslam_mapq_stats *stats, double *d_lambda3, double *d_entropy, int32_t *d_count) {
  LSLAM_RC(need_ctx(ctx, "lslam_mapq_eval_device"));
  lslam_mapq_params P;
  LSLAM_RC(check_params(params, &P));
  if (!stats || (n && !d_surface)) return bad("lslam_mapq_eval_device: null stats, or a null surface with points");
  if (d_queries && !nq) {  // an empty query cloud of its own: nothing to evaluate
    empty_stats(stats);
    return LSLAM_OK;
  }
  return run(ctx, (const float4 *)d_surface, n, (const float4 *)d_queries, nq, P, stats, d_lambda3, d_entropy, d_count);
}

int lslam_mapq_eval(lslam_ctx *ctx, const void *surface, size_t n, size_t stride_bytes, const void *queries, size_t nq, size_t qstride_bytes,
                    const lslam_mapq_params *params, lslam_mapq_stats *stats, double *out_lambda3, double *out_entropy, int32_t *out_count) {
  LSLAM_RC(need_ctx(ctx, "lslam_mapq_eval"));
  lslam_mapq_params P;
  LSLAM_RC(check_params(params, &P));
  if (!stats || (n && !surface)) return bad("lslam_mapq_eval: null stats, or a null surface with points");
  if (!stride_ok(stride_bytes) || (queries && !stride_ok(qstride_bytes))) return bad("lslam_mapq_eval: a stride under 12 bytes or no multiple of 4");
  if (n >= MQ_MAX_POINTS || (queries && nq >= MQ_MAX_POINTS)) return bad("map quality: 2^25 or more points in a cloud");
  if (queries && !nq) {
    empty_stats(stats);
    return LSLAM_OK;
  }
  LSLAM_TRY(hipSetDevice(lslam::ctx_device(ctx)));
  hipStream_t s = lslam::ctx_stream(ctx);
  Scratch &w = *lslam::ctx_slot<Scratch>(ctx, lslam::CTX_SLOT_MAPQ);
  std::vector<float4> hs, hq;  // alive until run() has waited
  LSLAM_RC(upload(s, w.up_s, hs, surface, n, stride_bytes));
  if (queries) LSLAM_RC(upload(s, w.up_q, hq, queries, nq, qstride_bytes));
  const size_t m = queries ? nq : n;
  if (out_lambda3) LSLAM_TRY(w.l3.reserve(3 * m + 1));
  if (out_entropy) LSLAM_TRY(w.h.reserve(m + 1));
  if (out_count) LSLAM_TRY(w.ocount.reserve(m + 1));
  int rc = run(ctx, w.up_s.p, n, queries ? w.up_q.p : nullptr, nq, P, stats, out_lambda3 ? w.l3.p : nullptr, out_entropy ? w.h.p : nullptr,
               out_count ? w.ocount.p : nullptr);
  if (rc != LSLAM_OK) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  if (m && out_lambda3) LSLAM_TRY(hipMemcpyAsync(out_lambda3, w.l3.p, 3 * m * sizeof(double), hipMemcpyDeviceToHost, s));
  if (m && out_entropy) LSLAM_TRY(hipMemcpyAsync(out_entropy, w.h.p, m * sizeof(double), hipMemcpyDeviceToHost, s));
  if (m && out_count) LSLAM_TRY(hipMemcpyAsync(out_count, w.ocount.p, m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  LSLAM_TRY(hipStreamSynchronize(s));
  return LSLAM_OK;
}

int lslam_mapq_fmap(lslam_fmap *fm, int32_t which, const lslam_mapq_params *params, lslam_mapq_stats *stats) {
  lslam_mapq_params P;
  LSLAM_RC(check_params(params, &P));
  if (!stats || which < 0 || which > 1) return bad("lslam_mapq_fmap: null stats, or which outside {0, 1}");
  lslam::FmapView v{};
  LSLAM_RC(lslam::fmap_view(fm, &v));  // refuses a null map; commits a pending add
  return run(lslam::fmap_ctx(fm), v.pts[which], v.n[which], nullptr, 0, P, stats, nullptr, nullptr, nullptr);
}

int lslam_mapq_keyframes(lslam_kfs *kfs, int32_t n_ids, const int32_t *ids, const float *poses16, int32_t which, const lslam_mapq_params *params,
                         lslam_mapq_stats *stats) {
  LSLAM_RC(lslam::check_kfs(kfs, "lslam_mapq_keyframes"));
  lslam_mapq_params P;
  LSLAM_RC(check_params(params, &P));
  if (!stats || which < 0 || which > 1 || n_ids < 0 || (n_ids && (!ids || !poses16)))
    return bad("lslam_mapq_keyframes: null stats, which outside {0, 1}, or keyframes named without ids and poses");
  for (int32_t c = 0; c < n_ids; ++c) {
    LSLAM_RC(lslam::check_id(kfs, "lslam_mapq_keyframes", ids[c]));
    for (int e = 0; e < 16; ++e)
      if (!std::isfinite(poses16[16 * (size_t)c + e])) return bad("lslam_mapq_keyframes: a pose that is not finite");
  }
  Scratch &w = *lslam::ctx_slot<Scratch>(kfs->ctx, lslam::CTX_SLOT_MAPQ);
  size_t total = 0;
  LSLAM_RC(lslam::kfs_gather_posed(kfs, n_ids, ids, poses16, which, w.gathered, &total));
  return run(kfs->ctx, w.gathered.p, total, nullptr, 0, P, stats, nullptr, nullptr, nullptr);
}

}  // extern "C"
