// lslam_sc.hip -- loop candidates by appearance: a Scan Context descriptor (Kim & Kim, IROS 2018) per keyframe of the keyframe
// store and the exhaustive comparison of a query keyframe with all earlier ones (lslam_sc_* of include/lslam_c.h, whose
// comment is the specification).  Not in the reference: its LoopDetector searches around the drifted estimate only.
//
// Three kernels:
//   sc_describe_kernel  one workgroup per keyframe.  The cells live in LDS; a point's value goes in with an integer atomic max on
//                       its bit pattern (values are > 0, so the orderings agree, and a maximum does not depend on arrival order).
//                       Corner and surf points stream from the store's slabs where they lie, LSLAM_SC_POINT_CHUNK per pass.  The
//                       same pass writes the record's query form: the columns divided by their norms plus a row of 1.0 / 0.0
//                       flags, so the query kernel's cosine is a plain dot and its column count a dot of flags.
//   sc_query_kernel     grid (tiles of LSLAM_SC_CAND_TILE candidates, queries).  The query's form stays in LDS; the tile's
//                       candidates pass through LDS `cb` at a time; one lane evaluates one (candidate, shift) pair over all
//                       columns.  Layout [ring][sector]: lanes of consecutive shifts read consecutive LDS words of the candidate
//                       (conflict-free but for the one wrap) and one broadcast word of the query.  The minimum over shifts is a
//                       64-bit integer atomic min of {distance bits, shift} in LDS; the tile's top-k is a rank count over its 64
//                       keys {distance bits, id}.
//   sc_merge_kernel     one workgroup per query: top_k rounds of a workgroup-wide minimum over the tiles' lists.
// Keys are unique (the id is part of them) and only integer min / max combine values across lanes: nothing depends on arrival order.
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

using lslam::ScJob;
using lslam::ScState;
using lslam::check_id;
using lslam::check_kfs;

constexpr int SC_BLOCK = 256;
constexpr int SC_TILE = LSLAM_SC_CAND_TILE;
constexpr int SC_MAX_K = LSLAM_SC_MAX_TOP_K;
constexpr unsigned SC_SLAB_SHIFT = 10;
static_assert(((size_t)1 << SC_SLAB_SHIFT) == ScState::SC_SLAB_KEYFRAMES, "slab size and shift disagree");
static_assert(LSLAM_SC_POINT_CHUNK == SC_BLOCK, "one point per lane and pass");
static_assert(SC_TILE <= SC_BLOCK && SC_MAX_K <= SC_TILE, "the tile's selection takes one lane per candidate");
constexpr size_t SC_LDS_BUDGET = 60 * 1024;  // dynamic LDS of the query kernel (the static part is under 2 KiB)
constexpr uint64_t SC_NO_KEY = ~(uint64_t)0;
constexpr int32_t SC_MAX_QUERIES = 65535;  // grid.y

struct ScShape {
  int32_t n_ring, n_sector, up_axis;
  float max_range, height_offset, ring_scale;
  double sector_scale;
  uint32_t stride;  // floats per record
};

__device__ __forceinline__ float *sc_record(float *const *slabs, uint32_t stride, uint32_t id) {
  return slabs[id >> SC_SLAB_SHIFT] + (size_t)(id & ((1u << SC_SLAB_SHIFT) - 1)) * stride;
}

// dynamic LDS: cells[n_ring * n_sector] (uint32: the bit patterns), norm[n_sector]
__global__ __launch_bounds__(SC_BLOCK) void sc_describe_kernel(const ScJob *jobs, uint32_t first_id, float *const *slabs,
                                                                const ScShape sh) {
  extern __shared__ uint32_t sc_lds[];
  const int R = sh.n_ring, S = sh.n_sector, cells = R * S;
  uint32_t *cell = sc_lds;
  float *norm = reinterpret_cast<float *>(sc_lds + cells);
  const int tid = (int)threadIdx.x;
  const ScJob job = jobs[blockIdx.x];
  for (int i = tid; i < cells; i += SC_BLOCK) cell[i] = 0u;
  __syncthreads();
  for (int t = 0; t < 2; ++t) {
    const float4 *pts = job.p[t];
    const uint32_t n = job.n[t];
    for (uint32_t base = 0; base < n; base += LSLAM_SC_POINT_CHUNK) {
      const uint32_t i = base + (uint32_t)tid;
      if (i >= n) continue;
      const float4 p = pts[i];
      if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) continue;
      const float a = sh.up_axis == 1 ? p.z : p.x, b = sh.up_axis == 1 ? p.x : p.y, h = sh.up_axis == 1 ? p.y : p.z;
      const float d2 = a * a + b * b;
      const float rho = sqrtf(d2);
      if (rho == 0.0f || !(rho < sh.max_range)) continue;
      const int ring = (int)(rho * sh.ring_scale);
      if (ring >= R) continue;
      double ang = atan2((double)b, (double)a);
      if (ang < 0.0) ang += 6.283185307179586;
      int sector = (int)(ang * sh.sector_scale);
      if (sector > S - 1) sector = S - 1;
      const float v = h + sh.height_offset;
      if (!(v > 0.0f)) continue;
      atomicMax(&cell[ring * S + sector], __builtin_bit_cast(uint32_t, v));  // (0 <= ring < R, 0 <= sector < S: in bounds)
    }
  }
  __syncthreads();
  for (int j = tid; j < S; j += SC_BLOCK) {
    float s2 = 0.0f;
    for (int r = 0; r < R; ++r) {
      const float v = __builtin_bit_cast(float, cell[r * S + j]);
      s2 = s2 + v * v;
    }
    norm[j] = sqrtf(s2);
  }
  __syncthreads();
  float *rec = sc_record(slabs, sh.stride, first_id + blockIdx.x);
  for (int i = tid; i < cells; i += SC_BLOCK) {  // consecutive lanes, consecutive words
    const float v = __builtin_bit_cast(float, cell[i]);
    const float nj = norm[i % S];
    rec[i] = v;
    rec[cells + i] = nj > 0.0f ? v / nj : 0.0f;
  }
  for (int j = tid; j < S; j += SC_BLOCK) rec[2 * cells + j] = norm[j] > 0.0f ? 1.0f : 0.0f;
}

// dynamic LDS: the query's form [(n_ring + 1) * n_sector], then cb candidates' forms
__global__ __launch_bounds__(SC_BLOCK) void sc_query_kernel(float *const *slabs, uint32_t stride, int R, int S, int cb,
                                                             const int32_t *query_ids, const int32_t *max_cand, int top_k,
                                                             uint32_t n_tiles, uint64_t *tile_key, int32_t *tile_shift,
                                                             float *tap_dist, int32_t *tap_shift, uint32_t n_tap) {
  extern __shared__ float sc_form[];
  __shared__ unsigned long long best[4];
  __shared__ uint64_t tkey[SC_TILE];
  __shared__ int32_t tshift[SC_TILE];
  __shared__ uint64_t okey[SC_MAX_K];
  __shared__ int32_t oshift[SC_MAX_K];
  const int tid = (int)threadIdx.x;
  const uint32_t q = blockIdx.y, tile = blockIdx.x;
  const int32_t maxc = max_cand[q];
  const int64_t tile0 = (int64_t)tile * SC_TILE;
  if (tile0 > (int64_t)maxc) return;  // (uniform) nothing eligible here: the merge does not read this tile either
  const int F = (R + 1) * S, RS = R * S;
  float *Q = sc_form, *Cs = sc_form + F;
  {
    const float *qrec = sc_record(slabs, stride, (uint32_t)query_ids[q]) + RS;
    for (int i = tid; i < F; i += SC_BLOCK) Q[i] = qrec[i];
  }
  for (int c0 = 0; c0 < SC_TILE; c0 += cb) {
    for (int c = 0; c < cb; ++c) {
      const int64_t id = tile0 + c0 + c;
      if (id > (int64_t)maxc) break;  // (uniform)
      const float *crec = sc_record(slabs, stride, (uint32_t)id) + RS;
      for (int i = tid; i < F; i += SC_BLOCK) Cs[c * F + i] = crec[i];
    }
    if (tid < cb) best[tid] = SC_NO_KEY;
    __syncthreads();
    for (int w = tid; w < cb * S; w += SC_BLOCK) {
      const int c = w / S, s = w - c * S;
      if (tile0 + c0 + c > (int64_t)maxc) continue;
      const float *C = Cs + c * F;
      float sum = 0.0f, cnt = 0.0f;
      int col = s;
      for (int j = 0; j < S; ++j) {
        float dot = 0.0f;
        // unrolled so that the LDS reads of several rings are in flight together; the order of the multiply-adds is unchanged
#pragma unroll 8
        for (int r = 0; r < R; ++r) dot = __builtin_fmaf(Q[r * S + j], C[r * S + col], dot);
        sum += dot;
        cnt += Q[RS + j] * C[RS + col];  // flags: exact
        col = col + 1 == S ? 0 : col + 1;
      }
      const float d = cnt > 0.0f ? fmaxf(1.0f - sum / cnt, 0.0f) : 1.0f;
      atomicMin(&best[c], ((unsigned long long)__builtin_bit_cast(uint32_t, d) << 32) | (unsigned)s);
    }
    __syncthreads();
    if (tid < cb) {
      const int64_t id = tile0 + c0 + tid;
      if (id <= (int64_t)maxc) {
        const uint64_t b = best[tid];
        tkey[c0 + tid] = (b & 0xffffffff00000000ull) | (uint64_t)id;
        tshift[c0 + tid] = (int32_t)(b & 0xffffffffu);
        if (tap_dist && (uint64_t)id < n_tap) {
          tap_dist[(size_t)q * n_tap + id] = __builtin_bit_cast(float, (uint32_t)(b >> 32));
          tap_shift[(size_t)q * n_tap + id] = (int32_t)(b & 0xffffffffu);
        }
      } else {
        tkey[c0 + tid] = SC_NO_KEY;
        tshift[c0 + tid] = 0;
      }
    }
    __syncthreads();
  }
  // the tile's top_k: an entry's rank is the number of smaller keys (keys are unique: the id is in them)
  if (tid < SC_MAX_K) {
    okey[tid] = SC_NO_KEY;
    oshift[tid] = 0;
  }
  __syncthreads();
  if (tid < SC_TILE) {
    const uint64_t k = tkey[tid];
    if (k != SC_NO_KEY) {
      int rank = 0;
      for (int j = 0; j < SC_TILE; ++j) rank += tkey[j] < k ? 1 : 0;
      if (rank < top_k) {
        okey[rank] = k;
        oshift[rank] = tshift[tid];
      }
    }
  }
  __syncthreads();
  if (tid < top_k) {
    const size_t at = ((size_t)q * n_tiles + tile) * (size_t)top_k + (size_t)tid;
    tile_key[at] = okey[tid];
    tile_shift[at] = oshift[tid];
  }
}

// out: ids [nq * top_k], shifts [nq * top_k], distance bits [nq * top_k]
__global__ __launch_bounds__(SC_BLOCK) void sc_merge_kernel(const int32_t *max_cand, int top_k, uint32_t n_tiles, uint32_t nq,
                                                             const uint64_t *tile_key, const int32_t *tile_shift, int32_t *out) {
  __shared__ unsigned long long sbest;
  const int tid = (int)threadIdx.x;
  const uint32_t q = blockIdx.x;
  const int32_t maxc = max_cand[q];
  const size_t n = maxc < 0 ? 0 : ((size_t)maxc / SC_TILE + 1) * (size_t)top_k;  // the lists of the tiles that ran
  const size_t base = (size_t)q * n_tiles * (size_t)top_k;
  const size_t total = (size_t)nq * (size_t)top_k;
  int32_t *ids = out + (size_t)q * top_k, *shifts = ids + total, *dist = shifts + total;
  if (tid < top_k) {
    ids[tid] = -1;
    shifts[tid] = 0;
    dist[tid] = 0x3f800000;  // 1.0f
  }
  uint64_t lower = 0;
  for (int round = 0; round < top_k; ++round) {
    uint64_t mine = SC_NO_KEY;
    size_t mine_at = 0;
    for (size_t i = (size_t)tid; i < n; i += SC_BLOCK) {
      const uint64_t k = tile_key[base + i];
      if (k >= lower && k < mine) {
        mine = k;
        mine_at = i;
      }
    }
    if (tid == 0) sbest = SC_NO_KEY;
    __syncthreads();
    if (mine != SC_NO_KEY) atomicMin(&sbest, (unsigned long long)mine);
    __syncthreads();
    const uint64_t b = sbest;
    if (b == SC_NO_KEY) break;  // (uniform) fewer than top_k eligible
    if (mine == b) {
      ids[round] = (int32_t)(b & 0xffffffffu);
      shifts[round] = tile_shift[base + mine_at];
      dist[round] = (int32_t)(uint32_t)(b >> 32);
    }
    lower = b + 1;
    __syncthreads();
  }
}

int sc_ready(lslam_kfs *k, const char *what) {
  if (!k->sc.set) {
    char b[200];
    snprintf(b, sizeof(b), "%s: lslam_sc_setup was not called on this store", what);
    lslam::set_error(b);
    return LSLAM_ERR_INVALID;
  }
  return LSLAM_OK;
}

ScShape sc_shape(const ScState &sc) {
  ScShape sh{};
  sh.n_ring = sc.params.n_ring;
  sh.n_sector = sc.params.n_sector;
  sh.up_axis = sc.params.up_axis;
  sh.max_range = sc.params.max_range;
  sh.height_offset = sc.params.height_offset;
  sh.ring_scale = sc.ring_scale;
  sh.sector_scale = sc.sector_scale;
  sh.stride = (uint32_t)sc.stride;
  return sh;
}

// Every keyframe without a record gets one, in one launch (enqueued, not waited for).
int sc_describe_pending(lslam_kfs *k) {
  ScState &sc = k->sc;
  const size_t n = k->kfs.size();
  if (sc.described >= n) return LSLAM_OK;
  const size_t want_slabs = (n + ScState::SC_SLAB_KEYFRAMES - 1) / ScState::SC_SLAB_KEYFRAMES;
  while (sc.slabs.size() < want_slabs) {
    std::unique_ptr<lslam::DevBuf<float>> s(new lslam::DevBuf<float>());
    const hipError_t e = s->alloc(ScState::SC_SLAB_KEYFRAMES * sc.stride);
    if (e != hipSuccess) {
      char b[200];
      snprintf(b, sizeof(b), "scan context: a descriptor slab could not be allocated: %s", hipGetErrorString(e));
      lslam::set_error(b);
      return LSLAM_ERR_HIP;
    }
    sc.slabs.push_back(std::move(s));
  }
  if (sc.slabs_uploaded != sc.slabs.size()) {  // the table of base pointers (the table may move; the slabs do not)
    std::vector<float *> tab(sc.slabs.size());
    for (size_t i = 0; i < tab.size(); ++i) tab[i] = sc.slabs[i]->p;
    LSLAM_TRY(hipStreamSynchronize(k->stream));
    LSLAM_TRY(sc.d_slabs.reserve(tab.size()));
    LSLAM_TRY(hipMemcpy(sc.d_slabs.p, tab.data(), tab.size() * sizeof(float *), hipMemcpyHostToDevice));
    sc.slabs_uploaded = sc.slabs.size();
  }
  const size_t m = n - sc.described;
  LSLAM_TRY(sc.h_jobs.reserve(m));
  LSLAM_TRY(sc.d_jobs.reserve(m));
  for (size_t i = 0; i < m; ++i) {
    const lslam::KeyframeClouds &kc = k->kfs[sc.described + i];
    ScJob j{};
    for (int t = 0; t < 2; ++t) {
      j.p[t] = kc.p[t];
      j.n[t] = (uint32_t)kc.n[t];
    }
    sc.h_jobs.p[i] = j;
  }
  LSLAM_TRY(hipMemcpyAsync(sc.d_jobs.p, sc.h_jobs.p, m * sizeof(ScJob), hipMemcpyHostToDevice, k->stream));
  const size_t lds = ((size_t)sc.params.n_ring * sc.params.n_sector + sc.params.n_sector) * sizeof(float);
  hipLaunchKernelGGL(sc_describe_kernel, dim3((unsigned)m), dim3(SC_BLOCK), lds, k->stream, sc.d_jobs.p, (uint32_t)sc.described,
                     sc.d_slabs.p, sc_shape(sc));
  LSLAM_TRY(hipGetLastError());
  // (h_jobs is rewritten by the next describe only: every caller waits for the stream before it returns)
  sc.described = n;
  ++sc.describe_launches;
  return LSLAM_OK;
}

// The query kernel for nq queries whose ids and limits are in d_in [0, nq) and [nq, 2 nq); max_limit: the largest limit (>= 0).
int sc_launch_query(lslam_kfs *k, int32_t nq, int32_t max_limit, int32_t top_k, float *tap_dist, int32_t *tap_shift, uint32_t n_tap,
                    uint32_t *n_tiles_out) {
  ScState &sc = k->sc;
  const uint32_t n_tiles = (uint32_t)max_limit / SC_TILE + 1;
  const size_t lists = (size_t)nq * n_tiles * (size_t)top_k;
  LSLAM_TRY(sc.d_tile_key.reserve(lists));
  LSLAM_TRY(sc.d_tile_shift.reserve(lists));
  const size_t form = ((size_t)sc.params.n_ring + 1) * sc.params.n_sector * sizeof(float);
  int cb = 4;
  while (cb > 1 && (size_t)(cb + 1) * form > SC_LDS_BUDGET) cb >>= 1;
  hipLaunchKernelGGL(sc_query_kernel, dim3(n_tiles, (unsigned)nq), dim3(SC_BLOCK), (size_t)(cb + 1) * form, k->stream, sc.d_slabs.p,
                     (uint32_t)sc.stride, (int)sc.params.n_ring, (int)sc.params.n_sector, cb, sc.d_in.p, sc.d_in.p + nq, (int)top_k,
                     n_tiles, sc.d_tile_key.p, sc.d_tile_shift.p, tap_dist, tap_shift, n_tap);
  LSLAM_TRY(hipGetLastError());
  ++sc.query_launches;
  *n_tiles_out = n_tiles;
  return LSLAM_OK;
}

// an error after work was enqueued: the stream is drained before the caller gets its buffers back
int sc_fail(lslam_kfs *k, int rc) {
  (void)hipStreamSynchronize(k->stream);
  return rc;
}

}  // namespace

extern "C" {

void lslam_sc_default_params(lslam_sc_params *p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->n_ring = 20;
  p->n_sector = 60;
  p->max_range = 80.0f;
  p->height_offset = 2.0f;
  p->up_axis = 1;
}

int lslam_sc_setup(lslam_kfs *k, const lslam_sc_params *params) {
  const int rc = check_kfs(k, "lslam_sc_setup");
  if (rc) return rc;
  lslam_sc_params p;
  lslam_sc_default_params(&p);
  if (params) p = *params;
  char b[240];
  b[0] = 0;
  if (p.n_ring < 2 || p.n_ring > 32) snprintf(b, sizeof(b), "lslam_sc_setup: n_ring %d outside 2 .. 32", p.n_ring);
  else if (p.n_sector < 4 || p.n_sector > 128) snprintf(b, sizeof(b), "lslam_sc_setup: n_sector %d outside 4 .. 128", p.n_sector);
  else if (!(p.max_range > 0.0f) || !std::isfinite(p.max_range))
    snprintf(b, sizeof(b), "lslam_sc_setup: max_range %g is not a positive finite length", (double)p.max_range);
  else if (!std::isfinite(p.height_offset)) snprintf(b, sizeof(b), "lslam_sc_setup: height_offset is not finite");
  else if (p.up_axis != 1 && p.up_axis != 2) snprintf(b, sizeof(b), "lslam_sc_setup: up_axis %d is neither 1 (y up) nor 2 (z up)", p.up_axis);
  if (b[0]) {
    lslam::set_error(b);
    return LSLAM_ERR_INVALID;
  }
  ScState &sc = k->sc;
  if (sc.set && std::memcmp(&sc.params, &p, sizeof(p)) == 0) return LSLAM_OK;
  LSLAM_TRY(hipStreamSynchronize(k->stream));
  sc.drop();
  sc.params = p;
  sc.ring_scale = (float)p.n_ring / p.max_range;
  sc.sector_scale = (double)p.n_sector / 6.283185307179586;
  sc.stride = (size_t)(2 * p.n_ring + 1) * (size_t)p.n_sector;
  sc.set = true;
  return LSLAM_OK;
}

int lslam_sc_descriptor(lslam_kfs *k, int32_t id, float *out) {
  int rc = check_kfs(k, "lslam_sc_descriptor");
  if (rc) return rc;
  rc = sc_ready(k, "lslam_sc_descriptor");
  if (rc) return rc;
  rc = check_id(k, "lslam_sc_descriptor", id);
  if (rc) return rc;
  if (!out) {
    lslam::set_error("lslam_sc_descriptor: null out");
    return LSLAM_ERR_INVALID;
  }
  rc = sc_describe_pending(k);
  if (rc) return sc_fail(k, rc);
  ScState &sc = k->sc;
  const float *rec = sc.slabs[(size_t)id / ScState::SC_SLAB_KEYFRAMES]->p + ((size_t)id % ScState::SC_SLAB_KEYFRAMES) * sc.stride;
  const size_t cells = (size_t)sc.params.n_ring * sc.params.n_sector;
  LSLAM_TRY(hipMemcpyAsync(out, rec, cells * sizeof(float), hipMemcpyDeviceToHost, k->stream));
  LSLAM_TRY(hipStreamSynchronize(k->stream));
  return LSLAM_OK;
}

int lslam_sc_query(lslam_kfs *k, int32_t n_query, const int32_t *query_ids, const int32_t *max_cand_id, int32_t top_k,
                       int32_t *ids_out, int32_t *shift_out, float *dist_out, int32_t *n_out) {
  int rc = check_kfs(k, "lslam_sc_query");
  if (rc) return rc;
  rc = sc_ready(k, "lslam_sc_query");
  if (rc) return rc;
  if (top_k < 1 || top_k > SC_MAX_K) {
    char b[160];
    snprintf(b, sizeof(b), "lslam_sc_query: top_k %d outside 1 .. %d", top_k, SC_MAX_K);
    lslam::set_error(b);
    return LSLAM_ERR_INVALID;
  }
  if (n_query < 0 || n_query > SC_MAX_QUERIES || (n_query && (!query_ids || !ids_out || !shift_out || !dist_out || !n_out))) {
    char b[160];
    snprintf(b, sizeof(b), "lslam_sc_query: n_query outside 0 .. %d, or a null array", SC_MAX_QUERIES);
    lslam::set_error(b);
    return LSLAM_ERR_INVALID;
  }
  if (!n_query) return LSLAM_OK;
  ScState &sc = k->sc;
  const size_t nq = (size_t)n_query, total = nq * (size_t)top_k;
  int32_t max_limit = -1;
  for (size_t q = 0; q < nq; ++q) {
    rc = check_id(k, "lslam_sc_query", query_ids[q]);
    if (rc) return rc;
    const int32_t lim = max_cand_id ? max_cand_id[q] : query_ids[q] - 1;
    if (lim >= 0 && (size_t)lim >= k->kfs.size()) {
      char b[200];
      snprintf(b, sizeof(b), "lslam_sc_query: max_cand_id %d out of range (the store holds %zu)", lim, k->kfs.size());
      lslam::set_error(b);
      return LSLAM_ERR_INVALID;
    }
    if (lim > max_limit) max_limit = lim;
  }
  LSLAM_TRY(sc.h_io.reserve(2 * nq + 3 * total));
  LSLAM_TRY(sc.d_in.reserve(2 * nq));
  LSLAM_TRY(sc.d_out.reserve(3 * total));
  int32_t *h_in = sc.h_io.p, *h_out = sc.h_io.p + 2 * nq;
  for (size_t q = 0; q < nq; ++q) {
    const int32_t lim = max_cand_id ? max_cand_id[q] : query_ids[q] - 1;
    h_in[q] = query_ids[q];
    h_in[nq + q] = lim < 0 ? -1 : lim;
    n_out[q] = lim < 0 ? 0 : (lim + 1 < top_k ? lim + 1 : top_k);
  }
  rc = sc_describe_pending(k);
  if (rc) return sc_fail(k, rc);
  LSLAM_TRY(hipMemcpyAsync(sc.d_in.p, h_in, 2 * nq * sizeof(int32_t), hipMemcpyHostToDevice, k->stream));
  uint32_t n_tiles = 1;
  if (max_limit >= 0) {
    rc = sc_launch_query(k, n_query, max_limit, top_k, nullptr, nullptr, 0, &n_tiles);
    if (rc) return sc_fail(k, rc);
  }
  hipLaunchKernelGGL(sc_merge_kernel, dim3((unsigned)nq), dim3(SC_BLOCK), 0, k->stream, sc.d_in.p + nq, (int)top_k, n_tiles, (uint32_t)nq,
                     sc.d_tile_key.p, sc.d_tile_shift.p, sc.d_out.p);
  LSLAM_TRY(hipGetLastError());
  LSLAM_TRY(hipMemcpyAsync(h_out, sc.d_out.p, 3 * total * sizeof(int32_t), hipMemcpyDeviceToHost, k->stream));
  LSLAM_TRY(hipStreamSynchronize(k->stream));  // the call's one wait
  std::memcpy(ids_out, h_out, total * sizeof(int32_t));
  std::memcpy(shift_out, h_out + total, total * sizeof(int32_t));
  std::memcpy(dist_out, h_out + 2 * total, total * sizeof(float));
  return LSLAM_OK;
}

int lslam_sc_distances(lslam_kfs *k, int32_t query_id, float *dist_out, int32_t *shift_out) {
  int rc = check_kfs(k, "lslam_sc_distances");
  if (rc) return rc;
  rc = sc_ready(k, "lslam_sc_distances");
  if (rc) return rc;
  rc = check_id(k, "lslam_sc_distances", query_id);
  if (rc) return rc;
  if (!dist_out || !shift_out) {
    lslam::set_error("lslam_sc_distances: null output");
    return LSLAM_ERR_INVALID;
  }
  ScState &sc = k->sc;
  const size_t n = k->kfs.size();
  LSLAM_TRY(sc.h_io.reserve(2));
  LSLAM_TRY(sc.d_in.reserve(2));
  LSLAM_TRY(sc.d_tap.reserve(2 * n));
  rc = sc_describe_pending(k);
  if (rc) return sc_fail(k, rc);
  sc.h_io.p[0] = query_id;
  sc.h_io.p[1] = (int32_t)n - 1;
  LSLAM_TRY(hipMemcpyAsync(sc.d_in.p, sc.h_io.p, 2 * sizeof(int32_t), hipMemcpyHostToDevice, k->stream));
  uint32_t n_tiles = 0;
  rc = sc_launch_query(k, 1, (int32_t)n - 1, 1, sc.d_tap.p, reinterpret_cast<int32_t *>(sc.d_tap.p + n), (uint32_t)n, &n_tiles);
  if (rc) return sc_fail(k, rc);
  LSLAM_TRY(hipMemcpyAsync(dist_out, sc.d_tap.p, n * sizeof(float), hipMemcpyDeviceToHost, k->stream));
  LSLAM_TRY(hipMemcpyAsync(shift_out, sc.d_tap.p + n, n * sizeof(int32_t), hipMemcpyDeviceToHost, k->stream));
  LSLAM_TRY(hipStreamSynchronize(k->stream));
  return LSLAM_OK;
}

int lslam_sc_info(lslam_kfs *k, lslam_sc_stats *out) {
  if (out) std::memset(out, 0, sizeof(*out));
  const int rc = check_kfs(k, "lslam_sc_info");
  if (rc) return rc;
  if (!out) {
    lslam::set_error("lslam_sc_info: null out");
    return LSLAM_ERR_INVALID;
  }
  const ScState &sc = k->sc;
  if (sc.set) out->params = sc.params;
  out->is_set = sc.set ? 1 : 0;
  out->n_described = (int64_t)sc.described;
  out->descriptor_bytes = (uint64_t)sc.bytes_held();
  out->describe_launches = sc.describe_launches;
  out->query_launches = sc.query_launches;
  return LSLAM_OK;
}

}  // extern "C"
