// lslam_floor.hip -- floor (ground plane) detection on the device: lslam_floor_detect, lslam_floor_detect_device,
// lslam_floor_detect_keyframes and the taps lslam_debug_floor_hypotheses, lslam_debug_floor_score (include/lslam_c.h, "floor detection").
//
// The reference only shows the intent (pose_graph/solver_g2o.h:61-65, :92, graph.cpp:321: floor coefficients that nothing
// produces); the design is hdl_graph_slam's floor detector restated as a deterministic RANSAC.  PARITY IS UNPINNED: the
// semantics are this project's own and the header states them completely.
//
// A call works on a batch of clouds (one for the single-cloud entry points, the named keyframes' surface clouds for the store's);
// every stage is ONE launch over the whole batch, workgroups indexed by (tile, cloud), and per-cloud arithmetic does not depend
// on the batch -- a batched detection returns the bits of the single ones.
//   floor_mark_kernel     candidates per tile of 1024 input points (the height band, the range gate, finite coordinates)
//   floor_scan_kernel     per cloud: exclusive prefix of its tiles' counts, K
//   floor_compact_kernel  stable compaction: the candidates' input indices and their points, in input order
//   floor_hypo_kernel     one lane per hypothesis: three hashed slots, the plane in fp64, rounded to fp32; degenerate / steep marks
//   floor_score_kernel    THE HOT LOOP: H x K point-plane tests (below)
//   floor_best_kernel     per cloud: largest count, lowest index on ties
//   floor_sums_kernel     inliers of the current plane: sum p, sum p p^T, sum dist^2, count in fp64 per tile, one fixed order
//   floor_reduce_kernel   per cloud: the tiles' records in one fixed order
// The host then reads one small record per cloud, fits (3x3 Jacobi) and, per refit iteration and for the final statistics,
// runs the last two kernels again under the new plane.  No point moves between host and device.
//
// floor_score_kernel: a workgroup of 256 lanes holds a tile of 1024 candidates in registers (four per lane, one float4 load
// each: every candidate is read from HBM once per workgroup) and tests them against a chunk of hypotheses.  The planes of 64
// hypotheses at a time sit in LDS and are read by broadcast (one ds_read_b128 per hypothesis and wavefront: wave-uniform data,
// no per-lane global loads); an excluded hypothesis is staged as NaN and counts nothing.  A test is the header's fp32
// expression, no FMA: 6 VALU operations and a compare.  Counting is ballot + population count on the scalar unit; lane j of a
// wavefront keeps the count of hypothesis j, the four wavefronts add theirs in LDS (integer adds) and the workgroup's 64 sums
// leave by integer atomic adds: integer arithmetic throughout, so the counts are exact and the order of workgroups is immaterial.
#include "../../include/lslam_c.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lslam_internal.hpp"
#include "lslam_kfs_impl.hpp"

namespace {

using lslam::FloorJob;
using lslam::FloorOut;
using lslam::FloorPlane;
using lslam::FloorScratch;

constexpr int FLOOR_BLOCK = 256;
constexpr int FLOOR_PPL = 4;                          // points per lane
constexpr int FLOOR_TILE = FLOOR_BLOCK * FLOOR_PPL;   // points per workgroup
constexpr int FLOOR_WAVES = FLOOR_BLOCK / 64;
constexpr int FLOOR_HCHUNK = 128;                     // hypotheses per scoring workgroup (a multiple of 64)
constexpr int FLOOR_NSUM = lslam::FLOOR_NSUM;         // sum x y z | xx xy xz yy yz zz | dist^2 | count
constexpr int FLOOR_MAX_CLOUDS = 65535;               // blockIdx.y

struct FloorDev {
  float up[3];        // the unit up direction rounded to fp32: the candidate rule
  float h_lo, h_hi;   // -(sensor_height + clip), -(sensor_height - clip), fp32
  float range2;       // max_range^2 in fp32 (use_range)
  int32_t use_range;
  float thr;
  int32_t H;
  uint32_t seed;
  double up64[3];
  double cos_max;
};

__device__ __forceinline__ bool floor_candidate(const FloorDev &P, const float4 p) {
  const float h = ((P.up[0] * p.x + P.up[1] * p.y) + P.up[2] * p.z);
  // (a non-finite coordinate makes h NaN or infinite, or -- inf * 0 -- NaN: the finiteness test is explicit all the same)
  bool ok = isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && h >= P.h_lo && h <= P.h_hi;
  if (P.use_range) ok = ok && ((p.x * p.x + p.y * p.y) + p.z * p.z) <= P.range2;
  return ok;
}

// point r of lane t of the tile that starts at `first`: first + r * 256 + t (consecutive lanes, consecutive points)
__global__ __launch_bounds__(FLOOR_BLOCK) void floor_mark_kernel(const FloorJob *jobs, const FloorDev P, int32_t *tile_cnt) {
  const FloorJob J = jobs[blockIdx.y];
  const uint32_t first = blockIdx.x * (uint32_t)FLOOR_TILE;
  if (first >= J.n) return;
  __shared__ int s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  int c = 0;
  for (int r = 0; r < FLOOR_PPL; ++r) {
    const uint32_t i = first + r * FLOOR_BLOCK + threadIdx.x;
    const bool ok = i < J.n && floor_candidate(P, J.pts[i]);
    c += __popcll(__ballot(ok));
  }
  if ((threadIdx.x & 63) == 0) atomicAdd(&s_cnt, c);
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[J.tile_base + blockIdx.x] = s_cnt;
}

// one workgroup per cloud: tile_off = exclusive prefix of tile_cnt over the cloud's tiles, K = their sum
__global__ __launch_bounds__(FLOOR_BLOCK) void floor_scan_kernel(const FloorJob *jobs, const int32_t *tile_cnt, int32_t *tile_off,
                                                                 FloorOut *out) {
  const FloorJob J = jobs[blockIdx.x];
  const uint32_t tiles = (J.n + FLOOR_TILE - 1) / FLOOR_TILE;
  const uint32_t per = (tiles + FLOOR_BLOCK - 1) / FLOOR_BLOCK;
  const uint32_t lo = threadIdx.x * per, hi = lo + per < tiles ? lo + per : tiles;
  __shared__ int s_sum[FLOOR_BLOCK];
  int sum = 0;
  for (uint32_t t = lo; t < hi; ++t) sum += tile_cnt[J.tile_base + t];
  s_sum[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int t = 0; t < FLOOR_BLOCK; ++t) {
      const int v = s_sum[t];
      s_sum[t] = run;
      run += v;
    }
    out[blockIdx.x].K = run;
  }
  __syncthreads();
  int run = s_sum[threadIdx.x];
  for (uint32_t t = lo; t < hi; ++t) {
    tile_off[J.tile_base + t] = run;
    run += tile_cnt[J.tile_base + t];
  }
}

__global__ __launch_bounds__(FLOOR_BLOCK) void floor_compact_kernel(const FloorJob *jobs, const FloorDev P, const int32_t *tile_off,
                                                                    int32_t *cand_idx, float4 *cand_pts) {
  const FloorJob J = jobs[blockIdx.y];
  const uint32_t first = blockIdx.x * (uint32_t)FLOOR_TILE;
  if (first >= J.n) return;
  __shared__ int s_wave[FLOOR_PPL * FLOOR_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4 p[FLOOR_PPL];
  bool ok[FLOOR_PPL];
  int before[FLOOR_PPL];
  for (int r = 0; r < FLOOR_PPL; ++r) {
    const uint32_t i = first + r * FLOOR_BLOCK + threadIdx.x;
    p[r] = i < J.n ? J.pts[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    ok[r] = i < J.n && floor_candidate(P, p[r]);
    const unsigned long long m = __ballot(ok[r]);
    before[r] = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[r * FLOOR_WAVES + wave] = __popcll(m);
  }
  __syncthreads();
  const int base = tile_off[J.tile_base + blockIdx.x];
  for (int r = 0; r < FLOOR_PPL; ++r) {
    if (!ok[r]) continue;
    int off = base + before[r];
    for (int q = 0; q < r * FLOOR_WAVES + wave; ++q) off += s_wave[q];  // input order: row r, then wavefront, then lane
    // off < K <= J.n: inside the cloud's slice [cand_base, cand_base + n)
    cand_idx[J.cand_base + off] = (int32_t)(first + r * FLOOR_BLOCK + threadIdx.x);
    cand_pts[J.cand_base + off] = p[r];
  }
}

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

// hstat: 0 takes part in the vote, -1 degenerate, -2 steep
__global__ __launch_bounds__(64) void floor_hypo_kernel(const FloorJob *jobs, const FloorDev P, const FloorOut *out, const float4 *cand_pts,
                                                        int32_t *triples, float4 *planes, int32_t *hstat) {
  const int job = blockIdx.y;
  const int h = blockIdx.x * 64 + threadIdx.x;  // < H: H is a multiple of 64
  const uint32_t K = (uint32_t)out[job].K;
  const size_t at = (size_t)job * P.H + h;
  uint32_t s[3];
  for (int j = 0; j < 3; ++j) s[j] = (uint32_t)(((uint64_t)fmix32(P.seed + 0x9E3779B9u * (uint32_t)(3 * h + j + 1)) * K) >> 32);
  for (int j = 0; j < 3; ++j) triples[at * 3 + j] = (int32_t)s[j];
  float4 pl = make_float4(0.f, 0.f, 0.f, 0.f);
  int st = -1;
  if (K > 0 && s[0] != s[1] && s[0] != s[2] && s[1] != s[2]) {  // (slots are < K)
    const float4 *pts = cand_pts + jobs[job].cand_base;
    const float4 a = pts[s[0]], b = pts[s[1]], c = pts[s[2]];
    const double ux = (double)b.x - (double)a.x, uy = (double)b.y - (double)a.y, uz = (double)b.z - (double)a.z;
    const double vx = (double)c.x - (double)a.x, vy = (double)c.y - (double)a.y, vz = (double)c.z - (double)a.z;
    double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const double n2 = (nx * nx + ny * ny) + nz * nz;
    const double u2 = (ux * ux + uy * uy) + uz * uz, v2 = (vx * vx + vy * vy) + vz * vz;
    if (n2 > (1e-12 * u2) * v2) {
      const double len = sqrt(n2);
      nx /= len;
      ny /= len;
      nz /= len;
      double dot = (nx * P.up64[0] + ny * P.up64[1]) + nz * P.up64[2];
      if (dot < 0.0) {
        nx = -nx;
        ny = -ny;
        nz = -nz;
        dot = -dot;
      }
      const double d = -((nx * (double)a.x + ny * (double)a.y) + nz * (double)a.z);
      pl = make_float4((float)nx, (float)ny, (float)nz, (float)d);
      st = dot < P.cos_max ? -2 : 0;
    }
  }
  planes[at] = pl;
  hstat[at] = st;
}

__global__ __launch_bounds__(FLOOR_BLOCK) void floor_score_kernel(const FloorJob *__restrict__ jobs, const FloorOut *__restrict__ out,
                                                                  const float4 *__restrict__ cand_pts, const float4 *__restrict__ planes,
                                                                  const int32_t *__restrict__ hstat, int32_t *__restrict__ counts, const int H,
                                                                  const float thr) {
  const int job = blockIdx.z;
  const int K = out[job].K;
  const int first = blockIdx.x * FLOOR_TILE;
  if (first >= K) return;
  __shared__ float4 s_plane[64];
  __shared__ int s_cnt[64];
  const float4 *pts = cand_pts + jobs[job].cand_base;
  const int lane = threadIdx.x & 63;
  float px[FLOOR_PPL], py[FLOOR_PPL], pz[FLOOR_PPL];
#pragma unroll
  for (int r = 0; r < FLOOR_PPL; ++r) {
    const int i = first + r * FLOOR_BLOCK + (int)threadIdx.x;
    float4 p = make_float4(NAN, NAN, NAN, 0.f);  // a lane without a candidate: the test fails
    if (i < K) p = pts[i];
    px[r] = p.x;
    py[r] = p.y;
    pz[r] = p.z;
  }
  const int h0 = blockIdx.y * FLOOR_HCHUNK;
  const int h1 = h0 + FLOOR_HCHUNK < H ? h0 + FLOOR_HCHUNK : H;
  const size_t hb_job = (size_t)job * H;
  for (int hb = h0; hb < h1; hb += 64) {  // hb + 63 < H: H and the chunk are multiples of 64
    if (threadIdx.x < 64) {
      float4 pl = planes[hb_job + hb + threadIdx.x];
      if (hstat[hb_job + hb + threadIdx.x] < 0) pl = make_float4(NAN, NAN, NAN, NAN);
      s_plane[threadIdx.x] = pl;
      s_cnt[threadIdx.x] = 0;
    }
    __syncthreads();
    int acc = 0;
#pragma unroll 4
    for (int j = 0; j < 64; ++j) {
      const float4 pl = s_plane[j];
      int c = 0;
#pragma unroll
      for (int r = 0; r < FLOOR_PPL; ++r) {
        const float dist = ((pl.x * px[r] + pl.y * py[r]) + pl.z * pz[r]) + pl.w;
        c += __popcll(__ballot(fabsf(dist) <= thr));
      }
      acc = lane == j ? c : acc;
    }
    atomicAdd(&s_cnt[lane], acc);
    __syncthreads();
    if (threadIdx.x < 64 && s_cnt[threadIdx.x]) atomicAdd(&counts[hb_job + hb + threadIdx.x], s_cnt[threadIdx.x]);
    __syncthreads();
  }
}

// per cloud: the vote.  counts[h] becomes the tap's: the count, or the mark of an excluded hypothesis
__global__ __launch_bounds__(FLOOR_BLOCK) void floor_best_kernel(const float4 *planes, const int32_t *hstat, int32_t *counts, const int H,
                                                                 FloorOut *out, FloorPlane *cur) {
  const int job = blockIdx.x;
  const size_t at = (size_t)job * H;
  __shared__ int s_c[FLOOR_BLOCK], s_i[FLOOR_BLOCK];
  int bc = -1, bi = -1;
  for (int h = threadIdx.x; h < H; h += FLOOR_BLOCK) {  // ascending h: a later equal count does not replace an earlier one
    const int st = hstat[at + h];
    if (st < 0) {
      counts[at + h] = st;
      continue;
    }
    const int c = counts[at + h];
    if (c > bc) {
      bc = c;
      bi = h;
    }
  }
  s_c[threadIdx.x] = bc;
  s_i[threadIdx.x] = bi;
  __syncthreads();
  for (int s = FLOOR_BLOCK / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const int c2 = s_c[threadIdx.x + s], i2 = s_i[threadIdx.x + s];
      const int c1 = s_c[threadIdx.x], i1 = s_i[threadIdx.x];
      if (i2 >= 0 && (i1 < 0 || c2 > c1 || (c2 == c1 && i2 < i1))) {
        s_c[threadIdx.x] = c2;
        s_i[threadIdx.x] = i2;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int best = s_i[0];
    out[job].best = best;
    out[job].best_count = best >= 0 ? s_c[0] : 0;
    FloorPlane c;
    if (best >= 0) {
      const float4 pl = planes[at + best];
      c.p32 = pl;
      c.p64[0] = (double)pl.x;
      c.p64[1] = (double)pl.y;
      c.p64[2] = (double)pl.z;
      c.p64[3] = (double)pl.w;
    } else {
      c.p32 = make_float4(NAN, NAN, NAN, NAN);
      c.p64[0] = c.p64[1] = c.p64[2] = c.p64[3] = 0.0;
    }
    cur[job] = c;
  }
}

// The inliers of cur[job].p32 (the fp32 test of the scoring kernel) among the cloud's candidates: per tile one record of fp64
// sums.  A lane adds its four points in order, then the 256 lanes are summed by one fixed tree: no floating-point atomics.
__global__ __launch_bounds__(FLOOR_BLOCK) void floor_sums_kernel(const FloorJob *jobs, const FloorOut *out, const float4 *cand_pts,
                                                                 const FloorPlane *cur, const float thr, double *partials) {
  const int job = blockIdx.y;
  const FloorJob J = jobs[job];
  const int K = out[job].K;
  const int first = blockIdx.x * FLOOR_TILE;
  if ((uint32_t)first >= J.n) return;  // every tile of the cloud's INPUT writes its record (the reduce reads them all)
  __shared__ double s_sum[FLOOR_BLOCK];
  const FloorPlane c = cur[job];
  const float4 *pts = cand_pts + J.cand_base;
  double acc[FLOOR_NSUM];
  for (int k = 0; k < FLOOR_NSUM; ++k) acc[k] = 0.0;
  for (int r = 0; r < FLOOR_PPL; ++r) {
    const int i = first + r * FLOOR_BLOCK + (int)threadIdx.x;
    if (i >= K) continue;
    const float4 p = pts[i];
    const float dist = ((c.p32.x * p.x + c.p32.y * p.y) + c.p32.z * p.z) + c.p32.w;
    if (!(fabsf(dist) <= thr)) continue;
    const double x = p.x, y = p.y, z = p.z;
    const double d = ((c.p64[0] * x + c.p64[1] * y) + c.p64[2] * z) + c.p64[3];
    acc[0] += x;
    acc[1] += y;
    acc[2] += z;
    acc[3] += x * x;
    acc[4] += x * y;
    acc[5] += x * z;
    acc[6] += y * y;
    acc[7] += y * z;
    acc[8] += z * z;
    acc[9] += d * d;
    acc[10] += 1.0;
  }
  double *rec = partials + (size_t)(J.tile_base + blockIdx.x) * FLOOR_NSUM;
  for (int k = 0; k < FLOOR_NSUM; ++k) {
    s_sum[threadIdx.x] = acc[k];
    __syncthreads();
    for (int s = FLOOR_BLOCK / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) s_sum[threadIdx.x] += s_sum[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) rec[k] = s_sum[0];
    __syncthreads();
  }
}

// per cloud: lane t adds the records of tiles t, t + 256, ... in that order, then the same fixed tree
__global__ __launch_bounds__(FLOOR_BLOCK) void floor_reduce_kernel(const FloorJob *jobs, const double *partials, FloorOut *out) {
  const FloorJob J = jobs[blockIdx.x];
  const uint32_t tiles = (J.n + FLOOR_TILE - 1) / FLOOR_TILE;
  __shared__ double s_sum[FLOOR_BLOCK];
  for (int k = 0; k < FLOOR_NSUM; ++k) {
    double a = 0.0;
    for (uint32_t t = threadIdx.x; t < tiles; t += FLOOR_BLOCK) a += partials[(size_t)(J.tile_base + t) * FLOOR_NSUM + k];
    s_sum[threadIdx.x] = a;
    __syncthreads();
    for (int s = FLOOR_BLOCK / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) s_sum[threadIdx.x] += s_sum[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x].sums[k] = s_sum[0];
    __syncthreads();
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

void refuse(const char *what, const char *why) {
  char b[240];
  snprintf(b, sizeof(b), "%s: %s", what, why);
  lslam::set_error(b);
}

// Everything a call is refused for, before anything runs.  -> the device's form of the parameters
int check_params(const char *what, const lslam_floor_params *in, lslam_floor_params *p, FloorDev *P) {
  if (in) *p = *in;
  else lslam_floor_default_params(p);
  double u[3] = {p->up[0], p->up[1], p->up[2]};
  const double un = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  if (!std::isfinite(un) || !(un > 0.0)) return refuse(what, "up is zero or not finite"), LSLAM_ERR_INVALID;
  if (!(p->inlier_threshold > 0.0f) || !std::isfinite(p->inlier_threshold))
    return refuse(what, "inlier_threshold is not positive and finite"), LSLAM_ERR_INVALID;
  if (p->n_hypotheses < 64 || p->n_hypotheses > 4096 || (p->n_hypotheses & 63))
    return refuse(what, "n_hypotheses is not a multiple of 64 in [64, 4096]"), LSLAM_ERR_INVALID;
  if (p->min_inliers < 0) return refuse(what, "min_inliers is negative"), LSLAM_ERR_INVALID;
  if (p->refit_iterations < 0) return refuse(what, "refit_iterations is negative"), LSLAM_ERR_INVALID;
  if (!std::isfinite(p->sensor_height) || !std::isfinite(p->height_clip_range) || p->height_clip_range < 0.0f)
    return refuse(what, "sensor_height is not finite, or height_clip_range is negative or not finite"), LSLAM_ERR_INVALID;
  if (!std::isfinite(p->max_range) || p->max_range < 0.0f) return refuse(what, "max_range is negative or not finite"), LSLAM_ERR_INVALID;
  if (!std::isfinite(p->max_normal_angle_deg) || p->max_normal_angle_deg < 0.0f || p->max_normal_angle_deg > 180.0f)
    return refuse(what, "max_normal_angle_deg is outside [0, 180]"), LSLAM_ERR_INVALID;
  for (int k = 0; k < 3; ++k) {
    P->up64[k] = u[k] / un;
    P->up[k] = (float)P->up64[k];
  }
  P->h_lo = -(p->sensor_height + p->height_clip_range);
  P->h_hi = -(p->sensor_height - p->height_clip_range);
  P->use_range = p->max_range > 0.0f;
  P->range2 = p->max_range * p->max_range;
  P->thr = p->inlier_threshold;
  P->H = p->n_hypotheses;
  P->seed = p->seed;
  P->cos_max = std::cos((double)p->max_normal_angle_deg * (3.14159265358979323846 / 180.0));
  return LSLAM_OK;
}

// eigenvector of the smallest eigenvalue of the symmetric C by cyclic Jacobi rotations
void smallest_eigenvector(const double C[6], double n[3]) {
  double A[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}};
  double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 64; ++sweep) {
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
    const double dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
    if (off <= 1e-32 * dia || off == 0.0) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; ++k) {  // A <- A J
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; ++k) {  // A <- J^T A
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  int m = 0;
  for (int k = 1; k < 3; ++k)
    if (A[k][k] < A[m][m]) m = k;
  const double len = std::sqrt(V[0][m] * V[0][m] + V[1][m] * V[1][m] + V[2][m] * V[2][m]);
  for (int k = 0; k < 3; ++k) n[k] = V[k][m] / len;
}

struct Cloud {
  const float4 *p;
  size_t n;
};

// The whole detection of a batch on `s`; results[nj].  tap: the scratch keeps the first cloud's lists for lslam_debug_floor_hypotheses.
int detect_batch(const char *what, hipStream_t s, FloorScratch &F, const std::vector<Cloud> &clouds, const lslam_floor_params &prm,
                 const FloorDev &P, lslam_floor_result *results) {
  const int nj = (int)clouds.size();
  F.tap_valid = false;
  F.last_clouds = 0;
  if (nj == 0) return LSLAM_OK;
  const int H = P.H;
  size_t total = 0, tiles_total = 0, n_max = 0;
  LSLAM_TRY(F.h_jobs.reserve(nj));
  for (int j = 0; j < nj; ++j) {
    if (clouds[j].n >= ((size_t)1 << 31) || total + clouds[j].n >= ((size_t)1 << 31)) return refuse(what, "the clouds hold 2^31 points or more"), LSLAM_ERR_INVALID;
    FloorJob &J = F.h_jobs.p[j];
    J.pts = clouds[j].p;
    J.n = (uint32_t)clouds[j].n;
    J.cand_base = (uint32_t)total;
    J.tile_base = (uint32_t)tiles_total;
    total += clouds[j].n;
    tiles_total += (clouds[j].n + FLOOR_TILE - 1) / FLOOR_TILE;
    if (clouds[j].n > n_max) n_max = clouds[j].n;
  }
  const unsigned tiles_max = (unsigned)((n_max + FLOOR_TILE - 1) / FLOOR_TILE);
  LSLAM_TRY(F.d_jobs.reserve(nj));
  LSLAM_TRY(F.d_tile_cnt.reserve(tiles_total));
  LSLAM_TRY(F.d_tile_off.reserve(tiles_total));
  LSLAM_TRY(F.d_cand_idx.reserve(total));
  LSLAM_TRY(F.d_cand_pts.reserve(total));
  LSLAM_TRY(F.d_triples.reserve((size_t)nj * H * 3));
  LSLAM_TRY(F.d_planes.reserve((size_t)nj * H));
  LSLAM_TRY(F.d_hstat.reserve((size_t)nj * H));
  LSLAM_TRY(F.d_counts.reserve((size_t)nj * H));
  LSLAM_TRY(F.d_partials.reserve(tiles_total * FLOOR_NSUM));
  LSLAM_TRY(F.d_out.reserve(nj));
  LSLAM_TRY(F.h_out.reserve(nj));
  LSLAM_TRY(F.d_cur.reserve(nj));
  LSLAM_TRY(F.h_cur.reserve(nj));
  LSLAM_TRY(hipMemcpyAsync(F.d_jobs.p, F.h_jobs.p, nj * sizeof(FloorJob), hipMemcpyHostToDevice, s));
  LSLAM_TRY(hipMemsetAsync(F.d_counts.p, 0, (size_t)nj * H * sizeof(int32_t), s));
  LSLAM_TRY(hipMemsetAsync(F.d_out.p, 0, nj * sizeof(FloorOut), s));
  if (tiles_max) {
    hipLaunchKernelGGL(floor_mark_kernel, dim3(tiles_max, nj), dim3(FLOOR_BLOCK), 0, s, F.d_jobs.p, P, F.d_tile_cnt.p);
    hipLaunchKernelGGL(floor_scan_kernel, dim3(nj), dim3(FLOOR_BLOCK), 0, s, F.d_jobs.p, F.d_tile_cnt.p, F.d_tile_off.p, F.d_out.p);
    hipLaunchKernelGGL(floor_compact_kernel, dim3(tiles_max, nj), dim3(FLOOR_BLOCK), 0, s, F.d_jobs.p, P, F.d_tile_off.p, F.d_cand_idx.p,
                       F.d_cand_pts.p);
  }
  hipLaunchKernelGGL(floor_hypo_kernel, dim3(H / 64, nj), dim3(64), 0, s, F.d_jobs.p, P, F.d_out.p, F.d_cand_pts.p, F.d_triples.p,
                     F.d_planes.p, F.d_hstat.p);
  if (tiles_max)
    hipLaunchKernelGGL(floor_score_kernel, dim3(tiles_max, (H + FLOOR_HCHUNK - 1) / FLOOR_HCHUNK, nj), dim3(FLOOR_BLOCK), 0, s, F.d_jobs.p,
                       F.d_out.p, F.d_cand_pts.p, F.d_planes.p, F.d_hstat.p, F.d_counts.p, H, P.thr);
  hipLaunchKernelGGL(floor_best_kernel, dim3(nj), dim3(FLOOR_BLOCK), 0, s, F.d_planes.p, F.d_hstat.p, F.d_counts.p, H, F.d_out.p, F.d_cur.p);
  LSLAM_TRY(hipGetLastError());

  // the passes over the inliers: refit_iterations fits, then the final plane's statistics
  const int need = prm.min_inliers > 3 ? prm.min_inliers : 3;
  std::vector<int> live(nj, 1);  // still refitting
  for (int pass = 0; pass <= prm.refit_iterations; ++pass) {
    if (tiles_max) hipLaunchKernelGGL(floor_sums_kernel, dim3(tiles_max, nj), dim3(FLOOR_BLOCK), 0, s, F.d_jobs.p, F.d_out.p, F.d_cand_pts.p, F.d_cur.p, P.thr, F.d_partials.p);
    hipLaunchKernelGGL(floor_reduce_kernel, dim3(nj), dim3(FLOOR_BLOCK), 0, s, F.d_jobs.p, F.d_partials.p, F.d_out.p);
    LSLAM_TRY(hipGetLastError());
    LSLAM_TRY(hipMemcpyAsync(F.h_out.p, F.d_out.p, nj * sizeof(FloorOut), hipMemcpyDeviceToHost, s));
    if (pass == 0) LSLAM_TRY(hipMemcpyAsync(F.h_cur.p, F.d_cur.p, nj * sizeof(FloorPlane), hipMemcpyDeviceToHost, s));
    LSLAM_TRY(hipStreamSynchronize(s));
    bool any_live = false;
    for (int j = 0; j < nj; ++j) {
      lslam_floor_result &R = results[j];
      const FloorOut &O = F.h_out.p[j];
      if (pass == 0) {
        R.n_candidates = O.K;
        R.best_hypothesis = O.best;
        R.best_count = O.best_count;
        if (O.K < 3 || O.K < prm.min_inliers) {
          R.status = LSLAM_FLOOR_FEW_CANDIDATES;
          R.best_hypothesis = -1;
          R.best_count = 0;
          live[j] = 0;
        } else if (O.best < 0) {
          R.status = LSLAM_FLOOR_NO_HYPOTHESIS;
          live[j] = 0;
        } else {
          for (int k = 0; k < 4; ++k) R.plane[k] = F.h_cur.p[j].p64[k];
        }
      }
      if (!live[j]) continue;
      const double N = O.sums[10];
      R.n_inliers = (int32_t)N;
      R.rms_distance = N > 0.0 ? std::sqrt(O.sums[9] / N) : 0.0;
      if (R.n_inliers < need) {
        R.status = LSLAM_FLOOR_FEW_INLIERS;
        live[j] = 0;
        continue;
      }
      if (pass == prm.refit_iterations) continue;  // the final statistics: done
      const double c[3] = {O.sums[0] / N, O.sums[1] / N, O.sums[2] / N};
      const double C[6] = {O.sums[3] / N - c[0] * c[0], O.sums[4] / N - c[0] * c[1], O.sums[5] / N - c[0] * c[2],
                           O.sums[6] / N - c[1] * c[1], O.sums[7] / N - c[1] * c[2], O.sums[8] / N - c[2] * c[2]};
      double n[3];
      smallest_eigenvector(C, n);
      double dot = (n[0] * P.up64[0] + n[1] * P.up64[1]) + n[2] * P.up64[2];
      if (dot < 0.0) {
        for (int k = 0; k < 3; ++k) n[k] = -n[k];
        dot = -dot;
      }
      for (int k = 0; k < 3; ++k) R.plane[k] = n[k];
      R.plane[3] = -((n[0] * c[0] + n[1] * c[1]) + n[2] * c[2]);
      FloorPlane &cp = F.h_cur.p[j];
      cp.p32 = make_float4((float)R.plane[0], (float)R.plane[1], (float)R.plane[2], (float)R.plane[3]);
      for (int k = 0; k < 4; ++k) cp.p64[k] = R.plane[k];
      if (dot < P.cos_max) {
        R.status = LSLAM_FLOOR_STEEP;
        live[j] = 0;
        continue;
      }
      any_live = true;
    }
    if (!any_live) break;
    // the new planes up (small records, not points); a cloud that has ended keeps its last plane and is not read again
    LSLAM_TRY(hipMemcpyAsync(F.d_cur.p, F.h_cur.p, nj * sizeof(FloorPlane), hipMemcpyHostToDevice, s));
  }
  F.tap_valid = true;
  F.tap_K = results[0].n_candidates;
  F.tap_H = H;
  F.last_clouds = nj;
  F.last_H = H;
  F.last_tiles = tiles_max;
  F.last_thr = P.thr;
  return LSLAM_OK;
}

void clear_results(lslam_floor_result *r, size_t n) {
  if (!r) return;
  std::memset(r, 0, n * sizeof(*r));
  for (size_t i = 0; i < n; ++i) r[i].best_hypothesis = -1;
}

int check_ctx(lslam_ctx *ctx, const char *what) {
  if (!ctx || !lslam::ctx_alive(ctx)) return refuse(what, "null ctx"), LSLAM_ERR_INVALID;
  LSLAM_TRY(hipSetDevice(lslam::ctx_device(ctx)));
  return LSLAM_OK;
}

}  // namespace

extern "C" {

void lslam_floor_default_params(lslam_floor_params *p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->up[2] = 1.0f;
  p->sensor_height = 1.8f;
  p->height_clip_range = 1.0f;
  p->max_range = 0.0f;
  p->n_hypotheses = 512;
  p->inlier_threshold = 0.1f;
  p->min_inliers = 512;
  p->max_normal_angle_deg = 10.0f;
  p->refit_iterations = 1;
  p->seed = 1;
}

size_t lslam_sizeof_floor_params(void) { return sizeof(lslam_floor_params); }
size_t lslam_sizeof_floor_result(void) { return sizeof(lslam_floor_result); }

int lslam_floor_detect_device(lslam_ctx *ctx, const float *d_xyzi, size_t n, const lslam_floor_params *params, lslam_floor_result *result) {
  const char *what = "lslam_floor_detect_device";
  int rc = check_ctx(ctx, what);
  if (rc) return rc;
  if (!result || (n && !d_xyzi)) return refuse(what, "null result, or null cloud with points"), LSLAM_ERR_INVALID;
  lslam_floor_params prm;
  FloorDev P;
  rc = check_params(what, params, &prm, &P);
  if (rc) return rc;
  clear_results(result, 1);  // (only now: a refused call leaves the caller's result as it was)
  FloorScratch &F = *lslam::ctx_slot<FloorScratch>(ctx, lslam::CTX_SLOT_FLOOR);
  const std::vector<Cloud> clouds(1, Cloud{reinterpret_cast<const float4 *>(d_xyzi), n});
  rc = detect_batch(what, lslam::ctx_stream(ctx), F, clouds, prm, P, result);
  if (rc) (void)hipStreamSynchronize(lslam::ctx_stream(ctx));
  return rc;
}

int lslam_floor_detect(lslam_ctx *ctx, const void *points, size_t n, size_t stride_bytes, const lslam_floor_params *params,
                       lslam_floor_result *result) {
  const char *what = "lslam_floor_detect";
  int rc = check_ctx(ctx, what);
  if (rc) return rc;
  if (!result || (n && !points) || stride_bytes < 16 || (stride_bytes & 3))
    return refuse(what, "null result, null cloud with points, or a stride under 16 bytes"), LSLAM_ERR_INVALID;
  lslam_floor_params prm;
  FloorDev P;
  rc = check_params(what, params, &prm, &P);
  if (rc) return rc;
  if (n >= ((size_t)1 << 31)) return refuse(what, "the cloud holds 2^31 points or more"), LSLAM_ERR_INVALID;
  clear_results(result, 1);
  FloorScratch &F = *lslam::ctx_slot<FloorScratch>(ctx, lslam::CTX_SLOT_FLOOR);
  hipStream_t s = lslam::ctx_stream(ctx);
  LSLAM_TRY(F.h_cloud.reserve(n));
  LSLAM_TRY(F.d_cloud.reserve(n));
  const char *p = static_cast<const char *>(points);
  for (size_t i = 0; i < n; ++i) {  // {x, y, z}; the intensity is not read
    float v[3];
    std::memcpy(v, p + i * stride_bytes, 12);
    F.h_cloud.p[i] = make_float4(v[0], v[1], v[2], 0.0f);
  }
  if (n) LSLAM_TRY(hipMemcpyAsync(F.d_cloud.p, F.h_cloud.p, n * sizeof(float4), hipMemcpyHostToDevice, s));
  const std::vector<Cloud> clouds(1, Cloud{F.d_cloud.p, n});
  rc = detect_batch(what, s, F, clouds, prm, P, result);
  if (rc) (void)hipStreamSynchronize(s);
  return rc;
}

int lslam_floor_detect_keyframes(lslam_kfs *k, int32_t n_ids, const int32_t *ids, const lslam_floor_params *params,
                                 lslam_floor_result *results) {
  const char *what = "lslam_floor_detect_keyframes";
  int rc = lslam::check_kfs(k, what);
  if (rc) return rc;
  if (n_ids < 0 || n_ids > FLOOR_MAX_CLOUDS || (n_ids && (!ids || !results)))
    return refuse(what, "between 0 and 65535 keyframes, with their ids and results"), LSLAM_ERR_INVALID;
  lslam_floor_params prm;
  FloorDev P;
  rc = check_params(what, params, &prm, &P);
  if (rc) return rc;
  std::vector<Cloud> clouds((size_t)n_ids);
  for (int32_t i = 0; i < n_ids; ++i) {
    rc = lslam::check_id(k, what, ids[i]);
    if (rc) return rc;
    const lslam::KeyframeClouds &kc = k->kfs[(size_t)ids[i]];
    clouds[(size_t)i] = Cloud{kc.p[1], kc.n[1]};
  }
  clear_results(results, (size_t)n_ids);
  rc = detect_batch(what, k->stream, k->floor, clouds, prm, P, results);
  if (rc) (void)hipStreamSynchronize(k->stream);
  return rc;
}

int lslam_debug_floor_score(lslam_kfs *k, int32_t launches) {
  const char *what = "lslam_debug_floor_score";
  int rc = lslam::check_kfs(k, what);
  if (rc) return rc;
  FloorScratch &F = k->floor;
  if (launches < 0 || F.last_clouds == 0 || F.last_tiles == 0)
    return refuse(what, "a negative count, or no lslam_floor_detect_keyframes call with points has run on this store"), LSLAM_ERR_INVALID;
  const size_t n = (size_t)F.last_clouds * F.last_H;
  LSLAM_TRY(F.d_counts_again.reserve(n));
  LSLAM_TRY(hipMemsetAsync(F.d_counts_again.p, 0, n * sizeof(int32_t), k->stream));
  for (int32_t i = 0; i < launches; ++i)
    hipLaunchKernelGGL(floor_score_kernel, dim3(F.last_tiles, (F.last_H + FLOOR_HCHUNK - 1) / FLOOR_HCHUNK, F.last_clouds), dim3(FLOOR_BLOCK), 0,
                       k->stream, F.d_jobs.p, F.d_out.p, F.d_cand_pts.p, F.d_planes.p, F.d_hstat.p, F.d_counts_again.p, F.last_H, F.last_thr);
  LSLAM_TRY(hipGetLastError());
  return LSLAM_OK;
}

int lslam_debug_floor_hypotheses(lslam_ctx *ctx, int32_t *cand_idx, size_t cap_candidates, size_t *n_candidates, int32_t *triples,
                                 float *planes, int32_t *counts, size_t cap_hypotheses, size_t *n_hypotheses) {
  const char *what = "lslam_debug_floor_hypotheses";
  if (n_candidates) *n_candidates = 0;
  if (n_hypotheses) *n_hypotheses = 0;
  int rc = check_ctx(ctx, what);
  if (rc) return rc;
  FloorScratch &F = *lslam::ctx_slot<FloorScratch>(ctx, lslam::CTX_SLOT_FLOOR);
  if (!F.tap_valid) return refuse(what, "no single-cloud detection has run on this ctx"), LSLAM_ERR_INVALID;
  const size_t K = (size_t)F.tap_K, H = (size_t)F.tap_H;
  if (n_candidates) *n_candidates = K;
  if (n_hypotheses) *n_hypotheses = H;
  if ((cand_idx && cap_candidates < K) || ((triples || planes || counts) && cap_hypotheses < H))
    return refuse(what, "output buffer too small"), LSLAM_ERR_INVALID;
  hipStream_t s = lslam::ctx_stream(ctx);
  // (the first cloud of the scratch: its candidate slice and its hypotheses start at 0)
  if (cand_idx && K) LSLAM_TRY(hipMemcpyAsync(cand_idx, F.d_cand_idx.p, K * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (triples) LSLAM_TRY(hipMemcpyAsync(triples, F.d_triples.p, H * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (planes) LSLAM_TRY(hipMemcpyAsync(planes, F.d_planes.p, H * sizeof(float4), hipMemcpyDeviceToHost, s));
  if (counts) LSLAM_TRY(hipMemcpyAsync(counts, F.d_counts.p, H * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  LSLAM_TRY(hipStreamSynchronize(s));
  return LSLAM_OK;
}

}  // extern "C"
