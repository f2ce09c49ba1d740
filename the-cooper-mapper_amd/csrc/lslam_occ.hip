// lslam_occ.hip -- the 2D occupancy grid from the keyframe store: every point of every keyframe is a ray from the sensor to the
// point, the cells it crosses were seen free, the cell it ends in -- at obstacle height above the keyframe's floor plane -- was
// seen occupied -- lslam_occ_* of include/lslam_c.h, whose comment is the specification; DESIGN 8i.  Not in the reference.
//
// Kernels:
//   occ_ray_kernel      grid (tiles of LSLAM_OCC_RAY_TILE points, the keyframes of a chunk).  One point per lane: gate, height
//                       class, fp32 transform, fp64 quantisation to 1/256 cell; the end cell's bit goes into the keyframe's HIT
//                       plane.  Then the tile's (ray, column) items -- a column is one cell step along the ray's major axis --
//                       are dealt to the lanes through a prefix sum of the rays' column counts: rays are 1 .. ~400 cells long,
//                       and a lane that walked its own ray would keep its wave waiting for the longest.  The cells a ray
//                       crosses inside one column follow in closed form from the integer line equation (two int64 divisions),
//                       no column depends on the one before; their bits go into the keyframe's FREE plane.  Bits are ORed
//                       (a plain load first: near the sensor every ray sets the same few bits).
//   occ_merge_kernel    per word of a keyframe's window: HIT bits add 1 << 16, FREE bits that are not HIT add 1, into the global
//                       counts with an integer atomic add (the windows of a chunk's keyframes overlap).
//   occ_values_kernel   the int8 values from the counts.
// Only integer OR / add combine values across lanes: nothing depends on arrival order, two calls give the same bits.
#include "../../include/lslam_c.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>

#include "lslam_internal.hpp"
#include "lslam_kfs_impl.hpp"

namespace {

using lslam::OccJob;
using lslam::OccState;
using lslam::check_id;
using lslam::check_kfs;

constexpr int OCC_BLOCK = LSLAM_OCC_RAY_TILE;
constexpr int OCC_CHUNK = LSLAM_OCC_KF_CHUNK;
static_assert(OCC_BLOCK == 256, "one point per lane, four waves per tile");
constexpr int32_t OCC_MAX_IDS = 65535;  // n_free and n_hit fit 16 bits each
constexpr int32_t OCC_MAX_SIDE = 8192;
constexpr int64_t OCC_MAX_CELLS = (int64_t)1 << 26;
constexpr double OCC_FIX_LIMIT = 1073741824.0;  // 2^30
enum { OCC_ST_DROPPED = 1, OCC_ST_OBSTACLE, OCC_ST_GROUND, OCC_ST_ESCAPED, OCC_ST_N = 8 };  // slots of the device counters

struct OccShape {
  int32_t width, height, up_axis, ground_clears;
  float lo2, hi2, obstacle_min, obstacle_max, ground_band;
  double ra, rb, scale;
};

// floor / ceiling of n / d, d > 0
__device__ __forceinline__ int64_t occ_floordiv(int64_t n, int64_t d) {
  const int64_t q = n / d;
  return (n % d < 0) ? q - 1 : q;
}
__device__ __forceinline__ int64_t occ_ceildiv(int64_t n, int64_t d) {
  const int64_t q = n / d;
  return (n % d > 0) ? q + 1 : q;
}

// the bit of grid cell (ci, cj) -- inside the grid -- in a plane of the keyframe's window
__device__ __forceinline__ void occ_set(const OccJob &job, uint32_t *plane, int ci, int cj, unsigned long long *stats) {
  const int wi = ci - job.wi0, wj = cj - job.wj0;
  if ((unsigned)wi >= (unsigned)job.ww || (unsigned)wj >= (unsigned)job.wh) {  // cannot happen (the header's WINDOW): reported, not lost
    atomicAdd(&stats[OCC_ST_ESCAPED], 1ull);
    return;
  }
  const uint32_t bit = (uint32_t)wj * (uint32_t)job.ww + (uint32_t)wi;  // (< ww * wh <= 2^26: inside the plane's `words`)
  uint32_t *w = plane + (bit >> 5);
  const uint32_t m = 1u << (bit & 31u);
  if (!(*w & m)) atomicOr(w, m);
}

__global__ __launch_bounds__(OCC_BLOCK) void occ_ray_kernel(const OccJob *__restrict__ jobs, const OccShape sh, uint32_t *planes,
                                                             unsigned long long *stats) {
  __shared__ int32_t s_bx[OCC_BLOCK], s_by[OCC_BLOCK], s_c0[OCC_BLOCK];
  __shared__ uint32_t s_flag[OCC_BLOCK];  // 1: obstacle, 2: the major axis is a, 4: zero length
  __shared__ uint32_t s_off[OCC_BLOCK + 1];
  __shared__ uint32_t s_wave[OCC_BLOCK / 64];
  const OccJob job = jobs[blockIdx.y];  // the same in every lane: scalar loads, held in SGPRs
  const uint32_t n = job.n[0] + job.n[1];
  if (blockIdx.x * (uint32_t)OCC_BLOCK >= n) return;  // (the whole workgroup: before any barrier)
  const uint32_t tid = threadIdx.x, i = blockIdx.x * OCC_BLOCK + tid;
  uint32_t *hit = planes + job.plane_at, *fre = hit + job.words;
  const int32_t ax = job.ax, ay = job.ay;

  bool ray = false, dropped = false, obstacle = false;
  int32_t bx = 0, by = 0;
  if (i < n) {
    const float4 p = i < job.n[0] ? job.p[0][i] : job.p[1][i - job.n[0]];
    if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
      const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(p.x, p.x), __fmul_rn(p.y, p.y)), __fmul_rn(p.z, p.z));
      if (d2 >= sh.lo2 && d2 <= sh.hi2) {
        const float hgt = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(job.plane[0], p.x), __fmul_rn(job.plane[1], p.y)),
                                              __fmul_rn(job.plane[2], p.z)), job.plane[3]);
        obstacle = hgt >= sh.obstacle_min && hgt <= sh.obstacle_max;
        const bool ground = sh.ground_clears && fabsf(hgt) <= sh.ground_band;
        if (obstacle || ground) {
          const float *Ta = job.T + (sh.up_axis == 1 ? 8 : 0), *Tb = job.T + (sh.up_axis == 1 ? 0 : 4);
          const float ea = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(Ta[0], p.x), __fmul_rn(Ta[1], p.y)), __fmul_rn(Ta[2], p.z)), Ta[3]);
          const float eb = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(Tb[0], p.x), __fmul_rn(Tb[1], p.y)), __fmul_rn(Tb[2], p.z)), Tb[3]);
          const double qa = floor(__dmul_rn(__dsub_rn((double)ea, sh.ra), sh.scale));
          const double qb = floor(__dmul_rn(__dsub_rn((double)eb, sh.rb), sh.scale));
          ray = job.a_ok && qa >= -OCC_FIX_LIMIT && qa < OCC_FIX_LIMIT && qb >= -OCC_FIX_LIMIT && qb < OCC_FIX_LIMIT;  // (NaN: false)
          dropped = !ray;
          if (ray) bx = (int32_t)qa, by = (int32_t)qb;
        }
      }
    }
  }
  {  // the ray counters: one atomic per wave and counter
    const unsigned long long md = __ballot(dropped), mo = __ballot(ray && obstacle), mg = __ballot(ray && !obstacle);
    if ((tid & 63u) == 0) {
      if (md) atomicAdd(&stats[OCC_ST_DROPPED], (unsigned long long)__popcll(md));
      if (mo) atomicAdd(&stats[OCC_ST_OBSTACLE], (unsigned long long)__popcll(mo));
      if (mg) atomicAdd(&stats[OCC_ST_GROUND], (unsigned long long)__popcll(mg));
    }
  }
  // the end cell, and the ray's columns inside the grid
  uint32_t ncol = 0, flag = obstacle ? 1u : 0u;
  int32_t c0 = 0;
  if (ray) {
    const int ei = bx >> 8, ej = by >> 8;  // (arithmetic shifts: floor)
    if (obstacle && ei >= 0 && ei < sh.width && ej >= 0 && ej < sh.height) occ_set(job, hit, ei, ej, stats);
    const int64_t dx = (int64_t)bx - ax, dy = (int64_t)by - ay;
    const bool major_a = (dx < 0 ? -dx : dx) >= (dy < 0 ? -dy : dy);
    if (major_a) flag |= 2u;
    if (dx == 0 && dy == 0) {
      const int ci = ax >> 8, cj = ay >> 8;
      flag |= 4u;
      ncol = ((ax & 255) && (ay & 255) && ci >= 0 && ci < sh.width && cj >= 0 && cj < sh.height) ? 1u : 0u;
    } else {
      const int32_t au = major_a ? ax : ay, bu = major_a ? bx : by, ext = major_a ? sh.width : sh.height;
      const int32_t umin = au < bu ? au : bu, umax = au < bu ? bu : au;
      int32_t first = umin >> 8, last = ((umax + 255) >> 8) - 1;  // the columns whose open interval meets (umin, umax)
      if (first < 0) first = 0;
      if (last > ext - 1) last = ext - 1;
      c0 = first;
      ncol = last >= first ? (uint32_t)(last - first + 1) : 0u;
    }
  }
  s_bx[tid] = bx;
  s_by[tid] = by;
  s_c0[tid] = c0;
  s_flag[tid] = flag;
  // exclusive prefix sum of ncol over the tile (<= 256 * 8192 items)
  uint32_t incl = ncol;
  const int lane = (int)(tid & 63u), wv = (int)(tid >> 6);
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(incl, d, 64);
    if (lane >= d) incl += t;
  }
  if (lane == 63) s_wave[wv] = incl;
  __syncthreads();
  uint32_t before = 0, total = 0;
  for (int j = 0; j < OCC_BLOCK / 64; ++j) {
    before += j < wv ? s_wave[j] : 0u;
    total += s_wave[j];
  }
  s_off[tid] = before + incl - ncol;
  if (tid == 0) s_off[OCC_BLOCK] = total;
  __syncthreads();

  for (uint32_t it = tid; it < total; it += OCC_BLOCK) {
    uint32_t lo = 0, hi = OCC_BLOCK;  // the ray r with s_off[r] <= it < s_off[r + 1]
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (s_off[mid] <= it) lo = mid;
      else hi = mid;
    }
    const uint32_t r = lo, f = s_flag[r];
    const int32_t rbx = s_bx[r], rby = s_by[r];
    const int ei = rbx >> 8, ej = rby >> 8;
    if (f & 4u) {  // zero length: its own cell (it is the end cell too, so only a ground ray clears it)
      if (!(f & 1u)) occ_set(job, fre, ax >> 8, ay >> 8, stats);
      continue;
    }
    const bool major_a = (f & 2u) != 0;
    const int32_t c = s_c0[r] + (int32_t)(it - s_off[r]);
    const int32_t au = major_a ? ax : ay, av = major_a ? ay : ax, bu = major_a ? rbx : rby, bv = major_a ? rby : rbx;
    int64_t du = (int64_t)bu - au, dv = (int64_t)bv - av;
    if (du < 0) du = -du, dv = -dv;  // the same slope, du > 0
    const int32_t umin = au < bu ? au : bu, umax = au < bu ? bu : au;
    const int32_t cl = c * 256, cr = cl + 256;
    const int64_t ul = cl > umin ? cl : umin, ur = cr < umax ? cr : umax;  // (ul < ur: the column meets the ray)
    const int64_t nl = dv * (ul - au), nr = dv * (ur - au);               // |.| < 2^31 * 2^31
    const int64_t vlo = av + occ_floordiv(dv >= 0 ? nl : nr, du), vhi = av + occ_ceildiv(dv >= 0 ? nr : nl, du);
    int64_t j0 = vlo >> 8, j1 = ((vhi + 255) >> 8) - 1;  // cells with 256 j < vhi and vlo < 256 (j + 1): at most two, |dv| <= du
    const int32_t extv = major_a ? sh.height : sh.width;
    if (j0 < 0) j0 = 0;
    if (j1 > extv - 1) j1 = extv - 1;
    for (int64_t j = j0; j <= j1; ++j) {
      const int ci = major_a ? c : (int)j, cj = major_a ? (int)j : c;
      if ((f & 1u) && ci == ei && cj == ej) continue;  // an obstacle ray does not clear its own end cell
      occ_set(job, fre, ci, cj, stats);
    }
  }
}

__global__ __launch_bounds__(OCC_BLOCK) void occ_merge_kernel(const OccJob *__restrict__ jobs, const uint32_t *__restrict__ planes, int32_t width, uint32_t *counts) {
  const OccJob job = jobs[blockIdx.y];
  const uint32_t *hit = planes + job.plane_at, *fre = hit + job.words;
  const uint32_t ww = (uint32_t)job.ww, bits = (uint32_t)job.ww * (uint32_t)job.wh;
  for (uint32_t w = blockIdx.x * OCC_BLOCK + threadIdx.x; w < job.words; w += gridDim.x * OCC_BLOCK) {
    const uint32_t h = hit[w], f = fre[w] & ~h;
    uint32_t any = h | f;
    while (any) {
      const uint32_t b = (uint32_t)__ffs((int)any) - 1u;
      any &= any - 1u;
      const uint32_t bit = w * 32u + b;
      if (bit >= bits) break;  // (never set: occ_set stays below ww * wh)
      const uint32_t wj = bit / ww, wi = bit - wj * ww;
      // (wi0 + wi < width, wj0 + wj < height: the window lies in the grid)
      atomicAdd(&counts[(size_t)(job.wj0 + (int32_t)wj) * (size_t)width + (size_t)(job.wi0 + (int32_t)wi)], ((h >> b) & 1u) ? 0x10000u : 1u);
    }
  }
}

__global__ __launch_bounds__(OCC_BLOCK) void occ_values_kernel(const uint32_t *counts, size_t n, uint32_t hit_weight, uint32_t min_obs,
                                                                int8_t *values) {
  for (size_t i = (size_t)blockIdx.x * OCC_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * OCC_BLOCK) {
    const uint32_t word = counts[i], n_free = word & 0xffffu, n_hit = word >> 16;
    const uint32_t H = hit_weight * n_hit, D = H + n_free;  // <= 17 * 65535
    values[i] = (n_hit + n_free < min_obs) ? (int8_t)-1 : (int8_t)((200u * H + D) / (2u * D));  // (min_obs >= 1: D > 0 here)
  }
}

void occ_error(const char *fmt, const char *what, double v) {
  char b[240];
  snprintf(b, sizeof(b), fmt, what, v);
  lslam::set_error(b);
}

// the limits fit_bounds and setup share; 0: fine
int occ_check_scale(const char *what, const lslam_occ_params &p) {
  if (!std::isfinite(p.resolution) || !(p.resolution >= 0.01f)) occ_error("%s: resolution %g is not a finite length of at least 0.01", what, p.resolution);
  else if (p.up_axis != 1 && p.up_axis != 2) occ_error("%s: up_axis %g is neither 1 (y up) nor 2 (z up)", what, p.up_axis);
  else if (!std::isfinite(p.min_range) || !(p.min_range > 0.0f)) occ_error("%s: min_range %g is not a positive finite length", what, p.min_range);
  else if (!std::isfinite(p.max_range) || !(p.max_range > p.min_range)) occ_error("%s: max_range %g is not a finite length above min_range", what, p.max_range);
  else if (!(p.max_range / p.resolution <= 2048.0f)) occ_error("%s: max_range / resolution = %g is above 2048 cells", what, p.max_range / p.resolution);
  else return LSLAM_OK;
  return LSLAM_ERR_INVALID;
}

int occ_check_size(const char *what, int64_t width, int64_t height) {
  char b[240];
  if (width < 1 || width > OCC_MAX_SIDE || height < 1 || height > OCC_MAX_SIDE || width * height > OCC_MAX_CELLS) {
    snprintf(b, sizeof(b), "%s: a grid of width %lld x height %lld cells is outside 1 .. %d per side and %lld cells in all", what,
             (long long)width, (long long)height, OCC_MAX_SIDE, (long long)OCC_MAX_CELLS);
    lslam::set_error(b);
    return LSLAM_ERR_INVALID;
  }
  return LSLAM_OK;
}

int occ_check_params(const char *what, const lslam_occ_params &p) {
  int rc = occ_check_scale(what, p);
  if (rc) return rc;
  if (!std::isfinite(p.origin[0]) || !std::isfinite(p.origin[1])) occ_error("%s: origin is not finite (%g)", what, p.origin[0]);
  else if ((rc = occ_check_size(what, p.width, p.height))) return rc;
  else if (!std::isfinite(p.obstacle_min) || !std::isfinite(p.obstacle_max) || !(p.obstacle_min < p.obstacle_max))
    occ_error("%s: obstacle_min %g is not finite and below a finite obstacle_max", what, p.obstacle_min);
  else if (!std::isfinite(p.ground_band) || !(p.ground_band >= 0.0f) || !(p.ground_band < p.obstacle_min))
    occ_error("%s: ground_band %g is not within [0, obstacle_min)", what, p.ground_band);
  else if (!std::isfinite(p.sensor_height)) occ_error("%s: sensor_height %g is not finite", what, p.sensor_height);
  else if (p.ground_clears != 0 && p.ground_clears != 1) occ_error("%s: ground_clears %g is neither 0 nor 1", what, p.ground_clears);
  else if (p.hit_weight < 1 || p.hit_weight > 16) occ_error("%s: hit_weight %g outside 1 .. 16", what, p.hit_weight);
  else if (p.min_observations < 1) occ_error("%s: min_observations %g below 1", what, p.min_observations);
  else if (p.reserved != 0) occ_error("%s: reserved %g is not 0", what, p.reserved);
  else return LSLAM_OK;
  return LSLAM_ERR_INVALID;
}

int occ_ready(lslam_kfs *k, const char *what) {
  if (!k->occ.set) {
    char b[200];
    snprintf(b, sizeof(b), "%s: lslam_occ_setup was not called on this store", what);
    lslam::set_error(b);
    return LSLAM_ERR_INVALID;
  }
  return LSLAM_OK;
}

// the counts and values, zeroed, if the store holds none (enqueued)
int occ_ensure_grid(lslam_kfs *k) {
  OccState &o = k->occ;
  if (o.held()) return LSLAM_OK;
  const size_t n = o.cells();
  hipError_t e = o.d_counts.alloc(n);
  if (e == hipSuccess) e = o.d_values.alloc(n);
  if (e == hipSuccess) e = hipMemsetAsync(o.d_counts.p, 0, n * sizeof(uint32_t), k->stream);
  if (e != hipSuccess) {
    o.d_counts.release();
    o.d_values.release();
    char b[200];
    snprintf(b, sizeof(b), "occupancy: the grid could not be allocated: %s", hipGetErrorString(e));
    lslam::set_error(b);
    return LSLAM_ERR_HIP;
  }
  o.zero_tallies();
  return LSLAM_OK;
}

OccShape occ_shape(const OccState &o) {
  OccShape sh{};
  sh.width = o.params.width;
  sh.height = o.params.height;
  sh.up_axis = o.params.up_axis;
  sh.ground_clears = o.params.ground_clears;
  sh.lo2 = o.params.min_range * o.params.min_range;  // (-ffp-contract=off: one fp32 product each)
  sh.hi2 = o.params.max_range * o.params.max_range;
  sh.obstacle_min = o.params.obstacle_min;
  sh.obstacle_max = o.params.obstacle_max;
  sh.ground_band = o.params.ground_band;
  sh.ra = o.params.origin[0];
  sh.rb = o.params.origin[1];
  sh.scale = o.scale;
  return sh;
}

// Q of the header, as a double (a whole number, or not finite)
double occ_q(double v, double r, double scale) { return std::floor((v - r) * scale); }

// The header's WINDOW along one axis: the cells first .. first + count - 1 of `extent` that pose row `row` can reach.
void occ_window(const float *row, double r, double scale, double max_range, int32_t extent, int32_t *first, int32_t *count) {
  const double r0 = row[0], r1 = row[1], r2 = row[2], t = row[3];
  const double norm = std::sqrt((r0 * r0 + r1 * r1) + r2 * r2), sum = (std::fabs(r0) + std::fabs(r1)) + std::fabs(r2);
  const double L = norm * max_range * (1.0 + 1e-6) + 1e-6 * (sum * max_range + std::fabs(t)) + 1e-30;
  const double lo = std::floor(occ_q(t - L, r, scale) / 256.0), hi = std::floor(occ_q(t + L, r, scale) / 256.0);
  *first = 0;
  *count = 0;
  if (!(lo <= hi) || hi < 0.0 || lo > (double)(extent - 1)) return;
  const int32_t a = lo < 0.0 ? 0 : (int32_t)lo, b = hi > (double)(extent - 1) ? extent - 1 : (int32_t)hi;
  *first = a;
  *count = b - a + 1;
}

// the chunk [c0, c1) of the jobs in h_jobs: its scratch words and its longest cloud
void occ_chunk_shape(const OccState &o, int32_t c0, int32_t c1, size_t *words, size_t *most, uint32_t *most_words) {
  *words = 0;
  *most = 0;
  *most_words = 0;
  for (int32_t i = c0; i < c1; ++i) {
    const OccJob &j = o.h_jobs.p[i];
    *words += 2 * (size_t)j.words;
    if ((size_t)j.n[0] + j.n[1] > *most) *most = (size_t)j.n[0] + j.n[1];
    if (j.words > *most_words) *most_words = j.words;
  }
}

// One chunk's bit planes zeroed and its ray kernel (enqueued); with `merge`, the merge into the counts behind it.
int occ_launch_chunk(lslam_kfs *k, int32_t c0, int32_t c1, uint32_t *d_planes, unsigned long long *d_stats, bool merge) {
  OccState &o = k->occ;
  size_t words, most;
  uint32_t most_words;
  occ_chunk_shape(o, c0, c1, &words, &most, &most_words);
  if (!most) return LSLAM_OK;  // no point: no ray, no bit
  if (words) LSLAM_TRY(hipMemsetAsync(d_planes, 0, words * sizeof(uint32_t), k->stream));
  const dim3 grid((unsigned)((most + OCC_BLOCK - 1) / OCC_BLOCK), (unsigned)(c1 - c0));
  hipLaunchKernelGGL(occ_ray_kernel, grid, dim3(OCC_BLOCK), 0, k->stream, o.d_jobs.p + c0, occ_shape(o), d_planes, d_stats);
  LSLAM_TRY(hipGetLastError());
  if (!merge) return LSLAM_OK;
  ++o.ray_launches;
  if (!most_words) return LSLAM_OK;
  const size_t mb = ((size_t)most_words + OCC_BLOCK - 1) / OCC_BLOCK;
  hipLaunchKernelGGL(occ_merge_kernel, dim3((unsigned)(mb < 1024 ? mb : 1024), (unsigned)(c1 - c0)), dim3(OCC_BLOCK), 0, k->stream,
                     o.d_jobs.p + c0, d_planes, o.params.width, o.d_counts.p);
  LSLAM_TRY(hipGetLastError());
  ++o.merge_launches;
  return LSLAM_OK;
}

int occ_fail(lslam_kfs *k, int rc) {  // an error after work was enqueued: the stream is drained first
  (void)hipStreamSynchronize(k->stream);
  return rc;
}

int occ_fresh_values(lslam_kfs *k) {
  OccState &o = k->occ;
  if (!o.values_stale) return LSLAM_OK;
  const size_t n = o.cells(), nb = (n + OCC_BLOCK - 1) / OCC_BLOCK;
  hipLaunchKernelGGL(occ_values_kernel, dim3((unsigned)(nb < 2048 ? nb : 2048)), dim3(OCC_BLOCK), 0, k->stream, o.d_counts.p, n,
                     (uint32_t)o.params.hit_weight, (uint32_t)o.params.min_observations, o.d_values.p);
  LSLAM_TRY(hipGetLastError());
  ++o.value_launches;
  o.values_stale = false;
  return LSLAM_OK;
}

int occ_entry(lslam_kfs *k, const char *what) {
  const int rc = check_kfs(k, what);
  if (rc) return rc;
  return occ_ready(k, what);
}

}  // namespace

extern "C" {

void lslam_occ_default_params(lslam_occ_params *p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->resolution = 0.1f;
  p->up_axis = 1;
  p->min_range = 1.0f;
  p->max_range = 40.0f;
  p->obstacle_min = 0.3f;
  p->obstacle_max = 2.0f;
  p->ground_band = 0.15f;
  p->sensor_height = 1.8f;
  p->ground_clears = 1;
  p->hit_weight = 3;
  p->min_observations = 1;
}

size_t lslam_sizeof_occ_params(void) { return sizeof(lslam_occ_params); }
size_t lslam_sizeof_occ_stats(void) { return sizeof(lslam_occ_stats); }

int lslam_occ_setup(lslam_kfs *k, const lslam_occ_params *params) {
  int rc = check_kfs(k, "lslam_occ_setup");
  if (rc) return rc;
  if (!params) {
    lslam::set_error("lslam_occ_setup: null params (width and height have no default)");
    return LSLAM_ERR_INVALID;
  }
  const lslam_occ_params p = *params;
  rc = occ_check_params("lslam_occ_setup", p);
  if (rc) return rc;
  OccState &o = k->occ;
  if (o.set && std::memcmp(&o.params, &p, sizeof(p)) == 0) return LSLAM_OK;
  LSLAM_TRY(hipStreamSynchronize(k->stream));
  o.drop();
  o.params = p;
  o.scale = 256.0 / (double)p.resolution;
  o.set = true;
  return LSLAM_OK;
}

int lslam_occ_info(lslam_kfs *k, lslam_occ_stats *out) {
  const int rc = check_kfs(k, "lslam_occ_info");
  if (rc) return rc;
  if (!out) {
    lslam::set_error("lslam_occ_info: null out");
    return LSLAM_ERR_INVALID;
  }
  std::memset(out, 0, sizeof(*out));
  const OccState &o = k->occ;
  if (o.set) out->params = o.params;
  out->is_set = o.set ? 1 : 0;
  out->n_integrated = o.n_integrated;
  out->rays_cast = o.rays[0];
  out->rays_dropped = o.rays[1];
  out->rays_obstacle = o.rays[2];
  out->rays_ground = o.rays[3];
  out->grid_bytes = (uint64_t)o.grid_bytes();
  out->scratch_bytes = (uint64_t)o.scratch_bytes();
  out->ray_launches = o.ray_launches;
  out->merge_launches = o.merge_launches;
  out->value_launches = o.value_launches;
  return LSLAM_OK;
}

int lslam_occ_clear(lslam_kfs *k) {
  const int rc = occ_entry(k, "lslam_occ_clear");
  if (rc) return rc;
  OccState &o = k->occ;
  if (o.held()) {
    LSLAM_TRY(hipMemsetAsync(o.d_counts.p, 0, o.cells() * sizeof(uint32_t), k->stream));
    LSLAM_TRY(hipStreamSynchronize(k->stream));
  }
  o.zero_tallies();
  return LSLAM_OK;
}

int lslam_occ_integrate(lslam_kfs *k, int32_t n_ids, const int32_t *ids, const float *poses, const double *planes,
                        const int32_t *plane_valid) {
  const char *what = "lslam_occ_integrate";
  int rc = occ_entry(k, what);
  if (rc) return rc;
  char b[240];
  if (n_ids < 0 || n_ids > OCC_MAX_IDS || (n_ids && (!ids || !poses))) {
    snprintf(b, sizeof(b), "%s: n_ids outside 0 .. %d, or null ids / poses", what, OCC_MAX_IDS);
    lslam::set_error(b);
    return LSLAM_ERR_INVALID;
  }
  OccState &o = k->occ;
  for (int32_t i = 0; i < n_ids; ++i) {
    rc = check_id(k, what, ids[i]);
    if (rc) return rc;
    for (int e = 0; e < 12; ++e)
      if (!std::isfinite(poses[16 * (size_t)i + e])) {
        snprintf(b, sizeof(b), "%s: pose %d is not finite", what, i);
        lslam::set_error(b);
        return LSLAM_ERR_INVALID;
      }
    if (planes && (!plane_valid || plane_valid[i])) {
      const double *pl = planes + 4 * (size_t)i;
      const float f[4] = {(float)pl[0], (float)pl[1], (float)pl[2], (float)pl[3]};
      if (!(std::isfinite(f[0]) && std::isfinite(f[1]) && std::isfinite(f[2]) && std::isfinite(f[3]))) {
        snprintf(b, sizeof(b), "%s: plane %d is not finite", what, i);
        lslam::set_error(b);
        return LSLAM_ERR_INVALID;
      }
      if (f[0] == 0.0f && f[1] == 0.0f && f[2] == 0.0f) {
        snprintf(b, sizeof(b), "%s: plane %d has a normal of zero length", what, i);
        lslam::set_error(b);
        return LSLAM_ERR_INVALID;
      }
    }
  }
  if (o.n_integrated + n_ids > OCC_MAX_IDS) {
    snprintf(b, sizeof(b), "%s: %d keyframes on top of the %d integrated would exceed the cap of %d votes per cell", what, n_ids,
             o.n_integrated, OCC_MAX_IDS);
    lslam::set_error(b);
    return LSLAM_ERR_INVALID;
  }
  if (!n_ids) return LSLAM_OK;

  // the jobs, and every allocation, before anything is enqueued
  LSLAM_TRY(o.h_jobs.reserve((size_t)n_ids));
  LSLAM_TRY(o.d_jobs.reserve((size_t)n_ids));
  LSLAM_TRY(o.d_stats.reserve(OCC_ST_N));
  LSLAM_TRY(o.h_stats.reserve(OCC_ST_N));
  const lslam_occ_params &p = o.params;
  const int ia = p.up_axis == 1 ? 2 : 0, ib = p.up_axis == 1 ? 0 : 1;
  size_t scratch = 0;
  for (int32_t c0 = 0; c0 < n_ids; c0 += OCC_CHUNK) {
    const int32_t c1 = c0 + OCC_CHUNK < n_ids ? c0 + OCC_CHUNK : n_ids;
    size_t at = 0;
    for (int32_t i = c0; i < c1; ++i) {
      const lslam::KeyframeClouds &kc = k->kfs[(size_t)ids[i]];
      const float *T = poses + 16 * (size_t)i;
      OccJob j{};
      for (int t = 0; t < 2; ++t) {
        j.p[t] = kc.p[t];
        j.n[t] = (uint32_t)kc.n[t];  // (the store holds at most 2^30 points per cloud)
      }
      std::memcpy(j.T, T, 12 * sizeof(float));
      if (planes && (!plane_valid || plane_valid[i])) {
        for (int e = 0; e < 4; ++e) j.plane[e] = (float)planes[4 * (size_t)i + e];
      } else {
        j.plane[p.up_axis == 1 ? 1 : 2] = 1.0f;
        j.plane[3] = p.sensor_height;
      }
      const double qa = occ_q((double)T[4 * ia + 3], p.origin[0], o.scale), qb = occ_q((double)T[4 * ib + 3], p.origin[1], o.scale);
      j.a_ok = (qa >= -OCC_FIX_LIMIT && qa < OCC_FIX_LIMIT && qb >= -OCC_FIX_LIMIT && qb < OCC_FIX_LIMIT) ? 1 : 0;
      if (j.a_ok) j.ax = (int32_t)qa, j.ay = (int32_t)qb;
      occ_window(T + 4 * ia, p.origin[0], o.scale, (double)p.max_range, p.width, &j.wi0, &j.ww);
      occ_window(T + 4 * ib, p.origin[1], o.scale, (double)p.max_range, p.height, &j.wj0, &j.wh);
      if (!j.a_ok || !j.ww || !j.wh) j.ww = j.wh = 0;
      j.words = (uint32_t)(((size_t)j.ww * (size_t)j.wh + 31) / 32);
      j.plane_at = at;
      at += 2 * (size_t)j.words;
      o.h_jobs.p[i] = j;
    }
    if (at > scratch) scratch = at;
  }
  o.last_ids = 0;
  LSLAM_TRY(o.d_planes.reserve(scratch));
  rc = occ_ensure_grid(k);
  if (rc) return rc;

  LSLAM_TRY(hipMemsetAsync(o.d_stats.p, 0, OCC_ST_N * sizeof(unsigned long long), k->stream));
  LSLAM_TRY(hipMemcpyAsync(o.d_jobs.p, o.h_jobs.p, (size_t)n_ids * sizeof(OccJob), hipMemcpyHostToDevice, k->stream));
  o.n_integrated += n_ids;  // from here on the counts may have changed
  o.values_stale = true;
  for (int32_t c0 = 0; c0 < n_ids; c0 += OCC_CHUNK) {
    rc = occ_launch_chunk(k, c0, c0 + OCC_CHUNK < n_ids ? c0 + OCC_CHUNK : n_ids, o.d_planes.p, o.d_stats.p, true);
    if (rc) return occ_fail(k, rc);
  }
  LSLAM_TRY(hipMemcpyAsync(o.h_stats.p, o.d_stats.p, OCC_ST_N * sizeof(unsigned long long), hipMemcpyDeviceToHost, k->stream));
  LSLAM_TRY(hipStreamSynchronize(k->stream));
  o.rays[1] += (int64_t)o.h_stats.p[OCC_ST_DROPPED];
  o.rays[2] += (int64_t)o.h_stats.p[OCC_ST_OBSTACLE];
  o.rays[3] += (int64_t)o.h_stats.p[OCC_ST_GROUND];
  o.rays[0] = o.rays[2] + o.rays[3];
  o.last_ids = n_ids;
  if (o.h_stats.p[OCC_ST_ESCAPED]) {
    snprintf(b, sizeof(b), "%s: %llu cells fell outside their keyframe's window (a defect: the counts miss them)", what,
             o.h_stats.p[OCC_ST_ESCAPED]);
    lslam::set_error(b);
    return LSLAM_ERR_HIP;
  }
  return LSLAM_OK;
}

int lslam_occ_counts(lslam_kfs *k, uint32_t *out) {
  int rc = occ_entry(k, "lslam_occ_counts");
  if (rc) return rc;
  if (!out) {
    lslam::set_error("lslam_occ_counts: null out");
    return LSLAM_ERR_INVALID;
  }
  rc = occ_ensure_grid(k);
  if (rc) return rc;
  OccState &o = k->occ;
  LSLAM_TRY(hipMemcpyAsync(out, o.d_counts.p, o.cells() * sizeof(uint32_t), hipMemcpyDeviceToHost, k->stream));
  LSLAM_TRY(hipStreamSynchronize(k->stream));
  return LSLAM_OK;
}

int lslam_occ_values(lslam_kfs *k, int8_t *out) {
  int rc = occ_entry(k, "lslam_occ_values");
  if (rc) return rc;
  if (!out) {
    lslam::set_error("lslam_occ_values: null out");
    return LSLAM_ERR_INVALID;
  }
  rc = occ_ensure_grid(k);
  if (rc) return rc;
  rc = occ_fresh_values(k);
  if (rc) return occ_fail(k, rc);
  OccState &o = k->occ;
  LSLAM_TRY(hipMemcpyAsync(out, o.d_values.p, o.cells(), hipMemcpyDeviceToHost, k->stream));
  LSLAM_TRY(hipStreamSynchronize(k->stream));
  return LSLAM_OK;
}

int lslam_occ_view(lslam_kfs *k, const uint32_t **d_counts, const int8_t **d_values) {
  int rc = occ_entry(k, "lslam_occ_view");
  if (rc) return rc;
  rc = occ_ensure_grid(k);
  if (rc) return rc;
  if (d_values) {
    rc = occ_fresh_values(k);
    if (rc) return occ_fail(k, rc);
  }
  LSLAM_TRY(hipStreamSynchronize(k->stream));
  if (d_counts) *d_counts = k->occ.d_counts.p;
  if (d_values) *d_values = k->occ.d_values.p;
  return LSLAM_OK;
}

int lslam_occ_fit_bounds(int32_t n, const float *poses, lslam_occ_params *params) {
  const char *what = "lslam_occ_fit_bounds";
  if (n < 1 || !poses || !params) {
    lslam::set_error("lslam_occ_fit_bounds: n below 1, or null poses / params");
    return LSLAM_ERR_INVALID;
  }
  int rc = occ_check_scale(what, *params);
  if (rc) return rc;
  const int row[2] = {params->up_axis == 1 ? 2 : 0, params->up_axis == 1 ? 0 : 1};
  const double r = (double)params->resolution, m = (double)params->max_range;
  double origin[2];
  int64_t cells[2];
  for (int c = 0; c < 2; ++c) {
    double lo = 0.0, hi = 0.0;
    for (int32_t i = 0; i < n; ++i) {
      const double v = (double)poses[16 * (size_t)i + 4 * row[c] + 3];
      if (!std::isfinite(v)) {
        char b[200];
        snprintf(b, sizeof(b), "%s: the position of pose %d is not finite", what, i);
        lslam::set_error(b);
        return LSLAM_ERR_INVALID;
      }
      if (i == 0 || v - m < lo) lo = v - m;
      if (i == 0 || v + m > hi) hi = v + m;
    }
    double i0 = std::floor(lo / r);
    while (i0 * r > lo) i0 -= 1.0;
    while ((i0 + 1.0) * r <= lo) i0 += 1.0;
    origin[c] = i0 * r;
    double w = std::ceil((hi - origin[c]) / r);
    if (w < 1.0) w = 1.0;
    if (w > 1e9) w = 1e9;  // (refused below; keeps the loops short)
    while (origin[c] + w * r < hi) w += 1.0;
    while (w > 1.0 && origin[c] + (w - 1.0) * r >= hi) w -= 1.0;
    cells[c] = (int64_t)w;
  }
  rc = occ_check_size(what, cells[0], cells[1]);
  if (rc) return rc;
  params->origin[0] = origin[0];
  params->origin[1] = origin[1];
  params->width = (int32_t)cells[0];
  params->height = (int32_t)cells[1];
  return LSLAM_OK;
}

int lslam_debug_occ_integrate(lslam_kfs *k, int32_t launches) {
  int rc = occ_entry(k, "lslam_debug_occ_integrate");
  if (rc) return rc;
  OccState &o = k->occ;
  if (!o.last_ids || launches < 0) {
    lslam::set_error("lslam_debug_occ_integrate: no lslam_occ_integrate call with keyframes has run last, or negative launches");
    return LSLAM_ERR_INVALID;
  }
  LSLAM_TRY(o.d_planes_again.reserve(o.d_planes.cap));
  LSLAM_TRY(o.d_stats_again.reserve(OCC_ST_N));
  LSLAM_TRY(hipMemsetAsync(o.d_stats_again.p, 0, OCC_ST_N * sizeof(unsigned long long), k->stream));
  for (int32_t i = 0; i < launches; ++i)
    for (int32_t c0 = 0; c0 < o.last_ids; c0 += OCC_CHUNK) {
      rc = occ_launch_chunk(k, c0, c0 + OCC_CHUNK < o.last_ids ? c0 + OCC_CHUNK : o.last_ids, o.d_planes_again.p, o.d_stats_again.p, false);
      if (rc) return occ_fail(k, rc);
    }
  return LSLAM_OK;
}

}  // extern "C"
