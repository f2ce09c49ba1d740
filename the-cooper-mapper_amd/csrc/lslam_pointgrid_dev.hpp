// lslam_pointgrid_dev.hpp -- the two building blocks every consumer of a device cloud needs, each defined once:
//   the bounding box   the order-preserving float <-> uint32 map, one workgroup reduction (box_add / box_reduce) and one kernel
//                      (box_kernel) -- lslam_grid.hip (grid_bbox2), lslam_lmap.hip (lm_transform_kernel, lm_index_box_kernel),
//                      lslam_fmap.hip (fm_gather_box_kernel), lslam_survey.hip (device_bbox), lslam_mapq.hip (both clouds)
//   the sorted grid    points sorted by the key of their cell, a cell's range found by binary search in the sorted keys (memory by
//                      the points, never by the box): SGrid, sg_cell / sg_key / sg_lower, sg_probe27, sg_key_kernel,
//                      sg_gather_kernel, sg_shape, sort_pairs -- lslam_survey.hip (normals, K nearest, boundary) and
//                      lslam_mapq.hip (mq_probe_kernel)
// Header-only: the build has no relocatable device code, so every file that includes this instantiates the kernels it launches.
// As with lslam_jacobi_dev.hpp the point is bit equality by construction: the survey extractor and map quality see the same
// cells, the same neighbour order and so the same neighbour sets for the same radius, and a box is the same words whichever
// file reduced it, because there is one definition to compile.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include <rocprim/device/device_radix_sort.hpp>

#include "lslam_buf.hpp"

namespace lslam {

// ---- ordered floats ----------------------------------------------------------------------------------------------------------
// Monotone map float -> uint32 (for atomicMin / atomicMax on floats) and its inverse.  -0 sorts below +0; a NaN sorts beyond
// the infinity of its sign, so a non-finite coordinate shows in a box that was reduced through this map.
__device__ __forceinline__ uint32_t ordered_u32(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float ordered_back(uint32_t o) {
  return __builtin_bit_cast(float, (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

__device__ __forceinline__ bool finite3(const float4 &p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

// ---- bounding box --------------------------------------------------------------------------------------------------------------
// A box is six words that start at zero and only grow: [0..2] the maxima of ~ordered (the minima), [3..5] the maxima of ordered.
// Zero decodes to NaN on both sides: the box of no point.
constexpr int BOX_BLOCK = 256;

__device__ __forceinline__ void box_add(uint32_t mm[6], const float4 &p) {
  const uint32_t o[3] = {ordered_u32(p.x), ordered_u32(p.y), ordered_u32(p.z)};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    mm[a] = max(mm[a], ~o[a]);
    mm[3 + a] = max(mm[3 + a], o[a]);
  }
}
// mm over the workgroup -> six atomics into box[0..5].  Called by every thread of a BOX_BLOCK-thread workgroup; a workgroup
// none of whose threads has a point (`any`) leaves early.  Wavefront butterfly in registers, then the four wavefronts through
// LDS: same-address atomics from a whole grid serialise at the memory side, six per workgroup do not show.
__device__ __forceinline__ void box_reduce(uint32_t mm[6], bool any, uint32_t *box) {
  if (!__syncthreads_or(any)) return;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1)
#pragma unroll
    for (int a = 0; a < 6; ++a) mm[a] = max(mm[a], (uint32_t)__shfl_xor((int)mm[a], d, 64));
  __shared__ uint32_t part[4][6];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 6; ++a) part[wave][a] = mm[a];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int a = threadIdx.x;
    atomicMax(&box[a], max(max(part[0][a], part[1][a]), max(part[2][a], part[3][a])));
  }
}
inline void box_back(const uint32_t box[6], float lo[3], float hi[3]) {
  for (int a = 0; a < 3; ++a) {
    lo[a] = ordered_back(~box[a]);
    hi[a] = ordered_back(box[3 + a]);
  }
}

// The box of a device cloud, grid-stride over box_blocks(n) workgroups, into a zeroed box.  FINITE_ONLY: a point with a
// non-finite coordinate is skipped and box[6] counts the others; without it such a point shows in the box (see ordered_u32).
template <bool FINITE_ONLY>
__global__ __launch_bounds__(BOX_BLOCK) void box_kernel(const float4 *pts, int n, uint32_t *box) {
  uint32_t mm[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  uint32_t count = 0;
  for (int i = blockIdx.x * BOX_BLOCK + threadIdx.x; i < n; i += gridDim.x * BOX_BLOCK) {
    const float4 p = pts[i];
    if (FINITE_ONLY && !finite3(p)) continue;
    box_add(mm, p);
    ++count;
  }
  if (FINITE_ONLY) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) count += (uint32_t)__shfl_xor((int)count, d, 64);
    if ((threadIdx.x & 63) == 0 && count) atomicAdd(box + 6, count);
  }
  box_reduce(mm, count != 0, box);
}
inline dim3 box_blocks(int n) { return dim3((unsigned)std::min((n + 4095) / 4096, 256)); }

// ---- sorted search grid ----------------------------------------------------------------------------------------------------
// Cell coordinate of x along axis d: floor(((double)x - lo) / cell), clamped into the grid.  In fp64 the map is monotone and
// two coordinates closer than `cell` land in the same or in adjacent cells; clamping (a monotone map too) keeps that, also for
// a query that lies outside the grid's box.  A radius search uses cell = r * GRID_CELL_PAD: the fp32 distance test
// dx*dx + dy*dy + dz*dz < r2 can pass for a |dx| that exceeds r by a few ulp, never by a thousandth.
constexpr double GRID_CELL_PAD = 1.0 + 1.0 / 1024.0;
constexpr int SG_BLOCK = 256;

struct SGrid {  // (a kernel argument: the geometry first, as mq_probe_kernel has always been handed it -- DESIGN 8j)
  double lo[3];
  double cell;
  int dim[3];
  const uint64_t *keys;  // [n] ascending: x + DX * (y + DY * z)
  const float4 *pts;     // [n] in key order, w = bitcast(original index); equal keys in ascending index
  int n;
};

__device__ __forceinline__ int sg_cell(const SGrid &g, float x, int d) {
  const double t = floor(((double)x - g.lo[d]) / g.cell);
  if (!(t > 0.0)) return 0;
  if (t >= (double)g.dim[d]) return g.dim[d] - 1;
  return (int)t;
}
__device__ __forceinline__ uint64_t sg_key(const SGrid &g, int x, int y, int z) {
  return (uint64_t)x + (uint64_t)g.dim[0] * ((uint64_t)y + (uint64_t)g.dim[1] * (uint64_t)z);
}
__device__ __forceinline__ int sg_lower(const SGrid &g, uint64_t key) {  // first position with keys[pos] >= key
  int lo = 0, hi = g.n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (g.keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// every point of the grid within the 27 cells around q, in ascending (key, index) order: f(point)
template <class F>
__device__ __forceinline__ void sg_probe27(const SGrid &g, const float4 &q, F f) {
  const int cx = sg_cell(g, q.x, 0), cy = sg_cell(g, q.y, 1), cz = sg_cell(g, q.z, 2);
  const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dim[0] - 1);
  for (int z = max(cz - 1, 0); z <= min(cz + 1, g.dim[2] - 1); ++z)
    for (int y = max(cy - 1, 0); y <= min(cy + 1, g.dim[1] - 1); ++y) {
      const int a = sg_lower(g, sg_key(g, x0, y, z)), b = sg_lower(g, sg_key(g, x1, y, z) + 1);
      for (int e = a; e < b; ++e) f(g.pts[e]);
    }
}

// key of every point's cell and its position (g.keys / g.pts / g.n are not read).  NONFINITE_BEHIND: a non-finite point gets
// `behind`, a key above every cell's, and sorts behind the grid.
template <bool NONFINITE_BEHIND>
__global__ __launch_bounds__(SG_BLOCK) void sg_key_kernel(const float4 *pts, int n, SGrid g, uint64_t behind, uint64_t *keys, uint32_t *idx) {
  const int i = blockIdx.x * SG_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  keys[i] = NONFINITE_BEHIND && !finite3(p) ? behind : sg_key(g, sg_cell(g, p.x, 0), sg_cell(g, p.y, 1), sg_cell(g, p.z, 2));
  idx[i] = (uint32_t)i;
}
// the points in sorted order, w = bitcast(original index).  (A template only so that the kernel is emitted in the files that
// launch it, not in every file that includes this header: launch sg_gather_kernel<>.)
template <int = 0>
__global__ __launch_bounds__(SG_BLOCK) void sg_gather_kernel(const float4 *pts, const uint32_t *idx, int n, float4 *out) {
  const int i = blockIdx.x * SG_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t j = idx[i];
  const float4 p = pts[j];
  out[i] = make_float4(p.x, p.y, p.z, __uint_as_float(j));
}
// the launch shape of the two kernels above: sg_blocks(n) workgroups of SG_BLOCK
inline dim3 sg_blocks(size_t n) { return dim3((unsigned)((n + SG_BLOCK - 1) / SG_BLOCK)); }

// the key bits a radix sort has to look at for keys up to and including max_key
inline int key_bits(uint64_t max_key) {
  int b = 1;
  while (b < 64 && (max_key >> b)) ++b;
  return b;
}

// The grid over the box [lo, hi] with cells of `cell` or wider: at most 2^20 cells per axis, so a key stays inside 60 bits.
// Fills g.lo / g.cell / g.dim; *cells: the number of cells, itself a key above every cell's; *end_bit: key_bits(*cells).
inline void sg_shape(const float lo[3], const float hi[3], double cell, SGrid *g, uint64_t *cells, int *end_bit) {
  double ext = 0.0;
  for (int d = 0; d < 3; ++d) ext = std::max(ext, (double)hi[d] - (double)lo[d]);
  cell = std::max(cell, ext / 1048576.0);
  if (!(cell > 0.0)) cell = 1.0;
  g->cell = cell;
  *cells = 1;
  for (int d = 0; d < 3; ++d) {
    g->lo[d] = (double)lo[d];
    g->dim[d] = (int)std::floor(((double)hi[d] - (double)lo[d]) / cell) + 1;
    *cells *= (uint64_t)g->dim[d];
  }
  *end_bit = key_bits(*cells);
}

// (k0, i0) -> (k1, i1) by the low end_bit bits of the key, stable; rocPRIM's scratch in tmp (grown as needed)
inline hipError_t sort_pairs(DevBuf<char> &tmp, uint64_t *k0, uint64_t *k1, uint32_t *i0, uint32_t *i1, size_t n, int end_bit, hipStream_t s) {
  size_t bytes = 0;
  hipError_t e = rocprim::radix_sort_pairs(nullptr, bytes, k0, k1, i0, i1, n, 0u, (unsigned)end_bit, s);
  if (e == hipSuccess) e = tmp.reserve(bytes);
  if (e == hipSuccess) e = rocprim::radix_sort_pairs((void *)tmp.p, bytes, k0, k1, i0, i1, n, 0u, (unsigned)end_bit, s);
  return e;
}

}  // namespace lslam
