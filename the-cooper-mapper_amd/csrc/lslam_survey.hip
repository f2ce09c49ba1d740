// lslam_survey.hip -- the survey-cloud feature map extractor on the device: io_module/feature_extracter.cpp:43-130 over
// util/pcl_util.h:39-62,107-182 and util/voxel_grid_partition.hpp:80-330.  A dense survey cloud becomes the corner / surf cube
// map that the localisation node loads (lslam_loc_load, lslam_pmap_open after lslam_index_convert).
//
// PARITY UNPINNED: the reference delegates every stage to PCL (VoxelGrid, NormalEstimation, RegionGrowing,
// BoundaryEstimation), which is neither in the reference tree nor installed.  Restated here -- and independently, in numpy, in
// tests/survey_map_ref.py -- is the pipeline include/lslam_c.h describes; DESIGN "Survey-cloud extractor" lists what is fixed
// by this library where PCL's answer depends on its version or is unspecified.
//
// Shape of the work.  The partition runs on the host (one pass over the cloud, a sort of 64-bit words): the cloud never has to
// fit on the device, a block at a time does.  Everything per block is device work:
//   sv_vkey / sv_voxel / sv_scatter   VoxelGrid with a minimum count (keys -> radix sort -> one lane per voxel head)
//   sg_key_kernel / sg_gather_kernel  points sorted into the cells of a search grid (cell >= search radius, 27-cell probe);
//                                     a cell's range is found by binary search in the sorted keys: no table per cell
//                                     (lslam_pointgrid_dev.hpp, shared with lslam_mapq.hip: same cells, same neighbour sets)
//   sv_normals                        one lane per query: fp64 sums in ascending (cell, index) order, cyclic Jacobi in fp64
//   sv_knn                            one wavefront per query: lane t holds the t-th best of a sorted K-list (K <= 64),
//                                     candidates by rings of cells until the K-th distance is inside the searched rings
//   sv_edges / sv_sweep               the edge test once (a 64-bit mask per point), then in-place atomicMin label sweeps
//                                     until a device flag stays clear (read by the host every SWEEPS_PER_CHECK launches)
//   sv_bcount / sv_bgap               per point: its neighbours' angles into its slice of a scratch array, heap sort, gaps
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "../../include/lslam_c.h"
#include "lslam_internal.hpp"
#include "lslam_jacobi_dev.hpp"
#include "lslam_pointgrid_dev.hpp"

namespace {

using lslam::DevBuf;

constexpr int SV_BLOCK = 256;
constexpr int SWEEPS_PER_CHECK = 4;
using lslam::JACOBI_SWEEPS;
using lslam::sv_rotate;
using lslam::SGrid;
using lslam::sg_cell;
using lslam::sg_key;
using lslam::sg_lower;
using lslam::sg_probe27;

inline dim3 blocks_for(size_t n) { return dim3((unsigned)((n + SV_BLOCK - 1) / SV_BLOCK)); }

// ---- search grid: SGrid, sg_cell / sg_key / sg_lower, sg_probe27 of lslam_pointgrid_dev.hpp (shared with lslam_mapq.hip) -------
// fp32 squared distance as the reference's searches see it: the three products summed left to right, nothing contracted
__device__ __forceinline__ float sv_d2(const float4 &p, const float4 &q) {
  const float dx = __fsub_rn(p.x, q.x), dy = __fsub_rn(p.y, q.y), dz = __fsub_rn(p.z, q.z);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// ---- VoxelGrid with a minimum count ----------------------------------------------------------------------------------------
struct VoxParams {
  float inv_leaf;
  int32_t base[3];
  int32_t div[3];
};
__global__ void sv_vkey_kernel(const float4 *pts, int n, VoxParams v, uint64_t *keys, uint32_t *idx, int32_t *err) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  const float c[3] = {p.x, p.y, p.z};
  int64_t r[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    r[d] = (int64_t)(int32_t)floorf(__fmul_rn(c[d], v.inv_leaf)) - v.base[d];
    if (r[d] < 0 || r[d] >= v.div[d]) {  // (a non-finite point: the bounding box is the cloud's own)
      atomicExch(err, 1);
      r[d] = 0;
    }
  }
  keys[i] = (uint64_t)r[0] + (uint64_t)v.div[0] * ((uint64_t)r[1] + (uint64_t)v.div[1] * (uint64_t)r[2]);
  idx[i] = (uint32_t)i;
}
// one lane per sorted entry; the head of a voxel walks its members (input order: the sort is stable), sums them as PCL does
// (fp32, sequential, from zero) and divides by the count.  keep[i] = 1 where a centroid was written to tmp[i].
__global__ void sv_voxel_kernel(const float4 *pts, const uint64_t *keys, const uint32_t *idx, int n, int min_points, float4 *tmp,
                                uint32_t *keep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  if (i == n) { keep[i] = 0u; return; }
  const uint64_t k = keys[i];
  if (i > 0 && keys[i - 1] == k) { keep[i] = 0u; return; }
  float4 p = pts[idx[i]];
  // from zero: 0 + x is x for every x but -0.0f, which becomes +0.0f as in PCL's sums (and lslam_voxel_grid's)
  float sx = __fadd_rn(0.0f, p.x), sy = __fadd_rn(0.0f, p.y), sz = __fadd_rn(0.0f, p.z), sw = __fadd_rn(0.0f, p.w);
  int j = i + 1;
  for (; j < n && keys[j] == k; ++j) {
    p = pts[idx[j]];
    sx = __fadd_rn(sx, p.x);
    sy = __fadd_rn(sy, p.y);
    sz = __fadd_rn(sz, p.z);
    sw = __fadd_rn(sw, p.w);
  }
  if (j - i < min_points) { keep[i] = 0u; return; }
  const float cnt = (float)(j - i);
  tmp[i] = make_float4(__fdiv_rn(sx, cnt), __fdiv_rn(sy, cnt), __fdiv_rn(sz, cnt), __fdiv_rn(sw, cnt));
  keep[i] = 1u;
}
// out[pos[i]] = in[i] where keep[i] (pos: the exclusive scan of keep)
template <class T>
__global__ void sv_scatter_kernel(const T *in, const uint32_t *keep, const uint32_t *pos, int n, T *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !keep[i]) return;
  out[pos[i]] = in[i];
}

// ---- normals -----------------------------------------------------------------------------------------------------------------
// (the Jacobi rotation sv_rotate: lslam_jacobi_dev.hpp, shared with lslam_mapq.hip)
__global__ __launch_bounds__(SV_BLOCK) void sv_normals_kernel(SGrid g, const float4 *query, int nq, float r2, float4 *out, int32_t *count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  const float4 q = query[i];
  int n = 0;
  double sx = 0, sy = 0, sz = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
  sg_probe27(g, q, [&](const float4 &p) {
    if (!(sv_d2(p, q) < r2)) return;
    const double dx = (double)p.x - (double)q.x, dy = (double)p.y - (double)q.y, dz = (double)p.z - (double)q.z;
    ++n;
    sx += dx; sy += dy; sz += dz;
    sxx += dx * dx; sxy += dx * dy; sxz += dx * dz;
    syy += dy * dy; syz += dy * dz; szz += dz * dz;
  });
  count[i] = n;
  if (n < 3) {
    const float qnan = __uint_as_float(0x7fc00000u);
    out[i] = make_float4(qnan, qnan, qnan, qnan);
    return;
  }
  const double dn = (double)n;
  const double mx = sx / dn, my = sy / dn, mz = sz / dn;
  double a00 = sxx / dn - mx * mx, a01 = sxy / dn - mx * my, a02 = sxz / dn - mx * mz;
  double a11 = syy / dn - my * my, a12 = syz / dn - my * mz, a22 = szz / dn - mz * mz;
  double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};  // eigenvector columns (v0[k] = V[k][0])
  for (int it = 0; it < JACOBI_SWEEPS; ++it) {
    sv_rotate(a00, a11, a01, a02, a12, v0, v1);  // (p, q) = (0, 1), r = 2
    sv_rotate(a00, a22, a02, a01, a12, v0, v2);  // (0, 2), r = 1
    sv_rotate(a11, a22, a12, a01, a02, v1, v2);  // (1, 2), r = 0
  }
  double l0 = a00;
  double nx = v0[0], ny = v0[1], nz = v0[2];
  if (a11 < l0) { l0 = a11; nx = v1[0]; ny = v1[1]; nz = v1[2]; }
  if (a22 < l0) { l0 = a22; nx = v2[0]; ny = v2[1]; nz = v2[2]; }
  const double trace = (a00 + a11) + a22;
  const double curv = trace == 0.0 ? 0.0 : l0 / trace;
  // flipNormalTowardsViewpoint, viewpoint (0, 0, 0): the normal looks back along the point's position
  const double along = (nx * (double)q.x + ny * (double)q.y) + nz * (double)q.z;
  if (along > 0.0) { nx = -nx; ny = -ny; nz = -nz; }
  out[i] = make_float4((float)nx, (float)ny, (float)nz, (float)curv);
}

// ---- K nearest -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool sv_less(float d, int i, float e, int j) { return d < e || (d == e && i < j); }

// one wavefront per query: lane t holds the t-th best (distance, index) seen so far, ascending
__global__ __launch_bounds__(SV_BLOCK) void sv_knn_kernel(SGrid g, const float4 *query, int nq, int K, int32_t *lists) {
  const int lane = threadIdx.x & 63;
  const int qi = blockIdx.x * (SV_BLOCK / 64) + (threadIdx.x >> 6);
  if (qi >= nq) return;  // (wave-uniform)
  const float4 q = query[qi];
  const int cx = sg_cell(g, q.x, 0), cy = sg_cell(g, q.y, 1), cz = sg_cell(g, q.z, 2);
  float bd = INFINITY;
  int bi = INT32_MAX;
  float wd = INFINITY;  // the K-th best
  int wi = INT32_MAX;
  const int last = K - 1;
  auto scan_range = [&](int a, int b) {
    for (int base = a; base < b; base += 64) {
      const int e = base + lane;
      float d = INFINITY;
      int id = INT32_MAX;
      if (e < b) {
        const float4 p = g.pts[e];
        d = sv_d2(p, q);
        id = (int)__float_as_uint(p.w);
      }
      unsigned long long m = __ballot(e < b && sv_less(d, id, wd, wi));
      while (m) {
        const int l = __builtin_ctzll(m);
        m &= m - 1;
        const float cd = __shfl(d, l, 64);
        const int ci = __shfl(id, l, 64);
        if (!sv_less(cd, ci, wd, wi)) continue;
        const int pos = __popcll(__ballot(sv_less(bd, bi, cd, ci)));  // the slots ahead of the candidate: a prefix
        const float ud = __shfl_up(bd, 1, 64);
        const int ui = __shfl_up(bi, 1, 64);
        if (lane > pos) { bd = ud; bi = ui; }
        else if (lane == pos) { bd = cd; bi = ci; }
        wd = __shfl(bd, last, 64);
        wi = __shfl(bi, last, 64);
      }
    }
  };
  const int reach = max(max(max(cx, g.dim[0] - 1 - cx), max(cy, g.dim[1] - 1 - cy)), max(cz, g.dim[2] - 1 - cz));
  for (int R = 0; R <= reach; ++R) {
    for (int dz = -R; dz <= R; ++dz) {
      const int z = cz + dz;
      if (z < 0 || z >= g.dim[2]) continue;
      for (int dy = -R; dy <= R; ++dy) {
        const int y = cy + dy;
        if (y < 0 || y >= g.dim[1]) continue;
        if (max(abs(dz), abs(dy)) == R) {  // a whole row of the shell
          const int x0 = max(cx - R, 0), x1 = min(cx + R, g.dim[0] - 1);
          scan_range(sg_lower(g, sg_key(g, x0, y, z)), sg_lower(g, sg_key(g, x1, y, z) + 1));
        } else {  // its two end cells
          if (cx - R >= 0) scan_range(sg_lower(g, sg_key(g, cx - R, y, z)), sg_lower(g, sg_key(g, cx - R, y, z) + 1));
          if (cx + R < g.dim[0]) scan_range(sg_lower(g, sg_key(g, cx + R, y, z)), sg_lower(g, sg_key(g, cx + R, y, z) + 1));
        }
      }
    }
    // a point not seen yet is more than R cells away along some axis: farther than R * cell.  The margin covers the fp32
    // rounding of its squared distance.
    const double rc = (double)R * g.cell;
    if (wi != INT32_MAX && (double)wd < rc * rc * 0.9999) break;
  }
  if (lane < K) lists[(size_t)qi * K + lane] = bi == INT32_MAX ? -1 : bi;
}

// ---- region growing ----------------------------------------------------------------------------------------------------------
// rank keys: (curvature as an order-preserving word, index), sorted ascending; labels start as ranks
__global__ void sv_rankkey_kernel(const float4 *normals, int n, uint64_t *keys) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float c = normals[i].w;
  if (c == 0.0f) c = 0.0f;  // -0 and +0 are equal curvatures
  keys[i] = ((uint64_t)lslam::ordered_u32(c) << 32) | (uint32_t)i;
}
__global__ void sv_rank_kernel(const uint64_t *sorted, int n, int32_t *label, int32_t *order) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int i = (int)(uint32_t)sorted[r];
  label[i] = r;
  order[r] = i;
}
// bit t of mask[i]: the edge i -> lists[i][t] exists
__global__ void sv_edges_kernel(const float4 *normals, const int32_t *lists, int n, int K, float cos_thr, uint64_t *mask) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 a = normals[i];
  uint64_t m = 0;
  for (int t = 0; t < K; ++t) {
    const int j = lists[(size_t)i * K + t];
    if (j < 0 || j >= n || j == i) continue;
    const float4 b = normals[j];
    const float dot = __fadd_rn(__fadd_rn(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y)), __fmul_rn(a.z, b.z));
    if (fabsf(dot) >= cos_thr) m |= 1ull << t;
  }
  mask[i] = m;
}
// label[j] = min(label[j], label[i]) over the edges, in place: the fixpoint is unique, the order free.  No lane waits for another.
__global__ void sv_sweep_kernel(const int32_t *lists, const uint64_t *mask, int n, int K, int32_t *label, int32_t *changed) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t m = mask[i];
  if (!m) return;
  const int32_t li = __atomic_load_n(label + i, __ATOMIC_RELAXED);
  bool any = false;
  while (m) {
    const int t = __builtin_ctzll(m);
    m &= m - 1;
    const int j = lists[(size_t)i * K + t];
    if (atomicMin(label + j, li) > li) any = true;
  }
  if (any) atomicOr(changed, 1);
}
__global__ void sv_csize_kernel(const int32_t *label, int n, int32_t *size) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  atomicAdd(size + label[i], 1);
}
// planar[i]: i's region is inside [cmin, cmax]; counters[0 / 1]: regions inside / outside; seed[i]: the region's seed point
__global__ void sv_classify_kernel(const int32_t *label, const int32_t *size, const int32_t *order, int n, int cmin, int cmax,
                                   uint32_t *planar, int32_t *seed, unsigned long long *counters) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int l = label[i];
  const int sz = size[l];
  const bool ok = sz >= cmin && sz <= cmax;
  if (planar) planar[i] = ok ? 1u : 0u;
  if (seed) seed[i] = order[l];
  if (counters && order[l] == i) atomicAdd(counters + (ok ? 0 : 1), 1ull);
}

// ---- boundary ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool sv_nonzero_delta(const float4 &p, const float4 &q) { return p.x != q.x || p.y != q.y || p.z != q.z; }
__global__ __launch_bounds__(SV_BLOCK) void sv_bcount_kernel(SGrid g, const float4 *pts, int n, float r2, uint32_t *cnt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  if (i == n) { cnt[i] = 0u; return; }
  const float4 q = pts[i];
  uint32_t c = 0;
  sg_probe27(g, q, [&](const float4 &p) {
    if (sv_d2(p, q) < r2 && sv_nonzero_delta(p, q)) ++c;
  });
  cnt[i] = c;
}
__device__ void sv_heapsort(double *a, int n) {
  auto sift = [&](int root, int end) {
    for (;;) {
      int child = 2 * root + 1;
      if (child >= end) return;
      if (child + 1 < end && a[child] < a[child + 1]) ++child;
      if (!(a[root] < a[child])) return;
      const double t = a[root]; a[root] = a[child]; a[child] = t;
      root = child;
    }
  };
  for (int s = n / 2 - 1; s >= 0; --s) sift(s, n);
  for (int e = n - 1; e > 0; --e) {
    const double t = a[0]; a[0] = a[e]; a[e] = t;
    sift(0, e);
  }
}
__global__ __launch_bounds__(SV_BLOCK) void sv_bgap_kernel(SGrid g, const float4 *pts, const float4 *normals, int n, float r2,
                                                            const uint32_t *off, double *angles, double thr, uint32_t *flag, double *gap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 q = pts[i];
  const float4 nn = normals[i];
  const double nx = nn.x, ny = nn.y, nz = nn.z;
  // Eigen's unitOrthogonal: the branch is taken in fp32 (isMuchSmallerThan with the type's precision 1e-5), the rest in fp64
  double vx, vy, vz;
  if (fabsf(nn.x) > __fmul_rn(fabsf(nn.z), 1e-5f) || fabsf(nn.y) > __fmul_rn(fabsf(nn.z), 1e-5f)) {
    const double inv = 1.0 / sqrt(nx * nx + ny * ny);
    vx = -ny * inv; vy = nx * inv; vz = 0.0;
  } else {
    const double inv = 1.0 / sqrt(ny * ny + nz * nz);
    vx = 0.0; vy = -nz * inv; vz = ny * inv;
  }
  const double ux = ny * vz - nz * vy, uy = nz * vx - nx * vz, uz = nx * vy - ny * vx;
  double *a = angles + off[i];
  const int m = (int)(off[i + 1] - off[i]);
  int w = 0;
  sg_probe27(g, q, [&](const float4 &p) {
    if (!(sv_d2(p, q) < r2) || !sv_nonzero_delta(p, q)) return;
    const double dx = (double)p.x - (double)q.x, dy = (double)p.y - (double)q.y, dz = (double)p.z - (double)q.z;
    if (w < m) a[w] = atan2((vx * dx + vy * dy) + vz * dz, (ux * dx + uy * dy) + uz * dz);
    ++w;
  });
  double best = 0.0;
  if (m > 0) {
    sv_heapsort(a, m);
    for (int k = 0; k + 1 < m; ++k) best = fmax(best, a[k + 1] - a[k]);
    best = fmax(best, (2.0 * M_PI - a[m - 1]) + a[0]);
  }
  if (gap) gap[i] = best;
  flag[i] = (m > 0 && best > thr) ? 1u : 0u;
}

// ---- output ------------------------------------------------------------------------------------------------------------------
struct CubeParams {
  float cube_size;
  int32_t origin[3], dims[3];
};
// (x, y, z) <- (y, z, x), then worldToCube (FeatureMap.h:475-487); keep = inside the cube array
__global__ void sv_cube_kernel(const float4 *in, int n, CubeParams c, float4 *out, int32_t *cube, uint32_t *keep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  if (i == n) { keep[i] = 0u; return; }
  const float4 p = in[i];
  const float4 o = make_float4(p.y, p.z, p.x, 0.f);
  const int gi = (int)(roundf(o.x / c.cube_size) + (float)c.origin[0]);
  const int gj = (int)(roundf(o.y / c.cube_size) + (float)c.origin[1]);
  const int gk = (int)(roundf(o.z / c.cube_size) + (float)c.origin[2]);
  const bool ok = gi >= 0 && gi < c.dims[0] && gj >= 0 && gj < c.dims[1] && gk >= 0 && gk < c.dims[2];
  out[i] = o;
  cube[i] = ok ? gi + gj * c.dims[0] + gk * c.dims[0] * c.dims[1] : -1;
  keep[i] = ok ? 1u : 0u;
}
__global__ void sv_not_nan_kernel(const float4 *normals, int n, uint32_t *keep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  keep[i] = (i < n && normals[i].x == normals[i].x) ? 1u : 0u;
}
__global__ void sv_zero_tail_kernel(uint32_t *keep, int n) { keep[n] = 0u; }

// ---- host side -----------------------------------------------------------------------------------------------------------------
// scratch of one call: freed when the call returns (a handle keeps only its result)
struct Work {
  hipStream_t s = nullptr;
  DevBuf<char> tmp;
  DevBuf<uint64_t> k0, k1;
  DevBuf<uint32_t> i0, i1, keep, pos, box;
  DevBuf<float4> vtmp;
  DevBuf<int32_t> err;
};

int sort_pairs(Work &w, size_t n, int end_bit) {  // k0, i0 -> k1, i1
  LSLAM_TRY(lslam::sort_pairs(w.tmp, w.k0.p, w.k1.p, w.i0.p, w.i1.p, n, end_bit, w.s));
  return LSLAM_OK;
}
// pos = exclusive scan of keep[0 .. n] (n + 1 words, keep[n] = 0) -> *total = pos[n]; waits
int scan_keep(Work &w, size_t n, size_t *total) {
  size_t bytes = 0;
  LSLAM_TRY(w.pos.reserve(n + 1));
  LSLAM_TRY(rocprim::exclusive_scan(nullptr, bytes, w.keep.p, w.pos.p, 0u, n + 1, rocprim::plus<uint32_t>(), w.s));
  LSLAM_TRY(w.tmp.reserve(bytes));
  LSLAM_TRY(rocprim::exclusive_scan((void *)w.tmp.p, bytes, w.keep.p, w.pos.p, 0u, n + 1, rocprim::plus<uint32_t>(), w.s));
  uint32_t t = 0;
  LSLAM_TRY(hipMemcpyAsync(&t, w.pos.p + n, sizeof(t), hipMemcpyDeviceToHost, w.s));
  LSLAM_TRY(hipStreamSynchronize(w.s));
  *total = t;
  return LSLAM_OK;
}

int device_bbox(Work &w, const float4 *pts, size_t n, float mn[3], float mx[3]) {  // (a non-finite point shows in the box)
  LSLAM_TRY(w.box.reserve(6));
  uint32_t got[6] = {};
  LSLAM_TRY(hipMemcpyAsync(w.box.p, got, sizeof(got), hipMemcpyHostToDevice, w.s));
  hipLaunchKernelGGL(lslam::box_kernel<false>, lslam::box_blocks((int)n), dim3(lslam::BOX_BLOCK), 0, w.s, pts, (int)n, w.box.p);
  LSLAM_TRY(hipMemcpyAsync(got, w.box.p, sizeof(got), hipMemcpyDeviceToHost, w.s));
  LSLAM_TRY(hipStreamSynchronize(w.s));
  lslam::box_back(got, mn, mx);
  return LSLAM_OK;
}

// pcl::VoxelGrid with a minimum count of a device cloud (n > 0, finite) into out (reserved here) -> *m points
int voxel_min(Work &w, const float4 *pts, size_t n, float leaf, int min_points, DevBuf<float4> &out, size_t *m) {
  float mn[3], mx[3];
  LSLAM_RC(device_bbox(w, pts, n, mn, mx));
  const float inv = 1.0f / leaf;
  VoxParams v{};
  v.inv_leaf = inv;
  long long vol = 1;
  uint64_t cells = 1;  // (exact wherever the sort runs: the guard below holds the volume under 2^31)
  for (int d = 0; d < 3; ++d) {
    if (!std::isfinite(mn[d]) || !std::isfinite(mx[d])) {
      lslam::set_error("voxel index outside its key range (non-finite point?)");
      return LSLAM_ERR_INVALID;
    }
    v.base[d] = (int32_t)std::floor(mn[d] * inv);
    v.div[d] = (int32_t)std::floor(mx[d] * inv) - v.base[d] + 1;
    cells *= (uint64_t)v.div[d];
    vol *= (long long)((mx[d] - mn[d]) * inv) + 1;
  }
  LSLAM_TRY(out.reserve(n));
  if (!(vol <= (long long)INT32_MAX)) {  // applyFilter: "Leaf size is too small for the input dataset": the input comes back
    LSLAM_TRY(hipMemcpyAsync(out.p, pts, n * sizeof(float4), hipMemcpyDeviceToDevice, w.s));
    LSLAM_TRY(hipStreamSynchronize(w.s));
    *m = n;
    return LSLAM_OK;
  }
  LSLAM_TRY(w.k0.reserve(n)); LSLAM_TRY(w.k1.reserve(n)); LSLAM_TRY(w.i0.reserve(n)); LSLAM_TRY(w.i1.reserve(n));
  LSLAM_TRY(w.keep.reserve(n + 1)); LSLAM_TRY(w.vtmp.reserve(n)); LSLAM_TRY(w.err.reserve(1));
  LSLAM_TRY(hipMemsetAsync(w.err.p, 0, sizeof(int32_t), w.s));
  hipLaunchKernelGGL(sv_vkey_kernel, blocks_for(n), dim3(SV_BLOCK), 0, w.s, pts, (int)n, v, w.k0.p, w.i0.p, w.err.p);
  LSLAM_RC(sort_pairs(w, n, lslam::key_bits(cells)));
  hipLaunchKernelGGL(sv_voxel_kernel, blocks_for(n + 1), dim3(SV_BLOCK), 0, w.s, pts, w.k1.p, w.i1.p, (int)n, min_points, w.vtmp.p, w.keep.p);
  LSLAM_RC(scan_keep(w, n, m));
  int32_t err = 0;
  LSLAM_TRY(hipMemcpy(&err, w.err.p, sizeof(err), hipMemcpyDeviceToHost));
  if (err) {
    lslam::set_error("voxel index outside its key range (non-finite point?)");
    return LSLAM_ERR_INVALID;
  }
  hipLaunchKernelGGL(sv_scatter_kernel<float4>, blocks_for(n), dim3(SV_BLOCK), 0, w.s, w.vtmp.p, w.keep.p, w.pos.p, (int)n, out.p);
  LSLAM_TRY(hipStreamSynchronize(w.s));
  return LSLAM_OK;
}

// a search grid over a device cloud whose bounding box [lo, hi] the caller knows
struct GridBuf {
  DevBuf<uint64_t> keys;
  DevBuf<float4> pts;
  SGrid view{};
};
int build_grid(Work &w, GridBuf &gb, const float4 *pts, size_t n, const float lo[3], const float hi[3], double cell) {
  SGrid g{};
  uint64_t cells;
  int end_bit;
  lslam::sg_shape(lo, hi, cell, &g, &cells, &end_bit);
  g.n = (int)n;
  LSLAM_TRY(w.k0.reserve(n)); LSLAM_TRY(w.k1.reserve(n)); LSLAM_TRY(w.i0.reserve(n)); LSLAM_TRY(w.i1.reserve(n));
  LSLAM_TRY(gb.keys.reserve(n)); LSLAM_TRY(gb.pts.reserve(n));
  hipLaunchKernelGGL(lslam::sg_key_kernel<false>, lslam::sg_blocks(n), dim3(lslam::SG_BLOCK), 0, w.s, pts, (int)n, g, (uint64_t)0, w.k0.p, w.i0.p);
  LSLAM_RC(sort_pairs(w, n, end_bit));
  LSLAM_TRY(hipMemcpyAsync(gb.keys.p, w.k1.p, n * sizeof(uint64_t), hipMemcpyDeviceToDevice, w.s));
  hipLaunchKernelGGL(lslam::sg_gather_kernel<>, lslam::sg_blocks(n), dim3(lslam::SG_BLOCK), 0, w.s, pts, w.i1.p, (int)n, gb.pts.p);
  g.keys = gb.keys.p;
  g.pts = gb.pts.p;
  gb.view = g;
  return LSLAM_OK;
}

inline float radius2(float r) { return (float)((double)r * (double)r); }

int run_normals(Work &w, GridBuf &gb, const float4 *surface, size_t ns, const float lo[3], const float hi[3], const float4 *query,
                size_t nq, float radius, float4 *out, int32_t *count) {
  LSLAM_RC(build_grid(w, gb, surface, ns, lo, hi, (double)radius * lslam::GRID_CELL_PAD));
  hipLaunchKernelGGL(sv_normals_kernel, blocks_for(nq), dim3(SV_BLOCK), 0, w.s, gb.view, query, (int)nq, radius2(radius), out, count);
  return LSLAM_OK;
}

int run_knn(Work &w, GridBuf &gb, const float4 *pts, size_t n, const float lo[3], const float hi[3], int K, double cell, int32_t *lists) {
  LSLAM_RC(build_grid(w, gb, pts, n, lo, hi, cell));
  hipLaunchKernelGGL(sv_knn_kernel, dim3((unsigned)((n + SV_BLOCK / 64 - 1) / (SV_BLOCK / 64))), dim3(SV_BLOCK), 0, w.s, gb.view, pts,
                     (int)n, K, lists);
  return LSLAM_OK;
}

struct RegionBuf {
  DevBuf<int32_t> label, order, size, changed;
  DevBuf<uint64_t> mask;
  DevBuf<unsigned long long> counters;
};
// labels to their fixpoint; then sizes.  planar / seed / counts: optional outputs
int run_region(Work &w, RegionBuf &rb, const float4 *normals, size_t n, const int32_t *lists, int K, float cos_thr, int cmin, int cmax,
               uint32_t *planar, int32_t *seed, int64_t counts[2], int64_t *sweeps) {
  LSLAM_TRY(rb.label.reserve(n)); LSLAM_TRY(rb.order.reserve(n)); LSLAM_TRY(rb.size.reserve(n)); LSLAM_TRY(rb.changed.reserve(1));
  LSLAM_TRY(rb.mask.reserve(n)); LSLAM_TRY(rb.counters.reserve(2));
  LSLAM_TRY(w.k0.reserve(n)); LSLAM_TRY(w.k1.reserve(n));
  hipLaunchKernelGGL(sv_rankkey_kernel, blocks_for(n), dim3(SV_BLOCK), 0, w.s, normals, (int)n, w.k0.p);
  size_t bytes = 0;
  LSLAM_TRY(rocprim::radix_sort_keys(nullptr, bytes, w.k0.p, w.k1.p, n, 0u, 64u, w.s));
  LSLAM_TRY(w.tmp.reserve(bytes));
  LSLAM_TRY(rocprim::radix_sort_keys((void *)w.tmp.p, bytes, w.k0.p, w.k1.p, n, 0u, 64u, w.s));
  hipLaunchKernelGGL(sv_rank_kernel, blocks_for(n), dim3(SV_BLOCK), 0, w.s, w.k1.p, (int)n, rb.label.p, rb.order.p);
  hipLaunchKernelGGL(sv_edges_kernel, blocks_for(n), dim3(SV_BLOCK), 0, w.s, normals, lists, (int)n, K, cos_thr, rb.mask.p);
  int64_t launched = 0;
  for (;;) {
    LSLAM_TRY(hipMemsetAsync(rb.changed.p, 0, sizeof(int32_t), w.s));
    for (int k = 0; k < SWEEPS_PER_CHECK; ++k)
      hipLaunchKernelGGL(sv_sweep_kernel, blocks_for(n), dim3(SV_BLOCK), 0, w.s, lists, rb.mask.p, (int)n, K, rb.label.p, rb.changed.p);
    launched += SWEEPS_PER_CHECK;
    int32_t changed = 0;
    LSLAM_TRY(hipMemcpyAsync(&changed, rb.changed.p, sizeof(changed), hipMemcpyDeviceToHost, w.s));
    LSLAM_TRY(hipStreamSynchronize(w.s));
    if (!changed) break;
    if (launched > (int64_t)n + SWEEPS_PER_CHECK) {  // a label travels at least one edge per launch: cannot happen
      lslam::set_error("region labels did not settle");
      return LSLAM_ERR_INVALID;
    }
  }
  if (sweeps) *sweeps += launched;
  LSLAM_TRY(hipMemsetAsync(rb.size.p, 0, n * sizeof(int32_t), w.s));
  LSLAM_TRY(hipMemsetAsync(rb.counters.p, 0, 2 * sizeof(unsigned long long), w.s));
  hipLaunchKernelGGL(sv_csize_kernel, blocks_for(n), dim3(SV_BLOCK), 0, w.s, rb.label.p, (int)n, rb.size.p);
  hipLaunchKernelGGL(sv_classify_kernel, blocks_for(n), dim3(SV_BLOCK), 0, w.s, rb.label.p, rb.size.p, rb.order.p, (int)n, cmin, cmax,
                     planar, seed, counts ? rb.counters.p : nullptr);
  if (counts) {
    unsigned long long c[2];
    LSLAM_TRY(hipMemcpyAsync(c, rb.counters.p, sizeof(c), hipMemcpyDeviceToHost, w.s));
    LSLAM_TRY(hipStreamSynchronize(w.s));
    counts[0] += (int64_t)c[0];
    counts[1] += (int64_t)c[1];
  }
  return LSLAM_OK;
}

struct BoundaryBuf {
  DevBuf<uint32_t> cnt, off;
  DevBuf<double> angles;
};
int run_boundary(Work &w, GridBuf &gb, BoundaryBuf &bb, const float4 *pts, const float4 *normals, size_t n, const float lo[3],
                 const float hi[3], float radius, double thr, uint32_t *flag, double *gap) {
  LSLAM_RC(build_grid(w, gb, pts, n, lo, hi, (double)radius * lslam::GRID_CELL_PAD));
  LSLAM_TRY(bb.cnt.reserve(n + 1)); LSLAM_TRY(bb.off.reserve(n + 1));
  const float r2 = radius2(radius);
  hipLaunchKernelGGL(sv_bcount_kernel, blocks_for(n + 1), dim3(SV_BLOCK), 0, w.s, gb.view, pts, (int)n, r2, bb.cnt.p);
  size_t bytes = 0;
  LSLAM_TRY(rocprim::exclusive_scan(nullptr, bytes, bb.cnt.p, bb.off.p, 0u, n + 1, rocprim::plus<uint32_t>(), w.s));
  LSLAM_TRY(w.tmp.reserve(bytes));
  LSLAM_TRY(rocprim::exclusive_scan((void *)w.tmp.p, bytes, bb.cnt.p, bb.off.p, 0u, n + 1, rocprim::plus<uint32_t>(), w.s));
  uint32_t total = 0;
  LSLAM_TRY(hipMemcpyAsync(&total, bb.off.p + n, sizeof(total), hipMemcpyDeviceToHost, w.s));
  LSLAM_TRY(hipStreamSynchronize(w.s));
  LSLAM_TRY(bb.angles.reserve((size_t)total + 1));
  hipLaunchKernelGGL(sv_bgap_kernel, blocks_for(n), dim3(SV_BLOCK), 0, w.s, gb.view, pts, normals, (int)n, r2, bb.off.p, bb.angles.p, thr,
                     flag, gap);
  return LSLAM_OK;
}

// host cloud (x y z at the head of every record) -> packed {x, y, z, w}; w from the record when it has one and keep_w
void pack_host(const void *cloud, size_t n, size_t stride, bool keep_w, std::vector<float4> &out) {
  out.resize(n);
  const char *b = (const char *)cloud;
  for (size_t i = 0; i < n; ++i) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    std::memcpy(v, b + i * stride, keep_w && stride >= 16 ? 16 : 12);
    out[i] = make_float4(v[0], v[1], v[2], v[3]);
  }
}
bool host_bbox(const float4 *p, size_t n, float lo[3], float hi[3]) {
  for (int d = 0; d < 3; ++d) { lo[d] = INFINITY; hi[d] = -INFINITY; }
  bool finite = true;
  for (size_t i = 0; i < n; ++i) {
    const float c[3] = {p[i].x, p[i].y, p[i].z};
    for (int d = 0; d < 3; ++d) {
      if (!std::isfinite(c[d])) finite = false;
      lo[d] = std::min(lo[d], c[d]);
      hi[d] = std::max(hi[d], c[d]);
    }
  }
  return finite;
}

int begin_call(lslam_ctx *ctx, Work &w, const char *what) {
  if (!ctx || !lslam::ctx_alive(ctx)) {
    lslam::set_error((std::string(what) + ": no context").c_str());
    return LSLAM_ERR_INVALID;
  }
  LSLAM_TRY(hipSetDevice(lslam::ctx_device(ctx)));
  w.s = lslam::ctx_stream(ctx);
  return LSLAM_OK;
}
int bad(const char *what) {
  lslam::set_error(what);
  return LSLAM_ERR_INVALID;
}
template <class T>
int upload(Work &w, DevBuf<T> &d, const T *h, size_t n) {
  LSLAM_TRY(d.reserve(n ? n : 1));
  if (n) LSLAM_TRY(hipMemcpyAsync(d.p, h, n * sizeof(T), hipMemcpyHostToDevice, w.s));
  return LSLAM_OK;
}

bool params_ok(const lslam_survey_params &p) {
  return p.partition_leaf > 0.f && p.partition_min_points >= 1 && p.filter_leaf > 0.f && p.filter_min_points >= 1 &&
         p.normal_radius > 0.f && p.knn_k >= 1 && p.knn_k <= 64 && p.smoothness_angle >= 0.f && p.curvature_threshold >= 1.0f / 3.0f &&
         p.cluster_min >= 0 && p.cluster_max >= p.cluster_min && p.boundary_radius > 0.f && p.boundary_angle >= 0.0 &&
         p.feature_leaf > 0.f && p.feature_min_points >= 1 && p.cube_size > 0.f && p.cube_dims[0] >= 1 && p.cube_dims[1] >= 1 &&
         p.cube_dims[2] >= 1 && (double)p.cube_dims[0] * p.cube_dims[1] * p.cube_dims[2] < 2147483647.0 && p.knn_cell >= 0.f;
}

}  // namespace

struct lslam_survey {
  int device = 0;
  hipStream_t stream = nullptr;
  lslam_survey_params params{};
  lslam_survey_stats st{};
  DevBuf<float4> pts[2];    // [0] corner (boundary points), [1] surf (planar points): block order, axes permuted
  DevBuf<int32_t> cube[2];  // each point's cube index
  size_t n[2] = {0, 0};
};

namespace {

// one feature cloud of a block: second filter, permutation, cubes; appended to the handle
int append_features(Work &w, lslam_survey *sv, int t, const float4 *cloud, size_t n, DevBuf<float4> &filt, DevBuf<float4> &perm,
                    DevBuf<int32_t> &cube) {
  if (!n) return LSLAM_OK;
  const lslam_survey_params &P = sv->params;
  size_t m = 0;
  LSLAM_RC(voxel_min(w, cloud, n, P.feature_leaf, P.feature_min_points, filt, &m));
  if (!m) return LSLAM_OK;
  CubeParams cp{};
  cp.cube_size = P.cube_size;
  for (int d = 0; d < 3; ++d) { cp.origin[d] = P.cube_origin[d]; cp.dims[d] = P.cube_dims[d]; }
  LSLAM_TRY(perm.reserve(m)); LSLAM_TRY(cube.reserve(m)); LSLAM_TRY(w.keep.reserve(m + 1));
  hipLaunchKernelGGL(sv_cube_kernel, blocks_for(m + 1), dim3(SV_BLOCK), 0, w.s, filt.p, (int)m, cp, perm.p, cube.p, w.keep.p);
  size_t k = 0;
  LSLAM_RC(scan_keep(w, m, &k));
  if (!k) return LSLAM_OK;
  LSLAM_TRY(sv->pts[t].grow(sv->n[t] + k, sv->n[t], w.s));
  LSLAM_TRY(sv->cube[t].grow(sv->n[t] + k, sv->n[t], w.s));
  hipLaunchKernelGGL(sv_scatter_kernel<float4>, blocks_for(m), dim3(SV_BLOCK), 0, w.s, perm.p, w.keep.p, w.pos.p, (int)m, sv->pts[t].p + sv->n[t]);
  hipLaunchKernelGGL(sv_scatter_kernel<int32_t>, blocks_for(m), dim3(SV_BLOCK), 0, w.s, cube.p, w.keep.p, w.pos.p, (int)m, sv->cube[t].p + sv->n[t]);
  LSLAM_TRY(hipStreamSynchronize(w.s));
  sv->n[t] += k;
  return LSLAM_OK;
}

struct BlockBufs {
  DevBuf<float4> block, filt, normals, pts2, normals2, planar_pts, bound_pts, feat, perm;
  DevBuf<int32_t> count, lists, cube;
  DevBuf<uint32_t> planar, bound;
  GridBuf grid;
  RegionBuf region;
  BoundaryBuf boundary;
};

int process_block(Work &w, BlockBufs &b, lslam_survey *sv, const float4 *h_block, size_t n) {
  const lslam_survey_params &P = sv->params;
  lslam_survey_stats &st = sv->st;
  float lo[3], hi[3];
  host_bbox(h_block, n, lo, hi);
  LSLAM_RC(upload(w, b.block, h_block, n));
  // voxelFilter(block, 0.05, 3)
  size_t nf = 0;
  LSLAM_RC(voxel_min(w, b.block.p, n, P.filter_leaf, P.filter_min_points, b.filt, &nf));
  st.filtered_points += (int64_t)nf;
  if (!nf) return LSLAM_OK;
  // normalEstimate(filtered, radius, surface = block)
  LSLAM_TRY(b.normals.reserve(nf)); LSLAM_TRY(b.count.reserve(nf));
  LSLAM_RC(run_normals(w, b.grid, b.block.p, n, lo, hi, b.filt.p, nf, P.normal_radius, b.normals.p, b.count.p));
  // points with an undefined normal leave here
  LSLAM_TRY(w.keep.reserve(nf + 1));
  hipLaunchKernelGGL(sv_not_nan_kernel, blocks_for(nf + 1), dim3(SV_BLOCK), 0, w.s, b.normals.p, (int)nf, w.keep.p);
  size_t m = 0;
  LSLAM_RC(scan_keep(w, nf, &m));
  st.undefined_normals += (int64_t)(nf - m);
  if (!m) return LSLAM_OK;
  LSLAM_TRY(b.pts2.reserve(m)); LSLAM_TRY(b.normals2.reserve(m));
  hipLaunchKernelGGL(sv_scatter_kernel<float4>, blocks_for(nf), dim3(SV_BLOCK), 0, w.s, b.filt.p, w.keep.p, w.pos.p, (int)nf, b.pts2.p);
  hipLaunchKernelGGL(sv_scatter_kernel<float4>, blocks_for(nf), dim3(SV_BLOCK), 0, w.s, b.normals.p, w.keep.p, w.pos.p, (int)nf, b.normals2.p);
  // plannarEstimate: K-nearest lists, labels, region sizes
  const int K = P.knn_k;
  LSLAM_TRY(b.lists.reserve(m * (size_t)K)); LSLAM_TRY(b.planar.reserve(m + 1)); LSLAM_TRY(b.bound.reserve(m + 1));
  // (a centroid may round an ulp outside the block's box: the grid clamps)
  LSLAM_RC(run_knn(w, b.grid, b.pts2.p, m, lo, hi, K, P.knn_cell > 0.f ? (double)P.knn_cell : 4.0 * (double)P.filter_leaf, b.lists.p));
  const float cos_thr = (float)std::cos((double)P.smoothness_angle);
  int64_t counts[2] = {0, 0};
  LSLAM_RC(run_region(w, b.region, b.normals2.p, m, b.lists.p, K, cos_thr, P.cluster_min, P.cluster_max, b.planar.p, nullptr, counts,
                   &st.label_sweeps));
  st.clusters_kept += counts[0];
  st.clusters_dropped += counts[1];
  // boundaryEstimate
  LSLAM_RC(run_boundary(w, b.grid, b.boundary, b.pts2.p, b.normals2.p, m, lo, hi, P.boundary_radius, P.boundary_angle, b.bound.p, nullptr));
  // the two feature clouds, in ascending filtered index
  for (int t = 0; t < 2; ++t) {
    uint32_t *flag = t == 0 ? b.bound.p : b.planar.p;
    DevBuf<float4> &sel = t == 0 ? b.bound_pts : b.planar_pts;
    LSLAM_TRY(w.keep.reserve(m + 1));
    LSLAM_TRY(hipMemcpyAsync(w.keep.p, flag, m * sizeof(uint32_t), hipMemcpyDeviceToDevice, w.s));
    hipLaunchKernelGGL(sv_zero_tail_kernel, dim3(1), dim3(1), 0, w.s, w.keep.p, (int)m);
    size_t k = 0;
    LSLAM_RC(scan_keep(w, m, &k));
    (t == 0 ? st.boundary_points : st.planar_points) += (int64_t)k;
    if (!k) continue;
    LSLAM_TRY(sel.reserve(k));
    hipLaunchKernelGGL(sv_scatter_kernel<float4>, blocks_for(m), dim3(SV_BLOCK), 0, w.s, b.pts2.p, w.keep.p, w.pos.p, (int)m, sel.p);
    LSLAM_RC(append_features(w, sv, t, sel.p, k, b.feat, b.perm, b.cube));
  }
  return LSLAM_OK;
}

int extract_impl(lslam_ctx *ctx, const void *cloud, size_t n, size_t stride, lslam_survey *sv) {
  Work w;
  LSLAM_RC(begin_call(ctx, w, "lslam_survey_extract"));
  sv->device = lslam::ctx_device(ctx);
  sv->stream = w.s;
  const lslam_survey_params &P = sv->params;
  lslam_survey_stats &st = sv->st;
  // voxelPartition(cloud, leaf, min): VoxelGridPartition::applyPartition in fp32 as written
  std::vector<float4> pts;
  pts.reserve(n);
  const char *base = (const char *)cloud;
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (size_t i = 0; i < n; ++i) {
    float v[3];
    std::memcpy(v, base + i * stride, 12);
    if (!std::isfinite(v[0]) || !std::isfinite(v[1]) || !std::isfinite(v[2])) { ++st.points_nonfinite; continue; }
    for (int d = 0; d < 3; ++d) { mn[d] = std::min(mn[d], v[d]); mx[d] = std::max(mx[d], v[d]); }
    pts.push_back(make_float4(v[0], v[1], v[2], 0.f));
  }
  st.points_in = (int64_t)pts.size();
  if (pts.empty()) return LSLAM_OK;
  const float inv = 1.0f / P.partition_leaf;
  int64_t guard = 1;
  int32_t min_b[3], div_b[3];
  for (int d = 0; d < 3; ++d) {
    guard *= (int64_t)((mx[d] - mn[d]) * inv) + 1;
    min_b[d] = (int32_t)std::floor(mn[d] * inv);
    div_b[d] = (int32_t)std::floor(mx[d] * inv) - min_b[d] + 1;
  }
  if (guard > (int64_t)INT32_MAX) return LSLAM_OK;  // "Leaf size is too small for the input dataset": no blocks
  std::vector<uint64_t> order(pts.size());
  if (pts.size() >= ((size_t)1 << 32)) return bad("lslam_survey_extract: more than 2^32 points");
  for (size_t i = 0; i < pts.size(); ++i) {
    const float c[3] = {pts[i].x, pts[i].y, pts[i].z};
    int64_t ijk[3];
    for (int d = 0; d < 3; ++d) ijk[d] = (int64_t)(int32_t)(std::floor(c[d] * inv) - (float)min_b[d]);
    const int64_t idx = ijk[0] + ijk[1] * (int64_t)div_b[0] + ijk[2] * (int64_t)div_b[0] * (int64_t)div_b[1];
    order[i] = ((uint64_t)(uint32_t)idx << 32) | (uint64_t)i;  // (the guard keeps the index inside 31 bits)
  }
  std::sort(order.begin(), order.end());  // ascending cell, input order inside a cell
  BlockBufs bufs;
  std::vector<float4> block;
  for (size_t a = 0; a < order.size();) {
    size_t e = a + 1;
    while (e < order.size() && (order[e] >> 32) == (order[a] >> 32)) ++e;
    if (e - a < (size_t)P.partition_min_points) {
      ++st.blocks_dropped;
    } else {
      ++st.blocks_kept;
      st.max_block_points = std::max<int64_t>(st.max_block_points, (int64_t)(e - a));
      block.resize(e - a);
      for (size_t k = a; k < e; ++k) block[k - a] = pts[(size_t)(uint32_t)order[k]];
      LSLAM_RC(process_block(w, bufs, sv, block.data(), block.size()));
    }
    a = e;
  }
  LSLAM_TRY(hipStreamSynchronize(w.s));
  st.n_corner = (int64_t)sv->n[0];
  st.n_surf = (int64_t)sv->n[1];
  return LSLAM_OK;
}

}  // namespace

extern "C" {

void lslam_survey_default_params(lslam_survey_params *p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->boundary_angle = 3.14159 / 2.0 * 0.9;  // pcl_util.h:133
  p->partition_leaf = 50.0f;                // feature_extracter.cpp:56
  p->partition_min_points = 1000;
  p->filter_leaf = 0.05f;                   // :68
  p->filter_min_points = 3;
  p->normal_radius = 0.05f;                 // :88
  p->knn_k = 60;                            // pcl_util.h:163
  p->smoothness_angle = (float)(3.0 / 180.0 * M_PI);  // :167
  p->curvature_threshold = 1.0f;            // :168
  p->cluster_min = 50;                      // :160-161
  p->cluster_max = 1000000;
  p->boundary_radius = 0.1f;                // :138
  p->feature_leaf = 0.2f;                   // feature_extracter.cpp:110-111
  p->feature_min_points = 3;
  p->cube_size = 50.0f;                     // :50-52
  p->cube_dims[0] = p->cube_dims[1] = p->cube_dims[2] = 21;
  p->cube_origin[0] = 10; p->cube_origin[1] = 5; p->cube_origin[2] = 10;
}

int lslam_survey_extract(lslam_ctx *ctx, const void *cloud, size_t n, size_t stride_bytes, const lslam_survey_params *params,
                         lslam_survey **out) {
  if (out) *out = nullptr;
  if (!ctx || !out || stride_bytes < 12 || (stride_bytes & 3) || (n && !cloud)) return bad("bad lslam_survey_extract arguments");
  lslam_survey_params p;
  if (params) p = *params; else lslam_survey_default_params(&p);
  if (!params_ok(p)) return bad("lslam_survey_extract: a parameter is outside its range (knn_k 1..64, curvature_threshold >= 1/3, sizes > 0)");
  lslam_survey *sv = new lslam_survey();
  sv->params = p;
  const int rc = extract_impl(ctx, cloud, n, stride_bytes, sv);
  if (rc != LSLAM_OK) {
    if (lslam::ctx_alive(ctx)) (void)hipStreamSynchronize(lslam::ctx_stream(ctx));  // nothing of the call is in flight when its scratch goes
    delete sv;
    return rc;
  }
  *out = sv;
  return LSLAM_OK;
}

int lslam_survey_extract_file(lslam_ctx *ctx, const char *pcd_path, const lslam_survey_params *params, lslam_survey **out) {
  if (out) *out = nullptr;
  if (!ctx || !pcd_path || !out) return bad("bad lslam_survey_extract_file arguments");
  std::vector<float4> pts;
  std::string err;
  if (!lslam::fmap_read_pcd(pcd_path, pts, err)) return bad(err.c_str());
  return lslam_survey_extract(ctx, pts.data(), pts.size(), sizeof(float4), params, out);
}

int lslam_survey_info(lslam_survey *sv, lslam_survey_stats *out) {
  if (!sv || !out) return bad("bad lslam_survey_info arguments");
  *out = sv->st;
  return LSLAM_OK;
}

int lslam_survey_get(lslam_survey *sv, float *corner_xyzi, size_t cap_corner, float *surf_xyzi, size_t cap_surf) {
  if (!sv) return bad("bad lslam_survey_get arguments");
  float *dst[2] = {corner_xyzi, surf_xyzi};
  const size_t cap[2] = {cap_corner, cap_surf};
  LSLAM_TRY(hipSetDevice(sv->device));
  for (int t = 0; t < 2; ++t) {
    if (!dst[t] || !sv->n[t]) continue;
    if (cap[t] < sv->n[t]) return bad("lslam_survey_get: output buffer too small");
    LSLAM_TRY(hipMemcpy(dst[t], sv->pts[t].p, sv->n[t] * sizeof(float4), hipMemcpyDeviceToHost));
  }
  return LSLAM_OK;
}

int lslam_survey_save(lslam_survey *sv, const char *directory) {
  if (!sv || !directory) return bad("bad lslam_survey_save arguments");
  LSLAM_TRY(hipSetDevice(sv->device));
  const lslam_survey_params &P = sv->params;
  const int W = P.cube_dims[0], H = P.cube_dims[1], D = P.cube_dims[2];
  const size_t ncube = (size_t)W * H * D;
  std::vector<float4> grouped[2];
  std::vector<size_t> begin[2];
  for (int t = 0; t < 2; ++t) {
    std::vector<float4> h(sv->n[t]);
    std::vector<int32_t> c(sv->n[t]);
    if (sv->n[t]) {
      LSLAM_TRY(hipMemcpy(h.data(), sv->pts[t].p, sv->n[t] * sizeof(float4), hipMemcpyDeviceToHost));
      LSLAM_TRY(hipMemcpy(c.data(), sv->cube[t].p, sv->n[t] * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    begin[t].assign(ncube + 1, 0);  // a counting sort by cube: block order inside a cube, as pushCornerPoint / pushSurfPoint leave it
    for (size_t i = 0; i < c.size(); ++i) ++begin[t][(size_t)c[i] + 1];
    for (size_t k = 0; k < ncube; ++k) begin[t][k + 1] += begin[t][k];
    std::vector<size_t> at(begin[t].begin(), begin[t].end() - 1);
    grouped[t].resize(h.size());
    for (size_t i = 0; i < c.size(); ++i) grouped[t][at[(size_t)c[i]]++] = h[i];
  }
  const std::string dir(directory);
  std::ofstream fout(dir + "/index.txt");
  if (!fout) return bad("save files error!");
  int count = 0;
  for (int i = 0; i < W; ++i)  // saveCloudToFiles, FeatureMap.h:378-413
    for (int j = 0; j < H; ++j)
      for (int k = 0; k < D; ++k) {
        const size_t c = (size_t)i + (size_t)j * W + (size_t)k * W * H;
        for (int t = 0; t < 2; ++t) {
          const size_t b = begin[t][c], e = begin[t][c + 1];
          if (e <= b) continue;
          if (!lslam::fmap_write_pcd((dir + "/" + std::to_string(count) + ".pcd").c_str(), grouped[t].data() + b, e - b))
            return bad("cannot write a cube file");
          fout << count << " " << t << " " << i << " " << j << " " << k << " " << (e - b) << std::endl;
          ++count;
        }
      }
  return LSLAM_OK;
}

void lslam_survey_destroy(lslam_survey *sv) {
  if (!sv) return;
  (void)hipSetDevice(sv->device);
  delete sv;  // (nothing is in flight: every entry point waits before it returns)
}

int lslam_voxel_grid_min(lslam_ctx *ctx, const void *cloud, size_t n, size_t stride_bytes, float leaf, int32_t min_points,
                         float *out_xyzi, size_t cap, size_t *n_out) {
  if (!ctx || !n_out || !(leaf > 0.f) || min_points < 1 || stride_bytes < 12 || (stride_bytes & 3) || (n && !cloud))
    return bad("bad voxel-grid arguments");
  *n_out = 0;
  if (n == 0) return LSLAM_OK;
  Work w;
  LSLAM_RC(begin_call(ctx, w, "lslam_voxel_grid_min"));
  std::vector<float4> h;
  pack_host(cloud, n, stride_bytes, true, h);
  DevBuf<float4> in, out;
  int rc = upload(w, in, h.data(), n);
  size_t m = 0;
  if (rc == LSLAM_OK) rc = voxel_min(w, in.p, n, leaf, min_points, out, &m);
  if (rc == LSLAM_OK && m > cap) rc = bad("voxel-grid output buffer too small");
  if (rc == LSLAM_OK && out_xyzi && m && hipMemcpy(out_xyzi, out.p, m * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess) {
    lslam::set_error("voxel-grid download failed");
    rc = LSLAM_ERR_HIP;
  }
  (void)hipStreamSynchronize(w.s);
  if (rc == LSLAM_OK) *n_out = m;
  return rc;
}

int lslam_debug_survey_normals(lslam_ctx *ctx, const float *surface_xyzw, size_t n_surface, const float *query_xyzw, size_t n_query,
                               float radius, float *out_normal, int32_t *out_count) {
  if (!ctx || !surface_xyzw || !n_surface || !query_xyzw || !n_query || !(radius > 0.f) || !out_normal || !out_count)
    return bad("bad lslam_debug_survey_normals arguments");
  Work w;
  LSLAM_RC(begin_call(ctx, w, "lslam_debug_survey_normals"));
  float lo[3], hi[3];
  if (!host_bbox((const float4 *)surface_xyzw, n_surface, lo, hi)) return bad("lslam_debug_survey_normals: non-finite surface point");
  DevBuf<float4> surf, query, normals;
  DevBuf<int32_t> count;
  GridBuf gb;
  int rc = upload(w, surf, (const float4 *)surface_xyzw, n_surface);
  if (rc == LSLAM_OK) rc = upload(w, query, (const float4 *)query_xyzw, n_query);
  if (rc == LSLAM_OK && (normals.reserve(n_query) != hipSuccess || count.reserve(n_query) != hipSuccess)) rc = LSLAM_ERR_HIP;
  if (rc == LSLAM_OK) rc = run_normals(w, gb, surf.p, n_surface, lo, hi, query.p, n_query, radius, normals.p, count.p);
  if (rc == LSLAM_OK && (hipMemcpyAsync(out_normal, normals.p, n_query * sizeof(float4), hipMemcpyDeviceToHost, w.s) != hipSuccess ||
                         hipMemcpyAsync(out_count, count.p, n_query * sizeof(int32_t), hipMemcpyDeviceToHost, w.s) != hipSuccess))
    rc = LSLAM_ERR_HIP;
  if (hipStreamSynchronize(w.s) != hipSuccess && rc == LSLAM_OK) rc = LSLAM_ERR_HIP;
  if (rc == LSLAM_ERR_HIP) lslam::set_error("HIP error in lslam_debug_survey_normals");
  return rc;
}

int lslam_debug_survey_knn(lslam_ctx *ctx, const float *pts_xyzw, size_t n, int32_t k, float cell, int32_t *out_lists) {
  if (!ctx || !pts_xyzw || !n || k < 1 || k > 64 || !out_lists) return bad("bad lslam_debug_survey_knn arguments (k: 1 .. 64)");
  Work w;
  LSLAM_RC(begin_call(ctx, w, "lslam_debug_survey_knn"));
  float lo[3], hi[3];
  if (!host_bbox((const float4 *)pts_xyzw, n, lo, hi)) return bad("lslam_debug_survey_knn: non-finite point");
  double c = (double)cell;
  if (!(c > 0.0)) {
    double ext = 0.0;
    for (int d = 0; d < 3; ++d) ext = std::max(ext, (double)hi[d] - (double)lo[d]);
    c = std::max(ext / 32.0, 1e-6);
  }
  DevBuf<float4> pts;
  DevBuf<int32_t> lists;
  GridBuf gb;
  int rc = upload(w, pts, (const float4 *)pts_xyzw, n);
  if (rc == LSLAM_OK && lists.reserve(n * (size_t)k) != hipSuccess) rc = LSLAM_ERR_HIP;
  if (rc == LSLAM_OK) rc = run_knn(w, gb, pts.p, n, lo, hi, k, c, lists.p);
  if (rc == LSLAM_OK && hipMemcpyAsync(out_lists, lists.p, n * (size_t)k * sizeof(int32_t), hipMemcpyDeviceToHost, w.s) != hipSuccess)
    rc = LSLAM_ERR_HIP;
  if (hipStreamSynchronize(w.s) != hipSuccess && rc == LSLAM_OK) rc = LSLAM_ERR_HIP;
  if (rc == LSLAM_ERR_HIP) lslam::set_error("HIP error in lslam_debug_survey_knn");
  return rc;
}

int lslam_debug_survey_region(lslam_ctx *ctx, const float *normals_curv, size_t n, const int32_t *lists, int32_t k, float cos_threshold,
                              int32_t *out_labels, int32_t *sweeps_out) {
  if (!ctx || !normals_curv || !n || !lists || k < 1 || k > 64 || !out_labels) return bad("bad lslam_debug_survey_region arguments (k: 1 .. 64)");
  for (size_t i = 0; i < n * (size_t)k; ++i)
    if (lists[i] < -1 || lists[i] >= (int64_t)n) return bad("lslam_debug_survey_region: a list entry is outside the cloud");
  Work w;
  LSLAM_RC(begin_call(ctx, w, "lslam_debug_survey_region"));
  DevBuf<float4> normals;
  DevBuf<int32_t> dl, seed;
  RegionBuf rb;
  int64_t sweeps = 0;
  int rc = upload(w, normals, (const float4 *)normals_curv, n);
  if (rc == LSLAM_OK) rc = upload(w, dl, lists, n * (size_t)k);
  if (rc == LSLAM_OK && seed.reserve(n) != hipSuccess) rc = LSLAM_ERR_HIP;
  if (rc == LSLAM_OK) rc = run_region(w, rb, normals.p, n, dl.p, k, cos_threshold, 0, INT32_MAX, nullptr, seed.p, nullptr, &sweeps);
  if (rc == LSLAM_OK && hipMemcpyAsync(out_labels, seed.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, w.s) != hipSuccess) rc = LSLAM_ERR_HIP;
  if (hipStreamSynchronize(w.s) != hipSuccess && rc == LSLAM_OK) rc = LSLAM_ERR_HIP;
  if (rc == LSLAM_ERR_HIP) lslam::set_error("HIP error in lslam_debug_survey_region");
  if (sweeps_out) *sweeps_out = (int32_t)sweeps;
  return rc;
}

int lslam_debug_survey_boundary(lslam_ctx *ctx, const float *pts_xyzw, const float *normals_xyzw, size_t n, float radius,
                                double angle_threshold, uint8_t *out_flags, double *out_gaps) {
  if (!ctx || !pts_xyzw || !normals_xyzw || !n || !(radius > 0.f) || !out_flags || !out_gaps)
    return bad("bad lslam_debug_survey_boundary arguments");
  Work w;
  LSLAM_RC(begin_call(ctx, w, "lslam_debug_survey_boundary"));
  float lo[3], hi[3];
  if (!host_bbox((const float4 *)pts_xyzw, n, lo, hi)) return bad("lslam_debug_survey_boundary: non-finite point");
  DevBuf<float4> pts, normals;
  DevBuf<uint32_t> flag;
  DevBuf<double> gap;
  GridBuf gb;
  BoundaryBuf bb;
  std::vector<uint32_t> hf(n);
  int rc = upload(w, pts, (const float4 *)pts_xyzw, n);
  if (rc == LSLAM_OK) rc = upload(w, normals, (const float4 *)normals_xyzw, n);
  if (rc == LSLAM_OK && (flag.reserve(n) != hipSuccess || gap.reserve(n) != hipSuccess)) rc = LSLAM_ERR_HIP;
  if (rc == LSLAM_OK) rc = run_boundary(w, gb, bb, pts.p, normals.p, n, lo, hi, radius, angle_threshold, flag.p, gap.p);
  if (rc == LSLAM_OK && (hipMemcpyAsync(hf.data(), flag.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, w.s) != hipSuccess ||
                         hipMemcpyAsync(out_gaps, gap.p, n * sizeof(double), hipMemcpyDeviceToHost, w.s) != hipSuccess))
    rc = LSLAM_ERR_HIP;
  if (hipStreamSynchronize(w.s) != hipSuccess && rc == LSLAM_OK) rc = LSLAM_ERR_HIP;
  if (rc == LSLAM_ERR_HIP) lslam::set_error("HIP error in lslam_debug_survey_boundary");
  if (rc == LSLAM_OK)
    for (size_t i = 0; i < n; ++i) out_flags[i] = (uint8_t)hf[i];
  return rc;
}

}  // extern "C"
