// lslam_loc.hip -- the localisation node (odometry/LaserLocalization.cpp over util/FeatureMap.h) resident on the device.
//
// A prebuilt map is loaded once: every cube with at least five points of a type gets its kd-tree in ONE forest build
// (loadCloudFromFiles builds them at FeatureMap.h:438,453) and keeps it until the map is replaced.  A sweep is then
//   transformMerge (host) -> both clouds voxel-filtered on the device -> FeatureMap::scanMatchScan (:490-691) -> transformUpdate
// behind one host wait.  The node owns its map (an lslam_fmap it never installs in the context), its trees, its cell grids
// and its scratch; the context's resident map is neither read nor written.
//
// The search (include/lslam_c.h has the argument): variant C fixes the RESULT of nearestKSearch in the tree of the query's
// cube.  loc_probe_kernel runs the 27-cell probe of lslam_grid.hpp over a cell grid of the cubes around the sensor; a point
// whose proven five all lie in its own cube is decided there (same five, same order), a point proven beyond the gate is
// rejected there, every other point is listed for loc_tree_kernel, which walks the tree of ITS CUBE.  Both leave the five
// neighbours per point (distances, positions in the cell-sorted array or in the trees' array); loc_fit_kernel then runs the
// residual chain and the block sums over all points in their fixed places, so the sums -- and the poses -- do not depend on
// which search decided a point.  The carried-neighbour certificates are not used here.
#include "../../include/lslam_c.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "lslam_internal.hpp"
#include "lslam_sweep_dev.hpp"

using namespace lslam;

#define LOC_TRY(expr)                                                                    \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) {                                                              \
      char _b[256];                                                                      \
      std::snprintf(_b, sizeof(_b), "HIP error %s at %s:%d", hipGetErrorString(_e), __FILE__, __LINE__); \
      lslam::set_error(_b);                                                              \
      return LSLAM_ERR_HIP;                                                              \
    }                                                                                    \
  } while (0)

namespace {

constexpr int LOC_BLOCK = SWEEP_BLOCK;  // one lane per scan point, as the sweeps of lslam_kernels.hip
constexpr int LOC_TREE_BLOCK = 128;     // the tree walk keeps its whole stack in LDS (32 levels x 2 words x 128 lanes)
constexpr int LOC_MAX_ITER = 10;        // FeatureMap::scanMatchScan's loop
enum : int { ST_SWEPT = 0, ST_PROVEN = 1, ST_REFUSED = 2, ST_TREES = 3, ST_N = 4 };
enum : int { HOW_SKIPPED = 0, HOW_GRID = 1, HOW_TREE = 2 };
static_assert(LOC_BLOCK == 256, "knn5_grid's row table and block_accumulate are sized for 256 lanes");

struct LocArgs {
  const float4 *q[2];       // the scan's corner / surf array (sensor frame)
  const int32_t *counts;    // device [4]: {first corner point, corner points, first surf point, surf points} in q[0] / q[1]
  int32_t nbc, nb_total;    // workgroups [0, nbc) take corner points, [nbc, nb_total) surf points; point slot = workgroup * 256 + lane
  CubeGridDev cg[2];
  CellGrid G[2];            // cell_start null: the type has no grid, every point goes to its cube's tree
  const int2 *range[2];     // per tree: [first, end) of its cube's points in the numbering the grid's points carry in .w; empty: not covered
  const float4 *tpts;       // the trees' point array (every TreeView::pts)
  const GNState *st;
  float *nb_d;              // [slots][5]
  int32_t *nb_p;            // [slots][5] positions in G.pts (HOW_GRID) or tpts (HOW_TREE)
  uint8_t *how;             // [slots]
  int32_t *list;            // slots left to the tree search
  int32_t *list_cnt;
  unsigned long long *stat; // [ST_N]
  float *partials;          // [nb_total][NCOL]
  int32_t tap;              // 1: the parity tap -- no gate, a point beyond it is searched in its tree
};

struct PointRef {
  int t, n, off, i;
  size_t slot;
};
LSLAM_DEV PointRef point_of_block(const LocArgs &a, int b, int tid) {
  PointRef r;
  r.t = b >= a.nbc ? 1 : 0;
  const int lb = b - (r.t ? a.nbc : 0);
  r.off = a.counts[2 * r.t];
  r.n = a.counts[2 * r.t + 1];
  r.i = lb * LOC_BLOCK + tid;
  r.slot = (size_t)b * LOC_BLOCK + tid;
  return r;
}
LSLAM_DEV void to_map(const GNState *st, const float4 &q, float (&sel)[3]) {
  // util/transform_utils.h:476-482 pointAssociateToMap, the sweep kernels' operation order
  sel[0] = ((st->R[0] * q.x + st->R[1] * q.y) + st->R[2] * q.z) + st->t[0];
  sel[1] = ((st->R[3] * q.x + st->R[4] * q.y) + st->R[5] * q.z) + st->t[1];
  sel[2] = ((st->R[6] * q.x + st->R[7] * q.y) + st->R[8] * q.z) + st->t[2];
}

// Pass 1: the 27-cell probe with its proof, and the cube check.
__global__ __launch_bounds__(LOC_BLOCK) void loc_probe_kernel(const LocArgs a) {
  __shared__ uint32_t rows_lds[18 * LOC_BLOCK];
  if (a.st->done) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const PointRef r = point_of_block(a, blockIdx.x, tid);
  if (r.i - tid >= r.n) return;  // workgroup-uniform: no point of the filtered cloud reaches this workgroup
  const bool on = r.i < r.n;
  const float4 q = on ? a.q[r.t][r.off + r.i] : make_float4(0.f, 0.f, 0.f, 0.f);
  float sel[3];
  to_map(a.st, q, sel);
  const CubeGridDev cg = r.t ? a.cg[1] : a.cg[0];
  const CellGrid G = r.t ? a.G[1] : a.G[0];
  const int2 *range = r.t ? a.range[1] : a.range[0];
  const int tree = on ? cube_tree_of(cg, sel[0], sel[1], sel[2]) : -1;
  const bool grid = G.cell_start != nullptr;  // workgroup-uniform
  int2 rg = make_int2(0, 0);
  if (grid && tree >= 0) rg = range[tree];
  const bool covered = rg.y > rg.x;
  float d[5], lb6 = 0.0f;
  int p[5];
  int verdict = GRID_UNPROVEN;
  if (grid) verdict = knn5_grid<LOC_BLOCK>(G, on && tree >= 0 && covered, sel[0], sel[1], sel[2], FLT_MAX, 0.0f, (lds_u32 *)(rows_lds + tid), d, p, lb6);
  (void)lb6;
  bool by_grid = false, refused = false, to_tree = false;
  if (on && tree >= 0) {
    if (grid && covered && verdict == GRID_PROVEN) {
      // the proven five are the five nearest among ALL points of the covered cubes, each closer than the sixth by the proof's
      // margin: if all of them belong to this point's cube they are the five nearest inside it, in this order
      bool all_in = true;
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int id = __float_as_int(G.pts[p[j]].w);
        all_in = all_in && id >= rg.x && id < rg.y;
      }
      by_grid = all_in;
      refused = !all_in;
      to_tree = !all_in;
    } else if (grid && covered && verdict == GRID_FAR && !a.tap) {
      // farther than sqrt(5) m from every point of the covered cubes, this point's own among them: its fifth in-cube distance
      // is no smaller, the gate rejects it (d = FLT_MAX, p = -1)
      by_grid = true;
    } else {
      to_tree = true;
    }
  }
  if (on) {
    a.how[r.slot] = (uint8_t)(by_grid ? HOW_GRID : (to_tree ? HOW_TREE : HOW_SKIPPED));
    if (by_grid) {
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        a.nb_d[r.slot * 5 + j] = d[j];
        a.nb_p[r.slot * 5 + j] = p[j];
      }
    }
  }
  // the list and the counters: one atomic per wavefront and word
  const unsigned long long m_tree = __ballot(to_tree), m_on = __ballot(on), m_grid = __ballot(by_grid), m_ref = __ballot(refused);
  int base = 0;
  if (lane == 0) {
    if (m_tree) base = atomicAdd(a.list_cnt, __popcll(m_tree));
    atomicAdd(a.stat + ST_SWEPT, (unsigned long long)__popcll(m_on));
    if (m_grid) atomicAdd(a.stat + ST_PROVEN, (unsigned long long)__popcll(m_grid));
    if (m_ref) atomicAdd(a.stat + ST_REFUSED, (unsigned long long)__popcll(m_ref));
    if (m_tree) atomicAdd(a.stat + ST_TREES, (unsigned long long)__popcll(m_tree));
  }
  base = __shfl(base, 0, 64);
  if (to_tree) a.list[base + __popcll(m_tree & ((1ull << lane) - 1ull))] = (int32_t)r.slot;
}

// Pass 2: the listed points, each in the tree of its cube (nanoflann's traversal, lslam_device.hpp).
__global__ __launch_bounds__(LOC_TREE_BLOCK) void loc_tree_kernel(const LocArgs a) {
  __shared__ uint32_t stack_lds[2 * KD_STACK_LDS * LOC_TREE_BLOCK];
  if (a.st->done) return;
  const int n = *a.list_cnt;
  for (int first = blockIdx.x * LOC_TREE_BLOCK; first < n; first += gridDim.x * LOC_TREE_BLOCK) {
    const int k = first + threadIdx.x;
    if (k >= n) continue;
    const int slot = a.list[k];
    const PointRef r = point_of_block(a, slot / LOC_BLOCK, slot % LOC_BLOCK);
    const float4 q = a.q[r.t][r.off + r.i];
    float sel[3];
    to_map(a.st, q, sel);
    const CubeGridDev cg = r.t ? a.cg[1] : a.cg[0];
    const int tree = cube_tree_of(cg, sel[0], sel[1], sel[2]);  // >= 0: pass 1 listed it
    const TreeView T = cg.trees[tree];
    float d[5];
    int p[5];
    KdStack<LOC_TREE_BLOCK, false, KD_STACK_LDS> stk;
    stk.lds = (lds_u32 *)(stack_lds + threadIdx.x);
    stk.ovf = nullptr;
    stk.ovf_stride = 0;
    // beyond the gate nothing is looked up (FeatureMap.h: pointSearchSqDis[4] < 5.0); the tap runs nanoflann's plain search
    knn5_search<LOC_TREE_BLOCK, false, KD_STACK_LDS>(T, sel[0], sel[1], sel[2], d, p, stk, a.tap ? FLT_MAX : 5.0f * (1.0f + 1e-5f));
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      a.nb_d[(size_t)slot * 5 + j] = d[j];
      a.nb_p[(size_t)slot * 5 + j] = p[j];
    }
  }
}

// Pass 3: gate, findLine / findPlane, coefficient, Jacobian row and the block's sums -- every point in its own lane whichever
// pass found its neighbours.
__global__ __launch_bounds__(LOC_BLOCK) void loc_fit_kernel(const LocArgs a, const int jtj_mode) {
  __shared__ float red[LOC_BLOCK / 64][NCOL];
  __shared__ uint32_t stage[8 * LOC_BLOCK];
  if (a.st->done) return;
  const int tid = threadIdx.x;
  const PointRef r = point_of_block(a, blockIdx.x, tid);
  const bool is_surf = r.t != 0;
  float row[6] = {0, 0, 0, 0, 0, 0};
  float rb = 0.0f, kept = 0.0f, matched = 0.0f, score = 0.0f;
  const int how = r.i < r.n ? (int)a.how[r.slot] : HOW_SKIPPED;
  if (how != HOW_SKIPPED) {
    const float4 q = a.q[r.t][r.off + r.i];
    float sel[3], d[5], sc[6];
    int p[5];
    to_map(a.st, q, sel);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      d[j] = a.nb_d[r.slot * 5 + j];
      p[j] = a.nb_p[r.slot * 5 + j];
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) sc[j] = a.st->sc[j];
    SweepArgs sa = {};
    sa.fine_gate_c = sa.fine_gate_s = -1.0f;
    BlockDesc bd = {};
    const float4 *P = how == HOW_GRID ? (is_surf ? a.G[1].pts : a.G[0].pts) : a.tpts;
    point_residual(sa, bd, is_surf, P, q, sel, d, p, sc, row, rb, kept, matched, score);
  }
  block_accumulate<LOC_BLOCK, false>(jtj_mode, is_surf, row, rb, kept, matched, score, stage, red, a.partials + (size_t)blockIdx.x * NCOL);
}

// the tap's outputs: coordinates of the five, their distances, how
__global__ void loc_tap_out_kernel(const LocArgs a, int which, int nq, float *xyz, float *d2, uint8_t *how_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  const size_t slot = (size_t)(which ? a.nbc * LOC_BLOCK : 0) + i;
  const int how = a.how[slot];
  how_out[i] = (uint8_t)how;
  const float4 *P = how == HOW_GRID ? (which ? a.G[1].pts : a.G[0].pts) : a.tpts;
  for (int j = 0; j < 5; ++j) {
    const int p = how != HOW_SKIPPED ? a.nb_p[slot * 5 + j] : -1;
    const float4 v = p >= 0 ? P[p] : make_float4(0.f, 0.f, 0.f, 0.f);
    xyz[((size_t)i * 5 + j) * 3 + 0] = v.x;
    xyz[((size_t)i * 5 + j) * 3 + 1] = v.y;
    xyz[((size_t)i * 5 + j) * 3 + 2] = v.z;
    d2[(size_t)i * 5 + j] = how != HOW_SKIPPED ? a.nb_d[slot * 5 + j] : 0.0f;
  }
}

__global__ void loc_two_segments_kernel(int32_t *seg, int na, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) seg[i] = i < na ? 0 : 1;
}

// {first corner point, corner points, first surf point, surf points} of the filtered clouds: the filter's output is grouped by
// segment (0: corner, 1: surf) and done_x[0] (pinned) holds its length; the corner points are taken from run A, the surf points
// from run B (the same run when the two leaves are equal)
__global__ void loc_counts_kernel(const int32_t *seg_a, const uint32_t *done_a, const int32_t *seg_b, const uint32_t *done_b, int32_t *counts) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int32_t *seg[2] = {seg_a, seg_b};
  const int m[2] = {(int)done_a[0], (int)done_b[0]};
  int split[2];
  for (int k = 0; k < 2; ++k) {
    int lo = 0, hi = m[k];  // first position whose segment is not 0
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (seg[k][mid] == 0) lo = mid + 1; else hi = mid;
    }
    split[k] = lo;
  }
  counts[0] = 0;
  counts[1] = split[0];
  counts[2] = split[1];
  counts[3] = m[1] - split[1];
}

// the grid's source points: the covered cubes' ranges of the trees' array back to back, .w = position in this numbering
__global__ void loc_gather_kernel(const float4 *pts, const int32_t *src_begin, const int32_t *dst_begin, int n_seg, int n_out, float4 *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_out) return;
  int lo = 0, hi = n_seg - 1;  // last segment with dst_begin <= i
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (dst_begin[mid] <= i) lo = mid; else hi = mid - 1;
  }
  float4 p = pts[src_begin[lo] + (i - dst_begin[lo])];
  p.w = __int_as_float(i);
  out[i] = p;
}

// ---- the paged window (util/DynamicFeatureMap.h) ----------------------------------------------------------------------------
// [first, end) of every segment in a VoxelGrid run's output, which is grouped by segment: bounds[2 s], bounds[2 s + 1]; a segment
// that left nothing keeps the zeros it was given.  done[0] (pinned) is the output's length, known to the device before the host;
// n_in bounds it.
__global__ __launch_bounds__(256) void pm_bounds_kernel(const int32_t *seg, const uint32_t *done, int n_in, int nseg, int32_t *bounds) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int m = min((int)done[0], n_in);
  if (i >= m) return;
  const int sg = seg[i];
  if (sg < 0 || sg >= nseg) return;
  if (i == 0 || seg[i - 1] != sg) bounds[2 * sg] = i;
  if (i == m - 1 || seg[i + 1] != sg) bounds[2 * sg + 1] = i + 1;
}

// Every filtered point of the entering cubes to its cube's extent, in both arenas: fpts keeps the filter's order
// (getSurroundFeature hands the clouds out as the filter left them), tpts is what the forest build permutes.  dst[s] < 0: the
// segment's cube got no room (nothing is written for it).
__global__ __launch_bounds__(256) void pm_place_kernel(const float4 *src, const int32_t *seg, const uint32_t *done, int n_in, int nseg,
                                                      const int32_t *bounds, const int32_t *dst, float4 *fpts, float4 *tpts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int m = min((int)done[0], n_in);
  if (i >= m) return;
  const int sg = seg[i];
  if (sg < 0 || sg >= nseg) return;
  const int base = dst[sg];
  if (base < 0) return;
  const int at = base + (i - bounds[2 * sg]);
  const float4 v = src[i];
  fpts[at] = v;
  tpts[at] = v;
}

typedef std::array<int, 3> CubeKey;  // a global cube index (i, j, k)

struct PmExtent {
  int64_t off, len;
};
// first fit; the free list is kept in ascending order with neighbours merged
bool ext_alloc(std::vector<PmExtent> &fl, int64_t len, int64_t *off) {
  for (size_t k = 0; k < fl.size(); ++k)
    if (fl[k].len >= len) {
      *off = fl[k].off;
      fl[k].off += len;
      fl[k].len -= len;
      if (!fl[k].len) fl.erase(fl.begin() + (long)k);
      return true;
    }
  return false;
}
void ext_free(std::vector<PmExtent> &fl, int64_t off, int64_t len) {
  if (len <= 0) return;
  size_t k = 0;
  while (k < fl.size() && fl[k].off < off) ++k;
  fl.insert(fl.begin() + (long)k, PmExtent{off, len});
  if (k + 1 < fl.size() && fl[k].off + fl[k].len == fl[k + 1].off) {
    fl[k].len += fl[k + 1].len;
    fl.erase(fl.begin() + (long)k + 1);
  }
  if (k > 0 && fl[k - 1].off + fl[k - 1].len == fl[k].off) {
    fl[k - 1].len += fl[k].len;
    fl.erase(fl.begin() + (long)k);
  }
}

struct PagedCube {  // a listed cube of one type the node holds: in the window, or staged beside it
  int32_t file = -1;
  int64_t off = 0;     // its filtered points: [off, off + len) of both arenas
  int32_t len = 0;
  int32_t batch = -1;  // the forest build its tree came from (-1: fewer than five points, no tree)
  TreeView view{};
  bool staged = false;
};
struct NodeBatch {  // the node extent of one forest build; it goes back when the last of its trees has left
  int64_t off = 0, cap = 0;
  int32_t refs = 0, depth = 0;
};

struct Paged {
  bool on = false, have_window = false;
  std::string dir;
  std::map<CubeKey, int32_t> index[2];  // setupPCDFileName: global cube -> <count> of its file
  int centre[3] = {0, 0, 0};
  std::map<CubeKey, PagedCube> cubes[2];
  std::vector<NodeBatch> batches;
  std::vector<CubeKey> active;          // computeActiveAera: global indices in its loop order
  // the arenas: lslam_loc::tpts (the trees' points) and fpts (the same extents in the filter's order), lslam_loc::nodes
  DevBuf<float4> fpts;
  size_t cap_pts = 0, cap_nodes = 0;
  std::vector<PmExtent> free_pts, free_nodes;
  size_t limit = 0;                     // lslam_pmap_setup_capacity (0: none)
  size_t used[2] = {0, 0};              // filtered points held per type, staged included
  size_t nodes_used = 0;
  bool tables_stale = false;            // an arena moved: the device tables point into the old one
  // a step's staging
  PinBuf<float4> in_pin;
  PinBuf<int32_t> seg_pin, h_bounds[2], h_dst[2];
  PinBuf<uint32_t> done;                // [2 types][4]
  DevBuf<float4> in_raw, out[2];
  DevBuf<int32_t> seg, oseg[2], bounds[2], dst[2];
  // the window tables, two sets that alternate
  int flip = 0;
  PinBuf<int32_t> h_cells[2][2];
  PinBuf<TreeView> h_views[2];
  DevBuf<int32_t> d_cells[2][2];
  DevBuf<TreeView> d_views[2];
  lslam_loc_window_stats st{};
};

struct Result {  // what one sweep brings back (pinned)
  GNState st;
  unsigned long long stat[ST_N];
};

void identity16(float T[16]) {
  for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0f : 0.0f;
}

}  // namespace

struct lslam_loc {
  lslam_ctx *ctx = nullptr;
  hipStream_t stream = nullptr;
  lslam_fmap *fm = nullptr;  // the map store: cubes, PCD reader, per-cube VoxelGrid (never installed in the context)
  int W = 0, H = 0, D = 0;
  float scan_leaf[2] = {1.0f, 1.0f};  // LaserMatcher.cpp:80-85
  float map_leaf[2] = {1.0f, 1.0f};   // :87-92,116
  bool use_grid = true;
  // ---- the map's search structures (install) ----
  bool have_map = false;
  FmapView view{};
  DevBuf<float4> tpts;        // [corner points | surf points], permuted inside every tree's range by its build
  DevBuf<KdNode> nodes;
  DevBuf<TreeView> d_views;   // [corner trees | surf trees]
  DevBuf<int32_t> d_cells[2]; // cube -> tree of the type, -1: none
  std::vector<int32_t> tree_cube[2], tree_l[2], tree_r[2];  // per tree: its cube, its range in tpts
  CubeGridDev cg[2] = {};
  int tree_depth = 0;
  int64_t cubes_loaded[2] = {0, 0};
  int64_t structure_builds = 0, grid_builds = 0;
  // ---- cell grids over the cubes around the sensor ----
  GridDev grid[2];
  DevBuf<float4> gsrc[2];
  DevBuf<int2> d_range[2];
  DevBuf<int32_t> d_gseg[2];  // [src begin | dst begin]
  std::vector<int2> h_range[2];
  std::vector<int32_t> h_gseg[2];
  DevBuf<uint32_t> bbox12;
  // cell edge per type: 1.4 x the leaf the map's cubes were filtered with, inside [0.6, 1.4] m -- the probe proves a point only
  // when its fifth neighbour is closer than c (1 + distance to the nearest cell wall), and in a map filtered at 1.0 m the fifth
  // neighbour is 1.0 - 1.4 m away (0.6 m cells proved 2 % of such a map's points); 0.6 m for a map whose spacing is not known
  float grid_cell[2] = {GRID_CELL_DEFAULT, GRID_CELL_DEFAULT};
  bool grid_valid = false;
  int grid_cube[3] = {0, 0, 0};
  int grid_reach = 0;
  // ---- one sweep's scratch ----
  PinBuf<float4> in_pin;
  DevBuf<float4> in_raw, out_pts[2];
  DevBuf<int32_t> seg, out_seg[2], counts, list, ctr;
  PinBuf<uint32_t> done;  // [2 runs][4]
  DevBuf<float> nb_d, partials;
  DevBuf<int32_t> nb_p;
  DevBuf<uint8_t> how;
  DevBuf<unsigned long long> stat;
  DevBuf<GNState> d_state;
  DevBuf<ProbBlocks> d_probs;
  PinBuf<GNState> h_state;
  PinBuf<Result> h_res;
  // ---- LaserLocalization's pose state ----
  bool initialized = false, reset_pending = false;
  float reset_pose[16], mapped_last[16], odom_last[16], pose_last[16];
  int64_t stamp_last = 0;
  float velocity[3] = {0, 0, 0};
  lslam_loc_search_counts cnt{};
  // ---- the paged mode (lslam_pmap_open) ----
  float cfg_cube = 50.0f, cfg_valid = 150.0f;  // what the setup calls said (the store's own defaults)
  Paged pg;
  // ---- re-localisation (lslam_reloc_*): the map's occupancy sets and the coarse stage's scratch ----
  DevBuf<unsigned long long> occ_tab;  // [2 types][occ_cap] packed voxel keys, RL_EMPTY: free
  DevBuf<unsigned long long> occ_cnt;  // [2]
  size_t occ_cap = 0;
  float occ_voxel = 0.0f;
  int64_t occ_epoch = -1;              // structure_builds when the sets were built
  int64_t occ_builds = 0, occ_voxels[2] = {0, 0};
  DevBuf<float4> rl_scan, rl_pos;
  DevBuf<float> rl_R;
  DevBuf<int32_t> rl_meta, rl_scores, rl_blk, rl_sel, rl_out;
  DevBuf<uint32_t> rl_hist;
  DevBuf<unsigned long long> rl_keys;
  PinBuf<float4> rl_pos_pin;
  PinBuf<float> rl_R_pin;
  PinBuf<int32_t> rl_out_pin;
};

namespace {

int check_loc(lslam_loc *loc, const char *fn) {
  if (!loc) {
    char b[128];
    std::snprintf(b, sizeof(b), "%s: null localisation node", fn);
    lslam::set_error(b);
    return LSLAM_ERR_INVALID;
  }
  if (!lslam::ctx_alive(loc->ctx)) {
    lslam::set_error("localisation node: its ctx was destroyed");
    return LSLAM_ERR_INVALID;
  }
  LOC_TRY(hipSetDevice(lslam::ctx_device(loc->ctx)));
  return LSLAM_OK;
}

int invalid(const char *fn, const char *what) {
  char b[256];
  std::snprintf(b, sizeof(b), "%s: %s", fn, what);
  lslam::set_error(b);
  return LSLAM_ERR_INVALID;
}

void set_grid_cells(lslam_loc *loc, bool filtered) {
  for (int t = 0; t < 2; ++t)
    loc->grid_cell[t] = filtered ? std::min(1.4f, std::max(GRID_CELL_DEFAULT, 1.4f * loc->map_leaf[t])) : GRID_CELL_DEFAULT;
}

void cube_of(const lslam_loc *loc, const float pos[3], int g[3]) {  // worldToCube, FeatureMap.h:475-487
  for (int d = 0; d < 3; ++d) g[d] = (int)(std::round(pos[d] / loc->view.cube_size) + (float)loc->view.origin[d]);
}

// Every cube tree of the map the store holds, in one forest build; the cell grids are built when the first sweep says where the sensor is.
int install(lslam_loc *loc) {
  loc->have_map = false;
  loc->grid_valid = false;
  int rc = lslam::fmap_view(loc->fm, &loc->view);
  if (rc) return rc;
  const FmapView &v = loc->view;
  hipStream_t s = loc->stream;
  const size_t ncube = (size_t)v.W * v.H * v.D;
  const size_t n0 = v.n[0], n_total = v.n[0] + v.n[1];
  std::vector<int32_t> cells[2], roots_lr;
  for (int t = 0; t < 2; ++t) {
    cells[t].assign(ncube, -1);
    loc->tree_cube[t].clear();
    loc->tree_l[t].clear();
    loc->tree_r[t].clear();
    loc->cubes_loaded[t] = 0;
    const size_t base = t ? n0 : 0;
    for (size_t c = 0; c < ncube; ++c) {
      const int32_t b = v.begin[t][c], e = v.end[t][c];
      if (e > b) loc->cubes_loaded[t]++;
      if (e - b < 5) continue;  // FeatureMap.h:524,546: such a cube is skipped by the match
      cells[t][c] = (int32_t)loc->tree_cube[t].size();
      loc->tree_cube[t].push_back((int32_t)c);
      loc->tree_l[t].push_back((int32_t)(base + (size_t)b));
      loc->tree_r[t].push_back((int32_t)(base + (size_t)e));
      roots_lr.push_back((int32_t)(base + (size_t)b));
      roots_lr.push_back((int32_t)(base + (size_t)e));
    }
  }
  const int Tc = (int)loc->tree_cube[0].size(), T = Tc + (int)loc->tree_cube[1].size();
  LOC_TRY(loc->tpts.reserve(n_total + 16));
  LOC_TRY(loc->d_views.reserve((size_t)T + 1));
  std::vector<TreeView> views((size_t)T);
  int max_depth = 0, fallback = 0;
  size_t n_leaves = 0;
  auto copy_points = [&]() -> hipError_t {
    hipError_t e = hipSuccess;
    for (int t = 0; t < 2 && e == hipSuccess; ++t)
      if (v.n[t]) e = hipMemcpyAsync(loc->tpts.p + (t ? n0 : 0), v.pts[t], v.n[t] * sizeof(float4), hipMemcpyDeviceToDevice, s);
    return e;
  };
  LOC_TRY(copy_points());
  for (int attempt = 0; attempt < 3 && T > 0; ++attempt) {
    const size_t mult[3] = {2, 8, 24};
    const size_t cap = ((mult[attempt] * n_total / 3 + 64 + 8 * (size_t)T) + 7) & ~(size_t)7;
    LOC_TRY(loc->nodes.reserve(cap));
    if (attempt > 0) LOC_TRY(copy_points());  // the failed attempt permuted the points
    LOC_TRY(lslam::build_kdforest_device(lslam::ctx_build_pool(loc->ctx, 0), loc->tpts.p, (int32_t)n_total, roots_lr.data(), T, loc->nodes.p,
                                         nullptr, (int32_t)cap, s, views.data(), &max_depth, &n_leaves, &fallback));
    if (fallback != 1) break;
  }
  if (fallback) {
    lslam::set_error("localisation node: the device cube-tree build hit a structure limit");
    return fallback == 1 || fallback == 2 ? LSLAM_ERR_TREE_BUILD : LSLAM_ERR_TREE_DEPTH;
  }
  if (max_depth > KD_STACK_LDS + 1) {
    lslam::set_error("localisation node: a cube tree is deeper than the device traversal stack");
    return LSLAM_ERR_TREE_DEPTH;
  }
  for (int t = 0; t < 2; ++t) {
    LOC_TRY(loc->d_cells[t].reserve(ncube));
    LOC_TRY(hipMemcpyAsync(loc->d_cells[t].p, cells[t].data(), ncube * sizeof(int32_t), hipMemcpyHostToDevice, s));
  }
  if (T) LOC_TRY(hipMemcpyAsync(loc->d_views.p, views.data(), (size_t)T * sizeof(TreeView), hipMemcpyHostToDevice, s));
  LOC_TRY(hipStreamSynchronize(s));  // (cells / views are locals)
  for (int t = 0; t < 2; ++t) {
    CubeGridDev &g = loc->cg[t];
    g.cube_size = v.cube_size;
    g.origin[0] = v.origin[0]; g.origin[1] = v.origin[1]; g.origin[2] = v.origin[2];
    g.dims[0] = v.W; g.dims[1] = v.H; g.dims[2] = v.D;
    g.cell_tree = loc->d_cells[t].p;
    g.trees = loc->d_views.p + (t ? Tc : 0);
  }
  loc->tree_depth = max_depth;
  loc->structure_builds++;
  loc->have_map = true;
  return LSLAM_OK;
}

// The cell grids over the cubes within `reach` cubes of the sensor's (all three axes), both types; rebuilt only when the
// sensor's cube changes.  A reach whose cell tables would be too large (GRID_MAX_DIM / GRID_MAX_CELLS) is shrunk; a type that
// gets no grid even for the sensor's own cube goes through its trees.
int ensure_grids(lslam_loc *loc, const int g[3]) {
  if (loc->grid_valid && g[0] == loc->grid_cube[0] && g[1] == loc->grid_cube[1] && g[2] == loc->grid_cube[2]) return LSLAM_OK;
  hipStream_t s = loc->stream;
  const FmapView &v = loc->view;
  const int dims[3] = {v.W, v.H, v.D};
  int reach = (int)std::ceil(v.valid_dist / v.cube_size);
  reach = std::max(0, std::min(reach, 8));
  loc->grid[0].view = CellGrid{};
  loc->grid[1].view = CellGrid{};
  for (; reach >= 0; --reach) {
    int n_sel[2] = {0, 0};
    for (int t = 0; t < 2; ++t) {
      const size_t nt = loc->tree_cube[t].size();
      loc->h_range[t].assign(nt, make_int2(0, 0));
      std::vector<int32_t> src, dst;
      for (size_t k = 0; k < nt; ++k) {
        const int c = loc->tree_cube[t][k];
        const int ci = c % v.W, cj = (c / v.W) % v.H, ck = c / (v.W * v.H);
        if (std::abs(ci - g[0]) > reach || std::abs(cj - g[1]) > reach || std::abs(ck - g[2]) > reach) continue;
        const int len = loc->tree_r[t][k] - loc->tree_l[t][k];
        loc->h_range[t][k] = make_int2(n_sel[t], n_sel[t] + len);
        src.push_back(loc->tree_l[t][k]);
        dst.push_back(n_sel[t]);
        n_sel[t] += len;
      }
      loc->h_gseg[t] = src;
      loc->h_gseg[t].insert(loc->h_gseg[t].end(), dst.begin(), dst.end());
      LOC_TRY(loc->d_range[t].reserve(nt + 1));
      if (nt) LOC_TRY(hipMemcpyAsync(loc->d_range[t].p, loc->h_range[t].data(), nt * sizeof(int2), hipMemcpyHostToDevice, s));
      if (n_sel[t]) {
        const int n_seg = (int)src.size();
        LOC_TRY(loc->d_gseg[t].reserve(2 * (size_t)n_seg));
        LOC_TRY(hipMemcpyAsync(loc->d_gseg[t].p, loc->h_gseg[t].data(), 2 * (size_t)n_seg * sizeof(int32_t), hipMemcpyHostToDevice, s));
        LOC_TRY(loc->gsrc[t].reserve((size_t)n_sel[t] + 16));
        hipLaunchKernelGGL(loc_gather_kernel, dim3((n_sel[t] + 255) / 256), dim3(256), 0, s, (const float4 *)loc->tpts.p,
                           (const int32_t *)loc->d_gseg[t].p, (const int32_t *)loc->d_gseg[t].p + n_seg, n_seg, n_sel[t], loc->gsrc[t].p);
      }
    }
    LOC_TRY(hipGetLastError());
    LOC_TRY(loc->bbox12.reserve(12));
    const float4 *const bp[2] = {loc->gsrc[0].p, loc->gsrc[1].p};
    float lo[2][3], hi[2][3];
    LOC_TRY(lslam::grid_bbox2(bp, n_sel, loc->bbox12.p, lo, hi, s));  // (one wait; also covers the uploads above)
    bool too_large = false;
    for (int t = 0; t < 2; ++t) {
      int status = 0;
      if (n_sel[t]) LOC_TRY(loc->grid[t].build(loc->gsrc[t].p, n_sel[t], lo[t], hi[t], loc->grid_cell[t], s, &status, true));
      if (status == 2 && reach > 0) too_large = true;
      if (status) loc->grid[t].view = CellGrid{};
    }
    if (!too_large) break;
  }
  loc->grid_reach = std::max(reach, 0);
  for (int d = 0; d < 3; ++d) loc->grid_cube[d] = g[d];
  (void)dims;
  loc->grid_valid = true;
  loc->grid_builds++;
  return LSLAM_OK;
}

void fill_args(lslam_loc *loc, LocArgs &a, int nbc, int nbs, int tap) {
  a = LocArgs{};
  a.counts = loc->counts.p;
  a.nbc = nbc;
  a.nb_total = nbc + nbs;
  for (int t = 0; t < 2; ++t) {
    a.cg[t] = loc->cg[t];
    a.G[t] = loc->use_grid ? loc->grid[t].view : CellGrid{};
    a.range[t] = loc->d_range[t].p;
  }
  a.tpts = loc->tpts.p;
  a.st = loc->d_state.p;
  a.nb_d = loc->nb_d.p;
  a.nb_p = loc->nb_p.p;
  a.how = loc->how.p;
  a.list = loc->list.p;
  a.stat = loc->stat.p;
  a.partials = loc->partials.p;
  a.tap = tap;
}

int reserve_search(lslam_loc *loc, int nb_total) {
  const size_t slots = (size_t)std::max(nb_total, 1) * LOC_BLOCK;
  LOC_TRY(loc->nb_d.reserve(slots * 5));
  LOC_TRY(loc->nb_p.reserve(slots * 5));
  LOC_TRY(loc->how.reserve(slots));
  LOC_TRY(loc->list.reserve(slots));
  LOC_TRY(loc->partials.reserve((size_t)std::max(nb_total, 1) * NCOL));
  LOC_TRY(loc->ctr.reserve(LOC_MAX_ITER + 2));
  LOC_TRY(loc->stat.reserve(ST_N));
  LOC_TRY(loc->counts.reserve(4));
  LOC_TRY(loc->d_state.reserve(1));
  LOC_TRY(loc->d_probs.reserve(1));
  LOC_TRY(loc->h_state.reserve(1));
  LOC_TRY(loc->h_res.reserve(1));
  LOC_TRY(loc->done.reserve(8));
  return LSLAM_OK;
}

void launch_search(const LocArgs &a, hipStream_t s) {
  if (a.nb_total <= 0) return;
  hipLaunchKernelGGL(loc_probe_kernel, dim3(a.nb_total), dim3(LOC_BLOCK), 0, s, a);
  const int tree_blocks = std::min(a.nb_total * (LOC_BLOCK / LOC_TREE_BLOCK), 1024);
  hipLaunchKernelGGL(loc_tree_kernel, dim3(tree_blocks), dim3(LOC_TREE_BLOCK), 0, s, a);
}

// prepareFeatureFrame: the clouds are in in_raw already ([corner | surf], packed) when from_device, else they are packed and
// uploaded here; both go through the scan filters, and counts (device) says where the filtered clouds lie.  Nothing is waited
// for unless sync_filter: then the filter waits for its own result (the fall-back of a key-range error).
int prepare_scan(lslam_loc *loc, const void *corner, size_t n_corner, const void *surf, size_t n_surf, size_t stride_bytes,
                 bool from_device, bool sync_filter) {
  hipStream_t s = loc->stream;
  const size_t n = n_corner + n_surf;
  if (n > ((size_t)1 << 27)) return invalid("lslam_loc_process", "too many scan points");
  const int nbc = (int)((n_corner + LOC_BLOCK - 1) / LOC_BLOCK), nbs = (int)((n_surf + LOC_BLOCK - 1) / LOC_BLOCK);
  int rc = reserve_search(loc, nbc + nbs);
  if (rc) return rc;
  LOC_TRY(hipMemsetAsync(loc->counts.p, 0, 4 * sizeof(int32_t), s));
  for (int k = 0; k < 8; ++k) loc->done.p[k] = 0;
  const bool two_runs = loc->scan_leaf[0] != loc->scan_leaf[1];
  if (n) {
    LOC_TRY(loc->in_raw.reserve(n));
    LOC_TRY(loc->seg.reserve(n));
    for (int k = 0; k < 2; ++k) {
      LOC_TRY(loc->out_pts[k].reserve(n));
      LOC_TRY(loc->out_seg[k].reserve(n));
    }
    if (from_device) {
      if (n_corner) LOC_TRY(hipMemcpyAsync(loc->in_raw.p, corner, n_corner * sizeof(float4), hipMemcpyDeviceToDevice, s));
      if (n_surf) LOC_TRY(hipMemcpyAsync(loc->in_raw.p + n_corner, surf, n_surf * sizeof(float4), hipMemcpyDeviceToDevice, s));
    } else {
      LOC_TRY(loc->in_pin.reserve(n));
      const void *src[2] = {corner, surf};
      const size_t cnt[2] = {n_corner, n_surf};
      size_t at = 0;
      for (int k = 0; k < 2; ++k) {
        const char *p = static_cast<const char *>(src[k]);
        float4 *h = loc->in_pin.p + at;
        if (stride_bytes == 16) {
          if (cnt[k]) std::memcpy(h, p, cnt[k] * sizeof(float4));
        } else {
          for (size_t i = 0; i < cnt[k]; ++i) {
            float v[3], w = 0.0f;
            std::memcpy(v, p + i * stride_bytes, 12);
            if (stride_bytes >= 20) std::memcpy(&w, p + i * stride_bytes + 16, 4);  // pcl::PointXYZI keeps the intensity at byte 16
            h[i] = make_float4(v[0], v[1], v[2], w);
          }
        }
        at += cnt[k];
      }
      LOC_TRY(hipMemcpyAsync(loc->in_raw.p, loc->in_pin.p, n * sizeof(float4), hipMemcpyHostToDevice, s));
      loc->cnt.bytes_up[0] += n * sizeof(float4);
    }
    hipLaunchKernelGGL(loc_two_segments_kernel, dim3(((unsigned)n + 255) / 256), dim3(256), 0, s, loc->seg.p, (int)n_corner, (int)n);
    // lslam_voxel_grid2's pipeline (two segments, each with its own min_b and "leaf too small" guard), device to device
    for (int k = 0; k < (two_runs ? 2 : 1); ++k) {
      size_t m = 0;
      uint32_t *done = loc->done.p + 4 * k;
      rc = lslam::voxel_filter_segments(loc->ctx, loc->in_raw.p, loc->seg.p, n, 2, loc->scan_leaf[k], loc->out_pts[k].p, loc->out_seg[k].p, &m,
                                        true, sync_filter ? nullptr : done);
      if (rc) return rc;
      if (sync_filter) {
        LOC_TRY(hipStreamSynchronize(s));
        loc->cnt.host_waits[0]++;
        done[0] = (uint32_t)m;
        done[1] = 0;
      }
    }
    const int kb = two_runs ? 1 : 0;
    hipLaunchKernelGGL(loc_counts_kernel, dim3(1), dim3(64), 0, s, (const int32_t *)loc->out_seg[0].p, (const uint32_t *)loc->done.p,
                       (const int32_t *)loc->out_seg[kb].p, (const uint32_t *)(loc->done.p + 4 * kb), loc->counts.p);
  }
  return LSLAM_OK;
}

// the filter's wide key did not hold a voxel extent (known after a wait): prepare_scan has to run again with sync_filter
bool scan_filter_overflowed(const lslam_loc *loc) { return loc->done.p[1] || loc->done.p[5]; }

// optimizeTransform over the scan prepare_scan left (n_corner / n_surf as given there), from a Twist (in/out): one host wait.
// *refilter: the wait showed that the scan has to be prepared again (nothing was written).
int solve_scan(lslam_loc *loc, size_t n_corner, size_t n_surf, float pose[6], lslam_stats *stats, bool *refilter) {
  hipStream_t s = loc->stream;
  *refilter = false;
  const int nbc = (int)((n_corner + LOC_BLOCK - 1) / LOC_BLOCK), nbs = (int)((n_surf + LOC_BLOCK - 1) / LOC_BLOCK);
  const int nb_total = nbc + nbs;
  const bool two_runs = loc->scan_leaf[0] != loc->scan_leaf[1];
  {
    float pos[3] = {pose[3], pose[4], pose[5]};
    int g[3];
    cube_of(loc, pos, g);
    int rc = ensure_grids(loc, g);
    if (rc) return rc;
  }
  LOC_TRY(hipMemsetAsync(loc->ctr.p, 0, (LOC_MAX_ITER + 2) * sizeof(int32_t), s));
  LOC_TRY(hipMemsetAsync(loc->stat.p, 0, ST_N * sizeof(unsigned long long), s));
  // the Gauss-Newton loop, enqueued whole: a launch whose loop has ended leaves at once (GNState::done)
  GNState &h = *loc->h_state.p;
  std::memset(&h, 0, sizeof(h));
  for (int i = 0; i < 6; ++i) h.pose[i] = pose[i];
  struct HostSinCos {
    void operator()(float a, float &sn, float &cs) const { sn = std::sin(a); cs = std::cos(a); }
  };
  pose_to_Rt_sc(pose, h.R, h.t, h.sc, HostSinCos());
  LOC_TRY(hipMemcpyAsync(loc->d_state.p, &h, sizeof(GNState), hipMemcpyHostToDevice, s));
  const ProbBlocks pb = {0, nb_total};
  LOC_TRY(hipMemcpyAsync(loc->d_probs.p, &pb, sizeof(pb), hipMemcpyHostToDevice, s));
  LocArgs a;
  fill_args(loc, a, nbc, nbs, 0);
  a.q[0] = loc->out_pts[0].p;
  a.q[1] = loc->out_pts[two_runs ? 1 : 0].p;
  SolveArgs so{};
  so.states = loc->d_state.p;
  so.partials = loc->partials.p;
  so.probs = loc->d_probs.p;
  so.n_prob = 1;
  so.max_iterations = LOC_MAX_ITER;
  so.delta_r_abort = 0.05f;
  so.delta_t_abort = 0.05f;
  so.eig_thresh = 100.0f;
  so.min_rows = 50;
  for (int it = 0; it < LOC_MAX_ITER; ++it) {
    a.list_cnt = loc->ctr.p + it;
    launch_search(a, s);
    if (nb_total > 0) hipLaunchKernelGGL(loc_fit_kernel, dim3(nb_total), dim3(LOC_BLOCK), 0, s, a, 1);
    LOC_TRY(hipGetLastError());
    LOC_TRY(launch_solve(so, s));
  }
  Result &res = *loc->h_res.p;
  LOC_TRY(hipMemcpyAsync(&res.st, loc->d_state.p, sizeof(GNState), hipMemcpyDeviceToHost, s));
  LOC_TRY(hipMemcpyAsync(res.stat, loc->stat.p, sizeof(res.stat), hipMemcpyDeviceToHost, s));
  LOC_TRY(hipStreamSynchronize(s));  // the sweep's one wait
  loc->cnt.host_waits[0]++;
  loc->cnt.bytes_down[0] += sizeof(Result);
  loc->cnt.bytes_up[0] += sizeof(GNState) + sizeof(ProbBlocks);
  if (scan_filter_overflowed(loc)) {
    *refilter = true;
    return LSLAM_OK;
  }
  const GNState &g = res.st;
  for (int i = 0; i < 6; ++i) pose[i] = g.pose[i];  // transformf = transform: always written back
  const int status = g.converged ? LSLAM_OK : (g.too_few ? LSLAM_TOO_FEW_MATCHES : LSLAM_NOT_CONVERGED);
  loc->cnt.swept[0] += res.stat[ST_SWEPT];
  loc->cnt.grid_proven[0] += res.stat[ST_PROVEN];
  loc->cnt.cube_refused[0] += res.stat[ST_REFUSED];
  loc->cnt.to_trees[0] += res.stat[ST_TREES];
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    stats->status = status;
    stats->iterations = g.iter;
    stats->n_line = g.n_line;
    stats->n_plane = g.n_plane;
    stats->n_rows = g.n_rows;
    stats->degenerate = g.degenerate;
    stats->converged = g.converged;
    stats->delta_r = g.delta_r;
    stats->delta_t = g.delta_t;
    stats->sweeps = g.sweeps;
    stats->point_residuals = (int64_t)res.stat[ST_SWEPT];
  }
  return status;
}

// prepareFeatureFrame + optimizeTransform
int match_impl(lslam_loc *loc, const void *corner, size_t n_corner, const void *surf, size_t n_surf, size_t stride_bytes,
               bool from_device, float pose[6], lslam_stats *stats, bool sync_filter, int32_t *flags) {
  int rc = prepare_scan(loc, corner, n_corner, surf, n_surf, stride_bytes, from_device, sync_filter);
  if (rc) return rc;
  bool refilter = false;
  rc = solve_scan(loc, n_corner, n_surf, pose, stats, &refilter);
  if (refilter && !sync_filter) {
    // the filter's wide key did not hold a voxel extent: once more, with the filter measuring it (waits inside)
    if (flags) *flags |= LSLAM_LOC_SECOND_WAIT;
    return match_impl(loc, corner, n_corner, surf, n_surf, stride_bytes, from_device, pose, stats, true, flags);
  }
  return rc;
}

void begin_sweep_counts(lslam_loc *loc) {
  lslam_loc_search_counts &c = loc->cnt;
  uint64_t *f[] = {c.swept, c.grid_proven, c.cube_refused, c.to_trees, c.fallback_sweeps, c.host_waits, c.bytes_up, c.bytes_down};
  for (uint64_t *p : f) p[0] = 0;
}
void end_sweep_counts(lslam_loc *loc) {
  lslam_loc_search_counts &c = loc->cnt;
  uint64_t *f[] = {c.swept, c.grid_proven, c.cube_refused, c.to_trees, c.fallback_sweeps, c.host_waits, c.bytes_up, c.bytes_down};
  for (uint64_t *p : f) p[1] += p[0];
}

// ---- the paged window: host side -------------------------------------------------------------------------------------------
bool pm_in_window(const lslam_loc *loc, const int c[3], const CubeKey &g) {
  return std::abs(g[0] - c[0]) <= loc->W / 2 && std::abs(g[1] - c[1]) <= loc->H / 2 && std::abs(g[2] - c[2]) <= loc->D / 2;
}

void pm_release_cube(lslam_loc *loc, int t, const PagedCube &cu) {
  Paged &pg = loc->pg;
  ext_free(pg.free_pts, cu.off, cu.len);
  pg.used[t] -= (size_t)cu.len;
  if (cu.batch >= 0) {
    NodeBatch &b = pg.batches[(size_t)cu.batch];
    if (--b.refs == 0) {
      ext_free(pg.free_nodes, b.off, b.cap);
      pg.nodes_used -= (size_t)b.cap;
      b.cap = 0;
    }
  }
}

// staged cubes a window centred on `keep` would not take: their room goes back
void pm_drop_staged(lslam_loc *loc, const int keep[3]) {
  Paged &pg = loc->pg;
  for (int t = 0; t < 2; ++t)
    for (auto it = pg.cubes[t].begin(); it != pg.cubes[t].end();) {
      if (it->second.staged && !(keep && pm_in_window(loc, keep, it->first))) {
        pm_release_cube(loc, t, it->second);
        pg.st.staged_dropped_total[t]++;
        it = pg.cubes[t].erase(it);
      } else {
        ++it;
      }
    }
}

void pm_reset(lslam_loc *loc) {  // every cube gone, the arenas empty (their memory is kept)
  Paged &pg = loc->pg;
  pg.cubes[0].clear();
  pg.cubes[1].clear();
  pg.batches.clear();
  pg.active.clear();
  pg.free_pts.clear();
  pg.free_nodes.clear();
  if (pg.cap_pts) pg.free_pts.push_back(PmExtent{0, (int64_t)pg.cap_pts});
  if (pg.cap_nodes) pg.free_nodes.push_back(PmExtent{0, (int64_t)pg.cap_nodes});
  pg.used[0] = pg.used[1] = 0;
  pg.nodes_used = 0;
  pg.have_window = false;
  pg.tables_stale = false;
}

// Both point arenas to at least `want` points, contents kept; every view is moved along.  The device tables keep pointing into
// the old arena until they are rewritten (tables_stale).
int pm_grow_points(lslam_loc *loc, size_t want) {
  Paged &pg = loc->pg;
  hipStream_t s = loc->stream;
  if (want > ((size_t)1 << 30)) return invalid("paged window", "more than 2^30 points");
  const size_t old = pg.cap_pts;
  const float4 *before = loc->tpts.p;
  LOC_TRY(pg.fpts.grow(want + 16, old, s));
  LOC_TRY(loc->tpts.grow(want + 16, old, s));
  if (loc->tpts.p != before) {
    for (int t = 0; t < 2; ++t)
      for (auto &kv : pg.cubes[t])
        if (kv.second.batch >= 0) kv.second.view.pts = loc->tpts.p;
    pg.tables_stale = true;
  }
  const size_t cap = std::min(pg.fpts.cap, loc->tpts.cap) - 16;
  if (cap > old) ext_free(pg.free_pts, (int64_t)old, (int64_t)(cap - old));
  pg.cap_pts = std::max(cap, old);
  return LSLAM_OK;
}
int pm_grow_nodes(lslam_loc *loc, size_t want) {
  Paged &pg = loc->pg;
  const size_t old = pg.cap_nodes;
  const KdNode *before = loc->nodes.p;
  LOC_TRY(loc->nodes.grow(want, old, loc->stream));
  if (loc->nodes.p != before) {
    for (int t = 0; t < 2; ++t)
      for (auto &kv : pg.cubes[t])
        if (kv.second.batch >= 0) kv.second.view.nodes = loc->nodes.p + pg.batches[(size_t)kv.second.batch].off;
    pg.tables_stale = true;
  }
  const size_t cap = loc->nodes.cap & ~(size_t)7;
  if (cap > old) ext_free(pg.free_nodes, (int64_t)old, (int64_t)(cap - old));
  pg.cap_nodes = std::max(cap, old);
  return LSLAM_OK;
}

// The window tables for centre c from the cubes the node holds: per type cell_tree over W x H x D and the TreeViews, in ascending
// window-cell order; CubeGridDev.origin = (W/2, H/2, D/2) - c.  Written into the set of buffers the kernels are not reading.
int pm_write_tables(lslam_loc *loc, const int c[3]) {
  Paged &pg = loc->pg;
  hipStream_t s = loc->stream;
  const int W = loc->W, H = loc->H, D = loc->D;
  const size_t ncell = (size_t)W * H * D;
  const int f = pg.flip ^ 1;
  size_t n_tree[2] = {0, 0};
  int depth = 0;
  for (int t = 0; t < 2; ++t) {
    LOC_TRY(pg.h_cells[f][t].reserve(ncell));
    LOC_TRY(pg.d_cells[f][t].reserve(ncell));
    for (const auto &kv : pg.cubes[t])
      if (!kv.second.staged && kv.second.batch >= 0 && pm_in_window(loc, c, kv.first)) n_tree[t]++;
  }
  LOC_TRY(pg.h_views[f].reserve(n_tree[0] + n_tree[1] + 1));
  LOC_TRY(pg.d_views[f].reserve(n_tree[0] + n_tree[1] + 1));
  size_t at = 0;
  for (int t = 0; t < 2; ++t) {
    loc->tree_cube[t].clear();
    loc->tree_l[t].clear();
    loc->tree_r[t].clear();
    loc->cubes_loaded[t] = 0;
    size_t n_pts = 0;
    int32_t *cells = pg.h_cells[f][t].p;
    for (int k = 0; k < D; ++k)
      for (int j = 0; j < H; ++j)
        for (int i = 0; i < W; ++i) {
          const size_t cell = (size_t)i + (size_t)j * W + (size_t)k * W * H;
          cells[cell] = -1;
          const CubeKey g = {c[0] + i - W / 2, c[1] + j - H / 2, c[2] + k - D / 2};
          const auto it = pg.cubes[t].find(g);
          if (it == pg.cubes[t].end() || it->second.staged) continue;
          const PagedCube &cu = it->second;
          if (cu.len > 0) loc->cubes_loaded[t]++;
          n_pts += (size_t)cu.len;
          if (cu.batch < 0) continue;  // DynamicFeatureMap.h: a cube with fewer than five points is skipped by the match
          cells[cell] = (int32_t)loc->tree_cube[t].size();
          loc->tree_cube[t].push_back((int32_t)cell);
          loc->tree_l[t].push_back((int32_t)cu.off);
          loc->tree_r[t].push_back((int32_t)(cu.off + cu.len));
          pg.h_views[f].p[at++] = cu.view;
          depth = std::max(depth, pg.batches[(size_t)cu.batch].depth);
        }
    loc->view.n[t] = n_pts;
    LOC_TRY(hipMemcpyAsync(pg.d_cells[f][t].p, cells, ncell * sizeof(int32_t), hipMemcpyHostToDevice, s));
  }
  if (at) LOC_TRY(hipMemcpyAsync(pg.d_views[f].p, pg.h_views[f].p, at * sizeof(TreeView), hipMemcpyHostToDevice, s));
  LOC_TRY(hipStreamSynchronize(s));  // (this set of pinned tables is written again two steps from now)
  pg.st.step_host_waits++;
  pg.flip = f;
  FmapView &v = loc->view;
  v.W = W; v.H = H; v.D = D;
  v.origin[0] = W / 2 - c[0]; v.origin[1] = H / 2 - c[1]; v.origin[2] = D / 2 - c[2];
  v.cube_size = loc->cfg_cube;
  v.valid_dist = loc->cfg_valid;
  for (int t = 0; t < 2; ++t) {
    CubeGridDev &g = loc->cg[t];
    g.cube_size = v.cube_size;
    for (int d = 0; d < 3; ++d) g.origin[d] = v.origin[d];
    g.dims[0] = W; g.dims[1] = H; g.dims[2] = D;
    g.cell_tree = pg.d_cells[f][t].p;
    g.trees = pg.d_views[f].p + (t ? n_tree[0] : 0);
  }
  loc->tree_depth = depth;
  loc->grid_valid = false;  // the cell grids are rebuilt from the arena for the new centre (ensure_grids)
  loc->have_map = true;
  pg.tables_stale = false;
  return LSLAM_OK;
}

struct PmEnter {  // a cube that a step (or a staging) brings in
  int t, seg;
  CubeKey g;
  int32_t file;
  size_t first, n_raw;  // its file's points in the upload
  PagedCube cu;
};
struct PmTxn {  // what a step has taken and must give back when it is refused
  std::vector<PmExtent> pts;
  PmExtent nodes = {0, 0};
};

int pm_filter_type(lslam_loc *loc, int t, size_t first, size_t n, int nseg, bool no_wait) {
  Paged &pg = loc->pg;
  hipStream_t s = loc->stream;
  uint32_t *done = pg.done.p + 4 * t;
  size_t m = 0;
  int rc = lslam::voxel_filter_segments(loc->ctx, pg.in_raw.p + first, pg.seg.p + first, n, nseg, loc->map_leaf[t], pg.out[t].p, pg.oseg[t].p, &m,
                                        true, no_wait ? done : nullptr);
  if (rc) return rc;
  if (!no_wait) {
    done[0] = (uint32_t)m;
    done[1] = 0;
  }
  pg.st.step_filter_runs++;
  LOC_TRY(hipMemsetAsync(pg.bounds[t].p, 0, 2 * (size_t)nseg * sizeof(int32_t), s));
  hipLaunchKernelGGL(pm_bounds_kernel, dim3(((unsigned)n + 255) / 256), dim3(256), 0, s, (const int32_t *)pg.oseg[t].p, (const uint32_t *)done, (int)n,
                     nseg, pg.bounds[t].p);
  LOC_TRY(hipGetLastError());
  pg.st.step_kernels++;
  LOC_TRY(hipMemcpyAsync(pg.h_bounds[t].p, pg.bounds[t].p, 2 * (size_t)nseg * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  return LSLAM_OK;
}

int pm_place_type(lslam_loc *loc, int t, size_t n, int nseg) {
  Paged &pg = loc->pg;
  hipLaunchKernelGGL(pm_place_kernel, dim3(((unsigned)n + 255) / 256), dim3(256), 0, loc->stream, (const float4 *)pg.out[t].p,
                     (const int32_t *)pg.oseg[t].p, (const uint32_t *)(pg.done.p + 4 * t), (int)n, nseg, (const int32_t *)pg.bounds[t].p,
                     (const int32_t *)pg.dst[t].p, pg.fpts.p, loc->tpts.p);
  LOC_TRY(hipGetLastError());
  pg.st.step_kernels++;
  return LSLAM_OK;
}

// Bring in the listed cubes of the window centred on c that the node does not hold.  stage: into spare room only -- no table
// changes, nothing leaves.  Otherwise the step: staged cubes of the new window are adopted, the others are read, the cubes
// outside the new window leave, the tables are rewritten.  Nothing live changes before the commit at the end.
int pm_bring_body(lslam_loc *loc, const int c[3], bool stage, PmTxn &txn) {
  Paged &pg = loc->pg;
  hipStream_t s = loc->stream;
  lslam_loc_window_stats &st = pg.st;
  const int W = loc->W, H = loc->H, D = loc->D;
  // 1. who enters
  std::vector<PmEnter> enter;
  int nseg[2] = {0, 0};
  int64_t adopted[2] = {0, 0};
  for (int t = 0; t < 2; ++t)
    for (int k = -D / 2; k <= D / 2; ++k)
      for (int j = -H / 2; j <= H / 2; ++j)
        for (int i = -W / 2; i <= W / 2; ++i) {
          const CubeKey g = {c[0] + i, c[1] + j, c[2] + k};
          const auto li = pg.index[t].find(g);
          if (li == pg.index[t].end()) continue;
          const auto cu = pg.cubes[t].find(g);
          if (cu != pg.cubes[t].end()) {
            if (cu->second.staged && !stage) adopted[t]++;
            continue;
          }
          PmEnter e{};
          e.t = t;
          e.seg = nseg[t]++;
          e.g = g;
          e.file = li->second;
          e.cu.file = li->second;
          e.cu.staged = stage;
          enter.push_back(e);
        }
  // 2. their files, into one pinned block [corner cubes | surf cubes] with the segment of every point
  std::vector<std::vector<float4>> raw(enter.size());
  size_t n_in[2] = {0, 0};
  int64_t files_read = 0, files_missing = 0;
  for (size_t k = 0; k < enter.size(); ++k) {
    std::string err;
    const std::string path = pg.dir + "/" + std::to_string(enter[k].file) + ".pcd";
    if (!lslam::fmap_read_pcd(path.c_str(), raw[k], err)) {  // reference: `if(!file) continue;` -- the cube stays empty
      raw[k].clear();
      files_missing++;
    } else {
      files_read++;
    }
    enter[k].n_raw = raw[k].size();
    n_in[enter[k].t] += raw[k].size();
  }
  const size_t n = n_in[0] + n_in[1];
  if (n > ((size_t)1 << 27)) return invalid("paged window", "too many points in the entering files");
  uint64_t bytes = 0;
  int waits = 0;
  if (n) {
    LOC_TRY(pg.in_pin.reserve(n));
    LOC_TRY(pg.seg_pin.reserve(n));
    LOC_TRY(pg.in_raw.reserve(n));
    LOC_TRY(pg.seg.reserve(n));
    LOC_TRY(pg.done.reserve(8));
    size_t at = 0;
    for (size_t k = 0; k < enter.size(); ++k) {
      enter[k].first = at;
      if (!raw[k].empty()) std::memcpy(pg.in_pin.p + at, raw[k].data(), raw[k].size() * sizeof(float4));
      for (size_t i = 0; i < raw[k].size(); ++i) pg.seg_pin.p[at + i] = enter[k].seg;
      at += raw[k].size();
    }
    LOC_TRY(hipMemcpyAsync(pg.in_raw.p, pg.in_pin.p, n * sizeof(float4), hipMemcpyHostToDevice, s));
    LOC_TRY(hipMemcpyAsync(pg.seg.p, pg.seg_pin.p, n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    bytes += n * (sizeof(float4) + sizeof(int32_t));
    for (int k = 0; k < 8; ++k) pg.done.p[k] = 0;
    // 3. pcl::VoxelGrid of every entering cube, one run per type over all of them; the runs' segment bounds
    for (int t = 0; t < 2; ++t) {
      if (!n_in[t]) continue;
      LOC_TRY(pg.out[t].reserve(n_in[t]));
      LOC_TRY(pg.oseg[t].reserve(n_in[t]));
      LOC_TRY(pg.bounds[t].reserve(2 * (size_t)nseg[t]));
      LOC_TRY(pg.h_bounds[t].reserve(2 * (size_t)nseg[t]));
      LOC_TRY(pg.h_dst[t].reserve((size_t)nseg[t]));
      LOC_TRY(pg.dst[t].reserve((size_t)nseg[t]));
      int rc = pm_filter_type(loc, t, t ? n_in[0] : 0, n_in[t], nseg[t], true);
      if (rc) return rc;
    }
    LOC_TRY(hipStreamSynchronize(s));  // the step's wait: how many points every cube keeps
    waits++;
    for (int t = 0; t < 2; ++t) {
      if (!n_in[t] || !pg.done.p[4 * t + 1]) continue;
      // the filter's wide key did not hold a voxel extent: this type once more, with the filter measuring it (waits inside)
      int rc = pm_filter_type(loc, t, t ? n_in[0] : 0, n_in[t], nseg[t], false);
      if (rc) return rc;
      LOC_TRY(hipStreamSynchronize(s));
      waits += 2;
    }
  }
  // 4. room: the counts against the capacity, then an extent per cube
  size_t n_new[2] = {0, 0};
  for (PmEnter &e : enter) {
    if (!e.n_raw) continue;
    const int32_t *hb = pg.h_bounds[e.t].p;
    e.cu.len = hb[2 * e.seg + 1] - hb[2 * e.seg];
    n_new[e.t] += (size_t)e.cu.len;
  }
  if (pg.limit)
    for (int t = 0; t < 2; ++t)
      if (pg.used[t] + n_new[t] > pg.limit) {
        if (!stage) pm_drop_staged(loc, c);  // staged cubes the window does not reach make room
        if (pg.used[t] + n_new[t] > pg.limit) {
          char b[200];
          std::snprintf(b, sizeof(b), "%zu + %zu %s points exceed the capacity of %zu per type (lslam_pmap_setup_capacity)", pg.used[t],
                        n_new[t], t ? "surf" : "corner", pg.limit);
          return invalid(stage ? "lslam_pmap_stage" : "paged window step", b);
        }
      }
  for (PmEnter &e : enter) {
    if (e.cu.len <= 0) continue;
    if (!ext_alloc(pg.free_pts, e.cu.len, &e.cu.off)) {
      // (the arena at least doubles, and holds everything held and entering even if its free room were all fragments)
      int rc = pm_grow_points(loc, std::max(2 * pg.cap_pts, pg.cap_pts + n_new[0] + n_new[1] + 1024));
      if (rc) return rc;
      if (!ext_alloc(pg.free_pts, e.cu.len, &e.cu.off)) return invalid("paged window", "no room in the point arena");
    }
    txn.pts.push_back(PmExtent{e.cu.off, e.cu.len});
  }
  // 5. placement
  std::vector<int32_t> roots_lr;
  std::vector<size_t> root_of;
  int64_t n_total = 0;
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < nseg[t]; ++k)
      if (n_in[t]) pg.h_dst[t].p[k] = -1;
  for (size_t k = 0; k < enter.size(); ++k) {
    const PmEnter &e = enter[k];
    if (e.cu.len <= 0) continue;
    pg.h_dst[e.t].p[e.seg] = (int32_t)e.cu.off;
    if (e.cu.len >= 5) {
      roots_lr.push_back((int32_t)e.cu.off);
      roots_lr.push_back((int32_t)(e.cu.off + e.cu.len));
      root_of.push_back(k);
      n_total = std::max(n_total, e.cu.off + e.cu.len);
    }
  }
  for (int t = 0; t < 2; ++t) {
    if (!n_new[t]) continue;
    LOC_TRY(hipMemcpyAsync(pg.dst[t].p, pg.h_dst[t].p, (size_t)nseg[t] * sizeof(int32_t), hipMemcpyHostToDevice, s));
    bytes += (size_t)nseg[t] * sizeof(int32_t);
    int rc = pm_place_type(loc, t, n_in[t], nseg[t]);
    if (rc) return rc;
  }
  // 6. ONE forest build over the entering cubes, into a node extent of its own
  const int T = (int)root_of.size();
  int batch = -1, forest_builds = 0;
  NodeBatch nb{};
  if (T > 0) {
    std::vector<TreeView> views((size_t)T);
    size_t n_root_pts = 0;
    for (int r = 0; r < T; ++r) n_root_pts += (size_t)(roots_lr[2 * (size_t)r + 1] - roots_lr[2 * (size_t)r]);
    int max_depth = 0, fallback = 0;
    size_t n_leaves = 0;
    for (int attempt = 0; attempt < 3; ++attempt) {
      // (generous at once: a step waits for its build, a second build costs more than the room, and what the trees do not use goes back below)
      const size_t mult[3] = {6, 12, 24};
      const size_t cap = ((mult[attempt] * n_root_pts / 3 + 64 + 8 * (size_t)T) + 7) & ~(size_t)7;
      if (txn.nodes.len) {
        ext_free(pg.free_nodes, txn.nodes.off, txn.nodes.len);
        txn.nodes = PmExtent{0, 0};
      }
      int64_t off = 0;
      if (!ext_alloc(pg.free_nodes, (int64_t)cap, &off)) {
        int rc = pm_grow_nodes(loc, std::max(2 * pg.cap_nodes, pg.cap_nodes + cap + 1024));
        if (rc) return rc;
        if (!ext_alloc(pg.free_nodes, (int64_t)cap, &off)) return invalid("paged window", "no room in the node arena");
      }
      txn.nodes = PmExtent{off, (int64_t)cap};
      if (attempt > 0)  // the failed attempt permuted the points
        for (int t = 0; t < 2; ++t)
          if (n_new[t]) {
            int rc = pm_place_type(loc, t, n_in[t], nseg[t]);
            if (rc) return rc;
          }
      LOC_TRY(lslam::build_kdforest_device(lslam::ctx_build_pool(loc->ctx, 0), loc->tpts.p, (int32_t)n_total, roots_lr.data(), T, loc->nodes.p + off,
                                           nullptr, (int32_t)cap, s, views.data(), &max_depth, &n_leaves, &fallback));
      forest_builds++;
      waits++;
      if (fallback != 1) break;
    }
    if (fallback) {
      lslam::set_error("paged window: the device cube-tree build hit a structure limit");
      return fallback == 1 || fallback == 2 ? LSLAM_ERR_TREE_BUILD : LSLAM_ERR_TREE_DEPTH;
    }
    if (max_depth > KD_STACK_LDS + 1) {
      lslam::set_error("paged window: a cube tree is deeper than the device traversal stack");
      return LSLAM_ERR_TREE_DEPTH;
    }
    const int64_t n_used = std::max<int64_t>(8, ((int64_t)views[0].n_nodes + 7) & ~(int64_t)7);  // node groups the build took, all trees together
    if (n_used < txn.nodes.len) {
      ext_free(pg.free_nodes, txn.nodes.off + n_used, txn.nodes.len - n_used);
      txn.nodes.len = n_used;
    }
    nb.off = txn.nodes.off;
    nb.cap = txn.nodes.len;
    nb.refs = T;
    nb.depth = max_depth;
    batch = (int)pg.batches.size();
    for (int r = 0; r < T; ++r) {
      enter[root_of[(size_t)r]].cu.view = views[(size_t)r];
      enter[root_of[(size_t)r]].cu.batch = batch;
    }
  }
  // 7. the commit
  if (T > 0) {
    pg.batches.push_back(nb);
    pg.nodes_used += (size_t)nb.cap;
  }
  txn = PmTxn{};
  int64_t entered[2] = {0, 0}, left[2] = {0, 0};
  for (const PmEnter &e : enter) {
    pg.cubes[e.t][e.g] = e.cu;
    pg.used[e.t] += (size_t)e.cu.len;
    entered[e.t]++;
  }
  st.files_read_total += files_read;
  st.files_missing_total += files_missing;
  st.trees_built_total += T;
  st.forest_builds_total += forest_builds;
  st.bytes_uploaded_total += bytes;
  if (stage) return LSLAM_OK;
  for (int t = 0; t < 2; ++t)
    for (auto it = pg.cubes[t].begin(); it != pg.cubes[t].end();) {
      if (pm_in_window(loc, c, it->first)) {
        it->second.staged = false;
        ++it;
      } else if (!it->second.staged) {
        pm_release_cube(loc, t, it->second);
        left[t]++;
        it = pg.cubes[t].erase(it);
      } else {
        ++it;
      }
    }
  for (int t = 0; t < 2; ++t) {
    st.entered[t] = entered[t] + adopted[t];
    st.adopted[t] = adopted[t];
    st.left[t] = left[t];
    st.entered_total[t] += entered[t] + adopted[t];
    st.adopted_total[t] += adopted[t];
    st.left_total[t] += left[t];
  }
  st.files_read = files_read;
  st.files_missing = files_missing;
  st.trees_built = T;
  st.bytes_uploaded = bytes;
  st.step_forest_builds = forest_builds;
  st.step_host_waits = waits;
  st.steps++;
  for (int d = 0; d < 3; ++d) pg.centre[d] = c[d];
  pg.have_window = true;
  return pm_write_tables(loc, c);
}

int pm_bring(lslam_loc *loc, const int c[3], bool stage) {
  Paged &pg = loc->pg;
  const lslam_loc_window_stats last = pg.st;  // (a staging leaves the last step's counters as they are)
  pg.st.step_kernels = pg.st.step_filter_runs = pg.st.step_forest_builds = pg.st.step_host_waits = 0;
  PmTxn txn;
  const int rc = pm_bring_body(loc, c, stage, txn);
  if (stage) {
    pg.st.step_kernels = last.step_kernels;
    pg.st.step_filter_runs = last.step_filter_runs;
    pg.st.step_forest_builds = last.step_forest_builds;
    pg.st.step_host_waits = last.step_host_waits;
  }
  if (rc == LSLAM_OK) {
    // (a staging that moved an arena: the same tables once more, pointing into the new one)
    if (stage && pg.tables_stale && pg.have_window) return pm_write_tables(loc, pg.centre);
    return rc;
  }
  // refused: what the step took goes back, and the node answers the next call as it did before
  (void)hipStreamSynchronize(loc->stream);
  for (const PmExtent &x : txn.pts) ext_free(pg.free_pts, x.off, x.len);
  ext_free(pg.free_nodes, txn.nodes.off, txn.nodes.len);
  if (!stage) pg.st.refused_steps++;
  if (pg.tables_stale && pg.have_window) {  // an arena moved before the refusal: the old window's tables, for where it is now
    const std::string msg = lslam_last_error();
    (void)pm_write_tables(loc, pg.centre);
    lslam::set_error(msg.c_str());
  }
  return rc;
}

// computeActiveAera + InVerticalFov (DynamicFeatureMap.h:748-804): the offsets within ws cubes, loops i, j, k, that are listed
// and -- the centre apart -- have one of their eight corners within the valid distance of the sensor's fractional position
void pm_active_area(lslam_loc *loc, const float pos[3]) {
  Paged &pg = loc->pg;
  pg.active.clear();
  const float cs = loc->cfg_cube, valid = loc->cfg_valid;
  const int *c = pg.centre;
  const double real[3] = {(double)(pos[0] / cs - (float)c[0]), (double)(pos[1] / cs - (float)c[1]), (double)(pos[2] / cs - (float)c[2])};
  const int ws = (int)std::ceil(valid / cs);
  const double d[2] = {-0.5, 0.5};
  for (int i = -ws; i <= ws; ++i)
    for (int j = -ws; j <= ws; ++j)
      for (int k = -ws; k <= ws; ++k) {
        const CubeKey g = {c[0] + i, c[1] + j, c[2] + k};
        if (!pg.index[0].count(g) && !pg.index[1].count(g)) continue;
        bool in = !i && !j && !k;
        if (!in) {
          double min_dis = -1.0;
          for (int dx = 0; dx < 2; ++dx)
            for (int dy = 0; dy < 2; ++dy)
              for (int dz = 0; dz < 2; ++dz) {
                const double x = i + d[dx] - real[0], y = j + d[dy] - real[1], z = k + d[dz] - real[2];
                const double dis = std::sqrt(std::pow(x * cs, 2) + std::pow(y * cs, 2) + std::pow(z * cs, 2));
                min_dis = min_dis == -1.0 ? dis : std::min(min_dis, dis);
              }
          in = !(min_dis > (double)valid);
        }
        if (in) pg.active.push_back(g);
      }
  pg.st.active_cubes = pg.active.size();
}

// DynamicFeatureMap::update
int pm_update(lslam_loc *loc, const float pos[3]) {
  Paged &pg = loc->pg;
  int c[3];
  for (int d = 0; d < 3; ++d) {
    if (!std::isfinite(pos[d])) return invalid("paged window", "the sensor position is not finite");
    c[d] = (int)std::round(pos[d] / loc->cfg_cube);  // Glo2GloIdx: a float quotient
  }
  if (!pg.have_window || c[0] != pg.centre[0] || c[1] != pg.centre[1] || c[2] != pg.centre[2]) {
    const int rc = pm_bring(loc, c, false);
    if (rc) return rc;
  }
  pm_active_area(loc, pos);
  return LSLAM_OK;
}

int pm_surround(lslam_loc *loc, const char *fn, float *corner_xyzi, size_t cap_corner, size_t *n_corner, float *surf_xyzi, size_t cap_surf,
                size_t *n_surf) {
  Paged &pg = loc->pg;
  size_t cnt[2] = {0, 0};
  for (int t = 0; t < 2; ++t)
    for (const CubeKey &g : pg.active) {
      const auto it = pg.cubes[t].find(g);
      if (it != pg.cubes[t].end() && !it->second.staged) cnt[t] += (size_t)it->second.len;
    }
  *n_corner = cnt[0];
  *n_surf = cnt[1];
  if (!corner_xyzi && !surf_xyzi) return LSLAM_OK;
  if ((corner_xyzi && cap_corner < cnt[0]) || (surf_xyzi && cap_surf < cnt[1]) || !corner_xyzi || !surf_xyzi)
    return invalid(fn, "both buffers are needed, each with room for its cloud");
  float *out[2] = {corner_xyzi, surf_xyzi};
  for (int t = 0; t < 2; ++t) {
    size_t at = 0;
    for (const CubeKey &g : pg.active) {
      const auto it = pg.cubes[t].find(g);
      if (it == pg.cubes[t].end() || it->second.staged || it->second.len <= 0) continue;
      LOC_TRY(hipMemcpyAsync(out[t] + 4 * at, pg.fpts.p + it->second.off, (size_t)it->second.len * sizeof(float4), hipMemcpyDeviceToHost, loc->stream));
      at += (size_t)it->second.len;
    }
  }
  LOC_TRY(hipStreamSynchronize(loc->stream));
  return LSLAM_OK;
}

int paged_only(lslam_loc *loc, const char *fn) {
  int rc = check_loc(loc, fn);
  if (rc) return rc;
  if (!loc->pg.on) return invalid(fn, "the node is not in the paged mode (lslam_pmap_open)");
  return LSLAM_OK;
}
void pm_leave(lslam_loc *loc) {  // a static map replaces the window: the arenas' memory is the static structures' again
  if (!loc->pg.on) return;
  (void)hipStreamSynchronize(loc->stream);
  pm_reset(loc);
  loc->pg.cap_pts = loc->pg.cap_nodes = 0;
  loc->pg.free_pts.clear();
  loc->pg.free_nodes.clear();
  loc->pg.on = false;
  loc->have_map = false;
}

int process_impl(lslam_loc *loc, const char *fn, const void *corner, size_t n_corner, const void *surf, size_t n_surf,
                 size_t stride_bytes, bool from_device, const float odom[16], int64_t stamp_ns, float mapped_out[16],
                 float velocity_out[3], int32_t *flags, lslam_stats *stats) {
  if (flags) *flags = 0;
  int rc = check_loc(loc, fn);
  if (rc) return rc;
  if (!odom || !flags || (n_corner && !corner) || (n_surf && !surf) || (!from_device && (stride_bytes < 12 || (stride_bytes & 3))))
    return invalid(fn, "bad arguments");
  if (!loc->initialized) {  // LaserLocalization.cpp:169: nothing happens before the initial pose
    *flags = LSLAM_LOC_DROPPED;
    return LSLAM_OK;
  }
  if (!loc->pg.on && !loc->have_map) {
    lslam::set_error("localisation node: no map (lslam_loc_load / _set_map / _set_map_from_fmap)");
    return LSLAM_ERR_NO_MAP;
  }
  // transformMerge (LaserMatcher.cpp:333-340)
  float Wnew[16];
  lslam_transform_associate(loc->odom_last, odom, loc->mapped_last, Wnew);
  bool at_edge = false;
  if (loc->pg.on) {
    // LaserMatcher.cpp:310-316: the window follows the merged prior (with a pose pending too: the quirk is kept); no edge here
    const float pos[3] = {Wnew[3], Wnew[7], Wnew[11]};
    rc = pm_update(loc, pos);
    if (rc) return rc;
  } else {
    const float pos[3] = {Wnew[3], Wnew[7], Wnew[11]};
    int g[3];
    cube_of(loc, pos, g);
    const int lim[3] = {loc->view.W, loc->view.H, loc->view.D};
    for (int d = 0; d < 3; ++d) at_edge = at_edge || g[d] < 3 || g[d] > lim[d] - 4;
  }
  // (with a pose pending the sweep's match result is discarded anyway: such a sweep is not matched and only takes the pose,
  // which is how a node that was sent to the edge is brought back)
  if (at_edge && !loc->reset_pending)
    return invalid(fn, "the sensor is within 3 cubes of the cube grid's edge: the reference would shift its cube array under its "
                       "kd-trees (FeatureMap.h:232-254,353-376); refused, the node is unchanged");
  float pose[6];
  lslam_isometry_to_pose(Wnew, pose);
  begin_sweep_counts(loc);
  int32_t fl = 0;
  int status = LSLAM_OK;
  if (at_edge) {
    if (stats) std::memset(stats, 0, sizeof(*stats));
  } else {
    status = match_impl(loc, corner, n_corner, surf, n_surf, stride_bytes, from_device, pose, stats, false, &fl);
  }
  end_sweep_counts(loc);
  if (status < 0) return status;
  float T[16];
  lslam_pose_to_isometry(pose, T);
  // transformUpdate (LaserLocalization.cpp:140-166): a pending pose replaces the match result AFTER the match
  if (loc->reset_pending) {
    std::memcpy(T, loc->reset_pose, sizeof(T));
    loc->reset_pending = false;
    fl |= LSLAM_LOC_POSE_RESET;
  }
  std::memcpy(loc->mapped_last, T, sizeof(T));
  std::memcpy(loc->odom_last, odom, sizeof(T));
  loc->velocity[0] = loc->velocity[1] = loc->velocity[2] = 0.0f;
  if (loc->stamp_last != 0) {  // !_timeLaserOdometryLast.is_zero()
    const float dt = (float)((double)(stamp_ns - loc->stamp_last) * 1e-9);  // ros::Duration::toSec(), then Eigen's float division
    float v[3] = {(T[3] - loc->pose_last[3]) / dt, (T[7] - loc->pose_last[7]) / dt, (T[11] - loc->pose_last[11]) / dt};
    const float norm = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (norm > 30.0f) {
      v[0] = v[1] = v[2] = 0.0f;
      fl |= LSLAM_LOC_VELOCITY_ZEROED;
    }
    std::memcpy(loc->velocity, v, sizeof(v));
    fl |= LSLAM_LOC_HAS_VELOCITY;
  }
  std::memcpy(loc->pose_last, T, sizeof(T));
  loc->stamp_last = stamp_ns;
  if (mapped_out) std::memcpy(mapped_out, T, sizeof(T));
  if (velocity_out) std::memcpy(velocity_out, loc->velocity, sizeof(loc->velocity));
  *flags = fl;
  return status;
}

}  // namespace

extern "C" {

int lslam_loc_create(lslam_ctx *ctx, int32_t w, int32_t h, int32_t d, lslam_loc **out) {
  if (out) *out = nullptr;
  if (!ctx) return invalid("lslam_loc_create", "null ctx");
  if (!out || w <= 0 || h <= 0 || d <= 0) return invalid("lslam_loc_create", "bad arguments");
  lslam_fmap *fm = nullptr;
  int rc = lslam_fmap_create(ctx, w, h, d, &fm);
  if (rc) return rc;
  lslam::fmap_set_private(fm);
  lslam_loc *loc = new lslam_loc();
  loc->ctx = ctx;
  loc->stream = lslam::ctx_stream(ctx);
  loc->fm = fm;
  loc->W = w; loc->H = h; loc->D = d;
  identity16(loc->reset_pose);
  identity16(loc->mapped_last);
  identity16(loc->odom_last);
  identity16(loc->pose_last);
  lslam_fmap_setup_filter_size(fm, loc->map_leaf[0], loc->map_leaf[1], 0.6f);
  *out = loc;
  return LSLAM_OK;
}

void lslam_loc_destroy(lslam_loc *loc) {
  if (!loc) return;
  if (lslam::ctx_alive(loc->ctx)) {  // a node may outlive its ctx; its stream is then gone
    (void)hipSetDevice(lslam::ctx_device(loc->ctx));
    (void)hipStreamSynchronize(loc->stream);
  }
  lslam_fmap_destroy(loc->fm);
  delete loc;
}

int lslam_loc_setup_scan_filter_size(lslam_loc *loc, float corner, float surf) {
  int rc = check_loc(loc, "lslam_loc_setup_scan_filter_size");
  if (rc) return rc;
  if (!(corner > 0.f) || !(surf > 0.f)) return invalid("lslam_loc_setup_scan_filter_size", "a leaf must be positive");
  loc->scan_leaf[0] = corner;
  loc->scan_leaf[1] = surf;
  return LSLAM_OK;
}
int lslam_loc_setup_map_filter_size(lslam_loc *loc, float corner, float surf) {
  int rc = check_loc(loc, "lslam_loc_setup_map_filter_size");
  if (rc) return rc;
  if (!(corner > 0.f) || !(surf > 0.f)) return invalid("lslam_loc_setup_map_filter_size", "a leaf must be positive");
  if (loc->pg.on) return invalid("lslam_loc_setup_map_filter_size", "set before lslam_pmap_open: the window's cubes were filtered with the old leaves");
  loc->map_leaf[0] = corner;
  loc->map_leaf[1] = surf;
  return lslam_fmap_setup_filter_size(loc->fm, corner, surf, 0.6f);
}
int lslam_loc_setup_world_origin(lslam_loc *loc, int32_t ox, int32_t oy, int32_t oz) {
  int rc = check_loc(loc, "lslam_loc_setup_world_origin");
  if (rc) return rc;
  if (loc->pg.on) return invalid("lslam_loc_setup_world_origin", "the paged window is addressed by global cube index: it has no origin to set");
  loc->have_map = false;  // the cubes of a map that is there were cut with the old origin
  return lslam_fmap_setup_world_origin(loc->fm, ox, oy, oz);
}
int lslam_loc_setup_world_cube_size(lslam_loc *loc, float size) {
  int rc = check_loc(loc, "lslam_loc_setup_world_cube_size");
  if (rc) return rc;
  if (!(size > 0.f)) return invalid("lslam_loc_setup_world_cube_size", "the cube size must be positive");
  if (loc->pg.on) return invalid("lslam_loc_setup_world_cube_size", "set before lslam_pmap_open: the index is in cubes of the old size");
  loc->cfg_cube = size;
  loc->have_map = false;
  return lslam_fmap_setup_world_cube_size(loc->fm, size);
}
int lslam_loc_setup_lidar_valid_distance(lslam_loc *loc, float dist) {
  int rc = check_loc(loc, "lslam_loc_setup_lidar_valid_distance");
  if (rc) return rc;
  if (loc->pg.on && (!(dist >= 0.f) || (int)std::ceil(dist / loc->cfg_cube) > std::min(loc->W, std::min(loc->H, loc->D)) / 2))
    return invalid("lslam_loc_setup_lidar_valid_distance", "the active area would reach beyond the paged window");
  loc->cfg_valid = dist;
  loc->view.valid_dist = dist;
  loc->grid_valid = false;
  return lslam_fmap_setup_lidar_valid_distance(loc->fm, dist);
}
int lslam_loc_setup_search(lslam_loc *loc, int32_t use_grid) {
  int rc = check_loc(loc, "lslam_loc_setup_search");
  if (rc) return rc;
  loc->use_grid = use_grid != 0;
  return LSLAM_OK;
}

int lslam_loc_load(lslam_loc *loc, const char *directory) {
  int rc = check_loc(loc, "lslam_loc_load");
  if (rc) return rc;
  if (!directory) return invalid("lslam_loc_load", "null directory");
  pm_leave(loc);
  loc->have_map = false;
  rc = lslam::fmap_clear(loc->fm);
  if (rc) return rc;
  rc = lslam_fmap_load(loc->fm, directory);
  if (rc) return rc;
  set_grid_cells(loc, true);
  return install(loc);
}

int lslam_loc_set_map(lslam_loc *loc, const void *corner, size_t n_corner, const void *surf, size_t n_surf, size_t stride_bytes,
                      int32_t filter) {
  int rc = check_loc(loc, "lslam_loc_set_map");
  if (rc) return rc;
  if ((n_corner && !corner) || (n_surf && !surf) || stride_bytes < 12 || (stride_bytes & 3)) return invalid("lslam_loc_set_map", "bad arguments");
  pm_leave(loc);
  loc->have_map = false;
  rc = lslam::fmap_set_clouds(loc->fm, corner, n_corner, surf, n_surf, stride_bytes, filter != 0);
  if (rc) return rc;
  set_grid_cells(loc, filter != 0);
  return install(loc);
}

int lslam_loc_set_map_from_fmap(lslam_loc *loc, lslam_fmap *fm) {
  int rc = check_loc(loc, "lslam_loc_set_map_from_fmap");
  if (rc) return rc;
  if (!fm) return invalid("lslam_loc_set_map_from_fmap", "null feature map");
  pm_leave(loc);
  loc->have_map = false;
  rc = lslam::fmap_copy(loc->fm, fm);
  if (rc) return rc;
  {  // cube size and valid distance are the adopted map's
    FmapView v{};
    if (lslam::fmap_view(loc->fm, &v) == LSLAM_OK) {
      loc->cfg_cube = v.cube_size;
      loc->cfg_valid = v.valid_dist;
    }
  }
  lslam_fmap_setup_filter_size(loc->fm, loc->map_leaf[0], loc->map_leaf[1], 0.6f);
  set_grid_cells(loc, false);
  return install(loc);
}

int lslam_loc_info(lslam_loc *loc, lslam_loc_map_stats *out) {
  if (out) std::memset(out, 0, sizeof(*out));
  int rc = check_loc(loc, "lslam_loc_info");
  if (rc) return rc;
  if (!out) return invalid("lslam_loc_info", "null output");
  for (int t = 0; t < 2; ++t) {
    out->cubes_loaded[t] = loc->have_map ? loc->cubes_loaded[t] : 0;
    out->cubes_with_tree[t] = loc->have_map ? (int64_t)loc->tree_cube[t].size() : 0;
    out->n_points[t] = loc->have_map ? loc->view.n[t] : 0;
    out->grid_on[t] = loc->have_map && loc->grid_valid && loc->grid[t].view.cell_start ? 1 : 0;
  }
  out->structure_builds = loc->structure_builds;
  out->grid_builds = loc->grid_builds;
  for (int d = 0; d < 3; ++d) out->grid_cube[d] = loc->grid_cube[d];
  out->grid_reach = loc->grid_reach;
  out->tree_depth = loc->tree_depth;
  return LSLAM_OK;
}

int lslam_loc_set_initial_pose(lslam_loc *loc, const float T[16]) {
  int rc = check_loc(loc, "lslam_loc_set_initial_pose");
  if (rc) return rc;
  if (!T) return invalid("lslam_loc_set_initial_pose", "null pose");
  std::memcpy(loc->reset_pose, T, sizeof(loc->reset_pose));
  loc->reset_pending = true;
  loc->initialized = true;
  return LSLAM_OK;
}

int lslam_loc_process(lslam_loc *loc, const void *corner, size_t n_corner, const void *surf, size_t n_surf, size_t stride_bytes,
                      const float odom[16], int64_t stamp_ns, float mapped_out[16], float velocity_out[3], int32_t *flags,
                      lslam_stats *stats) {
  const int rc = process_impl(loc, "lslam_loc_process", corner, n_corner, surf, n_surf, stride_bytes, false, odom, stamp_ns, mapped_out,
                              velocity_out, flags, stats);
  if (rc < 0 && loc && lslam::ctx_alive(loc->ctx)) (void)hipStreamSynchronize(loc->stream);  // (the staging is the next call's too)
  return rc;
}

int lslam_loc_process_device(lslam_loc *loc, const void *d_corner, size_t n_corner, const void *d_surf, size_t n_surf,
                             const float odom[16], int64_t stamp_ns, float mapped_out[16], float velocity_out[3], int32_t *flags,
                             lslam_stats *stats) {
  const int rc = process_impl(loc, "lslam_loc_process_device", d_corner, n_corner, d_surf, n_surf, 16, true, odom, stamp_ns, mapped_out,
                              velocity_out, flags, stats);
  if (rc < 0 && loc && lslam::ctx_alive(loc->ctx)) (void)hipStreamSynchronize(loc->stream);
  return rc;
}

int lslam_loc_match(lslam_loc *loc, const void *corner, size_t n_corner, const void *surf, size_t n_surf, size_t stride_bytes,
                    float pose[6], lslam_stats *stats) {
  int rc = check_loc(loc, "lslam_loc_match");
  if (rc) return rc;
  if (!pose || (n_corner && !corner) || (n_surf && !surf) || stride_bytes < 12 || (stride_bytes & 3)) return invalid("lslam_loc_match", "bad arguments");
  if (loc->pg.on) {
    const float pos[3] = {pose[3], pose[4], pose[5]};
    rc = pm_update(loc, pos);
    if (rc) return rc;
  }
  if (!loc->have_map) {
    lslam::set_error("localisation node: no map (lslam_loc_load / _set_map / _set_map_from_fmap)");
    return LSLAM_ERR_NO_MAP;
  }
  begin_sweep_counts(loc);
  rc = match_impl(loc, corner, n_corner, surf, n_surf, stride_bytes, false, pose, stats, false, nullptr);
  end_sweep_counts(loc);
  if (rc < 0) (void)hipStreamSynchronize(loc->stream);
  return rc;
}

int lslam_loc_get_surround(lslam_loc *loc, float *corner_xyzi, size_t cap_corner, size_t *n_corner, float *surf_xyzi,
                           size_t cap_surf, size_t *n_surf) {
  if (n_corner) *n_corner = 0;
  if (n_surf) *n_surf = 0;
  int rc = check_loc(loc, "lslam_loc_get_surround");
  if (rc) return rc;
  if (!n_corner || !n_surf) return invalid("lslam_loc_get_surround", "null count outputs");
  if (loc->pg.on) {
    const float at[3] = {loc->mapped_last[3], loc->mapped_last[7], loc->mapped_last[11]};
    rc = pm_update(loc, at);
    if (rc) return rc;
    return pm_surround(loc, "lslam_loc_get_surround", corner_xyzi, cap_corner, n_corner, surf_xyzi, cap_surf, n_surf);
  }
  if (!loc->have_map) {
    lslam::set_error("localisation node: no map (lslam_loc_load / _set_map / _set_map_from_fmap)");
    return LSLAM_ERR_NO_MAP;
  }
  const float pos[3] = {loc->mapped_last[3], loc->mapped_last[7], loc->mapped_last[11]};
  int g[3];
  cube_of(loc, pos, g);
  const int lim[3] = {loc->view.W, loc->view.H, loc->view.D};
  for (int d = 0; d < 3; ++d)
    if (g[d] < 3 || g[d] > lim[d] - 4) return invalid("lslam_loc_get_surround", "the sensor is within 3 cubes of the cube grid's edge (FeatureMap::update would shift the map)");
  rc = lslam_fmap_update(loc->fm, pos);  // no shift: the store's arrays and the trees built from them stay as they are
  if (rc) return rc;
  size_t nc = 0, ns = 0;
  rc = lslam_fmap_surround_counts(loc->fm, &nc, &ns);
  if (rc) return rc;
  *n_corner = nc;
  *n_surf = ns;
  if (!corner_xyzi && !surf_xyzi) return LSLAM_OK;
  if ((corner_xyzi && cap_corner < nc) || (surf_xyzi && cap_surf < ns) || !corner_xyzi || !surf_xyzi)
    return invalid("lslam_loc_get_surround", "both buffers are needed, each with room for its cloud");
  return lslam_fmap_get_surround(loc->fm, corner_xyzi, cap_corner, surf_xyzi, cap_surf);
}

int lslam_loc_search_stats(lslam_loc *loc, lslam_loc_search_counts *out) {
  if (out) std::memset(out, 0, sizeof(*out));
  int rc = check_loc(loc, "lslam_loc_search_stats");
  if (rc) return rc;
  if (!out) return invalid("lslam_loc_search_stats", "null output");
  *out = loc->cnt;
  return LSLAM_OK;
}

int lslam_loc_debug_knn5(lslam_loc *loc, int32_t which, const void *queries, size_t nq, size_t stride_bytes, float *xyz_out,
                         float *d2_out, uint8_t *how_out) {
  int rc = check_loc(loc, "lslam_loc_debug_knn5");
  if (rc) return rc;
  if ((which != 0 && which != 1) || (nq && (!queries || !xyz_out || !d2_out || !how_out)) || stride_bytes < 12 || (stride_bytes & 3) ||
      nq > ((size_t)1 << 26))
    return invalid("lslam_loc_debug_knn5", "bad arguments");
  if (!loc->have_map) {
    lslam::set_error("localisation node: no map (lslam_loc_load / _set_map / _set_map_from_fmap)");
    return LSLAM_ERR_NO_MAP;
  }
  if (nq == 0) return LSLAM_OK;
  hipStream_t s = loc->stream;
  const int nb = (int)((nq + LOC_BLOCK - 1) / LOC_BLOCK);
  rc = reserve_search(loc, nb);
  if (rc) return rc;
  std::vector<float4> h(nq);
  const char *p = static_cast<const char *>(queries);
  for (size_t i = 0; i < nq; ++i) {
    float v[3];
    std::memcpy(v, p + i * stride_bytes, 12);
    h[i] = make_float4(v[0], v[1], v[2], 0.0f);
  }
  if (!loc->grid_valid) {  // no sweep has said where the sensor is yet: the grids go around the first query
    const float pos[3] = {h[0].x, h[0].y, h[0].z};
    int g[3];
    cube_of(loc, pos, g);
    if (loc->pg.on) {  // the window's grids go around its centre, as a sweep's do
      g[0] = loc->W / 2; g[1] = loc->H / 2; g[2] = loc->D / 2;
    }
    rc = ensure_grids(loc, g);
    if (rc) return rc;
  }
  LOC_TRY(loc->in_raw.reserve(nq));
  LOC_TRY(hipMemcpyAsync(loc->in_raw.p, h.data(), nq * sizeof(float4), hipMemcpyHostToDevice, s));
  const int32_t counts[4] = {0, which ? 0 : (int32_t)nq, 0, which ? (int32_t)nq : 0};
  LOC_TRY(hipMemcpyAsync(loc->counts.p, counts, sizeof(counts), hipMemcpyHostToDevice, s));
  LOC_TRY(hipMemsetAsync(loc->ctr.p, 0, (LOC_MAX_ITER + 2) * sizeof(int32_t), s));
  LOC_TRY(hipMemsetAsync(loc->stat.p, 0, ST_N * sizeof(unsigned long long), s));
  GNState &st = *loc->h_state.p;
  std::memset(&st, 0, sizeof(st));
  const float zero[6] = {0, 0, 0, 0, 0, 0};
  struct HostSinCos {
    void operator()(float a, float &sn, float &cs) const { sn = std::sin(a); cs = std::cos(a); }
  };
  pose_to_Rt_sc(zero, st.R, st.t, st.sc, HostSinCos());  // the identity: sel = q, bit for bit
  LOC_TRY(hipMemcpyAsync(loc->d_state.p, &st, sizeof(GNState), hipMemcpyHostToDevice, s));
  LocArgs a;
  fill_args(loc, a, which ? 0 : nb, which ? nb : 0, 1);
  a.q[0] = a.q[1] = loc->in_raw.p;
  a.list_cnt = loc->ctr.p;
  launch_search(a, s);
  DevBuf<float> d_xyz, d_d2;
  DevBuf<uint8_t> d_how;
  LOC_TRY(d_xyz.reserve(nq * 15));
  LOC_TRY(d_d2.reserve(nq * 5));
  LOC_TRY(d_how.reserve(nq));
  hipLaunchKernelGGL(loc_tap_out_kernel, dim3(((unsigned)nq + 255) / 256), dim3(256), 0, s, a, (int)which, (int)nq, d_xyz.p, d_d2.p, d_how.p);
  LOC_TRY(hipGetLastError());
  LOC_TRY(hipMemcpyAsync(xyz_out, d_xyz.p, nq * 15 * sizeof(float), hipMemcpyDeviceToHost, s));
  LOC_TRY(hipMemcpyAsync(d2_out, d_d2.p, nq * 5 * sizeof(float), hipMemcpyDeviceToHost, s));
  LOC_TRY(hipMemcpyAsync(how_out, d_how.p, nq, hipMemcpyDeviceToHost, s));
  LOC_TRY(hipStreamSynchronize(s));
  return LSLAM_OK;
}

// ---- the paged mode --------------------------------------------------------------------------------------------------------
int lslam_pmap_open(lslam_loc *loc, const char *directory) {
  int rc = check_loc(loc, "lslam_pmap_open");
  if (rc) return rc;
  if (!directory) return invalid("lslam_pmap_open", "null directory");
  if (!(loc->W & 1) || !(loc->H & 1) || !(loc->D & 1))
    return invalid("lslam_pmap_open", "an even window dimension: the window has no centre cube (the reference would index out of range)");
  if (!(loc->cfg_valid >= 0.f) || (int)std::ceil(loc->cfg_valid / loc->cfg_cube) > std::min(loc->W, std::min(loc->H, loc->D)) / 2)
    return invalid("lslam_pmap_open", "ceil(valid distance / cube size) exceeds half the smallest window dimension: the active area would "
                                           "reach beyond the window");
  const std::string dir(directory);
  std::ifstream fin(dir + "/index2.txt");
  if (!fin) {
    lslam::set_error("no index2.txt in the directory");
    return LSLAM_ERR_INVALID;  // the reference prints "Fail to open index.txt!" and goes on without a map
  }
  std::map<CubeKey, int32_t> index[2];
  int count, type, i, j, k, size;
  while (fin >> count >> type >> i >> j >> k >> size) index[type ? 1 : 0][CubeKey{i, j, k}] = count;  // a later line replaces an earlier one
  (void)hipStreamSynchronize(loc->stream);
  Paged &pg = loc->pg;
  if (!pg.on) {  // the arenas share lslam_loc::tpts / nodes with the static structures, which end here
    pg.cap_pts = pg.cap_nodes = 0;
  }
  pm_reset(loc);
  pg.on = true;
  pg.dir = dir;
  pg.index[0].swap(index[0]);
  pg.index[1].swap(index[1]);
  pg.st = lslam_loc_window_stats{};
  loc->have_map = false;
  loc->grid_valid = false;
  set_grid_cells(loc, true);
  return LSLAM_OK;
}

int lslam_pmap_setup_capacity(lslam_loc *loc, size_t max_points_per_type) {
  int rc = check_loc(loc, "lslam_pmap_setup_capacity");
  if (rc) return rc;
  if (max_points_per_type > ((size_t)1 << 29)) return invalid("lslam_pmap_setup_capacity", "more than 2^29 points per type");
  loc->pg.limit = max_points_per_type;
  return LSLAM_OK;
}

int lslam_pmap_update(lslam_loc *loc, const float pos[3]) {
  int rc = paged_only(loc, "lslam_pmap_update");
  if (rc) return rc;
  if (!pos) return invalid("lslam_pmap_update", "null position");
  return pm_update(loc, pos);
}

int lslam_pmap_stage(lslam_loc *loc, const float pos[3]) {
  int rc = paged_only(loc, "lslam_pmap_stage");
  if (rc) return rc;
  if (!pos) return invalid("lslam_pmap_stage", "null position");
  int c[3];
  for (int d = 0; d < 3; ++d) {
    if (!std::isfinite(pos[d])) return invalid("lslam_pmap_stage", "the position is not finite");
    c[d] = (int)std::round(pos[d] / loc->cfg_cube);
  }
  return pm_bring(loc, c, true);
}

int lslam_pmap_get_surround(lslam_loc *loc, float *corner_xyzi, size_t cap_corner, size_t *n_corner, float *surf_xyzi,
                                  size_t cap_surf, size_t *n_surf) {
  if (n_corner) *n_corner = 0;
  if (n_surf) *n_surf = 0;
  int rc = paged_only(loc, "lslam_pmap_get_surround");
  if (rc) return rc;
  if (!n_corner || !n_surf) return invalid("lslam_pmap_get_surround", "null count outputs");
  if (!loc->pg.have_window) {
    lslam::set_error("paged window: no update yet");
    return LSLAM_ERR_NO_MAP;
  }
  return pm_surround(loc, "lslam_pmap_get_surround", corner_xyzi, cap_corner, n_corner, surf_xyzi, cap_surf, n_surf);
}

int lslam_pmap_window_info(lslam_loc *loc, lslam_loc_window_stats *out) {
  if (out) std::memset(out, 0, sizeof(*out));
  int rc = check_loc(loc, "lslam_pmap_window_info");
  if (rc) return rc;
  if (!out) return invalid("lslam_pmap_window_info", "null output");
  Paged &pg = loc->pg;
  *out = pg.st;
  out->paged = pg.on ? 1 : 0;
  out->have_window = pg.have_window ? 1 : 0;
  out->dims[0] = loc->W; out->dims[1] = loc->H; out->dims[2] = loc->D;
  for (int d = 0; d < 3; ++d) out->centre[d] = pg.centre[d];
  for (int t = 0; t < 2; ++t) {
    out->resident[t] = out->resident_with_tree[t] = out->staged[t] = 0;
    for (const auto &kv : pg.cubes[t]) {
      if (kv.second.staged) {
        out->staged[t]++;
      } else {
        out->resident[t]++;
        if (kv.second.batch >= 0) out->resident_with_tree[t]++;
      }
    }
  }
  out->arena_points_used = pg.used[0] + pg.used[1];
  out->arena_points_capacity = pg.cap_pts;
  out->arena_nodes_used = pg.nodes_used;
  out->arena_nodes_capacity = pg.cap_nodes;
  return LSLAM_OK;
}

int lslam_index_convert(const char *in_path, int32_t ox, int32_t oy, int32_t oz, const char *out_path) {
  if (!in_path || !out_path) return invalid("lslam_index_convert", "null path");
  std::ifstream fin(in_path);
  if (!fin) return invalid("lslam_index_convert", "input file error!");
  std::vector<std::array<long long, 6>> lines;
  long long count, type, i, j, k, size;
  while (fin >> count >> type >> i >> j >> k >> size) lines.push_back({count, type, i - ox, j - oy, k - oz, size});
  fin.close();  // (read whole before writing: out_path may be in_path)
  std::ofstream fout(out_path);
  if (!fout) return invalid("lslam_index_convert", "save file error!");
  for (const auto &l : lines) fout << l[0] << " " << l[1] << " " << l[2] << " " << l[3] << " " << l[4] << " " << l[5] << std::endl;
  return fout ? LSLAM_OK : invalid("lslam_index_convert", "save file error!");
}

}  // extern "C"

#include "lslam_reloc_impl.hpp"
