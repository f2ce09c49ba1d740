// lslam_pg_marginals.hip -- marginal covariances of pose-graph vertices on gfx950 (fp64): selected columns of H^-1 by a
// preconditioned CG over PANELS of right-hand sides (what g2o's computeMarginals gives the reference's solver).
//
// H is the system lslam_pg_linearize exports at the current estimate; lslam_posegraph.hip expands it at lambda = 0 into the
// solver's six-plane block-CSR and builds the block-Jacobi inverses and, when the second level is on, its dense inverse --
// once per call (lslam::pg_marginal_system).  This unit solves H X = E for the 6 unit columns of every listed vertex.
//
// A panel is MG_W = 60 columns (10 vertices) in MG_WS = 64 lanes: every panel vector is [6 n_v][64] doubles, a column per
// lane, so a wavefront works on ONE vertex row for the whole panel -- the 36 values of a matrix block are wave-uniform
// (one wave-uniform address per value, so one fetch serves the panel's 64 columns), the panel operands are read as 512-byte rows.  A thread owns
// the 6 scalar rows of its vertex in its column: the block-Jacobi inverse is applied in registers.
//
// One PCG iteration is a chain of plain launches, like the solver's multi-launch loop; nothing waits on another workgroup:
//   pgm_prod_kernel     the convergence test on the previous update and beta = r.z / r.z_old, by every block from the same
//                       partial sums in the same order (the first block records them); p_k = z + beta p_(k-1) recomputed
//                       where it is needed; Q = H P; per-block partials of p . q
//   pgm_update_kernel   alpha = r.z / p.q the same way; x += alpha p, r -= alpha q, z = D^-1 r; partials of r.z and r.r
//   pgm_restrict_kernel, pgm_coarse_kernel   (second level) R_c = P^T R, Y_c = A_c^-1 R_c, Z += P Y_c, partials of r_c . y_c
//   pgm_check_kernel    (one block, once per MG_CHUNK iterations) the convergence test, before the host reads the flags
// Columns are independent: each has its own alpha, beta, residual and done flag, a finished column is frozen (no kernel
// writes it again), and every sum has a fixed order that does not depend on which lane or panel the column sits in -- the
// vertices of a block in order inside a wavefront, the four wavefronts of a block in order, the blocks in order (split in
// four contiguous runs).  No atomics.  The host reads the flags every MG_CHUNK iterations and enforces the iteration cap.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/lslam_c.h"
#include "lslam_buf.hpp"
#include "lslam_pg_internal.hpp"

namespace {

constexpr int MG_W = 60;      // columns of a panel: 10 vertices
constexpr int MG_WS = 64;     // lanes / row stride of a panel vector (the last four lanes of a panel are never used)
constexpr int MG_BLOCK = 256;
constexpr int MG_WAVES = MG_BLOCK / 64;
constexpr int MG_VPW = 4;                   // vertices a wavefront handles, one after the other
constexpr int MG_VPB = MG_WAVES * MG_VPW;   // vertices per block: one partial sum per block and column
constexpr int MG_CHUNK = 8;   // iterations between two reads of the done flags
// scal[s][64]: per-column scalars
// S_RZ0 / S_RZ1: r.z entering iteration k lives in slot k & 1 (the product kernel of iteration k reads the other one for beta
// while its first block writes this one)
enum { S_RZ0 = 0, S_RZ1, S_RR, S_DONE /* 0 running, 1 converged, 2 broke down */, S_ITERS, S_N };

struct MgArgs {
  const double *vals;  // six planes of n_items (pg_expand_kernel)
  const int32_t *row_ptr, *row_col;
  const double *minv;
  double *x, *r, *z, *q, *p[2];       // [n6][MG_WS]; the direction of iteration k lives in p[k & 1]
  double *part_pq, *part_rz, *part_rr;  // [.][MG_WS]: n_blocks, n_blocks + n_agg, n_blocks
  double *scal;                       // [S_N][MG_WS]
  const int32_t *col_row;             // [MG_WS] the scalar row of this lane's unit vector; -1: the lane is not in use
  int n_v, n_blocks, n_agg;
  size_t n_items;
  double tol2;
};

#define MG_DEV __device__ __forceinline__

// the four wavefronts' values of one column, in wavefront order; every thread of the first wavefront returns its column's sum
MG_DEV double sum_waves(double v, double (*sh)[MG_WS], int wave, int lane) {
  sh[wave][lane] = v;
  __syncthreads();
  double s = sh[0][lane];
#pragma unroll
  for (int w = 1; w < MG_WAVES; ++w) s += sh[w][lane];
  __syncthreads();
  return s;
}
// the sum of n per-block partials of one column: four contiguous runs, one per wavefront, then those four in order
MG_DEV double sum_parts(const double *part, int n, double (*sh)[MG_WS], int wave, int lane) {
  const int per = (n + MG_WAVES - 1) / MG_WAVES;
  const int b0 = wave * per, b1 = min(n, b0 + per);
  double s = 0.0;
  for (int b = b0; b < b1; ++b) s += part[(size_t)b * MG_WS + lane];
  return sum_waves(s, sh, wave, lane);
}

// x = 0, r = e, z = D^-1 e, partials of r.z (r.r is 1)
__global__ __launch_bounds__(MG_BLOCK) void pgm_init_kernel(MgArgs a) {
  __shared__ double sh[MG_WAVES][MG_WS];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int erow = a.col_row[lane];
  double rz = 0.0;
  for (int i = 0; i < MG_VPW; ++i) {
    const int v = blockIdx.x * MG_VPB + wave * MG_VPW + i;
    if (v >= a.n_v) break;
    const double *mi = a.minv + (size_t)v * 36;
#pragma unroll
    for (int rr = 0; rr < 6; ++rr) {
      const size_t at = (size_t)(v * 6 + rr) * MG_WS + lane;
      const int c = erow - v * 6;  // the column of D_v^-1 the unit vector picks, when it sits in this vertex
      const double e = (c == rr) ? 1.0 : 0.0;
      const double z = (erow >= 0 && c >= 0 && c < 6) ? mi[rr * 6 + c] : 0.0;
      a.x[at] = 0.0;
      a.r[at] = (erow >= 0) ? e : 0.0;
      a.z[at] = z;
      rz += ((erow >= 0) ? e : 0.0) * z;
    }
  }
  const double s = sum_waves(rz, sh, wave, lane);
  if (wave == 0) {
    a.part_rz[(size_t)blockIdx.x * MG_WS + lane] = s;
    a.part_rr[(size_t)blockIdx.x * MG_WS + lane] = (blockIdx.x == 0 && erow >= 0) ? 1.0 : 0.0;  // |e|^2 = 1
  }
  if (blockIdx.x == 0 && wave == 0) {
    a.scal[S_RR * MG_WS + lane] = (erow >= 0) ? 1.0 : 0.0;
    a.scal[S_DONE * MG_WS + lane] = (erow >= 0) ? 0.0 : 1.0;
    a.scal[S_ITERS * MG_WS + lane] = 0.0;
    a.scal[S_RZ0 * MG_WS + lane] = 0.0;
    a.scal[S_RZ1 * MG_WS + lane] = 0.0;
  }
}

// What every block decides for its column from the same partial sums in the same order, hence identically: the column has
// converged (|r| <= tol |e|, |e| = 1), or r.z is not positive (the preconditioned system is not positive definite there).
MG_DEV double column_state(double done, double rz, double rr, double tol2) {
  if (done != 0.0) return done;
  if (rr <= tol2) return 1.0;
  if (!(rz > 0.0)) return 2.0;
  return 0.0;
}

// Iteration k, first half: Q = H P_k for the panel with P_k = Z + beta P_(k-1) recomputed at the columns of every entry (the
// diagonal entry, first in its row, publishes P_k), and the partials of p . q.  The block's 36 values are wave-uniform.
__global__ __launch_bounds__(MG_BLOCK) void pgm_prod_kernel(MgArgs a, int k) {
  __shared__ double sh[MG_WAVES][MG_WS];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // the convergence test on the previous update and beta, by every block for itself; the first block records them
  const double done0 = a.scal[S_DONE * MG_WS + lane], rz_old = a.scal[(S_RZ0 + ((k + 1) & 1)) * MG_WS + lane];
  const double rz = sum_parts(a.part_rz, a.n_blocks + a.n_agg, sh, wave, lane);
  const double rr = sum_parts(a.part_rr, a.n_blocks, sh, wave, lane);
  const double state = column_state(done0, rz, rr, a.tol2);
  const bool on = state == 0.0;
  const double beta = (k > 0 && on) ? rz / rz_old : 0.0;
  if (blockIdx.x == 0 && wave == 0 && done0 == 0.0) {
    a.scal[S_RR * MG_WS + lane] = rr;
    if (on) a.scal[(S_RZ0 + (k & 1)) * MG_WS + lane] = rz;
    else a.scal[S_DONE * MG_WS + lane] = state;
  }
  const double *po = (k > 0) ? a.p[(k + 1) & 1] : a.z;  // k == 0: beta = 0, p_0 = z
  double *pn = a.p[k & 1];
  double pq = 0.0;
  for (int i = 0; i < MG_VPW; ++i) {
    const int v = blockIdx.x * MG_VPB + wave * MG_VPW + i;
    if (v >= a.n_v) break;
    const int e0 = a.row_ptr[v], e1 = a.row_ptr[v + 1];
    double q[6] = {0, 0, 0, 0, 0, 0}, pv[6] = {0, 0, 0, 0, 0, 0};
    for (int e = e0; e < e1; ++e) {
      const size_t c0 = (size_t)a.row_col[e] * 6;
      double pc[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const size_t at = (c0 + c) * MG_WS + lane;
        const double zc = a.z[at], oc = po[at];
        pc[c] = (k > 0) ? zc + beta * oc : zc;
      }
      if (e == e0) {
#pragma unroll
        for (int c = 0; c < 6; ++c) pv[c] = pc[c];
      }
      const double *A = a.vals + (size_t)e * 6;
#pragma unroll
      for (int rr = 0; rr < 6; ++rr) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) s += A[(size_t)c * a.n_items + rr] * pc[c];
        q[rr] += s;
      }
    }
    if (on) {
#pragma unroll
      for (int rr = 0; rr < 6; ++rr) {
        const size_t at = (size_t)(v * 6 + rr) * MG_WS + lane;
        a.q[at] = q[rr];
        pn[at] = pv[rr];
        pq += pv[rr] * q[rr];
      }
    }
  }
  const double s = sum_waves(pq, sh, wave, lane);
  if (wave == 0 && on) a.part_pq[(size_t)blockIdx.x * MG_WS + lane] = s;
}

// Iteration k, second half: alpha = r.z / p.q by every block for itself ; x += alpha p ; r -= alpha q ; z = D^-1 r in
// registers ; partials of r.z and r.r
__global__ __launch_bounds__(MG_BLOCK) void pgm_update_kernel(MgArgs a, int k) {
  __shared__ double sh[MG_WAVES][MG_WS];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const double done0 = a.scal[S_DONE * MG_WS + lane];
  const double pq = sum_parts(a.part_pq, a.n_blocks, sh, wave, lane);
  // !(p.q > 0): H is not positive definite along p (or a NaN) -- this column cannot be solved
  const bool on = done0 == 0.0 && pq > 0.0;
  const double alpha = on ? a.scal[(S_RZ0 + (k & 1)) * MG_WS + lane] / pq : 0.0;
  if (blockIdx.x == 0 && wave == 0 && done0 == 0.0) {
    if (on) a.scal[S_ITERS * MG_WS + lane] = (double)(k + 1);
    else a.scal[S_DONE * MG_WS + lane] = 2.0;
  }
  const double *p = a.p[k & 1];
  double rz = 0.0, rr2 = 0.0;
  for (int i = 0; i < MG_VPW; ++i) {
    const int v = blockIdx.x * MG_VPB + wave * MG_VPW + i;
    if (v >= a.n_v) break;
    const double *mi = a.minv + (size_t)v * 36;
    double rn[6];
#pragma unroll
    for (int rr = 0; rr < 6; ++rr) {
      const size_t at = (size_t)(v * 6 + rr) * MG_WS + lane;
      const double xv = a.x[at], pv = p[at], rv = a.r[at], qv = a.q[at];
      rn[rr] = rv - alpha * qv;
      if (on) {
        a.x[at] = xv + alpha * pv;
        a.r[at] = rn[rr];
      }
    }
#pragma unroll
    for (int rr = 0; rr < 6; ++rr) {
      double z = 0.0;
#pragma unroll
      for (int c = 0; c < 6; ++c) z += mi[rr * 6 + c] * rn[c];
      if (on) a.z[(size_t)(v * 6 + rr) * MG_WS + lane] = z;
      rz += rn[rr] * z;
      rr2 += rn[rr] * rn[rr];
    }
  }
  const double s0 = sum_waves(rz, sh, wave, lane);
  const double s1 = sum_waves(rr2, sh, wave, lane);
  if (wave == 0 && on) {
    a.part_rz[(size_t)blockIdx.x * MG_WS + lane] = s0;
    a.part_rr[(size_t)blockIdx.x * MG_WS + lane] = s1;
  }
}

// second level, R_c = P^T R: one wavefront per aggregate, a column per lane, the members in order
__global__ __launch_bounds__(64) void pgm_restrict_kernel(MgArgs a, CoarseArgs c, double *Rc) {
  const int g = blockIdx.x, lane = threadIdx.x;
  if (a.scal[S_DONE * MG_WS + lane] != 0.0) return;
  double w[6] = {0, 0, 0, 0, 0, 0};
  for (int m = c.agg_ptr[g]; m < c.agg_ptr[g + 1]; ++m) {
    const int i = c.agg_mem[m];
    const double *P = c.P + (size_t)i * 36;
#pragma unroll
    for (int kk = 0; kk < 6; ++kk) {
      const double rk = a.r[(size_t)(i * 6 + kk) * MG_WS + lane];
#pragma unroll
      for (int mm = 0; mm < 6; ++mm) w[mm] += P[kk * 6 + mm] * rk;
    }
  }
#pragma unroll
  for (int mm = 0; mm < 6; ++mm) Rc[(size_t)(g * 6 + mm) * MG_WS + lane] = w[mm];
}
// ... Y_c = A_c^-1 R_c, the dense (n_c x n_c) x (n_c x panel) product: one workgroup per aggregate computes ITS six rows for
// the whole panel (the four wavefronts take a quarter of the inner index each, summed in order), its share r_c[a] . y_c[a] of
// r . z, and prolongs to its members: Z += P Y_c.  The six matrix rows are wave-uniform; plain fp64 FMA-rate arithmetic.
__global__ __launch_bounds__(MG_BLOCK) void pgm_coarse_kernel(MgArgs a, CoarseArgs c, const double *Rc) {
  __shared__ double sh[MG_WAVES][MG_WS];
  __shared__ double y6[6][MG_WS];
  const int g = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool on = a.scal[S_DONE * MG_WS + lane] == 0.0;
  const int per = (c.n_c + MG_WAVES - 1) / MG_WAVES;
  const int j0 = wave * per, j1 = min(c.n_c, j0 + per);
  double s[6] = {0, 0, 0, 0, 0, 0};
  const double *Arow = c.Ac + (size_t)(g * 6) * c.n_c;
  for (int j = j0; j < j1; ++j) {
    const double rc = Rc[(size_t)j * MG_WS + lane];
#pragma unroll
    for (int m = 0; m < 6; ++m) s[m] += Arow[(size_t)m * c.n_c + j] * rc;
  }
  double dot = 0.0;
#pragma unroll
  for (int m = 0; m < 6; ++m) {
    const double y = sum_waves(s[m], sh, wave, lane);
    if (wave == 0) {
      y6[m][lane] = y;
      dot += y * Rc[(size_t)(g * 6 + m) * MG_WS + lane];
    }
  }
  if (wave == 0 && on) a.part_rz[(size_t)(a.n_blocks + g) * MG_WS + lane] = dot;
  __syncthreads();
  if (!on) return;
  const int m0 = c.agg_ptr[g], m1 = c.agg_ptr[g + 1];
  for (int m = m0 + wave; m < m1; m += MG_WAVES) {
    const int i = c.agg_mem[m];
    const double *P = c.P + (size_t)i * 36;
#pragma unroll
    for (int rr = 0; rr < 6; ++rr) {
      double acc = 0.0;
#pragma unroll
      for (int mm = 0; mm < 6; ++mm) acc += P[rr * 6 + mm] * y6[mm][lane];
      a.z[(size_t)(i * 6 + rr) * MG_WS + lane] += acc;
    }
  }
}

// One block, before the host reads the flags: the convergence test on the last update -- what the next product kernel
// would decide from the same sums, and decides again if it runs.
__global__ __launch_bounds__(MG_BLOCK) void pgm_check_kernel(MgArgs a) {
  __shared__ double sh[MG_WAVES][MG_WS];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const double done0 = a.scal[S_DONE * MG_WS + lane];
  const double rz = sum_parts(a.part_rz, a.n_blocks + a.n_agg, sh, wave, lane);
  const double rr = sum_parts(a.part_rr, a.n_blocks, sh, wave, lane);
  if (wave != 0 || done0 != 0.0) return;
  a.scal[S_RR * MG_WS + lane] = rr;
  a.scal[S_DONE * MG_WS + lane] = column_state(done0, rz, rr, a.tol2);
}

// out[(i * 6 + r)][col0 + lane] = x[row vertex i][r][lane]; row_v[i] < 0 stands for the column's own vertex
__global__ void pgm_gather_kernel(const double *x, const int32_t *col_row, const int32_t *row_v, int n_rows_v, double *out,
                                  size_t out_stride, int col0) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (t >= n_rows_v * 6 || lane >= MG_W) return;
  const int erow = col_row[lane];
  if (erow < 0) return;
  const int i = t / 6, rr = t % 6;
  const int v = row_v[i] >= 0 ? row_v[i] : erow / 6;
  out[(size_t)t * out_stride + col0 + lane] = x[(size_t)(v * 6 + rr) * MG_WS + lane];
}

#define MG_TRY(expr)                                                                     \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) {                                                              \
      char _b[512];                                                                      \
      snprintf(_b, sizeof(_b), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      lslam::pg_error() = _b;                                                            \
      return LSLAM_ERR_HIP;                                                              \
    }                                                                                    \
  } while (0)

int invalid(const char *fmt, int a = 0, int b = 0, double c = 0.0) {
  char buf[512];
  snprintf(buf, sizeof(buf), fmt, a, b, c);
  lslam::pg_error() = buf;
  return LSLAM_ERR_INVALID;
}

// What one call solves for and takes home.
struct MargCall {
  std::vector<int32_t> solve_v;  // distinct vertices whose 6 columns are solved, none of them fixed; 10 per panel
  std::vector<int32_t> row_v;    // vertex rows gathered from every column; -1: the column's own vertex
  std::vector<double> out;       // [row_v.size() * 6][6 * solve_v.size()]
  size_t stride() const { return 6 * solve_v.size(); }
  int col_of(int v) const {      // first column of vertex v in `out`, -1: not solved for
    for (size_t k = 0; k < solve_v.size(); ++k)
      if (solve_v[k] == v) return (int)(6 * k);
    return -1;
  }
  // block (row slot i, vertex v's columns), row-major 6x6
  void block(int i, int v, double B[36]) const {
    const int c0 = col_of(v);
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) B[r * 6 + c] = out[(size_t)(i * 6 + r) * stride() + c0 + c];
  }
};

// Everything that is refused before a launch: arguments, sharded graphs, vertices out of range, components without a gauge.
int check_call(const lslam_pg *pg, int n_q, const int32_t *vertices, const double *cov36, int ref) {
  if (!pg || n_q < 0 || (n_q > 0 && (!vertices || !cov36))) return invalid("bad arguments for the marginal covariances");
  if (pg->sharded() || pg->row_v0 >= 0 || pg->e_begin != 0 || pg->e_end != pg->n_e)
    return invalid("marginal covariances are not available on a sharded graph (lslam_pg_set_shard / _set_comm / _set_row_shard)");
  if (ref >= pg->n_v || ref < -1) return invalid("reference vertex %d out of range (the graph has %d vertices)", ref, pg->n_v);
  for (int k = 0; k < n_q; ++k)
    if (vertices[k] < 0 || vertices[k] >= pg->n_v)
      return invalid("queried vertex %d out of range (the graph has %d vertices)", vertices[k], pg->n_v);
  // connected components over the edges (union-find with path halving); a component has a gauge when it holds the fixed
  // vertex or any unary constraint.  Whether the unary constraints it holds suffice is for the solve to find out.
  std::vector<int32_t> parent((size_t)pg->n_v);
  std::iota(parent.begin(), parent.end(), 0);
  const auto find = [&](int v) {
    while (parent[(size_t)v] != v) {
      parent[(size_t)v] = parent[(size_t)parent[(size_t)v]];
      v = parent[(size_t)v];
    }
    return v;
  };
  for (int e = 0; e < pg->n_e; ++e) {
    const int a = find(pg->h_ij[2 * (size_t)e]), b = find(pg->h_ij[2 * (size_t)e + 1]);
    if (a != b) parent[(size_t)std::max(a, b)] = std::min(a, b);
  }
  std::vector<char> gauge((size_t)pg->n_v, 0);
  if (pg->fixed >= 0) gauge[(size_t)find(pg->fixed)] = 1;
  for (int k = 0; k < pg->n_p; ++k) gauge[(size_t)find(pg->h_pv[(size_t)k])] = 1;
  for (int k = 0; k < pg->n_q; ++k) gauge[(size_t)find(pg->h_qv[(size_t)k])] = 1;
  for (int k = -1; k < n_q; ++k) {
    const int v = k < 0 ? ref : vertices[k];
    if (v >= 0 && !gauge[(size_t)find(v)])
      return invalid("vertex %d has no covariance: its connected component holds neither the fixed vertex nor a prior", v);
  }
  return LSLAM_OK;
}

// The panel PCG for the call's columns; fills m.out and the statistics, or fails with nothing written.
int solve_columns(lslam_pg *pg, const lslam_pg_marginal_opts *opts, MargCall &m, lslam_pg_marginal_stats &st) {
  const double tol = (opts && opts->rel_tol != 0.0) ? opts->rel_tol : pg->env_tol;
  if (!(tol > 0.0) || !(tol < 1.0)) return invalid("rel_tol must be in (0, 1), or 0 for the solver's default");
  const int cmode = opts ? opts->coarse : -1;
  if (cmode < -1 || cmode > 1) return invalid("coarse must be -1, 0 or 1");
  if (opts && opts->max_iters < 0) return invalid("max_iters must not be negative");
  const int max_iters = (opts && opts->max_iters > 0) ? opts->max_iters : std::max(100, 6 * pg->n_v);
  const bool coarse = cmode == 1 || (cmode < 0 && (pg->coarse_mode == 1 || (pg->coarse_mode < 0 && pg->coarse_on)));
  st.coarse_used = coarse ? 1 : 0;
  const int n_solve = (int)m.solve_v.size();
  if (n_solve == 0) return LSLAM_OK;
  MG_TRY(hipSetDevice(pg->device));
  CoarseArgs c{};
  int rc = lslam::pg_marginal_system(pg, coarse, &c);
  if (rc) return rc;

  const size_t n6 = (size_t)pg->n_v * 6;
  const int n_blocks = (pg->n_v + MG_VPB - 1) / MG_VPB;
  const int n_agg = coarse ? c.na : 0;
  const int vpp = MG_W / 6, n_panels = (n_solve + vpp - 1) / vpp;
  const size_t n_rows = m.row_v.size() * 6, stride = m.stride();
  MG_TRY(pg->d_mg_vec.reserve(6 * n6 * MG_WS));
  MG_TRY(pg->d_mg_part.reserve((size_t)(3 * n_blocks + n_agg) * MG_WS));
  MG_TRY(pg->d_mg_scal.reserve((size_t)S_N * MG_WS));
  MG_TRY(pg->d_mg_rc.reserve((size_t)std::max(1, 6 * n_agg) * MG_WS));
  MG_TRY(pg->d_mg_out.reserve(n_rows * stride));
  MG_TRY(pg->d_mg_idx.reserve((size_t)n_panels * MG_WS + m.row_v.size()));
  // the panels' unit rows and the gather's row list, in one upload
  std::vector<int32_t> idx((size_t)n_panels * MG_WS + m.row_v.size(), -1);
  for (int k = 0; k < n_solve; ++k)
    for (int r = 0; r < 6; ++r) idx[(size_t)(k / vpp) * MG_WS + (size_t)(k % vpp) * 6 + r] = m.solve_v[(size_t)k] * 6 + r;
  std::copy(m.row_v.begin(), m.row_v.end(), idx.begin() + (size_t)n_panels * MG_WS);
  MG_TRY(hipMemcpyAsync(pg->d_mg_idx.p, idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice, pg->stream));
  const int32_t *d_row_v = pg->d_mg_idx.p + (size_t)n_panels * MG_WS;

  MgArgs a{};
  a.vals = pg->d_vals.p; a.row_ptr = pg->d_row_ptr.p; a.row_col = pg->d_row_col.p; a.minv = pg->d_minv.p;
  double *vec = pg->d_mg_vec.p;
  a.x = vec; a.r = vec + n6 * MG_WS; a.z = vec + 2 * n6 * MG_WS; a.q = vec + 3 * n6 * MG_WS;
  a.p[0] = vec + 4 * n6 * MG_WS; a.p[1] = vec + 5 * n6 * MG_WS;
  a.part_pq = pg->d_mg_part.p;
  a.part_rr = a.part_pq + (size_t)n_blocks * MG_WS;
  a.part_rz = a.part_rr + (size_t)n_blocks * MG_WS;
  a.scal = pg->d_mg_scal.p;
  a.n_v = pg->n_v; a.n_blocks = n_blocks; a.n_agg = n_agg;
  a.n_items = (size_t)pg->n_entries * 6;
  a.tol2 = tol * tol;
  double *Rc = pg->d_mg_rc.p;
  const dim3 grid(n_blocks), blk(MG_BLOCK);
  const auto coarse_correct = [&]() {  // Z += P A_c^-1 P^T R and the matching share of r.z
    if (!coarse) return;
    hipLaunchKernelGGL(pgm_restrict_kernel, dim3(n_agg), dim3(64), 0, pg->stream, a, c, Rc);
    hipLaunchKernelGGL(pgm_coarse_kernel, dim3(n_agg), blk, 0, pg->stream, a, c, (const double *)Rc);
  };
  std::vector<double> scal((size_t)S_N * MG_WS);
  double worst_rr = 0.0;
  for (int pnl = 0; pnl < n_panels; ++pnl) {
    a.col_row = pg->d_mg_idx.p + (size_t)pnl * MG_WS;
    hipLaunchKernelGGL(pgm_init_kernel, grid, blk, 0, pg->stream, a);
    coarse_correct();
    bool all_done = false;
    for (int it = 0; it < max_iters && !all_done;) {
      const int chunk = std::min(MG_CHUNK, max_iters - it);
      for (int k = it; k < it + chunk; ++k) {
        hipLaunchKernelGGL(pgm_prod_kernel, grid, blk, 0, pg->stream, a, k);
        hipLaunchKernelGGL(pgm_update_kernel, grid, blk, 0, pg->stream, a, k);
        coarse_correct();
      }
      it += chunk;
      hipLaunchKernelGGL(pgm_check_kernel, dim3(1), blk, 0, pg->stream, a);
      MG_TRY(hipGetLastError());
      MG_TRY(hipMemcpyAsync(scal.data(), a.scal, scal.size() * sizeof(double), hipMemcpyDeviceToHost, pg->stream));
      MG_TRY(hipStreamSynchronize(pg->stream));
      all_done = true;
      for (int w = 0; w < MG_WS; ++w) all_done = all_done && scal[(size_t)S_DONE * MG_WS + w] != 0.0;
    }
    {  // every column of the panel must have converged: the cap ends the call, not the column
      for (int w = 0; w < MG_W; ++w) {
        const int erow = idx[(size_t)pnl * MG_WS + w];
        if (erow < 0) continue;
        const double done = scal[(size_t)S_DONE * MG_WS + w], rr = scal[(size_t)S_RR * MG_WS + w];
        if (done != 1.0) {
          char buf[512];
          snprintf(buf, sizeof(buf),
                   "no covariance for vertex %d: column %d %s (|r|/|e| = %.3g after %d of at most %d iterations, tolerance %.3g) -- "
                   "is its component constrained in all six directions?",
                   erow / 6, erow % 6,
                   std::isnan(rr) ? "is not a number (with the second level, a component ANYWHERE in the graph that nothing holds makes its coarse matrix singular)"
                   : done == 2.0  ? "met a direction in which the system is not positive definite"
                                  : "did not reach the tolerance",
                   std::sqrt(rr), (int)scal[(size_t)S_ITERS * MG_WS + w], max_iters, tol);
          lslam::pg_error() = buf;
          return LSLAM_ERR_INVALID;
        }
        const int iters = (int)scal[(size_t)S_ITERS * MG_WS + w];
        st.iters_max = std::max(st.iters_max, iters);
        st.iters_sum += iters;
        worst_rr = std::max(worst_rr, rr);
      }
    }
    const int gthreads = 256, rows_per_block = gthreads / 64;
    hipLaunchKernelGGL(pgm_gather_kernel, dim3((unsigned)((n_rows + rows_per_block - 1) / rows_per_block)), dim3(gthreads), 0,
                       pg->stream, (const double *)a.x, a.col_row, d_row_v, (int)m.row_v.size(), pg->d_mg_out.p, stride,
                       pnl * MG_W);
    MG_TRY(hipGetLastError());
  }
  m.out.resize(n_rows * stride);
  MG_TRY(hipMemcpyAsync(m.out.data(), pg->d_mg_out.p, m.out.size() * sizeof(double), hipMemcpyDeviceToHost, pg->stream));
  MG_TRY(hipStreamSynchronize(pg->stream));
  st.panels = n_panels;
  st.worst_rel_residual = std::sqrt(worst_rr);
  return LSLAM_OK;
}

void push_distinct(std::vector<int32_t> &list, int v) {
  if (std::find(list.begin(), list.end(), v) == list.end()) list.push_back(v);
}

void symmetrise(const double X[36], double *S) {
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) S[r * 6 + c] = 0.5 * (X[r * 6 + c] + X[c * 6 + r]);
}

}  // namespace

extern "C" {

int lslam_pg_marginals(lslam_pg *pg, int32_t n_q, const int32_t *vertices, const lslam_pg_marginal_opts *opts, double *cov36,
                       double *cross36, lslam_pg_marginal_stats *stats) {
  int rc = check_call(pg, n_q, vertices, cov36, -1);
  if (rc) return rc;
  lslam_pg_marginal_stats st{};
  MargCall m;
  std::vector<int32_t> distinct;
  for (int k = 0; k < n_q; ++k) {
    push_distinct(distinct, vertices[k]);
    if (vertices[k] != pg->fixed) push_distinct(m.solve_v, vertices[k]);
  }
  st.columns = 6 * (int)distinct.size();
  // rows to take home: the column's own vertex for the diagonal blocks; with cross blocks every solved vertex's rows
  if (cross36) m.row_v = m.solve_v; else m.row_v.assign(1, -1);
  rc = solve_columns(pg, opts, m, st);
  if (rc) return rc;
  const auto row_slot = [&](int v) { return cross36 ? m.col_of(v) / 6 : 0; };
  for (int k = 0; k < n_q; ++k) {
    const int v = vertices[k];
    double X[36];
    if (v == pg->fixed) {
      std::memset(cov36 + (size_t)k * 36, 0, 36 * sizeof(double));
      continue;
    }
    m.block(row_slot(v), v, X);
    symmetrise(X, cov36 + (size_t)k * 36);
  }
  if (cross36)
    for (int ka = 0; ka < n_q; ++ka)
      for (int kb = 0; kb < n_q; ++kb) {
        double *o = cross36 + ((size_t)ka * n_q + kb) * 36;
        const int va = vertices[ka], vb = vertices[kb];
        if (va == pg->fixed || vb == pg->fixed) {
          std::memset(o, 0, 36 * sizeof(double));
        } else if (va == vb) {
          std::memcpy(o, cov36 + (size_t)ka * 36, 36 * sizeof(double));
        } else {  // ONE solved block per pair, rows of the lower vertex in the columns of the higher: (b, a) is its exact transpose
          double X[36];
          m.block(row_slot(std::min(va, vb)), std::max(va, vb), X);
          for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c) o[r * 6 + c] = va < vb ? X[r * 6 + c] : X[c * 6 + r];
        }
      }
  if (stats) *stats = st;
  return LSLAM_OK;
}

// Test tap: the six solved columns of one vertex as the panel PCG left them, every row, nothing symmetrised or zeroed.
int lslam_debug_pg_marginal_columns(lslam_pg *pg, int32_t vertex, const lslam_pg_marginal_opts *opts, double *x_out,
                                    lslam_pg_marginal_stats *stats) {
  int rc = check_call(pg, 1, &vertex, x_out, -1);
  if (rc) return rc;
  if (vertex == pg->fixed) return invalid("vertex %d is the fixed one: no column is solved for it", vertex);
  lslam_pg_marginal_stats st{};
  st.columns = 6;
  MargCall m;
  m.solve_v.assign(1, vertex);
  m.row_v.resize((size_t)pg->n_v);
  std::iota(m.row_v.begin(), m.row_v.end(), 0);
  rc = solve_columns(pg, opts, m, st);
  if (rc) return rc;
  std::memcpy(x_out, m.out.data(), m.out.size() * sizeof(double));
  if (stats) *stats = st;
  return LSLAM_OK;
}

int lslam_pg_relative_covariances(lslam_pg *pg, int32_t ref, int32_t n_q, const int32_t *vertices,
                                  const lslam_pg_marginal_opts *opts, double *cov36, lslam_pg_marginal_stats *stats) {
  if (pg && ref < 0) return invalid("reference vertex %d out of range (the graph has %d vertices)", ref, pg->n_v);
  int rc = check_call(pg, n_q, vertices, cov36, ref);
  if (rc) return rc;
  lslam_pg_marginal_stats st{};
  MargCall m;
  std::vector<int32_t> distinct(1, ref), query_v;  // query_v: the distinct queries other than ref, in order
  if (ref != pg->fixed) m.solve_v.push_back(ref);
  for (int k = 0; k < n_q; ++k) {
    push_distinct(distinct, vertices[k]);
    if (vertices[k] != ref) push_distinct(query_v, vertices[k]);
    if (vertices[k] != pg->fixed) push_distinct(m.solve_v, vertices[k]);
  }
  st.columns = 6 * (int)distinct.size();
  // rows to take home from every column: those of ref (the cross block) and the column's own vertex
  m.row_v = {ref, -1};
  rc = solve_columns(pg, opts, m, st);
  if (rc) return rc;
  std::vector<double> J(72 * std::max<size_t>(1, query_v.size()));
  if (!query_v.empty()) {
    MG_TRY(hipSetDevice(pg->device));
    MG_TRY(pg->d_mg_idx.reserve(query_v.size()));
    MG_TRY(pg->d_mg_jac.reserve(72 * query_v.size()));
    MG_TRY(hipMemcpyAsync(pg->d_mg_idx.p, query_v.data(), query_v.size() * sizeof(int32_t), hipMemcpyHostToDevice, pg->stream));
    rc = lslam::pg_relative_jacobians(pg, ref, (int)query_v.size(), pg->d_mg_idx.p, pg->d_mg_jac.p);
    if (rc) return rc;
    MG_TRY(hipMemcpyAsync(J.data(), pg->d_mg_jac.p, 72 * query_v.size() * sizeof(double), hipMemcpyDeviceToHost, pg->stream));
    MG_TRY(hipStreamSynchronize(pg->stream));
  }
  double Srr[36] = {0};
  if (ref != pg->fixed) {
    double X[36];
    m.block(1, ref, X);
    symmetrise(X, Srr);
  }
  for (int k = 0; k < n_q; ++k) {
    const int v = vertices[k];
    double *o = cov36 + (size_t)k * 36;
    if (v == ref) {
      std::memset(o, 0, 36 * sizeof(double));
      continue;
    }
    // the joint 12x12 marginal [Srr Srj; Srj^T Sjj]: zero wherever the fixed vertex is involved
    double S[144] = {0}, X[36], Sjj[36] = {0}, Srj[36] = {0};
    if (v != pg->fixed) {
      m.block(1, v, X);
      symmetrise(X, Sjj);
      if (ref != pg->fixed) m.block(0, v, Srj);  // rows of ref in the columns of v
    }
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) {
        S[r * 12 + c] = Srr[r * 6 + c];
        S[(6 + r) * 12 + 6 + c] = Sjj[r * 6 + c];
        S[r * 12 + 6 + c] = Srj[r * 6 + c];
        S[(6 + c) * 12 + r] = Srj[r * 6 + c];
      }
    const double *Jk = J.data() + 72 * (size_t)(std::find(query_v.begin(), query_v.end(), v) - query_v.begin());
    double T[72], M[36];  // T = [J_r J_j] S (6 x 12), M = T [J_r J_j]^T
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 12; ++c) {
        double s = 0.0;
        for (int kk = 0; kk < 12; ++kk) s += Jk[(kk / 6) * 36 + r * 6 + kk % 6] * S[kk * 12 + c];
        T[r * 12 + c] = s;
      }
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) {
        double s = 0.0;
        for (int kk = 0; kk < 12; ++kk) s += T[r * 12 + kk] * Jk[(kk / 6) * 36 + c * 6 + kk % 6];
        M[r * 6 + c] = s;
      }
    symmetrise(M, o);
  }
  if (stats) *stats = st;
  return LSLAM_OK;
}

}  // extern "C"
