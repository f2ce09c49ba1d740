// lslam_posegraph.hip -- SE(3) pose-graph Levenberg-Marquardt on gfx950 (fp64).
//
// Replaces pose_graph::SolverG2O (pose_graph/solver_g2o.cpp:51-95: add_se3_node,
// add_se3_edge, optimize), i.e. g2o's VertexSE3 / EdgeSE3 / "lm_var".  g2o itself is not
// under /root/reference (and not pinned by it): the conventions restated here are g2o's
// published ones -- update X <- X * fromVectorMQT(d), error toVectorMQT(Z^-1 Xi^-1 Xj),
// LM schedule of OptimizationAlgorithmLevenberg -- see oracle/posegraph_oracle.py.
//
// Data parallel structure
//   pg_edge_kernel, pg_edge_robust_kernel (edges with robust kernels; pg_edge_robust_tap_kernel: their e2 / rho for the host)
//                       one lane per edge of this rank's shard: error, analytic Jacobians,
//                       J^T Omega J blocks, J^T Omega e, chi2 -> per-edge records
//   pg_prior_kernel     one lane per unary constraint (GPS position / absolute pose on one vertex; pg_prior_chi2_kernel,
//                       pg_prior_tap_kernel: the trial's and the host's values) -- launched only while a graph has priors
//   pg_assemble_vertex_kernel (pg_assemble_vertex_prior_kernel with priors), pg_assemble_off_kernel, pg_sum_kernel
//                       deterministic gather of the records into the block system
//                       [diag blocks | off-diagonal blocks | b | chi2]  (fixed order, no atomics)
//   (all-reduce of that buffer across ranks: callback, or the library's RCCL communicator)
//   pg_expand_kernel, pg_precond_kernel          block rows of H + lambda I, inverses of its diagonal blocks
//   pg_cg_init / init2 / prod / update / check_kernel   replicated block-Jacobi PCG, a launch per step
//   pg_rs_*_kernel      what the row-sharded form of that loop adds (several GPUs share one solve)
//   pgc_*_kernel        second preconditioner level: rigid motions of graph aggregates, dense inverse by Gauss-Jordan
//                       (pgc_gj_pivot / update_kernel per pivot, or pgc_gj_persistent_kernel in one launch)
//   pg_pcg_persistent_kernel   the whole PCG loop, second level included, in one cooperative launch
//   pg_update_kernel    X <- X * fromVectorMQT(dx);  pg_chi2_kernel, pg_chi2_robust_kernel: chi2 of a trial
//   pg_dot_scale_kernel, pg_maxdiag_kernel       LM's gain denominator and first damping
//   pg_rel_jac_kernel   the edge Jacobians of a relative pose, for the marginal covariances (lslam_pg_marginals.hip, which
//                       takes the lambda = 0 system and the coarse inverse from this unit: lslam::pg_marginal_system)
// The host side is cut into named stages: solve(), lslam_pg_create() and lslam_pg_optimize() each read as their list.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/lslam_c.h"
#include "lslam_buf.hpp"
#include "lslam_pg_internal.hpp"  // struct lslam_pg, CoarseArgs, the comm entry points

namespace {

#define PG_DEV __device__ __forceinline__

struct Q4 { double x, y, z, w; };
struct V3 { double x, y, z; };

PG_DEV Q4 qmul(const Q4 &a, const Q4 &b) {
  return {a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
          a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
PG_DEV Q4 qconj(const Q4 &q) { return {-q.x, -q.y, -q.z, q.w}; }
PG_DEV void qrotmat(const Q4 &q, double R[9]) {
  const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
  const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
  const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
  const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
PG_DEV V3 mulR(const double R[9], const V3 &v) {
  return {R[0] * v.x + R[1] * v.y + R[2] * v.z, R[3] * v.x + R[4] * v.y + R[5] * v.z,
          R[6] * v.x + R[7] * v.y + R[8] * v.z};
}
PG_DEV V3 mulRt(const double R[9], const V3 &v) {
  return {R[0] * v.x + R[3] * v.y + R[6] * v.z, R[1] * v.x + R[4] * v.y + R[7] * v.z,
          R[2] * v.x + R[5] * v.y + R[8] * v.z};
}
PG_DEV void skew(const V3 &v, double S[9]) {
  S[0] = 0; S[1] = -v.z; S[2] = v.y;
  S[3] = v.z; S[4] = 0; S[5] = -v.x;
  S[6] = -v.y; S[7] = v.x; S[8] = 0;
}

struct Pose { V3 t; Q4 q; };
PG_DEV Pose load_pose(const double *p) { return {{p[0], p[1], p[2]}, {p[3], p[4], p[5], p[6]}}; }

// e = toVectorMQT(Z^-1 * Xi^-1 * Xj); optionally the Jacobians w.r.t. the local updates.
// Ji/Jj row-major 6x6.
template <bool JAC>
PG_DEV void edge_error(const Pose &xi, const Pose &xj, const Pose &z, double e[6], double *Ji,
                       double *Jj) {
  double Ri[9], Rz[9];
  qrotmat(xi.q, Ri);
  qrotmat(z.q, Rz);
  const V3 d = {xj.t.x - xi.t.x, xj.t.y - xi.t.y, xj.t.z - xi.t.z};
  const V3 tb = mulRt(Ri, d);                                  // Xi^-1 Xj translation
  const Q4 qb = qmul(qconj(xi.q), xj.q);                       // Xi^-1 Xj rotation
  const V3 te = mulRt(Rz, {tb.x - z.t.x, tb.y - z.t.y, tb.z - z.t.z});
  Q4 qe = qmul(qconj(z.q), qb);
  const double nrm = sqrt(qe.x * qe.x + qe.y * qe.y + qe.z * qe.z + qe.w * qe.w);
  qe = {qe.x / nrm, qe.y / nrm, qe.z / nrm, qe.w / nrm};
  const double sgn = qe.w < 0 ? -1.0 : 1.0;
  qe = {sgn * qe.x, sgn * qe.y, sgn * qe.z, sgn * qe.w};
  e[0] = te.x; e[1] = te.y; e[2] = te.z;
  e[3] = qe.x; e[4] = qe.y; e[5] = qe.z;
  if (!JAC) return;
  // ---- vertex j: E' = E * Delta_j ------------------------------------------------
  double Re[9];
  qrotmat(qe, Re);
  double Sv[9];
  skew({qe.x, qe.y, qe.z}, Sv);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Jj[r * 6 + c] = Re[r * 3 + c];                                  // d te / d dt_j = R_e
      Jj[r * 6 + 3 + c] = 0.0;
      Jj[(3 + r) * 6 + c] = 0.0;
      Jj[(3 + r) * 6 + 3 + c] = (r == c ? qe.w : 0.0) + Sv[r * 3 + c];  // w_e I + [v_e]x
    }
  // ---- vertex i: E' = Z^-1 Delta_i^-1 Xi^-1 Xj ----------------------------------
  // translation: -Rz^T ; Rz^T * 2 [t_b]x
  double Stb[9];
  skew(tb, Stb);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Ji[r * 6 + c] = -Rz[c * 3 + r];
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) s += Rz[k * 3 + r] * 2.0 * Stb[k * 3 + c];
      Ji[r * 6 + 3 + c] = s;
      Ji[(3 + r) * 6 + c] = 0.0;
    }
  // rotation: q' = qz* (x) (1,-d) (x) qb ;  d q'_v / d d =
  //   wz (-wb I + [vb]x) - vz vb^T - [vz]x (-wb I + [vb]x), times the sign of q_e
  const V3 vb = {qb.x, qb.y, qb.z}, vz = {z.q.x, z.q.y, z.q.z};
  double Sb[9], Sz[9], M[9];
  skew(vb, Sb);
  skew(vz, Sz);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) M[r * 3 + c] = (r == c ? -qb.w : 0.0) + Sb[r * 3 + c];
  const double vzv[3] = {vz.x, vz.y, vz.z}, vbv[3] = {vb.x, vb.y, vb.z};
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double s = z.q.w * M[r * 3 + c] - vzv[r] * vbv[c];
#pragma unroll
      for (int k = 0; k < 3; ++k) s -= Sz[r * 3 + k] * M[k * 3 + c];
      Ji[(3 + r) * 6 + 3 + c] = sgn * s / nrm;
    }
}

// Per-edge record: [Hii(36) bi(6) | Hjj(36) bj(6) | Hoff(36) | chi2] = 121 doubles
constexpr int REC = 121;

// Robust kernels on edges, g2o's semantics (BaseBinaryEdge::constructQuadraticForm with robust_kernel_impl.cpp; g2o is not
// pinned by the reference, see the head of this file): rho = (rho0, rho1) of e2 = e^T Omega e.  The edge adds rho1 J^T Omega J
// to H, -rho1 J^T Omega e to b and rho0 to chi2; the second-order rho2 term is dropped, as g2o drops it.  DCS's rho1 is
// g2o's s^2, NOT d rho0 / d e2.
PG_DEV void robustify(int kind, double delta, double e2, double &rho0, double &rho1) {
  rho0 = e2;
  rho1 = 1.0;
  if (kind == LSLAM_PG_KERNEL_HUBER) {
    if (e2 > delta * delta) {
      const double sq = sqrt(e2);
      rho0 = 2.0 * delta * sq - delta * delta;
      rho1 = delta / sq;
    }
  } else if (kind == LSLAM_PG_KERNEL_CAUCHY) {
    const double d2 = delta * delta, a = e2 / d2 + 1.0;
    rho0 = d2 * log(a);
    rho1 = 1.0 / a;
  } else if (kind == LSLAM_PG_KERNEL_DCS) {
    const double s = 2.0 * delta / (delta + e2);
    if (!(s >= 1.0)) {
      rho0 = s * s * e2;
      rho1 = s * s;
    }
  }
}

PG_DEV double edge_e2(const double *info_e, const double er[6]) {
  double c2 = 0.0;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) s += info_e[r * 6 + c] * er[c];
    c2 += er[r] * s;
  }
  return c2;
}

// ROBUST = false is the plain solver: no kernel arrays are read and the record is e^T Omega e's.  ROBUST = true scales the
// record's 120 system entries by rho1 as they are written and stores rho0 in both chi2 slots, so assembly, the all-reduce of
// a sharded run, the PCG and the coarse level read a weighted system without knowing it.
template <bool ROBUST>
PG_DEV void edge_record(const double *poses, const int32_t *ij, const double *meas, const double *info, int e_begin,
                        int e_end, int fixed, const int32_t *kind, const double *delta, double *rec, double *chi) {
  const int e = e_begin + blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= e_end) return;
  const int i = ij[2 * e], j = ij[2 * e + 1];
  const Pose xi = load_pose(poses + 7 * i), xj = load_pose(poses + 7 * j), z = load_pose(meas + 7 * e);
  double er[6], Ji[36], Jj[36], Om[36];
  edge_error<true>(xi, xj, z, er, Ji, Jj);
#pragma unroll
  for (int k = 0; k < 36; ++k) Om[k] = info[(size_t)e * 36 + k];
  double *o = rec + (size_t)(e - e_begin) * REC;
  double c2 = 0.0, w = 1.0;
  if (ROBUST) {  // the weight is needed before the record is written; the plain instantiation computes chi2 where it always did
    const int kd = kind[e];
    robustify(kd, kd != LSLAM_PG_KERNEL_NONE ? delta[e] : 1.0, edge_e2(Om, er), c2, w);
  }
  // A = J^T Omega
  double Ai[36], Aj[36];
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double si = 0.0, sj = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        si += Ji[k * 6 + r] * Om[k * 6 + c];
        sj += Jj[k * 6 + r] * Om[k * 6 + c];
      }
      Ai[r * 6 + c] = si;
      Aj[r * 6 + c] = sj;
    }
  const bool fi = (i == fixed), fj = (j == fixed);
#pragma unroll
  for (int r = 0; r < 6; ++r) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double hii = 0.0, hjj = 0.0, hij = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        hii += Ai[r * 6 + k] * Ji[k * 6 + c];
        hjj += Aj[r * 6 + k] * Jj[k * 6 + c];
        hij += Ai[r * 6 + k] * Jj[k * 6 + c];
      }
      if (ROBUST) { hii *= w; hjj *= w; hij *= w; }
      o[r * 6 + c] = fi ? 0.0 : hii;
      o[42 + r * 6 + c] = fj ? 0.0 : hjj;
      // off-diagonal block is stored for the pair (min,max): transposed when i > j
      const double v = (fi || fj) ? 0.0 : hij;
      if (i < j) o[84 + r * 6 + c] = v; else o[84 + c * 6 + r] = v;
    }
    double bi = 0.0, bj = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      bi += Ai[r * 6 + k] * er[k];
      bj += Aj[r * 6 + k] * er[k];
    }
    if (ROBUST) { bi *= w; bj *= w; }
    o[36 + r] = fi ? 0.0 : -bi;
    o[42 + 36 + r] = fj ? 0.0 : -bj;
  }
  if (!ROBUST) {
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < 6; ++c) s += Om[r * 6 + c] * er[c];
      c2 += er[r] * s;
    }
  }
  o[120] = c2;
  chi[e - e_begin] = c2;  // also compact: the sum over the edges then reads consecutive doubles instead of one per record
}

__global__ void pg_edge_kernel(const double *poses, const int32_t *ij, const double *meas,
                               const double *info, int e_begin, int e_end, int fixed, double *rec, double *chi) {
  edge_record<false>(poses, ij, meas, info, e_begin, e_end, fixed, nullptr, nullptr, rec, chi);
}
// the same with per-edge kernels: kind / delta are indexed by GLOBAL edge id, like ij / meas / info
__global__ void pg_edge_robust_kernel(const double *poses, const int32_t *ij, const double *meas, const double *info,
                                      int e_begin, int e_end, int fixed, const int32_t *kind, const double *delta,
                                      double *rec, double *chi) {
  edge_record<true>(poses, ij, meas, info, e_begin, e_end, fixed, kind, delta, rec, chi);
}

// chi2 only (trial evaluation): per-edge value
__global__ void pg_chi2_kernel(const double *poses, const int32_t *ij, const double *meas,
                               const double *info, int e_begin, int e_end, double *out) {
  const int e = e_begin + blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= e_end) return;
  const int i = ij[2 * e], j = ij[2 * e + 1];
  const Pose xi = load_pose(poses + 7 * i), xj = load_pose(poses + 7 * j), z = load_pose(meas + 7 * e);
  double er[6];
  edge_error<false>(xi, xj, z, er, nullptr, nullptr);
  double c2 = 0.0;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) s += info[(size_t)e * 36 + r * 6 + c] * er[c];
    c2 += er[r] * s;
  }
  out[e - e_begin] = c2;
}
// trial evaluation with kernels: per-edge rho0
__global__ void pg_chi2_robust_kernel(const double *poses, const int32_t *ij, const double *meas, const double *info,
                                      int e_begin, int e_end, const int32_t *kind, const double *delta, double *out) {
  const int e = e_begin + blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= e_end) return;
  const int i = ij[2 * e], j = ij[2 * e + 1];
  const Pose xi = load_pose(poses + 7 * i), xj = load_pose(poses + 7 * j), z = load_pose(meas + 7 * e);
  double er[6];
  edge_error<false>(xi, xj, z, er, nullptr, nullptr);
  const double e2 = edge_e2(info + (size_t)e * 36, er);
  const int kd = kind[e];
  double rho0, rho1;
  robustify(kd, kd != LSLAM_PG_KERNEL_NONE ? delta[e] : 1.0, e2, rho0, rho1);
  out[e - e_begin] = rho0;
}
// Tap: per edge of the WHOLE graph (not the shard) e2, rho0 and rho1 at `poses`; kind == nullptr: no kernels, (e2, e2, 1)
__global__ void pg_edge_robust_tap_kernel(const double *poses, const int32_t *ij, const double *meas, const double *info,
                                          int n_e, const int32_t *kind, const double *delta, double *e2_out,
                                          double *rho_out, double *w_out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_e) return;
  const int i = ij[2 * e], j = ij[2 * e + 1];
  const Pose xi = load_pose(poses + 7 * i), xj = load_pose(poses + 7 * j), z = load_pose(meas + 7 * e);
  double er[6];
  edge_error<false>(xi, xj, z, er, nullptr, nullptr);
  const double e2 = edge_e2(info + (size_t)e * 36, er);
  const int kd = kind ? kind[e] : LSLAM_PG_KERNEL_NONE;
  double rho0, rho1;
  robustify(kd, kd != LSLAM_PG_KERNEL_NONE ? delta[e] : 1.0, e2, rho0, rho1);
  e2_out[e] = e2;
  rho_out[e] = rho0;
  w_out[e] = rho1;
}

// ---- unary constraints (lslam_pg_set_priors): a GPS position or an absolute pose on one vertex ------------------------------
// hdl_graph_slam's EdgeSE3PriorXYZ and g2o's EdgeSE3Prior (zero offset); neither is pinned by the reference, like the rest of
// this solver: the semantics are their published ones, in this file's conventions (update X <- X * fromVectorMQT(d)).
//   XYZ   e = t - z in the graph frame (rows 3..5 of the 6-row form below are zero), J = [R(q) | 0], Omega = the upper-left
//         3x3 of info36 (the host zeroes the rest before it is uploaded, so one code path serves both types)
//   POSE  e = toVectorMQT(Z^-1 X): the binary edge's error with Xi = identity, J = its Jj
// Per-prior record: [H(36) b(6) chi2] = 43 doubles
constexpr int PREC = 43;

template <bool JAC>
PG_DEV void prior_error(int type, const Pose &x, const Pose &z, double e[6], double *J) {
  if (type == LSLAM_PG_PRIOR_POSE) {
    const Pose id = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 1.0}};
    double Ji[36];  // of the identity "vertex": never used
    edge_error<JAC>(id, x, z, e, JAC ? Ji : nullptr, J);
    return;
  }
  e[0] = x.t.x - z.t.x; e[1] = x.t.y - z.t.y; e[2] = x.t.z - z.t.z;
  e[3] = 0.0; e[4] = 0.0; e[5] = 0.0;
  if (!JAC) return;
  double R[9];
  qrotmat(x.q, R);
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c < 6; ++c) J[r * 6 + c] = (r < 3 && c < 3) ? R[r * 3 + c] : 0.0;
}

// The record of one unary constraint from its 6-row error, Jacobian and information (a constraint with fewer rows pads with
// zeros): [rho1 J^T Omega J | -rho1 J^T Omega e | rho0], and rho0 once more into *chi.  fx: the vertex is the fixed one.
template <bool ROBUST>
PG_DEV void unary_record(const double er[6], const double J[36], const double Om[36], int kd, double dl, bool fx, double *o,
                         double *chi) {
  double c2 = edge_e2(Om, er), w = 1.0;
  if (ROBUST) robustify(kd, dl, c2, c2, w);
  double A[36];  // J^T Omega
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) s += J[k * 6 + r] * Om[k * 6 + c];
      A[r * 6 + c] = s;
    }
#pragma unroll
  for (int r = 0; r < 6; ++r) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double h = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) h += A[r * 6 + k] * J[k * 6 + c];
      if (ROBUST) h *= w;
      o[r * 6 + c] = fx ? 0.0 : h;
    }
    double bv = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) bv += A[r * 6 + k] * er[k];
    if (ROBUST) bv *= w;
    o[36 + r] = fx ? 0.0 : -bv;
  }
  o[42] = c2;
  *chi = c2;
}

// One lane per prior.  ROBUST as in edge_record: rho1 scales H and b, rho0 goes to chi2.  A prior on the fixed vertex adds its
// rho0 to chi2 and nothing to H or b (g2o: an active edge on a fixed vertex).  chi: this rank's compact per-constraint values,
// the priors' behind the edges'.
template <bool ROBUST>
PG_DEV void prior_record(const double *poses, const int32_t *pv, const int32_t *ptype, const double *pmeas,
                         const double *pinfo, int n_p, int fixed, const int32_t *kind, const double *delta, double *rec,
                         double *chi) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_p) return;
  const int v = pv[p];
  const Pose x = load_pose(poses + 7 * v), z = load_pose(pmeas + 7 * p);
  double er[6], J[36], Om[36];
  prior_error<true>(ptype[p], x, z, er, J);
#pragma unroll
  for (int k = 0; k < 36; ++k) Om[k] = pinfo[(size_t)p * 36 + k];
  int kd = LSLAM_PG_KERNEL_NONE;
  double dl = 1.0;
  if (ROBUST) {
    kd = kind[p];
    if (kd != LSLAM_PG_KERNEL_NONE) dl = delta[p];
  }
  unary_record<ROBUST>(er, J, Om, kd, dl, v == fixed, rec + (size_t)p * PREC, chi + p);
}

template <bool ROBUST>
__global__ void pg_prior_kernel(const double *poses, const int32_t *pv, const int32_t *ptype, const double *pmeas,
                                const double *pinfo, int n_p, int fixed, const int32_t *kind, const double *delta,
                                double *rec, double *chi) {
  prior_record<ROBUST>(poses, pv, ptype, pmeas, pinfo, n_p, fixed, kind, delta, rec, chi);
}

// trial evaluation: per-prior chi2 (ROBUST: rho0)
template <bool ROBUST>
__global__ void pg_prior_chi2_kernel(const double *poses, const int32_t *pv, const int32_t *ptype, const double *pmeas,
                                     const double *pinfo, int n_p, const int32_t *kind, const double *delta, double *out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_p) return;
  const Pose x = load_pose(poses + 7 * pv[p]), z = load_pose(pmeas + 7 * p);
  double er[6];
  prior_error<false>(ptype[p], x, z, er, nullptr);
  double c2 = edge_e2(pinfo + (size_t)p * 36, er), w = 1.0;
  if (ROBUST) {
    const int kd = kind[p];
    robustify(kd, kd != LSLAM_PG_KERNEL_NONE ? delta[p] : 1.0, c2, c2, w);
  }
  out[p] = c2;
}
// Tap: per prior e2, rho0 and rho1 at `poses`; kind == nullptr: no kernels, (e2, e2, 1)
__global__ void pg_prior_tap_kernel(const double *poses, const int32_t *pv, const int32_t *ptype, const double *pmeas,
                                    const double *pinfo, int n_p, const int32_t *kind, const double *delta, double *e2_out,
                                    double *rho_out, double *w_out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_p) return;
  const Pose x = load_pose(poses + 7 * pv[p]), z = load_pose(pmeas + 7 * p);
  double er[6];
  prior_error<false>(ptype[p], x, z, er, nullptr);
  const double e2 = edge_e2(pinfo + (size_t)p * 36, er);
  const int kd = kind ? kind[p] : LSLAM_PG_KERNEL_NONE;
  double rho0, rho1;
  robustify(kd, kd != LSLAM_PG_KERNEL_NONE ? delta[p] : 1.0, e2, rho0, rho1);
  e2_out[p] = e2;
  rho_out[p] = rho0;
  w_out[p] = rho1;
}

// ---- plane priors (lslam_pg_set_plane_priors): a plane known in the graph frame, measured in the sensor frame ---------------
// hdl_graph_slam's floor constraint in this file's conventions; nothing under the reference pins it, like the rest of this
// solver.  Per prior 8 doubles: the world plane (n_w, d_w) and the measured plane (n_m, d_m), both normals unit (the host
// normalises).  With X = (t, R): n_l = R^T n_w, d_l = d_w + n_w.t; a = the unit axis of the smallest |n_m| component (the lowest
// index among equals), b1 = normalise(n_m x a), b2 = n_m x b1;
//   e = (b1.n_l, b2.n_l, d_l - d_m),  J rows 0, 1 = [0 | 2 (b_k x n_l)^T], row 2 = [n_l^T | 0]
// (under X <- X fromVectorMQT(d): n_l -> n_l + 2 n_l x dq, d_l -> d_l + n_l.dt).  Rows 3..5 are zero and the information is the
// 3x3 padded to 6x6, so the record is unary_record's.
constexpr int QPL = 8;

template <bool JAC>
PG_DEV void plane_prior_error(const Pose &x, const double *pl, double e[6], double *J) {
  double R[9];
  qrotmat(x.q, R);
  const double nw[3] = {pl[0], pl[1], pl[2]}, nm[3] = {pl[4], pl[5], pl[6]};
  double nl[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) nl[c] = (R[c] * nw[0] + R[3 + c] * nw[1]) + R[6 + c] * nw[2];
  const double dl = pl[3] + ((nw[0] * x.t.x + nw[1] * x.t.y) + nw[2] * x.t.z);
  int a = 0;
  double m = fabs(nm[0]);
  if (fabs(nm[1]) < m) {
    a = 1;
    m = fabs(nm[1]);
  }
  if (fabs(nm[2]) < m) a = 2;
  const double ax[3] = {a == 0 ? 1.0 : 0.0, a == 1 ? 1.0 : 0.0, a == 2 ? 1.0 : 0.0};
  double b1[3] = {nm[1] * ax[2] - nm[2] * ax[1], nm[2] * ax[0] - nm[0] * ax[2], nm[0] * ax[1] - nm[1] * ax[0]};
  const double len = sqrt((b1[0] * b1[0] + b1[1] * b1[1]) + b1[2] * b1[2]);
#pragma unroll
  for (int c = 0; c < 3; ++c) b1[c] /= len;
  const double b2[3] = {nm[1] * b1[2] - nm[2] * b1[1], nm[2] * b1[0] - nm[0] * b1[2], nm[0] * b1[1] - nm[1] * b1[0]};
  e[0] = (b1[0] * nl[0] + b1[1] * nl[1]) + b1[2] * nl[2];
  e[1] = (b2[0] * nl[0] + b2[1] * nl[1]) + b2[2] * nl[2];
  e[2] = dl - pl[7];
  e[3] = 0.0; e[4] = 0.0; e[5] = 0.0;
  if (!JAC) return;
#pragma unroll
  for (int k = 0; k < 36; ++k) J[k] = 0.0;
  J[0 * 6 + 3] = 2.0 * (b1[1] * nl[2] - b1[2] * nl[1]);
  J[0 * 6 + 4] = 2.0 * (b1[2] * nl[0] - b1[0] * nl[2]);
  J[0 * 6 + 5] = 2.0 * (b1[0] * nl[1] - b1[1] * nl[0]);
  J[1 * 6 + 3] = 2.0 * (b2[1] * nl[2] - b2[2] * nl[1]);
  J[1 * 6 + 4] = 2.0 * (b2[2] * nl[0] - b2[0] * nl[2]);
  J[1 * 6 + 5] = 2.0 * (b2[0] * nl[1] - b2[1] * nl[0]);
  J[2 * 6 + 0] = nl[0];
  J[2 * 6 + 1] = nl[1];
  J[2 * 6 + 2] = nl[2];
}

// One lane per plane prior; the record, the fixed vertex's rule and chi as for prior_record (qinfo: 36 doubles per prior)
template <bool ROBUST>
__global__ void pg_plane_prior_kernel(const double *poses, const int32_t *qv, const double *qpl, const double *qinfo, int n_q,
                                      int fixed, const int32_t *kind, const double *delta, double *rec, double *chi) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_q) return;
  const int v = qv[p];
  const Pose x = load_pose(poses + 7 * v);
  double er[6], J[36], Om[36];
  plane_prior_error<true>(x, qpl + (size_t)p * QPL, er, J);
#pragma unroll
  for (int k = 0; k < 36; ++k) Om[k] = qinfo[(size_t)p * 36 + k];
  int kd = LSLAM_PG_KERNEL_NONE;
  double dl = 1.0;
  if (ROBUST) {
    kd = kind[p];
    if (kd != LSLAM_PG_KERNEL_NONE) dl = delta[p];
  }
  unary_record<ROBUST>(er, J, Om, kd, dl, v == fixed, rec + (size_t)p * PREC, chi + p);
}
// Trial evaluation and tap in one: per plane prior e2, rho0, rho1 at `poses`; any output may be null; kind == nullptr: no kernels
__global__ void pg_plane_prior_chi2_kernel(const double *poses, const int32_t *qv, const double *qpl, const double *qinfo, int n_q,
                                           const int32_t *kind, const double *delta, double *e2_out, double *rho_out,
                                           double *w_out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_q) return;
  const Pose x = load_pose(poses + 7 * qv[p]);
  double er[6];
  plane_prior_error<false>(x, qpl + (size_t)p * QPL, er, nullptr);
  const double e2 = edge_e2(qinfo + (size_t)p * 36, er);
  const int kd = kind ? kind[p] : LSLAM_PG_KERNEL_NONE;
  double rho0, rho1;
  robustify(kd, kd != LSLAM_PG_KERNEL_NONE ? delta[p] : 1.0, e2, rho0, rho1);
  if (e2_out) e2_out[p] = e2;
  if (rho_out) rho_out[p] = rho0;
  if (w_out) w_out[p] = rho1;
}

// fixed-order sum of n doubles into *dst, single block of 1024 (four independent accumulators per thread keep four
// loads in flight: with one, the 25 000-edge chi2 sum was a 36 us chain of dependent strided loads)
constexpr int SUM_BLOCK = 1024;
__global__ __launch_bounds__(SUM_BLOCK) void pg_sum_kernel(const double *src, int n, int stride, double *dst) {
  __shared__ double sh[SUM_BLOCK];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int k = threadIdx.x;
  for (; k + 3 * SUM_BLOCK < n; k += 4 * SUM_BLOCK) {
    const double a0 = src[(size_t)k * stride], a1 = src[(size_t)(k + SUM_BLOCK) * stride];
    const double a2 = src[(size_t)(k + 2 * SUM_BLOCK) * stride], a3 = src[(size_t)(k + 3 * SUM_BLOCK) * stride];
    s0 += a0; s1 += a1; s2 += a2; s3 += a3;
  }
  for (; k < n; k += SUM_BLOCK) s0 += src[(size_t)k * stride];
  sh[threadIdx.x] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  for (int w = SUM_BLOCK / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *dst = sh[0];
}

// Gather the per-edge records into the block system, fixed order (edge index order).
// vertex part: thread per (vertex, k<42): sum over incident shard edges.
__global__ void pg_assemble_vertex_kernel(const double *rec, const int32_t *v_ptr, const int32_t *v_adj,
                                          int n_v, int fixed, double *diag, double *b) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int v = t / 42, k = t % 42;
  if (v >= n_v) return;
  double s = 0.0;
  for (int a = v_ptr[v]; a < v_ptr[v + 1]; ++a) {
    const int code = v_adj[a];  // (local edge << 1) | role
    s += rec[(size_t)(code >> 1) * REC + (code & 1) * 42 + k];
  }
  if (v == fixed) s = (k < 36 && (k / 6 == k % 6)) ? 1.0 : 0.0;  // identity row: dx_fixed = 0
  if (k < 36) diag[(size_t)v * 36 + k] = s; else b[(size_t)v * 6 + (k - 36)] = s;
}
// The same for a graph with priors: the edge records in their order, then the vertex's prior records in prior order through
// a second CSR (p_ptr / p_adj) -- still one fixed summation order, no atomics.
__global__ void pg_assemble_vertex_prior_kernel(const double *rec, const int32_t *v_ptr, const int32_t *v_adj,
                                                const double *prec, const int32_t *p_ptr, const int32_t *p_adj, int n_v,
                                                int fixed, double *diag, double *b) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int v = t / 42, k = t % 42;
  if (v >= n_v) return;
  double s = 0.0;
  for (int a = v_ptr[v]; a < v_ptr[v + 1]; ++a) {
    const int code = v_adj[a];
    s += rec[(size_t)(code >> 1) * REC + (code & 1) * 42 + k];
  }
  for (int a = p_ptr[v]; a < p_ptr[v + 1]; ++a) s += prec[(size_t)p_adj[a] * PREC + k];
  if (v == fixed) s = (k < 36 && (k / 6 == k % 6)) ? 1.0 : 0.0;
  if (k < 36) diag[(size_t)v * 36 + k] = s; else b[(size_t)v * 6 + (k - 36)] = s;
}
// ... and with plane priors: behind the vertex's POSE / XYZ priors (p_ptr null: the graph has none), in plane-prior order
__global__ void pg_assemble_vertex_plane_kernel(const double *rec, const int32_t *v_ptr, const int32_t *v_adj,
                                                const double *prec, const int32_t *p_ptr, const int32_t *p_adj,
                                                const double *qrec, const int32_t *q_ptr, const int32_t *q_adj, int n_v,
                                                int fixed, double *diag, double *b) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int v = t / 42, k = t % 42;
  if (v >= n_v) return;
  double s = 0.0;
  for (int a = v_ptr[v]; a < v_ptr[v + 1]; ++a) {
    const int code = v_adj[a];
    s += rec[(size_t)(code >> 1) * REC + (code & 1) * 42 + k];
  }
  if (p_ptr)
    for (int a = p_ptr[v]; a < p_ptr[v + 1]; ++a) s += prec[(size_t)p_adj[a] * PREC + k];
  for (int a = q_ptr[v]; a < q_ptr[v + 1]; ++a) s += qrec[(size_t)q_adj[a] * PREC + k];
  if (v == fixed) s = (k < 36 && (k / 6 == k % 6)) ? 1.0 : 0.0;
  if (k < 36) diag[(size_t)v * 36 + k] = s; else b[(size_t)v * 6 + (k - 36)] = s;
}
__global__ void pg_assemble_off_kernel(const double *rec, const int32_t *o_ptr, const int32_t *o_adj,
                                       int n_off, double *off) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int blk = t / 36, k = t % 36;
  if (blk >= n_off) return;
  double s = 0.0;
  for (int a = o_ptr[blk]; a < o_ptr[blk + 1]; ++a) s += rec[(size_t)o_adj[a] * REC + 84 + k];
  off[(size_t)blk * 36 + k] = s;
}

// Full block-CSR copy of the symmetric system for the solver: entry a of row v refers to
// block `src` (diag: v; off: n_v + id), transposed or not.
__global__ void pg_expand_kernel(const double *sys, const int32_t *row_src, int n_entries, double lambda,
                                 double *vals) {
  // solver layout: six column planes, vals[c * n_items + entry * 6 + r] (n_items = 6 n_entries), so
  // that the product kernel's lanes (one per (entry, r)) read consecutive doubles
  const size_t n_items = (size_t)n_entries * 6;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_items * 6) return;
  const int c = (int)(t / n_items);
  const size_t item = t - (size_t)c * n_items;
  const int a = (int)(item / 6), r = (int)(item % 6);
  const int code = row_src[a];  // (block index in [diag|off] << 2) | transposed<<1 | is_diag
  const int blk = code >> 2;
  const bool tr = (code & 2) != 0, dg = (code & 1) != 0;
  double v = sys[(size_t)blk * 36 + (tr ? c * 6 + r : r * 6 + c)];
  if (dg && r == c) v += lambda;
  vals[t] = v;
}

// block-Jacobi preconditioner: inverse of the (damped) 6x6 diagonal blocks via Cholesky
__global__ void pg_precond_kernel(const double *vals, const int32_t *row_ptr, int n_v, size_t n_items,
                                  double *minv) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_v) return;
  const double *Ad = vals + (size_t)row_ptr[v] * 6;  // the diagonal entry is first in its row
  double A[36];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) A[i * 6 + j] = Ad[(size_t)j * n_items + i];
  double L[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) L[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double s = A[i * 6 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[i * 6 + k] * L[j * 6 + k];
      L[i * 6 + j] = (i == j) ? sqrt(s > 1e-300 ? s : 1e-300) : s / L[j * 6 + j];
    }
  // inverse: solve L L^T X = I column by column
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double s = (i == c) ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < i; ++k) s -= L[i * 6 + k] * y[k];
      y[i] = s / L[i * 6 + i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
      double s = y[i];
#pragma unroll
      for (int k = i + 1; k < 6; ++k) s -= L[k * 6 + i] * y[k];
      y[i] = s / L[i * 6 + i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) minv[(size_t)v * 36 + i * 6 + c] = y[i];
  }
}

// ---- PCG on the expanded block-CSR, one thread per scalar row ---------------------
// scal: [0] rz_old  [1] alpha-den (p.q)  [2] rz_new  [3] rr  [4] bb  [5] done flag (as double)
constexpr int CG_BLOCK = 128;
constexpr int CG_ROWS = 126;  // rows per block: a multiple of 6, so a vertex never straddles blocks

PG_DEV double block_sum(double v, double *sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int w = CG_BLOCK / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}
// Fixed-order sums: xor butterfly inside each wavefront (every lane ends with the same
// total), then the four wavefront totals in order.  M values at once.
template <int M, int BLOCK = CG_BLOCK>
PG_DEV void block_sum_m(double (&v)[M], double *sh /* [M * BLOCK / 64] */) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int m = 0; m < M; ++m) v[m] += __shfl_xor(v[m], off);
  constexpr int W = BLOCK / 64;
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int m = 0; m < M; ++m) sh[m * W + (threadIdx.x >> 6)] = v[m];
  __syncthreads();
#pragma unroll
  for (int m = 0; m < M; ++m) {
    double s = sh[m * W];
#pragma unroll
    for (int w = 1; w < W; ++w) s += sh[m * W + w];
    v[m] = s;
  }
  __syncthreads();
}
// sums of M per-block partial arrays, identical in every thread of every block
template <int M, int BLOCK = CG_BLOCK>
PG_DEV void sum_partials_m(const double *const (&part)[M], int n, double (&out)[M], double *sh) {
#pragma unroll
  for (int m = 0; m < M; ++m) {
    double s = 0.0;
    for (int k = threadIdx.x; k < n; k += BLOCK) s += part[m][k];
    out[m] = s;
  }
  block_sum_m<M, BLOCK>(out, sh);
}

struct CgArgs {
  const double *vals;  // six planes of n_items
  const int32_t *row_ptr, *row_col, *row_of;  // block-CSR; row_of[e] = the vertex entry e belongs to
  const double *minv;
  const double *b;
  double *x, *r, *z;
  double *d;             // [n_items] per-(entry,row) products A_e[r,:] . p[col_e]
  double *p[2];          // search direction of iteration k lives in p[k & 1]
  double *part_pq;       // [n_pblocks]
  double *part_rz[2];    // r.z entering iteration k lives in part_rz[k & 1]
  double *part_rr;       // [n_blocks]
  double *scal;          // [3] rr  [4] bb  [5] done flag  [6] iterations done
  int n6, n_blocks, n_items, n_pblocks;
  int n_parts;           // entries of part_rz[] / part_rr: n_blocks + the coarse level's blocks (zero when it is off)
  double tol2;
  // row-sharded solve (lslam_pg_set_row_shard): this rank's items [item_begin, item_end) and row blocks from block_begin on;
  // the partial arrays then hold ONE entry each, the sum over all ranks (n_parts = n_pblocks = 1)
  int item_begin, item_end, block_begin;
};

// ---- second level of the preconditioner (see solve()): CoarseArgs is in lslam_pg_internal.hpp -------------------

__global__ __launch_bounds__(CG_BLOCK) void pg_cg_init_kernel(CgArgs a) {
  __shared__ double sh[2 * CG_BLOCK / 64];
  const int row = blockIdx.x * CG_ROWS + threadIdx.x;
  double s[2] = {0.0, 0.0};
  if (threadIdx.x < CG_ROWS && row < a.n6) {
    const int v = row / 6, rr = row % 6;
    a.x[row] = 0.0;
    const double bi = a.b[row];
    a.r[row] = bi;
    double z = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) z += a.minv[(size_t)v * 36 + rr * 6 + c] * a.b[v * 6 + c];
    a.z[row] = z;
    s[0] = bi * z;
    s[1] = bi * bi;
  }
  block_sum_m<2>(s, sh);
  if (threadIdx.x == 0) {
    a.part_rz[0][blockIdx.x] = s[0];
    a.part_rr[blockIdx.x] = s[1];
  }
}
__global__ __launch_bounds__(CG_BLOCK) void pg_cg_init2_kernel(CgArgs a) {  // one block: |b|^2
  __shared__ double sh[CG_BLOCK / 64];
  const double *const parts[1] = {a.part_rr};
  double s[1];
  sum_partials_m<1>(parts, a.n_blocks, s, sh);
  if (threadIdx.x == 0) {
    a.scal[3] = s[0];
    a.scal[4] = s[0];
    a.scal[5] = (s[0] == 0.0) ? 1.0 : 0.0;
    a.scal[6] = 0.0;
  }
}

// Iteration k, first half: convergence test on the previous update, then the products
// d[e,r] = A_e[r,:] . p_k[col_e] with one lane per (entry, row) -- p_k = z + beta p_{k-1} is
// recomputed where it is needed, so no grid-wide barrier separates the direction update from
// the product -- and the partials of p_k . (A p_k) summed in item order.
constexpr int PROD_BLOCK = 256;
__global__ __launch_bounds__(PROD_BLOCK) void pg_cg_prod_kernel(CgArgs a, int k) {
  __shared__ double sh[3 * PROD_BLOCK / 64];
  if (a.scal[5] != 0.0) return;
  // operand loads first: they do not depend on beta, and the launch is latency bound
  const double *po = (k > 0) ? a.p[(k + 1) & 1] : a.z;  // k == 0: beta = 0, p_0 = z
  double *pn = a.p[k & 1];
  const int t = a.item_begin + blockIdx.x * PROD_BLOCK + threadIdx.x;
  const bool on = t < a.item_end;
  const int tt = on ? t : a.item_end - 1;
  const int e = tt / 6, r = tt - e * 6;
  const int v = a.row_of[e];
  const size_t c0 = (size_t)a.row_col[e] * 6;
  const int row = v * 6 + r;
  const bool diag = e == a.row_ptr[v];
  double A[6], zc[6], pc[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    A[c] = a.vals[(size_t)c * a.n_items + tt];
    zc[c] = a.z[c0 + c];
    pc[c] = po[c0 + c];
  }
  const double zr = a.z[row], pr0 = po[row];
  double beta = 0.0;
  if (k > 0) {
    const double *const parts[3] = {a.part_rz[k & 1], a.part_rz[(k + 1) & 1], a.part_rr};
    double s[3];
    sum_partials_m<3, PROD_BLOCK>(parts, a.n_parts, s, sh);
    if (s[2] <= a.tol2 * a.scal[4] || !(s[0] > 0.0)) {
      if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.scal[3] = s[2];
        a.scal[5] = 1.0;
      }
      return;
    }
    beta = s[0] / s[1];
  }
  double pq[1] = {0.0};
  if (on) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) s += A[c] * (zc[c] + beta * pc[c]);
    a.d[t] = s;
    const double pr = zr + beta * pr0;
    if (diag) pn[row] = pr;  // the diagonal entry publishes p_k
    pq[0] = pr * s;
  }
  block_sum_m<1, PROD_BLOCK>(pq, sh);
  if (threadIdx.x == 0) a.part_pq[blockIdx.x] = pq[0];
}
// Iteration k, second half: q = row sums of d ; x += alpha p ; r -= alpha q ; z = M r ; partial r.z, r.r
__global__ __launch_bounds__(CG_BLOCK) void pg_cg_update_kernel(CgArgs a, int k) {
  __shared__ double sh[2 * CG_BLOCK / 64];
  __shared__ double rloc[CG_BLOCK];
  if (a.scal[5] != 0.0) return;
  const int row = (a.block_begin + blockIdx.x) * CG_ROWS + threadIdx.x;
  const bool on = threadIdx.x < CG_ROWS && row < a.n6;
  const int rowc = on ? row : 0;
  const int v = rowc / 6, rrow = rowc % 6;
  // everything that does not need alpha first (latency bound launch)
  double q = 0.0;  // (A p)[row]: this row's products, in entry order
  {
    const int e0 = a.row_ptr[v], e1 = a.row_ptr[v + 1];
    for (int e = e0; e < e1; e += 4) {
      double dv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) dv[j] = a.d[(size_t)((e + j < e1) ? e + j : e1 - 1) * 6 + rrow];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < e1) q += dv[j];
    }
  }
  const double xr = a.x[rowc], pr = a.p[k & 1][rowc], rr0 = a.r[rowc];
  double mi[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) mi[c] = a.minv[(size_t)v * 36 + rrow * 6 + c];
  double s0[1], s1[1];
  {
    const double *const p0[1] = {a.part_rz[k & 1]};
    const double *const p1[1] = {a.part_pq};
    sum_partials_m<1>(p0, a.n_parts, s0, sh);
    sum_partials_m<1>(p1, a.n_pblocks, s1, sh);
  }
  const double alpha = s0[0] / s1[0];
  double rnew = 0.0;
  if (on) {
    a.x[row] = xr + alpha * pr;
    rnew = rr0 - alpha * q;
    a.r[row] = rnew;
  }
  rloc[threadIdx.x] = rnew;
  __syncthreads();
  double o[2] = {0.0, 0.0};
  if (on) {
    const int base = (int)threadIdx.x - rrow;  // this vertex's 6 residuals sit in this block
    double z = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) z += mi[c] * rloc[base + c];
    a.z[row] = z;
    o[0] = rnew * z;
    o[1] = rnew * rnew;
  }
  block_sum_m<2>(o, sh);
  if (threadIdx.x == 0) {
    a.part_rz[(k + 1) & 1][blockIdx.x] = o[0];
    a.part_rr[blockIdx.x] = o[1];
    if (blockIdx.x == 0) a.scal[6] = (double)(k + 1);
  }
}
// one block: convergence test after iteration k-1 (what pg_cg_spmv_kernel(k) would decide),
// run before the host reads the flag
__global__ __launch_bounds__(CG_BLOCK) void pg_cg_check_kernel(CgArgs a, int k) {
  __shared__ double sh[2 * CG_BLOCK / 64];
  if (a.scal[5] != 0.0) return;
  const double *const parts[2] = {a.part_rz[k & 1], a.part_rr};
  double s[2];
  sum_partials_m<2>(parts, a.n_parts, s, sh);
  if (threadIdx.x == 0) {
    a.scal[3] = s[1];
    if (s[1] <= a.tol2 * a.scal[4] || !(s[0] > 0.0)) a.scal[5] = 1.0;
  }
}

// ---- row-sharded solve (large graphs on several GPUs; lslam_pg_set_row_shard) ---------------------------------------------
// Every rank owns a contiguous range of vertex rows: it multiplies, updates and preconditions only those, and the ranks meet
// twice per iteration -- one scalar (p . A p), then the vector z with r . z and r . r behind it -- through the same all-reduce
// the linearisation uses: each rank contributes its own rows of z to a zero-padded buffer, the sum IS the gathered vector.
// The direction p_k = z + beta p_(k-1) is recomputed by every rank for ALL rows from the gathered z (an axpy of 6 n values:
// cheaper than a second exchange); every rank sees the same reduced scalars, hence takes the same decisions.
__global__ void pg_rs_direction_kernel(CgArgs a, int k) {  // p_k for every row (what pg_cg_prod_kernel recomputes per column)
  if (a.scal[5] != 0.0) return;
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= a.n6) return;
  double beta = 0.0;
  if (k > 0) {
    const double rz = a.part_rz[k & 1][0], rz_old = a.part_rz[(k + 1) & 1][0], rr = a.part_rr[0];
    if (rr <= a.tol2 * a.scal[4] || !(rz > 0.0)) return;  // pg_cg_prod_kernel ends the solve on the same numbers
    beta = rz / rz_old;
  }
  const double *po = (k > 0) ? a.p[(k + 1) & 1] : a.z;
  a.p[k & 1][row] = a.z[row] + beta * (k > 0 ? po[row] : 0.0);
}
__global__ void pg_rs_zero_others_kernel(double *v, int n6, int row_begin, int row_end) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row < n6 && (row < row_begin || row >= row_end)) v[row] = 0.0;
}
__global__ void pg_rs_pack_kernel(const double *src, double *dst, int n6, int row_begin, int row_end) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row < n6) dst[row] = (row >= row_begin && row < row_end) ? src[row] : 0.0;
}
__global__ void pg_rs_tail_sum_kernel(double *sums /* [rz, rr] */, const double *tail /* per rank: rz, rr */, int world) {
  if (threadIdx.x < 2) {  // in rank order on every rank: the same bits everywhere
    double s = 0.0;
    for (int r = 0; r < world; ++r) s += tail[2 * r + threadIdx.x];
    sums[threadIdx.x] = s;
  }
}
__global__ void pg_rs_copy_kernel(const double *src, double *d0, double *d1, double *d2) {  // up to three scalars to their slots
  if (threadIdx.x == 0) {
    if (d0) *d0 = src[0];
    if (d1) *d1 = src[1];
    if (d2) *d2 = src[2];
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Second level of the preconditioner: rigid motions of AGGREGATES of up to G keyframes that are close in the graph.
// A long trajectory bends almost for free -- moving a bundle of keyframes rigidly only strains the edges that leave
// it -- and those global modes are what block-Jacobi PCG needs thousands of iterations for once lambda is small.
// The aggregates are grown breadth-first over the graph's edges (odometry AND loop closures, lslam_pg_create), so a place
// that was visited on several laps -- keyframes tied together by loop edges -- falls into one aggregate; runs of
// consecutive keyframes instead (what this level used first) miss exactly those couplings and need six times the
// iterations on the bench graph (1 079 against 175 at lambda -> 0, numpy prototype and device agree).  The coarse
// unknown of aggregate a is a world-frame twist xi_a = (rho, phi) about the aggregate's first keyframe c_a; applied on
// the left it is, to first order, the local increment (g2o's right-multiplied [dt, dq]) delta_i = P_i xi_a of every
// keyframe i = (R_i, t_i) of the aggregate,  P_i = [ R_i^T   -R_i^T [t_i - c_a]x ;  0   R_i^T / 2 ].
// M^-1 = blockdiag(A)^-1 + P (P^T A P)^-1 P^T  (additive two-level Schwarz, symmetric positive definite).  The coarse
// matrix is dense (6 ceil(n/G) unknowns), inverted once per damped system by block Gauss-Jordan; per PCG iteration the
// level costs a restriction, a dense matrix-vector product and a prolongation.  No atomics: every sum has a fixed order,
// so the solve stays bit-reproducible and identical on every rank of a sharded run.
__global__ void pgc_P_kernel(CoarseArgs c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c.n_v) return;
  const Pose x = load_pose(c.poses + 7 * i);
  const Pose x0 = load_pose(c.poses + 7 * c.agg_mem[c.agg_ptr[c.agg_of[i]]]);
  double R[9];
  qrotmat(x.q, R);
  const double d[3] = {x.t.x - x0.t.x, x.t.y - x0.t.y, x.t.z - x0.t.z};
  // S = [d]x
  const double S[9] = {0, -d[2], d[1], d[2], 0, -d[0], -d[1], d[0], 0};
  double *P = c.P + (size_t)i * 36;
  for (int r = 0; r < 3; ++r)
    for (int col = 0; col < 3; ++col) {
      const double rt = R[col * 3 + r];  // R^T[r][col]
      double m = 0.0;                    // (R^T S)[r][col]
      for (int k = 0; k < 3; ++k) m += R[k * 3 + r] * S[k * 3 + col];
      P[r * 6 + col] = rt;
      P[r * 6 + 3 + col] = -m;
      P[(3 + r) * 6 + col] = 0.0;
      P[(3 + r) * 6 + 3 + col] = 0.5 * rt;
    }
}

// A_c[a][b] = sum over the fine entries (i, j) with i in a, j in b of P_i^T A_ij P_j; one 64-thread block per coarse block
__global__ __launch_bounds__(64) void pgc_assemble_kernel(CoarseArgs c, const double *vals, const int32_t *row_of,
                                                          const int32_t *row_col, size_t n_items) {
  __shared__ double T[36];
  const int cb = blockIdx.x, t = threadIdx.x;
  const int r = t / 6, col = t % 6;  // t < 36
  double acc = 0.0;
  for (int q = c.cb_ptr[cb]; q < c.cb_ptr[cb + 1]; ++q) {
    const int e = c.cb_ent[q];
    const int i = row_of[e], j = row_col[e];
    if (t < 36) {  // T = A_e P_j
      double s = 0.0;
      for (int l = 0; l < 6; ++l) s += vals[(size_t)l * n_items + (size_t)e * 6 + r] * c.P[(size_t)j * 36 + l * 6 + col];
      T[t] = s;
    }
    __syncthreads();
    if (t < 36) {
      for (int k = 0; k < 6; ++k) acc += c.P[(size_t)i * 36 + k * 6 + r] * T[k * 6 + col];
    }
    __syncthreads();
  }
  if (t < 36) c.Ac[(size_t)(c.cb_ab[2 * cb] * 6 + r) * c.n_c + c.cb_ab[2 * cb + 1] * 6 + col] = acc;
}

// block Gauss-Jordan, pivot block k: B = A_kk^-1, R = B A_k*, C = A_*k  (one workgroup)
__global__ __launch_bounds__(256) void pgc_gj_pivot_kernel(CoarseArgs c, int k) {
  __shared__ double B[36];
  const int n = c.n_c, t = threadIdx.x;
  if (t == 0) {  // 6x6 inverse by Gauss-Jordan with partial pivoting
    double M[6][12];
    for (int r = 0; r < 6; ++r)
      for (int q = 0; q < 6; ++q) {
        M[r][q] = c.Ac[(size_t)(k * 6 + r) * n + k * 6 + q];
        M[r][6 + q] = r == q ? 1.0 : 0.0;
      }
    for (int p = 0; p < 6; ++p) {
      int best = p;
      for (int r = p + 1; r < 6; ++r)
        if (fabs(M[r][p]) > fabs(M[best][p])) best = r;
      if (best != p)
        for (int q = 0; q < 12; ++q) { const double tmp = M[p][q]; M[p][q] = M[best][q]; M[best][q] = tmp; }
      const double inv = 1.0 / M[p][p];
      for (int q = 0; q < 12; ++q) M[p][q] *= inv;
      for (int r = 0; r < 6; ++r)
        if (r != p) {
          const double f = M[r][p];
          for (int q = 0; q < 12; ++q) M[r][q] -= f * M[p][q];
        }
    }
    for (int r = 0; r < 6; ++r)
      for (int q = 0; q < 6; ++q) { B[r * 6 + q] = M[r][6 + q]; c.Bbuf[r * 6 + q] = M[r][6 + q]; }
  }
  __syncthreads();
  for (int j = t; j < n; j += 256) {
    double a[6];
    for (int r = 0; r < 6; ++r) {
      a[r] = c.Ac[(size_t)(k * 6 + r) * n + j];
      c.Cbuf[(size_t)j * 6 + r] = c.Ac[(size_t)j * n + k * 6 + r];
    }
    for (int r = 0; r < 6; ++r) {
      double s = 0.0;
      for (int q = 0; q < 6; ++q) s += B[r * 6 + q] * a[q];
      c.Rbuf[(size_t)r * n + j] = s;
    }
  }
}
// ... and the update of every entry with it
__global__ __launch_bounds__(256) void pgc_gj_update_kernel(CoarseArgs c, int k) {
  const int n = c.n_c;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)n * n) return;
  const int i = (int)(idx / n), j = (int)(idx % n);
  const bool ik = i / 6 == k, jk = j / 6 == k;
  double v;
  if (ik && jk) {
    v = c.Bbuf[(i - k * 6) * 6 + (j - k * 6)];
  } else if (ik) {
    v = c.Rbuf[(size_t)(i - k * 6) * n + j];
  } else if (jk) {
    double s = 0.0;
    for (int m = 0; m < 6; ++m) s += c.Cbuf[(size_t)i * 6 + m] * c.Bbuf[m * 6 + (j - k * 6)];
    v = -s;
  } else {
    double s = 0.0;
    for (int m = 0; m < 6; ++m) s += c.Cbuf[(size_t)i * 6 + m] * c.Rbuf[(size_t)m * n + j];
    v = c.Ac[idx] - s;
  }
  c.Ac[idx] = v;
}

// r_c = P^T r: one wavefront per aggregate
__global__ __launch_bounds__(64) void pgc_restrict_kernel(CoarseArgs c, const double *r) {
  const int a = blockIdx.x, j = threadIdx.x;
  const int m0 = c.agg_ptr[a], m1 = c.agg_ptr[a + 1];
  double w[6] = {0, 0, 0, 0, 0, 0};
  for (int jj = j; m0 + jj < m1; jj += 64) {
    const int i = c.agg_mem[m0 + jj];
    const double *P = c.P + (size_t)i * 36;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double rk = r[(size_t)i * 6 + k];
#pragma unroll
      for (int m = 0; m < 6; ++m) w[m] += P[k * 6 + m] * rk;
    }
  }
#pragma unroll
  for (int m = 0; m < 6; ++m) {
    double s = w[m];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (j == 0) c.rc[a * 6 + m] = s;
  }
}
// y_c = A_c^-1 r_c and this block's share of r . (P y_c) = r_c . y_c; four rows per workgroup
__global__ __launch_bounds__(256) void pgc_mv_kernel(CoarseArgs c, double *part_rz_extra) {
  __shared__ double dots[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + w;
  double s = 0.0;
  if (row < c.n_c)
    for (int col = lane; col < c.n_c; col += 64) s += c.Ac[(size_t)row * c.n_c + col] * c.rc[col];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) {
    if (row < c.n_c) c.yc[row] = s;
    dots[w] = row < c.n_c ? s * c.rc[row] : 0.0;
  }
  __syncthreads();
  if (threadIdx.x == 0) part_rz_extra[blockIdx.x] = ((dots[0] + dots[1]) + dots[2]) + dots[3];
}
// The two steps above in one launch (a PCG iteration is a chain of dependent launches, each worth ~7 us): one workgroup
// per aggregate computes ITS six rows of y_c = A_c^-1 r_c, its share r_c[a] . y_c[a] of r . z, and prolongs to its members.
__global__ __launch_bounds__(256) void pgc_mvp_kernel(CoarseArgs c, double *z, double *part_rz_extra) {
  __shared__ double sh[6 * 256 / 64];
  __shared__ double y6[6];
  const int a = blockIdx.x, t = threadIdx.x;
  double s[6] = {0, 0, 0, 0, 0, 0};
  for (int col = t; col < c.n_c; col += 256) {
    const double rc = c.rc[col];
#pragma unroll
    for (int m = 0; m < 6; ++m) s[m] += c.Ac[(size_t)(a * 6 + m) * c.n_c + col] * rc;
  }
  block_sum_m<6, 256>(s, sh);  // every thread holds the six sums
  if (t == 0) {
    double dot = 0.0;
#pragma unroll
    for (int m = 0; m < 6; ++m) {
      y6[m] = s[m];
      dot += s[m] * c.rc[a * 6 + m];
    }
    part_rz_extra[a] = dot;
  }
  __syncthreads();
  const int m0 = c.agg_ptr[a], cnt = (c.agg_ptr[a + 1] - m0) * 6;
  for (int idx = t; idx < cnt; idx += 256) {
    const int i = c.agg_mem[m0 + idx / 6], r = idx % 6;
    const double *P = c.P + (size_t)i * 36 + r * 6;
    double acc = 0.0;
#pragma unroll
    for (int m = 0; m < 6; ++m) acc += P[m] * y6[m];
    z[(size_t)i * 6 + r] += acc;
  }
}
// z += P y_c
__global__ void pgc_prolong_kernel(CoarseArgs c, double *z) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= c.n_v * 6) return;
  const int i = row / 6, r = row % 6;
  const double *P = c.P + (size_t)i * 36 + r * 6;
  const double *y = c.yc + (size_t)c.agg_of[i] * 6;
  double s = 0.0;
#pragma unroll
  for (int m = 0; m < 6; ++m) s += P[m] * y[m];
  z[row] += s;
}


// ------------------------------------------------------------------------------------------------------------------
// The whole PCG solve in ONE persistent launch.  The multi-launch loop above spends a PCG iteration on four small
// dependent launches (~25-30 us: each kernel ramps up, reads its operands from L2 / Infinity Cache and drains; section 6
// of DESIGN.md); here one workgroup per AGGREGATE stays resident for the whole solve and keeps everything that does not
// change between iterations on chip -- its rows' matrix items in registers (6 doubles per (entry, row) item, PK_KREG
// items per thread), its rows of the block-Jacobi inverses and of P, in LDS its six rows of the coarse inverse -- and its
// rows' x, r, p, q in registers as well, so an iteration only moves the vectors other workgroups need and synchronises
// the grid TWICE:
//
//   phase 1   (exchange A: r.z / r.r partials and the columns' z of the previous phase 2)  beta -- every workgroup sums
//             the same partials in the same order: identical decisions everywhere, convergence included;  columns
//             p = z + beta p_old into LDS;  products of the workgroup's items, row sums q = (A p)[rows] in entry order;
//             publishes its partial p.q and the RESTRICTED q, P^T q
//   phase 2   (exchange B: p.q partials and P^T q of every aggregate)  alpha;  x += alpha p, r -= alpha q;  z = M^-1 r
//             with the block-Jacobi part local and the coarse part from  r_c(new) = r_c(old) - alpha P^T q  for ALL
//             aggregates (the same vector in every workgroup, so M^-1 is one symmetric operator; r_c(old) is the exact
//             restriction its owner published one iteration ago, so the recurrence never runs longer than one step), its own
//             six rows of A_c^-1 r_c, prolonged to its rows;  publishes z, the exact restriction of its new residual and
//             the partials r.z, r.r
//
// An exchange is barrier and data in one: what other workgroups read travels through relaxed agent-scope atomic stores /
// loads (written through to, and read from, the device's coherence point -- no cache write-back / invalidate: an acquire
// at agent scope empties the XCD's L2, after which every operand of the next phase, register spills included, came from
// the fabric: tools/ubench_gridbar.hip, 6.2 us per counter barrier with a published value against 2.7 us without the
// cache maintenance), and the values a phase waits for live in slots that hold a SENTINEL (a NaN payload no computation
// produces) until their owner publishes them: a reader polls the slots themselves, one round trip when everybody is
// on time, instead of a counter barrier (136 serialised atomics) followed by the loads.  Slots are double-buffered by
// iteration parity and reset by their owner one exchange after everybody has read them (a workgroup that has published
// exchange j+1 has finished reading exchange j); values that are not polled (p, the exact r_c) are complete before the
// polled ones are stored (an explicit s_waitcnt vmcnt(0) in every wavefront, then a workgroup barrier), so whoever sees the
// latter can read the former.
//
// Every sum has a fixed order: the solve is bit-reproducible and identical on every rank of a sharded run.  A spin limit
// raises an abort flag instead of hanging.  Used when the graph fits (one workgroup per aggregate co-resident, LDS for
// its columns and items); otherwise the multi-launch loop runs.
// ------------------------------------------------------------------------------------------------------------------
constexpr int PG_COARSE_MAX = 6144;        // coarse unknowns (1 024 aggregates): the dense inverse is 302 MB and O(n_c^3) beyond that is no preconditioner
constexpr int PK_BLOCK = 512;
constexpr int PG_AGG_MAX = 85;             // members of an aggregate: its 6 x 85 rows have a thread each in the persistent kernel
constexpr int PK_ROWS = 6 * PG_AGG_MAX;
constexpr int PK_W = PK_BLOCK / 64;
constexpr int PK_KREG = 9;   // matrix items per thread kept in registers (more are streamed from memory)
constexpr int PK_CM = 3;     // column values per thread whose p_old is fetched ahead of the poll
constexpr unsigned PK_SPIN_LIMIT = 1u << 20;
constexpr unsigned PK_SENT32 = 0xFFF8DEADu;  // both halves of the sentinel double (hipMemsetD32)
constexpr long long PK_SENT = (long long)(((unsigned long long)PK_SENT32 << 32) | PK_SENT32);

struct PkArgs {
  const double *vals, *minv, *b;
  double *x, *p0, *p1;
  const int32_t *agg_ptr, *agg_mem;     // aggregate -> member vertices
  const int32_t *bent_ptr, *bent, *blc; // aggregate -> its rows' entries (global entry id, local column), member by member
  const int32_t *bmptr;                 // per aggregate nm + 1 offsets: member -> its first local entry
  const int32_t *bcol_ptr, *bcol;       // aggregate -> the vertices its entries' columns refer to
  const double *P, *Ainv;
  double *rc0, *rc1;                    // exact restricted residual, by iteration parity
  double *zA, *rzA, *rrA;               // exchange A slots: [2][n6], [2][n_agg], [2][n_agg]
  double *pqB, *qcB;                    // exchange B slots: [2][n_agg], [2][n_c]
  double *scal;
  unsigned *bar;                        // [0] arrivals of the set-up barrier  [1] abort flag
  size_t n_items;
  int n6, n_agg, n_c, coarse, max_iter, lds_cols, lds_items;
  int debug_abort;                      // tests: workgroup 0 raises the abort flag at this iteration (-1: never)
  double tol2;
};

#ifdef LSLAM_PK_CLOCKS  // profiling build: where an iteration of the persistent kernel spends its time (workgroup 0)
#define PK_T(i) { const unsigned long long _n = wall_clock64(); pk_t[i] += _n - pk_last; pk_last = _n; }
#else
#define PK_T(i)
#endif
PG_DEV double pk_ld(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
PG_DEV void pk_st(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
PG_DEV bool pk_is_sent(double v) { return __double_as_longlong(v) == PK_SENT; }
PG_DEV double pk_sent() { return __longlong_as_double(PK_SENT); }
PG_DEV bool pk_aborted(unsigned *bar) { return __hip_atomic_load(bar + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u; }
PG_DEV void pk_abort(unsigned *bar) { __hip_atomic_store(bar + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// counter barrier of the set-up (once per solve)
PG_DEV bool pk_grid_barrier(unsigned *bar, unsigned target, int *ok_lds) {
  __builtin_amdgcn_s_waitcnt(0);  // this wavefront's published values are at the coherence point
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned spins = 0;
    int good = 1;
    while (__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      __builtin_amdgcn_s_sleep(1);
      ++spins;
      if ((spins & 1023u) == 0 && (spins > PK_SPIN_LIMIT || pk_aborted(bar))) {
        pk_abort(bar);
        good = 0;
        break;
      }
    }
    *ok_lds = good;
  }
  __syncthreads();
  return *ok_lds != 0;
}

// Sums of up to eight per-thread values over the workgroup, fixed order, every thread ends with the totals.  Inside a
// wavefront a butterfly that HALVES the values it carries at each of its first three steps: partners lane ^ 1 split the
// eight values (the even lane adds both lanes' first four, the odd lane the last four), lane ^ 2 split the four, lane ^ 4
// the two -- 4 + 2 + 1 additions instead of 3 x 8 -- then lane ^ 8, ^ 16, ^ 32 on the one value left: lane l ends with the
// wavefront's sum of value 4 (l & 1) + 2 (l >> 1 & 1) + (l >> 2 & 1).  The moves are DPP quad permutes, ds_swizzle and one
// ds_bpermute; the eight wavefronts' sums meet in LDS and are added by a second, three-step butterfly.
// (__shfl_xor on doubles is two ds_bpermute round trips per step and value: 3 us for seven values.)
template <int CTRL>
PG_DEV double pk_dpp(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
template <int PATTERN>
PG_DEV double pk_swz(double v) {  // ds_swizzle, bit mode: lane ^ (PATTERN >> 10) inside each half of the wavefront
  return __hiloint2double(__builtin_amdgcn_ds_swizzle(__double2hiint(v), PATTERN), __builtin_amdgcn_ds_swizzle(__double2loint(v), PATTERN));
}
template <int M>
PG_DEV void pk_reduce(double (&v)[M], double *sh) {
  static_assert(M <= 8, "at most eight values");
  const int lane = threadIdx.x & 63;
  double t8[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) t8[m] = m < M ? v[m] : 0.0;
  double t4[4], t2[2], t;
  {
    const bool hi = (lane & 1) != 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) t4[i] = (hi ? t8[4 + i] : t8[i]) + pk_dpp<0xB1>(hi ? t8[i] : t8[4 + i]);  // quad_perm [1,0,3,2]
  }
  {
    const bool hi = (lane & 2) != 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) t2[i] = (hi ? t4[2 + i] : t4[i]) + pk_dpp<0x4E>(hi ? t4[i] : t4[2 + i]);  // quad_perm [2,3,0,1]
  }
  {
    const bool hi = (lane & 4) != 0;
    t = (hi ? t2[1] : t2[0]) + pk_swz<0x101F>(hi ? t2[0] : t2[1]);  // lane ^ 4
  }
  t += pk_swz<0x201F>(t);  // lane ^ 8
  t += pk_swz<0x401F>(t);  // lane ^ 16
  t += __shfl_xor(t, 32);  // lane ^ 32
  if (lane < 8) sh[(4 * (lane & 1) + 2 * ((lane >> 1) & 1) + ((lane >> 2) & 1)) * PK_W + (threadIdx.x >> 6)] = t;
  __syncthreads();
  // lane l takes the sum of wavefront l & 7 for value l >> 3; three butterfly steps over the wavefront index leave every
  // lane of the group with the value's total, broadcast from lane 8 m
  static_assert(PK_W == 8, "eight wavefronts");
  double u = sh[lane];
  u += pk_dpp<0xB1>(u);
  u += pk_dpp<0x4E>(u);
  u += pk_swz<0x101F>(u);
#pragma unroll
  for (int m = 0; m < M; ++m)
    v[m] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(u), 8 * m), __builtin_amdgcn_readlane(__double2loint(u), 8 * m));
  __syncthreads();
}

__global__ __launch_bounds__(PK_BLOCK) void pg_pcg_persistent_kernel(PkArgs a) {
#pragma clang fp contract(fast)  // fused multiply-adds here (the library is built with -ffp-contract=off for the fp32 parity paths)
  extern __shared__ double pk_lds[];
  double *pf = pk_lds;                           // [lds_cols * 6] the columns' p
  double *dl = pf + (size_t)a.lds_cols * 6;      // [lds_items] products
  double *rloc = dl + a.lds_items;               // [PK_ROWS] residuals of the rows
  double *rcs = rloc + PK_ROWS;                  // [n_c] restricted residual
  double *ainv = rcs + a.n_c;                    // [6 * n_c] this aggregate's rows of the coarse inverse
  double *sh = ainv + 6 * (size_t)a.n_c;         // [8 * PK_W] wavefront sums
  __shared__ int bar_ok;
  const int ag = blockIdx.x, tid = threadIdx.x;
  const int m0 = a.agg_ptr[ag], nm = a.agg_ptr[ag + 1] - m0, nrow = nm * 6;
  const int e0 = a.bent_ptr[ag], nit = (a.bent_ptr[ag + 1] - e0) * 6;
  const int c0 = a.bcol_ptr[ag], ncol6 = (a.bcol_ptr[ag + 1] - c0) * 6;
  const bool coarse = a.coarse != 0;

  // ---- what stays on chip for the whole solve ----
  // a thread's items come in units of three consecutive rows of one entry (unit u = tid + PK_BLOCK ju holds items
  // 3 u .. 3 u + 2): the three share the entry's column, fetched from LDS once
  static_assert(PK_KREG % 3 == 0, "items in units of three rows");
  double A[PK_KREG][6];
  int lcol[PK_KREG];
#pragma unroll
  for (int j = 0; j < PK_KREG; ++j) {
    const int i = 3 * (tid + PK_BLOCK * (j / 3)) + j % 3;
    const bool on = i < nit;
    const int le = on ? i / 6 : 0, r = on ? i - le * 6 : 0;
    const int e = on ? a.bent[e0 + le] : 0;
    lcol[j] = on ? a.blc[e0 + le] * 6 : 0;
#pragma unroll
    for (int c = 0; c < 6; ++c) A[j][c] = on ? a.vals[(size_t)c * a.n_items + (size_t)e * 6 + r] : 0.0;
  }
  const bool isrow = tid < nrow;
  const int jm = tid / 6, rr = tid - jm * 6;
  const int v = isrow ? a.agg_mem[m0 + jm] : 0;
  const int row = v * 6 + rr;
  double mi[6], Pr[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    mi[c] = isrow ? a.minv[(size_t)v * 36 + rr * 6 + c] : 0.0;
    Pr[c] = (isrow && coarse) ? a.P[(size_t)v * 36 + rr * 6 + c] : 0.0;
  }
  const int le_b = isrow ? a.bmptr[m0 + ag + jm] : 0, le_e = isrow ? a.bmptr[m0 + ag + jm + 1] : 0;
  size_t gcol[PK_CM];  // the global (vertex, component) of the column values this thread fetches
#pragma unroll
  for (int j = 0; j < PK_CM; ++j) {
    const int i = tid + PK_BLOCK * j;
    const int ci = i < ncol6 ? i / 6 : 0;
    gcol[j] = i < ncol6 ? (size_t)a.bcol[c0 + ci] * 6 + (i - ci * 6) : 0;
  }
  if (coarse)
    for (int i = tid; i < 6 * a.n_c; i += PK_BLOCK) ainv[i] = a.Ainv[(size_t)ag * 6 * a.n_c + i];
  // y = this aggregate's six rows of A_c^-1 times rcs (both in LDS); every thread ends with the six sums
  auto coarse_rows = [&](double (&s)[6]) {
#pragma unroll
    for (int m = 0; m < 6; ++m) s[m] = 0.0;
    for (int col = tid; col < a.n_c; col += PK_BLOCK) {
      const double rcv = rcs[col];
#pragma unroll
      for (int m = 0; m < 6; ++m) s[m] += ainv[m * a.n_c + col] * rcv;
    }
    pk_reduce<6>(s, sh);
  };

  // ---- x = 0, r = b, z = M^-1 r ----
  double x = 0.0, r = isrow ? a.b[row] : 0.0, q = 0.0, p_own = 0.0, z_own = 0.0;
  if (tid < PK_ROWS) rloc[tid] = r;
  __syncthreads();
  {
    double zj = 0.0;
    if (isrow) {
#pragma unroll
      for (int c = 0; c < 6; ++c) zj += mi[c] * rloc[jm * 6 + c];
    }
    z_own = zj;
  }
  if (coarse) {
    double w[6];
#pragma unroll
    for (int m = 0; m < 6; ++m) w[m] = Pr[m] * r;
    pk_reduce<6>(w, sh);
    if (tid == 0) {
#pragma unroll
      for (int m = 0; m < 6; ++m) pk_st(a.rc0 + ag * 6 + m, w[m]);
    }
    if (!pk_grid_barrier(a.bar, gridDim.x, &bar_ok)) return;
    for (int col = tid; col < a.n_c; col += PK_BLOCK) rcs[col] = pk_ld(a.rc0 + col);
    __syncthreads();
    double y[6];
    coarse_rows(y);
#pragma unroll
    for (int m = 0; m < 6; ++m) z_own += Pr[m] * y[m];
  }
  {  // exchange A of iteration 0
    if (isrow) pk_st(a.zA + row, z_own);
    double o[2] = {r * z_own, r * r};
    pk_reduce<2>(o, sh);
    if (tid == 0) {
      pk_st(a.rzA + ag, o[0]);
      pk_st(a.rrA + ag, o[1]);
    }
  }

  double rz_old = 0.0, bb = 0.0, rr_last = 0.0;
  int k = 0, done = 0;
#ifdef LSLAM_PK_CLOCKS
  unsigned long long pk_t[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, pk_last = wall_clock64();
#endif
  for (;;) {
    const int g = k & 1;
    // ---- phase 1: exchange A ----
    const double *po = g ? a.p0 : a.p1;  // p of iteration k - 1 (complete: published before exchange B of k - 1)
    double *pn = g ? a.p1 : a.p0;
    double ppv[PK_CM];
#pragma unroll
    for (int j = 0; j < PK_CM; ++j) ppv[j] = (k > 0 && tid + PK_BLOCK * j < ncol6) ? pk_ld(po + gcol[j]) : 0.0;
    double S[2];
    {
      const double *zg = a.zA + (size_t)g * a.n6, *rzg = a.rzA + g * a.n_agg, *rrg = a.rrA + g * a.n_agg;
      for (unsigned spins = 0;; ++spins) {
        int bad = 0;
        S[0] = S[1] = 0.0;
        if (tid < a.n_agg) {
          S[0] = pk_ld(rzg + tid);
          S[1] = pk_ld(rrg + tid);
          bad |= (pk_is_sent(S[0]) || pk_is_sent(S[1])) ? 1 : 0;
        }
#pragma unroll
        for (int j = 0; j < PK_CM; ++j) {
          const int i = tid + PK_BLOCK * j;
          if (i < ncol6) {
            const double zz = pk_ld(zg + gcol[j]);
            pf[i] = zz;
            bad |= pk_is_sent(zz) ? 1 : 0;
          }
        }
        for (int i = tid + PK_BLOCK * PK_CM; i < ncol6; i += PK_BLOCK) {
          const int ci = i / 6;
          const double zz = pk_ld(zg + (size_t)a.bcol[c0 + ci] * 6 + (i - ci * 6));
          pf[i] = zz;
          bad |= pk_is_sent(zz) ? 1 : 0;
        }
        if (!__syncthreads_or(bad)) break;
        if ((spins & 255u) == 255u && (spins > PK_SPIN_LIMIT || pk_aborted(a.bar))) {
          pk_abort(a.bar);
          return;
        }
        __builtin_amdgcn_s_sleep(1);
      }
    }
    if (k > 0 && tid == 0) {  // everybody has read exchange B of iteration k - 1: its slots are free again
      double *pq = a.pqB + (g ^ 1) * a.n_agg, *qc = a.qcB + (size_t)(g ^ 1) * a.n_c;
      pk_st(pq + ag, pk_sent());
#pragma unroll
      for (int m = 0; m < 6; ++m) pk_st(qc + ag * 6 + m, pk_sent());
    }
    pk_reduce<2>(S, sh);
    PK_T(0)
    if (k == 0) bb = S[1];
    rr_last = S[1];
    if (S[1] <= a.tol2 * bb || !(S[0] > 0.0)) {
      done = 1;
      break;
    }
    if (k >= a.max_iter) break;
    if (k == a.debug_abort && ag == 0 && tid == 0) pk_abort(a.bar);
    const double beta = k > 0 ? S[0] / rz_old : 0.0;
#pragma unroll
    for (int j = 0; j < PK_CM; ++j) {
      const int i = tid + PK_BLOCK * j;
      if (i < ncol6) pf[i] += beta * ppv[j];
    }
    if (k > 0)
      for (int i = tid + PK_BLOCK * PK_CM; i < ncol6; i += PK_BLOCK) {
        const int ci = i / 6;
        pf[i] += beta * pk_ld(po + (size_t)a.bcol[c0 + ci] * 6 + (i - ci * 6));
      }
    if (isrow) {
      p_own = z_own + beta * p_own;
      pk_st(pn + row, p_own);
    }
    __syncthreads();
    PK_T(1)
#pragma unroll
    for (int ju = 0; ju < PK_KREG / 3; ++ju) {
      const int i0 = 3 * (tid + PK_BLOCK * ju);
      if (i0 < nit) {  // (the items of an entry come in sixes: a unit is whole or absent)
        double pc[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) pc[c] = pf[lcol[3 * ju] + c];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          double s = 0.0;
#pragma unroll
          for (int c = 0; c < 6; ++c) s += A[3 * ju + k][c] * pc[c];
          dl[i0 + k] = s;
        }
      }
      __builtin_amdgcn_sched_barrier(0);  // one unit's operands in flight, not all of them (register pressure)
    }
    for (int i = 3 * PK_BLOCK * (PK_KREG / 3) + tid; i < nit; i += PK_BLOCK) {  // an aggregate with more items than the registers hold
      const int le = i / 6, rw = i - le * 6;
      const int e = a.bent[e0 + le], lc = a.blc[e0 + le] * 6;
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < 6; ++c) s += a.vals[(size_t)c * a.n_items + (size_t)e * 6 + rw] * pf[lc + c];
      dl[i] = s;
    }
    __syncthreads();
    PK_T(2)
    q = 0.0;
    for (int le = le_b; le < le_e; ++le) q += dl[le * 6 + rr];
    {
      double w[7];
#pragma unroll
      for (int m = 0; m < 6; ++m) w[m] = Pr[m] * q;
      w[6] = p_own * q;
      // Everything this workgroup stored without a sentinel -- every wavefront's p, the exact r_c and the sentinel resets of the
      // previous phase -- must be at the coherence point before the polled slots below are filled: whoever sees those may read
      // the former.  The compiler's own wait ahead of a workgroup barrier covers LDS only (s_waitcnt lgkmcnt(0)), so every
      // wavefront waits for its outstanding vector-memory operations explicitly (they were issued a phase ago: no stall).
      __builtin_amdgcn_s_waitcnt(0);
      pk_reduce<7>(w, sh);  // (its workgroup barrier: nobody fills a slot before every wavefront has waited)
      if (tid == 0) {
        double *qc = a.qcB + (size_t)g * a.n_c;
#pragma unroll
        for (int m = 0; m < 6; ++m) pk_st(qc + ag * 6 + m, w[m]);
        pk_st(a.pqB + g * a.n_agg + ag, w[6]);
      }
    }
    PK_T(3)
    // ---- phase 2: exchange B ----
    const double *rco = g ? a.rc1 : a.rc0;  // exact r_c entering this iteration (complete: published before exchange A)
    double rcv[2] = {0.0, 0.0}, qcv[2] = {0.0, 0.0};
    if (coarse) {
#pragma unroll
      for (int jc = 0; jc < 2; ++jc) {
        const int col = tid + PK_BLOCK * jc;
        if (col < a.n_c) rcv[jc] = pk_ld(rco + col);
      }
    }
    double Spq[1];
    {
      const double *pq = a.pqB + g * a.n_agg, *qc = a.qcB + (size_t)g * a.n_c;
      for (unsigned spins = 0;; ++spins) {
        int bad = 0;
        Spq[0] = 0.0;
        if (tid < a.n_agg) {
          Spq[0] = pk_ld(pq + tid);
          bad |= pk_is_sent(Spq[0]) ? 1 : 0;
        }
        if (coarse) {
#pragma unroll
          for (int jc = 0; jc < 2; ++jc) {
            const int col = tid + PK_BLOCK * jc;
            if (col < a.n_c) {
              qcv[jc] = pk_ld(qc + col);
              bad |= pk_is_sent(qcv[jc]) ? 1 : 0;
            }
          }
          for (int col = tid + 2 * PK_BLOCK; col < a.n_c; col += PK_BLOCK) {
            const double t = pk_ld(qc + col);
            rcs[col] = t;
            bad |= pk_is_sent(t) ? 1 : 0;
          }
        }
        if (!__syncthreads_or(bad)) break;
        if ((spins & 255u) == 255u && (spins > PK_SPIN_LIMIT || pk_aborted(a.bar))) {
          pk_abort(a.bar);
          return;
        }
        __builtin_amdgcn_s_sleep(1);
      }
    }
    PK_T(4)
    {  // everybody has read exchange A of this iteration: its slots are free again
      double *zg = a.zA + (size_t)g * a.n6;
      if (isrow) pk_st(zg + row, pk_sent());
      if (tid == 0) {
        pk_st(a.rzA + g * a.n_agg + ag, pk_sent());
        pk_st(a.rrA + g * a.n_agg + ag, pk_sent());
      }
    }
    pk_reduce<1>(Spq, sh);
    PK_T(5)
    const double alpha = S[0] / Spq[0];
    x += alpha * p_own;
    r -= alpha * q;
    if (tid < PK_ROWS) rloc[tid] = r;
    if (coarse) {
#pragma unroll
      for (int jc = 0; jc < 2; ++jc) {
        const int col = tid + PK_BLOCK * jc;
        if (col < a.n_c) rcs[col] = rcv[jc] - alpha * qcv[jc];
      }
      for (int col = tid + 2 * PK_BLOCK; col < a.n_c; col += PK_BLOCK) rcs[col] = pk_ld(rco + col) - alpha * rcs[col];
    }
    __syncthreads();
    PK_T(6)
    {
      double zj = 0.0;
      if (isrow) {
#pragma unroll
        for (int c = 0; c < 6; ++c) zj += mi[c] * rloc[jm * 6 + c];
      }
      z_own = zj;
    }
    if (coarse) {
      double y[6];
      coarse_rows(y);
#pragma unroll
      for (int m = 0; m < 6; ++m) z_own += Pr[m] * y[m];
    }
    PK_T(7)
    // the sentinel resets of exchange A's slots (start of this phase) are complete before this workgroup publishes anything
    // of exchange A of the next iteration; the z stores below are polled themselves and stay in flight behind it
    __builtin_amdgcn_s_waitcnt(0);
    if (isrow) pk_st(a.zA + (size_t)(g ^ 1) * a.n6 + row, z_own);  // exchange A of iteration k + 1
    {
      double o[8];
#pragma unroll
      for (int m = 0; m < 6; ++m) o[m] = Pr[m] * r;
      o[6] = r * z_own;
      o[7] = r * r;
      pk_reduce<8>(o, sh);
      if (tid == 0) {
        double *rcn = g ? a.rc0 : a.rc1;
#pragma unroll
        for (int m = 0; m < 6; ++m) pk_st(rcn + ag * 6 + m, o[m]);
        // (the exact r_c is read after exchange B of the next iteration, which this workgroup publishes several workgroup
        // barriers from here: complete by then)
        pk_st(a.rzA + (g ^ 1) * a.n_agg + ag, o[6]);
        pk_st(a.rrA + (g ^ 1) * a.n_agg + ag, o[7]);
      }
    }
    rz_old = S[0];
    PK_T(8)
    ++k;
  }
  if (isrow) a.x[row] = x;
  if (ag == 0 && tid == 0) {
    a.scal[3] = rr_last;
    a.scal[4] = bb;
    a.scal[5] = done ? 1.0 : 0.0;
    a.scal[6] = (double)k;
#ifdef LSLAM_PK_CLOCKS
    for (int i = 0; i < 12; ++i) a.scal[8 + i] += (double)pk_t[i];  // 100 MHz ticks, accumulated over the solves
#endif
  }
}


// ------------------------------------------------------------------------------------------------------------------
// The coarse inverse in ONE persistent launch.  The two-launch-per-pivot loop above (pgc_gj_pivot_kernel: one workgroup,
// a serial 6 x 6 inverse, 29 us; pgc_gj_update_kernel: 7 us) costs 136 x 36 us = 4.9 ms per inverse on the bench graph,
// a quarter of the whole LM run once the PCG iterations are fused.  Here workgroup i owns block row i of the matrix
// (6 x n_c doubles, in registers, GJ_CREG columns per thread) for the whole elimination.  At step k the pivot's owner
// inverts A_kk (36 lanes, in-place Gauss-Jordan in LDS; the pivot blocks of an SPD matrix need no pivoting), scales its
// row, R = A_kk^-1 A_k*, and publishes it -- with A_kk^-1 itself in the pivot's own columns -- into slot k of a buffer
// that holds a sentinel until then; every other workgroup polls that slot for its own columns (barrier and data in one
// round trip, as in pg_pcg_persistent_kernel) and updates its row:  A_i* <- A_i* - A_ik R  (its pivot columns: -A_ik A_kk^-1).
// Same arithmetic as the launch-per-pivot form up to the 6 x 6 inverse's pivoting.
// ------------------------------------------------------------------------------------------------------------------
constexpr int GJ_BLOCK = 512;
constexpr int GJ_CREG = 4;
struct GjArgs {
  int debug_abort; // tests: workgroup 0 raises the abort flag at this pivot step (-1: never)
  double *Ac;      // [n_c][n_c], inverted in place
  double *slots;   // [na][6][n_c], sentinel-filled
  unsigned *bar;   // [1] abort flag
  int n_c, na;
};
__global__ __launch_bounds__(GJ_BLOCK) void pgc_gj_persistent_kernel(GjArgs g) {
#pragma clang fp contract(fast)
  __shared__ double Cb[36];
  __shared__ double Mb[36];
  const int i = blockIdx.x, tid = threadIdx.x, n = g.n_c;
  double A[GJ_CREG][6];
#pragma unroll
  for (int jc = 0; jc < GJ_CREG; ++jc) {
    const int col = tid + GJ_BLOCK * jc;
#pragma unroll
    for (int r = 0; r < 6; ++r) A[jc][r] = col < n ? g.Ac[(size_t)(i * 6 + r) * n + col] : 0.0;
  }
  for (int k = 0; k < g.na; ++k) {
    const int k6 = k * 6;
    double *slot = g.slots + (size_t)k * 6 * n;
    if (k == g.debug_abort && i == 0 && tid == 0) pk_abort(g.bar);
    if (i == k) {
#pragma unroll
      for (int jc = 0; jc < GJ_CREG; ++jc) {
        const int col = tid + GJ_BLOCK * jc;
        if (col >= k6 && col < k6 + 6) {
#pragma unroll
          for (int r = 0; r < 6; ++r) Mb[r * 6 + (col - k6)] = A[jc][r];
        }
      }
      __syncthreads();
      if (tid < 64) {  // in-place Gauss-Jordan on the 6 x 6 block, one lane per element (LDS serves a wavefront's accesses in order)
        volatile double *M = Mb;
        const int r = tid / 6, c = tid - r * 6;
#pragma unroll
        for (int p = 0; p < 6; ++p) {
          double nv = 0.0;
          if (tid < 36) {
            const double inv = 1.0 / M[p * 6 + p];
            const double mpc = M[p * 6 + c], mrp = M[r * 6 + p], mrc = M[r * 6 + c];
            if (r == p) nv = (c == p) ? inv : mpc * inv;
            else nv = (c == p) ? -(mrp * inv) : mrc - mrp * (mpc * inv);
          }
          __builtin_amdgcn_wave_barrier();
          if (tid < 36) M[tid] = nv;
          __builtin_amdgcn_wave_barrier();
        }
      }
      __syncthreads();
#pragma unroll
      for (int jc = 0; jc < GJ_CREG; ++jc) {
        const int col = tid + GJ_BLOCK * jc;
        if (col < n) {
          const bool ink = col >= k6 && col < k6 + 6;
          double Rv[6];
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            double t = 0.0;
#pragma unroll
            for (int q = 0; q < 6; ++q) t += Mb[r * 6 + q] * A[jc][q];
            Rv[r] = ink ? Mb[r * 6 + (col - k6)] : t;
          }
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            A[jc][r] = Rv[r];
            pk_st(slot + (size_t)r * n + col, Rv[r]);
          }
        }
      }
      __syncthreads();
    } else {
#pragma unroll
      for (int jc = 0; jc < GJ_CREG; ++jc) {
        const int col = tid + GJ_BLOCK * jc;
        if (col >= k6 && col < k6 + 6) {
#pragma unroll
          for (int r = 0; r < 6; ++r) Cb[r * 6 + (col - k6)] = A[jc][r];
        }
      }
      double Rv[GJ_CREG][6];
      for (unsigned spins = 0;; ++spins) {
        int bad = 0;
#pragma unroll
        for (int jc = 0; jc < GJ_CREG; ++jc) {
          const int col = tid + GJ_BLOCK * jc;
#pragma unroll
          for (int m = 0; m < 6; ++m) {
            Rv[jc][m] = col < n ? pk_ld(slot + (size_t)m * n + col) : 0.0;
            bad |= pk_is_sent(Rv[jc][m]) ? 1 : 0;
          }
        }
        if (!__syncthreads_or(bad)) break;  // (its barrier also makes Cb visible)
        if ((spins & 255u) == 255u && (spins > PK_SPIN_LIMIT || pk_aborted(g.bar))) {
          pk_abort(g.bar);
          return;
        }
        __builtin_amdgcn_s_sleep(1);
      }
#pragma unroll
      for (int jc = 0; jc < GJ_CREG; ++jc) {
        const int col = tid + GJ_BLOCK * jc;
        const bool ink = col >= k6 && col < k6 + 6;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          double t = 0.0;
#pragma unroll
          for (int m = 0; m < 6; ++m) t += Cb[r * 6 + m] * Rv[jc][m];
          A[jc][r] = (ink ? 0.0 : A[jc][r]) - t;
        }
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int jc = 0; jc < GJ_CREG; ++jc) {
    const int col = tid + GJ_BLOCK * jc;
    if (col < n) {
#pragma unroll
      for (int r = 0; r < 6; ++r) g.Ac[(size_t)(i * 6 + r) * n + col] = A[jc][r];
    }
  }
}

// X <- X * fromVectorMQT(dx)
__global__ void pg_update_kernel(const double *src, const double *dx, int n_v, int fixed, double *dst) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_v) return;
  if (v == fixed) {  // g2o never touches a fixed vertex: copied, not renormalised (|q| = 1 +- 1 ulp would drift per accepted step)
#pragma unroll
    for (int k = 0; k < 7; ++k) dst[7 * v + k] = src[7 * v + k];
    return;
  }
  const Pose x = load_pose(src + 7 * v);
  double d[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) d[k] = dx[v * 6 + k];
  const double w2 = 1.0 - (d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
  Q4 dq = {d[3], d[4], d[5], sqrt(w2 > 0 ? w2 : 0.0)};
  if (w2 < 0) dq = {0, 0, 0, 1};
  double R[9];
  qrotmat(x.q, R);
  const V3 t = mulR(R, {d[0], d[1], d[2]});
  Q4 q = qmul(x.q, dq);
  const double n = sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  double *o = dst + 7 * v;
  o[0] = x.t.x + t.x; o[1] = x.t.y + t.y; o[2] = x.t.z + t.z;
  o[3] = q.x / n; o[4] = q.y / n; o[5] = q.z / n; o[6] = q.w / n;
}

// [J_ref | J_j] of an edge (ref, v[k]) whose measurement is the current relative pose X_ref^-1 X_j, so that its error is zero:
// what lslam_pg_relative_covariances propagates the joint covariance of the two vertices through (lslam_pg_marginals.hip)
__global__ void pg_rel_jac_kernel(const double *poses, int ref, int n, const int32_t *v, double *J72) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const Pose xi = load_pose(poses + 7 * ref), xj = load_pose(poses + 7 * v[k]);
  double Ri[9];
  qrotmat(xi.q, Ri);
  Pose z;
  z.t = mulRt(Ri, {xj.t.x - xi.t.x, xj.t.y - xi.t.y, xj.t.z - xi.t.z});
  z.q = qmul(qconj(xi.q), xj.q);
  double e[6], Ji[36], Jj[36];
  edge_error<true>(xi, xj, z, e, Ji, Jj);
  double *o = J72 + (size_t)k * 72;
#pragma unroll
  for (int m = 0; m < 36; ++m) {
    o[m] = Ji[m];
    o[36 + m] = Jj[m];
  }
}

__global__ void pg_dot_scale_kernel(const double *dx, const double *b, int n6, double lambda, double *part) {
  __shared__ double sh[CG_BLOCK];
  const int row = blockIdx.x * CG_ROWS + threadIdx.x;
  const double v = (threadIdx.x < CG_ROWS && row < n6) ? dx[row] * (lambda * dx[row] + b[row]) : 0.0;
  const double s = block_sum(v, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ void pg_maxdiag_kernel(const double *diag, int n_v, int fixed, double *out) {
  __shared__ double sh[256];
  double m = 0.0;
  for (int k = threadIdx.x; k < n_v * 6; k += 256) {
    const int v = k / 6, r = k % 6;
    if (v != fixed) m = fmax(m, diag[(size_t)v * 36 + r * 6 + r]);
  }
  sh[threadIdx.x] = m;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = sh[0];
}

thread_local std::string g_pg_err;
#define PG_TRY(expr)                                                                     \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) {                                                              \
      char _b[512];                                                                      \
      snprintf(_b, sizeof(_b), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      g_pg_err = _b;                                                                     \
      return LSLAM_ERR_HIP;                                                              \
    }                                                                                    \
  } while (0)

template <typename T>
hipError_t dev_upload(lslam::DevBuf<T> &d, const std::vector<T> &h) {
  hipError_t e = d.alloc(h.size());
  if (e != hipSuccess) return e;
  if (!h.empty()) e = hipMemcpy(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
  return e;
}

}  // namespace

std::string &lslam::pg_error() { return g_pg_err; }

// (struct lslam_pg: lslam_pg_internal.hpp)
namespace {

int build_shard(lslam_pg *pg, int e_begin, int e_end) {
  pg->e_begin = e_begin;
  pg->e_end = e_end;
  const int ne = e_end - e_begin;
  std::vector<int32_t> vptr(pg->n_v + 1, 0), optr(pg->n_off + 1, 0);
  for (int e = e_begin; e < e_end; ++e) {
    vptr[pg->h_ij[2 * e] + 1]++;
    vptr[pg->h_ij[2 * e + 1] + 1]++;
    optr[pg->edge_block[e] + 1]++;
  }
  for (int v = 0; v < pg->n_v; ++v) vptr[v + 1] += vptr[v];
  for (int k = 0; k < pg->n_off; ++k) optr[k + 1] += optr[k];
  std::vector<int32_t> vadj(2 * (size_t)ne), oadj((size_t)ne), vc(vptr.begin(), vptr.end() - 1),
      oc(optr.begin(), optr.end() - 1);
  for (int e = e_begin; e < e_end; ++e) {  // edge order = summation order
    const int le = e - e_begin;
    vadj[vc[pg->h_ij[2 * e]]++] = (le << 1) | 0;
    vadj[vc[pg->h_ij[2 * e + 1]]++] = (le << 1) | 1;
    oadj[oc[pg->edge_block[e]]++] = le;
  }
  PG_TRY(pg->d_rec.alloc(std::max<size_t>(1, (size_t)ne) * REC));
  PG_TRY(pg->d_chi.alloc((size_t)ne + (size_t)pg->n_p + (size_t)pg->n_q));  // the priors' values sit behind the edges', the plane priors' behind those (linearize)
  PG_TRY(dev_upload(pg->d_vptr, vptr));
  PG_TRY(dev_upload(pg->d_vadj, vadj));
  PG_TRY(dev_upload(pg->d_optr, optr));
  PG_TRY(dev_upload(pg->d_oadj, oadj));
  return LSLAM_OK;
}

// system of this shard's edges into pg->d_sys.p, then the all-reduce over ranks
int linearize(lslam_pg *pg, const double *poses) {
  const int ne = pg->e_end - pg->e_begin;
  if (ne > 0 && pg->robust)
    hipLaunchKernelGGL(pg_edge_robust_kernel, dim3((ne + 127) / 128), dim3(128), 0, pg->stream, poses, pg->d_ij.p,
                       pg->d_meas.p, pg->d_info.p, pg->e_begin, pg->e_end, pg->fixed, pg->d_kind.p, pg->d_delta.p,
                       pg->d_rec.p, pg->d_chi.p);
  else if (ne > 0)
    hipLaunchKernelGGL(pg_edge_kernel, dim3((ne + 127) / 128), dim3(128), 0, pg->stream, poses, pg->d_ij.p,
                       pg->d_meas.p, pg->d_info.p, pg->e_begin, pg->e_end, pg->fixed, pg->d_rec.p, pg->d_chi.p);
  const int np = pg->local_priors(), nq = pg->local_plane_priors();
  if (np > 0) {
    const int32_t *kind = pg->prior_robust ? pg->d_pkind.p : nullptr;
    const double *delta = pg->prior_robust ? pg->d_pdelta.p : nullptr;
    hipLaunchKernelGGL(pg->prior_robust ? pg_prior_kernel<true> : pg_prior_kernel<false>, dim3((np + 127) / 128), dim3(128),
                       0, pg->stream, poses, pg->d_pv.p, pg->d_ptype.p, pg->d_pmeas.p, pg->d_pinfo.p, np, pg->fixed, kind,
                       delta, pg->d_prec.p, pg->d_chi.p + ne);
  }
  if (nq > 0) {  // plane priors: their records, then ONE assembly that sums edges, priors, plane priors in that order
    hipLaunchKernelGGL(pg->plane_robust ? pg_plane_prior_kernel<true> : pg_plane_prior_kernel<false>, dim3((nq + 127) / 128),
                       dim3(128), 0, pg->stream, poses, pg->d_qv.p, pg->d_qpl.p, pg->d_qinfo.p, nq, pg->fixed,
                       pg->plane_robust ? pg->d_qkind.p : (const int32_t *)nullptr,
                       pg->plane_robust ? pg->d_qdelta.p : (const double *)nullptr, pg->d_qrec.p, pg->d_chi.p + ne + np);
    hipLaunchKernelGGL(pg_assemble_vertex_plane_kernel, dim3((pg->n_v * 42 + 255) / 256), dim3(256), 0, pg->stream,
                       pg->d_rec.p, pg->d_vptr.p, pg->d_vadj.p, pg->d_prec.p, np > 0 ? pg->d_pptr.p : (const int32_t *)nullptr,
                       pg->d_padj.p, pg->d_qrec.p, pg->d_qptr.p, pg->d_qadj.p, pg->n_v, pg->sharded() ? -1 : pg->fixed,
                       pg->diag(), pg->b());
  } else if (np > 0) {
    hipLaunchKernelGGL(pg_assemble_vertex_prior_kernel, dim3((pg->n_v * 42 + 255) / 256), dim3(256), 0, pg->stream,
                       pg->d_rec.p, pg->d_vptr.p, pg->d_vadj.p, pg->d_prec.p, pg->d_pptr.p, pg->d_padj.p, pg->n_v,
                       pg->sharded() ? -1 : pg->fixed, pg->diag(), pg->b());
  } else {  // no priors: exactly the launches of a graph that never had any
    hipLaunchKernelGGL(pg_assemble_vertex_kernel, dim3((pg->n_v * 42 + 255) / 256), dim3(256), 0, pg->stream,
                       pg->d_rec.p, pg->d_vptr.p, pg->d_vadj.p, pg->n_v, pg->sharded() ? -1 : pg->fixed,
                       pg->diag(), pg->b());
  }
  if (pg->n_off > 0)
    hipLaunchKernelGGL(pg_assemble_off_kernel, dim3((pg->n_off * 36 + 255) / 256), dim3(256), 0, pg->stream,
                       pg->d_rec.p, pg->d_optr.p, pg->d_oadj.p, pg->n_off, pg->off());
  hipLaunchKernelGGL(pg_sum_kernel, dim3(1), dim3(SUM_BLOCK), 0, pg->stream, pg->d_chi.p, ne + np + nq, 1, pg->chi());
  PG_TRY(hipGetLastError());
  if (pg->sharded()) {
    const int rc = pg->reduce(pg->d_sys.p, pg->core_doubles());
    if (rc) return rc;
    // identity block of the fixed vertex after the sum over ranks
    static const double I[36] = {1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0,
                                 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1};
    if (pg->fixed >= 0)
      PG_TRY(hipMemcpyAsync(pg->diag() + (size_t)pg->fixed * 36, I, 36 * sizeof(double), hipMemcpyHostToDevice, pg->stream));
  }
  return LSLAM_OK;
}

int eval_chi2(lslam_pg *pg, const double *poses, double *out) {
  // the chi2 slot of the system buffer is free again once the current chi2 has been read
  // back, and it lives in the buffer the all-reduce hook knows how to address
  const int ne = pg->e_end - pg->e_begin;
  if (ne > 0 && pg->robust)  // the sum below is then the sum of rho0 (g2o's activeRobustChi2)
    hipLaunchKernelGGL(pg_chi2_robust_kernel, dim3((ne + 127) / 128), dim3(128), 0, pg->stream, poses, pg->d_ij.p,
                       pg->d_meas.p, pg->d_info.p, pg->e_begin, pg->e_end, pg->d_kind.p, pg->d_delta.p, pg->d_chi.p);
  else if (ne > 0)
    hipLaunchKernelGGL(pg_chi2_kernel, dim3((ne + 127) / 128), dim3(128), 0, pg->stream, poses, pg->d_ij.p,
                       pg->d_meas.p, pg->d_info.p, pg->e_begin, pg->e_end, pg->d_chi.p);
  const int np = pg->local_priors();
  if (np > 0)
    hipLaunchKernelGGL(pg->prior_robust ? pg_prior_chi2_kernel<true> : pg_prior_chi2_kernel<false>, dim3((np + 127) / 128),
                       dim3(128), 0, pg->stream, poses, pg->d_pv.p, pg->d_ptype.p, pg->d_pmeas.p, pg->d_pinfo.p, np,
                       pg->prior_robust ? pg->d_pkind.p : (const int32_t *)nullptr,
                       pg->prior_robust ? pg->d_pdelta.p : (const double *)nullptr, pg->d_chi.p + ne);
  const int nq = pg->local_plane_priors();
  if (nq > 0)
    hipLaunchKernelGGL(pg_plane_prior_chi2_kernel, dim3((nq + 127) / 128), dim3(128), 0, pg->stream, poses, pg->d_qv.p, pg->d_qpl.p,
                       pg->d_qinfo.p, nq, pg->plane_robust ? pg->d_qkind.p : (const int32_t *)nullptr,
                       pg->plane_robust ? pg->d_qdelta.p : (const double *)nullptr, (double *)nullptr, pg->d_chi.p + ne + np,
                       (double *)nullptr);
  hipLaunchKernelGGL(pg_sum_kernel, dim3(1), dim3(SUM_BLOCK), 0, pg->stream, pg->d_chi.p, ne + np + nq, 1, pg->chi());
  PG_TRY(hipGetLastError());
  if (pg->sharded()) {
    // chi2 and, next to it, whether this rank's persistent kernels gave way to their launch loops in the solve before:
    // one all-reduce carries both (lslam_pg_optimize makes every rank follow a rank that fell back)
    const double flag = pg->fell_back ? 1.0 : 0.0;
    PG_TRY(hipMemcpyAsync(pg->chi() + 1, &flag, sizeof(double), hipMemcpyHostToDevice, pg->stream));
    PG_TRY(hipStreamSynchronize(pg->stream));  // `flag` is a local
    const int rc = pg->reduce(pg->chi(), 2);
    if (rc) return rc;
  }
  if (!out) return LSLAM_OK;  // the caller reads pg->chi() itself, behind more work on the stream
  PG_TRY(hipMemcpyAsync(out, pg->chi(), sizeof(double), hipMemcpyDeviceToHost, pg->stream));
  PG_TRY(hipStreamSynchronize(pg->stream));
  return LSLAM_OK;
}

// ---- the host driver of the solve: solve() at the end of this section is the list of its stages ------------

// What one call of solve() works on.
struct SolveCall {
  CgArgs a{};
  CoarseArgs c{};
  bool coarse = false;         // the second level of the preconditioner takes part in this solve ...
  bool fresh_inverse = false;  // ... with an inverse built by this call
  size_t n_items = 0;
  double lambda = 0.0;
  int max_cg = 0;
  double tol = 0.0;
};

// vals = the block rows of H + lambda I, minv = the inverses of its diagonal blocks, and the coarse level's partial-sum slots
int expand_and_precondition(lslam_pg *pg, const SolveCall &s) {
  hipLaunchKernelGGL(pg_expand_kernel, dim3((unsigned)((s.n_items * 6 + 255) / 256)), dim3(256), 0, pg->stream,
                     pg->d_sys.p, pg->d_row_src.p, pg->n_entries, s.lambda, pg->d_vals.p);
  hipLaunchKernelGGL(pg_precond_kernel, dim3((pg->n_v + 63) / 64), dim3(64), 0, pg->stream, pg->d_vals.p,
                     pg->d_row_ptr.p, pg->n_v, s.n_items, pg->d_minv.p);
  PG_TRY(hipMemsetAsync(pg->d_part.p, 0, 3 * (size_t)pg->n_parts * sizeof(double), pg->stream));  // the coarse level's slots
  return LSLAM_OK;
}

void make_cg_args(const lslam_pg *pg, SolveCall &s) {
  const int n6 = pg->n_v * 6;
  CgArgs &a = s.a;
  a.vals = pg->d_vals.p;
  a.row_ptr = pg->d_row_ptr.p;
  a.row_col = pg->d_row_col.p;
  a.row_of = pg->d_row_of.p;
  a.minv = pg->d_minv.p;
  a.b = pg->b();
  a.x = pg->d_x.p; a.r = pg->d_r.p; a.z = pg->d_z.p; a.d = pg->d_q.p;
  a.p[0] = pg->d_p.p;
  a.p[1] = pg->d_p.p + n6;
  a.part_rz[0] = pg->d_part.p;
  a.part_rz[1] = pg->d_part.p + pg->n_parts;
  a.part_rr = pg->d_part.p + 2 * pg->n_parts;
  a.part_pq = pg->d_part.p + 3 * pg->n_parts;
  a.n_parts = pg->n_parts;
  a.n_items = (int)s.n_items;
  a.n_pblocks = (int)((s.n_items + PROD_BLOCK - 1) / PROD_BLOCK);
  a.scal = pg->d_scal.p;
  a.n6 = n6;
  a.n_blocks = pg->n_cg_blocks;
  a.tol2 = s.tol * s.tol;
  a.item_begin = 0;
  a.item_end = (int)s.n_items;
  a.block_begin = 0;
}

// The second level's arguments (see pgc_P_kernel).  Its dense matrix and the Gauss-Jordan scratch are allocated by the first
// solve that takes the second level; the pointers into them are assigned here, after that.
int make_coarse_args(lslam_pg *pg, SolveCall &s) {
  if (!pg->d_Ac.p) {
    PG_TRY(pg->d_Ac.alloc((size_t)pg->n_c * pg->n_c));
    PG_TRY(pg->d_gj.alloc((size_t)12 * pg->n_c + 36));
  }
  CoarseArgs &c = s.c;
  c.poses = pg->d_poses.p;
  c.P = pg->d_P.p; c.Ac = pg->d_Ac.p; c.rc = pg->d_rc.p; c.yc = pg->d_yc.p;
  c.Rbuf = pg->d_gj.p; c.Cbuf = pg->d_gj.p + (size_t)6 * pg->n_c; c.Bbuf = pg->d_gj.p + (size_t)12 * pg->n_c;
  c.cb_ptr = pg->d_cb_ptr.p; c.cb_ent = pg->d_cb_ent.p; c.cb_ab = pg->d_cb_ab.p;
  c.agg_of = pg->d_agg_of.p; c.agg_ptr = pg->d_agg_ptr.p; c.agg_mem = pg->d_agg_mem.p;
  c.n_v = pg->n_v; c.G = pg->agg; c.na = pg->n_agg; c.n_c = pg->n_c; c.n_cb = pg->n_cb; c.n_cblk = pg->n_cblk;
  return LSLAM_OK;
}

// The reuse rule of the coarse inverse (see lslam_pg::coarse_valid): a function of lambda and iteration counts only, which
// are identical on every rank of a sharded run.
bool coarse_needs_rebuild(const lslam_pg *pg, double lambda) {
  if (!pg->coarse_valid || pg->env_no_reuse) return true;  // (A/B switch LSLAM_PG_NO_REUSE, read when the graph was created)
  const double ratio = lambda > pg->coarse_lambda ? lambda / pg->coarse_lambda : pg->coarse_lambda / lambda;
  return !(ratio <= 10.0) || (pg->coarse_fresh_iters > 0 && 10 * pg->coarse_last_iters > 13 * pg->coarse_fresh_iters);
}

// Do `n_groups` workgroups of `kernel` (this block size, this much dynamic LDS) fit on the device at once?  What a
// cooperative launch needs; the caller adds the conditions of its own kernel.
bool fits_co_resident(const lslam_pg *pg, const void *kernel, int block, size_t lds_bytes, int n_groups) {
  hipDeviceProp_t prop;
  int per_cu = 0;
  return hipGetDeviceProperties(&prop, pg->device) == hipSuccess &&
         hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, lds_bytes) == hipSuccess &&
         (long)per_cu * prop.multiProcessorCount >= n_groups;
}

// One persistent kernel, a workgroup per aggregate: the barrier words zeroed, the exchange slots set to the sentinel, the
// cooperative launch, and the abort word (with `scal_out`, the PCG's eight scalars too) read back behind ONE wait.
// *aborted: an exchange ran into its spin limit, i.e. the workgroups were not all resident at once (another process's
// persistent kernel on the same device can do that -- cooperative launches are not coordinated across processes) -- or the
// launch was refused: no cooperative launch on this device / partition mode, or the runtime's residency count differs from
// the occupancy query.  Neither is an error of the solve: the caller's launch loop does the work.
int launch_persistent(lslam_pg *pg, const void *kernel, int block, size_t lds_bytes, void *args, double *slots,
                      size_t n_slot_doubles, double *scal_out, bool *aborted) {
  PG_TRY(hipMemsetAsync(pg->d_bar.p, 0, 2 * sizeof(unsigned), pg->stream));
  PG_TRY(hipMemsetD32Async((hipDeviceptr_t)slots, (int)PK_SENT32, 2 * n_slot_doubles, pg->stream));
  void *kargs[] = {args};
  unsigned bar[2] = {0, 0};
  if (hipLaunchCooperativeKernel(kernel, dim3((unsigned)pg->n_agg), dim3(block), kargs, (unsigned)lds_bytes, pg->stream) != hipSuccess) {
    (void)hipGetLastError();
    bar[1] = 1;
  } else {
    if (scal_out) PG_TRY(hipMemcpyAsync(scal_out, pg->d_scal.p, 8 * sizeof(double), hipMemcpyDeviceToHost, pg->stream));
    PG_TRY(hipMemcpyAsync(bar, pg->d_bar.p, sizeof(bar), hipMemcpyDeviceToHost, pg->stream));
    PG_TRY(hipStreamSynchronize(pg->stream));
  }
  *aborted = bar[1] != 0;
  return LSLAM_OK;
}

// A persistent kernel gave way to its launch loop: the graph stays on that loop (*fit = 0), and in a sharded run every rank
// must follow (fell_back, see eval_chi2 and lm_trial).
void record_fallback(lslam_pg *pg, int *fit, const char *what) {
  if (pg->env_debug) fprintf(stderr, "[lslam pg] persistent %s: launch loop from here on\n", what);
  *fit = 0;
  pg->pk_timeouts++;
  pg->fell_back = true;
}

int assemble_coarse(lslam_pg *pg, const SolveCall &s) {
  PG_TRY(hipMemsetAsync(s.c.Ac, 0, (size_t)s.c.n_c * s.c.n_c * sizeof(double), pg->stream));
  hipLaunchKernelGGL(pgc_assemble_kernel, dim3(s.c.n_cb), dim3(64), 0, pg->stream, s.c, pg->d_vals.p, pg->d_row_of.p, pg->d_row_col.p, s.n_items);
  return LSLAM_OK;
}

// P at the current poses, A_c = P^T (H + lambda I) P, and its inverse in place: by the persistent Gauss-Jordan kernel when
// it fits, else (or after it gave up) by the pivot / update launch loop.
int build_coarse_inverse(lslam_pg *pg, const SolveCall &s) {
  const CoarseArgs &c = s.c;
  hipLaunchKernelGGL(pgc_P_kernel, dim3((pg->n_v + 127) / 128), dim3(128), 0, pg->stream, c);
  int rc = assemble_coarse(pg, s);
  if (rc) return rc;
  if (pg->gj_fit < 0) {  // the persistent inverse when a workgroup per aggregate is co-resident and the row fits its registers
    pg->gj_fit = 0;
    if (!pg->env_persistent_off && c.n_c <= GJ_CREG * GJ_BLOCK &&
        fits_co_resident(pg, (const void *)pgc_gj_persistent_kernel, GJ_BLOCK, 0, c.na) &&
        pg->d_gjslots.alloc((size_t)c.na * 6 * c.n_c) == hipSuccess)
      pg->gj_fit = 1;
    (void)hipGetLastError();
  }
  if (pg->gj_fit == 1) {
    GjArgs gj;
    gj.Ac = c.Ac; gj.slots = pg->d_gjslots.p; gj.bar = pg->d_bar.p; gj.n_c = c.n_c; gj.na = c.na;
    const char *da = lslam::debug_env("LSLAM_DEBUG_GJ_ABORT");  // test hook (LSLAM_DEBUG_HOOKS=1)
    gj.debug_abort = da ? std::atoi(da) : -1;
    bool aborted = false;
    rc = launch_persistent(pg, (const void *)pgc_gj_persistent_kernel, GJ_BLOCK, 0, &gj, pg->d_gjslots.p,
                           (size_t)c.na * 6 * c.n_c, nullptr, &aborted);
    if (rc) return rc;
    if (aborted) {  // the launch loop inverts A_c, assembled once more (a kernel that timed out wrote nothing back, but
                    // nothing here relies on that)
      record_fallback(pg, &pg->gj_fit, "Gauss-Jordan kernel timed out");
      rc = assemble_coarse(pg, s);
      if (rc) return rc;
    }
  }
  if (pg->gj_fit != 1) {
    const size_t nn = (size_t)c.n_c * c.n_c;
    for (int k = 0; k < c.na; ++k) {
      hipLaunchKernelGGL(pgc_gj_pivot_kernel, dim3(1), dim3(256), 0, pg->stream, c, k);
      hipLaunchKernelGGL(pgc_gj_update_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, pg->stream, c, k);
    }
  }
  PG_TRY(hipGetLastError());
  pg->coarse_valid = true;
  pg->coarse_lambda = s.lambda;
  pg->coarse_fresh_iters = 0;
  pg->coarse_setups++;
  return LSLAM_OK;
}

// The launch-per-step PCG loops' common form: 50 iterations enqueued by step(k), then pg_cg_check_kernel and one read-back
// of the scalars (converged? iterations done) -- one host wait per 50 iterations.
template <typename Step>
int run_cg_chunks(lslam_pg *pg, const CgArgs &a, int max_cg, Step step, int *done_iters) {
  double scal[8] = {0};
  *done_iters = 0;
  for (int it = 0; it < max_cg;) {
    const int chunk = std::min(50, max_cg - it);
    for (int k = it; k < it + chunk; ++k) {
      const int rc = step(k);
      if (rc) return rc;
    }
    it += chunk;
    hipLaunchKernelGGL(pg_cg_check_kernel, dim3(1), dim3(CG_BLOCK), 0, pg->stream, a, it);
    PG_TRY(hipMemcpyAsync(scal, pg->d_scal.p, sizeof(scal), hipMemcpyDeviceToHost, pg->stream));
    PG_TRY(hipStreamSynchronize(pg->stream));
    *done_iters = (int)scal[6];
    if (scal[5] != 0.0) break;
  }
  return LSLAM_OK;
}

// Gather or all-reduce is ONE decision of all ranks: a rank that gathered (grouped broadcasts) while another all-reduced
// would hang the solve.  lslam_pg_set_row_shard accepts any whole-block range and a rank may have no gather transport at
// all, so no rank can tell from what it holds what the others will do: EVERY rank of EVERY row-sharded solve sums a
// "not from me" flag through the linearisation's transport -- 1 without a gather transport or with a range that is not
// the canonical one -- and the ranks gather only if nobody raised it.  (Cached per rank this was itself a collective
// that some ranks could skip: a rank whose setting had not changed did not enter it.  One scalar all-reduce per solve of
// ~100 iterations with two collectives each costs nothing.)
int agree_on_gather(lslam_pg *pg, bool can_gather, double *slot, bool *agreed) {
  double flag = can_gather ? 0.0 : 1.0;
  PG_TRY(hipMemcpyAsync(slot, &flag, sizeof(double), hipMemcpyHostToDevice, pg->stream));
  PG_TRY(hipStreamSynchronize(pg->stream));  // (flag is a local)
  const int rc = pg->reduce(slot, 1);
  if (rc) return rc;
  PG_TRY(hipMemcpyAsync(&flag, slot, sizeof(double), hipMemcpyDeviceToHost, pg->stream));
  PG_TRY(hipStreamSynchronize(pg->stream));
  *agreed = flag == 0.0;
  return LSLAM_OK;
}

// ---- row-sharded solve: several GPUs share ONE solve of a large graph (beyond "replicated solve") ----------
// Block-Jacobi PCG only (the dense second level is a single-device structure), launch per step; see pg_rs_direction_kernel.
int solve_row_sharded(lslam_pg *pg, SolveCall &s, int *iters_out) {
  CgArgs &a = s.a;
  const int n6 = a.n6;
  const int v0 = pg->row_v0, v1 = pg->row_v1;
  const int r0 = v0 * 6, r1 = v1 * 6;
  a.item_begin = pg->h_row_ptr[(size_t)v0] * 6;
  a.item_end = pg->h_row_ptr[(size_t)v1] * 6;
  a.block_begin = r0 / CG_ROWS;
  const int nb_rows = (r1 - a.block_begin * CG_ROWS + CG_ROWS - 1) / CG_ROWS;   // row blocks of this rank
  const int nb_items = (a.item_end - a.item_begin + PROD_BLOCK - 1) / PROD_BLOCK;  // item blocks of this rank
  double *X = pg->xchg();  // [z (6 n_v) | rz | rr | pq | ... (8) | per rank: its part of rz, rr]
  double *z_own = a.z;     // init runs replicated on the ordinary z
  // The exchange: an all-gather of the owned segments when the transport has one and the ranks' rows are the canonical
  // partition (every rank can then name every segment without asking); else the zero-padded all-reduce.
  int g_rank = 0, g_world = 1;
  bool gather = pg->gather_transport(&g_rank, &g_world) && g_world >= 1 && g_world <= lslam_pg::RS_MAX_WORLD;
  int cb = -1, ce = -1;
  if (gather) lslam_pg_row_shard_range(pg->n_v, g_rank, g_world, &cb, &ce);
  bool agreed = false;
  int rc = agree_on_gather(pg, gather && cb == v0 && ce == v1, X + n6 + 7, &agreed);
  if (rc) return rc;
  std::vector<int64_t> z_offs, s_offs;
  if (gather) {
    gather = agreed;
    z_offs.resize((size_t)g_world + 1);
    s_offs.resize((size_t)g_world + 1);
    for (int r = 0; r <= g_world; ++r) {
      int b = pg->n_v, e = pg->n_v;
      if (r < g_world) lslam_pg_row_shard_range(pg->n_v, r, g_world, &b, &e);
      z_offs[(size_t)r] = (int64_t)b * 6;
      s_offs[(size_t)r] = 2 * (int64_t)r;
    }
  }
  double *tail = X + n6 + 8;
  double *const g_bufs[2] = {X, tail};
  const int64_t *const g_offs[2] = {z_offs.data(), s_offs.data()};
  const dim3 blk(CG_BLOCK), gall((n6 + 255) / 256), b256(256);
  // x = 0, r = b, z = M^-1 b and their sums, on every row by every rank: b is complete everywhere after the linearisation's
  // all-reduce, so this needs no exchange
  hipLaunchKernelGGL(pg_cg_init_kernel, dim3(pg->n_cg_blocks), blk, 0, pg->stream, a);
  hipLaunchKernelGGL(pg_cg_init2_kernel, dim3(1), blk, 0, pg->stream, a);
  hipLaunchKernelGGL(pg_sum_kernel, dim3(1), dim3(SUM_BLOCK), 0, pg->stream, a.part_rz[0], pg->n_cg_blocks, 1, X + n6);
  hipLaunchKernelGGL(pg_sum_kernel, dim3(1), dim3(SUM_BLOCK), 0, pg->stream, a.part_rr, pg->n_cg_blocks, 1, X + n6 + 1);
  hipLaunchKernelGGL(pg_rs_copy_kernel, dim3(1), dim3(64), 0, pg->stream, (const double *)(X + n6), a.part_rz[0], a.part_rr, (double *)nullptr);
  PG_TRY(hipMemcpyAsync(X, z_own, (size_t)n6 * sizeof(double), hipMemcpyDeviceToDevice, pg->stream));
  a.z = X;  // from here on z lives in the exchange area: own rows written by the update, the others arrive by the all-reduce
  a.n_parts = 1;
  a.n_pblocks = 1;
  int done_iters = 0;
  rc = run_cg_chunks(pg, a, s.max_cg, [&](int k) -> int {
    hipLaunchKernelGGL(pg_rs_direction_kernel, gall, b256, 0, pg->stream, a, k);
    hipLaunchKernelGGL(pg_cg_prod_kernel, dim3(std::max(nb_items, 1)), dim3(PROD_BLOCK), 0, pg->stream, a, k);
    hipLaunchKernelGGL(pg_sum_kernel, dim3(1), dim3(SUM_BLOCK), 0, pg->stream, a.part_pq, nb_items, 1, X + n6 + 2);
    PG_TRY(hipGetLastError());
    int rc = pg->reduce(X + n6 + 2, 1);  // p . A p
    if (rc) return rc;
    hipLaunchKernelGGL(pg_rs_copy_kernel, dim3(1), dim3(64), 0, pg->stream, (const double *)(X + n6 + 2), a.part_pq, (double *)nullptr, (double *)nullptr);
    hipLaunchKernelGGL(pg_cg_update_kernel, dim3(std::max(nb_rows, 1)), blk, 0, pg->stream, a, k);
    if (gather) {  // own rows of z are in place; own parts of r . z and r . r go to this rank's slot behind them
      hipLaunchKernelGGL(pg_sum_kernel, dim3(1), dim3(SUM_BLOCK), 0, pg->stream, a.part_rz[(k + 1) & 1], nb_rows, 1, tail + 2 * g_rank);
      hipLaunchKernelGGL(pg_sum_kernel, dim3(1), dim3(SUM_BLOCK), 0, pg->stream, a.part_rr, nb_rows, 1, tail + 2 * g_rank + 1);
      PG_TRY(hipGetLastError());
      rc = pg->gather(2, g_bufs, g_offs, g_world);
      if (rc) return rc;
      hipLaunchKernelGGL(pg_rs_tail_sum_kernel, dim3(1), dim3(64), 0, pg->stream, X + n6, (const double *)tail, g_world);
    } else {
      hipLaunchKernelGGL(pg_rs_zero_others_kernel, gall, b256, 0, pg->stream, X, n6, r0, r1);
      hipLaunchKernelGGL(pg_sum_kernel, dim3(1), dim3(SUM_BLOCK), 0, pg->stream, a.part_rz[(k + 1) & 1], nb_rows, 1, X + n6);
      hipLaunchKernelGGL(pg_sum_kernel, dim3(1), dim3(SUM_BLOCK), 0, pg->stream, a.part_rr, nb_rows, 1, X + n6 + 1);
      PG_TRY(hipGetLastError());
      rc = pg->reduce(X, (size_t)n6 + 2);  // z gathered, r . z and r . r summed
      if (rc) return rc;
    }
    hipLaunchKernelGGL(pg_rs_copy_kernel, dim3(1), dim3(64), 0, pg->stream, (const double *)(X + n6), a.part_rz[(k + 1) & 1], a.part_rr, (double *)nullptr);
    return LSLAM_OK;
  }, &done_iters);
  if (rc) return rc;
  // the solution: every rank's rows, gathered the same way
  hipLaunchKernelGGL(pg_rs_pack_kernel, gall, b256, 0, pg->stream, (const double *)pg->d_x.p, X, n6, r0, r1);
  PG_TRY(hipGetLastError());
  rc = gather ? pg->gather(1, g_bufs, g_offs, g_world) : pg->reduce(X, (size_t)n6);
  if (rc) return rc;
  PG_TRY(hipMemcpyAsync(pg->d_x.p, X, (size_t)n6 * sizeof(double), hipMemcpyDeviceToDevice, pg->stream));
  // this path's own accounting: it never runs with the second level, and finish_solve's rules about it do not apply
  *iters_out = done_iters;
  pg->total_solves++;
  pg->rs_solves++;
  pg->rs_gathered += gather ? 1 : 0;
  return LSLAM_OK;
}

// The persistent kernel when the graph fits: one workgroup per aggregate, all co-resident, LDS for its columns / items.
void decide_pk_fit(lslam_pg *pg) {
  if (pg->pk_fit >= 0) return;
  pg->pk_fit = 0;
  if (!pg->env_persistent_off && pg->n_agg <= PK_BLOCK /* one thread per aggregate sums the partials */ &&
      pg->pk_lds_bytes <= 150 * 1024 &&
      hipFuncSetAttribute((const void *)pg_pcg_persistent_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)pg->pk_lds_bytes) == hipSuccess &&
      fits_co_resident(pg, (const void *)pg_pcg_persistent_kernel, PK_BLOCK, pg->pk_lds_bytes, pg->n_agg))
    pg->pk_fit = 1;
  (void)hipGetLastError();
}

// The whole PCG loop in one launch.  *finished: it ran to its end and *done_iters counts; else nothing was written that
// the launch-per-step loop reads, and this graph stays on that loop from here on.
int solve_persistent(lslam_pg *pg, const SolveCall &s, bool *finished, int *done_iters) {
  const int n6 = s.a.n6;
  PkArgs k;
  k.vals = pg->d_vals.p; k.minv = pg->d_minv.p; k.b = pg->b();
  k.x = pg->d_x.p; k.p0 = pg->d_p.p; k.p1 = pg->d_p.p + n6;
  k.agg_ptr = pg->d_agg_ptr.p; k.agg_mem = pg->d_agg_mem.p;
  k.bent_ptr = pg->d_bent_ptr.p; k.bent = pg->d_bent.p; k.blc = pg->d_blc.p; k.bmptr = pg->d_bmptr.p;
  k.bcol_ptr = pg->d_bcol_ptr.p; k.bcol = pg->d_bcol.p;
  k.P = pg->d_P.p; k.Ainv = pg->d_Ac.p;
  k.rc0 = pg->d_pk.p; k.rc1 = pg->d_pk.p + pg->n_c;
  double *slots = pg->d_pk.p + 2 * (size_t)pg->n_c;
  const size_t n_slots = 2 * (size_t)n6 + 6 * (size_t)pg->n_agg + 2 * (size_t)pg->n_c;
  k.zA = slots; k.rzA = k.zA + 2 * (size_t)n6; k.rrA = k.rzA + 2 * pg->n_agg; k.pqB = k.rrA + 2 * pg->n_agg;
  k.qcB = k.pqB + 2 * pg->n_agg;
  k.scal = pg->d_scal.p; k.bar = pg->d_bar.p;
  k.n_items = s.n_items;
  k.n6 = n6; k.n_agg = pg->n_agg; k.n_c = pg->n_c; k.coarse = s.coarse ? 1 : 0; k.max_iter = s.max_cg;
  k.lds_cols = pg->pk_lds_cols; k.lds_items = pg->pk_lds_items;
  k.tol2 = s.tol * s.tol;
  const char *da = lslam::debug_env("LSLAM_DEBUG_PG_ABORT");  // test hook (LSLAM_DEBUG_HOOKS=1)
  k.debug_abort = da ? std::atoi(da) : -1;
  double scal[8] = {0};
  bool aborted = false;
  const int rc = launch_persistent(pg, (const void *)pg_pcg_persistent_kernel, PK_BLOCK, pg->pk_lds_bytes, &k, slots, n_slots,
                                   scal, &aborted);
  if (rc) return rc;
  *finished = !aborted;
  if (aborted) {
    record_fallback(pg, &pg->pk_fit, "PCG kernel timed out in a grid exchange");
    return LSLAM_OK;
  }
  *done_iters = (int)scal[6];
  pg->fused_solves++;
  return LSLAM_OK;
}

// The same PCG, a launch per step (graphs that do not fit the persistent kernel, and after a fallback).
int solve_launch_loop(lslam_pg *pg, const SolveCall &s, int *done_iters) {
  const CgArgs &a = s.a;
  const CoarseArgs &c = s.c;
  const dim3 g(pg->n_cg_blocks), blk(CG_BLOCK);
  auto coarse_correct = [&](int k) {  // z += P A_c^-1 P^T r and the matching share of r.z, entering iteration k + 1
    if (!s.coarse) return;
    hipLaunchKernelGGL(pgc_restrict_kernel, dim3(c.na), dim3(64), 0, pg->stream, c, (const double *)a.r);
    hipLaunchKernelGGL(pgc_mvp_kernel, dim3(c.na), dim3(256), 0, pg->stream, c, a.z, a.part_rz[(k + 1) & 1] + pg->n_cg_blocks);
  };
  hipLaunchKernelGGL(pg_cg_init_kernel, g, blk, 0, pg->stream, a);
  hipLaunchKernelGGL(pg_cg_init2_kernel, dim3(1), blk, 0, pg->stream, a);
  coarse_correct(-1);
  const int rc = run_cg_chunks(pg, a, s.max_cg, [&](int k) -> int {
    hipLaunchKernelGGL(pg_cg_prod_kernel, dim3(a.n_pblocks), dim3(PROD_BLOCK), 0, pg->stream, a, k);
    hipLaunchKernelGGL(pg_cg_update_kernel, g, blk, 0, pg->stream, a, k);
    coarse_correct(k);
    return LSLAM_OK;
  }, done_iters);
  if (rc) return rc;
  PG_TRY(hipGetLastError());
  return LSLAM_OK;
}

// What a finished replicated solve leaves for the next one.
void finish_solve(lslam_pg *pg, const SolveCall &s, int done_iters, int *iters_out) {
  *iters_out = done_iters;
  if (done_iters > 300) pg->coarse_on = true;  // ill-conditioned from here on: later solves of this graph take the second level
  if (s.coarse) {
    if (s.fresh_inverse) pg->coarse_fresh_iters = done_iters;
    pg->coarse_last_iters = done_iters;
  }
}

// (H + lambda I) dx = b by block-Jacobi PCG, with the second level when it is on; returns iterations
int solve(lslam_pg *pg, double lambda, int max_cg, double tol, int *iters_out) {
  SolveCall s;
  s.n_items = (size_t)pg->n_entries * 6;
  s.lambda = lambda;
  s.max_cg = max_cg;
  s.tol = tol;
  // second level (see pgc_P_kernel): on when forced, or -- automatic -- once a solve of this graph needed many iterations
  s.coarse = pg->coarse_mode == 1 || (pg->coarse_mode < 0 && pg->coarse_on);
  int rc = expand_and_precondition(pg, s);
  if (rc) return rc;
  make_cg_args(pg, s);
  if (s.coarse) {
    rc = make_coarse_args(pg, s);
    if (rc) return rc;
    s.fresh_inverse = coarse_needs_rebuild(pg, lambda);
    if (s.fresh_inverse) rc = build_coarse_inverse(pg, s);
    if (rc) return rc;
    pg->coarse_solves++;
  }
  if (pg->sharded() && pg->row_v0 >= 0 && !s.coarse) return solve_row_sharded(pg, s, iters_out);
  decide_pk_fit(pg);
  pg->total_solves++;
  int done_iters = 0;
  bool finished = false;
  if (pg->pk_fit == 1) rc = solve_persistent(pg, s, &finished, &done_iters);
  if (rc) return rc;
  if (!finished) rc = solve_launch_loop(pg, s, &done_iters);
  if (rc) return rc;
  finish_solve(pg, s, done_iters, iters_out);
  return LSLAM_OK;
}

// ---- what lslam_pg_create builds on the host, before anything is uploaded: the builders below make no HIP call ------------
struct GraphLayout {
  int n_v = 0, n_e = 0;
  const int32_t *ij = nullptr;
  std::vector<int32_t> off_pairs, edge_block;                        // number_offdiag_blocks
  std::vector<int32_t> rptr, rcol, rsrc, rof;                        // build_solver_rows
  std::vector<int32_t> agg_of, agg_ptr, agg_mem;                     // grow_aggregates, merge_pockets
  std::vector<int32_t> cptr, cent, cab;                              // build_coarse_blocks
  std::vector<int32_t> bent_ptr, bent, blc, bmptr, bcol_ptr, bcol;   // build_persistent_view
  int max_cols = 0, max_items = 0;                                   // ... its widest aggregate
  int n_off() const { return (int)(off_pairs.size() / 2); }
  int n_agg() const { return (int)agg_ptr.size() - 1; }
};

// off-diagonal block ids: distinct (min,max) pairs in first-appearance order of a sorted map
void number_offdiag_blocks(GraphLayout &L) {
  const int32_t *ij = L.ij;
  std::map<std::pair<int, int>, int> ids;
  for (int e = 0; e < L.n_e; ++e) ids.emplace(std::minmax(ij[2 * e], ij[2 * e + 1]), 0);
  int nid = 0;
  for (auto &kv : ids) kv.second = nid++;
  L.off_pairs.resize(2 * (size_t)nid);
  for (auto &kv : ids) {
    L.off_pairs[2 * kv.second] = kv.first.first;
    L.off_pairs[2 * kv.second + 1] = kv.first.second;
  }
  L.edge_block.resize(L.n_e);
  for (int e = 0; e < L.n_e; ++e) L.edge_block[e] = ids[std::minmax(ij[2 * e], ij[2 * e + 1])];
}

// solver block-CSR: row v = [diag, then neighbours in block-id order]
void build_solver_rows(GraphLayout &L) {
  const int n_v = L.n_v, nid = L.n_off();
  std::vector<std::vector<std::pair<int, int>>> rows(n_v);  // (col, code)
  for (int v = 0; v < n_v; ++v) rows[v].push_back({v, (v << 2) | 1});
  for (int k = 0; k < nid; ++k) {
    const int a = L.off_pairs[2 * k], b = L.off_pairs[2 * k + 1];
    rows[a].push_back({b, ((n_v + k) << 2) | 0});
    rows[b].push_back({a, ((n_v + k) << 2) | 2});
  }
  L.rptr.assign(n_v + 1, 0);
  for (int v = 0; v < n_v; ++v) {
    L.rptr[v + 1] = L.rptr[v] + (int)rows[v].size();
    for (auto &pr : rows[v]) {
      L.rcol.push_back(pr.first);
      L.rsrc.push_back(pr.second);
      L.rof.push_back(v);
    }
  }
}

// aggregates: breadth-first from the lowest unassigned vertex over the solver rows (neighbours in block-id order,
// i.e. deterministic), at most `limit` members each
void grow_aggregates(GraphLayout &L, int limit) {
  const std::vector<int32_t> &rptr = L.rptr, &rcol = L.rcol;
  std::vector<int32_t> &agg_of = L.agg_of, &agg_ptr = L.agg_ptr, &agg_mem = L.agg_mem;
  agg_of.assign((size_t)L.n_v, -1);
  agg_ptr.assign(1, 0);
  for (int seed = 0; seed < L.n_v; ++seed) {
    if (agg_of[(size_t)seed] >= 0) continue;
    const int a = (int)agg_ptr.size() - 1;
    const size_t first = agg_mem.size();
    agg_of[(size_t)seed] = a;
    agg_mem.push_back(seed);
    for (size_t head = first; head < agg_mem.size() && (int)(agg_mem.size() - first) < limit; ++head) {
      const int u = agg_mem[head];
      for (int e = rptr[(size_t)u]; e < rptr[(size_t)u + 1] && (int)(agg_mem.size() - first) < limit; ++e) {
        const int v = rcol[(size_t)e];
        if (agg_of[(size_t)v] < 0) {
          agg_of[(size_t)v] = a;
          agg_mem.push_back(v);
        }
      }
    }
    agg_ptr.push_back((int32_t)agg_mem.size());
  }
}

// Breadth-first growth leaves pockets: a handful of keyframes cut off between two full aggregates (59 of the bench
// graph's 136 aggregates had fewer than eight members).  Each would be a workgroup of the persistent solver, a
// participant of every grid exchange and six coarse unknowns of little use: a pocket joins the smallest adjacent
// aggregate that has room for it (the growth stops at 7/8 of the limit G to leave that room).
void merge_pockets(GraphLayout &L, int G) {
  const std::vector<int32_t> &rptr = L.rptr, &rcol = L.rcol;
  std::vector<int32_t> &agg_of = L.agg_of, &agg_ptr = L.agg_ptr, &agg_mem = L.agg_mem;
  const int n0 = (int)agg_ptr.size() - 1;
  std::vector<int> size(n0), into(n0);
  for (int a = 0; a < n0; ++a) { size[a] = agg_ptr[(size_t)a + 1] - agg_ptr[(size_t)a]; into[a] = a; }
  for (int a = 0; a < n0; ++a) {
    if (size[a] > std::max(1, G / 8)) continue;
    int best = -1;
    for (int m = agg_ptr[(size_t)a]; m < agg_ptr[(size_t)a + 1]; ++m) {
      const int u = agg_mem[(size_t)m];
      for (int e = rptr[(size_t)u]; e < rptr[(size_t)u + 1]; ++e) {
        int b = agg_of[(size_t)rcol[(size_t)e]];
        while (into[b] != b) b = into[b];
        if (b != a && size[b] + size[a] <= G && (best < 0 || size[b] < size[best] || (size[b] == size[best] && b < best))) best = b;
      }
    }
    if (best >= 0) { into[a] = best; size[best] += size[a]; size[a] = 0; }
  }
  std::vector<int> newid(n0, -1);
  int nn = 0;
  for (int a = 0; a < n0; ++a) if (into[a] == a) newid[a] = nn++;
  std::vector<std::vector<int32_t>> mem((size_t)nn);
  for (int a = 0; a < n0; ++a) {  // the receiving aggregate's members first (its first member stays its origin), pockets after them in order
    int b = a;
    while (into[b] != b) b = into[b];
    if (b == a)
      for (int m = agg_ptr[(size_t)a]; m < agg_ptr[(size_t)a + 1]; ++m) mem[(size_t)newid[a]].push_back(agg_mem[(size_t)m]);
  }
  for (int a = 0; a < n0; ++a) {
    int b = a;
    while (into[b] != b) b = into[b];
    if (b != a)
      for (int m = agg_ptr[(size_t)a]; m < agg_ptr[(size_t)a + 1]; ++m) mem[(size_t)newid[b]].push_back(agg_mem[(size_t)m]);
  }
  agg_ptr.assign(1, 0);
  agg_mem.clear();
  for (int a = 0; a < nn; ++a) {
    for (int32_t u : mem[(size_t)a]) { agg_of[(size_t)u] = a; agg_mem.push_back(u); }
    agg_ptr.push_back((int32_t)agg_mem.size());
  }
}

// coarse blocks: fine entries grouped by (aggregate of the row, aggregate of the column), in entry order
void build_coarse_blocks(GraphLayout &L) {
  std::map<std::pair<int, int>, std::vector<int32_t>> cb;
  for (int e = 0; e < (int)L.rcol.size(); ++e) cb[{L.agg_of[(size_t)L.rof[(size_t)e]], L.agg_of[(size_t)L.rcol[(size_t)e]]}].push_back(e);
  L.cptr.assign(1, 0);
  for (auto &kv : cb) {
    L.cab.push_back(kv.first.first);
    L.cab.push_back(kv.first.second);
    L.cent.insert(L.cent.end(), kv.second.begin(), kv.second.end());
    L.cptr.push_back((int32_t)L.cent.size());
  }
}

// the persistent PCG kernel's view: per aggregate its rows' entries member by member, and a local numbering of
// the column vertices those entries refer to (first appearance order)
void build_persistent_view(GraphLayout &L) {
  const std::vector<int32_t> &rptr = L.rptr, &rcol = L.rcol, &agg_ptr = L.agg_ptr, &agg_mem = L.agg_mem;
  std::vector<int32_t> &bent = L.bent, &blc = L.blc, &bmptr = L.bmptr, &bcol = L.bcol;
  L.bent_ptr.assign(1, 0);
  L.bcol_ptr.assign(1, 0);
  std::vector<int32_t> local((size_t)L.n_v, -1);
  for (int a = 0; a < L.n_agg(); ++a) {
    const size_t cfirst = bcol.size();
    const size_t efirst = bent.size();
    for (int m = agg_ptr[(size_t)a]; m < agg_ptr[(size_t)a + 1]; ++m) {
      const int u = agg_mem[(size_t)m];
      bmptr.push_back((int32_t)(bent.size() - efirst));
      for (int e = rptr[(size_t)u]; e < rptr[(size_t)u + 1]; ++e) {
        const int cv = rcol[(size_t)e];
        if (local[(size_t)cv] < 0) {
          local[(size_t)cv] = (int32_t)(bcol.size() - cfirst);
          bcol.push_back(cv);
        }
        bent.push_back(e);
        blc.push_back(local[(size_t)cv]);
      }
    }
    bmptr.push_back((int32_t)(bent.size() - efirst));
    for (size_t c = cfirst; c < bcol.size(); ++c) local[(size_t)bcol[c]] = -1;
    L.bent_ptr.push_back((int32_t)bent.size());
    L.bcol_ptr.push_back((int32_t)bcol.size());
    L.max_cols = std::max(L.max_cols, (int)(bcol.size() - cfirst));
    L.max_items = std::max(L.max_items, 6 * (int)(bent.size() - efirst));
  }
}

// The layout's sizes into the graph, and what LSLAM_DEBUG says about it.
void adopt_layout_sizes(lslam_pg *pg, const GraphLayout &L) {
  pg->n_off = L.n_off();
  pg->n_entries = (int)L.rcol.size();
  pg->n_agg = L.n_agg();
  pg->n_c = 6 * pg->n_agg;
  pg->n_cblk = pg->n_agg;  // partial-sum slots of the coarse level: one per aggregate (pgc_mvp_kernel)
  pg->n_cb = (int)L.cptr.size() - 1;
  // the dense coarse matrix (n_c^2 doubles) and the Gauss-Jordan scratch are allocated by the first solve that takes the
  // second level (make_coarse_args); graphs whose coarse matrix would exceed PG_COARSE_MAX unknowns never take it
  if (pg->n_c > PG_COARSE_MAX) {
    if (pg->env_debug)
      fprintf(stderr, "[lslam pg] %d coarse unknowns > %d: the dense second level is not used for this graph (block-Jacobi PCG)\n", pg->n_c, PG_COARSE_MAX);
    pg->coarse_mode = 0;
  }
  pg->pk_lds_cols = L.max_cols;
  pg->pk_lds_items = L.max_items;
  pg->pk_lds_bytes = ((size_t)L.max_cols * 6 + (size_t)L.max_items + PK_ROWS + 7 * (size_t)pg->n_c + 8 * PK_W) * sizeof(double);
  const size_t n6 = (size_t)pg->n_v * 6;
  pg->n_cg_blocks = (int)((n6 + CG_ROWS - 1) / CG_ROWS);
  pg->n_parts = pg->n_cg_blocks + pg->n_cblk;
  if (pg->env_debug) {
    int hist[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int a = 0; a < pg->n_agg; ++a) hist[std::min(8, (L.agg_ptr[(size_t)a + 1] - L.agg_ptr[(size_t)a]) / 8)]++;
    fprintf(stderr, "[lslam pg] aggregate sizes (members / 8): %d %d %d %d %d %d %d %d %d\n", hist[0], hist[1], hist[2], hist[3],
            hist[4], hist[5], hist[6], hist[7], hist[8]);
    fprintf(stderr, "[lslam pg] %d aggregates, widest: %d columns, %d items; persistent-kernel LDS %zu bytes\n", pg->n_agg,
            L.max_cols, L.max_items, pg->pk_lds_bytes);
  }
}

// the second level and the persistent kernels' structures
int upload_aggregates(lslam_pg *pg, const GraphLayout &L) {
  PG_TRY(dev_upload(pg->d_agg_of, L.agg_of));
  PG_TRY(dev_upload(pg->d_agg_ptr, L.agg_ptr));
  PG_TRY(dev_upload(pg->d_agg_mem, L.agg_mem));
  PG_TRY(dev_upload(pg->d_cb_ptr, L.cptr));
  PG_TRY(dev_upload(pg->d_cb_ent, L.cent));
  PG_TRY(dev_upload(pg->d_cb_ab, L.cab));
  PG_TRY(pg->d_P.alloc((size_t)pg->n_v * 36));
  PG_TRY(pg->d_rc.alloc((size_t)pg->n_c));
  PG_TRY(pg->d_yc.alloc((size_t)pg->n_c));
  PG_TRY(dev_upload(pg->d_bent_ptr, L.bent_ptr));
  PG_TRY(dev_upload(pg->d_bent, L.bent));
  PG_TRY(dev_upload(pg->d_blc, L.blc));
  PG_TRY(dev_upload(pg->d_bmptr, L.bmptr));
  PG_TRY(dev_upload(pg->d_bcol_ptr, L.bcol_ptr));
  PG_TRY(dev_upload(pg->d_bcol, L.bcol));
  // [rc0 | rc1] then the sentinel-initialised slots [zA 2 n6 | rzA 2 n_agg | rrA 2 n_agg | pqB 2 n_agg | qcB 2 n_c]
  PG_TRY(pg->d_pk.alloc(4 * (size_t)pg->n_c + 6 * (size_t)pg->n_agg + 12 * (size_t)pg->n_v));
  PG_TRY(pg->d_bar.alloc(2));
  return LSLAM_OK;
}

// the graph, the solver rows, and the solver's vectors
int upload_graph_and_solver(lslam_pg *pg, const GraphLayout &L, const double *poses7, const double *meas7, const double *info36) {
  const size_t n_v = (size_t)pg->n_v, n_e = (size_t)pg->n_e;
  std::vector<double> hp(poses7, poses7 + 7 * n_v), hm(meas7, meas7 + 7 * n_e), hi(info36, info36 + 36 * n_e);
  PG_TRY(dev_upload(pg->d_poses, hp));
  PG_TRY(dev_upload(pg->d_trial, hp));
  PG_TRY(dev_upload(pg->d_meas, hm));
  PG_TRY(dev_upload(pg->d_info, hi));
  PG_TRY(dev_upload(pg->d_ij, pg->h_ij));
  PG_TRY(dev_upload(pg->d_row_ptr, L.rptr));
  PG_TRY(dev_upload(pg->d_row_col, L.rcol));
  PG_TRY(dev_upload(pg->d_row_src, L.rsrc));
  PG_TRY(dev_upload(pg->d_row_of, L.rof));
  const size_t n6 = n_v * 6;
  PG_TRY(pg->d_sys.alloc(pg->sys_doubles()));
  PG_TRY(pg->d_vals.alloc((size_t)pg->n_entries * 36));
  PG_TRY(pg->d_minv.alloc(n_v * 36));
  for (lslam::DevBuf<double> *p : {&pg->d_x, &pg->d_r, &pg->d_z})
    PG_TRY(p->alloc(n6));
  PG_TRY(pg->d_q.alloc((size_t)pg->n_entries * 6));
  PG_TRY(pg->d_p.alloc(2 * n6));
  PG_TRY(pg->d_part.alloc(3 * (size_t)pg->n_parts + ((size_t)pg->n_entries * 6 + PROD_BLOCK - 1) / PROD_BLOCK));
  PG_TRY(pg->d_scal.alloc(32));
  PG_TRY(hipMemset(pg->d_scal.p, 0, 32 * sizeof(double)));
  PG_TRY(pg->d_tmp.alloc(8));
  return LSLAM_OK;
}

}  // namespace

// ---- what the marginal-covariance unit takes from this one (lslam_pg_internal.hpp) ----------------------------------------
int lslam::pg_marginal_system(lslam_pg *pg, bool coarse, CoarseArgs *c) {
  if (coarse && pg->n_c > PG_COARSE_MAX) {
    g_pg_err = "the two-level preconditioner is not available for this graph (too many aggregates): ask for coarse = 0";
    return LSLAM_ERR_INVALID;
  }
  int rc = linearize(pg, pg->d_poses.p);
  if (rc) return rc;
  SolveCall s;
  s.n_items = (size_t)pg->n_entries * 6;
  s.lambda = 0.0;
  s.coarse = coarse;
  rc = expand_and_precondition(pg, s);
  if (rc || !coarse) return rc;
  rc = make_coarse_args(pg, s);
  if (rc) return rc;
  const int setups = pg->coarse_setups;
  rc = build_coarse_inverse(pg, s);
  // the inverse now in d_Ac is this call's, at lambda = 0: the graph's next damped solve builds its own and counts it
  pg->coarse_valid = false;
  pg->coarse_setups = setups;
  *c = s.c;
  return rc;
}

int lslam::pg_relative_jacobians(lslam_pg *pg, int ref, int n, const int32_t *d_v, double *d_J72) {
  if (n <= 0) return LSLAM_OK;
  hipLaunchKernelGGL(pg_rel_jac_kernel, dim3((n + 63) / 64), dim3(64), 0, pg->stream, (const double *)pg->d_poses.p, ref, n,
                     d_v, d_J72);
  PG_TRY(hipGetLastError());
  return LSLAM_OK;
}

extern "C" {

const char *lslam_pg_last_error(void) { return g_pg_err.c_str(); }

int lslam_pg_create(int device, int32_t n_v, const double *poses7, int32_t n_e, const int32_t *ij,
                    const double *meas7, const double *info36, int32_t fixed_vertex, lslam_pg **out) {
  if (!out || n_v <= 0 || n_e < 0 || !poses7 || (n_e && (!ij || !meas7 || !info36)) || fixed_vertex >= n_v) {
    g_pg_err = "bad pose-graph arguments";
    return LSLAM_ERR_INVALID;
  }
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    g_pg_err = "no HIP device available; this backend has no CPU fallback";
    return LSLAM_ERR_HIP;
  }
  PG_TRY(hipSetDevice(device));
  for (int e = 0; e < n_e; ++e)
    if (ij[2 * e] < 0 || ij[2 * e] >= n_v || ij[2 * e + 1] < 0 || ij[2 * e + 1] >= n_v || ij[2 * e] == ij[2 * e + 1]) {
      g_pg_err = "edge endpoint out of range";
      return LSLAM_ERR_INVALID;
    }
  lslam_pg *pg = new lslam_pg();
  struct Guard {  // a failure below frees what was built so far
    lslam_pg *p;
    ~Guard() { if (p) lslam_pg_destroy(p); }
  } guard{pg};
  pg->device = device;
  pg->n_v = n_v;
  pg->n_e = n_e;
  pg->fixed = fixed_vertex;
  // The one place where a pose graph reads the environment -- when it is created, never while it is optimised.  It stays
  // inside this function: tests/test_abi.py holds every getenv of this file to the text of lslam_pg_create.
  const auto read_env = [](lslam_pg *pg) {
    (void)lslam::debug_env("LSLAM_DEBUG_HOOKS");  // (the process-wide snapshot of the environment is taken no later than here)
    pg->env_no_reuse = std::getenv("LSLAM_PG_NO_REUSE") != nullptr;
    pg->env_no_merge = std::getenv("LSLAM_PG_NO_MERGE") != nullptr;
    pg->env_debug = std::getenv("LSLAM_DEBUG") != nullptr;
    if (const char *v = std::getenv("LSLAM_PG_PERSISTENT")) pg->env_persistent_off = std::atoi(v) == 0;
    if (const char *v = std::getenv("LSLAM_PG_MAX_CG")) pg->env_max_cg = std::atoi(v);
    if (const char *v = std::getenv("LSLAM_PG_TOL")) pg->env_tol = std::atof(v);
    if (const char *v = std::getenv("LSLAM_PG_AGG")) pg->agg = std::max(2, std::min(PG_AGG_MAX, std::atoi(v)));
    if (const char *v = std::getenv("LSLAM_PG_COARSE")) pg->coarse_mode = std::atoi(v);
  };
  read_env(pg);
  PG_TRY(hipStreamCreateWithFlags(&pg->stream, hipStreamNonBlocking));
  GraphLayout L;
  L.n_v = n_v;
  L.n_e = n_e;
  L.ij = ij;
  number_offdiag_blocks(L);
  build_solver_rows(L);
  // (the growth stops at 7/8 of the limit: the merge fills up to it)
  grow_aggregates(L, pg->env_no_merge ? pg->agg : std::max(2, pg->agg - pg->agg / 8));
  if (!pg->env_no_merge) merge_pockets(L, pg->agg);
  build_coarse_blocks(L);
  build_persistent_view(L);
  adopt_layout_sizes(pg, L);
  int rc = upload_aggregates(pg, L);
  if (rc) return rc;
  pg->h_ij.assign(ij, ij + 2 * (size_t)n_e);
  rc = upload_graph_and_solver(pg, L, poses7, meas7, info36);
  if (rc) return rc;
  pg->off_pairs = std::move(L.off_pairs);
  pg->edge_block = std::move(L.edge_block);
  pg->h_row_ptr = std::move(L.rptr);
  pg->h_row_of = std::move(L.rof);
  pg->h_row_col = std::move(L.rcol);
  rc = build_shard(pg, 0, n_e);
  if (rc) return rc;
  guard.p = nullptr;
  *out = pg;
  return LSLAM_OK;
}

void lslam_pg_destroy(lslam_pg *pg) {
  if (!pg) return;
  (void)hipSetDevice(pg->device);
  if (pg->stream) (void)hipStreamSynchronize(pg->stream);
  if (pg->stream) (void)hipStreamDestroy(pg->stream);
  delete pg;
}

size_t lslam_pg_system_doubles(const lslam_pg *pg) { return pg ? pg->sys_doubles() : 0; }

void lslam_pg_row_shard_range(int32_t n_vertices, int32_t rank, int32_t world, int32_t *v_begin, int32_t *v_end) {
  // whole row blocks of the PCG kernels (21 vertices), as even as that allows
  const int per = CG_ROWS / 6;
  const int nblk = (n_vertices + per - 1) / per;
  const int b0 = (int)((long long)nblk * rank / world), b1 = (int)((long long)nblk * (rank + 1) / world);
  if (v_begin) *v_begin = std::min(n_vertices, b0 * per);
  if (v_end) *v_end = std::min(n_vertices, b1 * per);
}

int lslam_pg_set_row_shard(lslam_pg *pg, int32_t v_begin, int32_t v_end) {
  if (!pg) return LSLAM_ERR_INVALID;
  if (v_begin < 0 && v_end < 0) {  // back to the replicated solve
    pg->row_v0 = pg->row_v1 = -1;
    return LSLAM_OK;
  }
  if (v_begin < 0 || v_end < v_begin || v_end > pg->n_v || (v_begin % (CG_ROWS / 6)) != 0 ||
      (v_end != pg->n_v && (v_end % (CG_ROWS / 6)) != 0)) {
    g_pg_err = "row shard must be a range of whole 21-vertex row blocks (lslam_pg_row_shard_range)";
    return LSLAM_ERR_INVALID;
  }
  if (v_begin == v_end) {
    // more ranks than 21-vertex row blocks (e.g. 20 keyframes on 2 ranks): a rank without rows has nothing to multiply or
    // update, and the solve's launches are not written for that.  Such a graph is far too small to share: replicated solve.
    g_pg_err = "empty row shard: the graph has fewer 21-vertex row blocks than ranks -- use the replicated solve (lslam_pg_set_row_shard(pg, -1, -1))";
    return LSLAM_ERR_INVALID;
  }
  pg->row_v0 = v_begin;
  pg->row_v1 = v_end;
  return LSLAM_OK;
}

int lslam_pg_set_solve_tolerance(lslam_pg *pg, double rel_tol) {
  if (!pg || !(rel_tol > 0.0) || !(rel_tol < 1.0)) {
    g_pg_err = "solve tolerance must be in (0, 1)";
    return LSLAM_ERR_INVALID;
  }
  pg->env_tol = rel_tol;
  return LSLAM_OK;
}

int32_t lslam_pg_row_sharded_solves(const lslam_pg *pg) { return pg ? pg->rs_solves : 0; }
int32_t lslam_pg_row_gathered_solves(const lslam_pg *pg) { return pg ? pg->rs_gathered : 0; }

int lslam_pg_set_row_gather(lslam_pg *pg, lslam_allgatherv_fn fn, void *user, int32_t rank, int32_t world) {
  if (!pg) return LSLAM_ERR_INVALID;
  if (fn && (world < 1 || world > lslam_pg::RS_MAX_WORLD || rank < 0 || rank >= world)) {
    g_pg_err = "bad rank / world for the row gather";
    return LSLAM_ERR_INVALID;
  }
  pg->gatherv = fn;
  pg->gatherv_user = user;
  pg->gatherv_rank = fn ? rank : -1;
  pg->gatherv_world = fn ? world : 0;
  return LSLAM_OK;
}

int lslam_pg_set_comm(lslam_pg *pg, lslam_comm *comm) {
  if (!pg) return LSLAM_ERR_INVALID;
  pg->comm = comm;
  return LSLAM_OK;
}
int32_t lslam_pg_num_offdiag(const lslam_pg *pg) { return pg ? pg->n_off : 0; }
void *lslam_pg_stream(lslam_pg *pg) { return pg ? (void *)pg->stream : nullptr; }

int lslam_pg_set_shard(lslam_pg *pg, int32_t e_begin, int32_t e_end, lslam_allreduce_fn fn, void *user,
                       double *system_buf) {
  if (!pg || e_begin < 0 || e_end < e_begin || e_end > pg->n_e) {
    g_pg_err = "bad shard";
    return LSLAM_ERR_INVALID;
  }
  PG_TRY(hipSetDevice(pg->device));
  pg->allreduce = fn;
  pg->allreduce_user = user;
  if (system_buf) {
    pg->d_sys.adopt(system_buf, pg->sys_doubles());
  }
  return build_shard(pg, e_begin, e_end);
}

int lslam_pg_linearize(lslam_pg *pg, double *diag_out, double *off_out, int32_t *off_ij_out, double *b_out,
                       double *chi2_out) {
  if (!pg) return LSLAM_ERR_INVALID;
  PG_TRY(hipSetDevice(pg->device));
  int rc = linearize(pg, pg->d_poses.p);
  if (rc) return rc;
  if (diag_out) PG_TRY(hipMemcpyAsync(diag_out, pg->diag(), (size_t)pg->n_v * 36 * 8, hipMemcpyDeviceToHost, pg->stream));
  if (off_out) PG_TRY(hipMemcpyAsync(off_out, pg->off(), (size_t)pg->n_off * 36 * 8, hipMemcpyDeviceToHost, pg->stream));
  if (b_out) PG_TRY(hipMemcpyAsync(b_out, pg->b(), (size_t)pg->n_v * 6 * 8, hipMemcpyDeviceToHost, pg->stream));
  if (chi2_out) PG_TRY(hipMemcpyAsync(chi2_out, pg->chi(), 8, hipMemcpyDeviceToHost, pg->stream));
  PG_TRY(hipStreamSynchronize(pg->stream));
  if (off_ij_out) std::memcpy(off_ij_out, pg->off_pairs.data(), pg->off_pairs.size() * sizeof(int32_t));
  return LSLAM_OK;
}

// ---- robust kernels on edges -------------------------------------------------------------------------------------------
int lslam_pg_kernel_from_name(const char *name) {
  static const char *const names[4] = {"NONE", "Huber", "Cauchy", "DCS"};
  if (!name) return -1;
  for (int k = 0; k < 4; ++k)
    if (std::strcmp(names[k], name) == 0) return k;
  return -1;
}
int lslam_pg_set_robust_kernels(lslam_pg *pg, const int32_t *kind, const double *delta) {
  if (!pg) return LSLAM_ERR_INVALID;
  if ((kind == nullptr) != (delta == nullptr)) {
    g_pg_err = "robust kernels: kind and delta are given together, or both NULL to clear";
    return LSLAM_ERR_INVALID;
  }
  PG_TRY(hipSetDevice(pg->device));
  if (!kind) {  // the plain solver again
    pg->robust = false;
    pg->h_kind.clear();
    return LSLAM_OK;
  }
  bool any = false;
  for (int e = 0; e < pg->n_e; ++e) {  // everything is checked before anything changes
    if (kind[e] < LSLAM_PG_KERNEL_NONE || kind[e] > LSLAM_PG_KERNEL_DCS) {
      g_pg_err = "robust kernels: unknown kind " + std::to_string(kind[e]) + " on edge " + std::to_string(e);
      return LSLAM_ERR_INVALID;
    }
    if (kind[e] == LSLAM_PG_KERNEL_NONE) continue;
    any = true;
    if (!std::isfinite(delta[e]) || !(delta[e] > 0.0)) {
      g_pg_err = "robust kernels: delta must be finite and > 0 (edge " + std::to_string(e) + ")";
      return LSLAM_ERR_INVALID;
    }
  }
  if (!any) {  // every edge NONE: nothing to weight
    pg->robust = false;
    pg->h_kind.clear();
    return LSLAM_OK;
  }
  std::vector<int32_t> hk(kind, kind + pg->n_e);
  std::vector<double> hd(delta, delta + pg->n_e);
  for (int e = 0; e < pg->n_e; ++e)
    if (hk[e] == LSLAM_PG_KERNEL_NONE) hd[e] = 1.0;  // ignored; never a NaN in device memory
  PG_TRY(hipStreamSynchronize(pg->stream));  // nothing in flight still reads the arrays replaced here
  PG_TRY(dev_upload(pg->d_kind, hk));
  PG_TRY(dev_upload(pg->d_delta, hd));
  pg->h_kind.swap(hk);
  pg->robust = true;
  return LSLAM_OK;
}

// e2 / rho0 / rho1 of every edge into pg->d_tap, at `poses7` (host; NULL: the current estimate), and back to `host` [3 n_e]
static int robust_tap(lslam_pg *pg, const double *poses7, std::vector<double> &host) {
  host.assign(3 * (size_t)pg->n_e, 0.0);
  if (pg->n_e == 0) return LSLAM_OK;
  const double *poses = pg->d_poses.p;
  if (poses7) {
    PG_TRY(pg->d_tap_poses.alloc((size_t)pg->n_v * 7));
    PG_TRY(hipMemcpyAsync(pg->d_tap_poses.p, poses7, (size_t)pg->n_v * 7 * 8, hipMemcpyHostToDevice, pg->stream));
    poses = pg->d_tap_poses.p;
  }
  const size_t ne = (size_t)pg->n_e;
  PG_TRY(pg->d_tap.alloc(3 * ne));
  hipLaunchKernelGGL(pg_edge_robust_tap_kernel, dim3((pg->n_e + 127) / 128), dim3(128), 0, pg->stream, poses, pg->d_ij.p,
                     pg->d_meas.p, pg->d_info.p, pg->n_e, pg->robust ? pg->d_kind.p : (const int32_t *)nullptr,
                     pg->robust ? pg->d_delta.p : (const double *)nullptr, pg->d_tap.p, pg->d_tap.p + ne,
                     pg->d_tap.p + 2 * ne);
  PG_TRY(hipGetLastError());
  PG_TRY(hipMemcpyAsync(host.data(), pg->d_tap.p, 3 * ne * 8, hipMemcpyDeviceToHost, pg->stream));
  PG_TRY(hipStreamSynchronize(pg->stream));
  return LSLAM_OK;
}

int lslam_pg_edge_robust(lslam_pg *pg, const double *poses7, double *e2, double *rho, double *weight) {
  if (!pg) return LSLAM_ERR_INVALID;
  PG_TRY(hipSetDevice(pg->device));
  std::vector<double> h;
  const int rc = robust_tap(pg, poses7, h);
  if (rc) return rc;
  const size_t ne = (size_t)pg->n_e;
  if (e2 && ne) std::memcpy(e2, h.data(), ne * 8);
  if (rho && ne) std::memcpy(rho, h.data() + ne, ne * 8);
  if (weight && ne) std::memcpy(weight, h.data() + 2 * ne, ne * 8);
  return LSLAM_OK;
}

int lslam_pg_robust_info(lslam_pg *pg, int32_t *n_robust, int32_t *n_downweighted, double *chi2_plain) {
  if (!pg) return LSLAM_ERR_INVALID;
  PG_TRY(hipSetDevice(pg->device));
  std::vector<double> h;
  const int rc = robust_tap(pg, nullptr, h);
  if (rc) return rc;
  const size_t ne = (size_t)pg->n_e;
  int nr = 0, nd = 0;
  double sum = 0.0;
  for (size_t e = 0; e < ne; ++e) {  // edge order
    sum += h[e];
    if (pg->robust && pg->h_kind[e] != LSLAM_PG_KERNEL_NONE) {
      ++nr;
      if (h[2 * ne + e] < 1.0) ++nd;
    }
  }
  if (n_robust) *n_robust = nr;
  if (n_downweighted) *n_downweighted = nd;
  if (chi2_plain) *chi2_plain = sum;
  return LSLAM_OK;
}

// ---- unary constraints ----------------------------------------------------------------------------------------------------
int lslam_pg_set_priors(lslam_pg *pg, int32_t n_priors, const int32_t *vertex, const int32_t *type, const double *meas7,
                        const double *info36, const int32_t *kind, const double *delta) {
  if (!pg || n_priors < 0 || (n_priors > 0 && (!vertex || !type || !meas7 || !info36))) {
    g_pg_err = "priors: bad arguments";
    return LSLAM_ERR_INVALID;
  }
  if ((kind == nullptr) != (delta == nullptr)) {
    g_pg_err = "priors: kind and delta are given together, or both NULL";
    return LSLAM_ERR_INVALID;
  }
  PG_TRY(hipSetDevice(pg->device));
  const size_t n = (size_t)n_priors;
  std::vector<double> dm(7 * n), di(36 * n, 0.0), dd(n, 1.0);
  bool any_kernel = false;
  for (size_t p = 0; p < n; ++p) {  // everything is checked before anything changes
    const std::string at = " (prior " + std::to_string(p) + ")";
    if (vertex[p] < 0 || vertex[p] >= pg->n_v) {
      g_pg_err = "priors: vertex out of range" + at;
      return LSLAM_ERR_INVALID;
    }
    if (type[p] != LSLAM_PG_PRIOR_XYZ && type[p] != LSLAM_PG_PRIOR_POSE) {
      g_pg_err = "priors: unknown type " + std::to_string(type[p]) + at;
      return LSLAM_ERR_INVALID;
    }
    const bool pose = type[p] == LSLAM_PG_PRIOR_POSE;
    const double *m = meas7 + 7 * p, *w = info36 + 36 * p;
    for (int k = 0; k < (pose ? 7 : 3); ++k)
      if (!std::isfinite(m[k])) {
        g_pg_err = "priors: measurement is not finite" + at;
        return LSLAM_ERR_INVALID;
      }
    if (pose && !(m[3] * m[3] + m[4] * m[4] + m[5] * m[5] + m[6] * m[6] > 0.0)) {
      g_pg_err = "priors: zero-norm quaternion" + at;
      return LSLAM_ERR_INVALID;
    }
    const int d = pose ? 6 : 3;  // the block that is used
    double big = 0.0;
    for (int r = 0; r < d; ++r)
      for (int c = 0; c < d; ++c) {
        if (!std::isfinite(w[r * 6 + c])) {
          g_pg_err = "priors: information is not finite" + at;
          return LSLAM_ERR_INVALID;
        }
        big = std::max(big, std::fabs(w[r * 6 + c]));
      }
    for (int r = 0; r < d; ++r) {
      if (w[r * 6 + r] < 0.0) {
        g_pg_err = "priors: information has a negative diagonal entry" + at;
        return LSLAM_ERR_INVALID;
      }
      for (int c = r + 1; c < d; ++c)
        if (std::fabs(w[r * 6 + c] - w[c * 6 + r]) > 1e-12 * big) {  // (rounding of a product A A^T is far below this)
          g_pg_err = "priors: information is not symmetric" + at;
          return LSLAM_ERR_INVALID;
        }
    }
    if (kind) {
      if (kind[p] < LSLAM_PG_KERNEL_NONE || kind[p] > LSLAM_PG_KERNEL_DCS) {
        g_pg_err = "priors: unknown robust kernel " + std::to_string(kind[p]) + at;
        return LSLAM_ERR_INVALID;
      }
      if (kind[p] != LSLAM_PG_KERNEL_NONE) {
        if (!std::isfinite(delta[p]) || !(delta[p] > 0.0)) {
          g_pg_err = "priors: delta must be finite and > 0" + at;
          return LSLAM_ERR_INVALID;
        }
        any_kernel = true;
        dd[p] = delta[p];
      }
    }
    // the device's copy: what the kernels read, nothing else (never a NaN in device memory)
    for (int k = 0; k < 3; ++k) dm[7 * p + k] = m[k];
    // (a POSE prior's quaternion normalised: edge_error takes the measurement's as a unit quaternion)
    const double qn = pose ? std::sqrt(m[3] * m[3] + m[4] * m[4] + m[5] * m[5] + m[6] * m[6]) : 1.0;
    for (int k = 3; k < 7; ++k) dm[7 * p + k] = pose ? m[k] / qn : (k == 6 ? 1.0 : 0.0);
    for (int r = 0; r < d; ++r)
      for (int c = 0; c < d; ++c) di[36 * p + r * 6 + c] = w[r * 6 + c];
  }
  PG_TRY(hipStreamSynchronize(pg->stream));  // nothing in flight still reads the arrays replaced here
  std::vector<int32_t> hv(vertex, vertex + n), ht(type, type + n), hk(n, LSLAM_PG_KERNEL_NONE);
  if (kind) hk.assign(kind, kind + n);
  // From here on only a device error can stop the call: the graph then has NO priors (n_p = 0 until every array of the new
  // set is in place), never a mixture of the old set's sizes and the new set's arrays.
  pg->n_p = 0;
  pg->prior_robust = false;
  pg->h_pv.clear();
  pg->h_ptype.clear();
  if (n > 0) {
    std::vector<int32_t> pptr((size_t)pg->n_v + 1, 0), padj(n);
    for (size_t p = 0; p < n; ++p) pptr[(size_t)hv[p] + 1]++;
    for (int v = 0; v < pg->n_v; ++v) pptr[(size_t)v + 1] += pptr[v];
    std::vector<int32_t> pc(pptr.begin(), pptr.end() - 1);
    for (size_t p = 0; p < n; ++p) padj[pc[hv[p]]++] = (int32_t)p;  // prior order = summation order
    PG_TRY(dev_upload(pg->d_pv, hv));
    PG_TRY(dev_upload(pg->d_ptype, ht));
    PG_TRY(dev_upload(pg->d_pmeas, dm));
    PG_TRY(dev_upload(pg->d_pinfo, di));
    PG_TRY(dev_upload(pg->d_pkind, hk));
    PG_TRY(dev_upload(pg->d_pdelta, dd));
    PG_TRY(dev_upload(pg->d_pptr, pptr));
    PG_TRY(dev_upload(pg->d_padj, padj));
    PG_TRY(pg->d_prec.alloc(n * PREC));
  }
  if ((size_t)(pg->e_end - pg->e_begin) + n + (size_t)pg->n_q > pg->d_chi.cap)  // the priors' chi2 values sit behind the edges'
    PG_TRY(pg->d_chi.alloc((size_t)(pg->e_end - pg->e_begin) + n + (size_t)pg->n_q));
  pg->n_p = (int)n;
  pg->prior_robust = any_kernel;
  pg->h_pv.swap(hv);
  pg->h_ptype.swap(ht);
  pg->h_pkind.swap(hk);
  pg->h_pmeas.assign(meas7, meas7 + 7 * n);
  pg->h_pinfo.assign(info36, info36 + 36 * n);
  pg->h_pdelta.swap(dd);
  return LSLAM_OK;
}

int32_t lslam_pg_num_priors(const lslam_pg *pg) { return pg ? pg->n_p : 0; }

int lslam_pg_prior_robust(lslam_pg *pg, const double *poses7, double *e2, double *rho, double *weight) {
  if (!pg) return LSLAM_ERR_INVALID;
  PG_TRY(hipSetDevice(pg->device));
  const size_t n = (size_t)pg->n_p;
  if (n == 0) return LSLAM_OK;
  const double *poses = pg->d_poses.p;
  if (poses7) {
    PG_TRY(pg->d_tap_poses.alloc((size_t)pg->n_v * 7));
    PG_TRY(hipMemcpyAsync(pg->d_tap_poses.p, poses7, (size_t)pg->n_v * 7 * 8, hipMemcpyHostToDevice, pg->stream));
    poses = pg->d_tap_poses.p;
  }
  PG_TRY(pg->d_ptap.alloc(3 * n));
  hipLaunchKernelGGL(pg_prior_tap_kernel, dim3((pg->n_p + 127) / 128), dim3(128), 0, pg->stream, poses, pg->d_pv.p,
                     pg->d_ptype.p, pg->d_pmeas.p, pg->d_pinfo.p, pg->n_p,
                     pg->prior_robust ? pg->d_pkind.p : (const int32_t *)nullptr,
                     pg->prior_robust ? pg->d_pdelta.p : (const double *)nullptr, pg->d_ptap.p, pg->d_ptap.p + n,
                     pg->d_ptap.p + 2 * n);
  PG_TRY(hipGetLastError());
  std::vector<double> h(3 * n);
  PG_TRY(hipMemcpyAsync(h.data(), pg->d_ptap.p, 3 * n * 8, hipMemcpyDeviceToHost, pg->stream));
  PG_TRY(hipStreamSynchronize(pg->stream));
  if (e2) std::memcpy(e2, h.data(), n * 8);
  if (rho) std::memcpy(rho, h.data() + n, n * 8);
  if (weight) std::memcpy(weight, h.data() + 2 * n, n * 8);
  return LSLAM_OK;
}

// ---- plane priors ----------------------------------------------------------------------------------------------------------
int lslam_pg_set_plane_priors(lslam_pg *pg, int32_t n_priors, const int32_t *vertex, const double *world4, const double *meas4,
                              const double *info9, const int32_t *kind, const double *delta) {
  if (!pg || n_priors < 0 || (n_priors > 0 && (!vertex || !world4 || !meas4 || !info9))) {
    g_pg_err = "plane priors: bad arguments";
    return LSLAM_ERR_INVALID;
  }
  if ((kind == nullptr) != (delta == nullptr)) {
    g_pg_err = "plane priors: kind and delta are given together, or both NULL";
    return LSLAM_ERR_INVALID;
  }
  PG_TRY(hipSetDevice(pg->device));
  const size_t n = (size_t)n_priors;
  std::vector<double> dp(QPL * n), di(36 * n, 0.0), dd(n, 1.0), poses;
  if (n > 0) {  // the current estimate: a world / measured pair must face the same way under it
    poses.resize((size_t)pg->n_v * 7);
    PG_TRY(hipMemcpyAsync(poses.data(), pg->d_poses.p, poses.size() * 8, hipMemcpyDeviceToHost, pg->stream));
    PG_TRY(hipStreamSynchronize(pg->stream));
  }
  bool any_kernel = false;
  for (size_t p = 0; p < n; ++p) {  // everything is checked before anything changes
    const std::string at = " (plane prior " + std::to_string(p) + ")";
    if (vertex[p] < 0 || vertex[p] >= pg->n_v) {
      g_pg_err = "plane priors: vertex out of range" + at;
      return LSLAM_ERR_INVALID;
    }
    const double *pl[2] = {world4 + 4 * p, meas4 + 4 * p};
    for (int s = 0; s < 2; ++s) {
      for (int k = 0; k < 4; ++k)
        if (!std::isfinite(pl[s][k])) {
          g_pg_err = std::string("plane priors: ") + (s ? "measured" : "world") + " plane is not finite" + at;
          return LSLAM_ERR_INVALID;
        }
      const double nn = std::sqrt(pl[s][0] * pl[s][0] + pl[s][1] * pl[s][1] + pl[s][2] * pl[s][2]);
      if (!(nn > 0.0) || !std::isfinite(nn)) {
        g_pg_err = std::string("plane priors: ") + (s ? "measured" : "world") + " plane has a zero normal" + at;
        return LSLAM_ERR_INVALID;
      }
      // (the plane n.p + d = 0 scaled to a unit normal: d scales with it)
      for (int k = 0; k < 4; ++k) dp[QPL * p + 4 * s + k] = pl[s][k] / nn;
    }
    const double *w = info9 + 9 * p;
    double big = 0.0;
    for (int k = 0; k < 9; ++k) {
      if (!std::isfinite(w[k])) {
        g_pg_err = "plane priors: information is not finite" + at;
        return LSLAM_ERR_INVALID;
      }
      big = std::max(big, std::fabs(w[k]));
    }
    for (int r = 0; r < 3; ++r) {
      if (w[r * 3 + r] < 0.0) {
        g_pg_err = "plane priors: information has a negative diagonal entry" + at;
        return LSLAM_ERR_INVALID;
      }
      for (int c = r + 1; c < 3; ++c)
        if (std::fabs(w[r * 3 + c] - w[c * 3 + r]) > 1e-12 * big) {
          g_pg_err = "plane priors: information is not symmetric" + at;
          return LSLAM_ERR_INVALID;
        }
    }
    if (kind) {
      if (kind[p] < LSLAM_PG_KERNEL_NONE || kind[p] > LSLAM_PG_KERNEL_DCS) {
        g_pg_err = "plane priors: unknown robust kernel " + std::to_string(kind[p]) + at;
        return LSLAM_ERR_INVALID;
      }
      if (kind[p] != LSLAM_PG_KERNEL_NONE) {
        if (!std::isfinite(delta[p]) || !(delta[p] > 0.0)) {
          g_pg_err = "plane priors: delta must be finite and > 0" + at;
          return LSLAM_ERR_INVALID;
        }
        any_kernel = true;
        dd[p] = delta[p];
      }
    }
    {  // n_l = R^T n_w against n_m
      const double *x = poses.data() + 7 * (size_t)vertex[p];
      const double qn = std::sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5] + x[6] * x[6]);
      const double qx = x[3] / qn, qy = x[4] / qn, qz = x[5] / qn, qw = x[6] / qn;
      const double R[9] = {1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw),
                           2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw),
                           2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)};
      const double *nw = dp.data() + QPL * p, *nm = nw + 4;
      double dot = 0.0;
      for (int c = 0; c < 3; ++c) dot += (R[c] * nw[0] + R[3 + c] * nw[1] + R[6 + c] * nw[2]) * nm[c];
      if (!(dot >= 0.0)) {
        g_pg_err = "plane priors: world and measured normals lie in opposite hemispheres at the current estimate" + at;
        return LSLAM_ERR_INVALID;
      }
    }
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) di[36 * p + r * 6 + c] = w[r * 3 + c];
  }
  PG_TRY(hipStreamSynchronize(pg->stream));  // nothing in flight still reads the arrays replaced here
  std::vector<int32_t> hv(vertex, vertex + n), hk(n, LSLAM_PG_KERNEL_NONE);
  if (kind) hk.assign(kind, kind + n);
  // From here on only a device error can stop the call: the graph then has NO plane priors, as for lslam_pg_set_priors
  pg->n_q = 0;
  pg->plane_robust = false;
  pg->h_qv.clear();
  if (n > 0) {
    std::vector<int32_t> qptr((size_t)pg->n_v + 1, 0), qadj(n);
    for (size_t p = 0; p < n; ++p) qptr[(size_t)hv[p] + 1]++;
    for (int v = 0; v < pg->n_v; ++v) qptr[(size_t)v + 1] += qptr[v];
    std::vector<int32_t> qc(qptr.begin(), qptr.end() - 1);
    for (size_t p = 0; p < n; ++p) qadj[qc[hv[p]]++] = (int32_t)p;  // plane-prior order = summation order
    PG_TRY(dev_upload(pg->d_qv, hv));
    PG_TRY(dev_upload(pg->d_qpl, dp));
    PG_TRY(dev_upload(pg->d_qinfo, di));
    PG_TRY(dev_upload(pg->d_qkind, hk));
    PG_TRY(dev_upload(pg->d_qdelta, dd));
    PG_TRY(dev_upload(pg->d_qptr, qptr));
    PG_TRY(dev_upload(pg->d_qadj, qadj));
    PG_TRY(pg->d_qrec.alloc(n * PREC));
  }
  const size_t chi_need = (size_t)(pg->e_end - pg->e_begin) + (size_t)pg->n_p + n;
  if (chi_need > pg->d_chi.cap) PG_TRY(pg->d_chi.alloc(chi_need));
  pg->n_q = (int)n;
  pg->plane_robust = any_kernel;
  pg->h_qv.swap(hv);
  pg->h_qkind.swap(hk);
  pg->h_qworld.assign(world4, world4 + 4 * n);
  pg->h_qmeas.assign(meas4, meas4 + 4 * n);
  pg->h_qinfo.assign(info9, info9 + 9 * n);
  pg->h_qdelta.swap(dd);
  return LSLAM_OK;
}

int32_t lslam_pg_num_plane_priors(const lslam_pg *pg) { return pg ? pg->n_q : 0; }

int lslam_pg_plane_prior_robust(lslam_pg *pg, const double *poses7, double *e2, double *rho, double *weight) {
  if (!pg) return LSLAM_ERR_INVALID;
  PG_TRY(hipSetDevice(pg->device));
  const size_t n = (size_t)pg->n_q;
  if (n == 0) return LSLAM_OK;
  const double *poses = pg->d_poses.p;
  if (poses7) {
    PG_TRY(pg->d_tap_poses.alloc((size_t)pg->n_v * 7));
    PG_TRY(hipMemcpyAsync(pg->d_tap_poses.p, poses7, (size_t)pg->n_v * 7 * 8, hipMemcpyHostToDevice, pg->stream));
    poses = pg->d_tap_poses.p;
  }
  PG_TRY(pg->d_qtap.alloc(3 * n));
  hipLaunchKernelGGL(pg_plane_prior_chi2_kernel, dim3((pg->n_q + 127) / 128), dim3(128), 0, pg->stream, poses, pg->d_qv.p,
                     pg->d_qpl.p, pg->d_qinfo.p, pg->n_q, pg->plane_robust ? pg->d_qkind.p : (const int32_t *)nullptr,
                     pg->plane_robust ? pg->d_qdelta.p : (const double *)nullptr, pg->d_qtap.p, pg->d_qtap.p + n,
                     pg->d_qtap.p + 2 * n);
  PG_TRY(hipGetLastError());
  std::vector<double> h(3 * n);
  PG_TRY(hipMemcpyAsync(h.data(), pg->d_qtap.p, 3 * n * 8, hipMemcpyDeviceToHost, pg->stream));
  PG_TRY(hipStreamSynchronize(pg->stream));
  if (e2) std::memcpy(e2, h.data(), n * 8);
  if (rho) std::memcpy(rho, h.data() + n, n * 8);
  if (weight) std::memcpy(weight, h.data() + 2 * n, n * 8);
  return LSLAM_OK;
}

// The plane priors of a file lslam_pg_save_g2o wrote (host only), in file order; as lslam_g2o_read_priors.
int lslam_g2o_read_plane_priors(const char *path, int32_t *n_priors, int32_t *vertex, double *world4, double *meas4, double *info9) {
  if (!path || !n_priors) return LSLAM_ERR_INVALID;
  std::ifstream ifs(path);
  if (!ifs) {
    g_pg_err = std::string("cannot open ") + path;
    return LSLAM_ERR_INVALID;
  }
  std::map<long, int> ids;
  int nv = 0, np = 0;
  const int cap = *n_priors;
  std::string line, tag;
  while (std::getline(ifs, line)) {
    std::istringstream ls(line);
    if (!(ls >> tag)) continue;
    if (tag == "VERTEX_SE3:QUAT") {
      long id;
      if (ls >> id) ids[id] = nv++;
    } else if (tag == "EDGE_SE3_PRIOR_PLANE") {
      long v;
      double m[8], u[6];
      ls >> v;
      for (int k = 0; k < 8; ++k) ls >> m[k];
      for (int k = 0; k < 6; ++k) ls >> u[k];
      if (!ls) { g_pg_err = "malformed " + tag + " line"; return LSLAM_ERR_INVALID; }
      auto iv = ids.find(v);
      if (iv == ids.end()) { g_pg_err = "plane prior refers to an unknown vertex"; return LSLAM_ERR_INVALID; }
      if (np < cap) {
        if (vertex) vertex[np] = iv->second;
        if (world4) for (int k = 0; k < 4; ++k) world4[(size_t)np * 4 + k] = m[k];
        if (meas4) for (int k = 0; k < 4; ++k) meas4[(size_t)np * 4 + k] = m[4 + k];
        if (info9) {
          int q = 0;
          for (int r = 0; r < 3; ++r)
            for (int c = r; c < 3; ++c) {
              info9[(size_t)np * 9 + r * 3 + c] = u[q];
              info9[(size_t)np * 9 + c * 3 + r] = u[q];
              ++q;
            }
        }
      }
      ++np;
    }
  }
  *n_priors = np;
  return LSLAM_OK;
}

// The fixed vertex is no unknown (g2o removes it; here its row is the identity with a zero right-hand side and no coupling): its
// step is exactly zero.  Block-Jacobi PCG keeps it so; the second preconditioner level prolongs an aggregate's correction onto
// every member, the fixed one included, and PCG then only drives that row back to within its tolerance (~1e-9 seen).
static int zero_fixed_step(lslam_pg *pg) {
  if (pg->fixed < 0) return LSLAM_OK;
  PG_TRY(hipMemsetAsync(pg->d_x.p + (size_t)pg->fixed * 6, 0, 6 * sizeof(double), pg->stream));
  return LSLAM_OK;
}

int lslam_pg_solve(lslam_pg *pg, double lambda, double *dx_out, int32_t *cg_iters) {
  if (!pg) return LSLAM_ERR_INVALID;
  PG_TRY(hipSetDevice(pg->device));
  int it = 0;
  int rc = solve(pg, lambda, 4000, 1e-10, &it);
  if (rc) return rc;
  rc = zero_fixed_step(pg);
  if (rc) return rc;
  if (dx_out) {
    PG_TRY(hipMemcpyAsync(dx_out, pg->d_x.p, (size_t)pg->n_v * 6 * 8, hipMemcpyDeviceToHost, pg->stream));
    PG_TRY(hipStreamSynchronize(pg->stream));
  }
  if (cg_iters) *cg_iters = it;
  return LSLAM_OK;
}

// Profiling tap (-DLSLAM_PK_CLOCKS builds): accumulated per-phase time of the persistent PCG kernel, 100 MHz ticks.
int lslam_pg_debug_clocks(lslam_pg *pg, double out[12]) {
  if (!pg || !out) return LSLAM_ERR_INVALID;
  PG_TRY(hipSetDevice(pg->device));
  PG_TRY(hipMemcpy(out, pg->d_scal.p + 8, 12 * sizeof(double), hipMemcpyDeviceToHost));
  return LSLAM_OK;
}

int lslam_pg_get_poses(lslam_pg *pg, double *poses7) {
  if (!pg || !poses7) return LSLAM_ERR_INVALID;
  PG_TRY(hipSetDevice(pg->device));
  PG_TRY(hipMemcpyAsync(poses7, pg->d_poses.p, (size_t)pg->n_v * 7 * 8, hipMemcpyDeviceToHost, pg->stream));
  PG_TRY(hipStreamSynchronize(pg->stream));
  return LSLAM_OK;
}

// SolverG2O::save (solver_g2o.cpp:97-100 -> g2o::OptimizableGraph::save): the graph in g2o's text
// format -- VERTEX_SE3:QUAT id x y z qx qy qz qw, FIX id, EDGE_SE3:QUAT i j x y z qx qy qz qw and
// the 21 upper-triangular information entries, row by row -- with the current estimates.  Numbers are
// written with 17 significant digits (g2o uses the stream default of 6; readers accept both).
int lslam_pg_save_g2o(lslam_pg *pg, const char *path) {
  if (!pg || !path) return LSLAM_ERR_INVALID;
  PG_TRY(hipSetDevice(pg->device));
  std::vector<double> poses((size_t)pg->n_v * 7), meas((size_t)pg->n_e * 7), info((size_t)pg->n_e * 36);
  PG_TRY(hipMemcpyAsync(poses.data(), pg->d_poses.p, poses.size() * 8, hipMemcpyDeviceToHost, pg->stream));
  if (pg->n_e) {
    PG_TRY(hipMemcpyAsync(meas.data(), pg->d_meas.p, meas.size() * 8, hipMemcpyDeviceToHost, pg->stream));
    PG_TRY(hipMemcpyAsync(info.data(), pg->d_info.p, info.size() * 8, hipMemcpyDeviceToHost, pg->stream));
  }
  PG_TRY(hipStreamSynchronize(pg->stream));
  std::ofstream ofs(path);
  if (!ofs) {
    g_pg_err = std::string("cannot open ") + path;
    return LSLAM_ERR_INVALID;
  }
  ofs << std::setprecision(17);
  for (int v = 0; v < pg->n_v; ++v) {
    ofs << "VERTEX_SE3:QUAT " << v;
    for (int k = 0; k < 7; ++k) ofs << ' ' << poses[(size_t)v * 7 + k];
    ofs << '\n';
    if (v == pg->fixed) ofs << "FIX " << v << '\n';
  }
  for (int e = 0; e < pg->n_e; ++e) {
    ofs << "EDGE_SE3:QUAT " << pg->h_ij[2 * e] << ' ' << pg->h_ij[2 * e + 1];
    for (int k = 0; k < 7; ++k) ofs << ' ' << meas[(size_t)e * 7 + k];
    for (int r = 0; r < 6; ++r)
      for (int c = r; c < 6; ++c) ofs << ' ' << info[(size_t)e * 36 + r * 6 + c];
    ofs << '\n';
  }
  // Unary constraints: g2o's own EDGE_SE3_PRIOR (vertex, offset parameter id, measurement, 21 upper-triangular entries) with
  // one zero offset parameter in front, and hdl_graph_slam's EDGE_SE3_PRIORXYZ (vertex, x y z, 6 upper-triangular entries).
  // Like an edge's, a prior's robust kernel has no place in the format.
  if (std::find(pg->h_ptype.begin(), pg->h_ptype.end(), (int32_t)LSLAM_PG_PRIOR_POSE) != pg->h_ptype.end())
    ofs << "PARAMS_SE3OFFSET 0 0 0 0 0 0 0 1\n";
  for (int p = 0; p < pg->n_p; ++p) {
    const bool pose = pg->h_ptype[p] == LSLAM_PG_PRIOR_POSE;
    const int d = pose ? 6 : 3;
    ofs << (pose ? "EDGE_SE3_PRIOR " : "EDGE_SE3_PRIORXYZ ") << pg->h_pv[p];
    if (pose) ofs << " 0";
    for (int k = 0; k < (pose ? 7 : 3); ++k) ofs << ' ' << pg->h_pmeas[(size_t)p * 7 + k];
    for (int r = 0; r < d; ++r)
      for (int c = r; c < d; ++c) ofs << ' ' << pg->h_pinfo[(size_t)p * 36 + r * 6 + c];
    ofs << '\n';
  }
  // Plane priors, behind them: this project's OWN tag (no g2o or hdl_graph_slam type reads it) -- vertex, the world plane, the
  // measured plane (both as given), the 6 upper-triangular information entries.  lslam_g2o_read and lslam_g2o_read_priors
  // compare whole tags, so they skip these lines; lslam_g2o_read_plane_priors returns them.
  for (int p = 0; p < pg->n_q; ++p) {
    ofs << "EDGE_SE3_PRIOR_PLANE " << pg->h_qv[p];
    for (int k = 0; k < 4; ++k) ofs << ' ' << pg->h_qworld[(size_t)p * 4 + k];
    for (int k = 0; k < 4; ++k) ofs << ' ' << pg->h_qmeas[(size_t)p * 4 + k];
    for (int r = 0; r < 3; ++r)
      for (int c = r; c < 3; ++c) ofs << ' ' << pg->h_qinfo[(size_t)p * 9 + r * 3 + c];
    ofs << '\n';
  }
  return ofs.good() ? LSLAM_OK : LSLAM_ERR_INVALID;
}

// The unary constraints of such a file (host only), in file order.  *n_priors: in = capacity, out = what the file holds;
// vertices are numbered as lslam_g2o_read numbers them (order of appearance of the VERTEX_SE3:QUAT lines).
int lslam_g2o_read_priors(const char *path, int32_t *n_priors, int32_t *vertex, int32_t *type, double *meas7,
                          double *info36) {
  if (!path || !n_priors) return LSLAM_ERR_INVALID;
  std::ifstream ifs(path);
  if (!ifs) {
    g_pg_err = std::string("cannot open ") + path;
    return LSLAM_ERR_INVALID;
  }
  std::map<long, int> ids;
  int nv = 0, np = 0;
  const int cap = *n_priors;
  std::string line, tag;
  while (std::getline(ifs, line)) {
    std::istringstream ls(line);
    if (!(ls >> tag)) continue;
    if (tag == "VERTEX_SE3:QUAT") {
      long id;
      if (ls >> id) ids[id] = nv++;
    } else if (tag == "EDGE_SE3_PRIOR" || tag == "EDGE_SE3_PRIORXYZ") {
      const bool pose = tag == "EDGE_SE3_PRIOR";
      const int d = pose ? 6 : 3, nm = pose ? 7 : 3, nu = pose ? 21 : 6;
      long v, param;
      double m[7] = {0, 0, 0, 0, 0, 0, 1}, u[21];
      ls >> v;
      if (pose) ls >> param;  // the offset parameter: lslam_pg_save_g2o writes one, the identity
      for (int k = 0; k < nm; ++k) ls >> m[k];
      for (int k = 0; k < nu; ++k) ls >> u[k];
      if (!ls) { g_pg_err = "malformed " + tag + " line"; return LSLAM_ERR_INVALID; }
      auto iv = ids.find(v);
      if (iv == ids.end()) { g_pg_err = "prior refers to an unknown vertex"; return LSLAM_ERR_INVALID; }
      if (np < cap) {
        if (vertex) vertex[np] = iv->second;
        if (type) type[np] = pose ? LSLAM_PG_PRIOR_POSE : LSLAM_PG_PRIOR_XYZ;
        if (meas7) for (int k = 0; k < 7; ++k) meas7[(size_t)np * 7 + k] = m[k];
        if (info36) {
          for (int k = 0; k < 36; ++k) info36[(size_t)np * 36 + k] = 0.0;
          int q = 0;
          for (int r = 0; r < d; ++r)
            for (int c = r; c < d; ++c) {
              info36[(size_t)np * 36 + r * 6 + c] = u[q];
              info36[(size_t)np * 36 + c * 6 + r] = u[q];
              ++q;
            }
        }
      }
      ++np;
    }
  }
  *n_priors = np;
  return LSLAM_OK;
}

// Reader for the same format (host only, no device needed).  Two-call pattern: with NULL arrays it
// returns the counts; vertex ids are mapped to 0..n-1 in order of appearance.
int lslam_g2o_read(const char *path, int32_t *n_vertices, double *poses7, int32_t *n_edges, int32_t *ij,
                   double *meas7, double *info36, int32_t *fixed_vertex) {
  if (!path || !n_vertices || !n_edges) return LSLAM_ERR_INVALID;
  std::ifstream ifs(path);
  if (!ifs) {
    g_pg_err = std::string("cannot open ") + path;
    return LSLAM_ERR_INVALID;
  }
  std::map<long, int> ids;
  int nv = 0, ne = 0, fixed = -1;
  const int cap_v = *n_vertices, cap_e = *n_edges;
  std::string line, tag;
  while (std::getline(ifs, line)) {
    std::istringstream ls(line);
    if (!(ls >> tag)) continue;
    if (tag == "VERTEX_SE3:QUAT") {
      long id;
      double v[7];
      if (!(ls >> id)) continue;
      for (int k = 0; k < 7; ++k) ls >> v[k];
      if (!ls) { g_pg_err = "malformed VERTEX_SE3:QUAT line"; return LSLAM_ERR_INVALID; }
      ids[id] = nv;
      if (poses7 && nv < cap_v) for (int k = 0; k < 7; ++k) poses7[(size_t)nv * 7 + k] = v[k];
      ++nv;
    } else if (tag == "FIX") {
      long id;
      if (ls >> id) { auto it = ids.find(id); if (it != ids.end() && fixed < 0) fixed = it->second; }
    } else if (tag == "EDGE_SE3:QUAT") {
      long a, b;
      double m[7], u[21];
      ls >> a >> b;
      for (int k = 0; k < 7; ++k) ls >> m[k];
      for (int k = 0; k < 21; ++k) ls >> u[k];
      if (!ls) { g_pg_err = "malformed EDGE_SE3:QUAT line"; return LSLAM_ERR_INVALID; }
      auto ia = ids.find(a), ib = ids.find(b);
      if (ia == ids.end() || ib == ids.end()) { g_pg_err = "edge refers to an unknown vertex"; return LSLAM_ERR_INVALID; }
      if (ne < cap_e) {
        if (ij) { ij[2 * ne] = ia->second; ij[2 * ne + 1] = ib->second; }
        if (meas7) for (int k = 0; k < 7; ++k) meas7[(size_t)ne * 7 + k] = m[k];
        if (info36) {
          int q = 0;
          for (int r = 0; r < 6; ++r)
            for (int c = r; c < 6; ++c) {
              info36[(size_t)ne * 36 + r * 6 + c] = u[q];
              info36[(size_t)ne * 36 + c * 6 + r] = u[q];
              ++q;
            }
        }
      }
      ++ne;
    }
  }
  *n_vertices = nv;
  *n_edges = ne;
  if (fixed_vertex) *fixed_vertex = fixed;
  return LSLAM_OK;
}

// g2o OptimizationAlgorithmLevenberg schedule (see oracle/posegraph_oracle.py)
namespace {
struct EventPair {  // destroyed on every exit path
  hipEvent_t a = nullptr, b = nullptr;
  ~EventPair() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

struct LmState {
  double lambda = -1.0, ni = 2.0;  // damping (< 0: not chosen yet) and the factor a rejected trial raises it by
  double cur = 0.0;                // chi2 at the current estimate
  double rho = 0.0;                // gain ratio of the last trial
  int qmax = 0;                    // trials of this iteration
};

// the first iteration's damping: 1e-5 of the largest diagonal entry of H (behind the linearisation on the stream)
int initial_lambda(lslam_pg *pg, double *lambda) {
  hipLaunchKernelGGL(pg_maxdiag_kernel, dim3(1), dim3(256), 0, pg->stream, pg->diag(), pg->n_v, pg->fixed, pg->d_tmp.p + 1);
  PG_TRY(hipGetLastError());
  double md;
  PG_TRY(hipMemcpyAsync(&md, pg->d_tmp.p + 1, 8, hipMemcpyDeviceToHost, pg->stream));
  PG_TRY(hipStreamSynchronize(pg->stream));
  *lambda = 1e-5 * md;
  return LSLAM_OK;
}

// One LM trial at lm.lambda: solve, step, the trial's chi2 and the gain ratio, accept or reject.  *again: another trial of
// this iteration follows (the step was rejected and fewer than ten were tried -- or, sharded, the trial has to be repeated).
int lm_trial(lslam_pg *pg, LmState &lm, lslam_pg_stats &st, bool *again) {
  *again = true;
  int cg = 0;
  // Every damped system is solved to a relative residual of 1e-8 (1e-10 until the PCG was fused; 1e-8 leaves every parity
  // and convergence test unchanged, 1e-6 -- g2o's own PCG default -- shows in the sharded-against-full comparison at 3e-8 m;
  // LSLAM_PG_TOL overrides), however many PCG iterations that takes: near the
  // optimum lambda shrinks, the system of a 5 000-keyframe chain reaches a condition number of ~1e7 and block-Jacobi
  // PCG needs thousands of iterations -- but a TRUNCATED solve leaves exactly the slow (global bending) modes
  // unresolved, and LM then crawls (measured: capped at 800 iterations the 5 k / 25 k graph is still 5 m from its
  // optimum after 2 000 LM iterations; uncapped it arrives in 342).  LSLAM_PG_MAX_CG overrides the cap for A/B runs.
  pg->fell_back = false;
  int rc = solve(pg, lm.lambda, pg->env_max_cg, pg->env_tol, &cg);
  if (rc) return rc;
  rc = zero_fixed_step(pg);
  if (rc) return rc;
  st.cg_iterations += cg;
  hipLaunchKernelGGL(pg_update_kernel, dim3((pg->n_v + 127) / 128), dim3(128), 0, pg->stream, pg->d_poses.p,
                     pg->d_x.p, pg->n_v, pg->fixed, pg->d_trial.p);
  PG_TRY(hipGetLastError());
  // the trial's chi2 and the gain denominator are enqueued together and read back after ONE wait
  double scale;
  rc = eval_chi2(pg, pg->d_trial.p, nullptr);  // enqueue only
  if (rc) return rc;
  hipLaunchKernelGGL(pg_dot_scale_kernel, dim3(pg->n_cg_blocks), dim3(CG_BLOCK), 0, pg->stream, pg->d_x.p,
                     pg->b(), pg->n_v * 6, lm.lambda, pg->d_part.p);
  hipLaunchKernelGGL(pg_sum_kernel, dim3(1), dim3(SUM_BLOCK), 0, pg->stream, pg->d_part.p, pg->n_cg_blocks, 1, pg->d_tmp.p + 2);
  PG_TRY(hipGetLastError());  // a failed launch must not turn into a stale read below
  double chi_flag[2] = {0.0, 0.0};
  PG_TRY(hipMemcpyAsync(chi_flag, pg->chi(), pg->sharded() ? 16 : 8, hipMemcpyDeviceToHost, pg->stream));
  PG_TRY(hipMemcpyAsync(&scale, pg->d_tmp.p + 2, 8, hipMemcpyDeviceToHost, pg->stream));
  PG_TRY(hipStreamSynchronize(pg->stream));
  const double tmp = chi_flag[0];
  if (pg->sharded() && chi_flag[1] > 0.0) {
    // Some rank's persistent kernel timed out (or was refused) in this trial and that rank solved with the launch loop: a
    // different summation order, dx equal to ~1e-8 instead of bit for bit -- and the replicated solve is only useful while
    // every rank takes the same LM decisions.  Every rank switches to the launch loops for good and repeats the trial
    // (one more chi2 all-reduce on every rank: the collectives stay matched).
    pg->pk_fit = 0;
    if (pg->gj_fit == 1) pg->gj_fit = 0;
    pg->coarse_valid = false;
    return LSLAM_OK;
  }
  scale += 1e-3;
  lm.rho = (lm.cur - tmp) / scale;
  st.lm_trials++;
  if (lm.rho > 0 && std::isfinite(tmp)) {
    double alpha = 1.0 - std::pow(2 * lm.rho - 1, 3);
    alpha = std::min(alpha, 2.0 / 3.0);
    lm.lambda *= std::max(1.0 / 3.0, alpha);
    lm.ni = 2.0;
    std::swap(pg->d_poses, pg->d_trial);  // accept
    lm.cur = tmp;
  } else {
    lm.lambda *= lm.ni;
    lm.ni *= 2.0;
  }
  lm.qmax++;
  *again = lm.rho < 0 && lm.qmax < 10;
  return LSLAM_OK;
}
}  // namespace

int lslam_pg_optimize(lslam_pg *pg, int32_t max_iters, lslam_pg_stats *st_out) {
  if (!pg) return LSLAM_ERR_INVALID;
  PG_TRY(hipSetDevice(pg->device));
  lslam_pg_stats st;
  std::memset(&st, 0, sizeof(st));
  EventPair ev;
  PG_TRY(hipEventCreate(&ev.a));
  PG_TRY(hipEventCreate(&ev.b));
  PG_TRY(hipEventRecord(ev.a, pg->stream));
  const int fused0 = pg->fused_solves;
  LmState lm;
  for (int it = 0; it < max_iters; ++it) {
    int rc = linearize(pg, pg->d_poses.p);
    if (rc) return rc;
    PG_TRY(hipMemcpyAsync(&lm.cur, pg->chi(), 8, hipMemcpyDeviceToHost, pg->stream));
    if (lm.lambda < 0) rc = initial_lambda(pg, &lm.lambda);
    if (rc) return rc;
    PG_TRY(hipStreamSynchronize(pg->stream));
    if (it == 0) st.chi2_initial = lm.cur;
    lm.rho = 0.0;
    lm.qmax = 0;
    for (bool again = true; again;) {
      rc = lm_trial(pg, lm, st, &again);
      if (rc) return rc;
    }
    st.iterations = it + 1;
    st.chi2_final = lm.cur;
    st.lambda = lm.lambda;
    if (lm.qmax == 10 || lm.rho == 0) break;
  }
  PG_TRY(hipEventRecord(ev.b, pg->stream));
  PG_TRY(hipStreamSynchronize(pg->stream));
  PG_TRY(hipEventElapsedTime(&st.gpu_ms_total, ev.a, ev.b));
  st.fused_solves = pg->fused_solves - fused0;
  if (st_out) *st_out = st;
  return LSLAM_OK;
}

int lslam_posegraph_optimize(int device, int32_t n_vertices, double *poses7, int32_t n_edges, const int32_t *ij,
                             const double *meas7, const double *info36, int32_t fixed_vertex, int32_t max_iters,
                             lslam_pg_stats *stats) {
  lslam_pg *pg = nullptr;
  int rc = lslam_pg_create(device, n_vertices, poses7, n_edges, ij, meas7, info36, fixed_vertex, &pg);
  if (rc < 0) return rc;
  rc = lslam_pg_optimize(pg, max_iters, stats);
  if (rc >= 0) {
    const int rc2 = lslam_pg_get_poses(pg, poses7);
    if (rc2 < 0) rc = rc2;
  }
  lslam_pg_destroy(pg);
  return rc;
}

}  // extern "C"
