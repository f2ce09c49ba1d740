// lslam_pg_internal.hpp -- what the pose-graph units share: the graph object (lslam_posegraph.hip owns its construction and
// the LM / PCG solver; lslam_pg_marginals.hip solves the same system for panels of unit columns), the second preconditioner
// level's arguments, and the few host entry points one unit offers the other.  Host side only, like lslam_buf.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/lslam_c.h"
#include "lslam_buf.hpp"

namespace lslam {  // lslam_comm.hip
hipError_t comm_allreduce_f64(lslam_comm *comm, double *buf, size_t count, hipStream_t s);
hipError_t comm_allgatherv_f64(lslam_comm *comm, int n_lists, double *const *bufs, const int64_t *const *offs, hipStream_t s);
int comm_world(const lslam_comm *comm);
int comm_rank(const lslam_comm *comm);
const char *debug_env(const char *name);  // lslam_api.hip: a test hook's value, only in a process started with LSLAM_DEBUG_HOOKS=1
}

// ---- second level of the preconditioner (see solve() in lslam_posegraph.hip) ------------------------------------------------
struct CoarseArgs {
  const double *poses;    // current estimate (7 per vertex)
  double *P;              // [n_v][36] prolongation blocks: delta_i = P_i xi_a
  double *Ac;             // [n_c][n_c] coarse matrix, inverted in place
  double *rc, *yc;        // [n_c]
  double *Rbuf, *Cbuf, *Bbuf;  // block Gauss-Jordan scratch: [6][n_c], [n_c][6], [36]
  const int32_t *cb_ptr, *cb_ent, *cb_ab;  // coarse blocks: fine entries of each, its (row, column) aggregate
  const int32_t *agg_of, *agg_ptr, *agg_mem;  // vertex -> aggregate; aggregate -> its members (at most PG_AGG_MAX), first = its origin
  int n_v, G, na, n_c, n_cb, n_cblk;
};

struct lslam_pg {
  int device = 0;
  hipStream_t stream = nullptr;
  int n_v = 0, n_e = 0, fixed = 0, n_off = 0, n_entries = 0;
  int e_begin = 0, e_end = 0;
  lslam_allreduce_fn allreduce = nullptr;
  void *allreduce_user = nullptr;
  lslam_comm *comm = nullptr;  // the library's RCCL communicator (not owned); used when no callback is set
  bool sharded() const { return allreduce != nullptr || comm != nullptr; }
  // in-place sum over the ranks, ordered on the stream
  int reduce(double *buf, size_t count) {
    if (allreduce) {
      if (hipStreamSynchronize(stream) != hipSuccess) return LSLAM_ERR_HIP;
      allreduce(allreduce_user, buf, count);  // contract: complete when it returns
      return LSLAM_OK;
    }
    return lslam::comm_allreduce_f64(comm, buf, count, stream) == hipSuccess ? LSLAM_OK : LSLAM_ERR_COMM;
  }
  // the row-sharded solve's exchange as an all-gather of the owned segments (half the bytes of the zero-padded all-reduce):
  // through the communicator when there is one, else through a callback of its own type (lslam_pg_set_row_gather)
  lslam_allgatherv_fn gatherv = nullptr;
  void *gatherv_user = nullptr;
  int gatherv_rank = -1, gatherv_world = 0;
  int rs_gathered = 0;
  // rank / world of whichever transport can gather; false: only the all-reduce is available
  bool gather_transport(int *rank, int *world) const {
    if (gatherv) { *rank = gatherv_rank; *world = gatherv_world; return true; }
    if (!allreduce && comm) { *rank = lslam::comm_rank(comm); *world = lslam::comm_world(comm); return true; }
    return false;
  }
  int gather(int n_lists, double *const *bufs, const int64_t *const *offs, int world) {
    if (gatherv) {
      if (hipStreamSynchronize(stream) != hipSuccess) return LSLAM_ERR_HIP;
      for (int l = 0; l < n_lists; ++l) gatherv(gatherv_user, bufs[l], offs[l], world);  // contract: complete when it returns
      return LSLAM_OK;
    }
    return lslam::comm_allgatherv_f64(comm, n_lists, bufs, offs, stream) == hipSuccess ? LSLAM_OK : LSLAM_ERR_COMM;
  }
  // graph
  lslam::DevBuf<double> d_poses, d_trial, d_meas, d_info;
  lslam::DevBuf<int32_t> d_ij;
  std::vector<int32_t> h_ij;
  std::vector<int32_t> edge_block;  // per edge: off-diagonal block id
  std::vector<int32_t> off_pairs;   // [n_off][2]
  // robust kernels (lslam_pg_set_robust_kernels): per GLOBAL edge id; `robust` selects the robust instantiations of the edge
  // and chi2 kernels, and is false while no edge carries a kernel -- the plain solver then launches what it always launched
  lslam::DevBuf<int32_t> d_kind;
  lslam::DevBuf<double> d_delta;
  std::vector<int32_t> h_kind;
  bool robust = false;
  lslam::DevBuf<double> d_tap, d_tap_poses;  // lslam_pg_edge_robust: [e2 | rho0 | rho1] of n_e each; caller-supplied poses
  // unary constraints (lslam_pg_set_priors).  n_p == 0 -- the default -- launches exactly what a graph without them launches.
  // The host copies are what the caller gave (save_g2o writes them); the device's info has everything outside an XYZ
  // prior's 3x3 zeroed and its measurement quaternion set to the identity.
  int n_p = 0;
  bool prior_robust = false;  // some prior carries a kernel: the robust instantiations of the prior kernels
  std::vector<int32_t> h_pv, h_ptype, h_pkind;
  std::vector<double> h_pmeas, h_pinfo, h_pdelta;
  lslam::DevBuf<int32_t> d_pv, d_ptype, d_pkind, d_pptr, d_padj;
  lslam::DevBuf<double> d_pmeas, d_pinfo, d_pdelta, d_prec, d_ptap;
  // In a sharded run the system is summed over the ranks, so every prior must be counted once: the rank whose edge range
  // starts at 0 and is not empty carries all of them (a graph without edges: its one range [0, 0) does).
  int local_priors() const { return (e_begin == 0 && (e_end > 0 || n_e == 0)) ? n_p : 0; }
  // plane priors (lslam_pg_set_plane_priors): a set of their own behind the priors above -- in the per-vertex sums, in d_chi
  // and in the file lslam_pg_save_g2o writes.  n_q == 0 -- the default -- launches exactly what a graph without them launches.
  // The host copies are what the caller gave; the device's planes have unit normals, its information is padded to 6x6.
  int n_q = 0;
  bool plane_robust = false;
  std::vector<int32_t> h_qv, h_qkind;
  std::vector<double> h_qworld, h_qmeas, h_qinfo, h_qdelta;
  lslam::DevBuf<int32_t> d_qv, d_qkind, d_qptr, d_qadj;
  lslam::DevBuf<double> d_qpl, d_qinfo, d_qdelta, d_qrec, d_qtap;
  int local_plane_priors() const { return (e_begin == 0 && (e_end > 0 || n_e == 0)) ? n_q : 0; }
  // shard structures
  lslam::DevBuf<double> d_rec, d_chi;
  lslam::DevBuf<int32_t> d_vptr, d_vadj, d_optr, d_oadj;
  // system buffer [diag | off | b | chi2]; owned unless supplied by the caller (adopted)
  lslam::DevBuf<double> d_sys;
  // solver
  lslam::DevBuf<int32_t> d_row_ptr, d_row_col, d_row_src, d_row_of;
  lslam::DevBuf<double> d_vals, d_minv;
  lslam::DevBuf<double> d_x, d_r, d_z, d_p, d_q;
  lslam::DevBuf<double> d_part, d_scal, d_tmp;
  int n_cg_blocks = 0;
  // second level of the preconditioner (rigid motions of graph aggregates of at most `agg` keyframes)
  std::vector<int32_t> h_row_of, h_row_col;
  int agg = 64, n_agg = 0, n_c = 0, n_cb = 0, n_cblk = 0, n_parts = 0;
  lslam::DevBuf<int32_t> d_agg_of, d_agg_ptr, d_agg_mem;
  lslam::DevBuf<double> d_P, d_Ac, d_rc, d_yc, d_gj;
  lslam::DevBuf<int32_t> d_cb_ptr, d_cb_ent, d_cb_ab;
  // environment switches, read when the graph is created (lslam_pg_create) -- never while it is optimised
  bool env_no_reuse = false, env_no_merge = false, env_persistent_off = false, env_debug = false;
  int env_max_cg = 20000;
  double env_tol = 1e-8;
  int coarse_mode = -1;     // -1 automatic (switched on by a solve that needed many iterations), 0 off, 1 on
  bool coarse_on = false;
  int coarse_solves = 0;    // damped systems solved with the second level (statistics)
  // The coarse inverse (with the P it was built from) is a preconditioner, not part of the answer: it is kept across
  // damped solves while it still works -- rebuilt when lambda has moved by more than 10x since it was built, or when the
  // previous solve that used it needed over 1.3x the iterations of the first solve after it was built.  The rule only
  // looks at lambda and iteration counts, which are identical on every rank of a sharded run.
  bool coarse_valid = false;
  double coarse_lambda = 0.0;
  int coarse_fresh_iters = 0, coarse_last_iters = 0;
  int coarse_setups = 0;
  // persistent PCG kernel (pg_pcg_persistent_kernel): per-aggregate entry / column lists, its buffers, whether the graph fits
  lslam::DevBuf<int32_t> d_bent_ptr, d_bent, d_blc, d_bmptr, d_bcol_ptr, d_bcol;
  lslam::DevBuf<double> d_pk;      // [rc0 | rc1] then the exchange slots of pg_pcg_persistent_kernel
  lslam::DevBuf<unsigned> d_bar;
  int pk_lds_cols = 0, pk_lds_items = 0;
  size_t pk_lds_bytes = 0;
  lslam::DevBuf<double> d_gjslots; // pgc_gj_persistent_kernel's pivot-row slots [n_agg][6][n_c]
  int gj_fit = -1;             // as pk_fit, for the coarse inverse
  int pk_fit = -1;             // -1 not decided yet, 0 the multi-launch loop, 1 the persistent kernel
  int fused_solves = 0, total_solves = 0, pk_timeouts = 0;
  bool fell_back = false;      // a persistent kernel gave way to its launch loop during the last solve() (sharded runs: every rank must follow)
  // row-sharded solve (lslam_pg_set_row_shard): this rank's vertex rows [row_v0, row_v1); -1: the solve is replicated
  int row_v0 = -1, row_v1 = -1;
  std::vector<int32_t> h_row_ptr;
  int rs_solves = 0;
  // marginal covariances (lslam_pg_marginals.hip): the panel PCG's vectors [x r z q p0 p1] of 6 n_v x 64 each, its per-block
  // partial sums and per-column scalars, the restricted panel, the gathered result and the small index lists; grown on demand
  lslam::DevBuf<double> d_mg_vec, d_mg_part, d_mg_scal, d_mg_rc, d_mg_out, d_mg_jac;
  lslam::DevBuf<int32_t> d_mg_idx;
  // [diag | off | b | chi2 | fallback flag | exchange area of the row-sharded solve: 6 n_v + 8 + two partial sums per rank]: the system part is all-reduced
  // per linearisation, chi2 + flag per trial, the exchange area per PCG iteration of a row-sharded solve
  size_t core_doubles() const { return (size_t)n_v * 36 + (size_t)n_off * 36 + (size_t)n_v * 6 + 2; }
  static constexpr int RS_MAX_WORLD = 64;  // ranks whose partial sums the exchange area has room for (gather mode)
  size_t sys_doubles() const { return core_doubles() + (size_t)n_v * 6 + 8 + 2 * RS_MAX_WORLD; }
  double *xchg() const { return d_sys.p + core_doubles(); }
  double *diag() const { return d_sys.p; }
  double *off() const { return d_sys.p + (size_t)n_v * 36; }
  double *b() const { return d_sys.p + (size_t)n_v * 36 + (size_t)n_off * 36; }
  double *chi() const { return b() + (size_t)n_v * 6; }
};

namespace lslam {
// what lslam_pg_last_error returns, per thread (lslam_posegraph.hip)
std::string &pg_error();

// lslam_posegraph.hip, for lslam_pg_marginals.hip.
// The system H of lslam_pg_linearize at the current estimate, expanded at lambda = 0 into the solver's block-CSR planes
// (pg->d_vals) with the block-Jacobi inverses (pg->d_minv); with `coarse`, the second level's P and its dense inverse, built
// once by the solver's own build_coarse_inverse, and *c filled.  The inverse is marked stale afterwards: the next damped solve
// of the graph builds its own, as if this call had not happened.
int pg_marginal_system(lslam_pg *pg, bool coarse, CoarseArgs *c);
// The Jacobians [J_ref | J_j] (two row-major 6x6 each, 72 doubles per query) the solver's edge has for an edge (ref, v[k])
// whose measurement is the current relative pose, by the edge's own device function; v is a device array.
int pg_relative_jacobians(lslam_pg *pg, int ref, int n, const int32_t *d_v, double *d_J72);
}  // namespace lslam
