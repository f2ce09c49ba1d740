// lslam_solver_g2o.hpp -- header-only C++ shim with the class surface of the reference's
// pose_graph::SolverG2O (/root/reference/L_SLAM/src/pose_graph/solver_g2o.h:46-72,
// solver_g2o.cpp:51-100) over the C ABI (lslam_pg_* in lslam_c.h), so that the call sites
//   pose_graph/graph.cpp:261,289 (add_se3_node / add_se3_edge), :341 (loop edges), :352 (optimize)
// compile against it unchanged.  Templated on the pose / matrix types so that neither Eigen nor g2o
// is needed to build the backend:
//   Isometry : .matrix()(r,c) read/write, default constructible (Eigen::Isometry3d works)
//   Matrix   : (r,c) read access to a 6x6 (Eigen::MatrixXd works)
// Vertices are returned as pointers with ->id() and ->estimate(), like g2o::VertexSE3*.
#pragma once

#include <cmath>
#include <cstdint>
#include <deque>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "lslam_c.h"

namespace pose_graph {

template <typename Isometry, typename Matrix>
class SolverG2OT {
public:
  struct VertexSE3 {
    int id() const { return _id; }
    Isometry estimate() const { return _owner->estimate_of(_id); }
    int _id;
    SolverG2OT *_owner;
  };
  struct EdgeSE3 { int index; };
  struct EdgeSE3Prior { int index; };  // a unary constraint (lslam_pg_set_priors), by prior index
  struct EdgeSE3Plane { int index; };  // a plane prior (lslam_pg_set_plane_priors), by plane-prior index

  explicit SolverG2OT(int device = 0) : is_first(true), _device(device), _pg(nullptr) {}
  ~SolverG2OT() { lslam_pg_destroy(_pg); }
  SolverG2OT(const SolverG2OT &) = delete;
  SolverG2OT &operator=(const SolverG2OT &) = delete;

  // solver_g2o.cpp:51-63 -- the first vertex is fixed
  VertexSE3 *add_se3_node(const Isometry &pose) {
    pull();
    double p[7];
    to_pose7(pose, p);
    _poses.insert(_poses.end(), p, p + 7);
    is_first = false;
    _vertices.push_back(VertexSE3{(int)_vertices.size(), this});
    return &_vertices.back();
  }
  // solver_g2o.cpp:65-77
  EdgeSE3 *add_se3_edge(VertexSE3 *v1, VertexSE3 *v2, const Isometry &relative_pose, const Matrix &information_matrix) {
    pull();
    double z[7];
    to_pose7(relative_pose, z);
    _ij.push_back(v1->id());
    _ij.push_back(v2->id());
    _meas.insert(_meas.end(), z, z + 7);
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) _info.push_back(information_matrix(r, c));
    _edges.push_back(EdgeSE3{(int)_edges.size()});
    _kind.push_back(LSLAM_PG_KERNEL_NONE);
    _delta.push_back(1.0);
    return &_edges.back();
  }
  // A robust kernel on one edge, with the signature of the solver this one descends from (the reference itself only includes
  // g2o's robust-kernel headers, solver_g2o.h:25-26, and prints the factory's kernels, solver_g2o.cpp:27-28).  kernel_type is
  // "NONE", "Huber", "Cauchy" or "DCS" -- anything else throws -- and kernel_size its delta (g2o: setDelta); semantics in
  // lslam_c.h.  Applied when the device graph is built; kept across add_se3_node / add_se3_edge.
  void add_robust_kernel(EdgeSE3 *edge, const std::string &kernel_type, double kernel_size) {
    if (!edge || edge->index < 0 || edge->index >= (int)_edges.size()) throw std::invalid_argument("add_robust_kernel: no such edge");
    const int kind = lslam_pg_kernel_from_name(kernel_type.c_str());
    if (kind < 0) throw std::invalid_argument("add_robust_kernel: unknown kernel type " + kernel_type);
    // checked here, before anything changes: the library would refuse it only when the device graph is built
    if (kind != LSLAM_PG_KERNEL_NONE && !(std::isfinite(kernel_size) && kernel_size > 0.0))
      throw std::invalid_argument("add_robust_kernel: kernel_size must be finite and > 0");
    _kind[(size_t)edge->index] = kind;
    _delta[(size_t)edge->index] = kernel_size;
    if (_pg) apply_kernels();
  }
  // ---- unary constraints (not in the reference, whose keyframes only carry the utm_coord / imu_quat fields, keyframe.h:40-41;
  // names and meaning of hdl_graph_slam's GraphSLAM, semantics in lslam_c.h).  Vec3: (i) read access; Mat3: (r, c) read access
  // to a 3x3; Quat: .x() .y() .z() .w() (Eigen::Vector3d / Eigen::MatrixXd / Eigen::Quaterniond work).
  // A position fix in the graph frame (GPS): EdgeSE3PriorXYZ.
  template <typename Vec3, typename Mat3>
  EdgeSE3Prior *add_se3_prior_xyz_edge(VertexSE3 *v, const Vec3 &xyz, const Mat3 &information_matrix) {
    double z[7] = {xyz(0), xyz(1), xyz(2), 0.0, 0.0, 0.0, 1.0}, w[36] = {0.0};
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) w[r * 6 + c] = information_matrix(r, c);
    return add_prior(v, LSLAM_PG_PRIOR_XYZ, z, w);
  }
  // An absolute orientation (IMU): EdgeSE3PriorQuat -- a pose prior whose translation block is zero.
  template <typename Quat, typename Mat3>
  EdgeSE3Prior *add_se3_prior_quat_edge(VertexSE3 *v, const Quat &quat, const Mat3 &information_matrix) {
    double z[7] = {0.0, 0.0, 0.0, quat.x(), quat.y(), quat.z(), quat.w()}, w[36] = {0.0};
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) w[(3 + r) * 6 + 3 + c] = information_matrix(r, c);
    return add_prior(v, LSLAM_PG_PRIOR_POSE, z, w);
  }
  // The full form: an absolute pose with a 6x6 information over [translation, rotation] (g2o's EdgeSE3Prior, zero offset).
  EdgeSE3Prior *add_se3_prior_pose_edge(VertexSE3 *v, const Isometry &pose, const Matrix &information_matrix) {
    double z[7], w[36];
    to_pose7(pose, z);
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) w[r * 6 + c] = information_matrix(r, c);
    return add_prior(v, LSLAM_PG_PRIOR_POSE, z, w);
  }
  // add_robust_kernel for a prior: GPS multipath is the outlier case
  void add_robust_kernel(EdgeSE3Prior *prior, const std::string &kernel_type, double kernel_size) {
    if (!prior || prior->index < 0 || prior->index >= (int)_priors.size()) throw std::invalid_argument("add_robust_kernel: no such prior");
    const int kind = lslam_pg_kernel_from_name(kernel_type.c_str());
    if (kind < 0) throw std::invalid_argument("add_robust_kernel: unknown kernel type " + kernel_type);
    if (kind != LSLAM_PG_KERNEL_NONE && !(std::isfinite(kernel_size) && kernel_size > 0.0))
      throw std::invalid_argument("add_robust_kernel: kernel_size must be finite and > 0");
    _pkind[(size_t)prior->index] = kind;
    _pdelta[(size_t)prior->index] = kernel_size;
    if (_pg) apply_priors();
  }
  // the robust weight (rho1) of every prior at the current estimate, by prior index; all 1 without kernels
  std::vector<double> priorWeights() {
    build();
    std::vector<double> w(_priors.size());
    if (lslam_pg_prior_robust(_pg, nullptr, nullptr, nullptr, w.data()) < 0)
      throw std::runtime_error(std::string("lslam_pg_prior_robust: ") + lslam_pg_last_error());
    return w;
  }
  // ---- plane priors (the reference's add_plane_node is commented out, solver_g2o.h:61-65; hdl_graph_slam's floor constraint,
  // semantics in lslam_c.h "plane priors").  The plane `world_plane` = (n, d) of the graph frame was measured as `measured_plane`
  // in v's sensor frame; Vec4: (i) read access (Eigen::Vector4d works); the information is 3x3 over (tangent 1, tangent 2, distance).
  template <typename Vec4, typename Mat3, typename World4>
  EdgeSE3Plane *add_se3_prior_plane_edge(VertexSE3 *v, const Vec4 &measured_plane, const Mat3 &information_matrix,
                                         const World4 &world_plane) {
    if (!v) throw std::invalid_argument("plane prior: no vertex");
    pull();
    _qv.push_back(v->id());
    for (int k = 0; k < 4; ++k) {
      _qworld.push_back(world_plane(k));
      _qmeas.push_back(measured_plane(k));
    }
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) _qinfo.push_back(information_matrix(r, c));
    _qkind.push_back(LSLAM_PG_KERNEL_NONE);
    _qdelta.push_back(1.0);
    _planes.push_back(EdgeSE3Plane{(int)_planes.size()});
    return &_planes.back();
  }
  // ... against the floor z = 0 of the graph frame, (0, 0, 1, 0)
  struct FloorZ0 {
    double operator()(int k) const { return k == 2 ? 1.0 : 0.0; }
  };
  template <typename Vec4, typename Mat3>
  EdgeSE3Plane *add_se3_prior_plane_edge(VertexSE3 *v, const Vec4 &measured_plane, const Mat3 &information_matrix) {
    return add_se3_prior_plane_edge(v, measured_plane, information_matrix, FloorZ0());
  }
  void add_robust_kernel(EdgeSE3Plane *plane, const std::string &kernel_type, double kernel_size) {
    if (!plane || plane->index < 0 || plane->index >= (int)_planes.size()) throw std::invalid_argument("add_robust_kernel: no such plane prior");
    const int kind = lslam_pg_kernel_from_name(kernel_type.c_str());
    if (kind < 0) throw std::invalid_argument("add_robust_kernel: unknown kernel type " + kernel_type);
    if (kind != LSLAM_PG_KERNEL_NONE && !(std::isfinite(kernel_size) && kernel_size > 0.0))
      throw std::invalid_argument("add_robust_kernel: kernel_size must be finite and > 0");
    _qkind[(size_t)plane->index] = kind;
    _qdelta[(size_t)plane->index] = kernel_size;
    if (_pg) apply_plane_priors();
  }
  // the robust weight (rho1) of every plane prior at the current estimate, by plane-prior index; all 1 without kernels
  std::vector<double> planePriorWeights() {
    build();
    std::vector<double> w(_planes.size());
    if (lslam_pg_plane_prior_robust(_pg, nullptr, nullptr, nullptr, w.data()) < 0)
      throw std::runtime_error(std::string("lslam_pg_plane_prior_robust: ") + lslam_pg_last_error());
    return w;
  }
  size_t numPlanePriors() const { return _planes.size(); }
  // true (default, solver_g2o.cpp:55-59): the first vertex is held fixed; false: no vertex is -- for graphs whose priors fix
  // the gauge.  Takes effect when the device graph is next built.
  void setFixFirstNode(bool fix) {
    if (fix == _fix_first) return;
    pull();
    _fix_first = fix;
  }
  // Replaces the graph by the one in a .g2o file written by save(): vertices, edges, priors and whether a vertex is fixed
  // (lslam_g2o_read / lslam_g2o_read_priors).  Vertex and edge pointers handed out before are invalid afterwards.
  void load(const std::string &filename) {
    int32_t nv = 0, ne = 0, np = 0, nq = 0, fixed = -1;
    if (lslam_g2o_read(filename.c_str(), &nv, nullptr, &ne, nullptr, nullptr, nullptr, &fixed) < 0 ||
        lslam_g2o_read_priors(filename.c_str(), &np, nullptr, nullptr, nullptr, nullptr) < 0 ||
        lslam_g2o_read_plane_priors(filename.c_str(), &nq, nullptr, nullptr, nullptr, nullptr) < 0)
      throw std::runtime_error(std::string("load: ") + lslam_pg_last_error());
    std::vector<int32_t> qv((size_t)nq);
    std::vector<double> qworld((size_t)nq * 4), qmeas((size_t)nq * 4), qinfo((size_t)nq * 9);
    if (lslam_g2o_read_plane_priors(filename.c_str(), &nq, qv.data(), qworld.data(), qmeas.data(), qinfo.data()) < 0)
      throw std::runtime_error(std::string("load: ") + lslam_pg_last_error());
    std::vector<double> poses((size_t)nv * 7), meas((size_t)ne * 7), info((size_t)ne * 36), pmeas((size_t)np * 7), pinfo((size_t)np * 36);
    std::vector<int32_t> ij((size_t)ne * 2), pv((size_t)np), pt((size_t)np);
    if (lslam_g2o_read(filename.c_str(), &nv, poses.data(), &ne, ij.data(), meas.data(), info.data(), &fixed) < 0 ||
        lslam_g2o_read_priors(filename.c_str(), &np, pv.data(), pt.data(), pmeas.data(), pinfo.data()) < 0)
      throw std::runtime_error(std::string("load: ") + lslam_pg_last_error());
    if (fixed > 0) throw std::runtime_error("load: only the first vertex can be the fixed one");
    lslam_pg_destroy(_pg);
    _pg = nullptr;
    _vertices.clear();
    _edges.clear();
    _priors.clear();
    for (int k = 0; k < nv; ++k) _vertices.push_back(VertexSE3{k, this});
    for (int k = 0; k < ne; ++k) _edges.push_back(EdgeSE3{k});
    for (int k = 0; k < np; ++k) _priors.push_back(EdgeSE3Prior{k});
    _poses.swap(poses); _meas.swap(meas); _info.swap(info); _ij.swap(ij);
    _pv.swap(pv); _ptype.swap(pt); _pmeas.swap(pmeas); _pinfo.swap(pinfo);
    _kind.assign((size_t)ne, LSLAM_PG_KERNEL_NONE);
    _delta.assign((size_t)ne, 1.0);
    _pkind.assign((size_t)np, LSLAM_PG_KERNEL_NONE);
    _pdelta.assign((size_t)np, 1.0);
    _planes.clear();
    for (int k = 0; k < nq; ++k) _planes.push_back(EdgeSE3Plane{k});
    _qv.swap(qv); _qworld.swap(qworld); _qmeas.swap(qmeas); _qinfo.swap(qinfo);
    _qkind.assign((size_t)nq, LSLAM_PG_KERNEL_NONE);
    _qdelta.assign((size_t)nq, 1.0);
    _fix_first = fixed == 0;
    is_first = nv == 0;
  }
  size_t numPriors() const { return _priors.size(); }
  // the robust weight (rho1) of every edge at the current estimate, by edge index; all 1 without kernels
  std::vector<double> edgeWeights() {
    build();
    std::vector<double> w(_edges.size());
    if (lslam_pg_edge_robust(_pg, nullptr, nullptr, nullptr, w.data()) < 0)
      throw std::runtime_error(std::string("lslam_pg_edge_robust: ") + lslam_pg_last_error());
    return w;
  }
  // solver_g2o.cpp:79-95: graph->optimize(1000) with "lm_var"
  void optimize() {
    build();
    lslam_pg_stats st;
    std::cout << "\n--- g2o optimization ---\nnodes: " << _vertices.size() << "   edges: " << _edges.size() << std::endl;
    if (lslam_pg_optimize(_pg, 1000, &st) < 0) throw std::runtime_error(std::string("lslam_pg_optimize: ") + lslam_pg_last_error());
    _last = st;
    std::cout << "iterations: " << st.iterations << std::endl;
  }
  // solver_g2o.cpp:97-100
  void save(const std::string &filename) {
    build();
    if (lslam_pg_save_g2o(_pg, filename.c_str()) < 0) throw std::runtime_error(lslam_pg_last_error());
  }
  const lslam_pg_stats &lastStats() const { return _last; }
  // ---- marginal covariances (g2o: SparseOptimizer::computeMarginals; lslam_pg_marginals in lslam_c.h, which states the
  // coordinates).  The 6x6 blocks of `vertices` at the current estimate, row-major, 36 doubles each in `cov`; with `cross`
  // the [n][n] cross blocks as well.  opts: rel_tol / max_iters / coarse, zero-initialised = the defaults with coarse = -1.
  // Throws std::runtime_error with the library's message (a vertex without a gauge, a column that does not converge).
  static lslam_pg_marginal_opts defaultMarginalOpts() { lslam_pg_marginal_opts o = {0.0, 0, -1}; return o; }
  void marginals(const std::vector<int> &vertices, std::vector<double> &cov, std::vector<double> *cross = nullptr,
                 const lslam_pg_marginal_opts *opts = nullptr) {
    build();
    const std::vector<int32_t> v(vertices.begin(), vertices.end());
    const size_t n = v.size();
    std::vector<double> c(n * 36), x(cross ? n * n * 36 : 0);
    if (lslam_pg_marginals(_pg, (int32_t)n, v.data(), opts, c.data(), cross ? x.data() : nullptr, &_marginal_stats) < 0)
      throw std::runtime_error(std::string("lslam_pg_marginals: ") + lslam_pg_last_error());
    cov.swap(c);
    if (cross) cross->swap(x);
  }
  // ... and of the relative poses X_ref^-1 X_j, j in `vertices` (lslam_pg_relative_covariances); j == ref: zeros
  void relativeCovariances(int ref, const std::vector<int> &vertices, std::vector<double> &cov,
                           const lslam_pg_marginal_opts *opts = nullptr) {
    build();
    const std::vector<int32_t> v(vertices.begin(), vertices.end());
    std::vector<double> c(v.size() * 36);
    if (lslam_pg_relative_covariances(_pg, ref, (int32_t)v.size(), v.data(), opts, c.data(), &_marginal_stats) < 0)
      throw std::runtime_error(std::string("lslam_pg_relative_covariances: ") + lslam_pg_last_error());
    cov.swap(c);
  }
  const lslam_pg_marginal_stats &marginalStats() const { return _marginal_stats; }
  // No reference counterpart ("lm_var" factorises: its solves are exact).  rel_tol in (0, 1): the relative residual at which a
  // damped solve's PCG stops from now on; 0 (default) leaves the library's 1e-8.  Looser = an inexact LM: same optimum, another
  // trajectory of iterates (lslam_pg_set_solve_tolerance, include/lslam_c.h).
  void setSolveTolerance(double rel_tol) { _solve_tol = rel_tol; if (_pg && rel_tol > 0.0) (void)lslam_pg_set_solve_tolerance(_pg, rel_tol); }

  bool is_first;

private:
  friend struct VertexSE3;
  static void to_pose7(const Isometry &T, double p[7]) {  // {t, Eigen::Quaterniond(R)} (Shepperd)
    double R[3][3];
    Isometry &M = const_cast<Isometry &>(T);
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) R[r][c] = M.matrix()(r, c);
      p[r] = M.matrix()(r, 3);
    }
    const double tr = R[0][0] + R[1][1] + R[2][2];
    double q[4];
    if (tr > 0) {
      double s = std::sqrt(tr + 1.0);
      q[3] = 0.5 * s;
      s = 0.5 / s;
      q[0] = (R[2][1] - R[1][2]) * s; q[1] = (R[0][2] - R[2][0]) * s; q[2] = (R[1][0] - R[0][1]) * s;
    } else {
      int i = 0;
      if (R[1][1] > R[0][0]) i = 1;
      if (R[2][2] > R[i][i]) i = 2;
      const int j = (i + 1) % 3, k = (i + 2) % 3;
      double s = std::sqrt(R[i][i] - R[j][j] - R[k][k] + 1.0);
      q[i] = 0.5 * s;
      s = 0.5 / s;
      q[3] = (R[k][j] - R[j][k]) * s;
      q[j] = (R[j][i] + R[i][j]) * s;
      q[k] = (R[k][i] + R[i][k]) * s;
    }
    for (int k = 0; k < 4; ++k) p[3 + k] = q[k];
  }
  Isometry estimate_of(int id) {
    pull_keep();
    const double *p = &_poses[(size_t)id * 7];
    const double x = p[3], y = p[4], z = p[5], w = p[6];
    Isometry T;
    const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                            {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                            {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) T.matrix()(r, c) = R[r][c];
      T.matrix()(r, 3) = p[r];
      T.matrix()(3, r) = 0.0;
    }
    T.matrix()(3, 3) = 1.0;
    return T;
  }
  void build() {
    if (_pg) return;
    if (_vertices.empty()) throw std::runtime_error("empty pose graph");
    if (lslam_pg_create(_device, (int32_t)_vertices.size(), _poses.data(), (int32_t)_edges.size(), _ij.data(), _meas.data(),
                        _info.data(), _fix_first ? 0 : -1, &_pg) != LSLAM_OK)
      throw std::runtime_error(std::string("lslam_pg_create: ") + lslam_pg_last_error());
    if (_solve_tol > 0.0) (void)lslam_pg_set_solve_tolerance(_pg, _solve_tol);
    apply_kernels();
    if (!_priors.empty()) apply_priors();
    if (!_planes.empty()) apply_plane_priors();
  }
  void apply_plane_priors() {
    bool any = false;
    for (size_t p = 0; p < _qkind.size(); ++p) any = any || _qkind[p] != LSLAM_PG_KERNEL_NONE;
    if (lslam_pg_set_plane_priors(_pg, (int32_t)_planes.size(), _qv.data(), _qworld.data(), _qmeas.data(), _qinfo.data(),
                                  any ? _qkind.data() : nullptr, any ? _qdelta.data() : nullptr) < 0) {
      const std::string why = lslam_pg_last_error();
      lslam_pg_destroy(_pg);  // never a device graph without the plane priors it was asked to carry
      _pg = nullptr;
      throw std::runtime_error("lslam_pg_set_plane_priors: " + why);
    }
  }
  EdgeSE3Prior *add_prior(VertexSE3 *v, int type, const double z[7], const double w[36]) {
    if (!v) throw std::invalid_argument("prior: no vertex");
    pull();
    _pv.push_back(v->id());
    _ptype.push_back(type);
    _pmeas.insert(_pmeas.end(), z, z + 7);
    _pinfo.insert(_pinfo.end(), w, w + 36);
    _pkind.push_back(LSLAM_PG_KERNEL_NONE);
    _pdelta.push_back(1.0);
    _priors.push_back(EdgeSE3Prior{(int)_priors.size()});
    return &_priors.back();
  }
  void apply_priors() {
    bool any = false;
    for (size_t p = 0; p < _pkind.size(); ++p) any = any || _pkind[p] != LSLAM_PG_KERNEL_NONE;
    if (lslam_pg_set_priors(_pg, (int32_t)_priors.size(), _pv.data(), _ptype.data(), _pmeas.data(), _pinfo.data(),
                            any ? _pkind.data() : nullptr, any ? _pdelta.data() : nullptr) < 0) {
      const std::string why = lslam_pg_last_error();
      lslam_pg_destroy(_pg);  // never a device graph without the priors it was asked to carry
      _pg = nullptr;
      throw std::runtime_error("lslam_pg_set_priors: " + why);
    }
  }
  void apply_kernels() {
    bool any = false;
    for (size_t e = 0; e < _kind.size(); ++e) any = any || _kind[e] != LSLAM_PG_KERNEL_NONE;
    if (lslam_pg_set_robust_kernels(_pg, any ? _kind.data() : nullptr, any ? _delta.data() : nullptr) < 0) {
      const std::string why = lslam_pg_last_error();
      lslam_pg_destroy(_pg);  // never a device graph without the kernels it was asked to carry
      _pg = nullptr;
      throw std::runtime_error("lslam_pg_set_robust_kernels: " + why);
    }
  }
  void pull_keep() {  // current estimates into _poses, device graph kept
    if (_pg) lslam_pg_get_poses(_pg, _poses.data());
  }
  void pull() {  // ... and the device graph dropped: the topology is about to change
    if (!_pg) return;
    pull_keep();
    lslam_pg_destroy(_pg);
    _pg = nullptr;
  }

  int _device;
  lslam_pg *_pg;
  lslam_pg_stats _last{};
  lslam_pg_marginal_stats _marginal_stats{};
  double _solve_tol = 0.0;
  std::deque<VertexSE3> _vertices;  // deque: pointers handed out stay valid
  std::deque<EdgeSE3> _edges;
  std::vector<double> _poses, _meas, _info;
  std::vector<int32_t> _ij;
  std::vector<int32_t> _kind;  // per edge: LSLAM_PG_KERNEL_* and its delta
  std::vector<double> _delta;
  bool _fix_first = true;
  std::deque<EdgeSE3Prior> _priors;  // unary constraints: vertex, LSLAM_PG_PRIOR_*, measurement, information, kernel
  std::vector<int32_t> _pv, _ptype, _pkind;
  std::vector<double> _pmeas, _pinfo, _pdelta;
  std::deque<EdgeSE3Plane> _planes;  // plane priors: vertex, world plane, measured plane, 3x3 information, kernel
  std::vector<int32_t> _qv, _qkind;
  std::vector<double> _qworld, _qmeas, _qinfo, _qdelta;
};

}  // namespace pose_graph
