"""Host-side mirror of the reference's pose-graph solver interface over the C ABI.

``PoseGraph`` keeps the method names and argument meaning of ``pose_graph::SolverG2O``
(/root/reference/L_SLAM/src/pose_graph/solver_g2o.h:46-95, solver_g2o.cpp:51-95):
``add_se3_node(pose)`` (the first node is fixed), ``add_se3_edge(v1, v2, relative_pose,
information)``, ``optimize()``.  Poses are 4x4 homogeneous matrices (Eigen::Isometry3d) or
7-vectors {t, q_xyzw}.  The arithmetic runs in the HIP kernels of csrc/lslam_posegraph.hip.
"""
import ctypes as C

import numpy as np

from .capi import (ALLGATHERV_FN, ALLREDUCE_FN, LslamError, LslamPgMarginalOpts, LslamPgMarginalStats, LslamPgStats, c_double_p,
                   c_int32_p, load_library)


def _dp(a):
    return a.ctypes.data_as(c_double_p)


# include/lslam_c.h: LSLAM_PG_KERNEL_*
KERNEL_NONE, KERNEL_HUBER, KERNEL_CAUCHY, KERNEL_DCS = 0, 1, 2, 3
_KERNEL_NAMES = {"none": KERNEL_NONE, "huber": KERNEL_HUBER, "cauchy": KERNEL_CAUCHY, "dcs": KERNEL_DCS}
# include/lslam_c.h: LSLAM_PG_PRIOR_*
PRIOR_XYZ, PRIOR_POSE = 0, 1


def kernel_kind(k):
    """None / "NONE" / "Huber" / "Cauchy" / "DCS" (any case) or an LSLAM_PG_KERNEL_* integer -> the integer.  An integer is
    passed through as it is: the library decides whether it names a kernel."""
    if k is None:
        return KERNEL_NONE
    if isinstance(k, str):
        if k.lower() not in _KERNEL_NAMES:
            raise ValueError("unknown robust kernel %r (NONE, Huber, Cauchy, DCS)" % (k,))
        return _KERNEL_NAMES[k.lower()]
    return int(k)


def mat_to_pose7(T):
    """4x4 -> {t, q_xyzw} (Eigen Quaterniond(R), Shepperd's method)."""
    T = np.asarray(T, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    tr = np.trace(R)
    if tr > 0:
        s = np.sqrt(tr + 1.0)
        w = 0.5 * s
        s = 0.5 / s
        q = [(R[2, 1] - R[1, 2]) * s, (R[0, 2] - R[2, 0]) * s, (R[1, 0] - R[0, 1]) * s, w]
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q = [0.0, 0.0, 0.0, 0.0]
        q[i] = 0.5 * s
        s = 0.5 / s
        q[3] = (R[k, j] - R[j, k]) * s
        q[j] = (R[j, i] + R[i, j]) * s
        q[k] = (R[k, i] + R[i, k]) * s
    return np.array([t[0], t[1], t[2], *q])


def pose7_to_mat(p):
    x, y, z, w = p[3:]
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = p[:3]
    return T


class PoseGraph:
    def __init__(self, device=0, fixed=0):
        """`fixed`: the vertex held at its estimate (the first, as the reference's add_se3_node); -1 holds none -- for graphs
        whose priors fix the gauge."""
        self.lib = load_library()
        self.device = device
        self._nodes = []
        self._ij = []
        self._meas = []
        self._info = []
        self._kind = []   # per edge: LSLAM_PG_KERNEL_* and its delta; applied by _build, so they survive a topology change
        self._delta = []
        self._priors = []  # unary constraints: dicts (vertex, type, meas (7), info (6, 6), kind, delta); applied by _build
        self._plane_priors = []  # plane priors: dicts (vertex, world (4), meas (4), info (3, 3), kind, delta); applied by _build
        self.fixed = int(fixed)  # the vertex lslam_pg_create pins (g2o: setFixed); -1 pins none
        self.h = None
        self._cb = None
        self.last_stats = None
        self.marginal_stats = None  # lslam_pg_marginal_stats of the last marginals() / relative_covariances()

    # ---- SolverG2O interface ------------------------------------------------------
    def add_se3_node(self, pose):
        """solver_g2o.cpp:51-63: returns the vertex id; the first vertex is fixed."""
        p = np.asarray(pose, np.float64)
        self._drop()  # first: it pulls the optimised estimates of the existing vertices back
        self._nodes.append(mat_to_pose7(p) if p.shape == (4, 4) else p.reshape(7).copy())
        return len(self._nodes) - 1

    def add_se3_edge(self, v1, v2, relative_pose, information_matrix, robust_kernel=None, robust_delta=1.0):
        """solver_g2o.cpp:65-77.  ``robust_kernel`` (not in the reference, which only includes g2o's kernel headers): None /
        "NONE", "Huber", "Cauchy" or "DCS" with parameter ``robust_delta`` on this edge, g2o's semantics (lslam_c.h)."""
        z = np.asarray(relative_pose, np.float64)
        kind = kernel_kind(robust_kernel)
        self._drop()
        self._kind.append(kind)
        self._delta.append(float(robust_delta))
        self._ij.append((int(v1), int(v2)))
        self._meas.append(mat_to_pose7(z) if z.shape == (4, 4) else z.reshape(7).copy())
        self._info.append(np.asarray(information_matrix, np.float64).reshape(6, 6).copy())
        return len(self._ij) - 1

    def add_se3_prior_xyz_edge(self, v, xyz, information3, robust_kernel=None, robust_delta=1.0):
        """hdl_graph_slam's add_se3_prior_xyz_edge (not in the reference, whose keyframes only carry the utm_coord field): a
        position fix `xyz` in the graph frame on vertex `v` with a 3x3 information matrix.  Returns the prior's index."""
        info = np.zeros((6, 6))
        info[:3, :3] = np.asarray(information3, np.float64).reshape(3, 3)
        meas = np.array([*np.asarray(xyz, np.float64).reshape(3), 0.0, 0.0, 0.0, 1.0])
        return self._add_prior(v, PRIOR_XYZ, meas, info, robust_kernel, robust_delta)

    def add_se3_prior_pose_edge(self, v, pose, information6, robust_kernel=None, robust_delta=1.0):
        """An absolute pose (4x4 or 7-vector) on vertex `v` with a 6x6 information matrix over [translation, rotation]; it
        may be positive semi-definite only (a zero translation block: an orientation prior)."""
        z = np.asarray(pose, np.float64)
        meas = mat_to_pose7(z) if z.shape == (4, 4) else z.reshape(7).copy()
        return self._add_prior(v, PRIOR_POSE, meas, np.asarray(information6, np.float64).reshape(6, 6).copy(), robust_kernel,
                               robust_delta)

    def _add_prior(self, v, type_, meas, info, robust_kernel, robust_delta):
        kind = kernel_kind(robust_kernel)
        self._drop()
        self._priors.append(dict(vertex=int(v), type=int(type_), meas=meas, info=info, kind=kind, delta=float(robust_delta)))
        return len(self._priors) - 1

    def add_se3_prior_plane_edge(self, v, measured_plane4, info3, world_plane4=(0.0, 0.0, 1.0, 0.0), robust_kernel=None,
                                 robust_delta=1.0):
        """hdl_graph_slam's floor constraint (not in the reference, which only shows the intent): the plane `world_plane4`
        = (n, d) of the graph frame was measured as `measured_plane4` in the sensor frame of vertex `v`; `info3` is the 3x3
        information over (tangent 1, tangent 2, distance) -- include/lslam_c.h, "plane priors".  Returns the plane prior's index."""
        kind = kernel_kind(robust_kernel)
        self._drop()
        self._plane_priors.append(dict(vertex=int(v), world=np.asarray(world_plane4, np.float64).reshape(4).copy(),
                                       meas=np.asarray(measured_plane4, np.float64).reshape(4).copy(),
                                       info=np.asarray(info3, np.float64).reshape(3, 3).copy(), kind=kind, delta=float(robust_delta)))
        return len(self._plane_priors) - 1

    @property
    def num_plane_priors(self):
        return int(self.lib.lslam_pg_num_plane_priors(self.h)) if self.h else len(self._plane_priors)

    @staticmethod
    def _plane_prior_list(priors):
        """dict(vertex (n), world (n, 4), meas (n, 4), info (n, 3, 3)[, kernels (n), deltas (n or scalar)]) or None -> list"""
        if priors is None:
            return []
        vertex = np.asarray(priors["vertex"]).reshape(-1)
        n = len(vertex)
        world = np.asarray(priors["world"], np.float64).reshape(n, 4)
        meas = np.asarray(priors["meas"], np.float64).reshape(n, 4)
        info = np.asarray(priors["info"], np.float64).reshape(n, 3, 3)
        kind, delta = PoseGraph._kernel_lists(priors.get("kernels"), priors.get("deltas"), n)
        return [dict(vertex=int(vertex[p]), world=world[p].copy(), meas=meas[p].copy(), info=info[p].copy(), kind=kind[p],
                     delta=float(delta[p])) for p in range(n)]

    def set_plane_priors(self, priors):
        """Replace the whole set of plane priors (lslam_pg_set_plane_priors); None or an empty set clears.  Checked by the
        library: on an error nothing changes."""
        new = self._plane_prior_list(priors)
        if self.h:
            self._upload_plane_priors(new)
        self._plane_priors = new

    def plane_prior_robust(self, poses=None):
        """Per plane prior at `poses` ((n, 7); None: the current estimate): dict(e2, rho = rho0, weight = rho1)."""
        self._build()
        n = len(self._plane_priors)
        e2, rho, w = np.zeros(n), np.zeros(n), np.zeros(n)
        p = None
        if poses is not None:
            p = np.ascontiguousarray(poses, np.float64)
            if p.shape != (len(self._nodes), 7):
                raise ValueError("poses must be (%d, 7)" % len(self._nodes))
        self._check(self.lib.lslam_pg_plane_prior_robust(self.h, _dp(p) if p is not None else None, _dp(e2), _dp(rho), _dp(w)))
        return dict(e2=e2, rho=rho, weight=w)

    def _upload_plane_priors(self, priors):
        n = len(priors)
        if n == 0:
            self._check(self.lib.lslam_pg_set_plane_priors(self.h, 0, None, None, None, None, None, None))
            return
        v = np.ascontiguousarray([q["vertex"] for q in priors], np.int32)
        a = np.ascontiguousarray(np.stack([q["world"] for q in priors]), np.float64)
        m = np.ascontiguousarray(np.stack([q["meas"] for q in priors]), np.float64)
        w = np.ascontiguousarray(np.stack([q["info"] for q in priors]), np.float64)
        k = np.ascontiguousarray([q["kind"] for q in priors], np.int32)
        d = np.ascontiguousarray([q["delta"] for q in priors], np.float64)
        robust = bool((k != KERNEL_NONE).any())
        self._check(self.lib.lslam_pg_set_plane_priors(self.h, n, v.ctypes.data_as(c_int32_p), _dp(a), _dp(m), _dp(w),
                                                       k.ctypes.data_as(c_int32_p) if robust else None, _dp(d) if robust else None))

    @property
    def num_priors(self):
        return int(self.lib.lslam_pg_num_priors(self.h)) if self.h else len(self._priors)

    @staticmethod
    def _prior_list(priors):
        """dict(vertex (n), type (n), meas (n, 7), info (n, 6, 6)[, kernels (n), deltas (n or scalar)]) or None -> list"""
        if priors is None:
            return []
        vertex = np.asarray(priors["vertex"]).reshape(-1)
        n = len(vertex)
        type_ = np.asarray(priors["type"]).reshape(-1)
        meas = np.asarray(priors["meas"], np.float64).reshape(n, 7)
        info = np.asarray(priors["info"], np.float64).reshape(n, 6, 6)
        kind, delta = PoseGraph._kernel_lists(priors.get("kernels"), priors.get("deltas"), n)
        if len(type_) != n:
            raise ValueError("%d prior types for %d priors" % (len(type_), n))
        return [dict(vertex=int(vertex[p]), type=int(type_[p]), meas=meas[p].copy(), info=info[p].copy(), kind=kind[p],
                     delta=float(delta[p])) for p in range(n)]

    def set_priors(self, priors):
        """Replace the whole set of unary constraints (lslam_pg_set_priors); None or an empty set clears.  `priors`: the dict
        of set_graph.  Checked by the library: on an error nothing changes."""
        new = self._prior_list(priors)
        if self.h:
            self._upload_priors(new)
        self._priors = new

    def prior_robust(self, poses=None):
        """Per prior at `poses` ((n, 7); None: the current estimate): dict(e2 = e^T Omega e, rho = rho0, weight = rho1)."""
        self._build()
        n = len(self._priors)
        e2, rho, w = np.zeros(n), np.zeros(n), np.zeros(n)
        p = None
        if poses is not None:
            p = np.ascontiguousarray(poses, np.float64)
            if p.shape != (len(self._nodes), 7):
                raise ValueError("poses must be (%d, 7)" % len(self._nodes))
        self._check(self.lib.lslam_pg_prior_robust(self.h, _dp(p) if p is not None else None, _dp(e2), _dp(rho), _dp(w)))
        return dict(e2=e2, rho=rho, weight=w)

    def _upload_priors(self, priors):
        n = len(priors)
        if n == 0:
            self._check(self.lib.lslam_pg_set_priors(self.h, 0, None, None, None, None, None, None))
            return
        v = np.ascontiguousarray([q["vertex"] for q in priors], np.int32)
        t = np.ascontiguousarray([q["type"] for q in priors], np.int32)
        m = np.ascontiguousarray(np.stack([q["meas"] for q in priors]), np.float64)
        w = np.ascontiguousarray(np.stack([q["info"] for q in priors]), np.float64)
        k = np.ascontiguousarray([q["kind"] for q in priors], np.int32)
        d = np.ascontiguousarray([q["delta"] for q in priors], np.float64)
        robust = bool((k != KERNEL_NONE).any())
        self._check(self.lib.lslam_pg_set_priors(self.h, n, v.ctypes.data_as(c_int32_p), t.ctypes.data_as(c_int32_p), _dp(m), _dp(w),
                                                 k.ctypes.data_as(c_int32_p) if robust else None, _dp(d) if robust else None))

    def optimize(self, max_iterations=1000):
        """solver_g2o.cpp:79-95: graph->optimize(1000).  Returns the iteration count."""
        self._build()
        st = LslamPgStats()
        self._check(self.lib.lslam_pg_optimize(self.h, int(max_iterations), C.byref(st)))
        self.last_stats = st
        return st.iterations

    # ---- bulk construction / access ---------------------------------------------------
    def set_graph(self, poses7, ij, meas7, info, fixed=0, kernels=None, deltas=None, priors=None, plane_priors=None):
        """Replace the graph; `fixed` is the vertex held at its estimate (default: the first, as add_se3_node; -1: none, for
        graphs whose priors fix the gauge).  `kernels` / `deltas`: per edge, as set_robust_kernels (None: plain edges).
        `priors`: None or dict(vertex (n), type (n) of PRIOR_XYZ / PRIOR_POSE, meas (n, 7), info (n, 6, 6)[, kernels, deltas]).
        `plane_priors`: None or dict(vertex (n), world (n, 4), meas (n, 4), info (n, 3, 3)[, kernels, deltas])."""
        new_priors = self._prior_list(priors)
        new_planes = self._plane_prior_list(plane_priors)
        kind, delta = self._kernel_lists(kernels, deltas, len(np.asarray(ij).reshape(-1, 2)))  # raises before anything is dropped
        if int(fixed) >= len(np.asarray(poses7).reshape(-1, 7)):
            raise ValueError("fixed vertex %d of a graph with %d vertices" % (int(fixed), len(np.asarray(poses7).reshape(-1, 7))))
        self._drop(keep_estimates=False)
        self._kind, self._delta = kind, delta
        self._priors = new_priors
        self._plane_priors = new_planes
        self._nodes = [p for p in np.asarray(poses7, np.float64).reshape(-1, 7)]
        self._ij = [tuple(int(v) for v in e) for e in np.asarray(ij).reshape(-1, 2)]
        self._meas = [m for m in np.asarray(meas7, np.float64).reshape(-1, 7)]
        self._info = [w for w in np.asarray(info, np.float64).reshape(-1, 6, 6)]
        self.fixed = int(fixed)
        if self.fixed >= len(self._nodes):
            raise ValueError("fixed vertex %d of a graph with %d vertices" % (self.fixed, len(self._nodes)))
        self._drop()

    # ---- robust kernels on edges (lslam_pg_set_robust_kernels) ------------------------------
    @staticmethod
    def _kernel_lists(kinds, deltas, ne):
        if kinds is None:
            return [KERNEL_NONE] * ne, [1.0] * ne
        kinds = [kernel_kind(k) for k in (kinds.tolist() if isinstance(kinds, np.ndarray) else kinds)]
        deltas = np.broadcast_to(np.asarray(1.0 if deltas is None else deltas, np.float64), (ne,)).tolist()
        if len(kinds) != ne:
            raise ValueError("%d kernels for %d edges" % (len(kinds), ne))
        return kinds, deltas

    def set_robust_kernels(self, kinds, deltas):
        """One kernel per edge: `kinds` names or LSLAM_PG_KERNEL_* integers, `deltas` a scalar or one per edge (ignored where
        the kind is NONE).  Checked by the library: on an error (delta not finite and > 0, unknown kind) nothing changes."""
        kinds, deltas = self._kernel_lists(kinds, deltas, len(self._ij))
        if self.h:
            self._upload_kernels(kinds, deltas)
        self._kind, self._delta = kinds, deltas

    def clear_robust_kernels(self):
        """The plain solver again."""
        if self.h:
            self._check(self.lib.lslam_pg_set_robust_kernels(self.h, None, None))
        self._kind, self._delta = self._kernel_lists(None, None, len(self._ij))

    def edge_robust(self, poses=None):
        """Per edge at `poses` ((n, 7); None: the current estimate): dict(e2 = e^T Omega e, rho = rho0, weight = rho1)."""
        self._build()
        ne = len(self._ij)
        e2, rho, w = np.zeros(ne), np.zeros(ne), np.zeros(ne)
        p = None
        if poses is not None:
            p = np.ascontiguousarray(poses, np.float64)
            if p.shape != (len(self._nodes), 7):
                raise ValueError("poses must be (%d, 7)" % len(self._nodes))
        self._check(self.lib.lslam_pg_edge_robust(self.h, _dp(p) if p is not None else None, _dp(e2), _dp(rho), _dp(w)))
        return dict(e2=e2, rho=rho, weight=w)

    def robust_info(self):
        """dict(n_robust: edges carrying a kernel, n_downweighted: of those, edges with weight < 1 at the current estimate,
        chi2_plain: the plain sum of e^T Omega e)."""
        self._build()
        nr, nd, c2 = C.c_int32(), C.c_int32(), C.c_double()
        self._check(self.lib.lslam_pg_robust_info(self.h, C.byref(nr), C.byref(nd), C.byref(c2)))
        return dict(n_robust=nr.value, n_downweighted=nd.value, chi2_plain=c2.value)

    def _upload_kernels(self, kinds, deltas):
        k = np.ascontiguousarray(kinds, np.int32)
        d = np.ascontiguousarray(deltas, np.float64)
        self._check(self.lib.lslam_pg_set_robust_kernels(self.h, k.ctypes.data_as(c_int32_p), _dp(d)))

    # ---- g2o text format (solver_g2o.cpp:97-100) -----------------------------------------
    def save(self, path):
        """SolverG2O::save: the graph with its current estimates as a .g2o file, priors included (EDGE_SE3_PRIOR /
        EDGE_SE3_PRIORXYZ lines, and this project's own EDGE_SE3_PRIOR_PLANE lines for plane priors).  The format has no place for a robust kernel: none is written, and a graph loaded back has
        plain edges and priors."""
        self._build()
        self._check(self.lib.lslam_pg_save_g2o(self.h, str(path).encode()))

    @staticmethod
    def read_g2o(path, lib=None):
        """-> dict(poses (n,7), ij (m,2), meas (m,7), info (m,6,6), fixed, priors) from a .g2o file (host only); `priors` is
        the dict set_graph takes (vertex, type, meas, info), empty arrays for a file without any."""
        from .capi import load_library
        lib = lib or load_library()
        nv, ne, fx = C.c_int32(0), C.c_int32(0), C.c_int32(-1)
        rc = lib.lslam_g2o_read(str(path).encode(), C.byref(nv), None, C.byref(ne), None, None, None, C.byref(fx))
        if rc < 0:
            raise LslamError(rc, lib.lslam_pg_last_error().decode())
        poses = np.zeros((nv.value, 7))
        ij = np.zeros((ne.value, 2), np.int32)
        meas = np.zeros((ne.value, 7))
        info = np.zeros((ne.value, 6, 6))
        rc = lib.lslam_g2o_read(str(path).encode(), C.byref(nv), _dp(poses), C.byref(ne),
                                ij.ctypes.data_as(c_int32_p), _dp(meas), _dp(info), C.byref(fx))
        if rc < 0:
            raise LslamError(rc, lib.lslam_pg_last_error().decode())
        npr = C.c_int32(0)
        rc = lib.lslam_g2o_read_priors(str(path).encode(), C.byref(npr), None, None, None, None)
        if rc < 0:
            raise LslamError(rc, lib.lslam_pg_last_error().decode())
        pv, pt = np.zeros(npr.value, np.int32), np.zeros(npr.value, np.int32)
        pm, pw = np.zeros((npr.value, 7)), np.zeros((npr.value, 6, 6))
        rc = lib.lslam_g2o_read_priors(str(path).encode(), C.byref(npr), pv.ctypes.data_as(c_int32_p), pt.ctypes.data_as(c_int32_p),
                                       _dp(pm), _dp(pw))
        if rc < 0:
            raise LslamError(rc, lib.lslam_pg_last_error().decode())
        nq = C.c_int32(0)
        rc = lib.lslam_g2o_read_plane_priors(str(path).encode(), C.byref(nq), None, None, None, None)
        if rc < 0:
            raise LslamError(rc, lib.lslam_pg_last_error().decode())
        qv, qa, qm, qw = np.zeros(nq.value, np.int32), np.zeros((nq.value, 4)), np.zeros((nq.value, 4)), np.zeros((nq.value, 3, 3))
        rc = lib.lslam_g2o_read_plane_priors(str(path).encode(), C.byref(nq), qv.ctypes.data_as(c_int32_p), _dp(qa), _dp(qm), _dp(qw))
        if rc < 0:
            raise LslamError(rc, lib.lslam_pg_last_error().decode())
        return dict(poses=poses, ij=ij, meas=meas, info=info, fixed=fx.value, priors=dict(vertex=pv, type=pt, meas=pm, info=pw),
                    plane_priors=dict(vertex=qv, world=qa, meas=qm, info=qw))

    def load(self, path):
        """Replace the graph by the one in a .g2o file, its priors included; the file's FIX vertex stays the fixed one.  A
        file without FIX: the first vertex, as add_se3_node -- unless the file holds priors, which then fix the gauge (-1)."""
        g = PoseGraph.read_g2o(path, self.lib)
        has_priors = len(g["priors"]["vertex"]) > 0
        has_planes = len(g["plane_priors"]["vertex"]) > 0
        self.set_graph(g["poses"], g["ij"], g["meas"], g["info"], fixed=g["fixed"] if g["fixed"] >= 0 or has_priors else 0,
                       priors=g["priors"] if has_priors else None, plane_priors=g["plane_priors"] if has_planes else None)
        return g

    def poses(self):
        self._build()
        out = np.zeros((len(self._nodes), 7))
        self._check(self.lib.lslam_pg_get_poses(self.h, _dp(out)))
        return out

    def estimate(self, v):
        return pose7_to_mat(self.poses()[v])

    def set_estimates(self, poses, fixed=None):
        """Replace every vertex's estimate (n 7-vectors or n 4x4 matrices) and, with `fixed`, the vertex held fixed (-1:
        none); edges, kernels and priors stay.  The device graph is rebuilt by the next call that needs it."""
        poses = [np.asarray(p, np.float64) for p in poses]
        if len(poses) != len(self._nodes):
            raise ValueError("%d estimates for %d vertices" % (len(poses), len(self._nodes)))
        if fixed is not None and int(fixed) >= len(self._nodes):
            raise ValueError("fixed vertex %d of a graph with %d vertices" % (int(fixed), len(self._nodes)))
        self._drop(keep_estimates=False)
        self._nodes = [mat_to_pose7(p) if p.shape == (4, 4) else p.reshape(7).copy() for p in poses]
        if fixed is not None:
            self.fixed = int(fixed)

    # ---- multi-GPU ------------------------------------------------------------------------
    def set_shard(self, e_begin, e_end, allreduce=None, system_tensor=None):
        """This rank linearises edges [e_begin, e_end); `allreduce(ptr, count)` must sum the
        `count` doubles at device address `ptr` over all ranks in place (e.g. a
        torch.distributed.all_reduce on `system_tensor`, whose storage the library then
        assembles into)."""
        self._build()
        if allreduce is None:
            self._cb = ALLREDUCE_FN(0)
        else:
            def _tramp(_user, ptr, count):
                allreduce(ptr, count)
            self._cb = ALLREDUCE_FN(_tramp)
        buf = C.c_void_p(system_tensor.data_ptr()) if system_tensor is not None else None
        self._check(self.lib.lslam_pg_set_shard(self.h, int(e_begin), int(e_end), self._cb, None, buf))
        self._sys_tensor = system_tensor

    def set_comm(self, comm, e_begin, e_end):
        """Edge shard [e_begin, e_end) of this rank, the block system all-reduced by the library's own
        RCCL communicator (lslam_pg_set_comm) on the solver's stream."""
        self._build()
        self._cb = ALLREDUCE_FN(0)
        self._check(self.lib.lslam_pg_set_shard(self.h, int(e_begin), int(e_end), self._cb, None, None))
        self._check(self.lib.lslam_pg_set_comm(self.h, comm.h if comm is not None else None))
        self._comm = comm

    def row_shard_range(self, rank, world):
        """lslam_pg_row_shard_range: this rank's vertex rows [v_begin, v_end) of an even partition in whole row blocks."""
        b, e = C.c_int32(), C.c_int32()
        self.lib.lslam_pg_row_shard_range(len(self._nodes), int(rank), int(world), C.byref(b), C.byref(e))
        return b.value, e.value

    def set_row_shard(self, v_begin, v_end):
        """lslam_pg_set_row_shard: the damped solves are shared by the ranks (row-sharded block-Jacobi PCG) instead of replicated;
        (-1, -1) switches back.  Needs set_shard / set_comm first (the transport)."""
        self._build()
        self._check(self.lib.lslam_pg_set_row_shard(self.h, int(v_begin), int(v_end)))

    def set_solve_tolerance(self, rel_tol):
        """lslam_pg_set_solve_tolerance: relative residual at which a damped solve's PCG stops (default 1e-8 = the direct
        solver's answer as far as LM can tell; looser = inexact LM, same optimum, another trajectory)."""
        self._build()
        self._check(self.lib.lslam_pg_set_solve_tolerance(self.h, float(rel_tol)))

    def row_sharded_solves(self):
        return int(self.lib.lslam_pg_row_sharded_solves(self.h)) if self.h else 0

    def set_row_gather(self, allgatherv, rank, world):
        """lslam_pg_set_row_gather: `allgatherv(ptr, offsets, world)` gathers in place -- doubles [offsets[r], offsets[r + 1])
        at device address `ptr` are valid on rank r on entry, on every rank on return.  None removes it.  (With the library's
        RCCL communicator nothing needs registering: the gather is taken by itself.)"""
        self._build()
        if allgatherv is None:
            self._gcb = ALLGATHERV_FN(0)
        else:
            def _tramp(_user, ptr, offs, w):
                allgatherv(ptr, [int(offs[i]) for i in range(w + 1)], int(w))
            self._gcb = ALLGATHERV_FN(_tramp)
        self._check(self.lib.lslam_pg_set_row_gather(self.h, self._gcb, None, int(rank), int(world)))

    def row_gathered_solves(self):
        return int(self.lib.lslam_pg_row_gathered_solves(self.h)) if self.h else 0

    def system_doubles(self):
        self._build()
        return self.lib.lslam_pg_system_doubles(self.h)

    # ---- parity taps --------------------------------------------------------------------------
    def linearize(self):
        self._build()
        n, no = len(self._nodes), self.lib.lslam_pg_num_offdiag(self.h)
        diag = np.zeros((n, 6, 6))
        off = np.zeros((no, 6, 6))
        oij = np.zeros((no, 2), np.int32)
        b = np.zeros(6 * n)
        chi = np.zeros(1)
        self._check(self.lib.lslam_pg_linearize(self.h, _dp(diag), _dp(off), oij.ctypes.data_as(c_int32_p),
                                                _dp(b), _dp(chi)))
        return dict(diag=diag, off=off, off_ij=oij, b=b, chi2=float(chi[0]))

    def solve(self, lam):
        self._build()
        dx = np.zeros(6 * len(self._nodes))
        it = C.c_int32()
        self._check(self.lib.lslam_pg_solve(self.h, float(lam), _dp(dx), C.byref(it)))
        return dx, it.value

    # ---- marginal covariances (lslam_pg_marginals, lslam_pg_relative_covariances) ------------------
    @staticmethod
    def _marginal_opts(rel_tol=0.0, max_iters=0, coarse=-1):
        return LslamPgMarginalOpts(float(rel_tol), int(max_iters), int(coarse))

    @staticmethod
    def _vertex_list(vertices):
        v = np.ascontiguousarray(np.asarray(vertices).reshape(-1), np.int32)
        return v, (v.ctypes.data_as(c_int32_p) if len(v) else None)

    def marginals(self, vertices, cross=False, **opts):
        """Covariance blocks of `vertices` at the current estimate, g2o's computeMarginals: (n, 6, 6), and with `cross` also the
        (n, n, 6, 6) cross blocks.  Coordinates are the solver's increments (body-frame translation [m], then the quaternion
        vector = half the angle); the fixed vertex has exact zeros.  `opts`: rel_tol, max_iters, coarse
        (lslam_pg_marginal_opts).  Raises LslamError for a vertex without a gauge, a column that does not converge, a sharded
        graph; nothing is returned then.  The call's statistics are in ``marginal_stats``."""
        self._build()
        v, vp = self._vertex_list(vertices)
        n = len(v)
        cov = np.zeros((n, 6, 6))
        crs = np.zeros((n, n, 6, 6)) if cross else None
        o, st = self._marginal_opts(**opts), LslamPgMarginalStats()
        self._check(self.lib.lslam_pg_marginals(self.h, n, vp, C.byref(o), _dp(cov) if n else None,
                                                _dp(crs) if cross and n else None, C.byref(st)))
        self.marginal_stats = st
        return (cov, crs) if cross else cov

    def relative_covariances(self, ref, vertices, **opts):
        """Covariance (n, 6, 6) of the relative poses X_ref^-1 X_j, j in `vertices`, in the coordinates of an edge error (ref's
        frame); j == ref gives exact zeros.  `opts` and errors as ``marginals``."""
        self._build()
        v, vp = self._vertex_list(vertices)
        n = len(v)
        cov = np.zeros((n, 6, 6))
        o, st = self._marginal_opts(**opts), LslamPgMarginalStats()
        self._check(self.lib.lslam_pg_relative_covariances(self.h, int(ref), n, vp, C.byref(o), _dp(cov) if n else None, C.byref(st)))
        self.marginal_stats = st
        return cov

    def debug_marginal_columns(self, vertex, **opts):
        """Test tap (lslam_debug_pg_marginal_columns): the six solved columns of H^-1 of one free vertex, (6 n, 6), raw."""
        self._build()
        x = np.zeros((6 * len(self._nodes), 6))
        o, st = self._marginal_opts(**opts), LslamPgMarginalStats()
        self._check(self.lib.lslam_debug_pg_marginal_columns(self.h, int(vertex), C.byref(o), _dp(x), C.byref(st)))
        self.marginal_stats = st
        return x

    # ---- internals ---------------------------------------------------------------------------------
    def _check(self, rc):
        if rc < 0:
            raise LslamError(rc, self.lib.lslam_pg_last_error().decode())
        return rc

    def build(self):
        """Upload the graph and build the device-side structures now (otherwise the first
        optimize()/linearize() does it); the counterpart of g2o's initializeOptimization()."""
        self._build()

    def _drop(self, keep_estimates=True):
        """Release the device graph.  The optimised estimates are pulled back first (g2o keeps its
        vertices' estimates when vertices or edges are added after an optimize())."""
        if self.h:
            if keep_estimates and len(self._nodes):
                out = np.zeros((len(self._nodes), 7))
                if self.lib.lslam_pg_get_poses(self.h, _dp(out)) == 0:
                    self._nodes = [p for p in out]
            self.lib.lslam_pg_destroy(self.h)
            self.h = None

    def _build(self):
        if self.h:
            return
        poses = np.ascontiguousarray(np.stack(self._nodes), np.float64)
        ne = len(self._ij)
        ij = np.ascontiguousarray(np.array(self._ij, np.int32).reshape(ne, 2))
        meas = np.ascontiguousarray(np.stack(self._meas) if ne else np.zeros((0, 7)), np.float64)
        info = np.ascontiguousarray(np.stack(self._info) if ne else np.zeros((0, 6, 6)), np.float64)
        h = C.c_void_p()
        rc = self.lib.lslam_pg_create(self.device, len(poses), _dp(poses), ne, ij.ctypes.data_as(c_int32_p),
                                      _dp(meas), _dp(info), self.fixed, C.byref(h))
        if rc != 0:
            raise LslamError(rc, self.lib.lslam_pg_last_error().decode())
        self.h = h
        try:
            if any(k != KERNEL_NONE for k in self._kind):
                self._upload_kernels(self._kind, self._delta)
            if self._priors:
                self._upload_priors(self._priors)
            if self._plane_priors:
                self._upload_plane_priors(self._plane_priors)
        except Exception:
            self._drop(keep_estimates=False)
            raise

    def close(self):
        self._drop(keep_estimates=False)

    def __del__(self):
        try:
            self._drop()
        except Exception:
            pass
