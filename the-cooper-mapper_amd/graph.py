"""Host-side mirror of the pose-graph node's bookkeeping, ``pose_graph::Graph`` +
``KeyframeUpdater`` (/root/reference/L_SLAM/src/pose_graph/graph.cpp:230-385,
keyframe_updater.hpp:10-60): keyframe selection, odometry edges with the reference's information
matrices, loop detection, optimisation and the odom -> graph correction.  The
ROS plumbing (topics, threads, tf) is not mirrored; the arithmetic runs on the device through
:class:`PoseGraph` (LM) and :class:`LoopDetector` (scanMatchLocal).
"""
import numpy as np

from .loop_closure import KeyFrame, LoopDetector
from .pose_graph import PoseGraph, kernel_kind


def _angle_of(R):
    """Eigen::AngleAxisd(R).angle() in [0, pi]."""
    c = (np.trace(R) - 1.0) / 2.0
    return float(np.arccos(min(1.0, max(-1.0, c))))


class KeyframeUpdater:
    """keyframe_updater.hpp:10-60."""

    def __init__(self):
        self.is_first = True
        self.prev_keypose = np.eye(4)
        self.keyframe_delta_trans = 0.25
        self.keyframe_delta_angle = 0.05
        self.accum_distance = 0.0
        self.frame_count = 0
        self.frame_id = 0

    def update(self, pose):
        pose = np.asarray(pose, np.float64).reshape(4, 4)
        if self.is_first:
            self.is_first = False
            self.prev_keypose = pose.copy()
            return True
        delta = np.linalg.inv(self.prev_keypose) @ pose
        dx = float(np.linalg.norm(delta[:3, 3]))
        da = _angle_of(delta[:3, :3])
        if dx < self.keyframe_delta_trans and da < self.keyframe_delta_angle:
            return False
        self.accum_distance += dx
        self.prev_keypose = pose.copy()
        self.frame_count += 1
        return True

    def get_accum_distance(self):
        return self.accum_distance

    def get_unique_id(self):
        self.frame_id += 1
        return self.frame_id


# graph.cpp:279-288 and :333-339
ODOMETRY_INFORMATION = np.diag([0.8, 0.4, 0.8, 1.0, 2.0, 1.0])
LOOP_INFORMATION = 2.0 * np.eye(6)
# ScanMatch.cpp:142: the reference's floor for a usable match; below it an edge keeps the reference's constant
EDGE_INFORMATION_MIN_ROWS = 50
# scanMatchLocal's leaves (ScanMatch.cpp:29-30): reference corner / surf, new corner / surf
EDGE_INFORMATION_LEAVES = (0.2, 0.4, 0.2, 0.4)


def hessian_information(omega_ref, H, sum_b2, n_rows, range_sigma):
    """The information of an edge from its match Hessian (``lslam_edge_info``; DESIGN, pose-graph section):
    ``omega_ref + H / max(sum_b2 / (n_rows - 6), range_sigma^2)``, and ``omega_ref`` alone below 50 rows.  ``omega_ref`` --
    the reference's constant for the edge type -- acts as a weak prior: the result is positive definite whatever the match
    saw, and a direction the match did not observe keeps exactly the reference's weight."""
    omega_ref = np.asarray(omega_ref, np.float64)
    H = np.asarray(H, np.float64).reshape(6, 6)
    # (a scan point exactly on its line gives the reference's coefficient a 0 / 0, ScanMatch.cpp:160-170: such sums say nothing)
    if n_rows < EDGE_INFORMATION_MIN_ROWS or not (np.isfinite(H).all() and np.isfinite(sum_b2)):
        return omega_ref.copy()
    s2 = max(float(sum_b2) / float(n_rows - 6), float(range_sigma) * float(range_sigma))
    return omega_ref + H / s2


def rigid_fit(source, target):
    """The rigid transform (4x4) that moves `source` onto `target` in the least-squares sense (Kabsch / Umeyama without
    scale): the library's host fit ``lslam_debug_icp_fit`` on the 18 sums ``n | 0 | sum s | sum t | sum s t^T | 0`` -- no
    device needed."""
    from .scan_match import icp_fit
    s, t = np.asarray(source, np.float64).reshape(-1, 3), np.asarray(target, np.float64).reshape(-1, 3)
    fit = icp_fit(np.r_[float(len(s)), 0.0, s.sum(0), t.sum(0), (s.T @ t).reshape(-1), 0.0])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = fit["R"], fit["t"]
    return T


class Graph:
    def __init__(self, device=0, ctx=None, loop_detector=None, max_keyframes_per_update=10, resident=False,
                 keep_host_clouds=True, store_max_points=0, store_max_keyframes=0, store_slab_points=0, appearance_loops=False,
                 sc_params=None, loop_robust_kernel=None, loop_robust_delta=1.0, edge_information=None, range_sigma=None,
                 gps_sigma=None, gps_robust_kernel=None, gps_robust_delta=1.0, gps_min_spread=None, imu_orientation_sigma=None,
                 floor_sigma=None, floor_params=None, floor_robust_kernel=None, floor_robust_delta=1.0,
                 floor_world_plane=(0.0, 0.0, 1.0, 0.0), odometry_information=None, remove_dynamic=False, dynamic_params=None,
                 occupancy=None, loop_search=None, loop_gate_prob=0.99, loop_max_candidates=32, loop_consistency_prob=None,
                 covariance_opts=None):
        """``resident=True``: the keyframes' clouds live in a :class:`KeyframeStore` on the loop detector's context --
        ``add_frame`` uploads them once (``kf.store_id``), loop closure and ``get_final_feature_map`` read them there;
        ``keep_host_clouds=False`` then drops the host copies (``kf.corner_cloud`` / ``kf.surf_cloud`` fetch on demand).
        The ``store_*`` limits are :class:`KeyframeStore`'s (0: its defaults).  Without ``resident`` nothing changes.
        ``appearance_loops=True`` (not in the reference; implies ``resident``): ``optimize`` also runs
        ``LoopDetector.detect_appearance`` -- scan-context candidates over the store, ``sc_params`` being
        ``KeyframeStore.sc_setup``'s keywords -- for the new keyframes for which ``detect_nearest`` found no loop.
        ``loop_robust_kernel`` (not in the reference, which includes g2o's robust-kernel headers and uses none): "Huber",
        "Cauchy" or "DCS" with parameter ``loop_robust_delta`` on every LOOP edge, whichever detector found it; odometry edges
        never carry one.  A false loop -- two places that look alike -- then loses its weight instead of bending the map:
        :meth:`loop_weights`, :meth:`rejected_loops`.  The default stays None (every edge at full weight, the reference's
        behaviour); switching a kernel on is the caller's decision.  Huber is convex and CANNOT reject an outlier, it only
        bounds its pull: on graphs with this node's weak odometry information the trajectory still bends to meet a false loop
        (DESIGN, pose-graph section); Cauchy (0.1) and DCS (1) do reject.
        ``edge_information="hessian"`` (not in the reference, whose InformationEstimator returns the identity; needs
        ``resident=True`` and ``range_sigma``): every edge's information is the reference's constant plus the fp64 match Hessian
        of the two keyframes at the edge's measurement (``lslam_keyframe_edge_information``) over the residual variance, floored at
        ``range_sigma``^2 -- :func:`hessian_information`.  ``range_sigma`` [m] is the range noise of the caller's sensor and
        has no default: the library does not guess it.  None (the default) changes nothing.
        ``gps_sigma=(sigma_xy, sigma_z)`` [m] (not in the reference, whose keyframes only carry the ``utm_coord`` / ``imu_quat``
        fields, keyframe.h:40-41): the fixes handed to ``add_frame(utm_coord=...)`` become XYZ priors with information
        ``diag(1/sxy^2, 1/sxy^2, 1/sz^2)`` (``lslam_pg_set_priors``), with ``gps_robust_kernel`` / ``gps_robust_delta`` on each
        (GPS multipath: "Cauchy" rejects an outlying fix; :meth:`gps_weights`, :meth:`rejected_fixes`).  Like ``range_sigma`` it
        has no default: the library does not guess a receiver's noise.  ``utm_origin`` is the first keyframe fix, kept in fp64
        on the host and subtracted before anything reaches the solver (UTM coordinates are ~1e6 m).  GAUGE: the graph frame
        starts as the first lidar pose, not ENU, and priors under a fixed, misaligned first vertex would bend the map -- so
        until the fixes span a plane (second singular value of the centred fix positions >= ``gps_min_spread``, default
        ``10 * sigma_xy``: the heading is then observable well above the noise) the priors are queued and the first vertex
        stays fixed, the reference's behaviour; once they do, the keyframe estimates and ``tf_odom2graph`` are moved by the
        rigid fit of estimate positions to fixes (:func:`rigid_fit`), all queued priors are added and the solver is
        rebuilt with no fixed vertex.  ``imu_orientation_sigma`` [rad]: ``add_frame(imu_quat=...)`` (x, y, z, w, in the frame
        the fixes are in) becomes a POSE prior with a zero translation block and ``(2 / sigma)^2`` on the quaternion vector
        (half the angle); queued with the fixes when ``gps_sigma`` is set.  ``optimize`` then runs the solver when a pass
        added loops OR priors.  All of it is off by default.
        ``floor_sigma=(sigma_normal [rad], sigma_distance [m])`` (not in the reference, which only shows the intent:
        solver_g2o.h:61-65, :92, graph.cpp:321 "floor coeffs"): on each pass the floor of every new keyframe's surface cloud is
        detected on the device -- one ``lslam_floor_detect_keyframes`` call over the store with ``resident=True``, one
        ``lslam_floor_detect`` per cloud on ``ctx`` otherwise -- with ``floor_params`` (:func:`floor.floor_params`' keywords;
        None: the defaults).  An accepted floor (status OK) is stored as ``kf.floor_coeffs`` (n, d in the sensor frame) and
        becomes a plane prior (``lslam_pg_set_plane_priors``) against ``floor_world_plane`` -- the floor in the GRAPH frame,
        z = 0 by default: a graph frame that starts at the first sensor pose has its floor at (0, 0, 1, sensor_height) -- with
        information ``diag(1/sn^2, 1/sn^2, 1/sd^2)`` and ``floor_robust_kernel`` / ``floor_robust_delta`` (a kerb or a ramp
        taken for the floor: "Cauchy" rejects it; :meth:`floor_weights`, :meth:`rejected_floors`).  A keyframe whose floor was
        not found adds nothing and is counted (``floors_not_found``).  Like the other sigmas it has no default.
        LIMIT of ``floor_robust_kernel`` (and of every kernel here): with the reference's constant odometry information
        (sigma about 1 m / 0.7 rad) bending the trajectory onto an outlying floor costs less than ANY kernel charges for
        rejecting it, so no kernel rejects in the default configuration; it does once the edges are worth something --
        ``odometry_information`` or ``edge_information="hessian"`` (DESIGN, pose-graph section).
        ``odometry_information`` (6x6, or its 6 diagonal entries, over [translation, rotation]): the information of every
        odometry edge; None: the reference's constant (graph.cpp:279-288).
        ``remove_dynamic=True`` (not in the reference, whose addFeatureCloud only voxel-filters; needs ``resident=True``): the
        maps :meth:`get_final_feature_map` and :meth:`save` build leave out the points other keyframes looked through -- a car
        that stood at a junction for two keyframes and drove off (``lslam_vis_*``, :mod:`.visibility`).  ``dynamic_params``:
        ``KeyframeStore.vis_setup``'s keywords.  Voters of keyframe j: every keyframe, j included, whose optimised
        translation lies within ``2 * max_range`` of j's, at its optimised ``estimate``; the keyframe's own points are
        queried at the pose they are added with.  Off by default.
        ``occupancy=True`` or a dict of ``KeyframeStore.occ_setup``'s keywords (not in the reference; needs ``resident=True``):
        :meth:`occupancy_grid` is available and :meth:`save` also writes ``map.pgm`` / ``map.yaml``, the 2D occupancy grid a
        ``map_server`` loads (``lslam_occ_*``, :mod:`.occupancy`).  A dict without ``width`` / ``height`` has the bounds fitted
        to the poses.  None (the default): nothing changes.
        ``loop_search="covariance"`` (not in the reference, whose search is a fixed sqrt(5) m sphere): the candidates of a
        new keyframe are searched inside a radius sized by its pose uncertainty and gated on the Mahalanobis distance of the
        relative translation at probability ``loop_gate_prob``, the nearest ``loop_max_candidates`` at most
        (``LoopDetector.find_covariance_candidates``; ``PoseGraph.marginals`` / ``relative_covariances`` with
        ``covariance_opts``, e.g. ``dict(max_iters=..., coarse=1)``).  Every loop found by any detector then carries
        ``loop.mahalanobis`` = e^T (Sigma_rel + Omega_loop^-1)^-1 e, e the edge error of the verified relative pose at the
        current estimates; with ``loop_consistency_prob`` set, a loop whose value exceeds the chi-square quantile with 6
        degrees of freedom is dropped before it reaches the solver (:meth:`inconsistent_loops`).  None (the default):
        nothing changes, bit for bit."""
        if loop_search not in (None, "covariance"):
            raise ValueError("Graph: loop_search is None or \"covariance\"")
        self.loop_search = loop_search
        self.loop_gate_prob = float(loop_gate_prob)
        self.loop_max_candidates = int(loop_max_candidates)
        self.loop_consistency_prob = None if loop_consistency_prob is None else float(loop_consistency_prob)
        self.covariance_opts = dict(covariance_opts or {})
        self._inconsistent = []
        self.occupancy = None if occupancy is None or occupancy is False else ({} if occupancy is True else dict(occupancy))
        if self.occupancy is not None and not (resident or appearance_loops):
            raise ValueError("Graph: occupancy needs resident=True")
        self.remove_dynamic = bool(remove_dynamic)
        if self.remove_dynamic and not (resident or appearance_loops):
            raise ValueError("Graph: remove_dynamic=True needs resident=True")
        self.dynamic_params = dict(dynamic_params or {})
        if odometry_information is None:
            self.odometry_information = ODOMETRY_INFORMATION
        else:
            w = np.asarray(odometry_information, np.float64)
            self.odometry_information = np.diag(w) if w.shape == (6,) else w.reshape(6, 6).copy()
        self.floor_sigma = None
        if floor_sigma is not None:
            sn, sd = (float(v) for v in floor_sigma)
            if not (sn > 0.0 and sd > 0.0 and np.isfinite(sn) and np.isfinite(sd)):
                raise ValueError("Graph: floor_sigma is (sigma_normal [rad], sigma_distance [m]), both > 0")
            self.floor_sigma = (sn, sd)
        self.floor_params = floor_params
        self.floor_robust_kernel = floor_robust_kernel if kernel_kind(floor_robust_kernel) else None
        self.floor_robust_delta = float(floor_robust_delta)
        self.floor_world_plane = np.array(floor_world_plane, np.float64).reshape(4)
        self.floors = []            # (keyframe, plane prior index in the solver) of every accepted floor
        self.floors_not_found = []  # (keyframe, LSLAM_FLOOR_* status) of every keyframe whose floor was not found
        self.ctx = ctx
        self.gps_sigma = None
        if gps_sigma is not None:
            sxy, sz = (float(v) for v in gps_sigma)
            if not (sxy > 0.0 and sz > 0.0 and np.isfinite(sxy) and np.isfinite(sz)):
                raise ValueError("Graph: gps_sigma is (sigma_xy, sigma_z) in metres, both > 0")
            self.gps_sigma = (sxy, sz)
        self.gps_robust_kernel = gps_robust_kernel if kernel_kind(gps_robust_kernel) else None
        self.gps_robust_delta = float(gps_robust_delta)
        self.gps_min_spread = None if self.gps_sigma is None else (10.0 * self.gps_sigma[0] if gps_min_spread is None else float(gps_min_spread))
        self.imu_orientation_sigma = None if imu_orientation_sigma is None else float(imu_orientation_sigma)
        if self.imu_orientation_sigma is not None and not self.imu_orientation_sigma > 0.0:
            raise ValueError("Graph: imu_orientation_sigma [rad] must be > 0")
        self.utm_origin = None      # the first keyframe fix (fp64, host)
        self.gps_aligned = False    # the graph frame has been moved onto the fixes and no vertex is fixed any more
        self.gps_fixes = []         # (keyframe, prior index in the solver) of every GPS prior added
        self._prior_queue = []      # keyframes whose priors wait for the alignment
        self._bookkeeping_only = False  # tests: optimize() adds keyframes, edges and priors but never runs the solver
        if edge_information not in (None, "hessian"):
            raise ValueError("Graph: edge_information is None or \"hessian\"")
        if edge_information == "hessian":
            if range_sigma is None or not float(range_sigma) > 0.0:
                raise ValueError("Graph: edge_information=\"hessian\" needs range_sigma, the sensor's range noise [m]")
            if not (resident or appearance_loops):
                raise ValueError("Graph: edge_information=\"hessian\" needs resident=True")
        self.edge_information = edge_information
        self.range_sigma = None if range_sigma is None else float(range_sigma)
        self.edge_infos = []  # the lslam_edge_info of every solver edge, in edge order (edge_information="hessian" only)
        self.loop_robust_kernel = loop_robust_kernel if kernel_kind(loop_robust_kernel) else None
        self.loop_robust_delta = float(loop_robust_delta)
        self.solver = PoseGraph(device)
        self.loop_detector = loop_detector or LoopDetector(device=device, ctx=ctx)
        self.store = None
        self.keep_host_clouds = bool(keep_host_clouds)
        self.appearance_loops = bool(appearance_loops)
        if resident or self.appearance_loops:
            from .keyframe_store import KeyframeStore
            self.store = KeyframeStore(self.loop_detector.scan_match.ctx, store_max_points, store_max_keyframes, store_slab_points)
            if self.appearance_loops:
                self.store.sc_setup(**(sc_params or {}))
            if self.remove_dynamic:
                self.store.vis_setup(**self.dynamic_params)
        self.keyframe_updater = KeyframeUpdater()
        self.keyframes = []
        self.new_keyframes = []
        self.keyframe_queue = []
        self.max_keyframes_per_update = max_keyframes_per_update
        self.tf_odom2graph = np.eye(4)
        self.loops = []
        self.loop_edges = []  # solver edge index of every entry of self.loops

    # graph.cpp:230-246
    def add_frame(self, odom, corner_cloud, surf_cloud, utm_coord=None, imu_quat=None):
        """``utm_coord`` (x, y, z [m], projected -- what kf_fusion/fpdReceiver.cpp makes of a fix) and ``imu_quat`` (x, y, z, w)
        are keyframe.h:40-41's optional fields: stored on the keyframe, used only with ``gps_sigma`` / ``imu_orientation_sigma``."""
        odom = np.asarray(odom, np.float64).reshape(4, 4)
        if not self.keyframe_updater.update(odom):
            return None
        kf = KeyFrame(np.eye(4), self.keyframe_updater.get_accum_distance(), corner_cloud, surf_cloud,
                      frame_id=self.keyframe_updater.get_unique_id())
        kf.odom = odom.copy()
        kf.node = None
        kf.utm_coord = None if utm_coord is None else np.array(utm_coord, np.float64).reshape(3)
        kf.imu_quat = None if imu_quat is None else np.array(imu_quat, np.float64).reshape(4)
        if self.store is not None:
            kf.put_in_store(self.store, self.keep_host_clouds)
        self.keyframe_queue.append(kf)
        return kf

    # graph.cpp:248-297
    def flush_keyframe_queue(self):
        if not self.keyframe_queue:
            return False
        odom2map = self.tf_odom2graph.copy()
        n = min(len(self.keyframe_queue), self.max_keyframes_per_update)
        for i in range(n):
            kf = self.keyframe_queue[i]
            self.new_keyframes.append(kf)
            kf.estimate = odom2map @ kf.odom
            kf.node = self.solver.add_se3_node(kf.estimate)
            if i == 0 and not self.keyframes:
                continue
            prev = self.keyframes[-1] if i == 0 else self.keyframe_queue[i - 1]
            relative = np.linalg.inv(prev.odom) @ kf.odom
            info = self.odometry_information
            if self.edge_information == "hessian":  # the previous keyframe is the reference, the edge's measurement the pose
                info = self._hessian_information(self.odometry_information, [prev.store_id], np.eye(4, dtype=np.float32)[None],
                                                 kf.store_id, relative.astype(np.float32))
            self.solver.add_se3_edge(prev.node, kf.node, relative, info)
        del self.keyframe_queue[:n]
        return True

    def _hessian_information(self, omega_ref, ref_ids, rel_T, new_id, T):
        """One edge's information under ``edge_information="hessian"``; its lslam_edge_info is kept for reporting."""
        sm = self.loop_detector.scan_match
        ei = self.store.edge_information(ref_ids, rel_T, new_id, T, EDGE_INFORMATION_LEAVES)
        sm._resident, sm._resident_map = None, 0  # the context's map and scan belong to that call now
        self.edge_infos.append(ei)
        return hessian_information(omega_ref, np.array(ei.H, np.float64), ei.sum_b2, ei.n_rows, self.range_sigma)

    def edge_informations(self):
        """The ``lslam_edge_info`` (:class:`LslamEdgeInfo`) of every edge, in the solver's edge order, for reporting; empty
        without ``edge_information="hessian"``."""
        return list(self.edge_infos)

    # one pass of the loop in graph.cpp:313-383
    def optimize(self, max_iterations=1000):
        """-> (loops found in this pass, LM iterations run)."""
        if not self.flush_keyframe_queue():
            return [], 0
        if self.loop_search == "covariance":
            loops = self.loop_detector.detect_covariance(self.keyframes, self.new_keyframes, self._covariance_source(),
                                                         self.loop_gate_prob, self.loop_max_candidates)
        else:
            loops = self.loop_detector.detect_nearest(self.keyframes, self.new_keyframes)
        if self.appearance_loops:
            closed = set(id(lp.key2) for lp in loops)
            loops = loops + self.loop_detector.detect_appearance(self.keyframes,
                                                                 [k for k in self.new_keyframes if id(k) not in closed])
        if self.loop_search == "covariance":
            loops = self._consistent(loops)
        for lp in loops:
            info = LOOP_INFORMATION
            if self.edge_information == "hessian":
                if lp.ref_ids is None:
                    raise ValueError("Graph: edge_information=\"hessian\" needs loops verified in the keyframe store")
                info = self._hessian_information(LOOP_INFORMATION, lp.ref_ids, lp.rel_T, lp.key2.store_id, lp.relative_pose)
            self.loop_edges.append(self.solver.add_se3_edge(lp.key1.node, lp.key2.node, lp.relative_pose.astype(np.float64),
                                                            info, robust_kernel=self.loop_robust_kernel,
                                                            robust_delta=self.loop_robust_delta))
        self.loops.extend(loops)
        self.keyframes.extend(self.new_keyframes)
        added_priors = self._add_priors(self.new_keyframes)
        added_floors = self._add_floors(self.new_keyframes)
        self.new_keyframes = []
        iterations = 0
        if (loops or added_priors or added_floors) and not self._bookkeeping_only:
            iterations = self.solver.optimize(max_iterations)
            poses = self.solver.poses()
            from .pose_graph import pose7_to_mat
            for kf in self.keyframes:
                kf.estimate = pose7_to_mat(poses[kf.node])
        last = self.keyframes[-1]
        self.tf_odom2graph = last.estimate @ np.linalg.inv(last.odom)
        return loops, iterations

    # ---- covariance-gated loops (not in the reference) -------------------------------------------------------------------------
    def _covariance_source(self):
        """What the covariance search and the consistency test ask: the solver with this graph's options."""
        g = self

        class _Source:
            def marginals(self, vertices):
                return g.solver.marginals(vertices, **g.covariance_opts)

            def relative_covariances(self, ref, vertices):
                return g.solver.relative_covariances(ref, vertices, **g.covariance_opts)
        return getattr(self, "covariance_source", None) or _Source()

    def loop_consistency(self, key1, key2, relative_pose, information=None):
        """``loop_mahalanobis`` of a (would-be) loop edge key1 -> key2 at the current estimates, both keyframes in the solver."""
        from .loop_closure import loop_mahalanobis
        s_rel = self._covariance_source().relative_covariances(key1.node, [key2.node])
        return loop_mahalanobis(key1.estimate, key2.estimate, relative_pose, np.asarray(s_rel)[0],
                                LOOP_INFORMATION if information is None else information)

    def _consistent(self, loops):
        """``loop.mahalanobis`` on every loop; the loops that pass ``loop_consistency_prob`` (all, when it is None)."""
        from .loop_closure import chi2_quantile
        keep = []
        for lp in loops:
            lp.mahalanobis = self.loop_consistency(lp.key1, lp.key2, lp.relative_pose)
            if self.loop_consistency_prob is not None and lp.mahalanobis > chi2_quantile(self.loop_consistency_prob, 6):
                self._inconsistent.append(lp)
            else:
                keep.append(lp)
        return keep

    def inconsistent_loops(self):
        """The verified loops the consistency test kept out of the solver (``loop_consistency_prob``)."""
        return list(self._inconsistent)

    # ---- GPS fixes and IMU orientations as unary constraints (not in the reference) ------------------------------------------
    def _add_priors(self, new_keyframes):
        """The priors of a pass's new keyframes: queued until the fixes span a plane, then added -- all of them, after the graph
        frame has been moved onto the fixes.  -> whether any prior reached the solver."""
        if self.gps_sigma is None and self.imu_orientation_sigma is None:
            return False
        for kf in new_keyframes:
            kf.gps_local = None
            if self.gps_sigma is not None and kf.utm_coord is not None:
                if self.utm_origin is None:
                    self.utm_origin = kf.utm_coord.copy()
                kf.gps_local = kf.utm_coord - self.utm_origin  # fp64, before anything reaches the solver
            if kf.gps_local is not None or (self.imu_orientation_sigma is not None and kf.imu_quat is not None):
                self._prior_queue.append(kf)
        if self.gps_sigma is not None and not self.gps_aligned and not self._align_to_fixes():
            return False
        added = False
        for kf in self._prior_queue:
            if kf.gps_local is not None:
                sxy, sz = self.gps_sigma
                self.gps_fixes.append((kf, self.solver.add_se3_prior_xyz_edge(
                    kf.node, kf.gps_local, np.diag([1.0 / (sxy * sxy), 1.0 / (sxy * sxy), 1.0 / (sz * sz)]),
                    robust_kernel=self.gps_robust_kernel, robust_delta=self.gps_robust_delta)))
                added = True
            if self.imu_orientation_sigma is not None and kf.imu_quat is not None:
                w = np.zeros((6, 6))
                w[3:, 3:] = np.eye(3) * (2.0 / self.imu_orientation_sigma) ** 2
                q = kf.imu_quat / np.linalg.norm(kf.imu_quat)
                self.solver.add_se3_prior_pose_edge(kf.node, np.r_[0.0, 0.0, 0.0, q], w)
                added = True
        self._prior_queue = []
        return added

    def gps_spread(self):
        """The second singular value of the centred fix positions of the keyframes in the graph [m]: 0 on a line."""
        fixes = np.array([kf.gps_local for kf in self.keyframes if getattr(kf, "gps_local", None) is not None]).reshape(-1, 3)
        if len(fixes) < 3:
            return 0.0
        return float(np.linalg.svd(fixes - fixes.mean(0), compute_uv=False)[1])

    def _align_to_fixes(self):
        """Once the fixes span a plane: the rigid fit of the keyframes' estimate positions to their fixes moves every estimate
        and tf_odom2graph, and the solver is rebuilt with no fixed vertex.  -> whether that has happened."""
        if not self.gps_spread() >= self.gps_min_spread:
            return False
        pairs = [(kf.estimate[:3, 3], kf.gps_local) for kf in self.keyframes if getattr(kf, "gps_local", None) is not None]
        s, t = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
        T = rigid_fit(s, t)
        for kf in self.keyframes:
            kf.estimate = T @ kf.estimate
        self.tf_odom2graph = T @ self.tf_odom2graph
        self.solver.set_estimates([kf.estimate for kf in sorted(self.keyframes, key=lambda k: k.node)], fixed=-1)
        self.gps_aligned = True
        return True

    def gps_weights(self):
        """The robust weight (rho1) of every GPS prior in ``self.gps_fixes`` at the solver's current estimate; all 1 without
        ``gps_robust_kernel``."""
        if not self.gps_fixes:
            return np.zeros(0)
        return self.solver.prior_robust()["weight"][np.asarray([p for _, p in self.gps_fixes], np.int64)]

    def rejected_fixes(self, threshold=0.1):
        """The keyframes whose fix has a weight below ``threshold``.  Reporting only: nothing is removed from the graph."""
        return [kf for (kf, _), w in zip(self.gps_fixes, self.gps_weights()) if w < threshold]

    # ---- floor planes as plane priors (not in the reference) ----------------------------------------------------------------
    def _add_floors(self, new_keyframes):
        """The floors of a pass's new keyframes: detected in one call over the store (resident) or per cloud, the accepted ones
        added as plane priors.  -> whether any reached the solver."""
        if self.floor_sigma is None or not new_keyframes:
            return False
        from . import floor as floor_mod
        if self.store is not None:
            results = self.store.floor_detect([kf.store_id for kf in new_keyframes], self.floor_params)
        else:
            ctx = self.ctx or self.loop_detector.scan_match.ctx
            results = [floor_mod.detect(ctx, kf.surf_cloud, self.floor_params) for kf in new_keyframes]
        sn, sd = self.floor_sigma
        info = np.diag([1.0 / (sn * sn), 1.0 / (sn * sn), 1.0 / (sd * sd)])
        added = False
        for kf, r in zip(new_keyframes, results):
            kf.floor_result = r
            if r["status"] != floor_mod.FLOOR_OK:
                kf.floor_coeffs = None
                self.floors_not_found.append((kf, r["status"]))
                continue
            kf.floor_coeffs = np.array(r["plane"], np.float64)
            self.floors.append((kf, self.solver.add_se3_prior_plane_edge(
                kf.node, kf.floor_coeffs, info, world_plane4=self.floor_world_plane, robust_kernel=self.floor_robust_kernel,
                robust_delta=self.floor_robust_delta)))
            added = True
        return added

    def floor_weights(self):
        """The robust weight (rho1) of every plane prior in ``self.floors`` at the solver's current estimate; all 1 without
        ``floor_robust_kernel``."""
        if not self.floors:
            return np.zeros(0)
        return self.solver.plane_prior_robust()["weight"][np.asarray([p for _, p in self.floors], np.int64)]

    def rejected_floors(self, threshold=0.1):
        """The keyframes whose floor has a weight below ``threshold``.  Reporting only: nothing is removed from the graph."""
        return [kf for (kf, _), w in zip(self.floors, self.floor_weights()) if w < threshold]

    def loop_weights(self):
        """The robust weight (rho1) of every entry of ``self.loops`` at the solver's current estimate, i.e. after the last
        optimise; all 1 without ``loop_robust_kernel``."""
        if not self.loops:
            return np.zeros(0)
        return self.solver.edge_robust()["weight"][np.asarray(self.loop_edges, np.int64)]

    def rejected_loops(self, threshold=0.1):
        """The loops whose weight is below ``threshold``.  Reporting only: nothing is removed from the graph."""
        w = self.loop_weights()
        return [lp for lp, wk in zip(self.loops, w) if wk < threshold]

    def _voters(self, kf, keyframes):
        """The keyframes that vote on ``kf``'s points (``remove_dynamic``): those of ``keyframes`` in the store, ``kf`` included,
        whose optimised translation lies within ``2 * max_range`` of ``kf``'s -> (store ids, 4x4 estimates)."""
        reach = 2.0 * float(self.store.vis_info()["max_range"])
        at = np.asarray(kf.estimate, np.float64)[:3, 3]
        near = [o for o in keyframes if getattr(o, "store", None) is self.store
                and np.linalg.norm(np.asarray(o.estimate, np.float64)[:3, 3] - at) <= reach]
        return [o.store_id for o in near], [np.asarray(o.estimate, np.float64) for o in near]

    def _add_stored(self, kf, fm, est, keyframes, removed):
        """A stored keyframe's clouds into ``fm`` at ``est``; with ``remove_dynamic`` through the visibility filter, the
        (corner, surf) points it left out appended to ``removed``."""
        if not self.remove_dynamic:
            kf.store.add_to_fmap(kf.store_id, fm, est)
            return
        if kf.store is not self.store:
            raise ValueError("Graph: remove_dynamic=True needs every keyframe in the graph's store")
        ids, poses = self._voters(kf, keyframes)
        removed.append(kf.store.vis_add_to_fmap(kf.store_id, fm, est, ids, poses))

    def occupancy_grid(self, poses="estimate", floor=True, keyframes=None):
        """The 2D occupancy grid of the keyframes' ray-cast votes (:mod:`.occupancy`; not in the reference), at
        ``poses="estimate"`` (the optimised ``kf.estimate``) or ``"odom"``.  The bounds are fitted to the poses unless the
        ``occupancy`` dict gives ``width`` and ``height``; with ``floor`` each keyframe's floor is detected where its cloud lies
        (``KeyframeStore.floor_detect``) and decides what is an obstacle, a keyframe whose status is not OK falls back to
        (up axis, ``sensor_height``); the detection runs with the graph's ``floor_params``, or -- without any -- with the
        grid's up axis and ``sensor_height``.  Clears the store's grid and integrates every keyframe -> dict: ``values`` (height,
        width) int8, ``counts`` uint32, ``params`` (:class:`LslamOccParams`), ``stats``, ``floors_found``."""
        from . import floor as floor_mod
        from . import occupancy as occ
        if self.occupancy is None:
            raise ValueError("Graph.occupancy_grid: the graph was created without occupancy")
        if poses not in ("estimate", "odom"):
            raise ValueError("Graph.occupancy_grid: poses is \"estimate\" or \"odom\"")
        every = self.keyframes if keyframes is None else keyframes
        if not every or not all(getattr(kf, "store", None) is self.store for kf in every):
            raise ValueError("Graph.occupancy_grid: needs keyframes, every one in the graph's store")
        T = [np.asarray(kf.estimate if poses == "estimate" else kf.odom, np.float64).astype(np.float32).reshape(4, 4) for kf in every]
        if "width" in self.occupancy and "height" in self.occupancy:
            p = occ.occ_params(self.occupancy)
        else:
            p = occ.fit_bounds(T, self.occupancy)
        ids = [kf.store_id for kf in every]
        planes = valid = None
        if floor:
            fp = self.floor_params
            if fp is None:  # the floor's up direction and height follow the grid's
                fp = dict(up=(0.0, 1.0, 0.0) if p.up_axis == 1 else (0.0, 0.0, 1.0), sensor_height=p.sensor_height)
            results = self.store.floor_detect(ids, fp)
            planes = np.array([r["plane"] for r in results], np.float64).reshape(len(ids), 4)
            valid = np.array([r["status"] == floor_mod.FLOOR_OK for r in results], np.int32)
            planes[valid == 0] = 0.0
        self.store.occ_setup(p)
        self.store.occ_clear()
        self.store.occ_integrate(ids, T, planes, valid)
        return dict(values=self.store.occ_values(), counts=self.store.occ_counts(), params=p, stats=self.store.occ_info(),
                    floors_found=int(valid.sum()) if valid is not None else 0)

    def map_quality(self, poses="estimate", which="surf", keyframes=None, **params):
        """Mean map entropy and mean plane variance (:mod:`.map_quality`; not in the reference) of the keyframes' clouds of
        one type put together at their poses -- ``poses="estimate"``: the optimised ``kf.estimate``; ``"odom"``: the odometry
        poses ``kf.odom`` they started from -- so the two calls score what the optimisation did to the MAP, without ground
        truth: lower is crisper.  A resident graph evaluates the clouds where they lie in the store
        (``KeyframeStore.map_quality``); a host graph moves them on the host by the same fp32 formula and uploads
        (``map_quality.evaluate``).  Keywords: ``radius``, ``min_neighbors``, ``lambda_floor`` -> the stats as a dict."""
        from . import map_quality
        if poses not in ("estimate", "odom"):
            raise ValueError("Graph.map_quality: poses is \"estimate\" or \"odom\"")
        every = self.keyframes if keyframes is None else keyframes
        t = map_quality._which(which)
        T = [np.asarray(kf.estimate if poses == "estimate" else kf.odom, np.float64).astype(np.float32).reshape(4, 4) for kf in every]
        if self.store is not None and all(getattr(kf, "store", None) is self.store for kf in every):
            return self.store.map_quality([kf.store_id for kf in every], T, t, **params)
        clouds = []
        for kf, M in zip(every, T):
            c = np.asarray(kf.surf_cloud if t else kf.corner_cloud, np.float32)[:, :3]
            x, y, z = c[:, 0:1], c[:, 1:2], c[:, 2:3]
            clouds.append(((M[None, :3, 0] * x + M[None, :3, 1] * y) + M[None, :3, 2] * z) + M[None, :3, 3])
        cloud = np.concatenate(clouds, axis=0) if clouds else np.zeros((0, 3), np.float32)
        return map_quality.evaluate(self.ctx or self.loop_detector.scan_match.ctx, cloud, **params)

    # graph.cpp:150-199 (driven by Graph::save, :106-147)
    def get_final_feature_map(self, ctx=None, directory=None, cube_dims=(121, 111, 121), bootstrap=False, keyframes=None):
        """``Graph::getFinalFeatureMap``: rebuild the map from the optimised keyframes, one after the other -- keyframe k is
        scan-matched against a map that already holds keyframes 0 .. k-1: ``feature_map2.update(estimate)`` ->
        ``getSurroundFeature`` -> VoxelGrid 0.2 / 0.3 of the keyframe's clouds -> ``scanMatchScan`` (default ``ScanMatch``: 10
        iterations, 0.05 / 0.05, score gate on) from the keyframe's estimate -> ``addFeatureCloud`` with the refined estimate
        iff the match succeeded -> ``saveCloudToFiles`` into ``directory`` (if given).  All of it on the device: the map never
        leaves HBM between keyframes.

        Quirk kept (``bootstrap=False``, the reference as written): the map starts empty, the first keyframe's match returns
        false for want of reference points (ScanMatch.cpp:57-61), nothing is added -- and so for every keyframe after it: the
        reference's ``graph2`` map stays empty.  ``bootstrap=True`` adds a keyframe WITHOUT a match while the surround holds
        fewer than the 50 corner / 100 surface points a match needs -- what the loop was presumably meant to do, and what the
        bench's ``final_feature_map`` leg times.

        Returns a dict: ``map`` (the FeatureMap; the caller closes it), ``matched`` (one bool per keyframe), ``poses`` (the
        refined 4x4 estimates, float32), ``added`` (keyframes added to the map), ``stats`` (the last lslam_stats) and, with
        ``remove_dynamic``, ``removed`` (the (corner, surf) points left out, one pair per keyframe added)."""
        from .feature_map import FeatureMap, voxel_grid
        ctx = ctx or self.loop_detector.scan_match.ctx
        if self.remove_dynamic and ctx is not self.store.ctx:
            raise ValueError("Graph: remove_dynamic=True needs the map on the store's context")
        removed = []
        every = self.keyframes if keyframes is None else keyframes
        fm = FeatureMap(ctx, *cube_dims)
        fm.setup_filter_size(0.2, 0.2, 0.4)
        opts = ctx.default_opts()  # lidar_slam::ScanMatch scan_match; (ScanMatch.cpp:21-33)
        matched, poses, added, last = [], [], 0, None
        for kf in every:
            est = np.asarray(kf.estimate, np.float64).astype(np.float32).reshape(4, 4)  # node->estimate().cast<float>()
            fm.update(est[:3, 3])
            nc, ns = fm.surround_counts()
            # a stored keyframe (resident=True) is filtered, matched and added where it is: no cloud crosses PCIe
            stored = getattr(kf, "store", None) is not None and kf.store.ctx is ctx
            if not stored:
                corner = voxel_grid(ctx, kf.corner_cloud, 0.2)
                surf = voxel_grid(ctx, kf.surf_cloud, 0.3)
            ok = False
            if nc >= 50 and ns >= 100:  # else scanMatchScan says "reference cloud points too few" and leaves the pose alone
                fm.surround_to_map()
                if stored:
                    status, pose, st = kf.store.scanmatch(kf.store_id, 0.2, 0.3, ctx.isometry_to_pose(est), opts)
                else:
                    status, pose, st = ctx.scanmatch_scan(corner, surf, ctx.isometry_to_pose(est), opts)
                last = st
                if int(status) != 1:
                    est = ctx.pose_to_isometry(pose)  # written back also when the match failed (ScanMatch.cpp:342-346)
                ok = int(status) == 0
            if ok or (bootstrap and not (nc >= 50 and ns >= 100)):
                if stored:
                    self._add_stored(kf, fm, est, every, removed)
                elif self.remove_dynamic:
                    raise ValueError("Graph: remove_dynamic=True needs every keyframe in the graph's store")
                else:
                    fm.add_feature_cloud(kf.corner_cloud, kf.surf_cloud, est)
                added += 1
            matched.append(ok)
            poses.append(np.array(est, np.float32))
        if directory is not None:
            fm.save_cloud_to_files(directory)
        out = {"map": fm, "matched": matched, "poses": poses, "added": added, "stats": last}
        if self.remove_dynamic:
            out["removed"] = removed
        return out

    # graph.cpp:106-147
    def save(self, directory, bootstrap=False, max_iterations=1000):
        """``Graph::save`` with the reference's hard-coded paths replaced by ``directory``: ``graph_before.g2o``, a final
        optimisation, ``graph_end.g2o``, the keyframes' estimates and ``tf_odom2graph`` refreshed, the map of all keyframes at
        their optimised poses (a ``FeatureMap(121, 111, 121)`` with its default filter sizes: ``update`` + ``addFeatureCloud``
        per keyframe, no match) saved into ``directory/graph``, the trajectory clouds ``traj_graph.pcd`` / ``traj_odom.pcd``,
        then :meth:`get_final_feature_map` into ``directory/graph2``.  Works with and without ``resident``.  -> the dict of
        :meth:`get_final_feature_map` (its map closed), with ``iterations`` of the final optimisation.  With ``occupancy``
        also ``directory/map.pgm`` and ``directory/map.yaml`` (:meth:`occupancy_grid`, ``occupancy.save_map``), and the grid
        under ``occupancy`` in the result; without it nothing new is written."""
        import os
        from .feature_map import FeatureMap
        from .pose_graph import pose7_to_mat
        if not self.keyframes:
            raise ValueError("Graph.save: the graph holds no keyframes")
        os.makedirs(directory, exist_ok=True)
        self.solver.save(os.path.join(directory, "graph_before.g2o"))
        iterations = self.solver.optimize(max_iterations)
        self.solver.save(os.path.join(directory, "graph_end.g2o"))
        poses = self.solver.poses()
        for kf in self.keyframes:
            kf.estimate = pose7_to_mat(poses[kf.node])
        last = self.keyframes[-1]
        self.tf_odom2graph = last.estimate @ np.linalg.inv(last.odom)
        ctx = self.loop_detector.scan_match.ctx
        fm = FeatureMap(ctx, 121, 111, 121)
        try:
            for kf in self.keyframes:
                est = np.asarray(kf.estimate, np.float64).astype(np.float32)
                fm.update(est[:3, 3])
                if getattr(kf, "store", None) is not None and kf.store.ctx is ctx:
                    self._add_stored(kf, fm, est, self.keyframes, [])
                else:
                    fm.add_feature_cloud(kf.corner_cloud, kf.surf_cloud, est)
            os.makedirs(os.path.join(directory, "graph"), exist_ok=True)
            fm.save_cloud_to_files(os.path.join(directory, "graph"))
        finally:
            fm.close()
        save_trajectory_cloud(os.path.join(directory, "traj_graph.pcd"), [kf.estimate for kf in self.keyframes])
        save_trajectory_cloud(os.path.join(directory, "traj_odom.pcd"), [kf.odom for kf in self.keyframes])
        os.makedirs(os.path.join(directory, "graph2"), exist_ok=True)
        out = self.get_final_feature_map(ctx=ctx, directory=os.path.join(directory, "graph2"), bootstrap=bootstrap)
        out["map"].close()
        out["iterations"] = iterations
        if self.occupancy is not None:
            from . import occupancy as occ
            grid = self.occupancy_grid()
            occ.save_map(os.path.join(directory, "map"), grid["values"], grid["params"])
            out["occupancy"] = grid
        return out


def trajectory_rows(poses):
    """generateGraphTrajectoryCloud / generateOdomTrajectoryCloud: one PointXYZINormal per pose -- position = translation,
    normal = the quaternion's x, y, z, intensity = its w (the quaternion of the float-cast rotation), curvature = index."""
    from .pose_graph import mat_to_pose7
    rows = np.zeros((len(poses), 8), np.float32)
    for i, T in enumerate(poses):
        Tf = np.asarray(T, np.float64).astype(np.float32)
        p = mat_to_pose7(Tf.astype(np.float64))
        q = p[3:]
        rows[i, :3] = Tf[:3, 3]
        rows[i, 3] = q[3]
        rows[i, 4:7] = q[:3]
        rows[i, 7] = i
    return rows


def save_trajectory_cloud(path, poses):
    """ASCII PCD, fields ``x y z intensity normal_x normal_y normal_z curvature``."""
    rows = trajectory_rows(poses)
    with open(path, "w") as f:
        f.write("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\n"
                "FIELDS x y z intensity normal_x normal_y normal_z curvature\nSIZE 4 4 4 4 4 4 4 4\nTYPE F F F F F F F F\n"
                "COUNT 1 1 1 1 1 1 1 1\nWIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA ascii\n" % (len(rows), len(rows)))
        for r in rows:
            f.write(" ".join(repr(float(v)) for v in r) + "\n")
