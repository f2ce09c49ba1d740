"""Host-side mirror of the loop-closure front end, ``pose_graph::LoopDetector``
(/root/reference/L_SLAM/src/pose_graph/loop_detector.hpp:50-280): trajectory radius search,
candidate gating, coarse alignment hook, ``ScanMatch::scanMatchLocal`` fine alignment (SURVEY 8f row
n3).  The arithmetic that matters -- the fine alignment -- runs on the device through
:class:`ScanMatch`; the gating is a few comparisons per keyframe and stays on the host, as in the
reference.

Three things of the reference are restated as they are, not as they were probably meant:
  * ``radiusSearch(pos, 5.0, ...)`` (loop_detector.hpp:124-126) hands 5.0 to nanoflann's
    RadiusResultSet, which compares SQUARED distances with it (util/nanoflann_pcl.h:166-186), so
    the search radius is sqrt(5) m and the ``>= estimated_distance_thresh`` break (:133) never fires;
  * the same ``KdTreeFLANN::radiusSearch`` takes its result count from
    ``_kdtree.findNeighbors(...)`` (nanoflann_pcl.h:173), which in the vendored nanoflann returns
    ``result.full()`` -- a bool, always true for a RadiusResultSet (nanoflann.hpp:171,1304-1322) --
    so it hands back exactly ONE result, the nearest trajectory point (after the sort, :175-176).
    Checked against the reference's own nanoflann (tests/test_loop_closure.py).  When nothing lies
    within the radius the reference still reports one result and reads element 0 of an empty
    vector (undefined behaviour: in practice a stale entry of an earlier search); that is not
    reproduced -- ``radius_search`` returns nothing then.  ``single_result_quirk = False`` gives
    the search its documented meaning (all points within the radius, ascending);
  * the trajectory is flattened with ``pos.y = 0`` (:98,120).
The coarse alignment (``corseMatching``, :232-255) is PCL's ``IterativeClosestPoint`` with default
settings -- external, parity unpinned: the default ``coarse_matcher`` is the device ICP
(``lslam_icp_align``, csrc/lslam_icp.hip, PCL's defaults restated), including the reference's two
guards -- an empty reference cloud and a non-converged ICP both reject the candidate.  Any
``(reference_surf, surf, guess4x4) -> (converged, guess4x4)`` callable can be passed instead.
"""
import numpy as np

from .scan_match import ScanMatch


class KeyFrame:
    """pose_graph/keyframe.h: estimate (4x4, float64), accumulated travel distance, feature clouds
    ((n, 4) {x,y,z,intensity} in the keyframe's own frame)."""

    def __init__(self, estimate, accum_distance, corner_cloud, surf_cloud, frame_id=0):
        self.estimate = np.asarray(estimate, np.float64).reshape(4, 4)
        self.accum_distance = float(accum_distance)
        self.store, self.store_id = None, None  # a KeyframeStore that holds the clouds on the device, and the id there
        self.corner_cloud = np.ascontiguousarray(corner_cloud, np.float32)
        self.surf_cloud = np.ascontiguousarray(surf_cloud, np.float32)
        self.frame_id = frame_id

    # the clouds on the host; a stored keyframe whose host copies were dropped (Graph(keep_host_clouds=False)) fetches them
    @property
    def corner_cloud(self):
        return self._corner if self._corner is not None else self.store.get(self.store_id, 0)

    @corner_cloud.setter
    def corner_cloud(self, cloud):
        self._corner = cloud

    @property
    def surf_cloud(self):
        return self._surf if self._surf is not None else self.store.get(self.store_id, 1)

    @surf_cloud.setter
    def surf_cloud(self, cloud):
        self._surf = cloud

    def put_in_store(self, store, keep_host_clouds=True):
        """Upload the clouds once into ``store`` (a :class:`KeyframeStore`) and remember the id."""
        self.store_id = store.add(self._corner, self._surf)
        self.store = store
        if not keep_host_clouds:
            self._corner = self._surf = None


class Loop:
    """loop_detector.hpp:18-48."""

    def __init__(self, key1, key2, relative_pose, ref_ids=None, rel_T=None):
        """``ref_ids`` / ``rel_T``: the store ids and transforms of the keyframes whose local clouds the verification matched
        against (None where the keyframes are not in a store) -- what ``Graph(edge_information="hessian")`` builds the edge's
        match Hessian from."""
        self.key1, self.key2 = key1, key2
        self.relative_pose = np.asarray(relative_pose, np.float32).reshape(4, 4)
        self.ref_ids = None if ref_ids is None else [int(i) for i in ref_ids]
        self.rel_T = None if rel_T is None else np.ascontiguousarray(rel_T, np.float32).reshape(-1, 4, 4)
        self.mahalanobis = None  # Graph(loop_search="covariance"): e^T (Sigma_rel + Omega^-1)^-1 e when the loop was found


# chi-square quantiles for the covariance gates: the two tabulated values the defaults need, Wilson-Hilferty otherwise
CHI2_3_99, CHI2_6_99 = 11.345, 16.812


def chi2_quantile_wh(p, k):
    """Wilson-Hilferty: chi2_k(p) ~ k (1 - 2 / (9 k) + z_p sqrt(2 / (9 k)))^3, z_p the normal quantile.  Within 1 % of the
    tabulated 0.99 quantiles for k = 3 and 6 (tests/test_loop_covariance_gate.py)."""
    from statistics import NormalDist
    if not 0.0 < p < 1.0:
        raise ValueError("chi2 quantile: the probability must be in (0, 1)")
    a = 2.0 / (9.0 * k)
    return k * (1.0 - a + NormalDist().inv_cdf(p) * a ** 0.5) ** 3


def chi2_quantile(p, k):
    if p == 0.99 and k == 3:
        return CHI2_3_99
    if p == 0.99 and k == 6:
        return CHI2_6_99
    return chi2_quantile_wh(p, k)


def edge_error(key1_estimate, key2_estimate, relative_pose):
    """The solver's edge error of an edge (key1, key2) measured as ``relative_pose`` at the given estimates:
    toVectorMQT(Z^-1 X1^-1 X2) = [translation, quaternion vector with w >= 0], fp64."""
    from .pose_graph import mat_to_pose7
    def inv(T):  # Eigen::Isometry3d::inverse(), [R^T | -R^T t], as the C++ mirror: a verified pose comes out of an fp32 matcher
        T = np.asarray(T, np.float64)  # and its rotation is orthonormal only to fp32 -- a general inverse differs from this by 1e-7
        out = np.eye(4)
        out[:3, :3] = T[:3, :3].T
        out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
        return out
    E = inv(relative_pose) @ (inv(key1_estimate) @ np.asarray(key2_estimate, np.float64))
    p = mat_to_pose7(E)
    q = p[3:] / np.linalg.norm(p[3:])
    if q[3] < 0:
        q = -q
    return np.r_[p[:3], q[:3]]


def loop_mahalanobis(key1_estimate, key2_estimate, relative_pose, sigma_rel, information):
    """e^T (Sigma_rel + Omega^-1)^-1 e for a verified loop: e the edge error of the verified relative pose at the current
    estimates, Sigma_rel the covariance of X1^-1 X2 (``PoseGraph.relative_covariances``), Omega the loop's information."""
    e = edge_error(key1_estimate, key2_estimate, relative_pose)
    S = np.asarray(sigma_rel, np.float64).reshape(6, 6) + np.linalg.inv(np.asarray(information, np.float64).reshape(6, 6))
    return float(e @ np.linalg.solve(S, e))


def transform_cloud(cloud, tf):
    """pcl::transformPointCloud with an Isometry3f: p' = R p + t, fp32, intensity kept."""
    c = np.ascontiguousarray(cloud, np.float32)
    T = np.asarray(tf, np.float32)
    out = c.copy()
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    for r in range(3):
        out[:, r] = ((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]
    return out


class LoopDetector:
    def __init__(self, scan_match=None, coarse_matcher=None, device=0, ctx=None):
        # loop_detector.hpp:55-63
        self.single_result_quirk = True  # nanoflann_pcl.h:173 (see the module docstring)
        self.estimated_distance_thresh = 25.0
        self.accum_distance_thresh = 30.0
        self.last_loop_interval_thresh = 3.0
        self.fitness_score_thresh = 0.5
        # detect_appearance (not in the reference).  0.2 is the upper end of the range the descriptor's authors use; it was not
        # tuned on this project's data
        self.sc_distance_thresh = 0.2
        self.sc_top_k = 4
        self.loop_count = 0
        self.last_gate = []  # find_covariance_candidates: (keyframe, d2) of every candidate it gated last
        self.last_loop_accum_distance = 0.0
        self._trajectory = np.zeros((0, 4), np.float32)
        self._scan_match = scan_match
        self._device, self._ctx = device, ctx
        self.coarse_matcher = coarse_matcher or self._icp_coarse_matcher

    @property
    def scan_match(self):
        if self._scan_match is None:  # created on first use: the gating needs no device
            self._scan_match = ScanMatch(10, device=self._device, ctx=self._ctx)
        return self._scan_match

    def _icp_coarse_matcher(self, refer_surf, surf, guess):
        """corseMatching, loop_detector.hpp:232-255: registration->align(aligned, guess) with PCL's defaults."""
        if len(refer_surf) == 0:  # :233-235
            return False, guess
        T, converged, _its, _fit = self.scan_match.ctx.icp_align(refer_surf, surf, guess)
        return converged, T

    def get_distance_thresh(self):
        return self.estimated_distance_thresh

    def get_loop_count(self):
        return self.loop_count

    # ---- loop_detector.hpp:66-87 --------------------------------------------------------------
    def detect_nearest(self, keyframes, new_keyframes):
        """-> list of Loop (the reference's bool is ``len(result) > 0``)."""
        self.update_trajectory(keyframes)
        loops = []
        for nk in new_keyframes:
            cand = self.find_nearest_candidates(keyframes, nk)
            if cand:
                loop = self.matching_nearest(cand, nk)
                if loop is not None:
                    loops.append(loop)
                    self.loop_count += 1
        return loops

    # ---- not in the reference: candidates by appearance (lslam_sc_*) --------------------------------
    def appearance_candidates(self, keyframes, new_keyframe):
        """The scan-context candidate list of one new keyframe -> (ids, shifts, dists) in the store's ids, best first; empty
        when the interval rule skips the keyframe or no keyframe is ``accum_distance_thresh`` of travel behind it.  No gate
        on the estimated distance: that is the point."""
        none = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
        store = new_keyframe.store
        if store is None:
            raise ValueError("detect_appearance: the new keyframe is not in a KeyframeStore")
        if new_keyframe.accum_distance - self.last_loop_accum_distance < self.last_loop_interval_thresh:
            return none
        # accumulated distance is monotone in the id: the eligible candidates are the ids up to one limit
        max_cand = -1
        for k in keyframes:
            if k.store is store and k.store_id < new_keyframe.store_id and k.store_id > max_cand and \
                    new_keyframe.accum_distance - k.accum_distance >= self.accum_distance_thresh:
                max_cand = k.store_id
        if max_cand < 0:
            return none
        if not store.sc_info()["is_set"]:
            store.sc_setup()
        return store.sc_query([new_keyframe.store_id], [max_cand], self.sc_top_k)[0]

    def detect_appearance(self, keyframes, new_keyframes):
        """Loops found from what the new keyframes look like, not from where their estimates put them: per new keyframe the
        ``sc_top_k`` nearest scan-context descriptors among the keyframes at least ``accum_distance_thresh`` of travel back;
        those below ``sc_distance_thresh`` are verified in list order by ``lslam_kfs_loop_match`` (one candidate, started from
        the rotation the descriptor shift stands for); the first accepted one is the Loop.  All keyframes involved must be in
        one :class:`KeyframeStore` on this detector's context.  -> list of Loop."""
        from .capi import Status
        from .keyframe_store import LOOP_ACCEPTED, MATCH_FAILED, sc_shift_guess
        by_id = {}
        for k in keyframes:
            if k.store is not None:
                by_id[(id(k.store), k.store_id)] = k
        loops = []
        for nk in new_keyframes:
            ids, shifts, dists = self.appearance_candidates(keyframes, nk)
            if not len(ids):
                continue
            store, sm = nk.store, self.scan_match
            if store.ctx is not sm.ctx:
                raise ValueError("detect_appearance: the keyframe store is not on the detector's context")
            info = store.sc_info()
            for cid, shift, dist in zip(ids, shifts, dists):
                if not dist < self.sc_distance_thresh:
                    break  # the list is sorted
                cand = by_id.get((id(store), int(cid)))
                if cand is None:
                    continue
                guess = sc_shift_guess(shift, info["n_sector"], info["up_axis"])
                r = store.loop_match([int(cid)], np.eye(4, dtype=np.float32)[None], nk.store_id, guess, sm.opts)
                if r["stage"] >= MATCH_FAILED:
                    sm._resident, sm._resident_map = None, 0
                    sm._finish(Status(r["stats"].status), r["stats"])
                if r["stage"] != LOOP_ACCEPTED:
                    continue
                self.last_loop_accum_distance = nk.accum_distance
                loops.append(Loop(cand, nk, r["guess"], [int(cid)], np.eye(4, dtype=np.float32)[None]))
                self.loop_count += 1
                break
        return loops

    # ---- :93-106 ----------------------------------------------------------------------------------
    def update_trajectory(self, keyframes):
        t = np.zeros((len(keyframes), 4), np.float32)
        for i, k in enumerate(keyframes):
            t[i, :3] = k.estimate[:3, 3].astype(np.float32)
            t[i, 1] = 0.0
            t[i, 3] = i
        self._trajectory = t

    def radius_search(self, pos, radius):
        """KdTreeFLANN::radiusSearch (util/nanoflann_pcl.h:166-186): `radius` is compared with
        SQUARED distances; results ascending by distance."""
        t = self._trajectory
        d = t[:, :3] - np.asarray(pos, np.float32)[None, :3]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        idx = np.nonzero(d2 < np.float32(radius))[0]
        order = np.argsort(d2[idx], kind="stable")
        if self.single_result_quirk:
            order = order[:1]
        return idx[order], d2[idx][order]

    # ---- :108-164 ---------------------------------------------------------------------------------
    def find_nearest_candidates(self, keyframes, new_keyframe):
        if new_keyframe.accum_distance - self.last_loop_accum_distance < self.last_loop_interval_thresh:
            return []
        pos = new_keyframe.estimate[:3, 3].astype(np.float32).copy()
        pos[1] = 0.0
        r_indices, r_sqr = self.radius_search(pos, 5.0)
        if len(r_indices) <= 0:
            return []
        candidates = []
        candidate_dist = 0.0
        for i in range(len(r_sqr)):
            if len(candidates) >= 6:
                break
            if r_sqr[i] >= self.estimated_distance_thresh:
                break
            keyframe_index = int(round(float(self._trajectory[r_indices[i], 3])))
            kf = keyframes[keyframe_index]
            if new_keyframe.accum_distance - kf.accum_distance < self.accum_distance_thresh:
                continue
            if not candidates:
                candidate_dist = kf.accum_distance
            elif abs(candidate_dist - kf.accum_distance) > 5.0:
                continue
            candidates.append(kf)
        return candidates

    # ---- not in the reference: candidates by pose uncertainty (lslam_pg_marginals) --------------------
    def find_covariance_candidates(self, keyframes, new_keyframe, solver, gate_prob=0.99, max_candidates=32):
        """:meth:`find_nearest_candidates` with the fixed sqrt(5) m sphere replaced by one sized by the new keyframe's
        uncertainty and a Mahalanobis gate per candidate.  ``solver``: whatever has ``marginals(vertices)`` and
        ``relative_covariances(ref, vertices)`` over the keyframes' ``node`` ids (:class:`PoseGraph`), the new keyframe in it.
          1. radius = max(sqrt(5), sqrt(chi2_3(p) lambda_max(Sigma_nn,tt))) -- a HEURISTIC proxy: Sigma_nn is the new
             keyframe's uncertainty against the gauge, not against each candidate; it only has to be generous.
          2. the old keyframes inside it (the detector's trajectory: y zeroed, as the reference's search) that are
             ``accum_distance_thresh`` of travel back; the nearest ``max_candidates`` of them.
          3. ONE relative_covariances call gives their exact Sigma_rel; each is gated on d2 = v^T Sigma_rel,tt^-1 v <=
             chi2_3(p), v = R_j^T (t_j - t_new): the relative translation in the candidate's frame, which is the frame the
             translation block of Sigma_rel (an edge error's coordinates) is in.
          4. survivors in order of d2; then the reference's grouping (5 m of accumulated distance around the first, at most 6).
        -> candidates, and ``self.last_gate`` = [(keyframe, d2)] of everything step 3 looked at."""
        self.last_gate = []
        if new_keyframe.accum_distance - self.last_loop_accum_distance < self.last_loop_interval_thresh:
            return []
        chi2 = chi2_quantile(gate_prob, 3)
        s_nn = np.asarray(solver.marginals([new_keyframe.node]), np.float64).reshape(6, 6)
        lam = float(np.linalg.eigvalsh(s_nn[:3, :3]).max())
        radius2 = max(5.0, chi2 * max(lam, 0.0))
        pos = new_keyframe.estimate[:3, 3].astype(np.float64).copy()
        pos[1] = 0.0
        t = self._trajectory.astype(np.float64)
        d = t[:, :3] - pos[None]
        d2 = (d * d).sum(1)
        near = []
        for i in np.argsort(d2, kind="stable"):
            if not d2[i] < radius2 or len(near) >= max_candidates:
                break
            kf = keyframes[int(round(float(t[i, 3])))]
            if kf is new_keyframe or new_keyframe.accum_distance - kf.accum_distance < self.accum_distance_thresh:
                continue
            near.append(kf)
        if not near:
            return []
        s_rel = np.asarray(solver.relative_covariances(new_keyframe.node, [k.node for k in near]), np.float64).reshape(-1, 6, 6)
        gated = []
        for kf, S in zip(near, s_rel):
            v = kf.estimate[:3, :3].T @ (kf.estimate[:3, 3] - new_keyframe.estimate[:3, 3])
            m = float(v @ np.linalg.solve(S[:3, :3], v))
            self.last_gate.append((kf, m))
            if m <= chi2:
                gated.append((m, len(gated), kf))
        gated.sort(key=lambda g: g[:2])
        candidates, candidate_dist = [], 0.0
        for _m, _k, kf in gated:
            if len(candidates) >= 6:
                break
            if not candidates:
                candidate_dist = kf.accum_distance
            elif abs(candidate_dist - kf.accum_distance) > 5.0:
                continue
            candidates.append(kf)
        return candidates

    def detect_covariance(self, keyframes, new_keyframes, solver, gate_prob=0.99, max_candidates=32):
        """:meth:`detect_nearest` over :meth:`find_covariance_candidates`: the same arguments, plus the solver that already
        holds the new keyframes' vertices and odometry edges."""
        self.update_trajectory(keyframes)
        loops = []
        for nk in new_keyframes:
            cand = self.find_covariance_candidates(keyframes, nk, solver, gate_prob, max_candidates)
            if cand:
                loop = self.matching_nearest(cand, nk)
                if loop is not None:
                    loops.append(loop)
                    self.loop_count += 1
        return loops

    # ---- :166-230 ---------------------------------------------------------------------------------
    def matching_nearest(self, candidate_keyframes, new_keyframe):
        if not candidate_keyframes:
            return None
        candidate_tf = candidate_keyframes[0].estimate
        inv = np.linalg.inv(candidate_tf)
        store = new_keyframe.store
        if store is not None and all(k.store is store for k in candidate_keyframes) and \
                self.coarse_matcher == self._icp_coarse_matcher and store.ctx is self.scan_match.ctx:
            return self._matching_nearest_stored(store, candidate_keyframes, new_keyframe, inv)
        corner_local = [candidate_keyframes[0].corner_cloud]
        surf_local = [candidate_keyframes[0].surf_cloud]
        for k in candidate_keyframes[1:]:
            rel = (inv @ k.estimate).astype(np.float32)
            corner_local.append(transform_cloud(k.corner_cloud, rel))
            surf_local.append(transform_cloud(k.surf_cloud, rel))
        corner_local = np.concatenate(corner_local)
        surf_local = np.concatenate(surf_local)
        new_relative = (inv @ new_keyframe.estimate).astype(np.float32)
        ok, coarse = self.coarse_matcher(surf_local, new_keyframe.surf_cloud, new_relative.copy())
        if not ok:
            return None
        converged, guess2 = self.scan_match.scanMatchLocal(corner_local, surf_local, new_keyframe.corner_cloud,
                                                           new_keyframe.surf_cloud,
                                                           np.asarray(coarse, np.float32).reshape(4, 4))
        if not converged:
            return None
        self.last_loop_accum_distance = new_keyframe.accum_distance
        return Loop(candidate_keyframes[0], new_keyframe, guess2)

    def _matching_nearest_stored(self, store, candidate_keyframes, new_keyframe, inv):
        """The rest of :meth:`matching_nearest` for keyframes whose clouds are in a KeyframeStore: one call
        (``lslam_kfs_loop_match``), no cloud crosses PCIe.  Same kernels in the same order as the host path: same result."""
        from .capi import Status
        from .keyframe_store import MATCH_FAILED, LOOP_ACCEPTED
        rel = np.stack([(inv @ k.estimate).astype(np.float32) for k in candidate_keyframes])
        new_relative = (inv @ new_keyframe.estimate).astype(np.float32)
        sm = self.scan_match
        r = store.loop_match([k.store_id for k in candidate_keyframes], rel, new_keyframe.store_id, new_relative, sm.opts)
        if r["stage"] >= MATCH_FAILED:  # scanMatchScan ran: ScanMatch's counters move as they do on the host path
            sm._resident, sm._resident_map = None, 0
            sm._finish(Status(r["stats"].status), r["stats"])
        if r["stage"] != LOOP_ACCEPTED:
            return None
        self.last_loop_accum_distance = new_keyframe.accum_distance
        return Loop(candidate_keyframes[0], new_keyframe, r["guess"], [k.store_id for k in candidate_keyframes], rel)
