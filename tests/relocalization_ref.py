"""Restatement in numpy of the global re-localisation stage of the localisation node (include/lslam_c.h, "global
re-localisation"): the occupancy sets of the map a ``localization_ref.RefLocalization`` holds, the hypothesis score, the top-M
selection, the greedy non-maximum suppression and the refinement by ``ref.match``.  Every fp32 operation is rounded on its own,
as the device kernels do it.  tests/test_gpu_relocalization.py holds the device stage against this file."""
import numpy as np

import localization_ref as lr

F = np.float32
IDX_LIM = 1 << 20  # voxel indices live in [-2^20, 2^20)
OK, NOT_CONVERGED, TOO_FEW_MATCHES = 0, 2, 5


def inv_of(voxel):
    return F(1.0) / F(2.0 if voxel == 0 else voxel)


def voxel_keys(xyz, inv):
    """floor(x * inv) per axis in fp32 -> (packed int64 key, valid).  A point with a non-finite or out-of-range index has no voxel."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((xyz * F(inv)).astype(F))
        ok = np.all((f >= -IDX_LIM) & (f < IDX_LIM), axis=1)  # false for NaN and the infinities
    i = np.where(ok[:, None], f, 0).astype(np.int64) + IDX_LIM
    return (i[:, 0] << 42) | (i[:, 1] << 21) | i[:, 2], ok


def occupancy_sets(ref, voxel):
    """Per feature type the sorted array of occupied voxel keys of the map the restatement holds."""
    inv = inv_of(voxel)
    out = []
    for t in range(2):
        k, ok = voxel_keys(ref.map[t][:, :3], inv)
        out.append(np.unique(k[ok]))
    return out


def occupied(sets, which, xyz, voxel):
    k, ok = voxel_keys(xyz, inv_of(voxel))
    return (ok & np.isin(k, sets[which])).astype(np.uint8)


def subsample(cloud, max_points):
    n = len(cloud)
    if max_points > 0 and n > max_points:
        return cloud[::-(-n // max_points)]
    return cloud


def edge_refused(ref, positions):
    """The rule of lslam_loc_process: the sensor cube within 3 cubes of the cube array's edge."""
    g = lr.cube_index(np.asarray(positions, F).reshape(-1, 3), ref.cube_size, ref.origin)
    dims = np.asarray(ref.dims)
    return np.any((g < 3) | (g > dims - 4), axis=1)


def scores(ref, corner, surf, Rs, positions, voxel=2.0, max_points=0, sets=None):
    """corner / surf: the RAW sweep (the scan filters are applied here).  Rs: (n_rot, 3, 3) float32.  -> (n_rot, n_pos) int32,
    -1 for a refused position; and the filtered point counts."""
    sets = occupancy_sets(ref, voxel) if sets is None else sets
    inv = inv_of(voxel)
    c, s = ref.prepare_frame(corner, surf)
    clouds = [subsample(np.asarray(c, F)[:, :3], max_points), subsample(np.asarray(s, F)[:, :3], max_points)]
    positions = np.asarray(positions, F).reshape(-1, 3)
    Rs = np.asarray(Rs, F).reshape(-1, 3, 3)
    refused = edge_refused(ref, positions)
    live = np.flatnonzero(~refused)
    out = np.zeros((len(Rs), len(positions)), np.int32)
    for r, R in enumerate(Rs):
        for t in range(2):
            p = clouds[t]
            if len(p) == 0:
                continue
            x, y, z = p[:, 0], p[:, 1], p[:, 2]
            with np.errstate(invalid="ignore", over="ignore"):
                rot = np.stack([((R[a, 0] * x).astype(F) + (R[a, 1] * y).astype(F)).astype(F) + (R[a, 2] * z).astype(F) for a in range(3)], 1).astype(F)
                for j0 in range(0, len(live), 128):
                    jj = live[j0:j0 + 128]
                    k, ok = voxel_keys((rot[None, :, :] + positions[jj][:, None, :]).astype(F).reshape(-1, 3), inv)
                    out[r, jj] += (ok & np.isin(k, sets[t])).reshape(len(jj), len(p)).sum(1).astype(np.int32)
    out[:, refused] = -1
    return out, (len(c), len(s))


def top_m(score, m):
    """Hypothesis indices by score descending then index ascending, -1 never selected -> (idx, score)."""
    flat = np.asarray(score, np.int64).ravel()
    idx = np.flatnonzero(flat >= 0)
    order = idx[np.lexsort((idx, -flat[idx]))][:m]
    return order.astype(np.int32), flat[order].astype(np.int32)


def nms(top_idx, positions, n_rot, nms_m=2.0, nms_rot=2, cyclic=False, max_candidates=8):
    """Greedy, in the list's order -> positions in the list of the survivors."""
    positions = np.asarray(positions, F).reshape(-1, 3)
    n_pos = len(positions)
    keep = []
    for i, h in enumerate(top_idx):
        if len(keep) >= max_candidates:
            break
        r, p = int(h) // n_pos, positions[int(h) % n_pos]
        dropped = False
        for k in keep:
            rk, pk = int(top_idx[k]) // n_pos, positions[int(top_idx[k]) % n_pos]
            dr = abs(r - rk)
            if cyclic:
                dr = min(dr, n_rot - dr)
            if np.abs(p - pk).max() <= F(nms_m) and dr <= nms_rot:
                dropped = True
                break
        if not dropped:
            keep.append(i)
    return np.asarray(keep, np.int32)


def refine(ref, corner, surf, pose, rounds=3):
    """ref.match repeated from its own result while it did not converge -> (status, pose, n_rows, rounds run)."""
    pose = np.asarray(pose, F).copy()
    status, n_rows, k = NOT_CONVERGED, 0, 0
    while k < rounds and status == NOT_CONVERGED:
        ok, pose, st = ref.match(corner, surf, pose)
        k += 1
        n_rows = int(st.n_rows)
        status = OK if ok else (TOO_FEW_MATCHES if n_rows < 50 else NOT_CONVERGED)
    return status, np.asarray(pose, F), n_rows, k
