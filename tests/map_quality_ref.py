"""numpy restatement of the map-quality semantics of include/lslam_c.h (lslam_mapq_*, csrc/lslam_mapq.hip) and of the
trajectory evaluation (lslam_traj_*, csrc/lslam_traj.hip; map_evaluation/Evaluation.cpp:39-150).

Map quality: brute-force neighbours with the survey extractor's fp32 distance rule, the nine sums as int64 in units of 2^-16 m,
the fixed fp64 tail (covariance, ten Jacobi sweeps with the survey reference's _rotate, sort, floor, three logarithms), and the
aggregates as integer sums.  The trajectory evaluation is written twice: literally as the reference's loops (its ring of fixes
included) and vectorised.  The scenes the GPU tests use are made here, so that test_map_quality_ref.py can check their
conditions on the reference alone."""
import functools

import numpy as np

from survey_map_ref import JACOBI_SWEEPS, _rotate, d2_f32, radius2

F = np.float32
ENTROPY_CONST = 4.2568155996140185  # 1.5 * ln(2 pi e), the header's literal
DEFAULTS = dict(radius=0.3, min_neighbors=5, lambda_floor=1e-8)


def eigenvalues(a00, a01, a02, a11, a12, a22):
    """Ten cyclic Jacobi sweeps (the device's sv_rotate through survey_map_ref._rotate) -> the diagonal, sorted ascending."""
    m = len(a00)
    v0, v1, v2 = (np.tile(np.eye(3)[k], (m, 1)) for k in range(3))
    with np.errstate(all="ignore"):
        for _ in range(JACOBI_SWEEPS):
            a00, a11, a01, a02, a12, v0, v1 = _rotate(a00, a11, a01, a02, a12, v0, v1)
            a00, a22, a02, a01, a12, v0, v2 = _rotate(a00, a22, a02, a01, a12, v0, v2)
            a11, a22, a12, a01, a02, v1, v2 = _rotate(a11, a22, a12, a01, a02, v1, v2)
    return np.sort(np.stack([a00, a11, a22], 1), axis=1)


def neighbour_sums(surface, queries, radius, chunk=128):
    """Per query (all finite): the neighbour count and the nine int64 sums over the finite surface points."""
    s32 = np.asarray(surface, F)[:, :3]
    s32 = s32[np.all(np.isfinite(s32), axis=1)]
    q32 = np.asarray(queries, F)[:, :3]
    r2 = radius2(radius)
    s64 = s32.astype(np.float64)
    count = np.zeros(len(q32), np.int64)
    sums = np.zeros((len(q32), 9), np.int64)
    for a in range(0, len(q32), chunk):
        q = q32[a:a + chunk]
        inside = d2_f32(s32, q).T < r2 if len(s32) else np.zeros((len(q), 0), bool)  # p - q, as the header writes it
        D = np.rint((s64[None, :, :] - q.astype(np.float64)[:, None, :]) * 65536.0).astype(np.int64)
        D = D * inside[:, :, None]
        X, Y, Z = D[:, :, 0], D[:, :, 1], D[:, :, 2]
        count[a:a + chunk] = inside.sum(1)
        sums[a:a + chunk] = np.stack([X.sum(1), Y.sum(1), Z.sum(1), (X * X).sum(1), (X * Y).sum(1), (X * Z).sum(1), (Y * Y).sum(1),
                                      (Y * Z).sum(1), (Z * Z).sum(1)], 1)
    return count, sums


def evaluate(surface, queries=None, radius=0.3, min_neighbors=5, lambda_floor=1e-8):
    """-> (stats dict, lambda3 (nq, 3), entropy (nq,), count (nq,) int32) as lslam_mapq_eval gives them."""
    surface = np.asarray(surface, F)[:, :3]
    q = surface if queries is None else np.asarray(queries, F)[:, :3]
    nq = len(q)
    finite = np.all(np.isfinite(q), axis=1) if nq else np.zeros(0, bool)
    lam = np.full((nq, 3), np.nan)
    ent = np.full(nq, np.nan)
    cnt = np.zeros(nq, np.int32)
    pv = np.full(nq, np.nan)
    k, sums = neighbour_sums(surface, q[finite], radius)
    cnt[finite] = k
    ok = k >= min_neighbors
    if ok.any():
        K = k[ok].astype(np.float64)
        s = sums[ok].astype(np.float64)
        s[:, :3] *= 2.0 ** -16
        s[:, 3:] *= 2.0 ** -32
        mx, my, mz = s[:, 0] / K, s[:, 1] / K, s[:, 2] / K
        l = eigenvalues(s[:, 3] / K - mx * mx, s[:, 4] / K - mx * my, s[:, 5] / K - mx * mz, s[:, 6] / K - my * my, s[:, 7] / K - my * mz,
                        s[:, 8] / K - mz * mz)
        lf = np.maximum(l, lambda_floor)
        h = 0.5 * ((np.log(lf[:, 0]) + np.log(lf[:, 1])) + np.log(lf[:, 2])) + ENTROPY_CONST
        idx = np.nonzero(finite)[0][ok]
        lam[idx], ent[idx], pv[idx] = l, h, np.maximum(l[:, 0], 0.0)
    defined = np.isfinite(ent)
    n_def = int(defined.sum())
    sh = int(np.rint(ent[defined] * 2.0 ** 32).astype(np.int64).sum())
    sv = int(np.rint(pv[defined] * 2.0 ** 30).astype(np.int64).sum())
    sk = int(cnt[defined].astype(np.int64).sum())
    nan = float("nan")
    st = dict(n_surface=int(np.all(np.isfinite(surface), axis=1).sum()) if len(surface) else 0, n_query=nq,
              n_nonfinite=int(nq - finite.sum()), n_sparse=int(finite.sum() - n_def), n_defined=n_def, sum_entropy_q32=sh,
              sum_plane_var_q30=sv, sum_neighbors=sk, max_neighbors=int(cnt[defined].max()) if n_def else 0,
              mean_entropy=(float(sh) / 2.0 ** 32) / n_def if n_def else nan,
              mean_plane_variance=(float(sv) / 2.0 ** 30) / n_def if n_def else nan,
              mean_neighbors=float(sk) / n_def if n_def else nan)
    return st, lam, ent, cnt


def transform_f32(cloud, T):
    """((T0 x + T1 y) + T2 z) + T3 per row in fp32: keyframe_store_ref.local_cloud's formula for one cloud -> (n, 3)."""
    from keyframe_store_ref import local_cloud
    c = np.zeros((len(cloud), 4), F)
    c[:, :3] = np.asarray(cloud, F)[:, :3]
    T = np.asarray(T, F).reshape(4, 4)
    return local_cloud([np.zeros((0, 4), F), c], np.stack([np.eye(4, dtype=F), T]))[:, :3]


# ---- trajectory evaluation ---------------------------------------------------------------------------------------------------
def traj_literal(est_stamp, est_xyz, ref_stamp, ref_xyz, gate=10.0, store_num=None):
    """Evaluation.cpp as written: gpsHandler for every fix into the ring, then lidarToMapHandler per estimate, then process()'s
    sums.  ``store_num``: the ring's size (the reference: 1000; None: room for every fix, what lslam_traj_eval does)."""
    est_stamp, ref_stamp = np.asarray(est_stamp, np.float64), np.asarray(ref_stamp, np.float64)
    est_xyz, ref_xyz = np.asarray(est_xyz, np.float64).reshape(-1, 3), np.asarray(ref_xyz, np.float64).reshape(-1, 3)
    N = max(len(ref_stamp), 1) if store_num is None else int(store_num)
    gx, gy, gz, gt = np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N)
    now_id, msg_num = 0, 0
    for j in range(len(ref_stamp)):  # gpsHandler, :27-37
        gx[now_id], gy[now_id], gz[now_id], gt[now_id] = ref_xyz[j, 0], ref_xyz[j, 1], ref_xyz[j, 2], ref_stamp[j]
        now_id = (now_id + 1) % N
        msg_num = min(msg_num + 1, N)
    dX, dY, dZ, dD, dT, pairs = [], [], [], [], [], []
    mx = [0.0, 0.0, 0.0, 0.0]
    gated = 0
    sqrt = lambda v: float(np.sqrt(np.float64(v)))
    for i in range(len(est_stamp) if msg_num else 0):  # lidarToMapHandler, :39-79
        now = float(est_stamp[i])
        dt, cor = -1.0, -1
        tmp = (now_id + N - 1) % N
        for k in range(msg_num):
            if k == 0 or dt > abs(now - gt[tmp]):
                dt, cor = abs(now - gt[tmp]), tmp
            else:
                break
            tmp = (tmp + N - 1) % N
        x, y, z = abs(est_xyz[i, 0] - gx[cor]), abs(est_xyz[i, 1] - gy[cor]), abs(est_xyz[i, 2] - gz[cor])
        d = sqrt(x * x + y * y + z * z)
        mx = [max(mx[0], x), max(mx[1], y), max(mx[2], z), max(mx[3], d)]
        if gate == 0.0 or d <= gate:
            dX.append(x), dY.append(y), dZ.append(z), dD.append(d), dT.append(dt)
            pairs.append((est_xyz[i].copy(), np.array([gx[cor], gy[cor], gz[cor]])))
        else:
            gated += 1
    num = len(dX)
    nan = float("nan")
    mean, var = [], []
    for col in (dX, dY, dZ, dD):  # process(), :107-131
        m = 0.0
        for v in col:
            m += v
        m = m / num if num else nan
        s = 0.0
        for v in col:
            s += (v - m) * (v - m)
        mean.append(m)
        var.append(s / (num - 1) if num >= 2 else nan)
    mt = 0.0
    for v in dT:
        mt += v
    return dict(n_used=num, n_gated=gated, mean=np.array(mean), var=np.array(var), max=np.array(mx), mean_dt=mt / num if num else nan,
                pairs=pairs)


def traj_vectorised(est_stamp, est_xyz, ref_stamp, ref_xyz, gate=10.0):
    """The same figures from array operations: nearest reference by searchsorted (a tie to the later sample)."""
    es, rs = np.asarray(est_stamp, np.float64), np.asarray(ref_stamp, np.float64)
    ex, rx = np.asarray(est_xyz, np.float64).reshape(-1, 3), np.asarray(ref_xyz, np.float64).reshape(-1, 3)
    hi = np.clip(np.searchsorted(rs, es, side="left"), 0, len(rs) - 1)
    lo = np.clip(hi - 1, 0, len(rs) - 1)
    cor = np.where(np.abs(es - rs[lo]) < np.abs(es - rs[hi]), lo, hi)  # (stamps strictly ascending: the scan's first minimum is the nearest)
    d = np.abs(ex - rx[cor])
    dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    cols = np.concatenate([d, dist[:, None]], 1)
    use = np.ones(len(es), bool) if gate == 0.0 else dist <= gate
    u = cols[use]
    num = len(u)
    with np.errstate(all="ignore"):
        mean = u.sum(0) / num if num else np.full(4, np.nan)
        var = ((u - mean) ** 2).sum(0) / (num - 1) if num >= 2 else np.full(4, np.nan)
    return dict(n_used=num, n_gated=int(len(es) - num), mean=mean, var=var, max=cols.max(0) if len(cols) else np.zeros(4),
                mean_dt=float(np.abs(es - rs[cor])[use].sum() / num) if num else float("nan"))


def align(est, ref):
    """Kabsch through numpy's SVD -> (aligned, R, t, ate_rmse, s) with s the singular values of H = sum e_c r_c^T; aligned is
    False for fewer than three pairs or s[1] <= 1e-6 s[0] (the header's rule)."""
    e, r = np.asarray(est, np.float64).reshape(-1, 3), np.asarray(ref, np.float64).reshape(-1, 3)
    if len(e) < 3:
        return False, np.eye(3), np.zeros(3), float("nan"), np.zeros(3)
    ce, cr = e.mean(0), r.mean(0)
    H = (e - ce).T @ (r - cr)
    U, s, Vt = np.linalg.svd(H)
    if not (s[0] > 0.0 and s[1] > 1e-6 * s[0]):
        return False, np.eye(3), np.zeros(3), float("nan"), s
    dgn = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ dgn @ U.T
    t = cr - R @ ce
    res = (R @ e.T).T + t - r
    return True, R, t, float(np.sqrt((res * res).sum() / len(e))), s


# ---- scenes --------------------------------------------------------------------------------------------------------------------
def wall_with_floor(seed=1, n_wall=1400, n_floor=900, sigma=0.01):
    """A noisy wall x = 2 over a floor z = 0, and a few stray points far from both (sparse)."""
    rng = np.random.default_rng(seed)
    wall = np.stack([2.0 + rng.normal(0, sigma, n_wall), rng.uniform(-2, 2, n_wall), rng.uniform(0, 2, n_wall)], 1)
    floor = np.stack([rng.uniform(-1, 2, n_floor), rng.uniform(-2, 2, n_floor), rng.normal(0, sigma, n_floor)], 1)
    stray = rng.uniform(8, 30, (12, 3))
    return np.concatenate([wall, floor, stray]).astype(F)


def uniform_box(seed=2, n=2500):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-1, 1, (n, 3)), np.array([[9.0, 9.0, 9.0]])]).astype(F)


def lattice(step=0.1, m=9, far=True):
    """An m^3 lattice of spacing ``step`` (fp32): at radius 3 * step many neighbours lie exactly on the radius, up to rounding --
    the strict < decides -- and with the cell edge r (1 + 1/1024) points sit on or beside cell faces."""
    g = np.arange(m, dtype=np.float64) * step
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    if far:
        p = np.concatenate([p, [[50.0, 50.0, 50.0]]])
    return p.astype(F)


def duplicates(seed=3, n=600):
    rng = np.random.default_rng(seed)
    base = rng.uniform(-0.6, 0.6, (n, 3)).astype(F)
    return np.concatenate([base, base[: n // 2], base[: n // 4], np.array([[7, 7, 7]], F)]).astype(F)


def exact_plane(m=40, step=2.0 ** -5):
    """Points exactly in the plane z = 0.5 (coordinates exact in fp32): l0 is exactly 0 and the floor engages."""
    g = np.arange(m, dtype=np.float64) * step
    p = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    p = np.concatenate([p, np.full((len(p), 1), 0.5)], 1)
    return np.concatenate([p, [[20.0, 0.0, 0.5]]]).astype(F)


def exact_line(n=400, step=2.0 ** -6):
    """Points exactly on a line along x: two eigenvalues are floored."""
    p = np.zeros((n, 3))
    p[:, 0] = np.arange(n) * step
    p[:, 1], p[:, 2] = 0.25, -0.5
    return np.concatenate([p, [[40.0, 0.25, -0.5]]]).astype(F)


ACCURACY_SCENES = {
    "wall_floor": (wall_with_floor, dict(radius=0.3)),
    "box": (uniform_box, dict(radius=0.3)),
    "lattice": (lattice, dict(radius=np.float32(0.3))),
    "duplicates": (duplicates, dict(radius=0.25)),
    "plane": (exact_plane, dict(radius=0.1)),
    "line": (exact_line, dict(radius=0.1)),
}


@functools.lru_cache(maxsize=None)
def scene_reference(name):
    """-> (cloud, params, (stats, lambda3, entropy, count)) of an accuracy scene, computed once per session."""
    make, params = ACCURACY_SCENES[name]
    cloud = make()
    return cloud, dict(params), evaluate(cloud, **params)


def two_walls(gap, seed=5, n=1500, sigma=0.01):
    """Two walls of noise sigma, ``gap`` apart along their normal (0: coincident)."""
    rng = np.random.default_rng(seed)
    walls = []
    for k in range(2):
        walls.append(np.stack([k * gap + rng.normal(0, sigma, n), rng.uniform(-1.5, 1.5, n), rng.uniform(0, 1.5, n)], 1))
    return np.concatenate(walls).astype(F)


def keyframe_scene(seed=7, n_wall=500, n_floor=250, sigma=0.01, shift=0.2):
    """Four keyframes that see one wall (y = 3 in the graph frame) and a floor patch from four positions.  -> (clouds in the
    sensor frames [(n, 4) float32], true poses [4x4 float64], poses with keyframe 1 displaced by ``shift`` along the wall
    normal).  A quarter of the wall points then lie shift off the others: planted variance f (1 - f) shift^2."""
    rng = np.random.default_rng(seed)
    clouds, poses = [], []
    for k in range(4):
        yaw = 0.15 * k - 0.2
        T = np.eye(4)
        T[:3, :3] = [[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]]
        T[:3, 3] = [0.5 * k - 0.75, 0.1 * k * k, 0.4]  # (not on a line: a trajectory alignment has something to hold on to)
        wall = np.stack([rng.uniform(-2, 2, n_wall), 3.0 + rng.normal(0, sigma, n_wall), rng.uniform(0, 1.5, n_wall)], 1)
        floor = np.stack([rng.uniform(-2, 2, n_floor), rng.uniform(0, 2.5, n_floor), rng.normal(0, sigma, n_floor)], 1)
        world = np.concatenate([wall, floor])
        local = (world - T[:3, 3]) @ T[:3, :3]  # R^T (p - t)
        c = np.zeros((len(local), 4), F)
        c[:, :3] = local
        clouds.append(c)
        poses.append(T)
    moved = [p.copy() for p in poses]
    moved[1][1, 3] += shift
    return clouds, poses, moved


def assemble(clouds, poses):
    return np.concatenate([transform_f32(c, np.asarray(T, np.float64).astype(F)) for c, T in zip(clouds, poses)])
