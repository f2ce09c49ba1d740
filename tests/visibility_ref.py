"""numpy restatement of the visibility-vote specification of include/lslam_c.h ("visibility votes"): the pixel of a point in
the specified arithmetic (float32 arrays for the fp32 steps, every operation rounded on its own; float64 arctan2 for the
bins), the range image as a minimum per pixel, the free / hit votes as integers.  No code shared with the kernels."""
import copy

import numpy as np

TWO_PI = 2.0 * np.pi
F = np.float32
DEFAULTS = dict(n_row=16, n_col=360, fov_down_deg=-16.0, fov_up_deg=16.0, min_range=1.0, max_range=80.0, window=1,
                abs_margin=0.5, rel_margin=0.02, min_free_votes=2, up_axis=1)


def params(**kw):
    p = dict(DEFAULTS)
    for k in kw:
        if k not in DEFAULTS:
            raise TypeError("unknown parameter %r" % k)
    p.update(kw)
    return p


def scales(p):
    """el0, row_scale, col_scale: float64 from the float32 parameters."""
    down, up = np.float64(F(p["fov_down_deg"])), np.float64(F(p["fov_up_deg"]))
    el0 = down * np.pi / 180.0
    row_scale = np.float64(p["n_row"]) / ((up - down) * np.pi / 180.0)
    return el0, row_scale, np.float64(p["n_col"]) / TWO_PI


def _xyz(points):
    c = np.asarray(points, F)
    return c.reshape(-1, c.shape[-1])[:, :3] if c.size else np.zeros((0, 3), F)


def project(xyz, p):
    """Points in a sensor frame -> dict: obs (observable), gate (finite and inside the range gate), r (float32), row, col,
    rowd, cold (the float64 values whose integer parts the bins are)."""
    xyz = _xyz(xyz)
    finite = np.isfinite(xyz).all(axis=1)
    s = np.where(finite[:, None], xyz, F(1))
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    a, b, h = (z, x, y) if p["up_axis"] == 1 else (x, y, z)
    with np.errstate(all="ignore"):
        d2 = a * a + b * b
        rho = np.sqrt(d2)
        r = np.sqrt(d2 + h * h)
    assert d2.dtype == F and r.dtype == F
    gate = finite & (r >= F(p["min_range"])) & (r <= F(p["max_range"]))
    el0, row_scale, col_scale = scales(p)
    rowd = (np.arctan2(h.astype(np.float64), rho.astype(np.float64)) - el0) * row_scale
    obs = gate & (rowd >= 0.0) & (rowd < p["n_row"])
    row = np.where(obs, rowd, 0.0).astype(np.int64)
    ang = np.arctan2(b.astype(np.float64), a.astype(np.float64))
    ang = np.where(ang < 0, ang + TWO_PI, ang)
    cold = ang * col_scale
    col = np.minimum(cold.astype(np.int64), p["n_col"] - 1)
    return dict(obs=obs, gate=gate, r=r, row=row, col=col, rowd=rowd, cold=cold)


def range_image(corner, surf, p):
    """(n_row, n_col) float32 over the corner cloud followed by the surf cloud: the minimum r per pixel, +inf without one."""
    img = np.full((p["n_row"], p["n_col"]), np.inf, F)
    for cloud in (corner, surf):
        q = project(cloud, p)
        o = q["obs"]
        np.minimum.at(img, (q["row"][o], q["col"][o]), q["r"][o])
    return img


def inverse_pose(T):
    """(R^T, -R^T t) in float64 from the float32 pose, rounded to float32 -> (3, 4)."""
    T = np.asarray(T, F).reshape(4, 4).astype(np.float64)
    out = np.zeros((3, 4), np.float64)
    for j in range(3):
        r0, r1, r2 = T[0, j], T[1, j], T[2, j]
        out[j, :3] = (r0, r1, r2)
        out[j, 3] = -((r0 * T[0, 3] + r1 * T[1, 3]) + r2 * T[2, 3])
    return out.astype(F)


def transform(M, xyz):
    """((M0 x + M1 y) + M2 z) + M3 per row in float32; M: the first three rows of a pose."""
    M = np.asarray(M, F).reshape(-1)[:12].reshape(3, 4)
    xyz = _xyz(xyz)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        out = np.stack([((M[j, 0] * x + M[j, 1] * y) + M[j, 2] * z) + M[j, 3] for j in range(3)], axis=1)
    assert out.dtype == F
    return out


def vote(image, pose, points, p):
    """One voter -> (free, hit) boolean arrays over the points (graph frame)."""
    q = project(transform(inverse_pose(pose), points), p)
    obs, r, row, col = q["obs"], q["r"], q["row"], q["col"]
    with np.errstate(all="ignore"):
        m = np.maximum(F(p["abs_margin"]), F(p["rel_margin"]) * r)
        beyond = r + m
    assert m.dtype == F and beyond.dtype == F
    w, R, C = p["window"], p["n_row"], p["n_col"]
    all_beyond, hit = np.ones(len(r), bool), np.zeros(len(r), bool)
    for dr in range(-w, w + 1):
        rr = row + dr
        inside = (rr >= 0) & (rr < R)
        rr = np.clip(rr, 0, R - 1)
        for dc in range(-w, w + 1):
            v = image[rr, (col + dc) % C]
            fin = inside & np.isfinite(v)
            with np.errstate(all="ignore"):
                all_beyond &= ~fin | (v > beyond)
                hit |= fin & (np.abs(v - r) <= m)
    centre = np.isfinite(image[row, col])
    return obs & centre & all_beyond, obs & hit


def votes(images, poses, points, p):
    """Voters (images[k], poses[k]) on points -> the packed words n_free | n_hit << 16, uint32."""
    n = len(_xyz(points))
    nf, nh = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for img, T in zip(images, poses):
        f, h = vote(img, T, points, p)
        nf += f
        nh += h
    return nf | (nh << np.uint32(16))


def dynamic(words, p):
    w = np.asarray(words, np.uint32)
    nf, nh = (w & 0xFFFF).astype(np.int64), (w >> 16).astype(np.int64)
    return (nf >= p["min_free_votes"]) & (nf > nh)


def unambiguous(points, poses, p, margin=1e-9):
    """Mask over the points: False where, for some pose of the call (None: the points are in the sensor frame already), the
    point passes the range gate and its float64 rowd or scaled azimuth lies within ``margin`` of an integer -- there two correct
    fp64 atan2 implementations may choose different bins."""
    xyz = _xyz(points)
    keep = np.ones(len(xyz), bool)
    for T in ([None] if poses is None else poses):
        q = project(xyz if T is None else transform(inverse_pose(T), xyz), p)
        near = (np.abs(q["rowd"] - np.round(q["rowd"])) <= margin) | (np.abs(q["cold"] - np.round(q["cold"])) <= margin)
        keep &= ~(q["gate"] & near)
    return keep


def drop_ambiguous(points, poses, p, margin=1e-9):
    """The points without the ambiguous ones (:func:`unambiguous`), as place_recognition_ref.drop_ambiguous."""
    pts = np.asarray(points, F)
    return pts[unambiguous(pts, poses, p, margin)]


def pose_matrix(pose6):
    """(rx, ry, rz, x, y, z) -> 4x4 float64, R = Rz Ry Rx."""
    rx, ry, rz = pose6[:3]
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rz @ Ry @ Rx, pose6[3:6]
    return T


# ---- the scene of the end-to-end tests: a box that is there for the first two of six keyframes ----------------------------------
SCENE_BOX = (14.0, 18.0, 3.0, 5.0, 1.6)
SCENE_POSES = [(0, 0, .3, 3, -2), (0, 0, .35, 4, -2), (0, 0, .2, 5, -2), (0, 0, .3, 6, -2), (0, 0, .4, 7, -1.5), (0, 0, .25, 8, -2)]
SCENE_BOX_PRESENT = 2
_scene_cache = {}


def scene(synth):
    """-> dict: ``clouds`` [(corner, surf)] per keyframe (sensor frame), ``poses`` (4x4 float32), ``params``, ``query`` (all
    points in the graph frame, float32, keyframe after keyframe, corner then surf), ``owner`` (the keyframe of each query point),
    ``is_box`` (the returns from the box).  Built once per process; nothing in it is modified."""
    if "s" in _scene_cache:
        return _scene_cache["s"]
    world = synth.World(half_extent=60)
    with_box = copy.deepcopy(world)
    with_box.boxes = np.concatenate([with_box.boxes, np.array([SCENE_BOX], np.float64)], axis=0)
    x0, x1, y0, y1, h = SCENE_BOX
    p = params(up_axis=2)
    clouds, poses, query, owner, is_box = [], [], [], [], []
    for i, (rx, ry, rz, x, y) in enumerate(SCENE_POSES):
        gt = (rx, ry, rz, x, y, synth.SENSOR_HEIGHT)
        corner, surf, _ = synth.make_scan(with_box if i < SCENE_BOX_PRESENT else world, rings=16, azimuth_steps=900, gt_pose=gt,
                                          noise_sigma=0.02, seed=10 + i)
        T = pose_matrix(np.asarray(gt, np.float64)).astype(F)
        clouds.append((corner, surf))
        poses.append(T)
        for c in (corner, surf):
            g = transform(T, c)
            query.append(g)
            owner.append(np.full(len(g), i, np.int32))
            w = c[:, :3].astype(np.float64) @ T[:3, :3].astype(np.float64).T + T[:3, 3].astype(np.float64)
            is_box.append((w[:, 0] >= x0 - 0.1) & (w[:, 0] <= x1 + 0.1) & (w[:, 1] >= y0 - 0.1) & (w[:, 1] <= y1 + 0.1) &
                          (w[:, 2] > 0.05) & (w[:, 2] <= h + 0.1) & (i < SCENE_BOX_PRESENT))
    s = dict(clouds=clouds, poses=poses, params=p, query=np.concatenate(query), owner=np.concatenate(owner),
             is_box=np.concatenate(is_box), box=SCENE_BOX)
    s["images"] = [range_image(c, sf, p) for c, sf in clouds]
    s["votes"] = votes(s["images"], poses, s["query"], p)
    s["keep"] = unambiguous(s["query"], poses, p)
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _scene_cache["s"] = s
    return s
