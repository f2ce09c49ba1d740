"""numpy restatement of the scan-context specification of include/lslam_c.h ("loop candidates by appearance"): the descriptor
in the specified arithmetic (fp32 with every operation rounded on its own, the sector in fp64), the distances in float64."""
import numpy as np

TWO_PI = 2.0 * np.pi


def params(**kw):
    p = dict(n_ring=20, n_sector=60, max_range=80.0, height_offset=2.0, up_axis=1)
    p.update(kw)
    return p


def tol(p):
    """The bound the header states for a distance against its float64 evaluation."""
    return (p["n_ring"] + p["n_sector"] + 8) * 2.0 ** -23


def _abh(cloud, up_axis):
    c = np.asarray(cloud, np.float32).reshape(-1, 4)
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    return (z, x, y) if up_axis == 1 else (x, y, z)


def _cells(cloud, p):
    """-> keep mask over the cloud's points, ring, float64 ang * sector_scale, value (all over the kept points)."""
    a, b, h = _abh(cloud, p["up_axis"])
    finite = np.isfinite(a) & np.isfinite(b) & np.isfinite(h)
    with np.errstate(all="ignore"):
        a0, b0 = np.where(finite, a, np.float32(1)), np.where(finite, b, np.float32(1))
        d2 = a0 * a0 + b0 * b0
        rho = np.sqrt(d2)
        ring_scale = np.float32(p["n_ring"]) / np.float32(p["max_range"])
        keep = finite & (rho != 0) & (rho < np.float32(p["max_range"]))
        ring = np.where(keep, rho * ring_scale, np.float32(0)).astype(np.int32)
    keep &= ring < p["n_ring"]
    ang = np.arctan2(b0.astype(np.float64), a0.astype(np.float64))
    ang = np.where(ang < 0, ang + TWO_PI, ang)
    scaled = ang * (p["n_sector"] / TWO_PI)
    with np.errstate(all="ignore"):
        v = np.where(finite, h, np.float32(0)) + np.float32(p["height_offset"])
    return keep, ring, scaled, v


def descriptor(corner, surf, p):
    """D[ring][sector] float32 over the corner cloud followed by the surf cloud."""
    D = np.zeros((p["n_ring"], p["n_sector"]), np.float32)
    for cloud in (corner, surf):
        cloud = np.asarray(cloud, np.float32).reshape(-1, 4)
        if not len(cloud):
            continue
        keep, ring, scaled, v = _cells(cloud, p)
        sector = np.minimum(scaled.astype(np.int64), p["n_sector"] - 1)
        keep &= v > 0
        np.maximum.at(D, (ring[keep], sector[keep]), v[keep])
    return D


def drop_ambiguous(cloud, p, margin=1e-9):
    """The cloud without the points whose float64 ``ang * sector_scale`` lies within ``margin`` of an integer: there two
    correct fp64 atan2 implementations may put the point into different sectors.  (The ring is exact fp32 arithmetic.)"""
    cloud = np.asarray(cloud, np.float32).reshape(-1, 4)
    if not len(cloud):
        return cloud
    _keep, _ring, scaled, _v = _cells(cloud, p)
    return cloud[np.abs(scaled - np.round(scaled)) > margin]


def shift_distances(Q, C):
    """d(s) for every shift, float64."""
    Q, C = np.asarray(Q, np.float64), np.asarray(C, np.float64)
    S = Q.shape[1]
    nq, nc = np.sqrt((Q * Q).sum(0)), np.sqrt((C * C).sum(0))
    out = np.ones(S)
    for s in range(S):
        Cs, ncs = np.roll(C, -s, axis=1), np.roll(nc, -s)  # Cs[:, j] = C[:, (j + s) mod S]
        ok = (nq > 0) & (ncs > 0)
        if ok.any():
            cos = (Q[:, ok] * Cs[:, ok]).sum(0) / (nq[ok] * ncs[ok])
            out[s] = max(0.0, 1.0 - cos.mean())
    return out


def distance(Q, C):
    """-> (min_s d(s), the smallest s attaining it), float64."""
    d = shift_distances(Q, C)
    s = int(np.argmin(d))
    return float(d[s]), s


def yaw_shift(psi, n_sector):
    return int(np.round(psi / (TWO_PI / n_sector))) % n_sector


def rotate_about_up(cloud, psi, up_axis):
    """The cloud seen from a sensor rotated by psi about the up axis at the same place: p_q = R(-psi) p_c (float64, rounded
    once)."""
    c = np.asarray(cloud, np.float64).copy()
    ia, ib = (2, 0) if up_axis == 1 else (0, 1)
    a, b = c[:, ia].copy(), c[:, ib].copy()
    cs, sn = np.cos(psi), np.sin(psi)
    c[:, ia] = cs * a + sn * b
    c[:, ib] = -sn * a + cs * b
    return c.astype(np.float32)
