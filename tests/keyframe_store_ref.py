"""numpy restatement of the keyframe store's candidate assembly (csrc/lslam_kfs.hip kfs_gather_kernel;
pose_graph/loop_detector.hpp:166-200): candidate 0's cloud as it is, bit for bit; candidates 1 .. n-1 transformed by their
4x4 ``rel`` as pcl::transformPointCloud does -- x' = ((T0 x + T1 y) + T2 z) + T3, left to right in fp32, every product and sum
rounded on its own, intensity kept -- and appended in candidate order."""
import numpy as np


def local_cloud(clouds, rel_T):
    """clouds: one (n_k, 4) float32 array per candidate; rel_T: (n, 4, 4) float32 (rel_T[0] is not read) -> (sum n_k, 4)."""
    total = sum(len(c) for c in clouds)
    out = np.empty((total, 4), np.float32)
    at = 0
    for k, c in enumerate(clouds):
        c = np.ascontiguousarray(c, np.float32).reshape(-1, 4)
        dst = out[at:at + len(c)]
        if k == 0:
            dst.view(np.uint32)[:] = c.view(np.uint32)  # the bits: -0.0 stays -0.0, a NaN keeps its payload
        else:
            T = np.asarray(rel_T[k], np.float32)
            x, y, z = c[:, 0], c[:, 1], c[:, 2]
            for r in range(3):
                p0, p1, p2 = T[r, 0] * x, T[r, 1] * y, T[r, 2] * z  # fp32 arrays: each product rounded to fp32
                dst[:, r] = ((p0 + p1) + p2) + T[r, 3]
            dst.view(np.uint32)[:, 3] = c.view(np.uint32)[:, 3]
        at += len(c)
    return out


def local_clouds(corner_clouds, surf_clouds, rel_T):
    return local_cloud(corner_clouds, rel_T), local_cloud(surf_clouds, rel_T)


def random_se3(rng, max_t=5.0):
    """A general rigid transform as float32 4x4 (rotation by QR of a Gaussian matrix, made proper)."""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    T = np.eye(4)
    T[:3, :3] = q
    T[:3, 3] = rng.uniform(-max_t, max_t, 3)
    return T.astype(np.float32)
