"""2D occupancy grid from the keyframe store (``csrc/lslam_occ.hip``, ``lslam_occ_*`` of include/lslam_c.h): every point of
every keyframe is a ray from the sensor to the point; the cells it crosses were seen free, the cell it ends in -- at obstacle
height above the keyframe's floor plane -- was seen occupied.  Integer votes per keyframe and cell, so the result is
reproducible to the bit.  The header states the semantics completely; ``tests/occupancy_ref.py`` restates them in numpy and
Python integers.

The functions here are what :class:`KeyframeStore`'s ``occ_*`` methods call, plus :func:`save_map`, which writes the grid as
the ``.pgm`` / ``.yaml`` pair ``map_server`` loads.
"""
import ctypes as C
import os

import numpy as np

from .capi import LslamError, LslamOccParams, LslamOccStats, c_float_p, c_int32_p, load_library

PARAM_FIELDS = ("resolution", "width", "height", "up_axis", "min_range", "max_range", "obstacle_min", "obstacle_max",
                "ground_band", "sensor_height", "ground_clears", "hit_weight", "min_observations")
RAY_TILE, KF_CHUNK = 256, 8  # LSLAM_OCC_RAY_TILE, LSLAM_OCC_KF_CHUNK
OCCUPIED_THRESH, FREE_THRESH = 0.65, 0.196  # map_saver's


def occ_params(params=None, **kw):
    """-> :class:`LslamOccParams`: the library's defaults, then ``params`` (a dict or an LslamOccParams), then ``kw``;
    ``origin`` is a pair."""
    p = LslamOccParams()
    load_library().lslam_occ_default_params(C.byref(p))
    if isinstance(params, LslamOccParams):
        C.memmove(C.byref(p), C.byref(params), C.sizeof(p))
        params = None
    for k, v in dict(params or {}, **kw).items():
        if k == "origin":
            p.origin[0], p.origin[1] = float(v[0]), float(v[1])
        elif k in PARAM_FIELDS:
            setattr(p, k, v)
        else:
            raise TypeError("occ_params: unknown parameter %r" % k)
    return p


def params_dict(p):
    out = {k: getattr(p, k) for k in PARAM_FIELDS}
    out["origin"] = (p.origin[0], p.origin[1])
    return out


def split_counts(counts):
    """The packed words ``n_free | n_hit << 16`` -> (n_free, n_hit) int32 arrays."""
    v = np.asarray(counts, np.uint32)
    return (v & 0xFFFF).astype(np.int32), (v >> 16).astype(np.int32)


def _check(store, rc):
    if rc < 0:
        raise LslamError(rc, store.lib.lslam_last_error().decode())
    return rc


def fit_bounds(poses, params=None, **kw):
    """``lslam_occ_fit_bounds``: the smallest grid with its origin on multiples of the resolution that holds every pose's
    position +- ``max_range`` -> :class:`LslamOccParams` with ``origin``, ``width`` and ``height`` set.  Host only."""
    p = occ_params(params, **kw)
    T = np.ascontiguousarray(np.asarray(poses, np.float64).astype(np.float32)).reshape(-1, 16)
    lib = load_library()
    rc = lib.lslam_occ_fit_bounds(len(T), T.ctypes.data_as(c_float_p), C.byref(p))
    if rc < 0:
        raise LslamError(rc, lib.lslam_last_error().decode())
    return p


def setup(store, params=None, **kw):
    """``lslam_occ_setup``: install the parameters (``width`` and ``height`` have no default).  Other parameters than those
    in force clear the grid."""
    p = occ_params(params, **kw)
    _check(store, store.lib.lslam_occ_setup(store.h, C.byref(p)))


def info(store):
    st = LslamOccStats()
    _check(store, store.lib.lslam_occ_info(store.h, C.byref(st)))
    out = params_dict(st.params)
    out.update({k: getattr(st, k) for k, _ in LslamOccStats._fields_ if k != "params"})
    out["is_set"] = bool(st.is_set)
    return out


def clear(store):
    _check(store, store.lib.lslam_occ_clear(store.h))


def integrate(store, ids, poses, planes=None, plane_valid=None):
    """Add the votes of keyframes ``ids`` at ``poses`` (4x4 each, graph <- sensor).  ``planes``: (n, 4) float64 floor planes in
    the sensor frame (``floor_detect``'s) or None for the fallback; ``plane_valid``: n flags, 0 -> the fallback."""
    ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
    T = np.ascontiguousarray(np.asarray(poses, np.float64).astype(np.float32)).reshape(len(ids), 16)
    pl = pv = None
    if planes is not None:
        pl = np.ascontiguousarray(planes, np.float64).reshape(len(ids), 4)
        if plane_valid is not None:
            pv = np.ascontiguousarray(plane_valid, np.int32).reshape(len(ids))
    _check(store, store.lib.lslam_occ_integrate(
        store.h, len(ids), ids.ctypes.data_as(c_int32_p), T.ctypes.data_as(c_float_p),
        pl.ctypes.data_as(C.POINTER(C.c_double)) if pl is not None else None,
        pv.ctypes.data_as(c_int32_p) if pv is not None else None))


def _shape(store):
    i = info(store)
    return max(i["height"], 1), max(i["width"], 1)


def counts(store):
    """-> (height, width) uint32, ``n_free | n_hit << 16`` per cell; row j is the cells at b index j."""
    out = np.zeros(_shape(store), np.uint32)
    _check(store, store.lib.lslam_occ_counts(store.h, out.ctypes.data_as(C.POINTER(C.c_uint32))))
    return out


def values(store):
    """-> (height, width) int8: -1 unknown, else 0 .. 100."""
    out = np.zeros(_shape(store), np.int8)
    _check(store, store.lib.lslam_occ_values(store.h, out.ctypes.data_as(C.POINTER(C.c_int8))))
    return out


def view(store):
    """-> (device pointer of the counts, device pointer of the values), valid until the next setup / clear of the store."""
    pc, pv = C.c_void_p(), C.c_void_p()
    _check(store, store.lib.lslam_occ_view(store.h, C.byref(pc), C.byref(pv)))
    return pc.value or 0, pv.value or 0


def trinary(values):
    """The pixels ``map_saver`` writes: value >= 65 -> 0 (occupied), 0 <= value <= 19 -> 254 (free), anything else -- unknown
    included -- 205; row 0 is the largest b."""
    v = np.asarray(values, np.int8)
    img = np.full(v.shape, 205, np.uint8)
    img[v >= 65] = 0
    img[(v >= 0) & (v <= 19)] = 254
    return np.ascontiguousarray(img[::-1])


def _num(x):
    return "%.17g" % float(x)  # (what printf gives the C++ mirror: the two write the same bytes)


def save_map(path_stem, values, params):
    """Write ``path_stem.pgm`` (binary P5, trinary) and ``path_stem.yaml`` in ``map_server``'s format -> the two paths.
    ``params``: an :class:`LslamOccParams` or a dict with ``resolution``, ``origin`` and ``up_axis``."""
    p = params_dict(params) if isinstance(params, LslamOccParams) else dict(params)
    img = trinary(values)
    h, w = img.shape
    pgm, yaml = path_stem + ".pgm", path_stem + ".yaml"
    with open(pgm, "wb") as f:
        f.write(b"P5\n# CREATOR: lslam occupancy %s m/pix\n%d %d\n255\n" % (_num(np.float32(p["resolution"])).encode(), w, h))
        f.write(img.tobytes())
    axes = "a = +z, b = +x (y up)" if int(p["up_axis"]) == 1 else "a = +x, b = +y (z up)"
    with open(yaml, "w") as f:
        f.write("# map axes in the graph frame: %s; origin is the corner of cell (0, 0)\n" % axes)
        f.write("image: %s\n" % os.path.basename(pgm))
        f.write("resolution: %s\n" % _num(np.float32(p["resolution"])))
        f.write("origin: [%s, %s, 0.0]\n" % (_num(p["origin"][0]), _num(p["origin"][1])))
        f.write("negate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n")
    return pgm, yaml


def load_map(path_stem):
    """Parse back what :func:`save_map` wrote -> (image (h, w) uint8, dict of the yaml's scalar entries)."""
    with open(path_stem + ".pgm", "rb") as f:
        data = f.read()
    fields, pos = [], 0
    while len(fields) < 4:  # P5, width, height, maxval; comment lines in between
        end = data.index(b"\n", pos)
        line = data[pos:end]
        pos = end + 1
        if not line.startswith(b"#"):
            fields += line.split()
    assert fields[0] == b"P5" and fields[3] == b"255"
    w, h = int(fields[1]), int(fields[2])
    img = np.frombuffer(data[pos:pos + w * h], np.uint8).reshape(h, w)
    meta = {}
    with open(path_stem + ".yaml") as f:
        for line in f:
            if line.startswith("#") or ":" not in line:
                continue
            k, v = line.split(":", 1)
            meta[k.strip()] = v.strip()
    return img, meta
