"""tests/cpp/occupancy_end_to_end.cpp: the C++ mirrors of the occupancy grid (KeyframeStore::occ*, saveMap of
include/lslam_loop_closure.hpp) against the Python path on the same keyframes: equal counts, equal files."""
import subprocess

import numpy as np
import pytest

from test_abi import _build_cpp


def _drive(path, up_axis, fit, p, poses, clouds):
    with open(path, "w") as f:
        f.write("%d %d %.9g %.9g %.9g %d %d %d %.17g %.17g\n" % (len(poses), up_axis, np.float32(p["resolution"]), np.float32(p["min_range"]),
                                                               np.float32(p["max_range"]), fit, p["width"], p["height"], p["origin"][0],
                                                               p["origin"][1]))
        for T, (c, s) in zip(poses, clouds):
            f.write(" ".join("%.9g" % v for v in np.asarray(T, np.float32).reshape(16)) + "\n%d %d\n" % (len(c), len(s)))
            for cloud in (c, s):  # 9 digits: the float32 values exactly
                f.write("".join("%.9g %.9g %.9g\n" % tuple(q[:3]) for q in np.asarray(cloud, np.float32)))


def test_cpp_program_compiles_and_needs_the_backend(pkg, tmp_path):
    """g++ -std=c++11 -Wall -Werror; without a GPU the program reports the missing backend."""
    import torch
    exe = _build_cpp(pkg, tmp_path, "occupancy_end_to_end")
    if not torch.cuda.is_available():  # (with a GPU the gpu-marked test below runs the program)
        _drive(tmp_path / "d.txt", 2, 0, dict(resolution=0.5, min_range=1.0, max_range=10.0, width=8, height=8, origin=(0.0, 0.0)),
               [np.eye(4)], [(np.zeros((0, 4)), np.ones((1, 4)))])
        out = subprocess.run([str(exe), str(tmp_path / "d.txt"), str(tmp_path / "map"), str(tmp_path / "counts.bin")],
                             capture_output=True, text=True, timeout=60)
        assert out.returncode == 1 and "no CPU fallback" in out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("fit", [0, 1], ids=["given_bounds", "fitted_bounds"])
def test_cpp_mirror_equals_the_python_path(pkg, ctx, tmp_path, fit):
    import test_gpu_occupancy as G
    sh = G.shapes_data(pkg)[2]
    occ = pkg.occupancy
    p = dict(sh["p"])
    store = pkg.KeyframeStore(ctx, slab_points=4096)
    try:
        ids = [store.add(c, s) for c, s in sh["kfs"]]
        params = occ.fit_bounds(sh["poses"], **{k: p[k] for k in ("resolution", "min_range", "max_range", "up_axis")}) if fit else occ.occ_params(**p)
        store.occ_setup(params)
        store.occ_integrate(ids, sh["poses"])
        counts, values, info = store.occ_counts(), store.occ_values(), store.occ_info()
        (tmp_path / "py").mkdir()
        (tmp_path / "cpp").mkdir()
        occ.save_map(str(tmp_path / "py" / "map"), values, params)
    finally:
        store.close()
    _drive(tmp_path / "drive.txt", 2, fit, p, sh["poses"], sh["kfs"])
    exe = _build_cpp(pkg, tmp_path, "occupancy_end_to_end")
    out = subprocess.run([str(exe), str(tmp_path / "drive.txt"), str(tmp_path / "cpp" / "map"), str(tmp_path / "counts.bin")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [l.split() for l in out.stdout.splitlines() if l.split()]
    assert ["GRID", str(params.width), str(params.height), "%.17g" % params.origin[0], "%.17g" % params.origin[1]] in rows
    assert ["RAYS"] + [str(info[k]) for k in ("rays_cast", "rays_dropped", "rays_obstacle", "rays_ground", "n_integrated")] in rows
    assert ["REFUSED", "1"] in rows and ["TWICE", "1"] in rows
    c_counts = np.fromfile(tmp_path / "counts.bin", np.uint32).reshape(counts.shape)
    assert np.array_equal(c_counts, counts) and counts.any()
    for name in ("map.pgm", "map.yaml"):  # byte for byte
        assert (tmp_path / "py" / name).read_bytes() == (tmp_path / "cpp" / name).read_bytes(), name
    img, _ = occ.load_map(str(tmp_path / "cpp" / "map"))
    assert (img == 0).any() and (img == 254).any() and (img == 205).any()
