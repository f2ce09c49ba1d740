"""The launch schedule of the scan-match driver (run_batch_impl and its stages in csrc/lslam_api.hip), not only its results.

Every configuration below runs on a context of its own -- the iteration hint and the
parity of the queue-launch counter carry over from call to call -- and issues the same call three times, so that the
iteration-hint rule (the spare iteration is dropped after three equal runs) is part of what is pinned.  Per call the return
status, every field of lslam_stats but the two times, the poses' bytes, and what the call added to the eight sweep-launch
counters and to the grid-launch counter are compared, field by field, with tests/golden/run_schedule.json.  That fixture
was recorded by tools/record_run_schedule.py from the library as it was BEFORE the driver was cut into stages: a host
round trip more, or a trailing sweep that finds every scan converged, changes a counter or stats.sweep_launches here even
where the poses stay the same."""
import importlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_schedule.json")
LANE, PACKET, GRID = 1, 2, 3  # LSLAM_SEARCH_*
# lslam_opts.ab_switches (include/lslam_c.h)
AB_NO_COMPACT = 64
N_CALLS = 3
STEREO_SHAPES = ((16, 900), (16, 450), (8, 300), (16, 1200))  # as tests/test_gpu_stereo_batch.py
STEREO_SET_SIZES = (1500, 300, 63, 800)
TIME_FIELDS = ("gpu_ms_total", "gpu_ms_sweep")

# name -> (map, scans, call, lslam_opts fields).  map: "trees" (lslam_map_set), "deferred" (device-side set with the
# trees deferred), "cubes" (lslam_cubemap_set); scans: how many copies of the small problem's scan are resident (each at a
# start pose of its own), or "stereo": four scans of their own shapes, each with a stereo set; call: "batch" / "sharded".
CONFIGS = {
    "one_default": ("trees", 1, "batch", {}),
    "one_profile": ("trees", 1, "batch", dict(profile=1)),
    "one_no_iterations": ("trees", 1, "batch", dict(max_iterations=0)),
    "one_cert_forced": ("trees", 1, "batch", dict(knn_cert=2)),
    "one_cert_off": ("trees", 1, "batch", dict(knn_cert=0)),
    "one_grid": ("trees", 1, "batch", dict(search_mode=GRID)),
    "one_grid_fine_score": ("trees", 1, "batch", dict(search_mode=GRID, fine_score=1, use_score=1)),
    "one_packet": ("trees", 1, "batch", dict(search_mode=PACKET)),
    "one_deferred_trees": ("deferred", 1, "batch", {}),
    "seven_trees": ("trees", 7, "batch", dict(scans_in_flight=3, search_mode=LANE)),
    "seven_grid": ("trees", 7, "batch", dict(scans_in_flight=3, search_mode=GRID)),
    "seven_grid_no_compact": ("trees", 7, "batch", dict(scans_in_flight=3, search_mode=GRID, ab_switches=AB_NO_COMPACT)),
    "four_stereo_grid": ("trees", "stereo", "batch", dict(scans_in_flight=2, search_mode=GRID)),
    "one_cubes": ("cubes", 1, "batch", {}),
    "sharded": ("trees", 1, "sharded", {}),
    "sharded_fine_score": ("trees", 1, "sharded", dict(fine_score=1, use_score=1)),
}


def _stereo_batch(synth, pr):
    pts = np.concatenate([pr["map_corner"], pr["map_surf"]])
    scans, inits, sets = [], [], []
    for k, ((rings, steps), n_obs) in enumerate(zip(STEREO_SHAPES, STEREO_SET_SIZES)):
        gt = (0.01 * (k % 3), -0.01, 0.3 + 0.2 * k, 3.0 - 0.7 * k, -2.0 + 0.5 * k, synth.SENSOR_HEIGHT)
        qc, qs, gt = synth.make_scan(pr["world"], rings, steps, gt_pose=gt, seed=300 + k)
        scans.append((qc, qs))
        inits.append(synth.perturb_pose(gt, seed=400 + k))
        lm, ob, w = synth.make_stereo(pts, gt, n=n_obs, seed=500 + k)
        sets.append((lm[:n_obs], ob[:n_obs], w[:n_obs]))
    return scans, np.stack(inits), sets


def _record(ctx, rc, poses, stats, before):
    after = ctx.sweep_launches(), ctx.grid_launches()
    rows = []
    for st in stats:
        row = {}
        for f, _ in type(st)._fields_:
            if f not in TIME_FIELDS:
                v = getattr(st, f)
                row[f] = float(v).hex() if isinstance(v, float) else int(v)
        rows.append(row)
    return dict(status=int(rc), stats=rows, poses=np.ascontiguousarray(poses, np.float32).tobytes().hex(),
                sweep_launches={k: after[0][k] - before[0][k] for k in after[0]}, grid_launches=after[1] - before[1])


def run_config(pkg, synth, pr, name):
    """The three calls of configuration `name` on a fresh context -> their records."""
    which_map, scans, call, fields = CONFIGS[name]
    ctx = pkg.Context(0)
    fm = None
    try:
        if which_map == "deferred":  # as tests/test_gpu_grid.py: the surround of a feature map, handed over on the device
            ctx.defer_trees(True)
            fm = pkg.FeatureMap(ctx, 21, 21, 11)
            fm.setup_filter_size(0.05, 0.05, 0.05)
            fm.update(np.zeros(3, np.float32))
            fm.add_feature_cloud(pr["map_corner"], pr["map_surf"], np.eye(4, dtype=np.float32))
            fm.surround_to_map()
            assert ctx.lazy_trees()[2]  # grids, no trees yet
        elif which_map == "cubes":
            ctx.cubemap_set(pr["map_corner"], pr["map_surf"], cube_size=20.0, origin=(5, 5, 1), dims=(11, 11, 3))
        else:
            ctx.map_set(pr["map_corner"], pr["map_surf"])
        if scans == "stereo":
            batch, inits, sets = _stereo_batch(synth, pr)
            ctx.scan_set_batch(batch)
            cam = ctx.default_stereo_cam()
            for i, v in enumerate(synth.T_CAM_LIDAR.reshape(-1)):
                cam.T_cl[i] = v
            cam.weight = 1e-2
            ctx.stereo_set_batch(sets, cam)
        elif scans == 1:
            ctx.scan_set(pr["corner"], pr["surf"])
            inits = np.asarray(pr["init_pose"], np.float32).reshape(1, 6)
        else:  # copies of the scan; start poses further and further from the truth, so the loops differ in length
            ctx.scan_set_batch([(pr["corner"], pr["surf"])] * scans)
            inits = np.stack([synth.perturb_pose(pr["gt_pose"], seed=40 + k, dt=0.05 + 0.05 * k, dr_deg=0.3 + 0.3 * k) for k in range(scans)])
        opts = ctx.default_opts()
        for f, v in fields.items():
            setattr(opts, f, v)
        out = []
        for _ in range(N_CALLS):
            before = ctx.sweep_launches(), ctx.grid_launches()
            if call == "sharded":  # one rank: the sum over the ranks is what is there
                import torch
                xchg = torch.zeros(32, dtype=torch.float64, device="cuda")
                rc, pose, st = ctx.run_sharded(inits[0], lambda ptr, n: None, xchg, opts=opts)
                out.append(_record(ctx, rc, pose, [st], before))
            else:
                rc, poses, stats = ctx.run_batch(inits, opts)
                out.append(_record(ctx, rc, poses, stats, before))
        return out
    finally:
        if fm is not None:
            fm.close()
        ctx.close()


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_every_configuration(fixture):
    assert sorted(fixture) == sorted(CONFIGS)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_run_schedule_is_the_recorded_one(pkg, synth, small_problem, fixture, name):
    got, want = run_config(pkg, synth, small_problem, name), fixture[name]
    assert len(got) == len(want) == N_CALLS
    for k, (g, w) in enumerate(zip(got, want)):
        assert g["status"] == w["status"], (name, k)
        assert g["sweep_launches"] == w["sweep_launches"], (name, k)
        assert g["grid_launches"] == w["grid_launches"], (name, k)
        assert len(g["stats"]) == len(w["stats"]), (name, k)
        for p, (gs, ws) in enumerate(zip(g["stats"], w["stats"])):
            assert sorted(gs) == sorted(ws), (name, k, p)
            for f in ws:
                assert gs[f] == ws[f], (name, k, p, f)
        assert g["poses"] == w["poses"], (name, k)
