"""CPU checks of the survey-extractor restatement (tests/survey_map_ref.py) against independent statements of the same things:
sequential region growing against the min-ancestor fixpoint, the Jacobi normals against numpy.linalg.eigh, the filter with a
minimum count against a plain loop -- and the scene's counts and decision margins, which the GPU tests rely on."""
import numpy as np
import pytest

import survey_map_ref as R

F = np.float32
# the restatement's own counts on the scene: filtered points, regions dropped, planar and boundary points, corner and surf points out
SCENE_LITERALS = (8425, 138, 8209, 684, 138, 462)


@pytest.fixture(scope="module")
def scene():
    return R.scene_reference()


def test_scene_counts(scene):
    cloud, ref = scene
    st = ref["stats"]
    print(st)
    assert len(cloud) == 40300
    # two blocks of 20 000 points (the planes and their copy); the detached patch of 300 stays below the block minimum
    assert (st["blocks_kept"], st["blocks_dropped"], st["max_block_points"], st["points_nonfinite"]) == (2, 1, 20000, 0)
    assert st["undefined_normals"] == 0
    for b in ref["blocks"]:
        assert 10 <= b["counts"].min() and b["counts"].max() <= 40
        sizes = np.sort(np.bincount(b["labels"])[np.unique(b["labels"])])[::-1]
        assert sizes[0] > 1900 and sizes[1] > 1900 and sizes[2] < 50  # the floor, the wall, and fragments along the edge
    assert st["clusters_kept"] == 4
    assert (st["filtered_points"], st["clusters_dropped"], st["planar_points"], st["boundary_points"], st["n_corner"], st["n_surf"]) == SCENE_LITERALS
    # the copy lands in a second cube
    assert len(np.unique(ref["corner_cube"])) == 2 and len(np.unique(ref["surf_cube"])) == 2




def test_sequential_region_growing_equals_the_fixpoint(scene):
    c = R.cos_threshold(R.DEFAULTS["smoothness_angle"])
    for b in scene[1]["blocks"]:
        seq = R.region_sequential(b["normals"], b["lists"], c)
        fix, rounds = R.region_fixpoint(b["normals"], b["lists"], c)
        assert np.array_equal(seq, fix) and rounds > 2
    # an asymmetric graph: a sparse line whose lists reach into a dense clump that never looks back; the line ranks first
    rng = np.random.default_rng(9)
    pts = np.concatenate([rng.uniform(0, 0.05, (40, 3)), np.stack([0.3 + 0.25 * np.arange(12), np.zeros(12), np.zeros(12)], 1)], 0).astype(F)
    lists = R.knn_lists(pts, 8)
    assert np.all(lists[:40] < 40) and np.any(lists[40:] < 40)
    for trial in range(4):
        nrm = np.concatenate([np.tile([0.0, 0.0, 1.0], (52, 1)), rng.uniform(0, 0.1, (52, 1))], 1).astype(F)
        if trial % 2:
            nrm[40:, 3] = rng.uniform(0, 0.001, 12)
        seq = R.region_sequential(nrm, lists, c)
        fix, _ = R.region_fixpoint(nrm, lists, c)
        assert np.array_equal(seq, fix)
    assert len(np.unique(seq)) > 1  # (were the graph symmetric, everything would be one region)


def test_normals_against_eigh(scene):
    b = scene[1]["blocks"][0]
    q = b["filtered"][::9]
    nrm, cnt = R.normals(b["block"], q, 0.05)
    count, cov = R.covariances(b["block"], q, 0.05)
    assert np.array_equal(cnt, count) and cnt.min() >= 3
    worst_n = worst_c = 0.0
    for k in range(len(q)):
        # the neighbours again, by the plain definition, on fp64 inputs
        d2 = R.d2_f32(q[k:k + 1], b["block"])[0]
        nb = b["block"][d2 < R.radius2(0.05)].astype(np.float64) - q[k].astype(np.float64)
        assert len(nb) == cnt[k]
        w, v = np.linalg.eigh(np.cov(nb.T, bias=True))
        n = v[:, 0] if v[:, 0] @ q[k].astype(np.float64) <= 0 else -v[:, 0]
        worst_n = max(worst_n, np.abs(n - nrm[k, :3]).max())
        worst_c = max(worst_c, abs(w[0] / w.sum() - nrm[k, 3]))
    print("normals against eigh: components within %.2e, curvature within %.2e" % (worst_n, worst_c))
    assert worst_n < 1e-6 and worst_c < 1e-7  # fp32 rounding of a unit vector / of a curvature below 1/3, and nothing more


def test_filter_with_minimum_against_a_plain_loop():
    rng = np.random.default_rng(2)
    c = np.concatenate([rng.uniform(-3, 3, (4000, 3)), rng.uniform(0, 9, (4000, 1))], 1).astype(F)
    got = R.voxel_filter_min(c, 0.4, 3)
    cells = {}
    for p in c:
        cells.setdefault(tuple(np.floor(p[:3] * (F(1.0) / F(0.4))).astype(int)[::-1]), []).append(p)
    want = []
    for key in sorted(cells):
        if len(cells[key]) >= 3:
            s = np.zeros(4, F)
            for p in cells[key]:
                s = (s + p).astype(F)
            want.append(s / F(len(cells[key])))
    assert np.array_equal(got.view(np.uint32), np.array(want, F).view(np.uint32))
    one = R.voxel_filter_min(c, 0.4, 1)
    assert len(one) == len(cells) > len(got) > 0


def test_scene_decision_margins(scene):
    """What lets the GPU tests compare decisions exactly: no tested pair within 1e-5 of the edge threshold, no point's largest gap
    within 1e-5 of the boundary threshold."""
    c = R.cos_threshold(R.DEFAULTS["smoothness_angle"])
    m_dot, m_gap = np.inf, np.inf
    for b in scene[1]["blocks"]:
        _, dot, tested = R.edge_table(b["normals"], b["lists"], c)
        m_dot = min(m_dot, np.abs(dot[tested].astype(np.float64) - np.float64(c)).min())
        m_gap = min(m_gap, np.abs(b["gaps"] - R.DEFAULTS["boundary_angle"]).min())
    print("margins: | |dot| - c | >= %.3g, | gap - threshold | >= %.3g" % (m_dot, m_gap))
    assert m_dot >= 1e-5 and m_gap >= 1e-5
