"""lslam_opts.ab_switches and LSLAM_AB_SWITCHES are input from outside: a bit the library has no variant for -- the six retired
ones (1, 2, 4, 8, 32, 128) among them -- is refused with LSLAM_ERR_INVALID before anything is enqueued, not ignored; the
bits it has are taken as before."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RETIRED = (1, 2, 4, 8, 32, 128)
AB_NO_COMPACT = 64


def _run(ctx, pose, opts):
    """lslam_scanmatch_run through the binding's library handle -> (return code, the pose buffer the call was given)."""
    p = np.array(pose, dtype=np.float32).reshape(6)
    rc = ctx.lib.lslam_scanmatch_run(ctx.h, p.ctypes.data_as(C.POINTER(C.c_float)), C.byref(opts), None)
    return rc, p


def test_retired_bits_are_refused_and_known_bits_accepted(pkg, ctx, small_problem):
    pr = small_problem
    ctx.map_set(pr["map_corner"], pr["map_surf"])
    ctx.scan_set(pr["corner"], pr["surf"])
    opts = ctx.default_opts()
    for bit in RETIRED:
        opts.ab_switches = bit
        rc, pose = _run(ctx, pr["init_pose"], opts)
        assert rc == pkg.Status.ERR_INVALID, bit
        assert np.array_equal(pose.view(np.uint32), np.asarray(pr["init_pose"], np.float32).view(np.uint32)), bit
        msg = ctx.lib.lslam_last_error().decode()
        assert "ab_switches" in msg and ("0x%x" % bit) in msg, (bit, msg)
    opts.ab_switches = AB_NO_COMPACT
    rc, pose = _run(ctx, pr["init_pose"], opts)
    assert rc == pkg.Status.OK
    assert not np.array_equal(pose, np.asarray(pr["init_pose"], np.float32))  # the loop ran


def test_a_context_made_under_a_retired_bit_is_refused(pkg, monkeypatch):
    monkeypatch.setenv("LSLAM_AB_SWITCHES", "1")
    with pytest.raises(pkg.LslamError) as e:
        pkg.Context(0).close()
    assert e.value.code == pkg.Status.ERR_INVALID and "LSLAM_AB_SWITCHES" in str(e.value)
    monkeypatch.setenv("LSLAM_AB_SWITCHES", str(AB_NO_COMPACT))
    pkg.Context(0).close()
