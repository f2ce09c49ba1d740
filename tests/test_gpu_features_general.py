"""GPU: lslam_extract_features against tests/features_ref.py, the independent float64 statement of
ScanRegistration::extractFeatures, over the constructed bank of tests/features_cases.py -- the places where the kernels differ
from the sequential reference (marks applied across the workgroup, the bitonic tie order, the caps under markAsPicked, ring
ends), each reached a counted number of times (tests/test_features_ref.py asserts the counts on the CPU).

On the rings the reference calls unambiguous the device must take the reference's marks, labels and lists; on every ring,
ambiguous or not, it must equal the CPU oracle bit for bit.  The first keeps the oracle / kernel pair honest, the second
covers the rings the first leaves out."""
import numpy as np
import pytest

import features_cases as CS
import features_ref as R
from test_features_ref import compare_with_ref, oracle_params
from test_gpu_features import _compare, bits

pytestmark = pytest.mark.gpu

BANK = CS.bank()
TAPS = ("curvature", "picked", "label")
LISTS = ("sharp", "less_sharp", "flat", "less_flat")


def device_params(pkg, ctx, params):
    return params.apply(pkg.scan_registration.default_params(ctx))


def run_device(pkg, ctx, call, ranges=None):
    return pkg.scan_registration.extract_features(ctx, call.cloud, call.ranges if ranges is None else ranges,
                                                  device_params(pkg, ctx, call.params), taps=True)


@pytest.mark.parametrize("call", BANK, ids=[c.name for c in BANK])
def test_bank_matches_reference_and_oracle(pkg, ctx, oracle, call):
    """every call of the bank; the tie and edge rings come round at nFeatureRegions 1, 6 and 40 (ties_nf*), so the same ties
    fall in sort stretches of different power-of-two paddings"""
    got = run_device(pkg, ctx, call)
    compare_with_ref(got, R.extract(call.cloud, call.ranges, call.params), call, call.name)
    _compare(got, oracle.extract_features(call.cloud, call.ranges, oracle_params(oracle, call.params)), call.name)


def test_device_takes_the_oracles_side_of_every_threshold_pair(pkg, ctx, oracle):
    """the adjacent fp32 pairs of the CPU threshold tests as rings of one call: one call for the accepted side, one for the
    rejected side, for the marking rules and for the classification gates"""
    pairs = CS.threshold_pairs(oracle)
    sides = []
    for side in (0, 1):
        outs = []
        for call in CS.threshold_calls(pairs, side):
            got = run_device(pkg, ctx, call)
            _compare(got, oracle.extract_features(call.cloud, call.ranges, oracle_params(oracle, call.params)), call.name)
            outs.append((call, got))
        sides.append(outs)
    for (call0, got0), (call1, got1), names in zip(sides[0], sides[1], (CS.MARK_FAMILIES, CS.CLASSIFY_FAMILIES)):
        assert np.array_equal(call0.ranges, call1.ranges)
        differ = [k for k, (a, b) in enumerate(call0.ranges.tolist())
                  if not (np.array_equal(got0["picked"][a:b + 1], got1["picked"][a:b + 1]) and
                          np.array_equal(got0["label"][a:b + 1], got1["label"][a:b + 1]))]
        assert differ == list(range(len(names))), (call0.name, differ)       # every rule ring flips, the control ring does not
    # and the flips are the rules' own: the mark or label each family is decided on
    (m0, g0), (m1, g1) = sides[0][0], sides[1][0]
    for k, name in enumerate(CS.MARK_FAMILIES):
        a, b = m0.ranges[k].tolist()
        cut = lambda g: dict(picked=g["picked"][a:b + 1], label=g["label"][a:b + 1])
        assert bool(CS.MARK_DECISION[name](cut(g0))) == pairs[name][2] and bool(CS.MARK_DECISION[name](cut(g1))) == pairs[name][3], name
    (c0, h0), (c1, h1) = sides[0][1], sides[1][1]
    shown = {R.SURFACE_FLAT: R.SURFACE_FLAT, R.ONESIDE_FLAT: R.ONESIDE_FLAT, R.CORNER_SHARP: R.CORNER_SHARP, R.MESSY: R.UNKNOW}
    for k, name in enumerate(CS.CLASSIFY_FAMILIES):
        a = int(c0.ranges[k, 0])
        assert h0["label"][a + 5] == shown[pairs[name][2]] and h1["label"][a + 5] == shown[pairs[name][3]], name


@pytest.mark.parametrize("call", BANK, ids=[c.name for c in BANK])
def test_one_launch_equals_ring_by_ring(pkg, ctx, call):
    """the whole call as one launch (rings whose helper workgroups finished long ago beside rings that classify for
    themselves) and again one ring per launch: identical outputs"""
    whole = run_device(pkg, ctx, call)
    taps = {k: np.zeros_like(whole[k]) for k in TAPS}
    taps["label"][:] = R.UNKNOW
    lists = {k: [] for k in LISTS}
    for a, b in call.ranges.tolist():
        one = run_device(pkg, ctx, call, np.array([[a, b]], np.int32))
        for k in LISTS:
            lists[k].append(one[k])
        if b >= a:
            for k in TAPS:
                taps[k][a:b + 1] = one[k][a:b + 1]
    for k in TAPS:
        assert np.array_equal(whole[k].view(np.uint8), taps[k].view(np.uint8)), (call.name, k)
    for k in LISTS:
        joined = np.concatenate(lists[k])
        assert joined.shape == whole[k].shape and np.array_equal(bits(joined), bits(whole[k])), (call.name, k)
