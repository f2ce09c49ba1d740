"""The in-range fit's two chains on the host (tools/fit_inrange_ref.cpp): div_inrange and sqrt_inrange of
csrc/lslam_device.hpp restated with fmaf, built with -ffp-contract=off, against `/` and sqrtf.  The device's v_rcp_f32 and
v_sqrt_f32 are accurate to one ulp, so each chain starts from the correctly rounded seed and from both of its neighbours, and
must give the correctly rounded result -- bit for bit -- from all three, for every operand the guard lets through:
FIT_LO = 2^-30 <= |a|, |b| <= FIT_HI = 2^30, a denominator's mantissa not all ones (over b = (2 - 2^-23) 2^m a power of two's
quotient lies 2^-25 above a rounding tie, which the chain reaches from the correctly rounded seed only: the one pair of
patterns the edge list finds), 2^-96 <= x < inf for the square root; numerators +0, and -0 over a negative denominator."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    flags = ["-O2", "-ffp-contract=off", "-std=c++17"]
    if cxx is None:  # the HIP compiler's host side
        cxx = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        flags += ["-x", "c++"]
    exe = str(tmp_path_factory.mktemp("fit_inrange") / "fit_inrange_ref")
    subprocess.check_call([cxx] + flags + ["-o", exe, os.path.join(ROOT, "tools", "fit_inrange_ref.cpp")])

    def run(*args):
        out = subprocess.check_output([exe] + [str(a) for a in args], text=True)
        print(out, end="")
        return out.strip().splitlines()[-1].split()

    return run


def test_random_operands_inside_the_range(ref):
    """10^7 operand pairs (random signs, exponents and mantissas inside the range) and 10^7 square-root operands, three seeds."""
    assert ref("random", 10_000_000, 20261020) == ["mismatch", "0"]


def test_edges_of_the_range_and_zero_numerators(ref):
    """Exponents at both limits and next to them, mantissas all zero / one / half / all ones but one / all ones, both signs,
    every numerator over every denominator the guard lets through; +0 over either sign and -0 over a negative denominator;
    the square root from 2^-96 to the largest finite value, and 0."""
    out = ref("edges")
    assert out[0] == "checked" and int(out[1]) > 4000
    assert out[2] == "refused" and int(out[3]) > 0  # (the all-ones mantissas among the denominators)
    assert out[4:] == ["mismatch", "0"]


def test_guard_refuses_what_is_just_outside(ref):
    """The limits themselves pass; one ulp outside either limit, +-0, +-inf, NaN and a denormal do not; a denominator with
    its mantissa all ones does not either."""
    out = " ".join(ref("guard"))
    assert out == "guard 1 1 1 1 1 | 0 0 0 0 0 0 0 0 0 0 | 1 0 0"


def test_reciprocal_of_five(ref):
    """The literal the divisions by 5 start from (FIT_RCP5 = 0x3e4ccccd) is what the chain's two refinement steps make of the
    reciprocal of 5 from all three seeds."""
    assert ref("rcp5") == ["rcp5", "3e4ccccd", "3e4ccccd", "3e4ccccd"]
