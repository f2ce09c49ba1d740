"""The marginal-covariance entry points of include/lslam_c.h: both symbols are exported and bound, both structs exist with the
field order the header documents, and the ctypes mirrors have the C compiler's layout.  CPU only."""
import ctypes as C
import os
import subprocess
from importlib import import_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS_FIELDS = ["rel_tol", "max_iters", "coarse"]
STATS_FIELDS = ["columns", "panels", "iters_max", "iters_sum", "coarse_used", "worst_rel_residual"]


def test_symbols_are_exported_and_bound(pkg):
    capi = import_module("the-cooper-mapper_amd.capi")
    lib = capi.load_library()
    for name in ("lslam_pg_marginals", "lslam_pg_relative_covariances"):
        assert hasattr(lib, name) and name in capi.SYMBOLS
    assert len(capi.SYMBOLS["lslam_pg_marginals"][1]) == 7 and len(capi.SYMBOLS["lslam_pg_relative_covariances"][1]) == 7


def test_struct_fields_and_layout_equal_the_c_compilers(pkg, tmp_path):
    capi = import_module("the-cooper-mapper_amd.capi")
    assert [f[0] for f in capi.LslamPgMarginalOpts._fields_] == OPTS_FIELDS
    assert [f[0] for f in capi.LslamPgMarginalStats._fields_] == STATS_FIELDS
    offs = ["offsetof(lslam_pg_marginal_opts, %s)" % f for f in OPTS_FIELDS] + ["sizeof(lslam_pg_marginal_opts)"]
    offs += ["offsetof(lslam_pg_marginal_stats, %s)" % f for f in STATS_FIELDS] + ["sizeof(lslam_pg_marginal_stats)"]
    src = tmp_path / "mg.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "lslam_c.h"\nint main(void){size_t v[] = {%s};\n'
                   'for (size_t k = 0; k < sizeof(v) / sizeof(v[0]); ++k) printf("%%zu ", v[k]);\n'
                   'return 0;}\n' % ", ".join(offs))
    exe = tmp_path / "mg"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    # the prototypes, as the header states them (compiled, not linked)
    proto = tmp_path / "proto.c"
    proto.write_text('#include "lslam_c.h"\n'
                     'int (*a)(lslam_pg *, int32_t, const int32_t *, const lslam_pg_marginal_opts *, double *, double *, lslam_pg_marginal_stats *) = lslam_pg_marginals;\n'
                     'int (*b)(lslam_pg *, int32_t, int32_t, const int32_t *, const lslam_pg_marginal_opts *, double *, lslam_pg_marginal_stats *) = lslam_pg_relative_covariances;\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(proto), "-o",
                           str(tmp_path / "proto.o")])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    o, s = capi.LslamPgMarginalOpts, capi.LslamPgMarginalStats
    want = [getattr(o, f).offset for f in OPTS_FIELDS] + [C.sizeof(o)] + [getattr(s, f).offset for f in STATS_FIELDS] + [C.sizeof(s)]
    assert got == want
