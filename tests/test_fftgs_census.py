"""The run table tests/fftgs_cases.py against the FFTGS kernels the compiler emitted into the built library
(tools/kernel_census.py): an instantiation added to a dispatch switch needs a table entry, an entry needs a compiled
kernel and a run, and the bars are 16 x the oracle's own error, no looser than the tolerances the suite already holds.
No GPU: the census reads the code objects of libgss_hip.so."""
import os
import sys

import numpy as np
import pytest

from gss import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_census
import fftgs_cases as FC
import fftgs_matrix as FM


@pytest.fixture(scope="module")
def compiled():
    if not kernel_census.tools_present():
        pytest.skip("llvm-readelf or a C++ demangler not available")
    found = [(f, tuple(int(a) if a.lstrip("-").isdigit() else a for a in args))
             for f, args in kernel_census.census(_lib.LIB_PATH)]
    assert len(found) > 500, len(found)          # the library's kernels were found at all
    return [k for k in found if k[0] in FC.FAMILIES]


def test_every_compiled_fftgs_kernel_has_a_table_entry(compiled):
    assert {f for f, _ in compiled} == set(FC.FAMILIES)
    missing = [k for k in compiled if k not in FC.CASES]
    assert not missing, "compiled kernels without an entry in tests/fftgs_cases.py: %s" % missing


def test_every_table_entry_names_a_compiled_kernel(compiled):
    stale = [k for k in FC.CASES if k not in set(compiled)]
    assert not stale, "entries of tests/fftgs_cases.py that name no compiled kernel: %s" % stale
    assert len(set(compiled)) == len(compiled) == len(FC.CASES)


def test_table_entries_are_runs_or_reasoned_exclusions():
    for key, entry in FC.CASES.items():
        assert key[0] in FC.FAMILIES, key
        if isinstance(entry, FC.UNREACHABLE):
            assert entry.reason.strip() and "csrc/" in entry.reason, key      # cites the dispatch line
        else:
            assert isinstance(entry, str) and entry in FC.RUNS, key
    for name, run in FC.RUNS.items():
        assert isinstance(run, FC.Run), name
        assert run.pipeline in FM.SCOPES and run.path in (None, "fused", "generic", "rocfft"), name
        assert 1 <= len(run.dims) <= 3 and int(np.prod(run.dims)) <= 600_000, name      # small runs only
        assert 0 <= run.nz <= 8 and (run.spacing is None or len(run.spacing) == len(run.dims)), name
        assert not run.rotated or len(run.dims) >= 2, name
    used = {e for e in FC.CASES.values() if isinstance(e, str)}
    assert used <= set(FC.RUNS)
    # the x variants of the fused pipeline sit in the runs the dispatch gives them
    assert FC.CASES[("ff_x_fwd2_kernel", (3, 4, 256, -1))] == "fused_1024x16x16_rot"
    assert FC.CASES[("ff_x_inv2_kernel", (8, 256, 8))] == "fused_512x16x16"


def test_bars_are_sixteen_times_the_oracle_and_no_looser_than_the_suite():
    assert set(FC.BARS) == set(FC.TOL) == {"F", "z"}
    for q, b in FC.BARS.items():
        assert b["oracle"] > 0.0
        assert b["bar"] == pytest.approx(16.0 * b["oracle"], rel=1e-3), q
        assert b["oracle"] <= FC.TOL[q] / 16.0 and b["bar"] <= FC.TOL[q], q      # the model keeps the oracle quiet


def test_long_double_is_finer_than_fp64_here():
    """The matrix skips where long double is a double; the machine that builds this library must not be one of those."""
    assert FM.long_double_ok(), np.finfo(np.longdouble).eps


@pytest.mark.parametrize("name", ["fused_1024x16x16", "gen_4096x16_rot", "lmc3_15x13"])
def test_recorded_oracle_error_is_reproduced(name):
    """The oracle's error on the two runs that set BARS, and on one co-simulation, measured again
    (tools/fftgs_matrix_oracle.py measures every run): about the recorded maxima.  A factor of two either way is left for
    another build of numpy's pocketfft or of libm, whose roundings need not be the ones recorded."""
    if not FM.long_double_ok():
        pytest.skip("numpy.longdouble is no finer than FP64 on this machine (eps %g): the 80-bit restatement of "
                    "tests/fftgs_matrix.py needs eps < 1e-18" % np.finfo(np.longdouble).eps)
    run = FC.RUNS[name]
    normals = FM.oracle_normals(run)
    e = FM.errors(FM.oracle_run(run, normals), FM.reference(run, normals))
    assert e["F"][0] <= 2.0 * FC.BARS["F"]["oracle"] and e["z"][0] <= 2.0 * FC.BARS["z"]["oracle"], e
    if name == "fused_1024x16x16":
        assert e["F"][0] >= 0.5 * FC.BARS["F"]["oracle"], e
    if name == "gen_4096x16_rot":
        assert e["z"][0] >= 0.5 * FC.BARS["z"]["oracle"], e
