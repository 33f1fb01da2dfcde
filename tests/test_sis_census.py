"""The run table tests/sis_cases.py against the sequential-indicator-simulation kernels the compiler emitted into the
built library (tools/kernel_census.py): an instantiation needs a table entry, an entry needs a compiled kernel and a run
that the dispatch (sis_realize_block, csrc/sis.hip) sends to it.  No GPU: the census reads the code objects of
libgss_hip.so."""
import os
import sys

import pytest

from gss import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_census
import sis_cases as SC


@pytest.fixture(scope="module")
def compiled():
    if not kernel_census.tools_present():
        pytest.skip("llvm-readelf or a C++ demangler not available")
    found = [(f, tuple(int(a) if a.lstrip("-").isdigit() else a for a in args))
             for f, args in kernel_census.census(_lib.LIB_PATH)]
    assert len(found) > 500, len(found)          # the library's kernels were found at all
    return [k for k in found if k[0].startswith("sis_")]


def test_every_compiled_sis_kernel_has_a_table_entry(compiled):
    assert {f for f, _ in compiled} == set(SC.FAMILIES)
    missing = [k for k in compiled if k not in SC.CASES]
    assert not missing, "compiled kernels without an entry in tests/sis_cases.py: %s" % missing


def test_every_table_entry_names_a_compiled_kernel(compiled):
    stale = [k for k in SC.CASES if k not in set(compiled)]
    assert not stale, "entries of tests/sis_cases.py that name no compiled kernel: %s" % stale
    assert len(set(compiled)) == len(compiled) == len(SC.CASES)


def test_the_kernels_sit_in_runs_the_dispatch_sends_to_them():
    for (family, args), name in SC.CASES.items():
        assert family in SC.FAMILIES and name in SC.RUNS, (family, args, name)
        run = SC.RUNS[name]
        if family in SC.SWEEP_FAMILY.values():
            assert SC.SWEEP_FAMILY[run.sweep] == family and args == (run.KT, "true" if run.categorical else "false"), name
        elif family == "sis_transpose_kernel":
            assert run.npaths == 1 and run.R % 64 and (run.dims[0] * run.dims[1]) % 64 and len(run.dims) == 2, name
        else:                                    # the field layout: node-major for a shared order
            assert args == ("true" if run.npaths == 1 else "false",), name
            assert family != "sis_seed_data_kernel" or run.nd > 0, name
