"""The case table tests/kernel_cases.py against the kernels the compiler emitted into the built library
(tools/kernel_census.py): an instantiation added to a dispatch switch needs a table entry, and an entry needs a
compiled kernel.  No GPU: the census reads the code objects of libgss_hip.so."""
import os
import sys

import pytest

from gss import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_census
import kernel_cases as KC


@pytest.fixture(scope="module")
def compiled():
    if not kernel_census.tools_present():
        pytest.skip("llvm-readelf or a C++ demangler not available")
    found = [(f, tuple(int(a) if a.lstrip("-").isdigit() else a for a in args))
             for f, args in kernel_census.census(_lib.LIB_PATH)]
    assert len(found) > 500, len(found)          # the library's kernels were found at all
    return [k for k in found if k[0] in KC.FAMILIES]


def test_every_compiled_kriging_kernel_has_a_table_entry(compiled):
    assert {f for f, _ in compiled} == set(KC.FAMILIES)
    missing = [k for k in compiled if k not in KC.CASES]
    assert not missing, "compiled kernels without a case in tests/kernel_cases.py: %s" % missing


def test_every_table_entry_names_a_compiled_kernel(compiled):
    stale = [k for k in KC.CASES if k not in set(compiled)]
    assert not stale, "entries of tests/kernel_cases.py that name no compiled kernel: %s" % stale
    assert len(set(compiled)) == len(compiled) == len(KC.CASES)


def test_table_entries_are_cases_or_reasoned_exclusions():
    for key, entry in KC.CASES.items():
        assert key[0] in KC.FAMILIES, key
        if isinstance(entry, KC.UNREACHABLE):
            assert entry.reason.strip() and ".hip" in entry.reason, key      # cites the dispatch line
        else:
            assert isinstance(entry, KC.Case), key
            assert key[1][0] == entry.dim, key
            assert (entry.k is None) != (entry.n is None), key
    for f in KC.FAMILIES:
        for q in ("mean", "var", "cov"):
            b = KC.BARS[f][q]
            assert b["bar"] == pytest.approx(min(max(16.0 * b["oracle"], 8.0), 1e-9 / (2.0 ** -53 * 1.5)), rel=1e-2)
