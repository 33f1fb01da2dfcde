"""The case table tests/search_cases.py against the neighbour-search and IDW / LWR kernels the compiler emitted into the
built library (tools/kernel_census.py): an instantiation added to a dispatch switch needs a table entry, and an entry
needs a compiled kernel.  Also builds every search problem of the table on the CPU: the exactness precondition of the
integer ranking, the haversine gap assertion (no query excluded) and the edges each case claims.  No GPU."""
import os
import sys

import numpy as np
import pytest

from gss import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_census
import search_cases as SC
import search_matrix as SM


@pytest.fixture(scope="module")
def compiled():
    if not kernel_census.tools_present():
        pytest.skip("llvm-readelf or a C++ demangler not available")
    found = [(f, tuple(int(a) if a.lstrip("-").isdigit() else a for a in args))
             for f, args in kernel_census.census(_lib.LIB_PATH)]
    assert len(found) > 500, len(found)          # the library's kernels were found at all
    return [k for k in found if k[0] in SC.FAMILIES]


def test_every_compiled_search_and_estimator_kernel_has_a_table_entry(compiled):
    assert {f for f, _ in compiled} == set(SC.FAMILIES)
    missing = [k for k in compiled if k not in SC.CASES]
    assert not missing, "compiled kernels without a case in tests/search_cases.py: %s" % missing


def test_every_table_entry_names_a_compiled_kernel(compiled):
    stale = [k for k in SC.CASES if k not in set(compiled)]
    assert not stale, "entries of tests/search_cases.py that name no compiled kernel: %s" % stale
    assert len(set(compiled)) == len(compiled) == len(SC.CASES)


def test_table_entries_are_cases_or_reasoned_exclusions():
    for key, entry in SC.CASES.items():
        assert key[0] in SC.FAMILIES, key
        if isinstance(entry, SC.UNREACHABLE):
            assert entry.reason.strip() and ".hip" in entry.reason, key      # cites the dispatch line
            continue
        assert isinstance(entry, SC.Case), key
        if key[1]:
            assert key[1][0] == entry.dim, key
        assert 1 <= entry.k <= entry.n, key
        assert (key[0] in SC.EST_FAMILIES) == (entry.op in ("idw", "lwr")), key
    assert [k for k, e in SC.CASES.items() if isinstance(e, SC.UNREACHABLE)] == [("knn_kernel", (1, 3)),
                                                                                 ("knn_kernel", (3, 3))]


def test_bars_follow_the_rule_and_are_no_looser_than_the_existing_tolerances():
    used = {f: set() for f in SC.EST_FAMILIES}
    for key, entry in SC.CASES.items():
        if key[0] in SC.EST_FAMILIES:
            used[key[0]].update(SC.quantities(entry))
    for f in SC.EST_FAMILIES:
        assert set(SC.BARS[f]) == used[f], f
        for q, b in SC.BARS[f].items():
            cap = SC.EXISTING_TOL[q] / SM.UNIT
            assert b["bar"] == pytest.approx(min(max(16.0 * b["oracle"], 8.0), cap), rel=1e-2), (f, q)
            assert b["bar"] * SM.UNIT <= SC.EXISTING_TOL[q]


def test_the_cases_cover_the_sizes_and_edges_of_the_search():
    cases = [c for c in SC.CASES.values() if isinstance(c, SC.Case) and c.op in ("search", "masked")]
    assert {63, 64, 65, 4095, 4096, 4097} <= {c.n for c in cases}
    assert {1, 7, 8, 12, 63, 64, 65, 128, 129, 200} <= {c.k for c in cases}
    assert any(c.n > 262144 and c.op == "search" and c.route == "index" for c in cases)
    assert any(c.build == "both" for c in cases) and any(c.n >= 16384 and not c.build for c in cases)
    assert {"brute", "few"} <= {c.route for c in cases}
    assert any(c.m == 1 for c in cases) and any(c.m % 4 and c.m % 16 for c in cases)
    assert {"radius", "radii", "rotated"} <= {c.ball for c in cases}
    edges = set().union(*[set(c.expect) for c in cases])
    assert {"boundary", "short", "empty", "tie64", "rank0"} <= edges
    masked = [c for c in cases if c.op == "masked"]
    assert any(c.k < 64 for c in masked) and any(c.k > 64 for c in masked) and any(c.path == "sweep" for c in masked)
    est = [c for c in SC.CASES.values() if isinstance(c, SC.Case) and c.op in ("idw", "lwr")]
    assert {16, 17, 64, 65} <= {c.k for c in est} and any(c.k == c.n - 1 for c in est) and any(c.k == c.n for c in est)
    assert {1, 4, 5} <= {c.nz for c in est} and {1.0, 2.0, 3.0} <= {c.exponent for c in est if c.op == "idw"}
    assert any(c.metric == "haversine" for c in est) and any("missing" in c.expect for c in est)


SEARCHES = [(k, c) for k, c in SC.CASES.items() if isinstance(c, SC.Case)]


@pytest.mark.parametrize("key,case", SEARCHES, ids=["%s-%s" % (k[0], "_".join(map(str, k[1]))) for k, _ in SEARCHES])
def test_problem_is_exact_and_shows_the_edges_it_claims(key, case):
    """problem_of asserts the bit-width precondition; reference_lists asserts the haversine gaps (every query kept)."""
    p = SM.problem_of(case)
    idx, cnt, keys = SM.reference_lists(p)
    assert idx.shape == (len(p.check), case.k) and (len(p.check) == p.c.shape[0] or p.c.shape[0] > 4500)
    SM.assert_expectations(case, p, idx, cnt, keys)
    assert np.all((idx >= 0).sum(axis=1) == cnt)
    if case.op == "lwr":
        assert SM.design_condition(case, p, idx, cnt) < 1e6
