"""The case table tests/vario_cases.py without a device: the compiled instantiations of vario_window_kernel,
vario_plane_kernel and vario_cross_kernel (tools/kernel_census.py on the built library) are exactly its keys, every
case dispatches to the kernel it is filed under, and every case is what the table's docstring says it is (numpy
references only)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vario_cases as VC
import varioplane_ref as pref
import variography_ref as vref

from gss import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_every_compiled_instantiation_has_a_device_case_and_every_case_a_kernel():
    import kernel_census
    if not kernel_census.tools_present():
        pytest.skip("llvm-readelf / c++filt not available")
    compiled = [(fam, tuple(int(a) if a.isdigit() else a for a in args))
                for fam, args in kernel_census.census(_lib.LIB_PATH) if fam in VC.FAMILIES]
    assert len(compiled) == len(set(compiled)) == 88
    assert set(compiled) == set(VC.CASES)
    forms = {"window": 0, "plane": 0, "cross": 0}
    for key, fn in VC.CASES.items():                            # the case really dispatches to its kernel
        c = fn()
        assert VC.kernel_of(c) == key
        forms[c["form"]] += 1
    assert forms == {"window": 48, "plane": 16, "cross": 24}


@pytest.mark.parametrize("key", sorted(VC.CASES), ids=VC.case_id)
def test_case_is_what_it_claims(key):
    c = VC.CASES[key]()
    x, z = c["x"], c["z"]
    n, dim = x.shape
    assert n == 129 and np.array_equal(x, np.round(x)) and np.array_equal(z, np.round(z)) and np.abs(z).max() <= 1024
    nlags, maxlag = c["calls"][0]
    count, _, _, ndup = vref.empirical(x, z, nlags, maxlag)
    assert ndup == 1 and nlags == 7
    assert 0 < count.sum() < n * (n - 1) // 2 - ndup             # pairs within, and pairs beyond the last edge
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    assert np.isin(d2[np.triu_indices(n, 1)], vref.edges2(nlags, maxlag)[1:]).sum() > 10      # pairs exactly on an edge
    if c["form"] == "window":
        assert len(c["calls"]) == 2 and c["calls"][1][0] == 256
        assert VC.window_overflows(c, *c["calls"][1])
    if c["form"] == "plane":
        pc = pref.plane(x, z, nlags, maxlag, c["dirs"], basis=c["basis"], ptol=c["ptol"])[0]
        assert pc.shape == (5, 7) and (pc.sum(axis=1) > 0).all()
        if dim == 3:                                            # the basis is oblique and orthonormal, the slab filters
            e = c["basis"]
            assert np.abs(e @ e.T - np.eye(3)).max() <= 1e-12 and np.count_nonzero(np.abs(e) < 1e-12) <= 1
            assert 0 < pc.sum() < count.sum()
        else:
            assert pc.sum() == count.sum()
