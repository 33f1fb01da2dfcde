"""The table tests/ik_kernel_cases.py against the indicator-kriging kernels the compiler emitted into the built library
(tools/kernel_census.py), and what the table promises, asserted on the numpy reference alone.  No GPU.

An arm added to ik_dispatch, ik_local_launch or ik_local_launch_kinds compiles a kernel the table lacks; an entry that
drifts to another kernel fails the restated dispatch; an entry that could not tell its kernel from the one of a
neighbouring kind fails the discrimination check."""
import os
import sys

import numpy as np
import pytest

from gss import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ik_kernel_cases as KC
import ik_ref
import kernel_census
import test_gpu_ik as G

LIVE = {key: fn for key, fn in KC.KERNELS.items() if not isinstance(fn, KC.UNREACHABLE)}
_REF = {}


def ref_of(key, kind=None):
    """The FP64 reference of an entry (of the entry with another kind in its place), computed once."""
    if (key, kind) not in _REF:
        c = KC.kernel_case(key, kind)
        _REF[key, kind] = (c, ik_ref.predict(c["x"], c["z"], c["x0"], c["cutoffs"], c["models"], c["k"], fstar=c["fstar"],
                                             radius=c["radius"]))
    return _REF[key, kind]


@pytest.fixture(scope="module")
def compiled():
    if not kernel_census.tools_present():
        pytest.skip("llvm-readelf or a C++ demangler not available")
    found = kernel_census.census(_lib.LIB_PATH)
    assert len(found) > 500, len(found)          # the library's kernels were found at all
    return found


def test_table_keys_are_the_compiled_instantiations(compiled):
    got = [(int(a[0]), int(a[1]), int(a[2]), {"true": True, "false": False}[a[3]])
           for f, a in compiled if f == "ik_local_kernel"]
    assert len(got) == len(set(got)) == 54
    assert set(got) == set(KC.KERNELS), (set(got) ^ set(KC.KERNELS))


def test_row_kernels_are_compiled(compiled):
    fams = {(f, a) for f, a in compiled}
    assert ("ik_post_kernel", ("false",)) in fams and ("ik_post_kernel", ("true",)) in fams
    assert ("ik_order_kernel", ()) in fams


def test_exclusions_are_reasoned():
    for key, entry in KC.KERNELS.items():
        if isinstance(entry, KC.UNREACHABLE):
            assert entry.reason.strip() and (".hip" in entry.reason or ".h" in entry.reason), key
        else:
            assert callable(entry), key
    assert len(LIVE) == 54                        # none is expected to be unreachable


def device_kind(g):
    """make_vgdev / gss_ik_predict_knn: the kind of a single structure, -1 for a nested model."""
    if g.kind == "nested":
        return -1 if len(g.terms) > 1 else device_kind(g.terms[0][1])
    if g.kind == "matern":
        return {0.5: 30, 1.5: 31, 2.5: 32}.get(g.nu, 33)
    return {"gaussian": 0, "exponential": 1, "spherical": 2}.get(g.kind, 99)


def kernel_of(c):
    """ik_dispatch (csrc/ik.hip) and ik_local_launch (csrc/ik_kernel.h), restated."""
    dim, K, nvg = c["x"].shape[1], len(c["cutoffs"]), len(c["models"])
    assert nvg in (1, K)
    full = nvg == K and K > 1
    kind = device_kind(c["models"][0])
    if full or dim == 1 or kind not in (0, 1, 2, 30, 31, 32):
        kind = -1
    nt = 1 if c["k"] <= 16 else (2 if c["k"] <= 32 else 4)
    assert c["k"] <= 64
    return dim, kind, nt, full


@pytest.mark.parametrize("key", list(LIVE))
def test_case_takes_its_own_kernel_and_keeps_its_promises(key):
    dim, kind, nt, full = key
    c, r = ref_of(key)
    assert kernel_of(c) == key
    n, m = c["x"].shape[0], c["x0"].shape[0]
    assert n <= 200 and m <= 67 and m % 4 != 0
    assert c["k"] == {1: 13, 2: 29, 4: 50}[nt] and c["k"] % 16 != 0
    cut, K = c["cutoffs"], len(c["cutoffs"])
    assert np.all(np.isin(cut, c["z"])) and np.all(np.diff(cut) > 0.0)
    if full:
        assert K == 3
        kinds = [g.kind for g in c["models"]]
        assert len(set(kinds)) == 3 and "nested" in kinds
    else:
        assert K == (16 if nt == 4 else 5)
        assert nt != 4 or c["fstar"] is None
    for g in c["models"]:
        assert g.nugget > 0.0 and g.sill != 1.0
    if nt == 2 and dim >= 2 and not full:
        structs = [s for _, s in c["models"][0].terms] if c["models"][0].kind == "nested" else c["models"]
        assert all(s.radii is not None and len(set(s.radii)) > 1 and s.rotation is None for s in structs)
    # what the reference alone shows
    cnt = r["cnt"]
    assert (cnt == c["k"]).any()
    assert (cnt % 16 != 0).any()
    if nt >= 2:
        assert ((cnt + 15) // 16 < nt).any()
    assert not r["status"].any() and np.isfinite(r["raw"]).all()


def test_variants_and_models_across_the_table():
    for dim in (1, 2, 3):
        for kind in (KC.KINDS if dim >= 2 else ()) + (-1,):
            for full in ((False, True) if kind == -1 else (False,)):
                simple = {LIVE[(dim, kind, nt, full)]()["fstar"] is not None for nt in (1, 2, 4)}
                assert simple == {False, True}, (dim, kind, full)
    general = [LIVE[(dim, -1, nt, False)]()["models"][0].kind for dim in (1, 2, 3) for nt in (1, 2, 4)]
    assert "nested" in general and "cubic" in general and "pentaspherical" in general
    assert all((a == "nested") != (b == "nested") for a, b in zip(general, general[1:]))
    for dim in (2, 3):                           # one full-form entry with a rotated member
        rot = [key for key in LIVE if key[0] == dim and key[3]
               and any(getattr(g, "rotation", None) is not None for g in LIVE[key]()["models"])]
        assert len(rot) == 1, (dim, rot)


@pytest.mark.parametrize("key", [k for k in LIVE if k[1] >= 0])
def test_case_tells_its_kind_from_the_neighbouring_one(key):
    """The reference under the neighbouring kind (same range or radii, sill and nugget) is at least 1000 bars away at
    some point and cutoff: the case would fail on the device if the dispatch took the other kernel."""
    c, r = ref_of(key)
    other = KC.NEIGHBOUR[key[1]]
    c2, r2 = ref_of(key, other)
    g, g2 = c["models"][0], c2["models"][0]
    assert kernel_of(c2)[1] == other != key[1]
    assert (g.range, g.radii, g.sill, g.nugget) == (g2.range, g2.radii, g2.sill, g2.nugget)
    assert np.array_equal(r["idx"], r2["idx"])
    gap = np.abs(r["raw"] - r2["raw"]) / (G.UNIT * r["wsum"])
    need = 1000.0 * G.bar(KC.name_of(key))
    print("%s: %.3g units from kind %d, needs %.3g" % (KC.name_of(key), gap.max(), other, need))
    assert gap.max() >= need
