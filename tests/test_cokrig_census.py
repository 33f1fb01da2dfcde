"""The table tests/cokrig_kernel_cases.py against the global-cokriging kernels the compiler emitted into the built library
(tools/kernel_census.py), the conditioning cap the 1e-9 bar rests on, and what the table promises.  No GPU.

An arm added to launch_cokrig_rhs or launch_cokrig_batch_mean compiles a kernel the table lacks; an entry whose
reference could not tell its kind from a neighbouring one fails the discrimination check."""
import os
import sys

import numpy as np
import pytest

from gss import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cokrig_cases as CC
import cokrig_kernel_cases as KC
import cokrig_ref as CR
import kernel_census

KEYS = sorted(KC.KERNELS)


@pytest.fixture(scope="module")
def compiled():
    if not kernel_census.tools_present():
        pytest.skip("llvm-readelf or a C++ demangler not available")
    found = kernel_census.census(_lib.LIB_PATH)
    assert len(found) > 500, len(found)          # the library's kernels were found at all
    return found


@pytest.mark.parametrize("family", ["cokrig_rhs_kernel", "cokrig_batch_mean_kernel"])
def test_table_keys_are_the_compiled_instantiations(compiled, family):
    got = [tuple(int(v) for v in a) for f, a in compiled if f == family]
    assert len(got) == len(set(got)) == 21
    assert set(got) == set(KC.KERNELS), (family, set(got) ^ set(KC.KERNELS))


def test_system_kernel_is_compiled_for_every_dimension(compiled):
    assert sorted(a for f, a in compiled if f == "cokrig_system_kernel") == [("1",), ("2",), ("3",)]


def device_kind(s):
    """device_kind of csrc/common.hip on the structure keywords: what both launchers switch on."""
    if s["kind"] == "matern":
        return {0.5: 30, 1.5: 31, 2.5: 32}.get(s.get("nu"), -1)
    return {"gaussian": 0, "exponential": 1, "spherical": 2}.get(s["kind"], -1)


@pytest.mark.parametrize("key", KEYS)
def test_case_takes_its_own_kernel_and_keeps_its_promises(key):
    dim, kind = key
    c = KC.KERNELS[key]()
    assert (c["x"].shape[1], device_kind(c["structure"])) == key
    n, m, nz = c["x"].shape[0], c["xdom"].shape[0], c["B1"].shape[0]
    assert 60 <= n <= 100 and nz in (2, 3) and m > 512 and m % 2 == 1
    counts = np.bincount(c["var"], minlength=nz)
    assert counts.min() > 0 and len(set(counts)) == nz                      # heterotopic, unequal counts
    assert np.unique(c["x"], axis=0).shape[0] == n                          # one variable per location
    assert np.any(np.diff(c["var"]) < 0)                                    # shuffled row order
    assert np.all(c["B0"] > 0.0) and np.all(np.linalg.eigvalsh(c["B0"]) > 0.0)
    assert abs(np.max(np.diag(c["B0"]) + np.diag(c["B1"])) - 1.0) < 1e-15
    on = c["on"]
    assert on.size >= 2 and np.array_equal(c["xdom"][:on.size], c["x"][on])
    assert (c["variant"] == "simple") == (c["means"] is not None)
    if c["means"] is not None:
        assert len(set(c["means"])) == nz


def test_variants_alternate_and_three_variables_occur_in_every_dimension():
    variants = [KC.KERNELS[key]()["variant"] for key in sorted(KC.KERNELS, key=lambda k: (k[0], KC.KINDS.index(k[1])))]
    assert all(a != b for a, b in zip(variants, variants[1:]))
    for dim in (1, 2, 3):
        assert any(KC.KERNELS[(dim, kind)]()["B1"].shape[0] == 3 for kind in KC.KINDS)
    general = {KC.KERNELS[(dim, -1)]()["structure"]["kind"] for dim in (1, 2, 3)}
    assert general == {"cubic", "pentaspherical"}


@pytest.mark.parametrize("key", KEYS)
def test_conditioning_cap(key):
    """The cap is a condition of the 1e-9 bar: every entry, the Gaussian ones too, stays under it."""
    c = KC.KERNELS[key]()
    ev = np.linalg.eigvalsh(c["B1"])
    assert ev[0] >= 0.05 * ev[-1]
    k = CR.cond(KC.model_of(c), c["x"], c["var"], c["variant"])
    print(key, "cond_2 = %.3g" % k)
    assert k <= CC.COND_CAP


@pytest.mark.parametrize("key", KEYS)
def test_case_tells_its_kind_from_the_neighbouring_one(key):
    """The reference under a neighbouring kind of the same range is at least 1000 bars away somewhere: the case would
    fail on the device if a launcher took the other kernel."""
    c = KC.KERNELS[key]()
    c2 = KC.kernel_case(*key, structure=KC.NEIGHBOUR[key[1]])
    assert device_kind(c2["structure"]) != key[1] and c2["structure"]["range"] == c["structure"]["range"]
    assert np.array_equal(c["x"], c2["x"]) and np.array_equal(c["z"], c2["z"])
    mu, var = CR.predict(KC.model_of(c), c["x"], c["z"], c["var"], c["xdom"], c["variant"], c["means"])
    mu2, var2 = CR.predict(KC.model_of(c2), c["x"], c["z"], c["var"], c["xdom"], c["variant"], c["means"])
    gap_mu = float(np.max(np.abs(mu - mu2) / (1.0 + np.abs(mu))))
    gap_var = float(np.max(np.abs(var - var2) / (1.0 + np.abs(var))))
    print(key, "mean gap %.3g, variance gap %.3g, needs %.3g" % (gap_mu, gap_var, 1000.0 * CC.TOL))
    assert gap_mu >= 1000.0 * CC.TOL and gap_var >= 1000.0 * CC.TOL
