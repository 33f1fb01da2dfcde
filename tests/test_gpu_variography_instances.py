"""Every compiled instantiation of the pair kernels of csrc/variography.hip run once on the device: the cases of
tests/vario_cases.py against the numpy restatements variography_ref, varioplane_ref and variography_cross_ref.

Bars.  Counts and nduplicates are compared exactly.  The values are integers with |z| <= 2^10, so Matheron sums and
sums of products are integers below 2^53 and are compared bit for bit (as in test_gpu_variography_cross.py).  Cressie
sums and lagsum keep the bar derived in test_gpu_variography.py: two FP64 sums of the same `count` non-negative terms
differ by at most 2 count 2^-53 S."""
import numpy as np
import pytest

import vario_cases as VC
import variography_cross_ref as cref
import variography_ref as vref
import varioplane_ref as pref

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EST = {"matheron": 0, "cressie": 1}


def _engine():
    from gss.engine import HipEngine
    return HipEngine


def check(dev, ref, exact):
    count, lagsum, zsum, ndup = dev[:4]
    rcount, rlagsum, rzsum, rndup = ref[:4]
    assert count.shape == rcount.shape and zsum.shape == rzsum.shape
    assert np.array_equal(count, rcount)
    assert ndup == rndup
    sums = [(lagsum, rlagsum)]
    if exact:
        assert np.array_equal(zsum, rzsum)                      # integers below 2^53: bit for bit
    else:
        sums += [(zsum[i], rzsum[i]) for i in range(zsum.shape[0])]
    for s_dev, s_ref in sums:
        bar = 2.0 * rcount * U * s_ref
        err = np.abs(s_dev - s_ref)
        assert (err <= bar).all(), (err, bar)


@pytest.mark.parametrize("key", sorted(VC.CASES), ids=VC.case_id)
def test_instance(key):
    c = VC.CASES[key]()
    assert VC.kernel_of(c) == key
    x, z, est = c["x"], c["z"], c["estimator"]
    for nlags, maxlag in c["calls"]:
        if c["form"] == "window":
            dev = _engine().variogram_empirical(x, z, nlags, maxlag, estimator=EST[est])
            ref = vref.empirical(x, z, nlags, maxlag, estimator=est)
        elif c["form"] == "plane":
            dev = _engine().variogram_plane(x, z, nlags, maxlag, c["dirs"], basis=c["basis"], ptol=c["ptol"],
                                            estimator=EST[est])
            ref = pref.plane(x, z, nlags, maxlag, c["dirs"], basis=c["basis"], ptol=c["ptol"], estimator=est)
        else:
            dev = _engine().variogram_cross(x, z, nlags, maxlag)
            ref = cref.cross(x, z, nlags, maxlag)
        assert ref[0].sum() > 0 and ref[3] == 1
        check(dev, ref, exact=est == "matheron")
