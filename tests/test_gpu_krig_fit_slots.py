"""Fit status slots of the process (gss_internal.h, FitSlot): a kriging handle borrows its pinned status words and its
events from a free list instead of allocating them; gss_stat "fit_slot_allocs" counts the pinned allocations."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _problem(seed, n=40, m=256):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 100, (n, 2)), rng.normal(size=n), rng.uniform(0, 100, (m, 2))


def _vg():
    import gss
    return gss.MaternVariogram(range=30.0, order=1.5)


def test_steady_state_allocates_no_slot():
    from gss import _lib
    from gss.engine import KrigHandle, OK
    x, z, x0 = _problem(1)
    after3 = None
    for i in range(50):
        h = KrigHandle(_vg(), OK, x, z, async_fit=True)
        h.predict_global(x0)
        h.close()
        if i == 2:
            after3 = _lib.stat("fit_slot_allocs")
    assert after3 >= 1 and _lib.stat("fit_slot_allocs") == after3


def test_two_fits_in_flight_keep_their_own_status():
    import gss
    from gss import _lib
    from gss.engine import KrigHandle, OK
    x, z, x0 = _problem(2)
    xb = x.copy()
    xb[7] = xb[3]                                        # duplicated datum, zero nugget: not positive definite
    good = KrigHandle(_vg(), OK, x, z, async_fit=True)
    bad = KrigHandle(gss.GaussianVariogram(range=20.0, nugget=0.0), OK, xb, z, async_fit=True)
    with pytest.raises(_lib.GSSError) as e:
        bad.predict_global(x0)                            # joined in the opposite order to their creation
    assert e.value.code == _lib.ERR_NOT_POSDEF
    mu, var, st = good.predict_global(x0)
    ref = KrigHandle(_vg(), OK, x, z)
    rmu, rvar, rst = ref.predict_global(x0)
    assert np.array_equal(mu, rmu) and np.array_equal(var, rvar) and not st.any()
    for h in (good, bad, ref):
        h.close()


def test_handle_closed_with_its_fit_never_joined():
    from gss.engine import KrigHandle, OK
    x, z, x0 = _problem(3)
    KrigHandle(_vg(), OK, x, z, async_fit=True).close()  # the slot goes back after the handle waited for its own fit
    h = KrigHandle(_vg(), OK, x, z, async_fit=True)
    mu, var, st = h.predict_global(x0)
    ref = KrigHandle(_vg(), OK, x, z)
    rmu, rvar, rst = ref.predict_global(x0)
    assert np.array_equal(mu, rmu) and np.array_equal(var, rvar) and np.array_equal(st, rst)
    h.close()
    ref.close()
