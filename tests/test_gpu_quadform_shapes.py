"""Global kriging at the shapes that select the specialisations of the quadratic-form kernel (K3).

K3 walks the rows 0 .. N1 of W' (N1 = n + nc, row N1 = dual weights) in blocks of 128 rows made of eight 16-row
tiles.  The last row block is compiled once per number of live tiles (1 .. 8), the diagonal block of every row block
is an unrolled sequence of stages with a constant first live tile, and a call uses two launch forms: whole strips for
each full round of 512 x 128 points and (strip, row block) units plus a finishing kernel for the rest.  Every case is
compared with `oracle.kriging.exactsolve` at the tolerances of tests/test_gpu_krig_global.py: 1e-9 relative on the
mean, 1e-9 absolute on the variance (sill = 1), status all zero."""
import numpy as np
import pytest

from oracle import kriging as K
from oracle.variogram import Variogram

pytestmark = pytest.mark.gpu

BM, TILE = 128, 16
NC = {K.SK: 0, K.OK: 1}


def _shape(n, nc):
    """(row blocks, live 16-row tiles of the last row block) for n data and nc constraints."""
    rows = n + nc + 1
    nI = (n + nc) // BM + 1
    return nI, -(-(rows - BM * (nI - 1)) // TILE)


def _n_for(nI, live, r, nc):
    """Data count whose last row block (of nI) has `live` tiles, the last of them holding r of its 16 rows."""
    assert 1 <= r <= TILE
    n = BM * (nI - 1) + TILE * (live - 1) + r - nc - 1
    assert _shape(n, nc) == (nI, live)
    return n


def _problem(n, m, dim, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 100, (n, dim))
    z = rng.normal(size=n)
    x0 = rng.uniform(0, 100, (m, dim))
    x0[:3] = x[:3]
    return x, z, x0


def _check(variant, x, z, x0, sample=None, **okw):
    """Device against oracle on all of x0, or on the rows `sample` of it."""
    import gss
    from gss.engine import KrigHandle
    h = KrigHandle(gss.MaternVariogram(range=30.0, order=1.5), variant, x, z, mean=okw.get("mean"),
                   degree=okw.get("degree"))
    mu, var, st = h.predict_global(x0)
    h.close()
    assert mu.shape == var.shape == st.shape == (len(x0),)
    assert not st.any()
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(var))
    if sample is not None:
        mu, var, x0 = mu[sample], var[sample], x0[sample]
    rmu, rvar = K.exactsolve(variant, Variogram("matern", range=30.0, nu=1.5), x, z, x0, mean=okw.get("mean") or 0.0,
                             degree=okw.get("degree"))
    emu = np.max(np.abs(mu - rmu)) / max(1.0, np.max(np.abs(rmu)))
    evar = np.max(np.abs(var - rvar))
    print(f"n={len(x)} m={len(x0)} mean err (rel) {emu:.3e}  variance err (abs) {evar:.3e}")
    assert emu < 1e-9
    assert evar < 1e-9
    return mu, var


# (row blocks, live tiles, rows in the last live tile): r = 1 puts the dual-weight row alone into its tile, r = 16
# fills the tile; live = 1 with r = 1 leaves the mean row as the only row of the last row block
LAST_BLOCK = [(2, 1, 1), (2, 2, 16), (3, 3, 5), (2, 4, 9), (2, 5, 1), (3, 6, 16), (2, 7, 10), (2, 8, 7), (2, 8, 16)]


@pytest.mark.parametrize("nI,live,r", LAST_BLOCK)
def test_ordinary_kriging_for_every_live_tile_count_of_the_last_row_block(nI, live, r):
    n = _n_for(nI, live, r, NC[K.OK])
    x, z, x0 = _problem(n, 1500, 3, seed=1000 * nI + 16 * live + r)
    mu, var = _check(K.OK, x, z, x0)
    assert np.allclose(mu[:3], z[:3], atol=1e-9) and np.all(var[:3] < 1e-9)     # exact at data


@pytest.mark.parametrize("nI,live,r", [(2, 1, 1), (3, 5, 3)])
def test_simple_kriging_has_no_constraint_row(nI, live, r):
    n = _n_for(nI, live, r, NC[K.SK])
    x, z, x0 = _problem(n, 1500, 3, seed=77 + live)
    _check(K.SK, x, z, x0, mean=0.7)


def test_bench_shape_n1000_ordinary():
    assert _shape(1000, 1) == (8, 7)            # 1 002 rows: seven live tiles in the eighth row block
    x, z, x0 = _problem(1000, 3000, 3, seed=1003)
    _check(K.OK, x, z, x0)


def test_universal_degree2_3d_constraint_rows_straddle_a_tile():
    """nc = 10 monomials: the negative-signed rows n .. n + 9 lie on both sides of row 304 = 19 x 16."""
    n, nc = 299, 10
    assert n < 304 < n + nc - 1 and _shape(n, nc) == (3, 4)
    x, z, x0 = _problem(n, 2000, 3, seed=299)
    _check(K.UK, x, z, x0, degree=2)


def test_remainder_units_only_and_main_launch_plus_remainder():
    """m < 128 x 512 runs as (strip, row block) units alone; m slightly above adds the launch of whole strips in front
    of them and the finishing kernel behind: there a seeded sample of 200 points, taken from both parts, goes to the
    oracle."""
    n = _n_for(2, 7, 10, NC[K.OK])
    full = BM * 512
    m = full + 300
    x, z, x0 = _problem(n, m, 3, seed=4242)
    rng = np.random.default_rng(5)
    sample = np.sort(np.r_[rng.choice(full, 150, replace=False), full + rng.choice(300, 50, replace=False)])
    _check(K.OK, x, z, x0, sample=sample)
    small = np.sort(rng.choice(full, 2500, replace=False))
    _check(K.OK, x, z, x0[small])
