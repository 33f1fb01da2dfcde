"""The quadratic-form kernel (K3) alone, through KrigHandle.predict_global, against oracle.kriging.exactsolve at the
tolerance of the global-kriging tests (1e-9).  The shapes are the smallest that reach every path of the kernel:

* the last 128-row block with each live-tile count 1 .. 8 (OK has n + 2 rows: ceil((n + 2 - 128) / 16) tiles),
  n = 190 being an exact multiple of 16 rows in that block;
* one row block only (n = 100: the block that opens the accumulators also holds row n and the mean row N1);
* three row blocks (n = 300: an interior block, whose epilogue is a plain sum of squares);
* SK / OK / UK with a linear drift in 3-D (0, 1 and 4 constraint rows), which move the sign change at row n and the
  mean row N1 to other tiles and other rows of a tile;
* point counts around one 128-point strip for the (strip, row block) form, and 65 536 + 200 points: one full round of
  512 strips through the one-workgroup-per-strip form plus a remainder."""
import numpy as np
import pytest

from oracle import kriging as K
from oracle.variogram import Variogram

pytestmark = pytest.mark.gpu

KW = dict(range=30.0, nu=1.5)


def _check(variant, n, m, seed, ref_idx=None, **okw):
    import gss
    from gss.engine import KrigHandle
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 100, (n, 3))
    z = rng.normal(size=n)
    x0 = rng.uniform(0, 100, (m, 3))
    h = KrigHandle(gss.MaternVariogram(range=KW["range"], order=KW["nu"]), variant, x, z, mean=okw.get("mean"),
                   degree=okw.get("degree"))
    mu, var, st = h.predict_global(x0)
    h.close()
    mu, var, st = np.asarray(mu), np.asarray(var), np.asarray(st)
    assert mu.shape == (m,) and var.shape == (m,)
    assert not st.any()
    assert np.all(var >= 0.0)
    idx = np.arange(m) if ref_idx is None else ref_idx
    rmu, rvar = K.exactsolve(variant, Variogram("matern", **KW), x, z, x0[idx], mean=okw.get("mean") or 0.0,
                             degree=okw.get("degree"))
    emu, evar = np.max(np.abs(mu[idx] - rmu)), np.max(np.abs(var[idx] - rvar))
    print(f"n={n} m={m} max|mean err|={emu:.3e} max|var err|={evar:.3e}")
    assert emu < 1e-9 * max(1.0, np.max(np.abs(rmu)))
    assert evar < 1e-9


@pytest.mark.parametrize("n", [130, 150, 170, 190, 200, 220, 230, 250])
def test_last_row_block_with_each_live_tile_count(n):
    assert (n + 2 - 128 + 15) // 16 == [130, 150, 170, 190, 200, 220, 230, 250].index(n) + 1
    _check(K.OK, n, 129, seed=n)


def test_one_row_block():
    _check(K.OK, 100, 129, seed=100)


def test_three_row_blocks():
    _check(K.OK, 300, 129, seed=300)


@pytest.mark.parametrize("variant,okw", [(K.SK, dict(mean=0.7)), (K.OK, {}), (K.UK, dict(degree=1))])
@pytest.mark.parametrize("n", [150, 300])
def test_drift_rows(variant, okw, n):
    _check(variant, n, 200, seed=7 * n, **okw)


@pytest.mark.parametrize("m", [1, 127, 128, 129, 1000])
def test_point_counts_of_the_split_form(m):
    _check(K.OK, 150, m, seed=m)


def test_both_launch_forms():
    m = 65536 + 200
    # the oracle on the head of the main launch, its last strip and the whole remainder
    idx = np.concatenate([np.arange(0, 200), np.arange(65536 - 128, m)])
    _check(K.OK, 300, m, seed=11, ref_idx=idx)
