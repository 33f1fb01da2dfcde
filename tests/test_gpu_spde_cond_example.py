"""examples/spde_conditional.py stays runnable and its numbers are sane."""
import os
import runpy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_spde_conditional_runs(capsys):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = runpy.run_path(os.path.join(root, "examples", "spde_conditional.py"))["out"]
    assert out["elements"].shape == (8, 1280) and out["mean"].shape == (1280,)
    assert np.isfinite(out["elements"]).all() and np.isfinite(out["mean"]).all()
    assert len(out["truth"]) == 40 and len(set(out["station_triangle"].tolist())) == 40
    # exact data: every realisation and the kriging mean carry the datum in its triangle (the solves stop at a relative
    # residual of 1e-10; the data-space system of 40 stations a range apart is well conditioned)
    assert out["misfit"] < 1e-6
    assert np.max(np.abs(out["mean"][out["station_triangle"]] - out["truth"])) < 1e-6
    # away from the stations the ensemble keeps a spread below the unconditional standard deviation (about 1.05 sill on
    # this mesh, tests/test_gpu_spde_example.py), and the mean stays between the prior mean and the data
    assert 0.2 * out["sill"] < out["spread"] < 1.2 * out["sill"]
    assert out["truth"].min() - out["sill"] < out["mean"].min() and out["mean"].max() < out["truth"].max() + out["sill"]
    # noisy data are not interpolated, but stay within a few error standard deviations (0.5)
    assert 0.05 < out["noisy_misfit"] < 1.5
    text = capsys.readouterr().out
    assert "642 vertices, 1280 triangles, 40 stations" in text and "kriging mean" in text
