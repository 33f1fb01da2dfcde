"""examples/indicator_kriging.py stays runnable: declustering weights, F*, median indicator kriging and postik."""
import os
import runpy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_indicator_kriging_example_runs_and_its_results_are_sane():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ns = runpy.run_path(os.path.join(root, "examples", "indicator_kriging.py"))
    out = ns["out"]
    assert out["ccdf"].shape == (1600, 6) and np.isfinite(out["ccdf"]).all()
    assert np.isfinite(out["etype"]).all() and (out["etype"] > 0.0).all()
    assert ((out["pabove"] >= 0.0) & (out["pabove"] <= 1.0)).all()
