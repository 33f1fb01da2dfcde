"""examples/spde_sphere.py stays runnable and its numbers are sane."""
import os
import runpy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_spde_sphere_runs(capsys):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = runpy.run_path(os.path.join(root, "examples", "spde_sphere.py"))["out"]
    assert out["elements"].shape == (8, 1280) and out["values"].shape == (8, 642)
    assert np.isfinite(out["elements"]).all() and np.isfinite(out["values"]).all()
    assert len(out["iterations"]) == 8 and all(1 <= k < 1000 for k in out["iterations"])
    # The vertex variance of this discretisation, tau^2 diag(inv(S) M inv(S)) from tests/spde_ref.py, is 1.09 .. 1.14
    # sill^2 on this mesh (its width, 0.15, is half the range).  8 fields with a correlation length of 0.3 on a sphere
    # of area 4 pi are some 8 * 4 pi / (pi 0.3^2) ~ 350 independent patches: the sample variance scatters by
    # sqrt(2 / 350) ~ 8 % around that, and four such deviations on either side give the interval.
    assert 0.8 * out["sill2"] < out["variance"] < 1.5 * out["sill2"]
    text = capsys.readouterr().out
    assert "642 vertices, 1280 triangles" in text and "CG iterations per realisation" in text
