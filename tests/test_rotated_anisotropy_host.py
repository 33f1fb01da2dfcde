"""Rotated anisotropy, host side: MetricBall rotations, the model field, the C struct and the frame helper."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "geostatssolvers.jl_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gss  # noqa: E402
from gss import _lib  # noqa: E402
from gss.engine import _vg_struct  # noqa: E402
from rotated_frame import frame, mahalanobis_sq, rot2, rot3  # noqa: E402


def test_metricball_refuses_bad_rotations():
    with pytest.raises(ValueError, match="orthonormal"):
        gss.MetricBall((2.0, 1.0), [[1.0, 0.1], [0.0, 1.0]])
    with pytest.raises(ValueError, match="det"):
        gss.MetricBall((2.0, 1.0), [[1.0, 0.0], [0.0, -1.0]])
    with pytest.raises(ValueError, match="2 x 2"):
        gss.MetricBall((2.0, 1.0), np.eye(3))
    with pytest.raises(ValueError, match="angle"):
        gss.MetricBall((3.0, 2.0, 1.0), 0.5)


def test_angle_gives_the_counter_clockwise_matrix():
    b = gss.MetricBall((20.0, 5.0), np.pi / 6)
    assert np.array_equal(np.array(b.rotation), rot2(np.pi / 6))


def test_identity_and_isotropic_rotations_normalise_to_none():
    assert gss.MetricBall((2.0, 1.0), np.eye(2)).rotation is None
    assert gss.MetricBall((2.0, 1.0), 0.0).rotation is None
    assert gss.MetricBall(3.0, 0.7).rotation is None
    assert gss.MetricBall((5.0, 5.0), 0.3) == gss.MetricBall((5.0, 5.0))           # a sphere: any rotation
    assert gss.MetricBall((2.0, 1.0), np.eye(2)) == gss.MetricBall((2.0, 1.0))
    assert gss.GaussianVariogram(gss.MetricBall((2.0, 1.0), np.eye(2))) == gss.GaussianVariogram(gss.MetricBall((2.0, 1.0)))


def test_model_carries_the_rotation():
    R = rot3(0.3, -0.2, 0.9)
    g = gss.SphericalVariogram(gss.MetricBall((30.0, 10.0, 5.0), R), sill=2.0)
    assert np.array_equal(np.array(g.rotation), R)
    assert g.radii == (30.0, 10.0, 5.0)


def test_nested_model_with_different_rotations_is_refused():
    a = gss.GaussianVariogram(gss.MetricBall((20.0, 5.0), 0.3))
    b = gss.ExponentialVariogram(gss.MetricBall((10.0, 2.0), 0.4))
    with pytest.raises(ValueError, match="different rotations"):
        a + b
    ok = a + gss.ExponentialVariogram(range=4.0) + gss.SphericalVariogram(gss.MetricBall((8.0, 3.0), 0.3))
    assert ok.rotation == a.rotation


def test_struct_carries_aniso_2_and_the_rotation():
    R = rot2(0.4)
    v = _vg_struct(gss.GaussianVariogram(gss.MetricBall((20.0, 5.0), R)), 2)
    assert v.aniso == 2
    R3 = np.array(v.rotation[:]).reshape(3, 3)
    assert np.array_equal(R3[:2, :2], R) and np.array_equal(R3[2], [0, 0, 1]) and R3[0, 2] == 0 and R3[1, 2] == 0
    assert np.allclose(v.inv_radii[:2], [1 / 20.0, 1 / 5.0])
    nested = gss.GaussianVariogram(gss.MetricBall((20.0, 5.0), R)) + gss.ExponentialVariogram(range=3.0)
    v = _vg_struct(nested, 2)
    assert v.aniso == 2 and v.nextra == 1 and v.extra[0].aniso == 0
    # an axis-aligned model leaves the appended field at the identity and aniso at 1
    v = _vg_struct(gss.GaussianVariogram(gss.MetricBall((20.0, 5.0))), 2)
    assert v.aniso == 1 and list(v.rotation) == list(np.eye(3).ravel())
    spec = _lib.rotated_ball_spec((20.0, 5.0), R)
    assert spec.shape == (12,) and spec[2] == 1.0 and np.array_equal(spec[3:].reshape(3, 3)[:2, :2], R)


@pytest.mark.parametrize("d", [2, 3])
def test_frame_helper_matches_mahalanobis(d):
    rng = np.random.default_rng(d)
    R = rot2(0.7) if d == 2 else rot3(0.4, 1.1, -0.3)
    r = np.array([30.0, 8.0, 3.0][:d])
    x = rng.uniform(-50, 50, (40, d))
    y = rng.uniform(-50, 50, (30, d))
    fx, fy = frame(x, R), frame(y, R, c=x[0])
    d2 = (((fx[:, None, :] - fy[None, :, :]) / r) ** 2).sum(-1)
    ref = mahalanobis_sq(x, y, r, R)
    assert np.max(np.abs(d2 - ref) / np.maximum(1.0, np.abs(ref))) < 1e-13


def test_rotated_and_axis_aligned_anisotropic_structures_do_not_mix():
    rot = gss.SphericalVariogram(gss.MetricBall((30.0, 5.0), 0.5))
    with pytest.raises(ValueError, match="axis-aligned"):
        rot + gss.ExponentialVariogram(gss.MetricBall((4.0, 20.0)))
    # isotropic structures, spheres included, do not depend on the frame
    ok = rot + gss.ExponentialVariogram(gss.MetricBall((4.0, 4.0))) + gss.GaussianVariogram(range=3.0)
    v = _vg_struct(ok, 2)
    assert v.aniso == 2 and v.extra[0].aniso == 1 and v.extra[1].aniso == 0
    with pytest.raises(ValueError, match="axis-aligned"):
        _lib.make_variogram("spherical", 2, radii=(30.0, 5.0), rotation=rot.rotation,
                            extras=[("exponential", 1.0, 1.0, 1.0, (4.0, 20.0))])
