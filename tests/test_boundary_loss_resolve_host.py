"""loss.resolve_boundary, the pure function between FCN8s.train(boundary_*) and Engine.set_boundary_loss: every row of its rule, the combined
table against the elementwise rule, the radius defaults and every ValueError.  No GPU."""
import numpy as np
import pytest

from fcn8s_tensorflow_amd import loss as LM


def test_nothing_is_off():
    assert LM.resolve_boundary() == (None, 0)
    assert LM.validate_boundary(*LM.resolve_boundary()) == (None, 0)


@pytest.mark.parametrize("weight,sigma,radius", [(10, 2, 6), (10.0, 5.0, 15), (0, 1.5, 1), (3.5, 0.7, 4)])
def test_weight_and_sigma_give_the_unet_table(weight, sigma, radius):
    T, R = LM.resolve_boundary(weight=weight, sigma=sigma, radius=radius)
    assert R == radius and T.dtype == np.float32 and T.shape == (256,)
    np.testing.assert_array_equal(T, LM.boundary_table(weight, sigma, radius))
    d2 = np.arange(1, R * R + 1, dtype=np.float64)
    np.testing.assert_array_equal(T[1:R * R + 1], (1.0 + weight * np.exp(-d2 / (2.0 * sigma * sigma))).astype(np.float32))
    assert (T[R * R + 1:] == 1.0).all() and T[0] == 1.0
    np.testing.assert_array_equal(LM.validate_boundary(T, R)[0], T)


@pytest.mark.parametrize("sigma,expected", [(0.1, 1), (1.0, 3), (2, 6), (2.5, 8), (4.9, 15), (5.0, 15), (40.0, 15)])
def test_the_radius_defaults_to_three_sigma_capped_at_15(sigma, expected):
    assert LM.default_boundary_radius(sigma) == expected
    T, R = LM.resolve_boundary(weight=10, sigma=sigma)
    assert R == expected
    np.testing.assert_array_equal(T, LM.boundary_table(10, sigma, expected))


@pytest.mark.parametrize("k", [1, 2, 7, 15])
def test_ignore_band_alone(k):
    T, R = LM.resolve_boundary(ignore_band=k)
    assert R == k
    np.testing.assert_array_equal(T, LM.ignore_band_table(k))
    assert (T[1:k * k + 1] == 0.0).all() and T[0] == 1.0 and (T[k * k + 1:] == 1.0).all()


@pytest.mark.parametrize("weight,sigma,radius,k,R", [(10, 2, None, 2, 6), (10, 2, 6, 2, 6), (10, 2, 3, 5, 5), (4, 1, None, 3, 3), (4, 0.5, None, 9, 9),
                                                     (7, 3, 15, 15, 15), (7, 3, 4, 4, 4)])
def test_both_zero_the_band_inside_the_unet_table(weight, sigma, radius, k, R):
    T, got = LM.resolve_boundary(weight=weight, sigma=sigma, radius=radius, ignore_band=k)
    assert got == R == max(radius if radius is not None else LM.default_boundary_radius(sigma), k)
    U = LM.boundary_table(weight, sigma, R)
    code = np.arange(256)
    band = (code >= 1) & (code <= k * k)
    np.testing.assert_array_equal(T, np.where(band, np.float32(0.0), U))            # the elementwise rule
    assert (T[band] == 0.0).all()
    if k < R:
        assert (T[k * k + 1:R * R + 1] > 1.0).all()                                # the Gaussian outside the band is kept
    np.testing.assert_array_equal(LM.validate_boundary(T, got)[0], T)


@pytest.mark.parametrize("kw", [
    dict(weight=10), dict(sigma=2), dict(weight=10, radius=4), dict(sigma=2, radius=4), dict(sigma=2, ignore_band=2), dict(weight=1, ignore_band=2),
    dict(radius=4), dict(radius=4, ignore_band=2),
    dict(weight=10, sigma=2, radius=0), dict(weight=10, sigma=2, radius=16), dict(weight=10, sigma=2, radius=2.5), dict(weight=10, sigma=2, radius=True),
    dict(weight=-1, sigma=2), dict(weight=float("nan"), sigma=2), dict(weight=float("inf"), sigma=2, radius=3), dict(weight="much", sigma=2, radius=3),
    dict(weight=10, sigma=0), dict(weight=10, sigma=-2), dict(weight=10, sigma=float("nan")), dict(weight=10, sigma=float("inf")),
    dict(weight=10, sigma="wide"), dict(weight=10, sigma=0, radius=3), dict(weight=10, sigma=float("nan"), radius=3),
    dict(ignore_band=0), dict(ignore_band=16), dict(ignore_band=-1), dict(ignore_band=1.5), dict(ignore_band=True),
    dict(weight=10, sigma=2, ignore_band=16), dict(weight=10, sigma=2, ignore_band=0),
])
def test_everything_else_is_a_value_error(kw):
    with pytest.raises(ValueError):
        LM.resolve_boundary(**kw)


def test_positional_order_is_weight_sigma_radius_ignore_band():
    T, R = LM.resolve_boundary(10, 2, 6, 2)
    T2, R2 = LM.resolve_boundary(weight=10, sigma=2, radius=6, ignore_band=2)
    assert R == R2 == 6
    np.testing.assert_array_equal(T, T2)
