"""BoundEvaluation (MPPIUtils.jl:135-151): the one-sided penalty form of bound_cost against the reference's
two-sided ordered accumulation, in numpy float64 with the device's operations in the device's order.

Reference, per state i = 0..6 in order:  c = lo ? c + slack*|x - XL| : c;  c = hi ? c + slack*|x - XU| : c.
One-sided (mppi_device.hpp):             b = lo ? XL : XU;  t = c + slack*|x - b|;  c = (lo | hi) ? t : c,
followed by the reference's second addition where lo and hi both hold -- which needs XL > XU.  With
XL <= XU that second addition never runs and the two forms must give the same bits; the last test shows that
the one-sided form alone is wrong for XL > XU, which is why the second addition stays."""
import numpy as np

N = 100_000


def _two_sided(x, xl, xu, slack):
    c = np.zeros(x.shape[0])
    for i in range(7):
        lo, hi = x[:, i] < xl[:, i], x[:, i] > xu[:, i]
        c = np.where(lo, c + slack * np.abs(x[:, i] - xl[:, i]), c)
        c = np.where(hi, c + slack * np.abs(x[:, i] - xu[:, i]), c)
    return c


def _one_sided(x, xl, xu, slack, second=False):
    c = np.zeros(x.shape[0])
    for i in range(7):
        lo, hi = x[:, i] < xl[:, i], x[:, i] > xu[:, i]
        b = np.where(lo, xl[:, i], xu[:, i])
        c = np.where(lo | hi, c + slack * np.abs(x[:, i] - b), c)
        if second:  # the device's guarded second addition (some lane of the wave has lo & hi)
            c = np.where(lo & hi, c + slack * np.abs(x[:, i] - xu[:, i]), c)
    return c


def _rows(seed):
    r = np.random.default_rng(seed)
    a, b = r.normal(0, 3, (N, 7)), r.normal(0, 3, (N, 7))
    xl, xu = np.minimum(a, b), np.maximum(a, b)
    xu[::17] = xl[::17]  # XL == XU rows
    x = r.normal(0, 6, (N, 7))
    on = r.random((N, 7))
    x = np.where(on < 0.1, xl, np.where(on < 0.2, xu, x))  # exactly on a bound: no violation
    x = np.where(r.random((N, 7)) < 0.02, np.nan, x)  # NaN states: both comparisons false
    x[::29] *= 1e150  # |x - b| large enough for the running sum to round
    slack = 10.0 ** r.uniform(-3, 8, N)
    return x, xl, xu, slack


def test_one_sided_is_two_sided_for_ordered_bounds():
    with np.errstate(invalid="ignore", over="ignore"):
        for seed in (1, 2):
            x, xl, xu, slack = _rows(seed)
            assert (xl <= xu).all()
            ref = _two_sided(x, xl, xu, slack)
            lo, hi = x < xl, x > xu
            assert lo.any() and hi.any() and not (lo & hi).any()
            assert ((x == xl) & ~lo).any() and ((x == xu) & ~hi).any() and np.isnan(x).any()
            assert (ref > 0).any() and (ref == 0).any()
            for second in (False, True):
                got = _one_sided(x, xl, xu, slack, second)
                assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))


def test_nan_bounds_penalise_nothing():
    x, xl, xu, slack = _rows(3)
    xl[:, 2], xu[:, 5] = np.nan, np.nan
    with np.errstate(invalid="ignore", over="ignore"):
        ref = _two_sided(x, xl, xu, slack)
        got = _one_sided(x, xl, xu, slack, True)
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))


def test_forms_differ_for_crossed_bounds():
    """XL > XU with x between them: below XL and above XU at once, two additions in the reference."""
    x = np.zeros((1, 7))
    xl, xu = np.full((1, 7), -1.0), np.full((1, 7), 1.0)
    xl[0, 3], xu[0, 3] = 0.5, -0.25
    slack = np.array([1e5])
    ref = _two_sided(x, xl, xu, slack)
    assert ref[0] == 1e5 * 0.5 + 1e5 * 0.25
    assert _one_sided(x, xl, xu, slack)[0] != ref[0]
    assert np.array_equal(_one_sided(x, xl, xu, slack, True).view(np.uint64), ref.view(np.uint64))
