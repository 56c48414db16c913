"""The long double reference of the summary statistics (tests/stats_common.py) pinned on the CPU: against exact rational arithmetic,
against numpy where numpy has the same definition, against the numpy host function of the API mirror, and the bound it states against
a numpy emulation of the device's summation order.  The device's kernels are held to it in tests/test_gpu_statistics.py."""
from fractions import Fraction

import numpy as np
import pytest

import stats_common as sc


def test_ref_cov_against_exact_rational_arithmetic():
    """three particles, two states, one weight zero (n = 2, not 3), weights that sum to one and to two — by hand in Fractions (dyadic
    throughout, so that fp64 holds every exact value)"""
    for scale in (1, 2):
        _rational_case(scale)


def _rational_case(scale):
    x = [[Fraction(1), Fraction(5, 2)], [Fraction(-7, 4), Fraction(3)], [Fraction(9), Fraction(-11, 8)]]
    we = [scale * Fraction(3, 8), Fraction(0), scale * Fraction(5, 8)]
    s = sum(we)
    n = sum(1 for w in we if w != 0)
    mu = [sum(w * xi[d] for w, xi in zip(we, x)) / s for d in range(2)]
    corr = Fraction(n) / ((n - 1) * s)
    C = [[corr * sum(w * (xi[r] - mu[r]) * (xi[c] - mu[c]) for w, xi in zip(we, x)) for c in range(2)] for r in range(2)]
    A = [[corr * sum(w * abs(xi[r] - mu[r]) * abs(xi[c] - mu[c]) for w, xi in zip(we, x)) for c in range(2)] for r in range(2)]
    xf, wf = np.array([[float(v) for v in xi] for xi in x]), np.array([float(w) for w in we])       # dyadic: exact in fp64
    Cr, Ar = sc.ref_cov(xf, wf)
    np.testing.assert_array_equal(Cr, np.array([[float(v) for v in row] for row in C]))             # dyadic results too: to the bit
    np.testing.assert_array_equal(Ar, np.array([[float(v) for v in row] for row in A]))
    # mu_0 = 3/8 + 45/8 = 6, deviations -5 and 3, scatter 75/8 + 45/8 = 15, correction 2 / (1 * 1)
    assert n == 2 and C[0][1] == C[1][0] and C[0][0] == 30
    m, am = sc.ref_mean(xf, wf)
    np.testing.assert_array_equal(m, [float(sum(w * xi[d] for w, xi in zip(we, x))) for d in range(2)])        # not divided by the sum
    np.testing.assert_array_equal(am, [float(sum(w * abs(xi[d]) for w, xi in zip(we, x))) for d in range(2)])


@pytest.mark.parametrize("N,nx", [(2, 1), (3, 2), (257, 3), (5000, 16)])
def test_ref_cov_with_equal_weights_is_numpys_cov(N, nx):
    rng = np.random.default_rng(N + nx)
    x = rng.standard_normal((N, nx)) + 3.0
    for w in (np.full(N, 1.0 / N), np.full(N, 0.37)):                   # the correction divides by the sum: any equal weight
        C, A = sc.ref_cov(x, w)
        np.testing.assert_allclose(C, np.cov(x.T).reshape(nx, nx), rtol=1e-12, atol=0)
        assert np.all(np.abs(C) <= A * (1 + 1e-15)) and np.array_equal(C, C.T) and np.array_equal(A, A.T)
    m, am = sc.ref_mean(x, np.full(N, 1.0 / N))
    np.testing.assert_allclose(m, x.mean(axis=0), rtol=1e-14)
    assert np.all(np.abs(m) <= am)


def test_one_particle_with_weight_gives_nan_everywhere():
    """n = 1: the scatter matrix is exactly 0 and the correction n / ((n - 1) sum we) is inf — NaN in every entry, the reference's formula"""
    x = np.array([[1.5, -2.0, 7.0], [0.25, 3.0, 1.0], [9.0, 9.0, 9.0]])
    for we in (np.array([0.0, 1.0, 0.0]), np.array([1.0])):
        C, A = sc.ref_cov(x[:len(we)], we)
        assert C.shape == (3, 3) and np.all(np.isnan(C)) and np.all(np.isnan(A))
        import llpf_amd
        with np.errstate(divide="ignore", invalid="ignore"):
            assert np.all(np.isnan(llpf_amd.weighted_cov(x[None, :len(we)], we[None])[0]))
        assert np.all(np.isnan(sc.emulate_wcov(x[:len(we)], we)))
    assert sc.ratio(C - C, A) == np.inf                                  # the ratio never lets a NaN pass


def test_exp_weights_and_the_gridded_log_weights():
    rng = np.random.default_rng(3)
    for N in (1, 2, 3, 64, 5000):
        lw = sc.grid_logweights(rng, N)
        assert lw.max() == 0.0 and np.all((lw * 1024 == np.round(lw * 1024)) | np.isneginf(lw)) and np.all(lw[np.isfinite(lw)] >= -30.0)
        assert np.count_nonzero(np.isfinite(lw)) >= min(N, 2)
        e = sc.exp_weights(lw)
        assert e.dtype == np.longdouble and abs(float(e.sum()) - 1.0) < 1e-18 and np.all((e == 0) == np.isneginf(lw))
        np.testing.assert_allclose(e.astype(np.float64), np.exp(lw) / np.exp(lw).sum(), rtol=1e-13)
    assert 0.25 < np.mean(np.isneginf(sc.grid_logweights(rng, 5000))) < 0.45
    e = sc.exp_weights([-np.inf, -1.0, -np.inf])
    assert e[1] == 1 and e[0] == 0 and e[2] == 0


def _weighted_state(rng, N, nx, offset):
    x = rng.standard_normal((N, nx)) * (1.0 + np.arange(nx)) + offset
    we = rng.random(N) ** 3
    if N > 3:
        we[rng.random(N) < 0.3] = 0.0
    if np.count_nonzero(we) < 2:
        we[:2] = 0.5
    return x, we / we.sum()


@pytest.mark.parametrize("N", [2, 3, 400, 5000])
def test_host_function_of_the_python_mirror(N):
    """api.weighted_cov(x, we) (numpy, fp64, for returned histories) against the long double reference within the device's bound
    (np.sum and a BLAS product: chains no longer than a thread's), zero weights included"""
    import llpf_amd
    rng = np.random.default_rng(N)
    for nx, offset in ((1, 0.0), (2, 1e6), (16, 0.0)):
        x, we = _weighted_state(rng, N, nx, offset)
        C, A = sc.ref_cov(x, we)
        got = llpf_amd.weighted_cov(x[None], we[None])[0]
        assert sc.ratio(got - C, A) <= sc.bound_units(N), (N, nx, offset, sc.ratio(got - C, A))
        wrong_n = got * (np.count_nonzero(we) - 1) / np.count_nonzero(we) * N / (N - 1)          # n = N instead of count(we != 0)
        if N > 3:
            assert sc.ratio(wrong_n - C, A) > 100 * sc.bound_units(N)                              # ... is far outside it


def test_the_second_order_term_of_the_means_rounding():
    """Two particles near 1e6, all the weight but 1e-7 on one of them: the rounding of the mean, squared, is u^2 1e12 against
    u A ~ u 1e-6 — the two-pass formula in fp64 (the device's order and numpy's alike) leaves K u A by an order of magnitude and stays
    within K u A + E, the term ref_cov derives from the bound of the mean.  For a cloud of ordinary spread E is nothing."""
    import llpf_amd
    rng = np.random.default_rng(11)
    K = sc.bound_units(2)
    worst = 0.0
    for _ in range(300):
        x = 1e6 + rng.standard_normal((2, 2))
        e = 1e-7 * (0.5 + rng.random())
        we = np.array([1.0 - e, e])
        C, A, E = sc.ref_cov(x, we, 2)
        for got in (sc.emulate_wcov(x, we), llpf_amd.weighted_cov(x[None], we[None])[0]):
            assert sc.ratio(got - C, A, E) <= K
            worst = max(worst, sc.ratio(got - C, A))
    assert worst > 2 * K, worst
    x, we = _weighted_state(rng, 5000, 3, 1e6)
    C, A, E = sc.ref_cov(x, we, 5000)
    assert sc.ratio(E, A) < 2.0 and np.array_equal(E, E.T)          # unit spread at 1e6: a unit of u A beside K = 52
    assert sc.ratio(sc.ref_cov(x - 1e6, we, 5000)[2], A) < 1e-9


@pytest.mark.parametrize("N", [2, 3, 65, 257, 1025, 5000, 100000])
def test_the_devices_summation_order_stays_within_the_bound(N):
    """256 strided partial sums, a pairwise tree per wave, four wave sums in order — in fp64 numpy — against the long double reference:
    within (ceil(N / 256) + 32) u A and u abs_mean, with 30 % of the weights zero and the states offset by 0 and by 1e6.  The largest
    ratio over these cases is 3.95 (covariance) and 2.1 (mean) — the bound's constant has a wide margin and comes from counting
    operations, not from these figures."""
    rng = np.random.default_rng(1000 + N)
    worst_c = worst_m = 0.0
    for nx in (1, 3, 16):
        for offset in (0.0, 1e6):
            x, we = _weighted_state(rng, N, nx, offset)
            C, A = sc.ref_cov(x, we)
            m, am = sc.ref_mean(x, we)
            worst_c = max(worst_c, sc.ratio(sc.emulate_wcov(x, we) - C, A))
            worst_m = max(worst_m, sc.ratio(sc.emulate_wmean(x, we) - m, am))
    print("N = %d: covariance %.2f, mean %.2f units of u (bound %d)" % (N, worst_c, worst_m, sc.bound_units(N)))
    assert worst_c <= sc.bound_units(N) and worst_m <= sc.bound_units(N)
