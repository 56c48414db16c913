"""The reference of the summary statistics (weighted_mean / xmean, weighted_cov / xcov) in np.longdouble, the bound the device's
fp64 results are held to, and a numpy emulation of the device's summation order.

The reference shares nothing with the engine or the oracle: it is the formula of the reference's src/filtering.jl:541-549 (mean) and
571-581 (cov(X, ProbabilityWeights(we), 2, corrected = true)) evaluated in the 64-bit significand of np.longdouble, every sum a pairwise
sum over a contiguous axis (error ~ log2(N) 2^-64: three decimal orders below what it judges).

The bound, entry by entry, with u = 2^-53 and K = bound_units(N) = ceil(N / 256) + 32:
    |C_gpu - C|       <= K u A + E,     A = corr sum_i we_i |x_i - mu| |x_i - mu|'
    |mean_gpu - mean| <= K u abs_mean,  abs_mean = sum_i we_i |x_i|
k_wmean and k_wcov (csrc/kernels/access.hpp) run one block of 256 threads per filter: ceil(N / 256) is the longest chain of additions
in a thread's strided partial sum; 32 covers the 6 levels of the wave's shuffle tree, the 3 additions of the four wave sums, the two
multiplications of a term, the subtraction x - mu, the correction factor and its division and the < 1 ulp of llpf_exp_le0
(test_detmath.py).  A common scale error of the exp-weights cancels in C (corr divides by their sum).  The rounding of the mean enters
the centred sum only in second order, sum we (x - mu - d)(x - mu - d)' = S + d d' sum we (the cross terms vanish): that term is E,
derived in ref_cov below from the bound of the mean — of the order u^2 |x|^2, far below u A unless the cloud is 1e8 times narrower than
it is far from the origin.  Derived, not measured: the emulation below stays below 4 u A (tests/test_statistics_reference.py)."""
import math

import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53
BLOCK = 256


def bound_units(N):
    return math.ceil(N / BLOCK) + 32


def ref_mean(x, we):
    """(mean, abs_mean) of particles x [N, nx] under weights we [N]: sum we x (NOT divided by sum we, as weighted_mean / xmean) and
    sum we |x|, as float64 arrays of the long double values"""
    xt = np.ascontiguousarray(np.asarray(x, dtype=LD).T)
    wl = np.asarray(we, dtype=LD)
    return (xt * wl).sum(axis=1).astype(np.float64), (np.abs(xt) * wl).sum(axis=1).astype(np.float64)


def ref_cov(x, we, N=None):
    """(C, A): C = corr sum we (x - mu)(x - mu)', mu = sum we x / sum we, corr = n / ((n - 1) sum we), n = count(we != 0), and the
    same sum over |x - mu| |x - mu|'.  n = 1: 0 * inf, NaN in every entry, as the reference's formula.
    With N, the particle count the bound is taken for: (C, A, E), E the second-order term of the mean's rounding (see below)."""
    xt = np.ascontiguousarray(np.asarray(x, dtype=LD).T)           # [nx, N]: sums run along the contiguous axis (pairwise)
    wl = np.asarray(we, dtype=LD)
    nx = xt.shape[0]
    s = wl.sum()
    n = LD(np.count_nonzero(wl))
    d = xt - ((xt * wl).sum(axis=1) / s)[:, None]
    wd, ad = d * wl, np.abs(d)
    Cm, Am = np.zeros((nx, nx), dtype=LD), np.zeros((nx, nx), dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        corr = n / ((n - 1) * s)
        for r in range(nx):
            Cm[r, :r + 1] = (wd[r] * d[:r + 1]).sum(axis=1) * corr
            Am[r, :r + 1] = (np.abs(wd[r]) * ad[:r + 1]).sum(axis=1) * corr
        iu = np.triu_indices(nx, 1)
        Cm[iu], Am[iu] = Cm.T[iu], Am.T[iu]
        if N is None:
            return Cm.astype(np.float64), Am.astype(np.float64)
        # What "the mean enters only in second order" leaves out.  The device centres on mu_g = fl(mean_g / s_g) = mu + delta with
        #     |delta_r| <= (2 K + 1) u abs_mean_r / s,   K = bound_units(N):
        # K u abs_mean_r for the sum mean_g (the bound of the mean), K u |mean_r| for the sum s_g of the weights (the same order of
        # additions), u for the division.  Exactly, sum we (x - mu - delta)(x - mu - delta)' = S + s delta delta': E = corr s delta delta'
        # is an error of the result that K u A does not hold — u^2 |x|^2 against u A, nothing for a cloud whose spread is comparable to
        # its distance from the origin, but the larger of the two once spread / distance falls below sqrt(u) ~ 1e-8 (states near 1e6
        # whose weight sits on one particle but for 1e-7: measured 305 u A on the device and in numpy's own fp64 two-pass formula).
        # The terms the device rounds are those around mu_g: their absolute sum exceeds A by at most corr (|delta_r| a_c + a_r |delta_c|
        # + s |delta_r| |delta_c|), a_r = sum we |x_r - mu_r|, which K u multiplies.
        K = bound_units(N)
        delta = (2 * K + 1) * U53 * (np.abs(xt) * wl).sum(axis=1) / s
        a = (ad * wl).sum(axis=1)
        dd = np.outer(delta, delta) * s
        Em = corr * (dd + K * U53 * (np.outer(delta, a) + np.outer(a, delta) + dd))
    return Cm.astype(np.float64), Am.astype(np.float64), Em.astype(np.float64)


def exp_weights(logw):
    """exp(logw - max) over its sum in long double (-inf: 0): the exp-weights of log-weights the test installs itself"""
    lw = np.asarray(logw, dtype=LD)
    with np.errstate(invalid="ignore"):
        e = np.where(np.isneginf(lw), LD(0), np.exp(lw - lw.max()))
    return e / e.sum()


def grid_logweights(rng, N, frac_inf=0.35):
    """log-weights on a grid of 2^-10 in [-30, 0] with the largest at 0 and about frac_inf of them -inf (never the largest, never all but
    one for N >= 2): w - max is exact in fp64, so exp_weights() of them is a reference that does not pass through the engine"""
    lw = -rng.integers(0, 30 * 1024 + 1, N).astype(np.float64) / 1024.0
    lw[rng.integers(0, N)] = 0.0
    drop = np.flatnonzero((rng.random(N) < frac_inf) & (lw != 0.0))
    if N >= 2 and drop.size > N - 2:
        drop = drop[:N - 2]
    lw[drop] = -np.inf
    return lw


def ratio(err, scale, slack=0.0):
    """max (|err| - slack) / (u scale) over the entries; an entry whose scale is 0 must be exact"""
    err, scale = np.maximum(np.abs(np.asarray(err, dtype=np.float64)) - slack, 0.0), np.asarray(scale, dtype=np.float64)
    if np.any(np.isnan(err)) or np.any(err[scale == 0.0] != 0.0):
        return np.inf
    nz = scale > 0.0
    return float(np.max(err[nz] / (U53 * scale[nz]))) if nz.any() else 0.0


# ---- the device's summation order in numpy (fp64) ---------------------------------------------------------------------------------
def _block_sum(N, shape, chunk):
    """sum of the terms chunk(j0, j1) -> [j1 - j0, *shape], j = 0 .. N - 1, as one block of 256 threads forms it: thread t adds terms
    t, t + 256, ... in order, a pairwise tree over the 64 lanes of each wave, the four wave sums added in order"""
    part = np.zeros((BLOCK,) + shape)
    for j in range(0, N, BLOCK):
        c = chunk(j, min(j + BLOCK, N))
        part[:len(c)] = part[:len(c)] + c
    w = part.reshape((4, 64) + shape)
    h = 64
    while h > 1:
        h //= 2
        w = w[:, :h] + w[:, h:2 * h]
    w = w[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def emulate_wmean(x, we):
    """k_wmean in numpy: fp64, the device's order"""
    x, we = np.asarray(x, dtype=np.float64), np.asarray(we, dtype=np.float64)
    return _block_sum(len(x), x.shape[1:], lambda a, b: x[a:b] * we[a:b, None])


def emulate_wcov(x, we):
    """k_wcov in numpy: fp64, the device's order (the mean from emulate_wmean, as bank_weighted_cov takes it from k_wmean)"""
    x, we = np.asarray(x, dtype=np.float64), np.asarray(we, dtype=np.float64)
    N, nx = x.shape
    stot = _block_sum(N, (), lambda a, b: we[a:b])
    ntot = _block_sum(N, (), lambda a, b: (we[a:b] != 0.0).astype(np.float64))
    d = x - emulate_wmean(x, we) / stot
    acc = _block_sum(N, (nx, nx), lambda a, b: (we[a:b, None] * d[a:b])[:, :, None] * d[a:b, None, :])      # [r, c] = (we d_r) d_c
    with np.errstate(divide="ignore", invalid="ignore"):
        low = np.tril(acc) * (ntot / ((ntot - 1.0) * stot))
    return low + np.tril(low, -1).T
