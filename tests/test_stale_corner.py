"""Which outputs of a resampling can have a threshold >= bins[N]: only the last one.

The reference leaves j[i] untouched where no bin lies above the threshold of output i (resample.jl:25-34, :52-58), and the fused timestep
reads the previous ancestor of exactly those outputs (kernels/resprop.hpp, the rounds of [c_end, M)).  A run whose fused launches store
no ancestors between its steps (k_resprop<..., SKIPA>) keeps only the entry of output M - 1 current, so it rests on this bound: with
M = N outputs, no output other than M - 1 has a threshold >= bins[N], whatever the offset.

The thresholds are the expressions of kernels/resample.hpp (ThrSys::at, ThrStrat::at; the oracle's thr_at is the same text), evaluated
here in IEEE double arithmetic, one rounding per operation, in the order written there:
    systematic  r = U * bins[N] / N;  thr(i) = r + i * (1 / M)
    stratified  thr(i) = (i + U_i) / M * bins[N]
bins[N] = fl(Td * fl(1 / Td)) is 1 or 1 - 2^-53 (res_counts); both are tried.  No tolerance: the comparison is the reference's own.

Every operation above is monotone in i and in U (rounding is monotone), so thr is non-decreasing in both; the largest U below 1 is
therefore the worst case of every output, and at N = 2^29 the outputs below the last 2^22 are covered by the window's first one."""
import numpy as np
import pytest

ONE_M = 1.0 - 2.0 ** -53            # the largest double below 1
NS = [2, 3, 1025, 70001, 10 ** 6, 2 ** 29]
WINDOW = 1 << 22


def thr_sys(i, U, N, binsN):
    r = np.float64(U) * np.float64(binsN) / np.float64(N)
    step = np.float64(1.0) / np.float64(N)
    return r + i.astype(np.float64) * step


def thr_strat(i, U, N, binsN):
    return (i.astype(np.float64) + U) / np.float64(N) * np.float64(binsN)


def _last(fn, U, N, binsN):
    return float(fn(np.array([N - 1], dtype=np.int64), U, N, binsN)[0])


def _smallest_u_reaching(fn, N, binsN, v):
    """the smallest U in [0, 1) whose last threshold is >= v, or None (thr is non-decreasing in U: bisection over the doubles)"""
    if not _last(fn, ONE_M, N, binsN) >= v:
        return None
    lo, hi = 0, int(np.float64(ONE_M).view(np.uint64))       # non-negative doubles order like their bit patterns
    if _last(fn, 0.0, N, binsN) >= v:
        return 0.0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _last(fn, float(np.uint64(mid).view(np.float64)), N, binsN) >= v:
            hi = mid
        else:
            lo = mid
    return float(np.uint64(hi).view(np.float64))


def _offsets(fn, N, binsN):
    """0, the largest double below 1, some in between, and the offsets at which the last threshold first reaches 1 - 2^-53 and 1, with
    their neighbours on either side"""
    us = {0.0, ONE_M, 0.5, 0.25, 1.0 / 3.0, 2.0 ** -53, 2.0 ** -30, float(np.nextafter(ONE_M, 0.0))}
    hit = set()
    for v in (ONE_M, 1.0):
        u = _smallest_u_reaching(fn, N, binsN, v)
        if u is None:
            continue
        for c in (u, float(np.nextafter(u, 0.0)), float(np.nextafter(u, 1.0))):
            if 0.0 <= c < 1.0:
                us.add(c)
        hit.add(_last(fn, u, N, binsN))
    return sorted(us), hit


def _windows(N):
    if N <= 10 ** 6:
        yield np.arange(N, dtype=np.int64)
    else:
        yield np.arange(N - WINDOW, N, dtype=np.int64)
        yield np.arange(0, N, 4099, dtype=np.int64)           # a sample of the rest (covered by monotonicity; a check of that claim)


@pytest.mark.parametrize("binsN", [1.0, ONE_M])
@pytest.mark.parametrize("name", ["systematic", "stratified"])
@pytest.mark.parametrize("N", NS)
def test_only_the_last_output_can_reach_bins_N(N, name, binsN):
    fn = thr_sys if name == "systematic" else thr_strat
    us, hit = _offsets(fn, N, binsN)
    # the corner itself is in the cases: some offset takes the last threshold to bins[N] or beyond, and to each of 1 - 2^-53 and 1 that
    # the expression can produce there
    assert _last(fn, ONE_M, N, binsN) >= binsN, "the largest offset does not take the last threshold to bins[N]: the corner is not in the cases"
    reached = sorted(_last(fn, U, N, binsN) for U in us)
    print(N, name, binsN, "offsets", len(us), "last threshold from", reached[0], "to", reached[-1], "corner values hit", sorted(hit))
    if name == "systematic":
        assert ONE_M in hit or 1.0 in hit, "no offset takes the last threshold of the systematic rule to 1 - 2^-53 or 1"
    for idx in _windows(N):
        prev_last = None
        for U in us:
            t = fn(idx, U, N, binsN)
            assert np.all(np.diff(t) >= 0.0), "thresholds decrease with the output"
            if prev_last is not None:
                assert t[-1] >= prev_last, "thresholds decrease with the offset"
            prev_last = t[-1]
            others = t[idx != N - 1]
            bad = idx[idx != N - 1][others >= binsN]
            assert bad.size == 0, "N = %d, %s, U = %r, bins[N] = %r: outputs %r besides M - 1 have a threshold >= bins[N]" % (
                N, name, U, binsN, bad[:8].tolist())


@pytest.mark.parametrize("binsN", [1.0, ONE_M])
@pytest.mark.parametrize("N", [2, 3, 1025, 70001, 10 ** 6])
def test_stratified_with_an_offset_per_output(N, binsN):
    """every output with its own uniform, the extremes among them"""
    rng = np.random.default_rng(N)
    idx = np.arange(N, dtype=np.int64)
    for k in range(3):
        U = rng.random(N)
        U[rng.integers(0, N, size=max(1, N // 7))] = ONE_M
        U[rng.integers(0, N, size=max(1, N // 7))] = 0.0
        if k == 2:
            U[:] = ONE_M
        t = thr_strat(idx, U, N, binsN)
        assert not np.any(t[:-1] >= binsN)
