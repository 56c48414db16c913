"""The mismatch reports of tests/gpu_common.py: a red full-length parity test must name the timestep where the engine and the
oracle part, not only say that two arrays differ."""
import numpy as np
import pytest

from gpu_common import assert_state_equal, assert_steps_equal, state_mismatch, step_mismatch


def test_identical_arrays_report_nothing():
    a = np.linspace(-3.0, 1.0, 1000)
    assert step_mismatch(a, a.copy()) is None
    assert state_mismatch(a.reshape(500, 2), a.reshape(500, 2).copy()) is None
    assert state_mismatch(np.arange(7), np.arange(7)) is None
    assert_steps_equal(a, a.copy())


def test_a_planted_difference_is_reported_at_its_step():
    rng = np.random.default_rng(0)
    want = rng.standard_normal(1000) - 5.0
    got = want.copy()
    got[731] = np.nextafter(got[731], 0.0)         # one ulp
    got[900] += 1e-3
    msg = step_mismatch(got, want, resamples=(412, 411))
    assert "step 731:" in msg
    assert float(got[731]).hex() in msg and float(want[731]).hex() in msg and repr(float(want[731])) in msg
    assert "2 of 1000 steps differ" in msg
    assert "resample counts 412 against 411" in msg
    with pytest.raises(AssertionError, match="ll_steps: first difference at step 731"):
        assert_steps_equal(got, want)


def test_a_sign_of_zero_and_a_nan_count_as_differences():
    want = np.zeros(10)
    got = want.copy()
    got[3] = -0.0
    assert "step 3:" in step_mismatch(got, want)
    got = want.copy()
    got[8] = np.nan
    assert "step 8:" in step_mismatch(got, want)


def test_per_step_rows_of_a_bank_name_step_and_filter():
    want = np.arange(400.0).reshape(100, 4)
    got = want.copy()
    got[57, 2] += 0.5
    got[60, 0] += 0.5
    msg = step_mismatch(got, want)
    assert "step 57, column 2" in msg and "2 of 100 steps differ" in msg


def test_final_state_reports_count_and_first_index():
    want = np.arange(2000.0).reshape(1000, 2)
    got = want.copy()
    got[731, 1] = -1.0
    got[999, 0] = -1.0
    msg = state_mismatch(got, want)
    assert "2 of 2000 entries differ" in msg and "index (731, 1)" in msg
    ja = np.arange(50, dtype=np.int64)
    jb = ja.copy()
    jb[17] = 3
    assert "1 of 50 entries differ, the first at index (17,): 17 against 3" in state_mismatch(ja, jb)
    with pytest.raises(AssertionError, match="ancestors differ: 1 of 50"):
        assert_state_equal(ja, jb, "ancestors")
    assert "shapes differ" in state_mismatch(ja, ja[:-1])
