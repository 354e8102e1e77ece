"""ezpz_solve, ezpz_solve_inner and ezpz_solve_batch on a machine without a device: the three entries work from the same
request plan, so they report request errors (and the lint warnings ahead of them) alike, and only then the missing device
(csrc/api.hip: ezpz_system_create reports request errors before the absence of a device)."""
import numpy as np
import pytest

from oracle import oracle as O

import ezpz_amd as E


@pytest.fixture(autouse=True)
def no_device():
    if E.device_count() > 0:
        pytest.skip("a device is present")


def _batch_error(recs, x0):
    with pytest.raises(E.NonLinearSystemError) as e:
        E.solve_batch(O.stack(recs), x0)
    return e.value.code, e.value.constraint_id, e.value.variable


def test_missing_guess_is_reported_before_the_missing_device_by_every_entry():
    recs, guesses = [O.fixed(0, 1.0), O.fixed(9, 1.0)], np.zeros(3)
    for kw in ({}, {"inner": True}):
        got = E.solve_records(recs, guesses, **kw)
        assert (got.error, got.err_constraint_id, got.err_variable) == (E.api.ERR_MISSING_GUESS, 1, 9), kw
    assert _batch_error(recs, np.zeros((4, 3))) == (E.api.ERR_MISSING_GUESS, 1, 9)
    got = E.solve_records(recs, guesses, inner=True, orig_ids=[10, 20])
    assert (got.error, got.err_constraint_id, got.err_variable) == (E.api.ERR_MISSING_GUESS, 20, 9)


def test_a_valid_request_fails_with_no_device_on_every_entry():
    recs, guesses = [O.fixed(0, 1.0), O.distance((0, 1), (2, 3), 2.0)], np.array([0.5, 0.0, 1.0, 1.0])
    assert E.solve_records(recs, guesses).error == E.api.ERR_NO_DEVICE
    assert E.solve_records(recs, guesses, inner=True).error == E.api.ERR_NO_DEVICE
    assert _batch_error(recs, np.tile(guesses, (3, 1)))[0] == E.api.ERR_NO_DEVICE


def test_no_requests_echo_the_guesses():
    """lib.rs:155-170"""
    none = np.zeros(0, dtype=E.CONSTRAINT_DTYPE)
    guesses = np.array([1.5, -2.0, 3.25])
    got = E.solve_records(none, guesses)
    assert got.error == 0 and got.converged and got.iterations == 0 and np.array_equal(got.final_values, guesses)
    x0 = np.arange(12.0).reshape(4, 3)
    x, st, prio, _ = E.solve_batch(none, x0)
    assert np.array_equal(x, x0) and np.all(st["converged"] == 1) and np.all(st["iterations"] == 0) and np.all(prio == 0)


def test_lint_warnings_arrive_ahead_of_the_error_with_the_callers_ids():
    """lib.rs:276-277: lint runs before Model::new; about_constraint is ConstraintEntry.id (orig_ids)."""
    recs = [O.fixed(0, 0.0), O.lines_at_angle((0, 1), (2, 3), (4, 5), (6, 7), ("deg", 90.0))]
    got = E.solve_records(recs, np.arange(8.0), inner=True, orig_ids=[30, 41])
    assert got.error == E.api.ERR_NO_DEVICE and got.warnings == [(41, O.WARN_SHOULD_BE_PERPENDICULAR)]
    # ... and ahead of a request error too (the guess of id 7 is missing)
    got = E.solve_records(recs, np.arange(7.0), inner=True, orig_ids=[30, 41])
    assert (got.error, got.err_constraint_id, got.err_variable) == (E.api.ERR_MISSING_GUESS, 41, 7)
    assert got.warnings == [(41, O.WARN_SHOULD_BE_PERPENDICULAR)]
    assert E.solve_records(recs, np.arange(7.0)).warnings == [(1, O.WARN_SHOULD_BE_PERPENDICULAR)]
