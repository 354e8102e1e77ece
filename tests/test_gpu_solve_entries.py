"""The reference's two solve functions behind the C ABI's entries (-m gpu): ezpz_solve_inner (solve_inner, lib.rs:265-356)
against the oracle's, against ezpz_solve on the same call, with the caller's ids and with priorities it must ignore; and
ezpz_solve_batch taking its tiers and analysed topologies from the request plan ezpz_solve uses (csrc/solve.cpp)."""
import numpy as np
import pytest

import cases
from adapters import OracleAdapter
from oracle import oracle as O
from oracle import textual as T
from test_gpu_parity import E, assert_x_close  # noqa: F401  (E: the module's device fixture)

pytestmark = pytest.mark.gpu

CASES = ["tiny", "square", "inconsistent", "two_rectangles", "warnings_lint"]
OUTCOME_FIELDS = ["error", "err_constraint_id", "err_variable", "iterations", "converged", "unsatisfied", "warnings",
                  "priority_solved", "num_vars", "num_eqs", "final_lambda", "final_residual_inf"]


class _Recorder(OracleAdapter):
    """Runs a case of tests/cases.py on the oracle and keeps the problem text it was given."""

    def run_text(self, text, config=None):
        self.text = text
        return super().run_text(text, config)


@pytest.fixture(scope="module")
def requests():
    """name -> (side-resolved records, guesses by id): what solve_inner is handed (lib.rs:183-186 has run already)."""
    out = {}
    for name in CASES:
        rec = _Recorder()
        getattr(cases, name)(rec)
        ref = T.load(rec.text)
        out[name] = (O.stack([O.set_from_initial_values(c, ref.guesses) for c in ref.constraints]), ref.guesses)
    return out


def _same_outcome(got, want):
    for f in ("iterations", "converged", "unsatisfied", "warnings", "priority_solved", "error"):
        assert getattr(got, f) == getattr(want, f), (f, getattr(got, f), getattr(want, f))
    assert_x_close(got.final_values, want.final_values)


def _priority_request():
    """The request list of test_batch_solve_with_priorities_and_inferred_sides and its 96 starts."""
    p0, p1, center, radius = (0, 1), (2, 3), (4, 5), 6
    reqs = [
        O.fixed(1, 3.0), O.fixed(3, 3.0), O.circle_radius(center, radius, 1.5),
        O.line_tangent_to_circle(p0, p1, center, radius, O.SIDE_UNDEFINED),
        O.fixed(4, 2.0, priority=1), O.fixed(5, 100.0, priority=2), O.fixed(0, 0.0, priority=1, weight=2.0),
    ]
    rng = np.random.default_rng(5)
    x0 = np.tile(np.array([0.0, 3.0, 5.0, 3.0, 2.0, 1.5, 1.5]), (96, 1)) + rng.uniform(-0.2, 0.2, (96, 7))
    x0[::2, 5] += 3.0
    return O.stack(reqs), x0


@pytest.mark.parametrize("name", CASES)
def test_solve_inner_matches_the_oracles(E, requests, name):
    recs, guesses = requests[name]
    want = O.solve(recs, guesses, inner=True)
    assert want.error == 0 and bool(want.unsatisfied) == (name == "inconsistent")
    assert bool(want.warnings) == (name == "warnings_lint")
    _same_outcome(E.solve_records(recs, guesses, inner=True), want)


@pytest.mark.parametrize("name", CASES)
def test_solve_inner_without_ids_is_solve_on_one_tier(E, requests, name):
    """One priority, every side resolved: both entries run solve_tier on a latency-analysed system of the same bytes."""
    recs, guesses = requests[name]
    inner = E.solve_records(recs, guesses, inner=True)
    outer = E.solve_records(recs, guesses)
    assert inner.final_values.tobytes() == outer.final_values.tobytes()
    for f in OUTCOME_FIELDS:
        assert getattr(inner, f) == getattr(outer, f), f


def test_orig_ids_name_the_unsatisfied_and_linted_constraints(E, requests):
    for name in ("inconsistent", "warnings_lint"):
        recs, guesses = requests[name]
        ids = 100 + 7 * np.arange(len(recs))
        plain = E.solve_records(recs, guesses, inner=True)
        got = E.solve_records(recs, guesses, inner=True, orig_ids=ids)
        assert plain.unsatisfied or plain.warnings
        assert got.unsatisfied == [int(ids[i]) for i in plain.unsatisfied]
        # lint warnings carry the caller's id, Degenerate ones the position inside the tier (solver.rs:327,:343)
        assert got.warnings == [(a if c == O.WARN_DEGENERATE else int(ids[a]), c) for a, c in plain.warnings]
        _same_outcome(got, O.solve(recs, guesses, inner=True, orig_ids=ids))


def test_degenerate_warnings_keep_tier_positions_under_orig_ids(E):
    """solver.rs:327,:343: a Degenerate warning is about the position inside the tier, whatever ConstraintEntry.id says."""
    center, start, end = (0, 1), (2, 3), (4, 5)
    recs = O.stack([O.fixed(0, 0.0), O.fixed(1, 0.0), O.fixed(2, 0.0), O.fixed(3, 0.0), O.arc_length(center, start, end, 1.0),
                    O.points_at_angle((0, 1), (2, 3), (4, 5), ("deg", 180.0))])
    guesses = np.array([0.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    ids = 100 + 7 * np.arange(len(recs))
    got = E.solve_records(recs, guesses, inner=True, orig_ids=ids)
    want = O.solve(recs, guesses, inner=True, orig_ids=ids)
    assert got.warnings == want.warnings and len(want.warnings) > 2
    assert all(c == O.WARN_DEGENERATE and 0 <= a < len(recs) for a, c in got.warnings)
    assert got.warnings == E.solve_records(recs, guesses, inner=True).warnings
    assert (got.iterations, got.converged, got.unsatisfied) == (want.iterations, want.converged, want.unsatisfied)


def test_solve_inner_ignores_priorities_and_its_plan_is_its_own(E):
    """lib.rs:340-344: solve_inner solves the list it is given and reports its maximum priority; ezpz_solve of the same
    bytes stops at the last satisfied tier.  The two plans of one request do not answer for each other."""
    recs, x0 = _priority_request()
    guesses = x0[1]
    recs = O.stack([O.set_from_initial_values(c, guesses) for c in recs])
    want_inner = O.solve(recs, guesses, inner=True)
    want_outer = O.solve(recs, guesses)
    assert (want_inner.priority_solved, want_outer.priority_solved) == (2, 1)
    assert want_inner.unsatisfied and not want_outer.unsatisfied
    first = E.solve_records(recs, guesses)
    inner = E.solve_records(recs, guesses, inner=True)
    again = E.solve_records(recs, guesses)
    _same_outcome(inner, want_inner)
    assert inner.num_eqs == 7
    for outer in (first, again):
        _same_outcome(outer, want_outer)
        assert outer.num_eqs == 6
    assert first.final_values.tobytes() == again.final_values.tobytes()


def test_solve_inner_with_sparse_ids_cannot_place_the_column(E):
    """Layout::index_of (solver.rs:107-109): id 5 has a guess but no column among three."""
    recs = [O.fixed(0, 1.0), O.fixed(5, 2.0)]
    guesses = [(0, 0.0), (1, 0.0), (5, 0.0)]
    assert E.solve_records(recs, guesses).error == E.api.ERR_MATRIX
    assert E.solve_records(recs, guesses, inner=True).error == E.api.ERR_MATRIX


def _traced(E, call):
    """(result of call(), the COLD_* stamps of csrc/call_trace.hpp it left: the symbolic phase ran)."""
    trace = np.zeros(512, dtype=np.uint64)
    E.lib().ezpz_debug_call_trace(trace.ctypes.data, trace.size)
    out = call()
    k = E.lib().ezpz_debug_call_trace(None, 0)
    return out, [int(s) for s in trace[:k:2] if s >= 20]


def _batch_bytes(result):
    x, st, prio, mask = result
    return x.tobytes(), st.tobytes(), prio.tobytes(), mask.tobytes()


def test_batch_solve_builds_nothing_on_a_repeat(E):
    """Three tiers x two inferred sides: every topology is analysed once, and found again by the next call."""
    recs, x0 = _priority_request()
    call = lambda: E.solve_batch(recs, x0, want_mask=True)  # noqa: E731
    first = call()
    assert set(first[2].tolist()) == {1}
    second, cold = _traced(E, call)
    assert cold == [] and _batch_bytes(second) == _batch_bytes(first)
    E.lib().ezpz_cache_clear()
    third, cold = _traced(E, call)
    assert cold.count(21) == 6 and _batch_bytes(third) == _batch_bytes(first)  # COLD_ANALYSED: once per tier and side
    fourth, cold = _traced(E, call)
    assert cold == [] and _batch_bytes(fourth) == _batch_bytes(first)


@pytest.mark.parametrize("order", [(1, 96), (96, 1)])
def test_batch_of_one_and_of_many_keep_their_own_topologies(E, order):
    """A batch of one is analysed for latency, a larger one for throughput: one request, two sets of systems."""
    recs, x0 = _priority_request()
    E.lib().ezpz_cache_clear()
    got = {}
    for b in order:
        got[b] = E.solve_batch(recs, x0[:b], want_mask=True)
    for b in order:  # warm now, whichever came first
        again, cold = _traced(E, lambda: E.solve_batch(recs, x0[:b], want_mask=True))
        assert cold == [] and _batch_bytes(again) == _batch_bytes(got[b])
    (x1, st1, prio1, mask1), (xn, stn, prion, maskn) = got[1], got[96]
    assert (int(st1["iterations"][0]), int(prio1[0])) == (int(stn["iterations"][0]), int(prion[0]))
    assert np.array_equal(mask1[0], maskn[0])
    assert_x_close(x1[0], xn[0])
