"""Host-side mirror of the `ezpz` crate's public solve API, on top of the C ABI (include/ezpz_amd.h).

Same names, argument meaning and error behaviour as the reference for the hot path:
    solve(reqs, initial_guesses, config)        reference ezpz/src/lib.rs:80-87
    Constraint / ConstraintRequest / Config     reference constraints.rs:37-93, constraint_request.rs, solver.rs:31-81
    DatumPoint / DatumLineSegment / ...         reference datatypes/inputs.rs
    SolveOutcome / FailureOutcome / Warning     reference solve_outcome.rs, error.rs, warnings.rs
`Result<SolveOutcome, FailureOutcome>` becomes "return SolveOutcome or raise FailureOutcome".
Everything numeric happens in the HIP kernel behind `ezpz_solve`; this module only packs records.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from ._lib import PARAMS_ROUTES, SENSITIVITY_ROUTES, SWEEP_ROUTE_NAMES, CONSTRAINT_DTYPE, GUARD_STEP_DTYPE, BRANCH_DTYPE, BRANCH_INFO_DTYPE, MC_DIST_DTYPE, MC_SEQUENCE, MC_MOMENT_MAX, MC_MOMENTS_INFO_DTYPE, MC_STATS_DTYPE, MC_TOTALS_DTYPE, IMAGE_INFO_DTYPE, STATUS_DTYPE, SEEK_INFO_DTYPE, SEEK_STATUS, SEEK_STEP, CBranchConfig, CConfig, CGuardConfig, CMcConfig, CMcContribConfig, CSobolConfig, SOBOL_MAX, SOBOL_SEED_B, CMcQuantileConfig, CMcEffectConfig, MC_EFFECT_MAX_BINS, MC_EFFECT_MAX_CELLS, MC_EFFECT_MAX_DIM, MC_QUANTILE_DTYPE, MC_QUANTILE_MAX_MEAS, MC_QUANTILE_MAX_PROBS, MC_FACTORIAL_DTYPE, MC_FACTORIAL_MAX_CORNERS, MC_FACTORIAL_MAX_MEAS, CSeekConfig, COutcome, CRedundancyConfig, CSensitivityPlan, CSweepPlan, CSystemInfo, CWarning, lib

Id = int

# EzpzKind
(LINE_TANGENT_TO_CIRCLE, CIRCLE_TANGENT_TO_CIRCLE, DISTANCE, DISTANCE_VAR, VERTICAL_DISTANCE, HORIZONTAL_DISTANCE,
 VERTICAL, HORIZONTAL, LINES_AT_ANGLE, FIXED, SCALAR_EQUAL, POINTS_COINCIDENT, CIRCLE_RADIUS, LINES_EQUAL_LENGTH,
 ARC_RADIUS, ARC, MIDPOINT, POINT_LINE_DISTANCE, VERTICAL_POINT_LINE_DISTANCE, HORIZONTAL_POINT_LINE_DISTANCE,
 SYMMETRIC, POINT_ARC_COINCIDENT, ARC_LENGTH, ARC_ANGLE, POINTS_AT_ANGLE) = range(25)

KIND_NAMES = [
    "LineTangentToCircle", "CircleTangentToCircle", "Distance", "DistanceVar", "VerticalDistance",
    "HorizontalDistance", "Vertical", "Horizontal", "LinesAtAngle", "Fixed", "ScalarEqual", "PointsCoincident",
    "CircleRadius", "LinesEqualLength", "ArcRadius", "Arc", "Midpoint", "PointLineDistance",
    "VerticalPointLineDistance", "HorizontalPointLineDistance", "Symmetric", "PointArcCoincident", "ArcLength",
    "ArcAngle", "PointsAtAngle",
]

# error codes (EzpzError)
ERR_WRONG_NUMBER_GUESSES = -2
ERR_MISSING_GUESS = -3
ERR_MATRIX = -4
ERR_EMPTY_SYSTEM = -8
ERR_NO_DEVICE = -100


class IdGenerator:
    """id.rs:5-30"""

    def __init__(self):
        self._next = 0

    def next_id(self) -> Id:
        out = self._next
        self._next += 1
        return out


@dataclass(frozen=True)
class DatumDistance:
    id: Id

    @staticmethod
    def new(id: Id) -> "DatumDistance":
        return DatumDistance(id)


@dataclass(frozen=True)
class DatumPoint:
    x_id: Id
    y_id: Id

    @staticmethod
    def new(ids: IdGenerator) -> "DatumPoint":
        return DatumPoint(ids.next_id(), ids.next_id())

    @staticmethod
    def new_xy(x: Id, y: Id) -> "DatumPoint":
        return DatumPoint(x, y)

    def id_x(self) -> Id:
        return self.x_id

    def id_y(self) -> Id:
        return self.y_id

    def _ids(self):
        return [self.x_id, self.y_id]


@dataclass(frozen=True)
class DatumLineSegment:
    p0: DatumPoint
    p1: DatumPoint

    @staticmethod
    def new(p0: DatumPoint, p1: DatumPoint) -> "DatumLineSegment":
        return DatumLineSegment(p0, p1)

    def _ids(self):
        return self.p0._ids() + self.p1._ids()


@dataclass(frozen=True)
class DatumCircle:
    center: DatumPoint
    radius: DatumDistance

    def _ids(self):
        return self.center._ids() + [self.radius.id]


@dataclass(frozen=True)
class DatumCircularArc:
    center: DatumPoint
    start: DatumPoint
    end: DatumPoint

    def _ids(self):
        return self.center._ids() + self.start._ids() + self.end._ids()


@dataclass(frozen=True)
class Angle:
    """datatypes.rs:18-73"""

    val: float
    degrees: bool

    @staticmethod
    def from_degrees(v: float) -> "Angle":
        return Angle(float(v), True)

    @staticmethod
    def from_radians(v: float) -> "Angle":
        return Angle(float(v), False)

    def to_degrees(self) -> float:
        return self.val if self.degrees else self.val * (180.0 / math.pi)

    def to_radians(self) -> float:
        return self.val * (math.pi / 180.0) if self.degrees else self.val

    def __str__(self):
        return f"{self.val}deg" if self.degrees else f"{self.val}rad"


class AngleKind:
    """datatypes.rs:9-16"""

    Parallel = "Parallel"
    Perpendicular = "Perpendicular"

    @staticmethod
    def Other(angle: Angle):
        return ("Other", angle)

    @staticmethod
    def _encode(kind) -> Tuple[int, float]:
        if kind == AngleKind.Parallel:
            return 0, 0.0
        if kind == AngleKind.Perpendicular:
            return 1, 0.0
        _, angle = kind
        return (2 if angle.degrees else 3), angle.val


class LineSide:
    Undefined, Left, Right = 0, 1, 2


class CircleSide:
    Undefined, Exterior, Interior = 0, 1, 2


def _rec(kind: int, ids: Sequence[int], param: float = 0.0, tag: int = 0):
    r = np.zeros((), dtype=CONSTRAINT_DTYPE)
    r["kind"] = kind
    r["tag"] = tag
    r["param"] = param
    r["weight"] = 1.0
    a = np.zeros(8, np.uint32)
    a[: len(ids)] = np.asarray(list(ids), dtype=np.uint32)
    r["ids"] = a
    return r


class Constraint:
    """constraints.rs:37-93.  One classmethod per enum variant, same field order."""

    __slots__ = ("record",)

    def __init__(self, record):
        self.record = record

    @property
    def kind(self) -> int:
        return int(self.record["kind"])

    def constraint_kind(self) -> str:
        return KIND_NAMES[self.kind]

    def __repr__(self):
        n = [7, 6, 4, 5, 4, 4, 4, 4, 8, 1, 2, 4, 3, 8, 6, 6, 6, 6, 6, 6, 8, 8, 6, 6, 6][self.kind]
        return f"{self.constraint_kind()}(ids={self.record['ids'][:n].tolist()}, param={float(self.record['param'])}, tag={int(self.record['tag'])})"

    @staticmethod
    def LineTangentToCircle(line: DatumLineSegment, circle: DatumCircle, side=LineSide.Undefined):
        return Constraint(_rec(LINE_TANGENT_TO_CIRCLE, line._ids() + circle._ids(), tag=side))

    @staticmethod
    def CircleTangentToCircle(a: DatumCircle, b: DatumCircle, side=CircleSide.Undefined):
        return Constraint(_rec(CIRCLE_TANGENT_TO_CIRCLE, a._ids() + b._ids(), tag=side))

    @staticmethod
    def Distance(p0: DatumPoint, p1: DatumPoint, d: float):
        return Constraint(_rec(DISTANCE, p0._ids() + p1._ids(), d))

    @staticmethod
    def DistanceVar(p0: DatumPoint, p1: DatumPoint, d: DatumDistance):
        return Constraint(_rec(DISTANCE_VAR, p0._ids() + p1._ids() + [d.id]))

    @staticmethod
    def VerticalDistance(p0: DatumPoint, p1: DatumPoint, d: float):
        return Constraint(_rec(VERTICAL_DISTANCE, p0._ids() + p1._ids(), d))

    @staticmethod
    def HorizontalDistance(p0: DatumPoint, p1: DatumPoint, d: float):
        return Constraint(_rec(HORIZONTAL_DISTANCE, p0._ids() + p1._ids(), d))

    @staticmethod
    def Vertical(line: DatumLineSegment):
        return Constraint(_rec(VERTICAL, line._ids()))

    @staticmethod
    def Horizontal(line: DatumLineSegment):
        return Constraint(_rec(HORIZONTAL, line._ids()))

    @staticmethod
    def LinesAtAngle(l0: DatumLineSegment, l1: DatumLineSegment, kind):
        tag, val = AngleKind._encode(kind)
        return Constraint(_rec(LINES_AT_ANGLE, l0._ids() + l1._ids(), val, tag))

    @staticmethod
    def Fixed(id: Id, value: float):
        return Constraint(_rec(FIXED, [id], value))

    @staticmethod
    def ScalarEqual(a: Id, b: Id):
        return Constraint(_rec(SCALAR_EQUAL, [a, b]))

    @staticmethod
    def PointsCoincident(p0: DatumPoint, p1: DatumPoint):
        return Constraint(_rec(POINTS_COINCIDENT, p0._ids() + p1._ids()))

    @staticmethod
    def CircleRadius(circle: DatumCircle, r: float):
        return Constraint(_rec(CIRCLE_RADIUS, circle._ids(), r))

    @staticmethod
    def LinesEqualLength(l0: DatumLineSegment, l1: DatumLineSegment):
        return Constraint(_rec(LINES_EQUAL_LENGTH, l0._ids() + l1._ids()))

    @staticmethod
    def ArcRadius(arc: DatumCircularArc, r: float):
        return Constraint(_rec(ARC_RADIUS, arc._ids(), r))

    @staticmethod
    def Arc(arc: DatumCircularArc):
        return Constraint(_rec(ARC, arc._ids()))

    @staticmethod
    def Midpoint(line: DatumLineSegment, point: DatumPoint):
        return Constraint(_rec(MIDPOINT, line._ids() + point._ids()))

    @staticmethod
    def PointLineDistance(point: DatumPoint, line: DatumLineSegment, d: float):
        return Constraint(_rec(POINT_LINE_DISTANCE, point._ids() + line._ids(), d))

    @staticmethod
    def VerticalPointLineDistance(point: DatumPoint, line: DatumLineSegment, d: float):
        return Constraint(_rec(VERTICAL_POINT_LINE_DISTANCE, point._ids() + line._ids(), d))

    @staticmethod
    def HorizontalPointLineDistance(point: DatumPoint, line: DatumLineSegment, d: float):
        return Constraint(_rec(HORIZONTAL_POINT_LINE_DISTANCE, point._ids() + line._ids(), d))

    @staticmethod
    def Symmetric(line: DatumLineSegment, a: DatumPoint, b: DatumPoint):
        return Constraint(_rec(SYMMETRIC, line._ids() + a._ids() + b._ids()))

    @staticmethod
    def PointArcCoincident(arc: DatumCircularArc, point: DatumPoint):
        return Constraint(_rec(POINT_ARC_COINCIDENT, arc._ids() + point._ids()))

    @staticmethod
    def ArcLength(arc: DatumCircularArc, d: float):
        return Constraint(_rec(ARC_LENGTH, arc._ids(), d))

    @staticmethod
    def ArcAngle(arc: DatumCircularArc, angle: Angle):
        return Constraint(_rec(ARC_ANGLE, arc._ids(), angle.val, 2 if angle.degrees else 3))

    @staticmethod
    def PointsAtAngle(p0: DatumPoint, p1: DatumPoint, p2: DatumPoint, kind):
        tag, val = AngleKind._encode(kind)
        return Constraint(_rec(POINTS_AT_ANGLE, p0._ids() + p1._ids() + p2._ids(), val, tag))

    # constraints/composite.rs:9-62
    @staticmethod
    def lines_parallel(lines):
        return Constraint.LinesAtAngle(lines[0], lines[1], AngleKind.Parallel)

    @staticmethod
    def lines_perpendicular(lines):
        return Constraint.LinesAtAngle(lines[0], lines[1], AngleKind.Perpendicular)

    @staticmethod
    def point_bisects_arc(arc: DatumCircularArc, point: DatumPoint):
        return [Constraint.PointArcCoincident(arc, point),
                Constraint.Symmetric(DatumLineSegment(arc.center, point), arc.start, arc.end)]

    @staticmethod
    def parallel_lines_distance(lines, distance: float):
        return [Constraint.lines_parallel(lines), Constraint.PointLineDistance(lines[0].p0, lines[1], distance)]

    @staticmethod
    def circle_arc_coincident(circle: DatumCircle, arc: DatumCircularArc):
        return [Constraint.PointsCoincident(circle.center, arc.center),
                Constraint.LinesEqualLength(DatumLineSegment(arc.center, arc.start),
                                            DatumLineSegment(arc.center, arc.end))]


class ConstraintRequest:
    """constraint_request.rs:5-60"""

    __slots__ = ("_constraint", "_priority", "_weight")

    def __init__(self, constraint: Constraint, priority: int, weight: float = 1.0):
        self._constraint, self._priority, self._weight = constraint, int(priority), float(weight)

    @staticmethod
    def new(constraint: Constraint, priority: int) -> "ConstraintRequest":
        return ConstraintRequest(constraint, priority)

    @staticmethod
    def highest_priority(constraint: Constraint) -> "ConstraintRequest":
        return ConstraintRequest(constraint, 0)

    def with_weight(self, weight: float) -> "ConstraintRequest":
        return ConstraintRequest(self._constraint, self._priority, weight)

    def constraint(self) -> Constraint:
        return self._constraint

    def priority(self) -> int:
        return self._priority

    def weight(self) -> float:
        return self._weight

    def record(self):
        r = self._constraint.record.copy()
        r["priority"] = self._priority
        r["weight"] = self._weight
        return r


@dataclass(frozen=True)
class Config:
    """solver.rs:31-81"""

    max_iterations: int = 35
    residual_tolerance: float = 1e-8
    step_tolerance: float = 1e-12
    initial_lambda: float = 1e-9

    def with_max_iterations(self, v: int) -> "Config":
        return Config(int(v), self.residual_tolerance, self.step_tolerance, self.initial_lambda)

    def with_convergence_tolerance(self, v: float) -> "Config":
        return Config(self.max_iterations, float(v), self.step_tolerance, self.initial_lambda)

    def with_step_tolerance(self, v: float) -> "Config":
        return Config(self.max_iterations, self.residual_tolerance, float(v), self.initial_lambda)

    def with_initial_lambda(self, v: float) -> "Config":
        return Config(self.max_iterations, self.residual_tolerance, self.step_tolerance, float(v))

    def _c(self) -> CConfig:
        return CConfig(self.max_iterations, self.residual_tolerance, self.step_tolerance, self.initial_lambda)


@dataclass(frozen=True)
class GuardConfig:
    """EzpzGuardConfig, the policy of a guarded sweep: a step's fraction is halved at most max_halvings times (0 .. 20), a step
    takes at most max_attempts solves (>= 1), and an attempt that moves any value further than max_move from the last accepted
    ones is rejected (0: no such test).  Policy defaults (ezpz_default_guard_config), not measurements."""

    max_halvings: int = 4
    max_attempts: int = 12
    max_move: float = 0.0

    def _c(self) -> CGuardConfig:
        if not (0 <= int(self.max_halvings) <= 20 and 1 <= int(self.max_attempts) <= 0xFFFFFFFF and math.isfinite(self.max_move)):
            raise ValueError(f"guard: max_halvings in 0..20, max_attempts >= 1, a finite max_move, got {self}")
        return CGuardConfig(int(self.max_halvings), int(self.max_attempts), float(self.max_move))


@dataclass
class RedundancyConfig:
    """EzpzRedundancyConfig: a row that keeps more than rank_tol of its length is independent, a dependent row whose unweighted
    leftover residual exceeds conflict_tol conflicts, an accepted row with a share above group_tol joins a conflict group."""

    rank_tol: float = 1e-6
    conflict_tol: float = 1e-4
    group_tol: float = 1e-6

    def _c(self) -> CRedundancyConfig:
        return CRedundancyConfig(self.rank_tol, self.conflict_tol, self.group_tol)


class WarningContent:
    Degenerate, ShouldBeParallel, ShouldBePerpendicular = 0, 1, 2


@dataclass(frozen=True)
class Warning:
    about_constraint: Optional[int]
    content: int


@dataclass
class RawResult:
    """Flat result of ezpz_solve (EzpzOutcome + buffers); what tests/cases.py consumes."""

    error: int
    err_constraint_id: int
    err_variable: int
    final_values: np.ndarray
    iterations: int
    converged: bool
    unsatisfied: List[int]
    warnings: List[Tuple[int, int]]
    priority_solved: int
    num_vars: int
    num_eqs: int
    final_lambda: float
    final_residual_inf: float
    underconstrained: Optional[List[int]] = None  # FreedomAnalysis; None = not requested


class NonLinearSystemError(Exception):
    """error.rs:35-86"""

    def __init__(self, code: int, constraint_id: int = -1, variable: int = -1):
        self.code, self.constraint_id, self.variable = code, constraint_id, variable
        msg = lib().ezpz_error_string(code).decode()
        if code == ERR_MISSING_GUESS:
            msg = (f"Constraint {constraint_id} references variable {variable} but no such variable appears in "
                   "your initial guesses.")
        super().__init__(msg)


class FailureOutcome(Exception):
    """solve_outcome.rs:126-136"""

    def __init__(self, error: NonLinearSystemError, warnings, num_vars, num_eqs):
        super().__init__(str(error))
        self.error, self.warnings, self.num_vars, self.num_eqs = error, warnings, num_vars, num_eqs


class SolveOutcome:
    """solve_outcome.rs:12-100"""

    def __init__(self, raw: RawResult):
        self._raw = raw

    def unsatisfied(self) -> List[int]:
        return self._raw.unsatisfied

    def converged(self) -> bool:
        return self._raw.converged

    def final_values(self) -> np.ndarray:
        return self._raw.final_values

    def iterations(self) -> int:
        return self._raw.iterations

    def warnings(self) -> List[Warning]:
        return [Warning(a, c) for a, c in self._raw.warnings]

    def priority_solved(self) -> int:
        return self._raw.priority_solved

    def final_value_distance(self, d: DatumDistance) -> float:
        return float(self._raw.final_values[d.id])

    def final_value_point(self, p: DatumPoint):
        return (float(self._raw.final_values[p.x_id]), float(self._raw.final_values[p.y_id]))

    def final_value_arc(self, arc: DatumCircularArc):
        return {"a": self.final_value_point(arc.start), "b": self.final_value_point(arc.end),
                "center": self.final_value_point(arc.center)}

    def final_value_circle(self, c: DatumCircle):
        return {"center": self.final_value_point(c.center), "radius": self.final_value_distance(c.radius)}

    def is_satisfied(self) -> bool:
        return not self._raw.unsatisfied

    def is_unsatisfied(self) -> bool:
        return bool(self._raw.unsatisfied)


def _ptr(a):
    """The address ctypes takes for an optional array: None for None and for an empty one."""
    return a.ctypes.data if a is not None and a.size else None


def stack_records(records) -> np.ndarray:
    if isinstance(records, np.ndarray) and records.dtype == CONSTRAINT_DTYPE:
        return np.ascontiguousarray(records).reshape(-1)
    out = np.zeros(len(records), dtype=CONSTRAINT_DTYPE)
    for i, r in enumerate(records):
        out[i] = r
    return out


def _split_guesses(guesses):
    if isinstance(guesses, np.ndarray) and guesses.ndim == 1 and guesses.dtype.kind == "f":
        ids = np.arange(len(guesses), dtype=np.uint32)
        vals = np.ascontiguousarray(guesses, dtype=np.float64)
    else:
        ids = np.ascontiguousarray([g[0] for g in guesses], dtype=np.uint32)
        vals = np.ascontiguousarray([g[1] for g in guesses], dtype=np.float64)
    return ids, vals


def solve_records(records, guesses, config: Optional[Config] = None, warn_cap: int = 4096,
                  analysis: bool = False, inner: bool = False, orig_ids=None) -> RawResult:
    """`ezpz_solve` (or `ezpz_solve_analysis`) on a record array; never raises for solver errors (error code in the
    result).  inner=True: `ezpz_solve_inner` (lib.rs:265-356) on the records as they stand -- one tier, no side inferred --
    with `orig_ids` (optional, one per record) as the ids it reports."""
    a = stack_records(records)
    ids, vals = _split_guesses(guesses)
    n = len(vals)
    cfg = (config or Config())._c()
    x_out = np.zeros(max(n, 1))
    unsat = np.zeros(max(len(a), 1), dtype=np.uint64)
    warns = (CWarning * max(warn_cap, 1))()
    out = COutcome()
    args = (a.ctypes.data if len(a) else None, len(a), ids.ctypes.data if n else None,
            vals.ctypes.data if n else None, n, C.byref(cfg), x_out.ctypes.data, unsat.ctypes.data,
            C.cast(warns, C.c_void_p), warn_cap, C.byref(out))
    under = np.zeros(max(n, 1), dtype=np.uint32)
    n_under = C.c_uint64(0)
    if inner:
        assert not analysis, "ezpz_solve_inner has no FreedomAnalysis"
        oid = None if orig_ids is None else np.ascontiguousarray(orig_ids, dtype=np.uint64)
        lib().ezpz_solve_inner(args[0], oid.ctypes.data if oid is not None and len(oid) else None, *args[1:])
    elif analysis:
        lib().ezpz_solve_analysis(*args, under.ctypes.data, C.byref(n_under))
    else:
        lib().ezpz_solve(*args)
    nw = min(int(out.n_warnings), warn_cap)
    return RawResult(
        underconstrained=under[: n_under.value].astype(int).tolist() if analysis else None,
        error=out.error, err_constraint_id=out.err_constraint_id, err_variable=out.err_variable,
        final_values=x_out[:n].copy(), iterations=int(out.iterations), converged=bool(out.converged),
        unsatisfied=unsat[: int(out.n_unsatisfied)].astype(int).tolist(),
        warnings=[(warns[i].about_constraint, warns[i].content) for i in range(nw)],
        priority_solved=int(out.priority_solved), num_vars=int(out.num_vars), num_eqs=int(out.num_eqs),
        final_lambda=out.final_lambda, final_residual_inf=out.final_residual_inf)


def solve(reqs: Iterable[ConstraintRequest], initial_guesses: Sequence[Tuple[Id, float]],
          config: Optional[Config] = None) -> SolveOutcome:
    """`ezpz::solve` (lib.rs:80-87): returns a SolveOutcome or raises FailureOutcome."""
    raw = solve_records([r.record() for r in reqs], list(initial_guesses), config)
    if raw.error != 0:
        err = NonLinearSystemError(raw.error, raw.err_constraint_id, raw.err_variable)
        raise FailureOutcome(err, [Warning(a, c) for a, c in raw.warnings], raw.num_vars, raw.num_eqs)
    return SolveOutcome(raw)


class FreedomAnalysis:
    """analysis.rs:24-77"""

    def __init__(self, underconstrained: List[int]):
        self._under = list(underconstrained)

    def is_underconstrained(self) -> bool:
        return bool(self._under)

    def underconstrained(self) -> List[int]:
        return self._under

    def into_underconstrained(self) -> List[int]:
        return self._under


class SolveOutcomeFreedomAnalysis:
    """solve_outcome.rs: `analysis` + `outcome`."""

    def __init__(self, raw: RawResult):
        self.analysis = FreedomAnalysis(raw.underconstrained or [])
        self.outcome = SolveOutcome(raw)


def solve_analysis(reqs: Iterable[ConstraintRequest], initial_guesses: Sequence[Tuple[Id, float]],
                   config: Optional[Config] = None) -> SolveOutcomeFreedomAnalysis:
    """`ezpz::solve_analysis` (lib.rs:134-146)."""
    raw = solve_records([r.record() for r in reqs], list(initial_guesses), config, analysis=True)
    if raw.error != 0:
        err = NonLinearSystemError(raw.error, raw.err_constraint_id, raw.err_variable)
        raise FailureOutcome(err, [Warning(a, c) for a, c in raw.warnings], raw.num_vars, raw.num_eqs)
    return SolveOutcomeFreedomAnalysis(raw)


def solve_batch(reqs, x0: np.ndarray, config: Optional[Config] = None, want_mask: bool = False):
    """`ezpz::solve` semantics (side inference, priority tiers) for a batch of guess vectors sharing one request list.

    reqs: ConstraintRequests or 56-byte records; x0: [batch, n_vars].  Returns (x, status, priority_solved, mask|None)."""
    recs = stack_records([r.record() if isinstance(r, ConstraintRequest) else r for r in reqs]
                         if not isinstance(reqs, np.ndarray) else reqs)
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    batch, n = x0.shape
    cfg = (config or Config())._c()
    x = np.empty_like(x0)
    st = np.zeros(batch, dtype=STATUS_DTYPE)
    prio = np.zeros(batch, dtype=np.uint32)
    mask = np.zeros((batch, max(len(recs), 1)), dtype=np.uint8) if want_mask else None
    ec, ev = C.c_int32(-1), C.c_int64(-1)
    rc = lib().ezpz_solve_batch(recs.ctypes.data if len(recs) else None, len(recs), n, x0.ctypes.data, batch,
                                C.byref(cfg), x.ctypes.data, st.ctypes.data, prio.ctypes.data,
                                mask.ctypes.data if want_mask else None, C.byref(ec), C.byref(ev))
    if rc != 0:
        raise NonLinearSystemError(rc, ec.value, ev.value)
    return x, st, prio, mask


def specialized_source(records, n_vars: int, compile=False, wave=False) -> str:
    """`ezpz_specialized_source`: the generated source of the request's class-specialised kernel ('' = none); with
    compile=True it is also compiled for gfx950 (hiprtc; no device needed) and a failure raises with the log;
    compile="cached": through the on-disk cache of code objects, like the solve entry points."""
    recs = stack_records(records)
    buf = C.create_string_buffer(1 << 22)
    rc = lib().ezpz_specialized_source(recs.ctypes.data if len(recs) else None, len(recs), int(n_vars),
                                       (2 if compile == "cached" else 1 if compile else 0) | (4 if wave else 0), buf, len(buf))
    if rc < 0:
        raise RuntimeError("run-time compilation failed:\n" + buf.value.decode(errors="replace")[-4000:])
    return buf.value.decode() if rc > 0 else ""


def host_register(array: np.ndarray) -> None:
    """`ezpz_host_register`: page-locks a (contiguous) array the caller will pass to batch calls again and again."""
    rc = lib().ezpz_host_register(array.ctypes.data, array.nbytes)
    if rc != 0:
        raise NonLinearSystemError(rc)


def host_unregister(array: np.ndarray) -> None:
    rc = lib().ezpz_host_unregister(array.ctypes.data)
    if rc != 0:
        raise NonLinearSystemError(rc)


def resolve_sides(records, values) -> np.ndarray:
    """`Constraint::set_from_initial_values` (constraints.rs:146-193) over a request list: a copy of `records` in which
    every undefined LineSide / CircleSide is the one `values` (by id) imply.  `System` takes side-resolved records."""
    recs = stack_records(records).copy()
    vals = np.ascontiguousarray(values, dtype=np.float64)
    rc = lib().ezpz_resolve_sides(recs.ctypes.data if len(recs) else None, len(recs),
                                  vals.ctypes.data if len(vals) else None, len(vals))
    if rc != 0:
        raise NonLinearSystemError(rc)
    return recs


TEAM_AUTO_LISTS = 0xFFFFFFFE  # `team_size`: automatic, list-walk shapes only (never component-resident)
TEAM_BATCH_LANES = 0xFFFFFFFD  # `team_size`: automatic, connected sketches one lane per system at every batch size
TEAM_LATENCY_PHASES = 0xFFFFFFFC  # `team_size`: TEAM_AUTO_LATENCY without the record walk (dense phases instead)
TEAM_LATENCY_WAVE = 0xFFFFFFFB  # `team_size`: TEAM_AUTO_LATENCY, a small system always on one wavefront per system where that form exists
TEAM_LATENCY_RECORDS = 0xFFFFFFF9  # `team_size`: TEAM_AUTO_LATENCY without the frontal shape (the record walk, as before round 5)
TEAM_FRONTS = 0xFFFFFFFA  # `team_size`: the frontal shape (team_mode 5) whatever the size of the system, TEAM_AUTO_LATENCY behind it
TEAM_AUTO_LATENCY = 0xFFFFFFFF  # `team_size`: choose for the latency of one solve instead of batch throughput (ezpz_amd.h)


class System:
    """One analysed topology resident on a device: `ezpz_system_create` + batched solves.

    This is the batch mode that has no counterpart in the reference (it solves one system per call);
    every system of a batch shares the constraint list and differs only in its initial guesses.
    """

    def __init__(self, records, n_vars: int, device: int = 0, team_size: int = 0):
        self.records = stack_records(records)
        self.n_vars = int(n_vars)
        self.device = device
        h = C.c_void_p()
        ec, ev = C.c_int32(-1), C.c_int64(-1)
        rc = lib().ezpz_system_create(self.records.ctypes.data if len(self.records) else None, len(self.records),
                                      self.n_vars, device, team_size, C.byref(h), C.byref(ec), C.byref(ev))
        if rc != 0:
            raise NonLinearSystemError(rc, ec.value, ev.value)
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:  # (at interpreter shutdown the module's globals may be gone already)
            lib().ezpz_system_destroy(h)
            self._h = None

    def specialize(self, wait: bool = True) -> int:
        """`ezpz_system_specialize`: 2 = the class-specialised kernel is ready, 1 = compiling, 0 = none for this system."""
        rc = lib().ezpz_system_specialize(self._h, 1 if wait else 0)
        if rc < 0:
            raise NonLinearSystemError(rc)
        return rc

    def info(self) -> dict:
        i = CSystemInfo()
        lib().ezpz_system_info(self._h, C.byref(i))
        return {f: getattr(i, f) for f, _ in CSystemInfo._fields_}

    def solve_batch_logged(self, x0: np.ndarray, config: Optional[Config] = None, warn_cap: int = 1024):
        """solve_batch plus the Degenerate warnings of every system: a list per system of (pass, constraint position)
        in the reference's chronological order (the kernel's log entries sorted), truncated to warn_cap."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1, max(self.n_vars, 1))
        batch = x0.shape[0]
        cfg = (config or Config())._c()
        x = np.empty_like(x0)
        st = np.zeros(batch, dtype=STATUS_DTYPE)
        log = np.zeros((batch, warn_cap), dtype=np.uint64)
        rc = lib().ezpz_system_solve_batch(self._h, x0.ctypes.data, batch, C.byref(cfg), x.ctypes.data, st.ctypes.data,
                                           None, log.ctypes.data, warn_cap)
        if rc != 0:
            raise NonLinearSystemError(rc)
        logs = []
        for b in range(batch):
            e = np.sort(log[b, : min(int(st["n_warnings"][b]), warn_cap)])
            logs.append([(int(v >> np.uint64(32)), int(v & np.uint64(0xFFFFFFFF))) for v in e])
        return x, st, logs

    def solve_batch(self, x0: np.ndarray, config: Optional[Config] = None, want_mask: bool = False):
        """Host arrays in/out.  x0 [batch, n_vars] -> (x [batch, n_vars], status (STATUS_DTYPE), mask or None)."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1, max(self.n_vars, 1))
        batch = x0.shape[0]
        cfg = (config or Config())._c()
        x = np.empty_like(x0)
        st = np.zeros(batch, dtype=STATUS_DTYPE)
        mask = np.zeros((batch, max(len(self.records), 1)), dtype=np.uint8) if want_mask else None
        rc = lib().ezpz_system_solve_batch(self._h, x0.ctypes.data, batch, C.byref(cfg), x.ctypes.data,
                                           st.ctypes.data, mask.ctypes.data if want_mask else None, None, 0)
        if rc != 0:
            raise NonLinearSystemError(rc)
        return x, st, mask

    def eval_batch(self, x: np.ndarray):
        """Residual + Jacobian sweep only.  Returns (r [batch, m], dense J [batch, m, n], degenerate counts)."""
        info = self.info()
        m, zj, n = info["n_rows"], info["nnz_j"], self.n_vars
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, max(n, 1))
        batch = x.shape[0]
        r = np.zeros((batch, max(m, 1)))
        jv = np.zeros((batch, max(zj, 1)))
        deg = np.zeros(batch, np.uint32)
        rc = lib().ezpz_system_eval_batch(self._h, x.ctypes.data, batch, r.ctypes.data, jv.ctypes.data,
                                          deg.ctypes.data)
        if rc != 0:
            raise NonLinearSystemError(rc)
        rows, cols = np.zeros(max(zj, 1), np.uint32), np.zeros(max(zj, 1), np.uint32)
        lib().ezpz_system_jacobian_pattern(self._h, rows.ctypes.data, cols.ctypes.data)
        J = np.zeros((batch, m, n))
        J[:, rows[:zj], cols[:zj]] = jv[:, :zj]
        return r[:, :m], J, deg

    def residual_field(self, x_base, var_x: int, var_y: int, viewport, constraint: Optional[int] = None,
                       want: Sequence[str] = ("mag", "rgb"), overlay=None):
        """The residual magnitude as a 2-D field while variables var_x / var_y sweep `viewport` (residual_viz.residual_field)."""
        from . import residual_viz

        return residual_viz.residual_field(self, x_base, var_x, var_y, viewport, constraint, want, overlay)

    def freedom_batch(self, x: np.ndarray):
        """FreedomAnalysis (find_dof.rs) of each value vector.  Returns (mask [batch, n] uint8, participation)."""
        n = self.n_vars
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, max(n, 1))
        batch = x.shape[0]
        mask = np.zeros((batch, max(n, 1)), np.uint8)
        part = np.zeros((batch, max(n, 1)))
        rc = lib().ezpz_system_freedom_batch(self._h, x.ctypes.data, batch, mask.ctypes.data, part.ctypes.data)
        if rc != 0:
            raise NonLinearSystemError(rc)
        return mask, part

    def freedom_batch_device(self, x_ptr: int, batch: int, mask_ptr: int, part_ptr: int = 0, count_ptr: int = 0,
                             stream: int = 0) -> None:
        rc = lib().ezpz_system_freedom_batch_device(self._h, x_ptr, batch, mask_ptr, part_ptr or None,
                                                    count_ptr or None, stream or None)
        if rc != 0:
            raise NonLinearSystemError(rc)

    INDEPENDENT, ZERO, REDUNDANT, CONFLICTING = 0, 1, 2, 3  # the statuses of `redundancy`

    def redundancy(self, x: np.ndarray, focus=None, config: Optional[RedundancyConfig] = None, want_rows: bool = False):
        """Redundancy analysis (`ezpz_system_redundancy`) of each value vector x [batch, n_vars], normally a solve's answers: the
        rows of the weighted Jacobian are visited in request order, and a row that depends on earlier ones is REDUNDANT or -- its
        residual cannot be met together with theirs -- CONFLICTING; a row without entries at x is ZERO.  Returns a dict:
        "con_status" [batch, n_constraints] uint8 (the maximum over a constraint's rows), "rank" [batch] (independent rows),
        "row_status" [batch, n_rows] with want_rows, and with `focus` (constraint positions) "group" [batch, len(focus),
        n_constraints]: 1 for focus[k] and for every constraint whose accepted rows the dependent rows of focus[k] are made of."""
        n, n_cs = self.n_vars, len(self.records)
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, max(n, 1))
        batch = x.shape[0]
        f = self._positions(focus) if focus is not None else np.zeros(0, np.uint32)
        cfg = (config or RedundancyConfig())._c()
        con = np.zeros((batch, n_cs), np.uint8)
        rank = np.zeros(batch, np.uint32)
        rows = np.zeros((batch, max(self.info()["n_rows"], 1)), np.uint8) if want_rows else None
        group = np.zeros((batch, len(f), n_cs), np.uint8)
        rc = lib().ezpz_system_redundancy(self._h, x.ctypes.data, batch, C.byref(cfg), con.ctypes.data,
                                          rows.ctypes.data if want_rows else None, rank.ctypes.data,
                                          f.ctypes.data if len(f) else None, len(f), group.ctypes.data if len(f) else None)
        if rc != 0:
            raise NonLinearSystemError(rc)
        out = {"con_status": con, "rank": rank}
        if want_rows:
            out["row_status"] = rows[:, : self.info()["n_rows"]]
        if focus is not None:
            out["group"] = group
        return out

    def redundancy_device(self, x_ptr: int, batch: int, con_status_ptr: int, row_status_ptr: int = 0, rank_ptr: int = 0,
                          focus=None, group_ptr: int = 0, stream: int = 0, config: Optional[RedundancyConfig] = None) -> None:
        """Device pointers (e.g. torch tensors' data_ptr()) and a hipStream_t handle; enqueue only.  `focus` stays a host list."""
        f = self._positions(focus) if focus is not None else np.zeros(0, np.uint32)
        cfg = (config or RedundancyConfig())._c()
        rc = lib().ezpz_system_redundancy_device(self._h, x_ptr or None, batch, C.byref(cfg), con_status_ptr or None,
                                                 row_status_ptr or None, rank_ptr or None, f.ctypes.data if len(f) else None,
                                                 len(f), group_ptr or None, stream or None)
        if rc != 0:
            raise NonLinearSystemError(rc)

    def solve_batch_device(self, x0_ptr: int, batch: int, x_out_ptr: int, status_ptr: int, mask_ptr: int = 0,
                           stream: int = 0, config: Optional[Config] = None) -> None:
        """Device pointers (e.g. torch tensors' data_ptr()) and a hipStream_t handle; enqueue only."""
        cfg = (config or Config())._c()
        rc = lib().ezpz_system_solve_batch_device(self._h, x0_ptr, batch, C.byref(cfg), x_out_ptr, status_ptr,
                                                  mask_ptr or None, None, 0, stream or None)
        if rc != 0:
            raise NonLinearSystemError(rc)


    def _positions(self, positions) -> np.ndarray:
        p = np.asarray(positions)
        if p.ndim != 1 or (p.size and not np.issubdtype(p.dtype, np.integer)) or (p.size and (p.min() < 0 or p.max() > 0xFFFFFFFF)):
            raise ValueError("positions: a 1-D sequence of constraint positions (non-negative integers)")
        return np.ascontiguousarray(p, dtype=np.uint32)

    def set_params_route(self, route: str) -> None:
        """`ezpz_system_set_params_route`: "fronts" makes solve_batch_params, sweep_params (and torch_ops.solve_params) of this
        system run on the frontal shape -- only a system whose frontal plan serves every call (info()["front_max_batch"] ==
        0xFFFFFFFF) accepts it; "default" restores the entry's own route."""
        if route not in PARAMS_ROUTES:
            raise ValueError(f"route: one of {sorted(PARAMS_ROUTES)}, got {route!r}")
        rc = lib().ezpz_system_set_params_route(self._h, PARAMS_ROUTES[route])
        if rc != 0:
            raise NonLinearSystemError(rc)

    def solve_batch_params(self, x0: np.ndarray, positions, params: np.ndarray, config: Optional[Config] = None,
                           want_mask: bool = False):
        """`ezpz_system_solve_batch_params`: one topology, a dimension set per system.  params [batch, len(positions)] replaces
        records[positions[j]]["param"] for system b (in that field's units); constraints not listed keep their values.
        Returns what solve_batch returns."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1, max(self.n_vars, 1))
        batch = x0.shape[0]
        pos = self._positions(positions)
        params = np.ascontiguousarray(params, dtype=np.float64)
        if params.size != batch * len(pos) or (params.ndim == 2 and params.shape != (batch, len(pos))) or params.ndim > 2:
            raise ValueError(f"params: expected shape ({batch}, {len(pos)}), got {params.shape}")
        cfg = (config or Config())._c()
        x = np.empty_like(x0)
        st = np.zeros(batch, dtype=STATUS_DTYPE)
        mask = np.zeros((batch, max(len(self.records), 1)), dtype=np.uint8) if want_mask else None
        rc = lib().ezpz_system_solve_batch_params(self._h, x0.ctypes.data, pos.ctypes.data if len(pos) else None, len(pos),
                                                  params.ctypes.data if len(pos) else None, batch, C.byref(cfg), x.ctypes.data,
                                                  st.ctypes.data, mask.ctypes.data if want_mask else None, None, 0)
        if rc != 0:
            raise NonLinearSystemError(rc)
        return x, st, mask

    def solve_batch_params_device(self, x0_ptr: int, positions, params_ptr: int, batch: int, x_out_ptr: int, status_ptr: int,
                                  mask_ptr: int = 0, stream: int = 0, config: Optional[Config] = None) -> None:
        """Device pointers and a hipStream_t handle, like solve_batch_device; `positions` is a host sequence and params_ptr
        addresses [batch, len(positions)] doubles on the device."""
        pos = self._positions(positions)
        cfg = (config or Config())._c()
        rc = lib().ezpz_system_solve_batch_params_device(self._h, x0_ptr, pos.ctypes.data if len(pos) else None, len(pos),
                                                         params_ptr or None, batch, C.byref(cfg), x_out_ptr, status_ptr,
                                                         mask_ptr or None, None, 0, stream or None)
        if rc != 0:
            raise NonLinearSystemError(rc)


    def sweep_params(self, x0: np.ndarray, positions, params: np.ndarray, config: Optional[Config] = None, want_mask: bool = False,
                     warn_log: Optional[np.ndarray] = None):
        """`ezpz_system_sweep_params`: a chain of driven solves per system.  x0 [batch, n_vars] are the sweeps' starts, params
        [steps, batch, len(positions)] their dimension sets step by step; step k of sweep b starts from step k - 1's answer.
        Returns (x [steps, batch, n_vars], status [steps, batch], mask [steps, batch, n_cs] or None) -- exactly what `steps` chained
        solve_batch_params calls give.  warn_log: a C-contiguous uint64 array [steps, batch, warn_cap] of the caller's that receives
        the raw warning log (the first min(status["n_warnings"], warn_cap) entries of a row are written: pass << 32 | constraint
        position; the others are left as they are)."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1, max(self.n_vars, 1))
        batch = x0.shape[0]
        pos = self._positions(positions)
        params = np.ascontiguousarray(params, dtype=np.float64)
        if params.ndim != 3 or params.shape[1:] != (batch, len(pos)):
            raise ValueError(f"params: expected shape (steps, {batch}, {len(pos)}), got {params.shape}")
        steps = params.shape[0]
        warn_cap = 0
        if warn_log is not None:
            if (not isinstance(warn_log, np.ndarray) or warn_log.dtype != np.uint64 or not warn_log.flags.c_contiguous
                    or not warn_log.flags.writeable or warn_log.ndim != 3 or warn_log.shape[:2] != (steps, batch)):
                raise ValueError(f"warn_log: expected a writeable C-contiguous uint64 array of shape ({steps}, {batch}, warn_cap)")
            warn_cap = warn_log.shape[2]
        cfg = (config or Config())._c()
        x = np.empty((steps, batch, x0.shape[1]))
        st = np.zeros((steps, batch), dtype=STATUS_DTYPE)
        mask = np.zeros((steps, batch, max(len(self.records), 1)), dtype=np.uint8) if want_mask else None
        rc = lib().ezpz_system_sweep_params(self._h, x0.ctypes.data, pos.ctypes.data if len(pos) else None, len(pos),
                                            params.ctypes.data if len(pos) else None, steps, batch, C.byref(cfg), x.ctypes.data,
                                            st.ctypes.data, mask.ctypes.data if want_mask else None,
                                            warn_log.ctypes.data if warn_cap else None, warn_cap)
        if rc != 0:
            raise NonLinearSystemError(rc)
        return x, st, mask

    def sweep_params_device(self, x0_ptr: int, positions, params_ptr: int, steps: int, batch: int, x_out_ptr: int, status_ptr: int,
                            mask_ptr: int = 0, stream: int = 0, config: Optional[Config] = None) -> None:
        """Device pointers and a hipStream_t handle; enqueue only.  params_ptr addresses [steps, batch, len(positions)] doubles,
        x_out_ptr [steps, batch, n_vars], status_ptr [steps, batch] statuses, mask_ptr [steps, batch, n_cs] bytes; x0_ptr
        [batch, n_vars] may be x_out_ptr itself."""
        pos = self._positions(positions)
        cfg = (config or Config())._c()
        rc = lib().ezpz_system_sweep_params_device(self._h, x0_ptr or None, pos.ctypes.data if len(pos) else None, len(pos),
                                                   params_ptr or None, steps, batch, C.byref(cfg), x_out_ptr or None,
                                                   status_ptr or None, mask_ptr or None, None, 0, stream or None)
        if rc != 0:
            raise NonLinearSystemError(rc)

    def sweep_params_plan(self, positions) -> dict:
        """`ezpz_system_sweep_params_plan`: the route a sweep of this list takes (`route`, and its name as `route_name`), whether it is
        one launch (`in_kernel`), `params_in_lds`, `lds_bytes`.  Diagnostic."""
        pos = self._positions(positions)
        p = CSweepPlan()
        rc = lib().ezpz_system_sweep_params_plan(self._h, pos.ctypes.data if len(pos) else None, len(pos), C.byref(p))
        if rc != 0:
            raise NonLinearSystemError(rc)
        out = {f: getattr(p, f) for f, _ in CSweepPlan._fields_}
        out["route_name"] = SWEEP_ROUTE_NAMES[p.route]
        return out

    def driven_values(self, positions) -> np.ndarray:
        """The records' own values of the constraints at `positions`: what a system's guesses belong to before anything is driven."""
        pos = self._positions(positions)
        return np.array([self.records[int(p)]["param"] for p in pos], dtype=np.float64)

    def sweep_guarded(self, x0: np.ndarray, positions, params0, params: np.ndarray, guard: Optional[GuardConfig] = None,
                      config: Optional[Config] = None, want_mask: bool = False, warn_log: Optional[np.ndarray] = None):
        """`ezpz_system_sweep_guarded`: sweep_params with step control -- a step whose solve fails, leaves constraints unsatisfied
        or moves a value by more than guard.max_move is halved and tried again, and a sweep holds on to its last accepted answer
        (the rule: include/ezpz_amd.h).  x0 [batch, n_vars]; params0 [batch, len(positions)] the driven values x0 belongs to (None:
        the records' own, for every sweep); params [steps, batch, len(positions)] the targets.  Returns (x [steps, batch, n_vars],
        status [steps, batch] of each step's LAST attempt, mask [steps, batch, n_cs] or None, guard [steps, batch] with fields
        reached / attempts / accepted, params_reached [steps, batch, len(positions)]).  warn_log: as for sweep_params."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1, max(self.n_vars, 1))
        batch = x0.shape[0]
        pos = self._positions(positions)
        params = np.ascontiguousarray(params, dtype=np.float64)
        if len(pos) == 0 or params.ndim != 3 or params.shape[1:] != (batch, len(pos)):
            raise ValueError(f"params: expected shape (steps, {batch}, {len(pos)}) with at least one position, got {params.shape}")
        steps = params.shape[0]
        if params0 is None:
            params0 = np.tile(self.driven_values(pos), (batch, 1))
        params0 = np.ascontiguousarray(params0, dtype=np.float64)
        if params0.shape != (batch, len(pos)):
            raise ValueError(f"params0: expected shape ({batch}, {len(pos)}), got {params0.shape}")
        warn_cap = 0
        if warn_log is not None:
            if (not isinstance(warn_log, np.ndarray) or warn_log.dtype != np.uint64 or not warn_log.flags.c_contiguous
                    or not warn_log.flags.writeable or warn_log.ndim != 3 or warn_log.shape[:2] != (steps, batch)):
                raise ValueError(f"warn_log: expected a writeable C-contiguous uint64 array of shape ({steps}, {batch}, warn_cap)")
            warn_cap = warn_log.shape[2]
        cfg = (config or Config())._c()
        g = (guard or GuardConfig())._c()
        x = np.empty((steps, batch, x0.shape[1]))
        st = np.zeros((steps, batch), dtype=STATUS_DTYPE)
        gs = np.zeros((steps, batch), dtype=GUARD_STEP_DTYPE)
        reached = np.empty((steps, batch, len(pos)))
        mask = np.zeros((steps, batch, max(len(self.records), 1)), dtype=np.uint8) if want_mask else None
        rc = lib().ezpz_system_sweep_guarded(self._h, x0.ctypes.data, pos.ctypes.data, len(pos), params0.ctypes.data, params.ctypes.data,
                                             steps, batch, C.byref(cfg), C.byref(g), x.ctypes.data, st.ctypes.data, gs.ctypes.data,
                                             reached.ctypes.data, mask.ctypes.data if want_mask else None,
                                             warn_log.ctypes.data if warn_cap else None, warn_cap)
        if rc != 0:
            raise NonLinearSystemError(rc)
        return x, st, mask, gs, reached

    def sweep_guarded_device(self, x0_ptr: int, positions, params0_ptr: int, params_ptr: int, steps: int, batch: int, x_out_ptr: int,
                             status_ptr: int, guard_ptr: int, params_reached_ptr: int, mask_ptr: int = 0, log_ptr: int = 0,
                             warn_cap: int = 0, stream: int = 0, guard: Optional[GuardConfig] = None,
                             config: Optional[Config] = None) -> None:
        """Device pointers and a hipStream_t handle; one launch, enqueue only (routes without a guarded kernel are declined: see
        sweep_guarded_plan).  The layouts of sweep_params_device, with params0_ptr [batch, len(positions)], guard_ptr [steps, batch]
        EzpzGuardStep (GUARD_STEP_DTYPE) and params_reached_ptr [steps, batch, len(positions)]; x0_ptr must not overlap x_out_ptr."""
        pos = self._positions(positions)
        cfg = (config or Config())._c()
        g = (guard or GuardConfig())._c()
        rc = lib().ezpz_system_sweep_guarded_device(self._h, x0_ptr or None, pos.ctypes.data if len(pos) else None, len(pos),
                                                    params0_ptr or None, params_ptr or None, steps, batch, C.byref(cfg), C.byref(g),
                                                    x_out_ptr or None, status_ptr or None, guard_ptr or None, params_reached_ptr or None,
                                                    mask_ptr or None, log_ptr or None, warn_cap if log_ptr else 0, stream or None)
        if rc != 0:
            raise NonLinearSystemError(rc)

    def sweep_guarded_plan(self, positions) -> dict:
        """`ezpz_system_sweep_guarded_plan`: sweep_params_plan's fields for a guarded sweep; `in_kernel` is 1 where the device form
        serves the route in one launch and 0 where only the host form does.  Diagnostic."""
        pos = self._positions(positions)
        p = CSweepPlan()
        rc = lib().ezpz_system_sweep_guarded_plan(self._h, pos.ctypes.data if len(pos) else None, len(pos), C.byref(p))
        if rc != 0:
            raise NonLinearSystemError(rc)
        out = {f: getattr(p, f) for f, _ in CSweepPlan._fields_}
        out["route_name"] = SWEEP_ROUTE_NAMES[p.route]
        return out

    def set_sensitivity_route(self, route: str) -> None:
        """`ezpz_system_set_sensitivity_route`: "fronts" makes param_sensitivity, its device form (and the backward of
        torch_ops.solve_params) of this system run on the frontal plan -- one factorisation for many right-hand sides, no limit on
        the size of a component; only a system whose frontal plan serves every call accepts it; "default" restores the entry's
        own route.  The params route (set_params_route) is a setting of its own."""
        if route not in SENSITIVITY_ROUTES:
            raise ValueError(f"route: one of {sorted(SENSITIVITY_ROUTES)}, got {route!r}")
        rc = lib().ezpz_system_set_sensitivity_route(self._h, SENSITIVITY_ROUTES[route])
        if rc != 0:
            raise NonLinearSystemError(rc)

    def param_sensitivity(self, x: np.ndarray, positions, params: Optional[np.ndarray] = None, lam: Optional[float] = None,
                          want_degenerate: bool = False):
        """`ezpz_system_param_sensitivity`: S[b, j, :] = -(JtJ + lam I)^-1 Jt dr/dp_j at the values x [batch, n_vars] (normally a
        solve's answer) with params [batch, len(positions)] overlaid as solve_batch_params overlays them (None: the system's own
        values); per unit of the `param` field.  lam defaults to Config().initial_lambda.  Returns (S [batch, k, n_vars], status
        [batch] uint32: 1 where the factorisation failed and S[b] is NaN; on the fronts route also 2: a wait between workgroups ran out) -- and the degenerate counts with want_degenerate."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, max(self.n_vars, 1))
        batch = x.shape[0]
        pos = self._positions(positions)
        if params is not None:
            params = np.ascontiguousarray(params, dtype=np.float64)
            if params.size != batch * len(pos) or (params.ndim == 2 and params.shape != (batch, len(pos))) or params.ndim > 2:
                raise ValueError(f"params: expected shape ({batch}, {len(pos)}), got {params.shape}")
        lam = Config().initial_lambda if lam is None else float(lam)
        S = np.zeros((batch, len(pos), self.n_vars))
        st = np.zeros(batch, dtype=np.uint32)
        deg = np.zeros(batch, dtype=np.uint32) if want_degenerate else None
        rc = lib().ezpz_system_param_sensitivity(self._h, x.ctypes.data, pos.ctypes.data if len(pos) else None, len(pos),
                                                 params.ctypes.data if params is not None and len(pos) else None, batch, lam,
                                                 S.ctypes.data if S.size else None, st.ctypes.data,
                                                 deg.ctypes.data if want_degenerate else None)
        if rc != 0:
            raise NonLinearSystemError(rc)
        return (S, st, deg) if want_degenerate else (S, st)

    def param_sensitivity_device(self, x_ptr: int, positions, params_ptr: int, batch: int, S_ptr: int, status_ptr: int,
                                 lam: Optional[float] = None, degenerate_ptr: int = 0, stream: int = 0) -> None:
        """Device pointers and a hipStream_t handle; enqueue only (a `positions` list other than the last one is planned and
        uploaded first).  params_ptr 0: the system's own values."""
        pos = self._positions(positions)
        lam = Config().initial_lambda if lam is None else float(lam)
        rc = lib().ezpz_system_param_sensitivity_device(self._h, x_ptr or None, pos.ctypes.data if len(pos) else None, len(pos),
                                                        params_ptr or None, batch, lam, S_ptr or None, status_ptr or None,
                                                        degenerate_ptr or None, stream or None)
        if rc != 0:
            raise NonLinearSystemError(rc)

    def param_sensitivity_plan(self, positions) -> dict:
        """`ezpz_system_param_sensitivity_plan`: which launch shape the components of this list take (host only)."""
        pos = self._positions(positions)
        p = CSensitivityPlan()
        rc = lib().ezpz_system_param_sensitivity_plan(self._h, pos.ctypes.data if len(pos) else None, len(pos), C.byref(p))
        if rc != 0:
            raise NonLinearSystemError(rc)
        return {f: getattr(p, f) for f, _ in CSensitivityPlan._fields_}

    # ---- reference dimensions (ezpz_system_measure and its siblings) ----------------------------------------------------------
    def _measure_x(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim == 0 or x.shape[-1] != self.n_vars:
            raise ValueError(f"x: expected [..., {self.n_vars}], got {x.shape}")
        return x, x.shape[:-1], int(np.prod(x.shape[:-1], dtype=np.int64))

    def measure(self, x: np.ndarray, records, want_grad: bool = False, want_flags: bool = False):
        """`ezpz_system_measure`: the reference dimensions `records` (measurable constraint records: only kind, tag and ids are read)
        at the values x [..., n_vars] -- any leading shape, e.g. [steps, batch, n_vars] from a sweep, which the outputs keep.
        Returns m [..., n_meas] in the units of the records' `param` field; with want_grad also grad [..., n_meas, 8] (d m / d
        x[ids[slot]]), with want_flags also flags [..., n_meas] uint8 (bit 0: the residual's guard fired, m and grad are 0; bit 1:
        a gradient guard fired) -- as a tuple in that order."""
        x, lead, batch = self._measure_x(x)
        recs = stack_records(records)
        k = len(recs)
        m = np.zeros(lead + (k,))
        grad = np.zeros(lead + (k, 8)) if want_grad else None
        flags = np.zeros(lead + (k,), np.uint8) if want_flags else None
        rc = lib().ezpz_system_measure(self._h, recs.ctypes.data if k else None, k, x.ctypes.data if x.size else None, batch,
                                       m.ctypes.data if m.size else None, flags.ctypes.data if want_flags and flags.size else None,
                                       grad.ctypes.data if want_grad and grad.size else None)
        if rc != 0:
            raise NonLinearSystemError(rc)
        if not (want_grad or want_flags):
            return m
        return (m,) + ((grad,) if want_grad else ()) + ((flags,) if want_flags else ())

    def measure_response(self, x: np.ndarray, records, S: np.ndarray, tol=None):
        """`ezpz_system_measure_response`: D [..., n_meas, n_param] = how each reference dimension answers to each driving dimension,
        from S [..., n_param, n_vars] (`param_sensitivity` at the same x).  With tol [n_param] (non-negative) also the tolerance
        stack-up: returns (D, worst [..., n_meas], rss [..., n_meas])."""
        x, lead, batch = self._measure_x(x)
        recs = stack_records(records)
        k = len(recs)
        S = np.ascontiguousarray(S, dtype=np.float64)
        if S.ndim < 2 or S.shape[:-2] != lead or S.shape[-1] != self.n_vars:
            raise ValueError(f"S: expected {lead + ('n_param', self.n_vars)}, got {S.shape}")
        n_param = S.shape[-2]
        D = np.zeros(lead + (k, n_param))
        if tol is not None:
            tol = np.ascontiguousarray(tol, dtype=np.float64)
            if tol.shape != (n_param,):
                raise ValueError(f"tol: expected shape ({n_param},), got {tol.shape}")
            worst, rss = np.zeros(lead + (k,)), np.zeros(lead + (k,))
        rc = lib().ezpz_system_measure_response(self._h, recs.ctypes.data if k else None, k, x.ctypes.data if x.size else None,
                                                S.ctypes.data if S.size else None, n_param, batch,
                                                tol.ctypes.data if tol is not None else None, D.ctypes.data if D.size else None,
                                                worst.ctypes.data if tol is not None else None,
                                                rss.ctypes.data if tol is not None else None)
        if rc != 0:
            raise NonLinearSystemError(rc)
        return (D, worst, rss) if tol is not None else D

    def measure_vjp(self, x: np.ndarray, records, grad_m: np.ndarray) -> np.ndarray:
        """`ezpz_system_measure_vjp`: grad_x [..., n_vars] = grad_m [..., n_meas] pulled back through `measure` at x."""
        x, lead, batch = self._measure_x(x)
        recs = stack_records(records)
        k = len(recs)
        grad_m = np.ascontiguousarray(grad_m, dtype=np.float64)
        if grad_m.shape != lead + (k,):
            raise ValueError(f"grad_m: expected {lead + (k,)}, got {grad_m.shape}")
        gx = np.zeros(x.shape)
        rc = lib().ezpz_system_measure_vjp(self._h, recs.ctypes.data if k else None, k, x.ctypes.data if x.size else None,
                                           grad_m.ctypes.data if grad_m.size else None, batch, gx.ctypes.data if gx.size else None)
        if rc != 0:
            raise NonLinearSystemError(rc)
        return gx

    def measure_device(self, x_ptr: int, records, batch: int, m_ptr: int, flags_ptr: int = 0, grad_ptr: int = 0, stream: int = 0) -> None:
        """Device pointers and a hipStream_t handle; enqueue only (a record list other than the last one is packed and uploaded
        first).  `records` stays a host array."""
        recs = stack_records(records)
        rc = lib().ezpz_system_measure_device(self._h, recs.ctypes.data if len(recs) else None, len(recs), x_ptr or None, batch,
                                              m_ptr or None, flags_ptr or None, grad_ptr or None, stream or None)
        if rc != 0:
            raise NonLinearSystemError(rc)

    def measure_response_device(self, x_ptr: int, records, S_ptr: int, n_param: int, batch: int, D_ptr: int, tol_ptr: int = 0,
                                worst_ptr: int = 0, rss_ptr: int = 0, stream: int = 0) -> None:
        """Device pointers (tol included) and a hipStream_t handle; enqueue only."""
        recs = stack_records(records)
        rc = lib().ezpz_system_measure_response_device(self._h, recs.ctypes.data if len(recs) else None, len(recs), x_ptr or None,
                                                       S_ptr or None, n_param, batch, tol_ptr or None, D_ptr or None,
                                                       worst_ptr or None, rss_ptr or None, stream or None)
        if rc != 0:
            raise NonLinearSystemError(rc)

    def measure_vjp_device(self, x_ptr: int, records, grad_m_ptr: int, batch: int, grad_x_ptr: int, stream: int = 0) -> None:
        """Device pointers and a hipStream_t handle; enqueue only."""
        recs = stack_records(records)
        rc = lib().ezpz_system_measure_vjp_device(self._h, recs.ctypes.data if len(recs) else None, len(recs), x_ptr or None,
                                                  grad_m_ptr or None, batch, grad_x_ptr or None, stream or None)
        if rc != 0:
            raise NonLinearSystemError(rc)

    # ---- Monte-Carlo tolerance analysis (ezpz_system_tolerance_mc) ---------------------------------------------------------------
    def _mc_x0(self, x0):
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1)
        if x0.size != self.n_vars:
            raise ValueError(f"x0: expected {self.n_vars} values, got {x0.size}")
        return x0

    def _mc_request(self, positions, dists, records, nominal, limits, hist, seed, chunk):
        pos = self._positions(positions)
        d = mc_dists(dists)
        if len(d) != len(pos):
            raise ValueError(f"dists: one per position ({len(pos)}), got {len(d)}")
        recs = stack_records(records)
        k = len(recs)
        if nominal is not None:
            nominal = np.ascontiguousarray(nominal, dtype=np.float64)
            if nominal.shape != (len(pos),):
                raise ValueError(f"nominal: expected shape ({len(pos)},), got {nominal.shape}")

        def pair(what, value, extra=0):
            if value is None:
                return None, None
            if len(value) != 2 + extra:
                raise ValueError(f"{what}: (lo [n_meas], hi [n_meas]{', bins' if extra else ''})")
            lo, hi = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (k,))) for v in value[:2])
            return lo, hi

        lim_lo, lim_hi = pair("limits", limits)
        hist_lo, hist_hi = pair("hist", hist, 1)
        mc = CMcConfig(seed, chunk, int(hist[2]) if hist is not None else 0)
        return pos, d, recs, nominal, lim_lo, lim_hi, hist_lo, hist_hi, mc

    def tolerance_mc(self, x0, positions, dists, records, samples: int, seed: int = 0, nominal=None, limits=None, hist=None,
                     chunk: int = 0, keep: bool = False, config: Optional[Config] = None, contributors: bool = False,
                     pivot_rel: Optional[float] = None, quantiles=None, quantile_z: float = 0.0,
                     effects: Optional["EffectsConfig"] = None, factorial: bool = False, keep_coef: bool = False,
                     sampling: str = "philox", image=None) -> "McResult":
        """`ezpz_system_tolerance_mc`: every driving dimension (`positions`, one `McDist` each) drawn `samples` times, every variant
        solved from x0 [n_vars] -- the nominal solution -- the reference dimensions `records` read off each answer, and their
        statistics reduced on the device.  nominal [n_param]: the values the deviations are added to (None: the system's own);
        limits = (lo, hi), each [n_meas] or a scalar: the yield's limits; hist = (lo, hi, bins): a histogram of `bins` <= 64 bins per
        record with an under and an over count; chunk: samples per round (0: the library's choice); keep: also every sample's
        params, m, flags and ok.  The sums' order is fixed: the same bits whatever the chunk.
        contributors: the same run through `ezpz_system_tolerance_mc_contrib` -- the result also has moments, n_complete, cov, beta,
        contrib, r2, dropped and corr (`McContributors`); pivot_rel: EzpzMcContribConfig's (None: the library's default).
        quantiles: a list of probabilities in [0, 1] -- the same run through `ezpz_system_tolerance_mc_quantiles`: every sample's m,
        flags and ok stay on the device (samples x n_meas x 9 + samples bytes) and the exact order statistics are selected there; the
        result also has `quantiles` (MC_QUANTILE_DTYPE [n_meas, n_q]) and q_value, q_lo, q_hi, q_band_lo, q_band_hi [n_meas, n_q];
        quantile_z: the band's half width in standard errors of the rank.  Not together with contributors.
        effects: an `EffectsConfig` -- the same run through `ezpz_system_tolerance_mc_effects`: every reference dimension's sums and
        counts per bin of every driving dimension, reduced on the device, and from them the main-effect curves and the first-order
        indices; the result also has `effects` (an `McEffects`, with the edges used).  Not together with contributors or quantiles.
        factorial: the same run through `ezpz_system_tolerance_mc_factorial` -- every dimension CORNER or FIXED and samples ==
        `mc_corner_count(dists)`: the corner run as a full two-level factorial design, every main effect and interaction by one
        Walsh-Hadamard transform on the device; the result also has `factorial` (an `McFactorial`); keep_coef: with all 2^kc
        coefficients per record.  Not together with contributors, quantiles or effects.
        sampling: "philox" -- the list as given -- or "sequence": every UNIFORM and NORMAL dimension of this call drawn from the
        low-discrepancy sequence (`McDist.uniform(..., sequence=True)`): for a smooth response mean, std and what is built on them
        converge nearly as 1 / samples; tail yields gain little.  At most 64 positions up to the last such dimension, 2^32 samples.
        image: a `sketch_image.ImageConfig(items, view, n_layers)` -- the same run through `ezpz_system_tolerance_mc_image`: every
        round's solved variants drawn on the device into `image` (uint32 [n_layers, height, width]; a variant that did not solve
        draws nothing), with `image_info`; no value vector leaves the device.  Not together with the other kinds."""
        if sampling != "philox":
            dists = _with_sampling(dists, sampling)
        kind = _mc_kind(contributors, quantiles, effects, factorial, image)
        x0 = self._mc_x0(x0)
        pos, d, recs, nominal, lim_lo, lim_hi, hist_lo, hist_hi, mc = self._mc_request(positions, dists, records, nominal, limits, hist,
                                                                                     seed, chunk)
        k, n_param, samples = len(recs), len(pos), int(samples)
        stats = np.zeros(k, dtype=MC_STATS_DTYPE)
        totals = np.zeros(1, dtype=MC_TOTALS_DTYPE)
        counts = np.zeros((k, mc.hist_bins + 2), dtype=np.uint64) if mc.hist_bins else None
        kept = (np.zeros((samples, n_param)), np.zeros((samples, k)), np.zeros((samples, k), np.uint8),
                np.zeros(samples, np.uint8)) if keep else (None,) * 4
        cfg = (config or Config())._c()
        kind = kind(self, pos, d, nominal, k, samples, pivot_rel=pivot_rel, quantiles=quantiles, quantile_z=quantile_z, effects=effects,
                    keep_coef=keep_coef, image=image)
        args = (self._h, _ptr(x0), _ptr(pos), n_param, _ptr(d), _ptr(nominal), _ptr(recs), k, _ptr(lim_lo), _ptr(lim_hi), _ptr(hist_lo), _ptr(hist_hi),
                samples, C.byref(mc), C.byref(cfg), stats.ctypes.data, totals.ctypes.data, _ptr(counts), *(_ptr(a) for a in kept))
        outputs = kind.outputs()
        rc = getattr(lib(), kind.entry)(*args, *(_mc_arg(a) for a in (*kind.inputs, *outputs)))
        if rc != 0:
            raise NonLinearSystemError(rc)
        return McResult(stats, totals, counts, kept if keep else None, **kind.result(stats, *outputs))

    def tolerance_mc_device(self, x0_ptr: int, positions, dists, records, samples: int, stats_ptr: int, totals_ptr: int, hist_ptr: int = 0,
                            seed: int = 0, nominal=None, limits=None, hist=None, chunk: int = 0, keep_params_ptr: int = 0,
                            keep_m_ptr: int = 0, keep_flags_ptr: int = 0, keep_ok_ptr: int = 0, stream: int = 0,
                            config: Optional[Config] = None, moments_ptr: int = 0, info_ptr: int = 0, cov_ptr: int = 0, beta_ptr: int = 0,
                            contrib_ptr: int = 0, r2_ptr: int = 0, dropped_ptr: int = 0, pivot_rel: Optional[float] = None,
                            quantiles=None, quantile_z: float = 0.0, quantiles_ptr: int = 0, effects: Optional["EffectsConfig"] = None,
                            effect_sums_ptr: int = 0, effect_counts_ptr: int = 0, cond_mean_ptr: int = 0, cond_var_ptr: int = 0,
                            eta2_ptr: int = 0, first_ptr: int = 0, bins_used_ptr: int = 0, factorial: bool = False,
                            factorial_info_ptr: int = 0, factorial_main_ptr: int = 0, factorial_pair_ptr: int = 0,
                            factorial_ss_order_ptr: int = 0, factorial_ss_total_ptr: int = 0, factorial_first_ptr: int = 0,
                            factorial_total_ptr: int = 0, factorial_coef_ptr: int = 0, image=None, image_counts_ptr: int = 0,
                            image_info_ptr: int = 0):
        """Device pointers for x0 and every output (stats: MC_STATS_DTYPE [n_meas], totals: MC_TOTALS_DTYPE [1], hist: uint64
        [n_meas, bins + 2]) and a hipStream_t handle; positions, dists, records, nominal, limits and hist = (lo, hi, bins) stay host
        values.  Enqueues only once the run's tables are the last run's.  With moments_ptr the run goes through
        `ezpz_system_tolerance_mc_contrib_device` and fills moments [K + K (K + 1) / 2], info (MC_MOMENTS_INFO_DTYPE [1]), cov [K, K],
        beta and contrib [n_meas, n_param], r2 [n_meas] and dropped (uint64 [1]) as well, K = n_param + n_meas.  With quantiles (host
        probabilities) the run goes through `ezpz_system_tolerance_mc_quantiles_device` and fills quantiles_ptr (MC_QUANTILE_DTYPE
        [n_meas, n_q]); it reads the kept rows from keep_m_ptr, keep_flags_ptr and keep_ok_ptr where given.  With effects (an
        `EffectsConfig`, host values) the run goes through `ezpz_system_tolerance_mc_effects_device` and fills effect_sums_ptr [n_param,
        bins, n_meas, 2], effect_counts_ptr (uint64 [n_param, bins, n_meas]), cond_mean_ptr and cond_var_ptr [n_param, bins, n_meas],
        eta2_ptr and first_ptr [n_meas, n_param] and bins_used_ptr (uint32 [n_meas, n_param]); the edges used [n_param, bins - 1] are
        returned (None without effects).  With factorial the run goes through `ezpz_system_tolerance_mc_factorial_device` and fills
        factorial_info_ptr (MC_FACTORIAL_DTYPE [n_meas]), factorial_main_ptr, factorial_ss_total_ptr, factorial_first_ptr and
        factorial_total_ptr [n_meas, kc], factorial_pair_ptr [n_meas, kc, kc], factorial_ss_order_ptr [n_meas, kc + 1] and, where
        given, factorial_coef_ptr [n_meas, 2^kc]; it reads the kept rows from keep_m_ptr, keep_flags_ptr and keep_ok_ptr where given.
        With image (a `sketch_image.ImageConfig`, host values, n_layers given) the run goes through
        `ezpz_system_tolerance_mc_image_device` and fills image_counts_ptr (uint32 [n_layers, height, width]) and image_info_ptr
        (IMAGE_INFO_DTYPE [1])."""
        given = locals()  # (the keywords by name: a kind names the ones that hold its outputs)
        kind = _mc_kind(bool(moments_ptr), quantiles, effects, factorial, image)
        pos, d, recs, nominal, lim_lo, lim_hi, hist_lo, hist_hi, mc = self._mc_request(positions, dists, records, nominal, limits, hist,
                                                                                     seed, chunk)
        cfg = (config or Config())._c()
        kind = kind(self, pos, d, nominal, len(recs), int(samples), pivot_rel=pivot_rel, quantiles=quantiles, quantile_z=quantile_z,
                    effects=effects, image=image)
        args = (self._h, x0_ptr or None, _ptr(pos), len(pos), _ptr(d), _ptr(nominal), _ptr(recs), len(recs), _ptr(lim_lo), _ptr(lim_hi), _ptr(hist_lo),
                _ptr(hist_hi), int(samples), C.byref(mc), C.byref(cfg), stats_ptr or None, totals_ptr or None, hist_ptr or None,
                keep_params_ptr or None, keep_m_ptr or None, keep_flags_ptr or None, keep_ok_ptr or None)
        rc = getattr(lib(), kind.entry + "_device")(*args, *(_mc_arg(a) for a in kind.inputs), *(given[name] or None for name in kind.device_outputs),
                                                    stream or None)
        if rc != 0:
            raise NonLinearSystemError(rc)
        return kind.device_returns

    # ---- Sobol tolerance indices (ezpz_system_tolerance_sobol) ------------------------------------------------------------------------
    def tolerance_sobol(self, x0, positions, dists, records, samples: int, seed: int = 0, seed_b: Optional[int] = None, chunk: int = 0,
                        keep: bool = False, nominal=None, config: Optional[Config] = None) -> "SobolResult":
        """`ezpz_system_tolerance_sobol`: first-order and total-effect Sobol indices of every reference dimension (`records`) for
        every driving dimension (`positions`, one `McDist` each; no CORNER ones) by pick-freeze sampling: (k' + 2) x samples
        driven solves from x0 -- the nominal solution -- for k' dimensions that are not FIXED, reduced on the device.  seed: matrix
        A's (the draws of `tolerance_mc` with this seed); seed_b: matrix B's (None: seed ^ 0x9E3779B97F4A7C15); chunk: samples per
        round (0: the library's choice); keep: also every row's f [samples, k + 2, n_meas], flags and ok [samples, k + 2]."""
        x0 = self._mc_x0(x0)
        pos, d, recs, nominal, _, _, _, _, mc = self._mc_request(positions, dists, records, nominal, None, None, seed, chunk)
        m, k, samples = len(recs), len(pos), int(samples)
        sc = _sobol_config(seed, seed_b)
        stats, totals = np.zeros(m, dtype=MC_STATS_DTYPE), np.zeros(1, dtype=MC_TOTALS_DTYPE)
        sums, n_complete, out = _sobol_outputs(k, m)
        kept = (np.zeros((samples, k + 2, m)), np.zeros((samples, k + 2, m), np.uint8), np.zeros((samples, k + 2), np.uint8)) if keep else (None,) * 3
        cfg = (config or Config())._c()
        rc = lib().ezpz_system_tolerance_sobol(self._h, _ptr(x0), _ptr(pos), k, _ptr(d), _ptr(nominal), _ptr(recs), m, samples, C.byref(mc), C.byref(cfg),
                                               C.byref(sc), _ptr(stats), totals.ctypes.data, _ptr(sums), _ptr(n_complete), *(_ptr(a) for a in out),
                                               *(_ptr(a) for a in kept))
        if rc != 0:
            raise NonLinearSystemError(rc)
        return SobolResult(stats, totals, sums, n_complete, *out, kept if keep else None, sc.seed_b)

    def tolerance_sobol_device(self, x0_ptr: int, positions, dists, records, samples: int, stats_ptr: int, totals_ptr: int, sums_ptr: int,
                               n_complete_ptr: int, var_ptr: int, first_ptr: int, total_ptr: int, first_var_ptr: int, total_var_ptr: int,
                               seed: int = 0, seed_b: Optional[int] = None, chunk: int = 0, keep_f_ptr: int = 0, keep_flags_ptr: int = 0,
                               keep_ok_ptr: int = 0, stream: int = 0, nominal=None, config: Optional[Config] = None) -> None:
        """Device pointers for x0 and every output (stats: MC_STATS_DTYPE [n_meas], totals: MC_TOTALS_DTYPE [1], sums [n_meas, 4 + 4
        n_param], n_complete uint64 [n_meas], var [n_meas], first, total, first_var, total_var [n_meas, n_param]) and a hipStream_t
        handle; positions, dists, records and nominal stay host values.  Enqueues only once the run's tables are the last run's."""
        pos, d, recs, nominal, _, _, _, _, mc = self._mc_request(positions, dists, records, nominal, None, None, seed, chunk)
        sc = _sobol_config(seed, seed_b)
        cfg = (config or Config())._c()
        rc = lib().ezpz_system_tolerance_sobol_device(self._h, x0_ptr or None, _ptr(pos), len(pos), _ptr(d), _ptr(nominal), _ptr(recs), len(recs),
                                                      int(samples), C.byref(mc), C.byref(cfg), C.byref(sc), stats_ptr or None, totals_ptr or None,
                                                      sums_ptr or None, n_complete_ptr or None, var_ptr or None, first_ptr or None,
                                                      total_ptr or None, first_var_ptr or None, total_var_ptr or None, keep_f_ptr or None,
                                                      keep_flags_ptr or None, keep_ok_ptr or None, stream or None)
        if rc != 0:
            raise NonLinearSystemError(rc)

    # ---- solution branches (ezpz_system_solve_branches) --------------------------------------------------------------------------
    def _branch_request(self, dists, compare, seed, branch):
        d = mc_dists(dists)
        if len(d) != self.n_vars:
            raise ValueError(f"dists: one per variable ({self.n_vars}), got {len(d)}")
        return d, _compare_mask(compare, self.n_vars), (branch or BranchConfig())._c(seed)

    def solve_branches(self, x0, dists, samples: int, seed: int = 0, compare=None, config: Optional[Config] = None,
                       branch: Optional["BranchConfig"] = None, keep: bool = False) -> "BranchResult":
        """`ezpz_system_solve_branches`: every base x0[b] ([n_vars] or [batch, n_vars]) gets `samples` starts -- sample 0 the base
        itself, the others drawn around it by dists (one `McDist` per variable; `mc_sample(seed, dists, x0[b], first, count)` gives
        the same starts) -- every start is solved, and the answers are clustered on the device by the sequential leader rule.
        compare: a mask [n_vars] of the compared variables (non-zero: compared), None for all; branch: eps, max_branches and
        chunk; keep: also every sample's label.  The same bytes whatever the chunk."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1, max(self.n_vars, 1))
        d, mask, bc = self._branch_request(dists, compare, seed, branch)
        batch, samples = x0.shape[0], int(samples)
        info, branches, x, labels = _branch_outputs(batch, samples, self.n_vars, bc.max_branches, keep)
        cfg = (config or Config())._c()
        rc = lib().ezpz_system_solve_branches(self._h, _ptr(x0), _ptr(d), _ptr(mask), batch, samples, C.byref(bc), C.byref(cfg), _ptr(info),
                                              _ptr(branches), _ptr(x), _ptr(labels))
        if rc != 0:
            raise NonLinearSystemError(rc)
        return BranchResult(info, branches, x, labels)

    def solve_branches_device(self, x0_ptr: int, dists, batch: int, samples: int, info_ptr: int, branches_ptr: int, x_branch_ptr: int,
                              keep_label_ptr: int = 0, seed: int = 0, compare=None, config: Optional[Config] = None,
                              branch: Optional["BranchConfig"] = None, stream: int = 0) -> None:
        """Device pointers for x0 [batch, n_vars] and every output (info: BRANCH_INFO_DTYPE [batch], branches: BRANCH_DTYPE
        [batch, max_branches], x_branch: float64 [batch, max_branches, n_vars], keep_label: int32 [batch, samples]) and a hipStream_t
        handle; dists, compare and the configs stay host values.  Enqueues only once the run's tables are the last run's."""
        d, mask, bc = self._branch_request(dists, compare, seed, branch)
        cfg = (config or Config())._c()
        rc = lib().ezpz_system_solve_branches_device(self._h, x0_ptr or None, _ptr(d), _ptr(mask), int(batch), int(samples), C.byref(bc),
                                                     C.byref(cfg), info_ptr or None, branches_ptr or None, x_branch_ptr or None,
                                                     keep_label_ptr or None, stream or None)
        if rc != 0:
            raise NonLinearSystemError(rc)

    # ---- dimension targets (ezpz_system_seek_targets) ---------------------------------------------------------------------------
    def seek_targets(self, x0, positions, params0, records, targets, config: Optional["SeekConfig"] = None,
                     want_trace: bool = False) -> "SeekResult":
        """`ezpz_system_seek_targets`: which values of the driving dimensions (`positions`) put the reference dimensions `records`
        on `targets` [batch, n_meas]?  x0 [batch, n_vars] are the starts (normally the current solution), params0 [batch, n_param]
        the dimensions' current values.  A projected Levenberg-Marquardt iteration per system, its rounds on the device; a seek
        never leaves its last accepted, assembled answer.  Returns a `SeekResult`."""
        pos = self._positions(positions)
        recs = stack_records(records)
        k, n_param = len(recs), len(pos)
        targets = np.ascontiguousarray(targets, dtype=np.float64)
        if targets.ndim != 2 or targets.shape[1] != k:
            raise ValueError(f"targets: expected [batch, {k}], got {targets.shape}")
        batch = targets.shape[0]
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        params0 = np.ascontiguousarray(params0, dtype=np.float64)
        if x0.shape != (batch, self.n_vars) or params0.shape != (batch, n_param):
            raise ValueError(f"x0, params0: expected ({batch}, {self.n_vars}) and ({batch}, {n_param}), got {x0.shape} and {params0.shape}")
        c, keep = (config or SeekConfig())._c(n_param, k)
        params, x, m = np.zeros((batch, n_param)), np.zeros((batch, self.n_vars)), np.zeros((batch, k))
        info = np.zeros(batch, dtype=SEEK_INFO_DTYPE)
        trace = np.zeros((batch, c.max_iterations + 1)) if want_trace else None
        rc = lib().ezpz_system_seek_targets(self._h, _ptr(x0), _ptr(pos), n_param, _ptr(params0), _ptr(recs), k, _ptr(targets), batch,
                                            C.byref(c), _ptr(params), _ptr(x), _ptr(m), _ptr(info), _ptr(trace))
        del keep
        if rc != 0:
            raise NonLinearSystemError(rc)
        return SeekResult(params, x, m, info, trace)

    def seek_targets_device(self, x0_ptr: int, positions, params0_ptr: int, records, targets_ptr: int, batch: int, params_ptr: int,
                            x_ptr: int, m_ptr: int, info_ptr: int, trace_ptr: int = 0, config: Optional["SeekConfig"] = None,
                            stream: int = 0) -> None:
        """Device pointers for x0, params0, targets and every output (info: SEEK_INFO_DTYPE [batch], trace: [batch, 1 +
        max_iterations]) and a hipStream_t handle; positions, records and the configuration stay host values.  Enqueues 1 +
        max_iterations rounds per chunk, with no host read-back between them."""
        pos = self._positions(positions)
        recs = stack_records(records)
        c, keep = (config or SeekConfig())._c(len(pos), len(recs))
        rc = lib().ezpz_system_seek_targets_device(self._h, x0_ptr or None, pos.ctypes.data if len(pos) else None, len(pos),
                                                   params0_ptr or None, recs.ctypes.data if len(recs) else None, len(recs),
                                                   targets_ptr or None, int(batch), C.byref(c), params_ptr or None, x_ptr or None,
                                                   m_ptr or None, info_ptr or None, trace_ptr or None, stream or None)
        del keep
        if rc != 0:
            raise NonLinearSystemError(rc)


@dataclass
class SeekConfig:
    """EzpzSeekConfig, the policy of a seek: weight, tol [n_meas] and lo, hi, scale [n_param] (a scalar is every entry's value;
    None: the library's default -- 1, 1e-6, -inf, +inf, 1), the damping's schedule, the step's end test, the lambda of the
    sensitivities (None: the inner config's initial_lambda), the inner solves' Config and the systems per pass (0: the library's
    choice).  Policy defaults (ezpz_default_seek_config), not measurements."""

    weight: object = None
    tol: object = None
    lo: object = None
    hi: object = None
    scale: object = None
    max_iterations: int = 40
    mu0: float = 1e-3
    mu_up: float = 10.0
    mu_down: float = 0.1
    mu_min: float = 1e-12
    mu_max: float = 1e12
    step_tol: float = 1e-12
    sens_lambda: Optional[float] = None
    inner: Optional[Config] = None
    chunk: int = 0

    def _c(self, n_param: int, n_meas: int):
        """(the C record, the arrays it points into: keep them alive for the call)."""
        keep = []

        def table(what, value, n):
            if value is None:
                return None
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(value, dtype=np.float64), (n,)))
            keep.append(a)
            return a.ctypes.data if n else None

        inner = self.inner or Config()
        lam = inner.initial_lambda if self.sens_lambda is None else float(self.sens_lambda)
        c = CSeekConfig(table("weight", self.weight, n_meas), table("tol", self.tol, n_meas), table("lo", self.lo, n_param),
                        table("hi", self.hi, n_param), table("scale", self.scale, n_param), int(self.max_iterations), int(self.chunk),
                        float(self.mu0), float(self.mu_up), float(self.mu_down), float(self.mu_min), float(self.mu_max),
                        float(self.step_tol), lam, inner._c())
        return c, keep


class SeekResult:
    """What `System.seek_targets` returns: params [batch, n_param], x [batch, n_vars] and m [batch, n_meas] of every system's
    last accepted answer, info (SEEK_INFO_DTYPE [batch]: status, iterations, accepted, rejected, cost0, cost, worst, mu) with its
    fields as attributes, status_names, and cost_trace [batch, 1 + max_iterations] (None unless asked for)."""

    def __init__(self, params, x, m, info, cost_trace):
        self.params, self.x, self.m, self.info, self.cost_trace = params, x, m, info, cost_trace
        for f in SEEK_INFO_DTYPE.names:
            setattr(self, f, info[f])

    @property
    def status_names(self):
        return [SEEK_STATUS[s] if s < len(SEEK_STATUS) else str(s) for s in self.info["status"]]


def seek_step(p, m, D, targets, mu: float, config: Optional[SeekConfig] = None):
    """`ezpz_seek_step`: one step of the seek's iteration from (p [n_param], m [n_meas], D [n_meas, n_param]) towards targets
    [n_meas] with the damping mu -- (kind, p_trial, delta, held) with kind one of "TRIAL", "MINIMUM", "PIVOT" and held a bit per
    dimension.  Host only."""
    p, m, targets = (np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (p, m, targets))
    D = np.ascontiguousarray(D, dtype=np.float64)
    if D.shape != (len(m), len(p)) or len(targets) != len(m):
        raise ValueError(f"D, targets: expected ({len(m)}, {len(p)}) and ({len(m)},), got {D.shape} and {targets.shape}")
    c, keep = (config or SeekConfig())._c(len(p), len(m))
    p_trial, delta, held = np.zeros(len(p)), np.zeros(len(p)), C.c_uint32(0)
    rc = lib().ezpz_seek_step(len(p), len(m), _ptr(p), _ptr(m), _ptr(D), _ptr(targets), C.byref(c), float(mu), _ptr(p_trial), _ptr(delta),
                              C.byref(held))
    del keep
    if rc < 0:
        raise NonLinearSystemError(rc)
    return SEEK_STEP[rc], p_trial, delta, held.value


class McDist:
    """A driving dimension's tolerance distribution (EzpzMcDist): the deviation added to its nominal value."""
    FIXED, UNIFORM, NORMAL, CORNER = range(4)

    def __init__(self, kind: int, a: float = 0.0, b: float = 0.0, sequence: bool = False):
        self.kind, self.a, self.b, self.sequence = int(kind), float(a), float(b), bool(sequence)

    def __repr__(self):
        return "McDist.%s(%r, %r%s)" % (("fixed", "uniform", "normal", "corner")[self.kind] if 0 <= self.kind < 4 else self.kind, self.a, self.b,
                                        ", sequence=True" if self.sequence else "")

    @staticmethod
    def fixed() -> "McDist":
        return McDist(McDist.FIXED)

    @staticmethod
    def uniform(lo: float, hi: float, sequence: bool = False) -> "McDist":
        """A deviation uniform in [lo, hi).  sequence: a low-discrepancy draw (EZPZ_MC_SEQUENCE) -- a Sobol' point with a seed-keyed
        shift in place of the pseudo-random words; at most the first 64 positions of a list, at most 2^32 samples."""
        return McDist(McDist.UNIFORM, lo, hi, sequence)

    @staticmethod
    def normal(sigma: float, trunc: float = 0.0, sequence: bool = False) -> "McDist":
        """A normal deviation of standard deviation sigma, truncated at +-trunc sigmas (0: not truncated, else >= 1).  sequence: as
        for `uniform`, through the inverse of the normal distribution; untruncated it reaches about +-6.34 sigma."""
        return McDist(McDist.NORMAL, sigma, trunc, sequence)

    @staticmethod
    def corner(lo: float, hi: float) -> "McDist":
        """The deviation lo or hi by a bit of the sample index: k such dimensions make samples 0 .. 2^k - 1 the 2^k corners."""
        return McDist(McDist.CORNER, lo, hi)


def mc_dists(dists) -> np.ndarray:
    """A sequence of McDist (or an MC_DIST_DTYPE array) as the array the library reads."""
    if isinstance(dists, np.ndarray) and dists.dtype == MC_DIST_DTYPE:
        return np.ascontiguousarray(dists)
    out = np.zeros(len(dists), dtype=MC_DIST_DTYPE)
    for j, d in enumerate(dists):
        out[j] = (d.kind, MC_SEQUENCE if getattr(d, "sequence", False) else 0, d.a, d.b)
    return out


def _with_sampling(dists, sampling: str) -> np.ndarray:
    """The list as the library reads it, for `System.tolerance_mc`'s sampling: "sequence" flags every UNIFORM and NORMAL dimension."""
    if sampling not in ("philox", "sequence"):
        raise ValueError(f"sampling: 'philox' or 'sequence', got {sampling!r}")
    d = mc_dists(dists)
    if sampling == "sequence":
        d = d.copy()
        d["reserved"][(d["kind"] == McDist.UNIFORM) | (d["kind"] == McDist.NORMAL)] |= MC_SEQUENCE
    return d


def mc_sample(seed: int, dists, nominal, first: int, count: int) -> np.ndarray:
    """`ezpz_mc_sample`: params [count, n_param] of the samples first .. first + count - 1 -- what a tolerance_mc run of that
    seed draws for them.  Host only."""
    d = mc_dists(dists)
    nominal = np.ascontiguousarray(nominal, dtype=np.float64)
    if nominal.shape != (len(d),):
        raise ValueError(f"nominal: expected shape ({len(d)},), got {nominal.shape}")
    out = np.zeros((int(count), len(d)))
    rc = lib().ezpz_mc_sample(int(seed), d.ctypes.data if len(d) else None, nominal.ctypes.data if len(d) else None, len(d), int(first),
                              int(count), out.ctypes.data if out.size else None)
    if rc != 0:
        raise NonLinearSystemError(rc)
    return out


def _mc_kind(contributors, quantiles, effects, factorial, image=None):
    """The class of the one kind of a `tolerance_mc` run: the kinds exclude one another."""
    if image is not None:
        if contributors or quantiles is not None or effects is not None or factorial:
            raise ValueError("image together with contributors, quantiles, effects or factorial: run them one after the other")
        return _McImageKind
    if quantiles is not None and contributors:
        raise ValueError("quantiles together with contributors: run them one after the other")
    if effects is not None and (contributors or quantiles is not None):
        raise ValueError("effects together with contributors or quantiles: run them one after the other")
    if factorial and (contributors or quantiles is not None or effects is not None):
        raise ValueError("factorial together with contributors, quantiles or effects: run them one after the other")
    return (_McQuantiles if quantiles is not None else _McEffectsKind if effects is not None else _McFactorialKind if factorial
            else _McContrib if contributors else _McPlain)


class _McPlain:
    """A kind of `tolerance_mc` run, made from the checked request and the caller's settings.  entry: the host entry's name (the
    device form's has "_device" behind it); inputs: the entry's arguments between the common ones and its outputs; device_outputs:
    the keywords of `tolerance_mc_device` that hold its outputs, in the entry's order, and device_returns: what that form returns;
    outputs(): the host form's output arrays, in the same order; result(stats, *outputs): what they add to `McResult`'s keywords."""
    entry, inputs, device_outputs, device_returns = "ezpz_system_tolerance_mc", (), (), None

    def __init__(self, system, pos, d, nominal, n_meas, samples, **settings):
        self.n_param, self.n_meas, self.samples = len(pos), n_meas, samples

    def outputs(self):
        return ()

    def result(self, stats):
        return {}


class _McContrib(_McPlain):
    entry = "ezpz_system_tolerance_mc_contrib"
    device_outputs = ("moments_ptr", "info_ptr", "cov_ptr", "beta_ptr", "contrib_ptr", "r2_ptr", "dropped_ptr")

    def __init__(self, *request, pivot_rel, **settings):
        super().__init__(*request)
        self.inputs = (C.byref(_contrib_config(pivot_rel)),)

    def outputs(self):
        moments, info, out = _contrib_outputs(self.n_param, self.n_meas)
        return (moments, info, *out)

    def result(self, stats, moments, info, *out):
        n_complete = int(info["n_complete"][0]) if self.samples else 0
        return dict(contributors=McContributors(moments, n_complete, self.n_param, self.n_meas, *out))


class _McQuantiles(_McPlain):
    entry, device_outputs = "ezpz_system_tolerance_mc_quantiles", ("quantiles_ptr",)

    def __init__(self, *request, quantiles, quantile_z, **settings):
        super().__init__(*request)
        probs = np.ascontiguousarray(quantiles, dtype=np.float64).reshape(-1)
        self.inputs = (probs, len(probs), C.byref(CMcQuantileConfig(float(quantile_z), 0)))

    def outputs(self):
        return (np.zeros((self.n_meas, self.inputs[1]), dtype=MC_QUANTILE_DTYPE),)

    def result(self, stats, out):
        return dict(quantiles=out)


class _McEffectsKind(_McPlain):
    entry = "ezpz_system_tolerance_mc_effects"
    device_outputs = ("effect_sums_ptr", "effect_counts_ptr", "cond_mean_ptr", "cond_var_ptr", "eta2_ptr", "first_ptr", "bins_used_ptr")

    def __init__(self, system, pos, d, nominal, *request, effects, **settings):
        super().__init__(system, pos, d, nominal, *request)
        self.ec, self.edges, self.bounds = _effects_request(effects, d, pos, nominal, system)
        self.inputs, self.device_returns = (C.byref(self.ec), self.edges), self.edges  # (the device form returns the edges used)

    def outputs(self):
        sums, cnt, out = _effect_outputs(self.n_param, self.n_meas, self.ec.bins)
        return (sums, cnt, *out)

    def result(self, stats, sums, cnt, *out):
        return dict(effects=McEffects(sums, cnt, stats["nominal"].copy(), self.edges, *out, bounds=self.bounds))


class _McFactorialKind(_McPlain):
    entry = "ezpz_system_tolerance_mc_factorial"
    device_outputs = tuple("factorial_%s_ptr" % name for name in ("info", "main", "pair", "ss_order", "ss_total", "first", "total", "coef"))

    def __init__(self, system, pos, d, *request, keep_coef=False, **settings):
        super().__init__(system, pos, d, *request)
        self.dims, self.keep_coef = _corner_dims(d), keep_coef

    def outputs(self):
        return _factorial_outputs(len(self.dims), self.n_meas, self.keep_coef)

    def result(self, stats, *out):
        return dict(factorial=McFactorial(*out, dims=self.dims, stats=stats))


class _McImageKind(_McPlain):
    entry, device_outputs = "ezpz_system_tolerance_mc_image", ("image_counts_ptr", "image_info_ptr")

    def __init__(self, *request, image, **settings):
        from .sketch_image import ImageInfo, _layers_of, _view, pack_items  # (the package's `sketch_image` is the function)

        super().__init__(*request)
        self.items, self.view = pack_items(image.items), _view(image.view)
        self.n_layers = _layers_of(self.items, image.n_layers)
        self.info_type = ImageInfo
        self.inputs = (self.items, len(self.items), C.byref(self.view), self.n_layers)

    def outputs(self):
        if not (1 <= self.view.width <= 16384 and 1 <= self.view.height <= 16384 and 1 <= self.n_layers <= 8):
            raise NonLinearSystemError(-103)
        return (np.zeros((self.n_layers, self.view.height, self.view.width), np.uint32), np.zeros(1, dtype=IMAGE_INFO_DTYPE))

    def result(self, stats, counts, info):
        return dict(image=counts, image_info=self.info_type(*(int(v) for v in info[0])))


def _mc_arg(a):
    return _ptr(a) if a is None or isinstance(a, np.ndarray) else a


class McResult:
    """What `System.tolerance_mc` returns: numpy fields per measurement record -- n_valid, mean, std, var, min, max, argmin, argmax,
    n_in, nominal, sum_d, sum_d2 -- hist [n_meas, bins + 2] (under, the bins, over; None without a histogram), the totals samples,
    n_ok and n_all_in, and with keep the samples: params, m, flags, ok.  `stats` and `totals` are the library's records.  A run with
    contributors also has moments, n_complete, cov, beta, contrib, r2, dropped (those of its `contributors`, a `McContributors`) and
    `corr`.  A run with quantiles also has `quantiles` (MC_QUANTILE_DTYPE [n_meas, n_q]) and its fields as q_value, q_lo, q_hi,
    q_band_lo, q_band_hi.  A run with effects also has `effects` (an `McEffects`), a run with factorial effects `factorial` (an
    `McFactorial`), a run with an image `image` (uint32 [n_layers, height, width]) and `image_info`."""

    def __init__(self, stats, totals, hist, kept, contributors=None, quantiles=None, effects=None, factorial=None, image=None,
                 image_info=None):
        self.stats, self.totals, self.hist = stats, totals, hist
        if image is not None:
            self.image, self.image_info = image, image_info
        if effects is not None:
            self.effects = effects
        if factorial is not None:
            self.factorial = factorial
        if quantiles is not None:
            self.quantiles = quantiles
            for f in ("value", "lo", "hi", "band_lo", "band_hi"):
                setattr(self, "q_" + f, quantiles[f])
        if contributors is not None:
            self.contributors = contributors
            for f in ("moments", "n_complete", "cov", "beta", "contrib", "r2", "dropped"):
                setattr(self, f, getattr(contributors, f))
        for f in MC_STATS_DTYPE.names:
            setattr(self, f, stats[f])
        self.std = np.sqrt(stats["var"])
        self.samples, self.n_ok, self.n_all_in = (int(totals[f][0]) for f in MC_TOTALS_DTYPE.names)
        if kept is not None:
            self.params, self.m, self.flags, self.ok = kept

    @property
    def corr(self) -> np.ndarray:
        """cov / sqrt(outer(diag)) of a run with contributors."""
        return self.contributors.corr


class McContributors:
    """What `mc_contributors` returns and a `tolerance_mc` run with contributors carries: moments and n_complete as given, cov
    [K, K] over (driving | reference) dimensions, beta and contrib [n_meas, n_param], r2 [n_meas], dropped (the library's bit mask)
    with dropped_mask [n_param], and corr."""

    def __init__(self, moments, n_complete, n_param, n_meas, cov, beta, contrib, r2, dropped):
        self.moments, self.n_complete, self.n_param, self.n_meas = moments, int(n_complete), n_param, n_meas
        self.cov, self.beta, self.contrib, self.r2 = cov, beta, contrib, r2
        self.dropped = int(dropped[0])
        self.dropped_mask = np.array([(self.dropped >> j) & 1 for j in range(n_param)], dtype=bool)

    @property
    def corr(self) -> np.ndarray:
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.cov / np.sqrt(np.outer(np.diag(self.cov), np.diag(self.cov)))


def _sobol_config(seed, seed_b) -> CSobolConfig:
    """seed_b None: matrix B's seed follows from matrix A's."""
    return CSobolConfig((int(seed) ^ SOBOL_SEED_B if seed_b is None else int(seed_b)) & 0xFFFFFFFFFFFFFFFF, 0)


def _contrib_config(pivot_rel) -> CMcContribConfig:
    cc = CMcContribConfig()
    lib().ezpz_default_mc_contrib_config(C.byref(cc))
    if pivot_rel is not None:
        cc.pivot_rel = float(pivot_rel)
    return cc


def _contrib_outputs(n_param: int, n_meas: int):
    K = n_param + n_meas
    return (np.zeros(K + K * (K + 1) // 2), np.zeros(1, dtype=MC_MOMENTS_INFO_DTYPE),
            (np.zeros((K, K)), np.zeros((n_meas, n_param)), np.zeros((n_meas, n_param)), np.zeros(n_meas), np.zeros(1, np.uint64)))


def mc_moments(params, m, flags, ok, nominal_p, nominal_m, chunk: int = 0):
    """`ezpz_mc_moments`: (moments [K + K (K + 1) / 2], n_complete) of the samples params [samples, n_param], m [samples, n_meas],
    flags [samples, n_meas] (None: clear) and ok [samples] (None: every one set) about nominal_p and nominal_m -- the reduction
    alone, on the device, no system involved; useful on the kept samples of any run."""
    params, m = np.ascontiguousarray(params, dtype=np.float64), np.ascontiguousarray(m, dtype=np.float64)
    if params.ndim != 2 or m.ndim != 2 or len(params) != len(m):
        raise ValueError(f"params [samples, n_param] and m [samples, n_meas]: got {params.shape} and {m.shape}")
    samples, n_param, n_meas = len(params), params.shape[1], m.shape[1]
    if flags is not None:
        flags = np.ascontiguousarray(flags, dtype=np.uint8).reshape(samples, n_meas)
    if ok is not None:
        ok = np.ascontiguousarray(np.asarray(ok).reshape(samples) != 0, dtype=np.uint8)
    nominal_p, nominal_m = np.ascontiguousarray(nominal_p, dtype=np.float64), np.ascontiguousarray(nominal_m, dtype=np.float64)
    if nominal_p.shape != (n_param,) or nominal_m.shape != (n_meas,):
        raise ValueError(f"nominal_p ({n_param},) and nominal_m ({n_meas},): got {nominal_p.shape} and {nominal_m.shape}")
    moments, info, _ = _contrib_outputs(n_param, n_meas)
    rc = lib().ezpz_mc_moments(_ptr(params), _ptr(m), _ptr(flags), _ptr(ok), _ptr(nominal_p), _ptr(nominal_m), samples, n_param, n_meas, int(chunk),
                               _ptr(moments), info.ctypes.data)
    if rc != 0:
        raise NonLinearSystemError(rc)
    return moments, int(info["n_complete"][0])


def mc_contributors(moments, n_complete: int, n_param: int, n_meas: int, pivot_rel: Optional[float] = None) -> McContributors:
    """`ezpz_mc_contributors`: the closing step on moments [K + K (K + 1) / 2] of n_complete samples.  Host only."""
    n_param, n_meas = int(n_param), int(n_meas)
    K = n_param + n_meas
    moments = np.ascontiguousarray(moments, dtype=np.float64)
    if not 1 <= K <= MC_MOMENT_MAX or moments.shape != (K + K * (K + 1) // 2,):
        raise ValueError(f"moments: expected K + K (K + 1) / 2 values with 1 <= K = {K} <= {MC_MOMENT_MAX}, got {moments.shape}")
    cc = _contrib_config(pivot_rel)
    _, _, out = _contrib_outputs(n_param, n_meas)
    rc = lib().ezpz_mc_contributors(moments.ctypes.data, int(n_complete), n_param, n_meas, C.byref(cc), *(_ptr(a) for a in out))
    if rc != 0:
        raise NonLinearSystemError(rc)
    return McContributors(moments, n_complete, n_param, n_meas, *out)


def mc_quantiles(m, flags, ok, probs, z: float = 0.0) -> np.ndarray:
    """`ezpz_mc_quantiles`: MC_QUANTILE_DTYPE [n_meas, n_q], the exact order statistics of the kept rows m [samples, n_meas], flags
    (the same shape; None: clear) and ok [samples] (None: every one set) at the probabilities `probs`, with the distribution-free
    band of z standard errors of the rank.  Computed on the host; the device form gives the same bytes."""
    m = np.ascontiguousarray(m, dtype=np.float64)
    if m.ndim != 2:
        raise ValueError(f"m [samples, n_meas]: got {m.shape}")
    samples, n_meas = m.shape
    if flags is not None:
        flags = np.ascontiguousarray(flags, dtype=np.uint8).reshape(m.shape)
    if ok is not None:
        ok = np.ascontiguousarray(np.asarray(ok).reshape(samples) != 0, dtype=np.uint8)
    probs = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    out = np.zeros((min(n_meas, MC_QUANTILE_MAX_MEAS), min(len(probs), MC_QUANTILE_MAX_PROBS)), dtype=MC_QUANTILE_DTYPE)
    qc = CMcQuantileConfig(float(z), 0)
    rc = lib().ezpz_mc_quantiles(_ptr(m), _ptr(flags), _ptr(ok), samples, n_meas, _ptr(probs), len(probs), C.byref(qc), _ptr(out))
    if rc != 0:
        raise NonLinearSystemError(rc)
    return out


def _corner_dims(d) -> List[int]:
    """The places, in the list, of the CORNER dimensions: rank c is dims[c]."""
    return [j for j in range(len(d)) if int(d["kind"][j]) == McDist.CORNER]


def mc_corner_count(dists) -> int:
    """2^kc for the kc CORNER dimensions of `dists`: the `samples` of a run with factorial effects."""
    return 1 << len(_corner_dims(mc_dists(dists)))


def _factorial_outputs(kc: int, n_meas: int, keep_coef: bool):
    """info, main, pair, ss_order, ss_total, first, total, coef (None unless kept), in the library's order."""
    return (np.zeros(n_meas, dtype=MC_FACTORIAL_DTYPE), np.zeros((n_meas, kc)), np.zeros((n_meas, kc, kc)), np.zeros((n_meas, kc + 1)),
            np.zeros((n_meas, kc)), np.zeros((n_meas, kc)), np.zeros((n_meas, kc)), np.zeros((n_meas, 1 << kc)) if keep_coef else None)


class McFactorial:
    """What `mc_factorial` returns and a `tolerance_mc` run with factorial effects carries, per reference dimension i: info
    (MC_FACTORIAL_DTYPE [n_meas]) and its fields n_valid, complete, corner_hi, corner_lo, mean_dev, var, m_hi, m_lo; main [n_meas, kc],
    pair [n_meas, kc, kc], ss_order [n_meas, kc + 1], ss_total, first and total [n_meas, kc]; coef [n_meas, 2^kc] or None.  dims [kc]:
    the place of the CORNER dimension of rank c in the run's list.  main_effect = 2 main (the classical main effect: the mean at the b
    end minus the mean at the a end); interaction = total - first (the share of the variance a dimension causes through interactions
    alone).  Every floating value of a record that is not complete is NaN."""

    def __init__(self, info, main, pair, ss_order, ss_total, first, total, coef=None, dims=None, stats=None):
        self.info, self.main, self.pair, self.ss_order, self.ss_total, self.first, self.total, self.coef = info, main, pair, ss_order, ss_total, first, total, coef
        self.kc = main.shape[1]
        self.dims = list(range(self.kc)) if dims is None else list(dims)
        self.stats = stats
        for f in ("n_valid", "complete", "corner_hi", "corner_lo", "mean_dev", "var", "m_hi", "m_lo"):
            setattr(self, f, info[f])
        self.main_effect = 2.0 * main
        self.interaction = total - first

    def largest(self, i: int, n: int = 5):
        """The n largest |coef| of record i among the mains and the pairs: a list of (coef, dimensions), dimensions a tuple of one or two
        places in the run's list, largest first (ties: mains before pairs, then ascending rank)."""
        terms = [(float(self.main[i, c]), (self.dims[c],)) for c in range(self.kc)]
        terms += [(float(self.pair[i, c, e]), (self.dims[c], self.dims[e])) for c in range(self.kc) for e in range(c + 1, self.kc)]
        order = sorted(range(len(terms)), key=lambda t: -abs(terms[t][0]) if terms[t][0] == terms[t][0] else math.inf)
        return [terms[t] for t in order[:int(n)]]

    def worst_case(self, i: int) -> dict:
        """The extremes of record i over the corners against the corners the linear signs predict: max, argmax, m_hi, corner_hi and
        hi_is_linear (argmax == corner_hi), and min, argmin, m_lo, corner_lo and lo_is_linear.  Needs the run's statistics."""
        if self.stats is None:
            raise ValueError("worst_case: the statistics of a run (tolerance_mc(..., factorial=True))")
        s = self.stats
        return dict(max=float(s["max"][i]), argmax=int(s["argmax"][i]), m_hi=float(self.m_hi[i]), corner_hi=int(self.corner_hi[i]),
                    hi_is_linear=bool(self.complete[i]) and int(s["argmax"][i]) == int(self.corner_hi[i]),
                    min=float(s["min"][i]), argmin=int(s["argmin"][i]), m_lo=float(self.m_lo[i]), corner_lo=int(self.corner_lo[i]),
                    lo_is_linear=bool(self.complete[i]) and int(s["argmin"][i]) == int(self.corner_lo[i]))


def mc_factorial(m, flags, ok, nominal_m, keep_coef: bool = False) -> McFactorial:
    """`ezpz_mc_factorial`: the factorial effects of the kept rows m [2^kc, n_meas] of a corner run, flags (the same shape; None: clear)
    and ok [2^kc] (None: every one set), about nominal_m [n_meas].  Computed on the host; the device form gives the same bytes."""
    m = np.ascontiguousarray(m, dtype=np.float64)
    if m.ndim != 2 or len(m) < 2 or len(m) & (len(m) - 1):
        raise ValueError(f"m [2^kc, n_meas] with kc >= 1: got {m.shape}")
    N, n_meas = m.shape
    kc = N.bit_length() - 1
    if flags is not None:
        flags = np.ascontiguousarray(flags, dtype=np.uint8).reshape(m.shape)
    if ok is not None:
        ok = np.ascontiguousarray(np.asarray(ok).reshape(N) != 0, dtype=np.uint8)
    nominal_m = np.ascontiguousarray(nominal_m, dtype=np.float64)
    if nominal_m.shape != (n_meas,):
        raise ValueError(f"nominal_m ({n_meas},): got {nominal_m.shape}")
    out = _factorial_outputs(min(kc, MC_FACTORIAL_MAX_CORNERS), min(n_meas, MC_FACTORIAL_MAX_MEAS), keep_coef)
    rc = lib().ezpz_mc_factorial(_ptr(m), _ptr(flags), _ptr(ok), _ptr(nominal_m), kc, n_meas, *(_ptr(a) for a in out))
    if rc != 0:
        raise NonLinearSystemError(rc)
    return McFactorial(*out)


class EffectsConfig:
    """The main effects of a `tolerance_mc` run: `bins` per driving dimension (2 .. 64; n_param x bins x n_meas <= 4096 cells) and
    their edges [n_param, bins - 1], absolute values, non-decreasing per dimension (+inf edges leave the upper bins empty).
    edges None: equiprobable edges from the run's distributions (`mc_effect_edges`)."""

    def __init__(self, bins: int = 8, edges=None):
        self.bins, self.edges = int(bins), edges


def mc_effect_edges(dists, nominal, bins: int) -> np.ndarray:
    """Equiprobable bin edges [n_param, bins - 1] for the distributions `dists` about `nominal`: UNIFORM nominal + a + (b - a) c /
    bins; NORMAL nominal + sigma z_c, z_c the equiprobable points of the (truncated) normal; CORNER one edge half way between its two
    values, the rest +inf; a dimension that does not vary (FIXED, sigma == 0, a == b): all +inf, one bin."""
    from statistics import NormalDist

    d = mc_dists(dists)
    nominal = np.ascontiguousarray(nominal, dtype=np.float64).reshape(-1)
    bins = int(bins)
    if len(nominal) != len(d):
        raise ValueError(f"nominal: one per distribution ({len(d)}), got {len(nominal)}")
    if bins < 2:
        raise ValueError(f"bins: at least 2, got {bins}")
    edges = np.full((len(d), bins - 1), np.inf)
    for j in range(len(d)):
        kind, a, b, nom = int(d["kind"][j]), float(d["a"][j]), float(d["b"][j]), float(nominal[j])
        if kind == McDist.UNIFORM and a != b:
            edges[j] = [nom + a + (b - a) * c / bins for c in range(1, bins)]
        elif kind == McDist.NORMAL and a != 0.0:
            nd = NormalDist()
            lo, hi = (nd.cdf(-b), nd.cdf(b)) if b > 0.0 else (0.0, 1.0)
            edges[j] = [nom + a * nd.inv_cdf(lo + (hi - lo) * c / bins) for c in range(1, bins)]
        elif kind == McDist.CORNER and a != b:
            edges[j, 0] = nom + (a + b) / 2.0
    return edges


def _effect_bounds(d, nominal) -> np.ndarray:
    """[n_param, 2]: the ends of every dimension's tolerance zone, infinite where it has none (an untruncated NORMAL)."""
    out = np.empty((len(d), 2))
    for j in range(len(d)):
        kind, a, b, nom = int(d["kind"][j]), float(d["a"][j]), float(d["b"][j]), float(nominal[j])
        if kind in (McDist.UNIFORM, McDist.CORNER):
            out[j] = (nom + min(a, b), nom + max(a, b))
        elif kind == McDist.NORMAL and b > 0.0:
            out[j] = (nom - a * b, nom + a * b)
        elif kind == McDist.NORMAL and a != 0.0:
            out[j] = (-np.inf, np.inf)
        else:
            out[j] = (nom, nom)
    return out


def _effects_request(effects: EffectsConfig, d, pos, nominal, system):
    """(EzpzMcEffectConfig, the edges used [n_param, bins - 1], the zones' ends [n_param, 2]) of a run with effects."""
    nom = np.array([system.records["param"][p] for p in pos], dtype=np.float64) if nominal is None else nominal
    bins = effects.bins
    if effects.edges is None:
        edges = mc_effect_edges(d, nom, min(max(bins, 2), MC_EFFECT_MAX_BINS))
    else:
        edges = np.ascontiguousarray(effects.edges, dtype=np.float64)
        if edges.shape != (len(pos), bins - 1):
            raise ValueError(f"edges: expected shape ({len(pos)}, {bins - 1}), got {edges.shape}")
    return CMcEffectConfig(bins, 0), edges, _effect_bounds(d, nom)


def _effect_outputs(n_param: int, n_meas: int, bins: int):
    k, m, B = min(n_param, MC_EFFECT_MAX_DIM), min(n_meas, MC_EFFECT_MAX_DIM), min(max(bins, 0), MC_EFFECT_MAX_BINS)
    return (np.zeros((k, B, m, 2)), np.zeros((k, B, m), np.uint64),
            (np.zeros((k, B, m)), np.zeros((k, B, m)), np.zeros((m, k)), np.zeros((m, k)), np.zeros((m, k), np.uint32)))


class McEffects:
    """What `mc_effect_indices` returns and a `tolerance_mc` run with effects carries: sums [k, B, m, 2] (sum_d, sum_d2) and counts
    [k, B, m] per (driving dimension, bin, reference dimension) as given, nominal_m [m], edges [k, B - 1] (None where unknown),
    cond_mean and cond_var [k, B, m] (the curve and the spread about it; NaN for an empty bin), eta2 and first [m, k] (the
    correlation ratio and its bias-corrected form, an estimate of the first-order Sobol index) and bins_used [m, k]."""

    def __init__(self, sums, counts, nominal_m, edges, cond_mean, cond_var, eta2, first, bins_used, bounds=None):
        self.sums, self.counts, self.nominal_m, self.edges = sums, counts, nominal_m, edges
        self.cond_mean, self.cond_var, self.eta2, self.first, self.bins_used = cond_mean, cond_var, eta2, first, bins_used
        self.bounds = bounds

    def curve(self, i: int, j: int):
        """(centres, means, counts) of reference dimension i along driving dimension j: the bins both of whose ends are finite --
        the edges, and at the two ends the tolerance zone's where the run knew them -- with their centre, conditional mean and
        count."""
        if self.edges is None:
            raise ValueError("curve: the edges are not known here")
        lo, hi = (-np.inf, np.inf) if self.bounds is None else self.bounds[j]
        ends = np.concatenate([[lo], self.edges[j], [hi]])
        with np.errstate(invalid="ignore"):
            live = np.isfinite(ends[:-1]) & np.isfinite(ends[1:])
        return ((ends[:-1][live] + ends[1:][live]) / 2.0, self.cond_mean[j, live, i], self.counts[j, live, i])


def mc_effects(params, m, flags, ok, nominal_m, edges, chunk: int = 0):
    """`ezpz_mc_effects`: (sums [n_param, bins, n_meas, 2], counts [n_param, bins, n_meas]) of the samples params [samples, n_param],
    m [samples, n_meas], flags (the same shape; None: clear) and ok [samples] (None: every one set) about nominal_m, binned by edges
    [n_param, bins - 1] -- the reduction alone, no system involved.  Computed on the host, in the device's order."""
    params, m = np.ascontiguousarray(params, dtype=np.float64), np.ascontiguousarray(m, dtype=np.float64)
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    if params.ndim != 2 or m.ndim != 2 or len(params) != len(m) or edges.ndim != 2 or len(edges) != params.shape[1]:
        raise ValueError(f"params [samples, n_param], m [samples, n_meas] and edges [n_param, bins - 1]: got {params.shape}, {m.shape} and {edges.shape}")
    samples, n_param, n_meas, bins = len(params), params.shape[1], m.shape[1], edges.shape[1] + 1
    if flags is not None:
        flags = np.ascontiguousarray(flags, dtype=np.uint8).reshape(samples, n_meas)
    if ok is not None:
        ok = np.ascontiguousarray(np.asarray(ok).reshape(samples) != 0, dtype=np.uint8)
    nominal_m = np.ascontiguousarray(nominal_m, dtype=np.float64)
    if nominal_m.shape != (n_meas,):
        raise ValueError(f"nominal_m ({n_meas},): got {nominal_m.shape}")
    sums, counts, _ = _effect_outputs(n_param, n_meas, bins)
    rc = lib().ezpz_mc_effects(_ptr(params), _ptr(m), _ptr(flags), _ptr(ok), _ptr(nominal_m), _ptr(edges), samples, n_param, n_meas, bins, int(chunk),
                               _ptr(sums), _ptr(counts))
    if rc != 0:
        raise NonLinearSystemError(rc)
    return sums, counts


def mc_effect_indices(sums, counts, nominal_m, edges=None, bounds=None) -> McEffects:
    """`ezpz_mc_effect_indices`: the closing step on sums [n_param, bins, n_meas, 2], counts [n_param, bins, n_meas] and nominal_m
    [n_meas].  Host only.  edges [n_param, bins - 1] and bounds [n_param, 2] only travel into the result, for `curve`."""
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    nominal_m = np.ascontiguousarray(nominal_m, dtype=np.float64)
    if sums.ndim != 4 or sums.shape[3] != 2 or counts.shape != sums.shape[:3] or nominal_m.shape != (sums.shape[2],):
        raise ValueError(f"sums [n_param, bins, n_meas, 2], counts [n_param, bins, n_meas] and nominal_m [n_meas]: got {sums.shape}, "
                         f"{counts.shape} and {nominal_m.shape}")
    n_param, bins, n_meas = counts.shape
    _, _, out = _effect_outputs(n_param, n_meas, bins)
    rc = lib().ezpz_mc_effect_indices(_ptr(sums), _ptr(counts), _ptr(nominal_m), n_param, n_meas, bins, *(_ptr(a) for a in out))
    if rc != 0:
        raise NonLinearSystemError(rc)
    return McEffects(sums, counts, nominal_m, None if edges is None else np.asarray(edges, dtype=np.float64), *out, bounds=bounds)


class SobolIndices:
    """What `mc_sobol_indices` returns and a `SobolResult` carries: sums [n_meas, 4 + 4 n_param] and n_complete [n_meas] as given,
    var [n_meas] (the pooled variance of A's and B's deviations), first and total [n_meas, n_param] (the first-order and the
    total-effect index) and first_var, total_var (the estimates' own variances: `first_se` and `total_se` are their square roots).
    `interaction` is total - first."""

    def __init__(self, sums, n_complete, var, first, total, first_var, total_var):
        self.sums, self.n_complete, self.var = sums, n_complete, var
        self.first, self.total, self.first_var, self.total_var = first, total, first_var, total_var

    @property
    def first_se(self) -> np.ndarray:
        with np.errstate(invalid="ignore"):
            return np.sqrt(self.first_var)

    @property
    def total_se(self) -> np.ndarray:
        with np.errstate(invalid="ignore"):
            return np.sqrt(self.total_var)

    @property
    def interaction(self) -> np.ndarray:
        return self.total - self.first


class SobolResult(SobolIndices):
    """What `System.tolerance_sobol` returns: the `SobolIndices`, matrix A's statistics as `tolerance_mc` gives them for the same
    seed (`stats`, `totals` and their fields -- n_valid, mean, std, var_a (stats' var), nominal, .. -- samples, n_ok), seed_b, and
    with keep the rows: f [samples, k + 2, n_meas], flags (the same shape) and ok [samples, k + 2]."""

    def __init__(self, stats, totals, sums, n_complete, var, first, total, first_var, total_var, kept, seed_b):
        super().__init__(sums, n_complete, var, first, total, first_var, total_var)
        self.stats, self.totals, self.seed_b = stats, totals, int(seed_b)
        for f in MC_STATS_DTYPE.names:
            setattr(self, "var_a" if f == "var" else f, stats[f])
        self.std = np.sqrt(stats["var"])
        self.samples, self.n_ok, self.n_all_in = (int(totals[f][0]) for f in MC_TOTALS_DTYPE.names)
        if kept is not None:
            self.f, self.flags, self.ok = kept


def _sobol_outputs(n_param: int, n_meas: int):
    return (np.zeros((n_meas, 4 + 4 * n_param)), np.zeros(n_meas, np.uint64),
            (np.zeros(n_meas), *(np.zeros((n_meas, n_param)) for _ in range(4))))


def mc_sobol_sums(f, flags, ok, nominal_m, fixed_mask: int = 0, chunk: int = 0):
    """`ezpz_mc_sobol_sums`: (sums [n_meas, 4 + 4 n_param], n_complete [n_meas]) of the pick-freeze rows f [samples, n_param + 2,
    n_meas] (row 0: A, row 1: B, row 2 + j: A with column j from B), flags (the same shape; None: clear) and ok [samples, n_param + 2]
    (None: every one set) about nominal_m; bit j of fixed_mask: dimension j is FIXED.  Computed on the host, in the device's order."""
    f = np.ascontiguousarray(f, dtype=np.float64)
    if f.ndim != 3 or f.shape[1] < 2:
        raise ValueError(f"f [samples, n_param + 2, n_meas]: got {f.shape}")
    samples, n_param, n_meas = f.shape[0], f.shape[1] - 2, f.shape[2]
    if flags is not None:
        flags = np.ascontiguousarray(flags, dtype=np.uint8).reshape(f.shape)
    if ok is not None:
        ok = np.ascontiguousarray(np.asarray(ok).reshape(samples, n_param + 2) != 0, dtype=np.uint8)
    nominal_m = np.ascontiguousarray(nominal_m, dtype=np.float64)
    if nominal_m.shape != (n_meas,):
        raise ValueError(f"nominal_m ({n_meas},): got {nominal_m.shape}")
    sums, n_complete, _ = _sobol_outputs(min(n_param, SOBOL_MAX), min(n_meas, SOBOL_MAX))
    rc = lib().ezpz_mc_sobol_sums(_ptr(f), _ptr(flags), _ptr(ok), _ptr(nominal_m), int(fixed_mask), samples, n_param, n_meas, int(chunk), _ptr(sums),
                                  _ptr(n_complete))
    if rc != 0:
        raise NonLinearSystemError(rc)
    return sums, n_complete


def mc_sobol_indices(sums, n_complete) -> SobolIndices:
    """`ezpz_mc_sobol_indices`: the closing step on sums [n_meas, 4 + 4 n_param] and n_complete [n_meas].  Host only."""
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    n_complete = np.ascontiguousarray(n_complete, dtype=np.uint64)
    if sums.ndim != 2 or sums.shape[1] < 4 or sums.shape[1] % 4 or n_complete.shape != (sums.shape[0],):
        raise ValueError(f"sums [n_meas, 4 + 4 n_param] and n_complete [n_meas]: got {sums.shape} and {n_complete.shape}")
    n_meas, n_param = sums.shape[0], sums.shape[1] // 4 - 1
    _, _, out = _sobol_outputs(min(n_param, SOBOL_MAX), min(n_meas, SOBOL_MAX))
    rc = lib().ezpz_mc_sobol_indices(_ptr(sums), _ptr(n_complete), n_param, n_meas, *(_ptr(a) for a in out))
    if rc != 0:
        raise NonLinearSystemError(rc)
    return SobolIndices(sums, n_complete, *out)


class BranchConfig:
    """EzpzBranchConfig but the seed: eps_abs, eps_rel (two answers are the same branch when every compared variable differs by at
    most eps_abs + eps_rel * max(|a|, |b|)), max_branches (1 .. 256) and chunk (samples per base and round; 0: the library's choice)."""

    def __init__(self, eps_abs: float = 1e-5, eps_rel: float = 1e-5, max_branches: int = 32, chunk: int = 0):
        self.eps_abs, self.eps_rel, self.max_branches, self.chunk = float(eps_abs), float(eps_rel), int(max_branches), int(chunk)

    def _c(self, seed: int = 0) -> CBranchConfig:
        return CBranchConfig(int(seed), self.chunk, self.max_branches, self.eps_abs, self.eps_rel)


class BranchResult:
    """What `System.solve_branches` and `cluster_branches` return: info (BRANCH_INFO_DTYPE [batch]), branches (BRANCH_DTYPE
    [batch, max_branches]; the slots at and beyond n_branches are zero), x [batch, max_branches, n_vars], the leaders' answers, and
    labels [batch, samples] (the slot, -1 not ok, -2 overflow; None without keep)."""

    def __init__(self, info, branches, x, labels):
        self.info, self.branches, self.x, self.labels = info, branches, x, labels
        self.n_branches = info["n_branches"].astype(np.int64)

    def nearest(self, base: int = 0) -> np.ndarray:
        """The slots of a base by dist_inf, the nearest first (equal distances: the lower slot)."""
        n = int(self.n_branches[base])
        return np.argsort(self.branches["dist_inf"][base, :n], kind="stable")


def _compare_mask(compare, n_vars: int):
    if compare is None:
        return None
    compare = np.asarray(compare)
    if compare.shape != (n_vars,):
        raise ValueError(f"compare: expected a mask of shape ({n_vars},), got {compare.shape}")
    return np.ascontiguousarray(compare != 0, dtype=np.uint8)


def _branch_outputs(batch: int, samples: int, n_vars: int, max_branches: int, keep: bool):
    return (np.zeros(batch, dtype=BRANCH_INFO_DTYPE), np.zeros((batch, max_branches), dtype=BRANCH_DTYPE),
            np.zeros((batch, max_branches, n_vars)), np.zeros((batch, samples), np.int32) if keep else None)


def cluster_branches(x, ok=None, compare=None, branch: Optional[BranchConfig] = None, keep: bool = False) -> BranchResult:
    """`ezpz_branch_cluster`: the clustering alone on x [batch, samples, n_vars] (or [samples, n_vars]: one base) with the flags ok
    [batch, samples] (None: every one set) -- no system involved.  dist_inf is measured from sample 0 of the base."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim == 2:
        x = x[None]
    if x.ndim != 3:
        raise ValueError(f"x: expected [batch, samples, n_vars], got {x.shape}")
    batch, samples, n_vars = x.shape
    if ok is not None:
        ok = np.ascontiguousarray(np.asarray(ok).reshape(batch, samples) != 0, dtype=np.uint8)
    mask, bc = _compare_mask(compare, n_vars), (branch or BranchConfig())._c()
    info, branches, xb, labels = _branch_outputs(batch, samples, n_vars, bc.max_branches, keep)
    rc = lib().ezpz_branch_cluster(_ptr(x), _ptr(ok), _ptr(mask), batch, samples, n_vars, C.byref(bc), _ptr(info), _ptr(branches), _ptr(xb),
                                   _ptr(labels))
    if rc != 0:
        raise NonLinearSystemError(rc)
    return BranchResult(info, branches, xb, labels)


def constraint_measure(record, x):
    """`ezpz_constraint_measure`: (m, grad [n_ids], flags) of one measurement record at the values x indexed by the record's ids;
    (0.0, an empty grad, 0) for a record that is not measurable.  Host only."""
    rec = stack_records([record])
    x = np.ascontiguousarray(x, dtype=np.float64)
    m, g, fl = C.c_double(0.0), np.zeros(8), C.c_int(0)
    n_ids = lib().ezpz_constraint_measure(rec.ctypes.data, x.ctypes.data, C.byref(m), g.ctypes.data, C.byref(fl))
    return m.value, g[:n_ids], fl.value


def constraint_param_derivative(record, x):
    """`ezpz_constraint_param_derivative`: (g [rows] = weight * d residual / d param at the values x indexed by the record's
    ids, degenerate flag); an empty g for a constraint without a parameter.  Host only."""
    rec = stack_records([record])
    x = np.ascontiguousarray(x, dtype=np.float64)
    g, deg = np.zeros(2), C.c_int(0)
    rows = lib().ezpz_constraint_param_derivative(rec.ctypes.data, x.ctypes.data, g.ctypes.data, C.byref(deg))
    return g[:rows], bool(deg.value)


def constraint_has_param(record) -> bool:
    """`ezpz_constraint_has_param`: whether the residual of this constraint record (its kind and tag) reads `param`."""
    rec = stack_records([record])
    return bool(lib().ezpz_constraint_has_param(rec.ctypes.data))


class MultiSystem:
    """One analysed topology resident on several devices of the node (`ezpz_multi_*`): a batch is sharded contiguously
    over them, one host worker thread per device, every shard over its own device's host link.  `device_mask` bit d =
    HIP device d, 0 = all."""

    def __init__(self, records, n_vars: int, device_mask: int = 0, team_size: int = 0):
        self.records = stack_records(records)
        self.n_vars = int(n_vars)
        h = C.c_void_p()
        ec, ev = C.c_int32(-1), C.c_int64(-1)
        rc = lib().ezpz_multi_create(self.records.ctypes.data if len(self.records) else None, len(self.records), self.n_vars,
                                     device_mask, team_size, C.byref(h), C.byref(ec), C.byref(ev))
        if rc != 0:
            raise NonLinearSystemError(rc, ec.value, ev.value)
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:
            lib().ezpz_multi_destroy(h)
            self._h = None

    def devices(self):
        return [lib().ezpz_multi_device(self._h, i) for i in range(lib().ezpz_multi_device_count(self._h))]

    def shard(self, batch: int, index: int):
        first, count = C.c_size_t(0), C.c_size_t(0)
        lib().ezpz_multi_shard(self._h, batch, index, C.byref(first), C.byref(count))
        return first.value, count.value

    def specialize(self, wait: bool = True) -> int:
        rc = lib().ezpz_multi_specialize(self._h, 1 if wait else 0)
        if rc < 0:
            raise NonLinearSystemError(rc)
        return rc

    def solve_batch(self, x0: np.ndarray, config: Optional[Config] = None, want_mask: bool = False, out=None):
        """x0 [batch, n_vars] -> (x, status, mask or None).  `out` = (x, status) arrays to fill (e.g. registered ones)."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1, max(self.n_vars, 1))
        batch = x0.shape[0]
        cfg = (config or Config())._c()
        x, st = out if out is not None else (np.empty_like(x0), np.zeros(batch, dtype=STATUS_DTYPE))
        mask = np.zeros((batch, max(len(self.records), 1)), dtype=np.uint8) if want_mask else None
        rc = lib().ezpz_multi_solve_batch(self._h, x0.ctypes.data, batch, C.byref(cfg), x.ctypes.data, st.ctypes.data,
                                          mask.ctypes.data if want_mask else None)
        if rc != 0:
            raise NonLinearSystemError(rc)
        return x, st, mask


class MixedBatch:
    """One batch of systems of DIFFERENT topologies (`ezpz_mixed_*`): system b has the topology
    `systems[topology_of_system[b]]`; x0 / x are RAGGED -- the systems' rows one after the other in batch order,
    `offsets[b]` = where system b's values start (`offsets[-1]` = the total).  Reusable for any number of solves."""

    def __init__(self, systems, topology_of_system):
        self.systems = list(systems)  # (kept alive: the handle refers to them)
        self.topology = np.ascontiguousarray(topology_of_system, dtype=np.uint32)
        self.batch = len(self.topology)
        handles = (C.c_void_p * len(self.systems))(*[s._h for s in self.systems])
        h = C.c_void_p()
        rc = lib().ezpz_mixed_create(handles, len(self.systems), self.topology.ctypes.data, self.batch, C.byref(h))
        if rc != 0:
            raise NonLinearSystemError(rc)
        self._h = h
        self.offsets = np.zeros(self.batch + 1, dtype=np.uint64)
        lib().ezpz_mixed_offsets(self._h, self.offsets.ctypes.data)
        self.total = int(lib().ezpz_mixed_total_values(self._h))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:
            lib().ezpz_mixed_destroy(h)
            self._h = None

    def solve(self, x0: np.ndarray, config: Optional[Config] = None):
        """x0: flat ragged array of `total` values -> (x flat, status [batch])."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1)
        assert x0.size == self.total, (x0.size, self.total)
        cfg = (config or Config())._c()
        x, st = np.empty_like(x0), np.zeros(self.batch, dtype=STATUS_DTYPE)
        rc = lib().ezpz_mixed_solve(self._h, x0.ctypes.data, C.byref(cfg), x.ctypes.data, st.ctypes.data)
        if rc != 0:
            raise NonLinearSystemError(rc)
        return x, st

    def solve_device(self, x0_ptr: int, x_out_ptr: int, status_ptr: int, stream: int = 0, config: Optional[Config] = None):
        """Device pointers (e.g. torch tensors' data_ptr()); only enqueues on `stream`."""
        cfg = (config or Config())._c()
        rc = lib().ezpz_mixed_solve_device(self._h, x0_ptr, C.byref(cfg), x_out_ptr, status_ptr, stream)
        if rc != 0:
            raise NonLinearSystemError(rc)


def solve_batch_mixed(systems, topology_of_system, x0: np.ndarray, config: Optional[Config] = None):
    """`ezpz_system_solve_batch_mixed`: the one-call form."""
    topo = np.ascontiguousarray(topology_of_system, dtype=np.uint32)
    x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1)
    handles = (C.c_void_p * len(systems))(*[s._h for s in systems])
    cfg = (config or Config())._c()
    x, st = np.empty_like(x0), np.zeros(len(topo), dtype=STATUS_DTYPE)
    rc = lib().ezpz_system_solve_batch_mixed(handles, len(systems), topo.ctypes.data, x0.ctypes.data, len(topo), C.byref(cfg),
                                             x.ctypes.data, st.ctypes.data)
    if rc != 0:
        raise NonLinearSystemError(rc)
    return x, st


def solve_batch_mixed_multi(multis, topology_of_system, x0: np.ndarray, config: Optional[Config] = None):
    """`ezpz_multi_solve_batch_mixed`: the ragged batch sharded over the devices the MultiSystems share."""
    topo = np.ascontiguousarray(topology_of_system, dtype=np.uint32)
    x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1)
    handles = (C.c_void_p * len(multis))(*[m._h for m in multis])
    cfg = (config or Config())._c()
    x, st = np.empty_like(x0), np.zeros(len(topo), dtype=STATUS_DTYPE)
    rc = lib().ezpz_multi_solve_batch_mixed(handles, len(multis), topo.ctypes.data, x0.ctypes.data, len(topo), C.byref(cfg),
                                            x.ctypes.data, st.ctypes.data)
    if rc != 0:
        raise NonLinearSystemError(rc)
    return x, st


def solve_batch_multi(records, n_vars: int, x0: np.ndarray, device_mask: int = 0, config: Optional[Config] = None):
    """`ezpz_system_solve_batch_multi`: the one-call form (handles cached by request bytes and mask)."""
    recs = stack_records(records)
    x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1, max(int(n_vars), 1))
    cfg = (config or Config())._c()
    x = np.empty_like(x0)
    st = np.zeros(x0.shape[0], dtype=STATUS_DTYPE)
    rc = lib().ezpz_system_solve_batch_multi(recs.ctypes.data if len(recs) else None, len(recs), int(n_vars), device_mask,
                                             x0.ctypes.data, x0.shape[0], C.byref(cfg), x.ctypes.data, st.ctypes.data)
    if rc != 0:
        raise NonLinearSystemError(rc)
    return x, st


def analyze(records, n_vars: int) -> dict:
    """Host-only symbolic analysis (`ezpz_analyze`): sizes of the topology program, no device needed."""
    a = stack_records(records)
    i = CSystemInfo()
    ec, ev = C.c_int32(-1), C.c_int64(-1)
    rc = lib().ezpz_analyze(a.ctypes.data if len(a) else None, len(a), int(n_vars), C.byref(i), C.byref(ec),
                            C.byref(ev))
    if rc != 0:
        raise NonLinearSystemError(rc, ec.value, ev.value)
    return {f: getattr(i, f) for f, _ in CSystemInfo._fields_}


def device_count() -> int:
    return lib().ezpz_device_count()


def launch_policy(compute_units: int = 0):
    """The table of launch-shape thresholds (include/ezpz_amd.h: EzpzLaunchPolicy) for a device of `compute_units` CUs
    (0 = the full 256-CU MI355X, as the header says -- NOT the current device: a caller on a CPX/DPX partition or a CU-masked
    device passes its own count, e.g. torch.cuda.get_device_properties(i).multi_processor_count)."""
    from ._lib import CLaunchPolicy

    p = CLaunchPolicy()
    rc = lib().ezpz_launch_policy(int(compute_units), C.byref(p))
    if rc != 0:
        raise NonLinearSystemError(rc, -1, -1)
    return p
