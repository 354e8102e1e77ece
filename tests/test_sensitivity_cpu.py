"""Dimension sensitivities, what can be checked without a device: the symbols and their signatures,
ezpz_constraint_param_derivative against central differences of the oracle's `residual` for every parametrised kind and tag, and
the numpy reference's own spread on every system the GPU tests use (tests/sensitivity_ref.py).

Bars.  The nine kinds that subtract their parameter (the issue counts ten; ArcLength is listed by kind_has_param but divides its
parameter by the radius): a central difference with h = 2^-10 is exact up to rounding, bar 1e-11 * max(1, |want|), the project's
residual parity bar.  ArcLength and the angle kinds: the oracle's central differences at h and h / 2 differ by three times the
error of the finer one (second order), so the bar is 4 x their difference + the 1e-11 bar.  Granted bars and spreads are appended
to $EZPZ_PROFILE_DIR/sensitivity_bar.txt when that variable is set (profiles/sensitivity_bar.txt is that file)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ezpz_amd as E
import sensitivity_ref as R
from ezpz_amd._lib import EXPORTS
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBTRACTING = (O.DISTANCE, O.VERTICAL_DISTANCE, O.HORIZONTAL_DISTANCE, O.FIXED, O.CIRCLE_RADIUS, O.ARC_RADIUS, O.POINT_LINE_DISTANCE,
               O.VERTICAL_POINT_LINE_DISTANCE, O.HORIZONTAL_POINT_LINE_DISTANCE)
CURVED = (O.ARC_LENGTH, O.LINES_AT_ANGLE, O.ARC_ANGLE, O.POINTS_AT_ANGLE)


def test_symbols_are_exported_with_the_documented_signatures():
    L = E.lib()
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ezpz_amd.h")).read())
    for name, nargs in (("ezpz_constraint_param_derivative", 4), ("ezpz_system_param_sensitivity_plan", 4),
                        ("ezpz_system_param_sensitivity_device", 11), ("ezpz_system_param_sensitivity", 10)):
        assert name in EXPORTS
        fn = getattr(L, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs
        decl = re.search(r"int %s\(([^)]*)\);" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs
    dev = re.search(r"int ezpz_system_param_sensitivity_device\(([^)]*)\);", header).group(1)
    assert [a.strip().split()[-1].lstrip("*") for a in dev.split(",")] == [
        "sys", "x_dev", "positions", "n_param", "params_dev", "batch", "lambda", "S_out_dev", "status_dev", "degenerate_count_dev", "stream"]
    host = re.search(r"int ezpz_system_param_sensitivity\(([^)]*)\);", header).group(1)
    assert [a.strip().split()[-1].lstrip("*") for a in host.split(",")] == [
        "sys", "x", "positions", "n_param", "params", "batch", "lambda", "S_out", "status_out", "degenerate_count_out"]
    assert "#define EZPZ_SENSITIVITY_MAX_COMPONENT_VARS 1024u" in header
    for method in ("param_sensitivity", "param_sensitivity_device", "param_sensitivity_plan"):
        assert callable(getattr(E.System, method))
    assert L.ezpz_constraint_param_derivative(None, None, None, None) == 0
    # the torch layer is a module of its own, not imported by the package
    assert "torch" not in open(os.path.join(ROOT, "ezpz_amd", "__init__.py")).read()
    assert os.path.exists(os.path.join(ROOT, "ezpz_amd", "torch_ops.py"))


def _points(rng):
    return rng.uniform(0.5, 3.0, 8) * rng.choice([-1.0, 1.0], 8) + np.arange(8) * 0.37


def test_param_derivative_against_the_oracles_residual():
    checked = 0
    widest = {}
    for kind in range(O.NUM_KINDS):
        for tag in range(4):
            rng = np.random.default_rng(100 * kind + tag)
            ids = list(rng.permutation(8)[: O.KIND_NUM_IDS[kind]])
            for weight in (1.0, 2.5, 0.375):
                x = _points(rng)
                rec = O.stack([O._mk(kind, ids, float(rng.uniform(0.3, 1.4)), tag=tag, weight=weight)])[0]
                got, deg = E.constraint_param_derivative(rec, x)
                if not E.constraint_has_param(rec):
                    assert len(got) == 0
                    continue
                assert len(got) == O.residual_dim(rec) and not deg
                d1, deg1 = R.central(rec, x, R.H)
                assert not deg1
                if kind in SUBTRACTING:
                    want, bar = d1, 1e-11 * np.maximum(1.0, np.abs(d1))
                    assert np.all(want == -weight)
                else:
                    assert kind in CURVED
                    d2, _ = R.central(rec, x, R.H / 2)
                    want, bar = d2, 4.0 * np.abs(d2 - d1) + 1e-11 * np.maximum(1.0, np.abs(d2))
                    # (and the extrapolated value the numpy reference uses is inside the same bar)
                    assert np.all(np.abs(R.dparam(rec, x)[0] - got) <= bar)
                err = np.abs(got - want)
                assert np.all(err <= bar), (O.KIND_NAMES[kind], tag, weight, got, want, bar)
                key = (O.KIND_NAMES[kind], tag)
                widest[key] = max(widest.get(key, (0.0, 0.0)), (float(bar.max()), float(err.max())))
                checked += 1
    assert checked == (10 * 4 + 3 * 2) * 3  # nine subtracting kinds and ArcLength whatever the tag, three angle kinds with two tags
    for (name, tag), (bar, err) in sorted(widest.items()):
        R.log(f"d residual / d param, {name} tag {tag}: widest bar granted {bar:.3e}, largest error {err:.3e}")


def test_param_derivative_of_a_degenerate_configuration_is_zero():
    x = np.asarray([1.0, 1.0, 1.0, 1.0, 2.0, 3.0, 0.5, 0.25])  # points 0 and 1 coincide
    for rec in (O.lines_at_angle((0, 1), (2, 3), (4, 5), (6, 7), ("rad", 0.4), weight=2.0), O.arc_length((0, 1), (2, 3), (4, 5), 1.5),
                O.points_at_angle((0, 1), (2, 3), (4, 5), ("deg", 20.0)), O.arc_angle((0, 1), (2, 3), (4, 5), ("deg", 20.0)),
                O.point_line_distance((4, 5), (0, 1), (2, 3), 1.0), O.vertical_point_line_distance((4, 5), (0, 1), (2, 3), 1.0)):
        rec = O.stack([rec])[0]
        assert O.residual(rec, x)[1]  # the oracle's residual calls it degenerate (and leaves zeros)
        got, deg = E.constraint_param_derivative(rec, x)
        want, _ = R.central(rec, x, R.H)
        assert deg and np.all(got == 0.0) and np.all(want == 0.0)
    # parallel / perpendicular: no parameter, no derivative
    assert len(E.constraint_param_derivative(O.stack([O.lines_at_angle((0, 1), (2, 3), (4, 5), (6, 7), "parallel")])[0], x)[0]) == 0


@pytest.mark.parametrize("name", R.all_names())
def test_the_references_own_spread_is_inside_the_ceiling(name):
    """20 x spread <= 1e-4 (the multiplier of tests/sensitivity.py, the reference's EPSILON) on every system the GPU tests use."""
    spreads = [s for _, s in R.references(name)]
    R.log(f"{name}: numpy reference, Cholesky against lstsq: spread {max(spreads):.3e} over {len(spreads)} systems (lambda {R.system(name)['lam']:g})")
    print(name, "spread", max(spreads))
    assert 20.0 * max(spreads) <= 1e-4, (name, spreads)
