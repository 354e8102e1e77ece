"""Guarded sweeps (ezpz_system_sweep_guarded) without a device: the surface the header declares, the crank -- the input whose
every decision the oracle fixes with a margin -- and a condition on the random-walk inputs of tests/test_gpu_guarded_sweep.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ezpz_amd as E
from guarded_sweep_common import (CRANK_MAX_MOVE, CRANK_PLAIN_TABLE, CRANK_PLAIN_TARGETS, CRANK_TABLE, CRANK_TARGETS, crank, crank_params,
                                  guard_table, guarded_shapes, oracle_rule, walk_inputs)

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ezpz_amd.h")
DEVICE_ARGS = ["sys", "x0_dev", "positions", "n_param", "params0_dev", "params_dev", "steps", "batch", "cfg", "guard_cfg", "x_out_dev",
               "status_dev", "guard_dev", "params_reached_dev", "unsat_mask_dev", "warn_log_dev", "warn_cap", "stream"]
HOST_ARGS = ["sys", "x0", "positions", "n_param", "params0", "params", "steps", "batch", "cfg", "guard_cfg", "x_out", "status", "guard",
             "params_reached", "unsat_mask", "warn_log", "warn_cap"]


def _arg_names(text, name):
    decl = re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1)
    return [a.split()[-1].lstrip("*") for a in decl.replace("\n", " ").split(",")]


def test_header_structs_exports_defaults_and_methods():
    from ezpz_amd import _lib

    text = open(HEADER).read()
    for name in ("ezpz_system_sweep_guarded_plan", "ezpz_system_sweep_guarded_device", "ezpz_system_sweep_guarded"):
        assert re.search(r"\bint %s\(EzpzSystem\* sys," % name, text), name
        assert name in _lib.EXPORTS and hasattr(E.lib(), name), name
    assert re.search(r"\bvoid ezpz_default_guard_config\(EzpzGuardConfig\* out\);", text)
    assert "ezpz_default_guard_config" in _lib.EXPORTS and hasattr(E.lib(), "ezpz_default_guard_config")
    assert _arg_names(text, "ezpz_system_sweep_guarded_device") == DEVICE_ARGS
    assert _arg_names(text, "ezpz_system_sweep_guarded") == HOST_ARGS
    assert _arg_names(text, "ezpz_system_sweep_guarded_plan") == ["sys", "positions", "n_param", "out"]
    assert len(E.lib().ezpz_system_sweep_guarded_device.argtypes) == len(DEVICE_ARGS)
    assert len(E.lib().ezpz_system_sweep_guarded.argtypes) == len(HOST_ARGS)
    # the structs: the header's fields, in order, are the ctypes structs' and the numpy record's
    ctype = {"uint32_t": C.c_uint32, "double": C.c_double}
    for struct, mirror, size in (("EzpzGuardConfig", _lib.CGuardConfig, 16), ("EzpzGuardStep", _lib.CGuardStep, 16)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
        fields = re.findall(r"^\s*(uint32_t|double)\s+(\w+);", body, re.M)
        assert [(n, ctype[t]) for t, n in fields] == list(mirror._fields_), struct
        assert C.sizeof(mirror) == size, struct
    assert _lib.GUARD_STEP_DTYPE.itemsize == 16 and _lib.GUARD_STEP_DTYPE.names == ("reached", "attempts", "accepted")
    assert [_lib.GUARD_STEP_DTYPE.fields[n][1] for n in _lib.GUARD_STEP_DTYPE.names] == [0, 8, 12]
    assert E.GUARD_STEP_DTYPE is _lib.GUARD_STEP_DTYPE
    # the defaults: the library's, the table's and the Python mirror's
    g = _lib.CGuardConfig(99, 99, 99.0)
    E.lib().ezpz_default_guard_config(C.byref(g))
    assert (g.max_halvings, g.max_attempts, g.max_move) == (4, 12, 0.0)
    d = E.GuardConfig()
    assert (d.max_halvings, d.max_attempts, d.max_move) == (4, 12, 0.0)
    c = E.GuardConfig(2, 5, 0.5)._c()
    assert (c.max_halvings, c.max_attempts, c.max_move) == (2, 5, 0.5)
    for bad in (E.GuardConfig(max_halvings=21), E.GuardConfig(max_attempts=0), E.GuardConfig(max_move=float("inf")),
                E.GuardConfig(max_move=float("nan")), E.GuardConfig(max_halvings=-1)):
        with pytest.raises(ValueError):
            bad._c()
    for method in ("sweep_guarded", "sweep_guarded_device", "sweep_guarded_plan"):
        assert callable(getattr(E.System, method))
    import inspect

    assert list(inspect.signature(E.System.sweep_guarded).parameters) == ["self", "x0", "positions", "params0", "params", "guard", "config",
                                                                          "want_mask", "warn_log"]


def test_the_crank_on_the_oracle():
    """A condition on the inputs: the oracle alone, under the rule, takes exactly the decisions of the table, each with a margin -- no
    displacement of a converged attempt lies within 0.02 of max_move, and every attempt that fails for infeasibility leaves three
    constraints unsatisfied."""
    recs, pos, x0, params0 = crank()
    moves, infeasible = [], []

    def see(k, b, info, moved, ok):
        it, conv, nun = info[b]
        if conv == 1 and nun == 0:
            moves.append(float(moved.max()))
        else:
            infeasible.append(nun)

    x, g, reached = oracle_rule(recs, pos, x0, params0, crank_params(CRANK_TARGETS), on_attempt=see, max_move=CRANK_MAX_MOVE)
    table = guard_table(g, reached)
    print("crank:", table, "| displacements of converged attempts:", sorted(round(m, 4) for m in moves), "| unsatisfied:", infeasible)
    assert [(r, a, c) for r, a, c, _ in table] == [(r, a, c) for r, a, c, _ in CRANK_TABLE], table
    assert np.allclose([p for *_, p in table], [p for *_, p in CRANK_TABLE], rtol=0, atol=1e-12), table
    assert all(abs(m - CRANK_MAX_MOVE) > 0.02 for m in moves), sorted(moves)
    below, above = max(m for m in moves if m < CRANK_MAX_MOVE), min(m for m in moves if m > CRANK_MAX_MOVE)
    assert abs(below - 0.2168) < 5e-4 and abs(above - 0.2783) < 5e-4, (below, above)
    assert infeasible and all(n == 3 for n in infeasible), infeasible
    # every row holds the last accepted answer: on the circle, at the driven value reached
    assert np.allclose(x[:, 0, 2], reached[:, 0, 0], atol=1e-7) and np.allclose(np.hypot(x[:, 0, 2], x[:, 0, 3]), 1.0, atol=1e-7)
    # the plain sweep that holds the last good answer
    x, g, reached = oracle_rule(recs, pos, x0, params0, crank_params(CRANK_PLAIN_TARGETS), max_halvings=0, max_move=0.0)
    assert [(float(r), int(a)) for r, a in zip(g["reached"][:, 0], g["attempts"][:, 0])] == CRANK_PLAIN_TABLE
    assert np.allclose(x[1, 0, 2:], [0.5, 0.866], atol=1e-3) and np.array_equal(x[1], x[0]) and reached[1, 0, 0] == 0.5


@pytest.mark.parametrize("name", ["sub-wavefront teams", "barrier workgroup", "record walk"])
def test_oracle_rule_reaches_the_targets_of_the_gpu_tests_walks(name):
    """A condition on the inputs, not on the device: under the rule the oracle alone reaches the target (reached == 1) on at least
    0.9 of all (sweep, step) pairs of each shape's walk -- and not all of them at the first attempt."""
    recs, g, _, _ = guarded_shapes(E)[name]
    sweeps, steps = (32, 5) if name == "sub-wavefront teams" else (6, 3)
    pos, params0, params, x0, max_move = walk_inputs(E, name, recs, g, sweeps, steps, 71)
    x, gs, reached = oracle_rule(recs, pos, x0, params0, params, max_move=max_move)
    print(name, "reached 1 on", int((gs["reached"] == 1.0).sum()), "of", gs.size, "| attempts", np.bincount(gs["attempts"].ravel()).tolist())
    assert np.all(np.isfinite(x))
    assert (gs["reached"] == 1.0).mean() >= 0.9, (name, gs["reached"])
    assert gs["attempts"].max() > 1, name
