"""Driven dimensions on the frontal shape (ezpz_system_set_params_route) without a device: the surface the header declares, and a
condition on the inputs of the oracle test of tests/test_gpu_front_params.py."""
import os
import re

import numpy as np
import pytest

import ezpz_amd as E
from oracle import oracle as O
from sweep_common import chain, substituted

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ezpz_amd.h")
ERR_INVALID_ARGUMENT = -103


def test_export_and_constants():
    from ezpz_amd import _lib

    text = open(HEADER).read()
    assert re.search(r"\bint ezpz_system_set_params_route\(EzpzSystem\* sys, uint32_t route\);", text)
    assert "ezpz_system_set_params_route" in _lib.EXPORTS and hasattr(E.lib(), "ezpz_system_set_params_route")
    assert "#define EZPZ_PARAMS_ROUTE_DEFAULT 0u" in text and "#define EZPZ_PARAMS_ROUTE_FRONTS 1u" in text
    assert (_lib.PARAMS_ROUTE_DEFAULT, _lib.PARAMS_ROUTE_FRONTS) == (0, 1)
    assert _lib.PARAMS_ROUTES == {"default": 0, "fronts": 1}
    assert callable(E.System.set_params_route)


def test_null_system_is_an_argument_error():
    assert E.lib().ezpz_system_set_params_route(None, 1) == ERR_INVALID_ARGUMENT
    assert E.lib().ezpz_system_set_params_route(None, 0) == ERR_INVALID_ARGUMENT


def test_sweep_route_of_the_fronts_is_5():
    from ezpz_amd import _lib

    text = open(HEADER).read()
    # (defined as the route behind the entry's own five, whose defines are literals 0u .. 4u)
    assert re.search(r"^#define EZPZ_SWEEP_FRONTS \(EZPZ_SWEEP_RECORD_WALK \+ 1u\)$", text, re.M)
    assert re.search(r"^#define EZPZ_SWEEP_RECORD_WALK 4u\b", text, re.M)
    assert _lib.SWEEP_FRONTS == 5 and _lib.SWEEP_ROUTE_NAMES[5] == "fronts" and len(_lib.SWEEP_ROUTE_NAMES) == 6


@pytest.mark.parametrize("npts", [40, 200])
def test_oracle_converges_on_the_oracle_tests_inputs(npts):
    """A condition on the inputs, not on the device: the chain of points with every parameter drawn +-0.1 and starts +-0.03 (the
    draw of test_chain_against_the_oracle) -- the oracle alone converges on all 8 systems."""
    recs, g = chain(npts)
    rng = np.random.default_rng(21)
    pos = np.asarray([i for i in range(len(recs)) if E.constraint_has_param(recs[i])], dtype=np.uint32)
    params = recs["param"][pos][None, :] + rng.uniform(-0.1, 0.1, (8, len(pos)))
    x0 = g[None, :] + rng.uniform(-0.03, 0.03, (8, len(g)))
    for b in range(8):
        rc, x, it, conv, nun = O.solve_batch(substituted(recs, pos, params[b]), x0[b:b + 1], None, linsolve=O.LINSOLVE_SPARSE)
        assert rc == 0 and int(conv[0]) == 1 and int(nun[0]) == 0 and np.all(np.isfinite(x)), (npts, b, int(it[0]))


@pytest.mark.parametrize("name,amplitude,jitter", [("tree60", 1e-3, 0.02), ("tree108", 1e-4, 1e-3)])
def test_oracle_converges_on_the_wide_fronts_oracle_tests_inputs(name, amplitude, jitter):
    """The same condition on the inputs of test_wide_fronts_against_the_oracle: tree60 at the default draw of
    tests/test_gpu_front_params.py (seed 33, parameters +-1e-3, starts +-0.02; measured: 3 iterations on each of the 8 systems),
    tree108 at its small draw (+-1e-4, +-1e-3; 3 to 4 iterations) -- at the default draw the oracle runs to its iteration limit
    on all 8 systems of tree108, which would make a test of statuses on the device a test of how two solvers fail."""
    import front_sens_ref as FS

    recs, g = FS.inputs(name)
    rng = np.random.default_rng(33)
    pos = np.asarray([i for i in range(len(recs)) if E.constraint_has_param(recs[i])], dtype=np.uint32)
    assert len(pos) == len(recs)
    params = recs["param"][pos][None, :] + rng.uniform(-amplitude, amplitude, (8, len(pos)))
    x0 = g[None, :] + rng.uniform(-jitter, jitter, (8, len(g)))
    for b in range(8):
        rc, x, it, conv, nun = O.solve_batch(substituted(recs, pos, params[b]), x0[b:b + 1], None, linsolve=O.LINSOLVE_SPARSE)
        assert rc == 0 and int(conv[0]) == 1 and int(nun[0]) == 0 and np.all(np.isfinite(x)), (name, b, int(it[0]))
        assert int(it[0]) <= 4, (name, b, int(it[0]))
