"""Dimension sweeps (ezpz_system_sweep_params) without a device: the surface the header declares, and a condition on the inputs of
the oracle test of tests/test_gpu_sweep.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ezpz_amd as E
from sweep_common import CASES, oracle_chain, oracle_inputs

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ezpz_amd.h")
ENTRIES = ("ezpz_system_sweep_params_plan", "ezpz_system_sweep_params_device", "ezpz_system_sweep_params")


def test_header_struct_and_exports():
    from ezpz_amd import _lib

    text = open(HEADER).read()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(EzpzSystem\* sys," % name, text), name
        assert name in _lib.EXPORTS and hasattr(E.lib(), name), name
    # the device form's arguments, in the order the issue fixes
    decl = re.search(r"int ezpz_system_sweep_params_device\((.*?)\);", text, re.S).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.replace("\n", " ").split(",")]
    assert names == ["sys", "x0_dev", "positions", "n_param", "params_dev", "steps", "batch", "cfg", "x_out_dev", "status_dev",
                     "unsat_mask_dev", "warn_log_dev", "warn_cap", "stream"]
    assert len(_lib.lib().ezpz_system_sweep_params_device.argtypes) == len(names)
    assert len(_lib.lib().ezpz_system_sweep_params.argtypes) == len(names) - 1
    # EzpzSweepPlan: the header's fields, in order, are the ctypes struct's
    body = re.search(r"typedef struct EzpzSweepPlan \{(.*?)\} EzpzSweepPlan;", text, re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|uint64_t)\s+(\w+);", body, re.M)
    ctype = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.CSweepPlan._fields_)
    assert [n for _, n in fields] == ["route", "in_kernel", "params_in_lds", "lds_bytes"] and C.sizeof(_lib.CSweepPlan) == 16
    routes = re.findall(r"#define EZPZ_SWEEP_(\w+) (\d)u", text)
    assert [int(v) for _, v in routes] == list(range(len(_lib.SWEEP_ROUTES))) == list(range(5))
    for method in ("sweep_params", "sweep_params_device", "sweep_params_plan"):
        assert callable(getattr(E.System, method))


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_chain_converges_on_the_oracle_tests_inputs(name):
    """A condition on the inputs, not on the device: the oracle alone, chained from its own answers, converges on at least 0.9 of
    all (sweep, step) pairs of every kind's paths."""
    recs, pos, params, x0 = oracle_inputs(name)
    x, it, conv, nun, mask, _ = oracle_chain(recs, pos, params, x0)
    print(name, "converged", int(conv.sum()), "of", conv.size, "| iterations up to", int(it.max()))
    assert np.all(np.isfinite(x))
    assert conv.mean() >= 0.9, (name, conv.mean())
