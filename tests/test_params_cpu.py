"""Per-system constraint parameters: what can be checked without a device -- the three symbols and their signatures, and
ezpz_constraint_has_param against the oracle's residuals (for every kind and tag: 1 exactly where changing `param` changes
residual(c, x) at a generic point)."""
import ctypes as C
import os
import re

import numpy as np

import ezpz_amd as E
from ezpz_amd._lib import EXPORTS
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_with_the_documented_signatures():
    L = E.lib()
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ezpz_amd.h")).read())
    for name, nargs in (("ezpz_constraint_has_param", 1), ("ezpz_system_solve_batch_params_device", 13),
                        ("ezpz_system_solve_batch_params", 12)):
        assert name in EXPORTS
        fn = getattr(L, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs
        decl = re.search(r"int %s\(([^)]*)\);" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs
    dev = re.search(r"int ezpz_system_solve_batch_params_device\(([^)]*)\);", header).group(1)
    assert [a.strip().split()[-1].lstrip("*") for a in dev.split(",")] == [
        "sys", "x0_dev", "positions", "n_param", "params_dev", "batch", "cfg", "x_out_dev", "status_dev", "unsat_mask_dev",
        "warn_log_dev", "warn_cap", "stream"]
    assert callable(E.System.solve_batch_params) and callable(E.System.solve_batch_params_device)
    assert E.lib().ezpz_constraint_has_param(None) == 0


def _residual_reads_param(kind, tag):
    """The oracle's residual of a constraint of this kind and tag at generic points, for several pairs of parameters."""
    rng = np.random.default_rng(1000 * kind + tag)
    ids = list(range(O.KIND_NUM_IDS[kind]))
    for _ in range(4):
        x = rng.uniform(0.5, 3.0, 8) * rng.choice([-1.0, 1.0], 8) + np.arange(8) * 0.37
        p, q = rng.uniform(0.2, 1.3, 2) * (1.0, 2.0)
        ra, da = O.residual(O._mk(kind, ids, float(p), tag=tag), x)
        rb, db = O.residual(O._mk(kind, ids, float(q), tag=tag), x)
        assert not da and not db, (kind, tag)
        if list(ra) != list(rb):
            return True
    return False


def test_has_param_is_where_the_oracles_residual_reads_it():
    seen = 0
    for kind in range(O.NUM_KINDS):
        for tag in range(4):  # every tag any kind gives a meaning to: sides 0-2, angle kinds 0-3
            want = _residual_reads_param(kind, tag)
            rec = O._mk(kind, list(range(O.KIND_NUM_IDS[kind])), 1.25, tag=tag)
            got = E.constraint_has_param(O.stack([rec])[0])
            assert got == want, (O.KIND_NAMES[kind], tag, got, want)
            seen += int(want)
    # ten kinds whatever their tag, three angle kinds with the two tags that carry a value
    assert seen == 10 * 4 + 3 * 2
