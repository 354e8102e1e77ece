"""The driver runs __graft_entry__.smoke() on the GPU box at the end of every round: the suite runs it too, so that a change of
launch shapes that smoke() asserts on is seen here first (round 5: the frontal shape changed what TEAM_AUTO_LATENCY means for a
140-variable sketch, and nothing but the driver would have noticed)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_the_drivers_smoke_check():
    import ezpz_amd

    if ezpz_amd.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: the product path has no CPU fallback")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import __graft_entry__ as entry

    entry.smoke()


def test_a_plain_bench_run_and_its_dumped_outputs(tmp_path):
    """`bench.py --steps K --warmup W` without --full prints the headline line and nothing the headline does not need; with
    --dump-outputs two runs of the same arguments write the same inputs' results, bit for bit, as float64 arrays."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dumps = []
    for run in ("a", "b"):
        out = tmp_path / run
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--batch", "2048", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        line = json.loads(lines[0])
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0 and line["results_ok"] is True
        assert line["unit"] == "solves/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
        assert not {"configs", "cpu_baseline", "oracle_check", "extras", "pmc_per_launch"} & set(line)
        dumps.append({f[:-4]: np.load(out / f) for f in os.listdir(out)})
    a, b = dumps
    assert set(a) == set(b) and {"x", "systems", "status_iterations", "status_converged"} <= set(a)
    assert all(v.dtype == np.float64 for v in a.values()) and sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["x"].shape == (2048, 2000) and np.array_equal(a["systems"], np.arange(2048))
    assert np.all(a["status_iterations"] == 2) and np.all(a["status_converged"] == 1)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
