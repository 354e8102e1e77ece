"""What the component planner outputs (csrc/comp_program.cpp, comp_source.cpp), pinned: tools/comp_plan_digest.cpp, a plain g++
program on the planner's sources, prints one digest per output -- blob, generated HIP source, scalar fields, parameter overlay of
comp_plan_build; both sources and the scalars of lane_plan_build; blob and scalars of batch_plan_build -- for 200 seeded random
block systems, a block system with constants that are not f32-exact, a hub, and the project's own workloads, under each of the
generator's environment switches.  Every line must equal tests/golden/comp_plan/digests.json: a change to the generator that is
meant for one shape shows here which other shapes it moved (tools/comp_plan_digest.cpp --dump shows where).  The outputs are a
pure function of the request, the limits and the switches, so no GPU is needed."""
import json
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

from ezpz_amd.synthetic import make_workload

PINNED = os.path.join(GOLDEN, "comp_plan", "digests.json")
WORKLOADS = ["massive500", "massive200", "massive600", "massive500o", "massive50000", "sketch24",
             "square", "two_rectangles", "tiny", "nonsquare", "underconstrained"]
# the switches are read into function statics: one process per setting (all other switches unset)
SETTINGS = {
    "default": {},
    "EZPZ_JIT_FASTDIV=0": {"EZPZ_JIT_FASTDIV": "0"},
    "EZPZ_JIT_FASTDIV=7": {"EZPZ_JIT_FASTDIV": "7"},
    "EZPZ_JIT_GRID_STAGE=0": {"EZPZ_JIT_GRID_STAGE": "0"},
    "EZPZ_JIT_GRID_STAGE=2": {"EZPZ_JIT_GRID_STAGE": "2"},
    "EZPZ_JIT_WAVES=8 EZPZ_JIT_MINWAVES=2 EZPZ_JIT_FAST_MINWAVES=3": {"EZPZ_JIT_WAVES": "8", "EZPZ_JIT_MINWAVES": "2", "EZPZ_JIT_FAST_MINWAVES": "3"},
}


@pytest.fixture(scope="module")
def digests(tmp_path_factory):
    """{setting: {case: line}} from the program built on the tree's planner sources."""
    tmp = tmp_path_factory.mktemp("comp_plan")
    exe = str(tmp / "comp_plan_digest")
    csrc = os.path.join(ROOT, "ezpz_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "comp_plan_digest.cpp")] +
                          [os.path.join(csrc, s) for s in ("comp_program.cpp", "comp_source.cpp", "program.cpp")] + ["-o", exe])
    args = []
    for name in WORKLOADS:
        _, records, guesses, _, _ = make_workload(name)
        path = str(tmp / (name + ".records"))
        records.tofile(path)
        args.append("%s:%s:%d" % (name, path, len(guesses)))
    clean = {k: v for k, v in os.environ.items() if not k.startswith("EZPZ_")}
    runs = {setting: subprocess.Popen([exe] + args, env=dict(clean, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            for setting, env in SETTINGS.items()}
    out = {}
    for setting, run in runs.items():
        stdout, stderr = run.communicate(timeout=300)
        assert run.returncode == 0, stderr[-2000:]
        out[setting] = {line.split(" ", 1)[0]: line.split(" ", 1)[1] for line in stdout.splitlines()}
    if os.environ.get("EZPZ_PIN_COMP_PLAN") == "1":  # recording (on the commit whose output is the measure): the default setting
        pinned = {"default": out["default"]}                # in full, of every other setting the lines that differ from it
        for setting in list(SETTINGS)[1:]:
            pinned[setting] = {case: line for case, line in out[setting].items() if line != out["default"][case]}
        os.makedirs(os.path.dirname(PINNED), exist_ok=True)
        with open(PINNED, "w") as f:
            json.dump(pinned, f, indent=0, sort_keys=True)
            f.write("\n")
    return out


def _fields(line):
    return dict(tok.split("=", 1) for tok in line.split())


def test_every_output_of_the_planners_is_the_pinned_one(digests):
    with open(PINNED) as f:
        pinned = json.load(f)
    assert list(pinned) == sorted(SETTINGS)
    for setting in SETTINGS:
        want = dict(pinned["default"], **pinned[setting])
        got = digests[setting]
        assert sorted(got) == sorted(want), setting
        moved = {case: (got[case], want[case]) for case in want if got[case] != want[case]}
        assert not moved, (setting, len(moved), sorted(moved)[:20], next(iter(moved.values())))


def test_every_switch_reaches_the_corpus(digests):
    for setting in list(SETTINGS)[1:]:
        assert digests[setting] != digests["default"], setting


def test_the_corpus_covers_the_generator(digests):
    """Counts of the seed's 200 block systems on the commit that introduced the test: 127 component plans, 34 interpretable, 93 on
    several workgroups, 40 with wavefront ranges; the thresholds leave room for nothing but a shrunken corpus to fail."""
    cases = {case: _fields(line) for case, line in digests["default"].items()}
    comp = [f for f in cases.values() if f["comp"] != "rejected"]
    assert len(cases) == 200 + 2 + len(WORKLOADS)
    assert len(comp) >= 120
    assert sum(f["interp"] == "1" for f in comp) >= 30
    assert sum(int(f["wgs"]) > 1 for f in comp) >= 30
    assert sum(f["ranges"] == "1" for f in comp) >= 30
    assert any(f["nonlinear"] == "1" for f in comp) and any(f["nonlinear"] == "0" for f in comp)
    assert any(f["unit"] == "0" for f in comp) and any(f["unit"] == "1" for f in comp)
    assert cases["inexact"]["inexact"] == "1"
    assert any(f["comp"] == "rejected" for f in cases.values())
    lanes = [f for f in cases.values() if f["lane"] != "rejected"]
    assert len(lanes) >= 200 and sum(f["batch"] != "rejected" for f in cases.values()) >= 200
    for kind in ("across", "serial", "none"):  # HAS_TAIL_WAVE = true / = false, no wave source at all
        assert any(f["wave"] == kind for f in lanes), kind
    for name in ("massive500", "massive200", "massive600", "massive500o", "massive50000"):
        assert cases[name]["comp"] != "rejected", name
    assert int(cases["massive50000"]["wgs"]) > 1 and cases["massive50000"]["interp"] == "0"
    assert cases["massive500o"]["nonlinear"] == "1"
    assert cases["sketch24"]["batch"] != "rejected"
    for name in ("square", "two_rectangles", "tiny", "nonsquare", "underconstrained"):
        assert cases[name]["lane"] != "rejected" and cases[name]["wave"] != "none", name
