"""tests/redundancy_ref.py held to definitions that do not share its code, and the inputs of tests/test_gpu_redundancy.py held to
margins around the tolerances (no GPU needed)."""
import numpy as np
import pytest

import redundancy_ref as R

NAMES = list(R.CASES)
# the kept drawn systems small enough for an SVD per row (a mosaic has sum(1 or 2 size) variables)
FUZZ_SMALL = [f"fuzz:{k}" for k, (sizes, _) in enumerate(R.FUZZ_DRAWN)
              if k not in R.FUZZ_REJECTED and sum(1 if v == 1 else 2 * v for v in sizes) <= 100]
GRID = ["grid:lane", "grid:rectangle", "grid:sketch45"]
# the systems of a case the GPU tests compare one by one (the block case: its first few here, all of them share one Jacobian)
SYSTEMS = 3


@pytest.mark.parametrize("name", NAMES + FUZZ_SMALL)
def test_reference_against_rank_definition(name):
    """Row i is independent iff it raises the rank of the rows up to it (SVD), and the rank is the matrix's."""
    for ref in R.references(name, 1 if name == "sketch150" else SYSTEMS):  # (300 SVDs of a 300-column matrix per system)
        J = ref["J"]
        prev = 0
        for i in range(len(J)):
            now = int(np.linalg.matrix_rank(J[: i + 1]))
            assert (ref["row_status"][i] == R.INDEPENDENT) == (now > prev), (name, i, ref["tau"][i])
            assert (ref["row_status"][i] == R.ZERO) == (not J[i].any()), (name, i)
            prev = now
        assert ref["rank"] == prev == int(np.linalg.matrix_rank(J))
        con = np.zeros(len(ref["con_status"]), np.uint8)
        for i, c in enumerate(ref["row_con"]):
            con[c] = max(con[c], ref["row_status"][i])
        assert np.array_equal(con, ref["con_status"])


@pytest.mark.parametrize("name", [n for n in NAMES if R.CASES[n][0] is not R.all_kinds] + FUZZ_SMALL)
def test_groups_against_least_squares(name):
    """A dependent row's expansion in the accepted rows before it, by lstsq instead of the triangular factor."""
    c = R.case(name)
    for ref in R.references(name, SYSTEMS):
        J, acc_all = ref["J"], np.asarray(ref["accepted"], dtype=int)
        norm = np.sqrt((J * J).sum(axis=1))
        for k, f in enumerate(c["focus"]):
            want = np.zeros(len(c["recs"]), np.uint8)
            rows = [i for i in range(len(J)) if ref["row_con"][i] == f and ref["row_status"][i] >= R.REDUNDANT]
            for i in rows:
                acc = acc_all[acc_all < i]
                coef = np.linalg.lstsq(J[acc].T, J[i], rcond=None)[0]
                for j in np.nonzero(np.abs(coef) * norm[acc] > R.GROUP_TOL * norm[i])[0]:
                    want[ref["row_con"][acc[j]]] = 1
                want[f] = 1
            assert np.array_equal(ref["group"][k], want), (name, f, np.nonzero(ref["group"][k])[0], np.nonzero(want)[0])


@pytest.mark.parametrize("name", NAMES + R.FUZZ_NAMES + list(R.PAIRS) + ["pairs:3", "pairs:3:embedded"] + GRID)
def test_inputs_keep_their_distance_from_the_tolerances(name):
    """Every tau is < 1e-11 or > 1e-3, every dependent row's |rho| / w < 1e-7 or > 1e-2, every group ratio < 1e-9 or > 1e-3: five
    decades and more around rank_tol = 1e-6, three and two around conflict_tol = 1e-4, three around group_tol = 1e-6 -- rounding in
    another summation order (1e-16 times a condition number these inputs keep small) cannot move a status."""
    c = R.case(name)
    for b, ref in enumerate(R.references(name, None if name != "blocks" else 8)):
        tau = ref["tau"][~np.isnan(ref["tau"])]
        assert np.all((tau < 1e-11) | (tau > 1e-3)), (name, b, tau[(tau >= 1e-11) & (tau <= 1e-3)])
        rho = ref["rho_w"][~np.isnan(ref["rho_w"])]
        assert np.all((rho < 1e-7) | (rho > 1e-2)), (name, b, rho[(rho >= 1e-7) & (rho <= 1e-2)])
        for per_focus in ref["ratios"]:
            for ratio in per_focus:
                assert np.all((ratio < 1e-9) | (ratio > 1e-3)), (name, b, ratio[(ratio >= 1e-9) & (ratio <= 1e-3)])


def _status(name, b=0):
    return R.references(name, 1)[b]["con_status"].tolist()


def test_what_the_cases_are_meant_to_show():
    """The statuses the issue names, on the reference: the GPU tests then only have to equal it."""
    for w in ("1:1", "0.001:1", "1:0.001"):
        for order in (0, 1):
            assert _status(f"one_variable:dup:{order}:{w}") == [0, 2]
            assert _status(f"one_variable:conflict:{order}:{w}") == [0, 3]  # the later record, whichever it is
    base = [0] * 8
    assert _status("rectangle:equal_length") == base + [2]
    assert _status("rectangle:side_weighted") == base + [2]
    assert _status("rectangle:side_conflict") == base + [3]
    ref = R.references("rectangle:coincident", 1)[0]
    assert ref["row_status"].tolist() == base + [2, 3] and ref["con_status"].tolist() == base + [3]
    # the side that cannot hold: made of the two verticals and the opposite side's length
    assert np.nonzero(R.references("rectangle:side_conflict", 1)[0]["group"][0])[0].tolist() == [3, 5, 6, 8]
    assert not R.references("rectangle:side_conflict", 1)[0]["group"][1].any()  # an independent constraint has no group
    ref = R.references("zero_row", 1)[0]
    assert ref["con_status"].tolist() == [0, 0, 1, 0] and ref["rank"] == 3
    rep, mov = R.references("all_kinds:repeated", 2), R.references("all_kinds:moved", 2)
    recs = R.case("all_kinds:moved")["recs"]
    for b in range(2):
        assert np.all(rep[b]["con_status"][25:] == R.REDUNDANT) and np.all(rep[b]["con_status"][:25] == R.INDEPENDENT)
        for kind in range(25):
            if int(recs[kind]["kind"]) in R.VALUE_KINDS:
                assert mov[b]["con_status"][25 + kind] == R.CONFLICTING, kind
    blocks = R.case("blocks")
    st = R.references("blocks", 2)
    nb = len(blocks["recs"]) - 8 - 6
    want = [R.CONFLICTING if float(blocks["recs"][i]["param"]) == 4.5 else R.REDUNDANT for i in range(nb, len(blocks["recs"]))]
    for b in range(2):
        assert st[b]["con_status"][nb:].tolist() == want and not st[b]["con_status"][:nb].any()
    for name, m_less in (("sketch24", False), ("sketch24:dropped", True), ("sketch150", False)):
        c, ref = R.case(name), R.references(name, 1)[0]
        nb = len(c["recs"]) - 6
        assert ref["con_status"][nb:].tolist() == [2, 2, 2, 3, 3, 2], (name, ref["con_status"][nb:])
        assert not ref["con_status"][:nb].any()
        assert (len(ref["row_status"]) < c["n_vars"]) == m_less


def test_drawn_systems_rejections_and_coverage():
    """FUZZ_REJECTED is what the margin bands reject of FUZZ_DRAWN, no more than a tenth of it; and the kept systems reach what they
    are drawn for -- every lane-group width, both thread counts, the three placements, several components, a focus list that
    moves the call from LANE to TEAM -- by the component sizes and workspaces restated in redundancy_ref.placement."""
    rejected = [k for k in range(len(R.FUZZ_DRAWN)) if R.within_margins(R.references(f"fuzz:{k}")[0])]
    assert rejected == sorted(R.FUZZ_REJECTED)
    assert 10 * len(rejected) <= len(R.FUZZ_DRAWN), (len(rejected), len(R.FUZZ_DRAWN))
    assert 36 <= len(R.FUZZ_NAMES) <= 44
    classes, several, moved = set(), 0, 0
    for name in R.FUZZ_NAMES:
        c = R.case(name)
        assert len(c["focus"]) == 6 and sorted(c["origin"]) == sorted(set(c["origin"]))
        comps = R.components(c["recs"], c["n_vars"])
        assert len(comps) >= len(R.DRAWN[name][1][0])  # (a part whose x and y chains never meet is two components)
        several += len(comps) >= 3
        with_l, without = R.placement(c["recs"], c["n_vars"], True), R.placement(c["recs"], c["n_vars"], False)
        moved += without[0] == R.LANE and with_l[0] != R.LANE
        for place, _, threads, n in (with_l, without):
            assert threads == (128 if place == R.LANE else 1024 if n > 64 else 256)
            classes.add((place, "n<=8" if n <= 8 else "n<=16" if n <= 16 else "n<=32" if n <= 32 else "n<=64" if n <= 64 else "n>64"))
    for want in [(R.TEAM_LDS, "n<=8"), (R.TEAM_LDS, "n<=16"), (R.TEAM_LDS, "n<=32"), (R.TEAM_LDS, "n<=64"), (R.TEAM_LDS, "n>64"),
                 (R.TEAM_GLOBAL, "n>64"), (R.LANE, "n<=8")]:
        assert want in classes, (want, sorted(classes))
    assert several >= 10 and moved >= 3, (several, moved)


def test_placements_of_the_named_cases():
    """The restated placement on the cases whose placement tests/redundancy_ref.py and the issue name."""
    place = lambda name, with_l: R.placement(R.case(name)["recs"], R.case(name)["n_vars"], with_l)
    assert place("blocks", True)[:3] == (R.LANE, 1, 128) and place("one_variable:dup:0:1:1", True)[:3] == (R.LANE, 128, 128)
    # (27 components: the two rows of points_coincident and of midpoint share no variable)
    assert place("all_kinds:moved", False)[:3] == (R.LANE, 4, 128) and place("all_kinds:moved", True)[:3] == (R.TEAM_LDS, 1, 256)
    assert place("rectangle:side_conflict", True) == (R.TEAM_LDS, 1, 256, 8)
    assert place("sketch24", True) == (R.TEAM_LDS, 1, 256, 48) and place("sketch150", True) == (R.TEAM_GLOBAL, 1, 1024, 300)
    assert place("grid:sketch45", True) == (R.TEAM_GLOBAL, 1, 1024, 90) and place("grid:sketch45", False)[0] == R.TEAM_LDS
    assert place("grid:lane", True)[:3] == (R.LANE, 1, 128)
    for (name, G) in (("pairs:30", 4), ("pairs:63", 2), ("pairs:1", 128), ("pairs:150", 1), ("pairs:3", 42)):
        assert place(name, True)[:3] == place(name, False)[:3] == (R.LANE, G, 128), name


@pytest.mark.parametrize("name", list(R.PAIRS) + ["pairs:3"])
def test_pairs_statuses_from_how_they_were_built(name):
    """[0, 2], [0, 3] or [1, 1] per component and system, all three present (one component: its own two), systems that differ."""
    c = R.case(name)
    want = R.pairs_expected(c)
    for b, ref in enumerate(R.references(name)):
        assert np.array_equal(ref["con_status"], want[b]), (name, b)
        assert ref["rank"] == int((want[b] == R.INDEPENDENT).sum())
    patterns = {tuple(p) for p in want.reshape(-1, 2).tolist()}
    assert patterns <= {(0, 2), (0, 3), (1, 1)} and (1, 1) in patterns and len(patterns) >= 2
    if len(c["moved"]) >= 30:
        assert len(patterns) == 3
    if len(want) > 1:
        assert len({w.tobytes() for w in want}) > 1


def test_what_the_grid_loop_inputs_show():
    """Neighbouring systems of a period differ (a kernel that read another system's data would show), and no shift of a period
    repeats it."""
    for name in GRID:
        refs = R.references(name)
        key = [r["con_status"].tobytes() + r["group"].tobytes() for r in refs]
        for shift in range(1, len(key)):
            assert key != key[shift:] + key[:shift], (name, shift)
    rect = R.references("grid:rectangle")
    assert [r["con_status"].tolist() for r in rect] == [[0] * 8 + [3], [0] * 6 + [1, 1, 1], [0] * 8 + [3]]
    assert [np.nonzero(r["group"][0])[0].tolist() for r in rect] == [[3, 5, 6, 8], [], [3, 4, 5, 6, 8]]


@pytest.mark.parametrize("name", ["all_kinds:repeated", "all_kinds:moved"])
def test_all_kinds_with_every_flagged_constraint_in_focus(name):
    """The focus list of test_gpu_redundancy.py: test_all_kinds_with_a_focus_list -- its group shares keep to the margins too."""
    c = R.case(name)
    focus = np.nonzero(R.references(name)[0]["con_status"] >= R.REDUNDANT)[0].tolist()
    assert focus == list(range(25, 50))
    for x in c["x"]:
        ref = R.analyse(c["recs"], c["n_vars"], x, focus)
        assert not R.within_margins(ref), R.within_margins(ref)[:3]
        assert all(ref["group"][k][focus[k]] and ref["group"][k][focus[k] - 25] for k in range(25))
