"""tests/redundancy_ref.py held to definitions that do not share its code, and the inputs of tests/test_gpu_redundancy.py held to
margins around the tolerances (no GPU needed)."""
import numpy as np
import pytest

import redundancy_ref as R

NAMES = list(R.CASES)
# the systems of a case the GPU tests compare one by one (the block case: its first few here, all of them share one Jacobian)
SYSTEMS = 3


@pytest.mark.parametrize("name", NAMES)
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


@pytest.mark.parametrize("name", [n for n in NAMES if R.CASES[n][0] is not R.all_kinds])
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


@pytest.mark.parametrize("name", NAMES)
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
