"""What tests/handle_history_cases.py promises of its clouds, checked without a GPU: the sizes at which the shared pieces of the
kernels change their shape, and that no kNN row of the table rests on an exact tie (DESIGN.md section 10 leaves those open)."""
import numpy as np
import pytest

import handle_history_cases as Cs


def test_cloud_statistics():
    s = {c: Cs.statistics(c) for c in Cs.SIZES}
    assert s["c70"]["groups"] == 2 and s["c70"]["last_leaf"] != 0 and s["c70"]["n"] == s["c70"]["n_in"] == 70  # two query groups, the last leaf part full
    assert s["c1300"]["tiles"] == 2 and 0 < s["c1300"]["last_tile"] < Cs.SCAN_TILE                               # a second scan tile, partly filled
    assert s["c1300b"]["n_in"] == s["c1300"]["n_in"] and not np.array_equal(Cs.inputs("c1300b")["points"], Cs.inputs("c1300")["points"])
    g = s["c5000g"]
    assert 0 < g["n"] < g["n_in"] == 5000          # the grid drops points
    assert g["n_in"] > g["leaf_slots"]             # the rows outnumber the leaf slots
    assert g["tiles"] > 1 and -(-g["n"] // Cs.SCAN_TILE) > 1  # several scan tiles, of the rows and of the indexed points
    assert g["n"] > 4 ** 3 * Cs.LEAF               # more leaves than three levels of the 4-ary tree hold: inner nodes
    assert s["c5000"]["n"] == s["c5000"]["n_in"] == 5000 and s["c5000"]["tiles"] > 1
    assert s["c33000"]["groups"] >= 512            # LPT_MIN_GROUPS of csrc/pcpx_query.hip: a self-kNN launch records its groups' times
    assert s["c0"]["n_in"] == 0


def test_the_gridded_cloud_has_its_duplicates_and_nothing_near_the_face():
    I = Cs.inputs("c5000g")
    pts = I["points"]
    assert len(pts) - len(np.unique(pts, axis=0)) == Cs.DUPLICATES
    assert (np.abs(pts[:, 0] - 0.6) >= 1e-3).all() and np.array_equal(I["inside"], pts[:, 0] < Cs.GRID[3])
    assert len(np.unique(pts[I["inside"]], axis=0)) < int(I["inside"].sum())  # (some of the copies are indexed)
    for c in Cs.KNN_CLOUDS:
        assert len(np.unique(Cs.inputs(c)["points"], axis=0)) == Cs.SIZES[c]


def test_a_radius_holds_about_eight_to_twelve_points(oracle):
    for c in ("c1300", "c5000", "c5000g"):
        I = Cs.inputs(c)
        sub = I["points"][I["inside"]]
        cnt = oracle.range_count_bruteforce(sub, sub, float(I["radius"][0]), nthreads=16)
        interior = ((sub > 0.2) & (sub < 0.8)).all(1) & (sub[:, 0] < 0.4)  # (a sphere that the cube or the grid's face does not cut)
        mean = float(cnt[interior].mean())
        print(c, "mean count of the interior spheres %.2f over %d" % (mean, int(interior.sum())))
        assert 8.0 <= mean <= 12.0, (c, mean)


@pytest.mark.parametrize("cloud", Cs.KNN_CLOUDS)
def test_no_knn_row_rests_on_a_tie(oracle, cloud):
    assert Cs.knn_ties(oracle, cloud) == 0


def test_the_table_names_every_family_and_the_rows_of_the_special_clouds():
    assert {f for f, _ in Cs.ROWS.values()} == {"knn", "any", "free"}
    assert set(Cs.EMPTY_OK) <= {r for r, (f, _) in Cs.ROWS.items() if f == "any"} and set(Cs.LARGE_OK) <= set(Cs.ROWS)
    assert all(Cs.runs_on(r, Cs.HOME[f]) for r, (f, _) in Cs.ROWS.items())
    assert not Cs.runs_on("knn_dev_k8", "c5000g") and Cs.runs_on("cluster_m1_compact", "c5000g")


def test_the_six_sequences_reach_their_coverage():
    plans = Cs.plans()
    assert sorted(plans) == sorted(Cs.SEQUENCE_SEEDS) and len(plans) == 6 and all(len(steps) == Cs.STEPS == 24 for _first, steps in plans.values())
    occur, follows, moves = Cs.coverage()
    assert occur == set(Cs.ROWS)                                                   # every row occurs
    assert not [r for r, before in follows.items() if len(before) < 3], follows    # ... after at least three different rows
    assert moves == set(Cs.TRANSITIONS)                                            # every kind of rebuild
    actions = [a for _first, steps in plans.values() for acts, _cloud, _row in steps for a in acts]
    assert {a[1] for a in actions if a[0] == "set"} == set(Cs.SWITCHES)            # every switch is moved
    assert {a[1] for a in actions if a[0] == "poison"} == {0x00, 0x55, 0xFF}
    # a cloud of 512 groups begins with the same self-kNN three times running, under long_groups_first = 1 and nothing in between
    for first, steps in plans.values():
        cloud, lpt = first, 1
        for i, (acts, at, row) in enumerate(steps):
            arrived = i == 0 and first == "c33000"
            for a in acts:
                lpt = a[2] if a[:2] == ("set", "long_groups_first") else lpt
                arrived = arrived or a == ("rebuild", "c33000")
            if arrived:
                assert lpt == 1 and [r for _a, _c, r in steps[i:i + Cs.REPEATS]] == ["knn_dev_k8"] * Cs.REPEATS
                assert not any(acts2 for acts2, _c, _r in steps[i + 1:i + Cs.REPEATS])
    assert sum(a == ("rebuild", "c33000") for a in actions) + sum(first == "c33000" for first, _ in plans.values()) >= 2
