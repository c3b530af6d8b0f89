"""CPU conditions on the pairs and tables of tests/rs_cases.py (oracle only): what tests/test_gpu_rs.py compares on
the device is only worth something if the set holds every path length, a NaN winner, many and few feasible
candidates and the special pairs, so that is asserted here rather than trusted to a seed."""
import numpy as np

import rs_cases as rc


def test_pairs_cover_what_the_gpu_tests_rely_on():
    ref = rc.reference()
    n = len(ref["best"])
    assert n == rc.N_RANDOM + len(rc.SPECIAL)
    assert (ref["minR"] < 0).any() and (ref["minR"] > 0).any()
    win = ref["cmds"][np.arange(n), ref["best"]]
    lens = 100 * rc.n_segments(win) + 1
    for want in (301, 401, 501):
        assert (lens == want).any(), want
    win_cost = ref["cost"][np.arange(n), ref["best"]]
    assert np.isnan(win_cost).any()
    assert np.array_equal(np.isnan(win_cost), np.isnan(ref["act_cost"]))
    feas = (ref["cost"] < np.inf).sum(1)
    assert feas.max() >= 10 and feas.min() <= 4, (feas.min(), feas.max())
    # a NaN cost is not feasible (findall(costs .< Inf)) and leaves an all-zero table, as an Inf cost does
    assert not ref["cmds"][~(ref["cost"] < np.inf)].any()
    assert (rc.n_segments(ref["cmds"][ref["cost"] < np.inf]) >= 3).all()


def test_special_pairs():
    ref = rc.reference()
    i = rc.SPECIAL["same"]
    assert np.array_equal(ref["norm"][i], np.zeros(3))
    assert np.isnan(ref["cost"][i]).sum() == 4 and ref["best"][i] == 16
    assert not ref["cmds"][i, 16].any()
    i = rc.SPECIAL["straight"]
    assert np.array_equal(ref["norm"][i], [2.0, 0.0, 0.0])
    assert ref["best"][i] == 0  # LSL with two zero-length arcs
    assert np.array_equal(ref["cmds"][i, 0], [[0, 1, 1], [2, 1, 0], [0, 1, 1], [0, 0, 0], [0, 0, 0]])
    assert ref["act_cost"][i] == 2.0 * 1.5
    assert np.array_equal(ref["norm"][rc.SPECIAL["pi"]], [3.0, 2.0, np.pi])
    assert np.array_equal(ref["norm"][rc.SPECIAL["minus_pi"]], [-3.0, -2.0, -np.pi])
    for k in ("wide_pos", "wide_neg"):
        assert abs(ref["init"][rc.SPECIAL[k], 2]) == 50.0
        assert np.isfinite(ref["act_cost"][rc.SPECIAL[k]])


def test_act_path_of_tables():
    """or_ha_act_path returns 1 for an all-zero table (the start alone), ignores the rows after a gear-0 row, and a
    table's path has 100 nseg + 1 poses."""
    t = rc.tables()
    paths = rc.table_paths(True)
    names = list(rc.HAND_TABLES)
    h0 = len(paths) - t["n_hand"]
    z = h0 + names.index("all_zero")
    assert not t["cmds"][z].any() and paths[z].shape == (1, 3) and np.array_equal(paths[z][0], t["init"][z])
    assert len(paths[h0 + names.index("gear0_in_the_middle")]) == 101
    assert len(paths[h0 + names.index("one_segment")]) == 101
    assert len(paths[h0 + names.index("two_segments")]) == 201
    assert len(paths[h0 + names.index("five_segments")]) == 501
    assert np.array_equal([len(p) for p in paths], 100 * rc.n_segments(t["cmds"]) + 1)
    # a straight segment keeps its heading; zero-length arcs repeat the pose
    s = paths[h0 + names.index("straight")]
    assert (s[:, 2] == s[0, 2]).all()
    za = paths[h0 + names.index("zero_length_arcs")]
    assert np.array_equal(za[:101], np.tile(za[0], (101, 1)))
    # createPath is createActPath from the origin at minR = 1.0
    plain = rc.table_paths(False)
    assert all(np.array_equal(p[0], np.zeros(3)) for p in plain)
    assert all(np.isfinite(p).all() for p in paths)
