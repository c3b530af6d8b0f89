"""CPU checks of tests/rollout_cases.py: the argmin checker against the oracle's DWAPlan and hand-written
vectors, and the coverage conditions of every input set tests/test_gpu_rollout.py runs on the device -- all
asserted on the oracle's outputs, never on the device's, so the GPU comparisons cannot pass vacuously."""
import numpy as np
import pytest

import oracle
import rollout_cases as rc
from motionplanning_amd import configs

NAN = float("nan")


# ------------------------------------------------------------ jl_first_min
@pytest.mark.parametrize("state", [configs.X0_REF] + [list(x) for x in rc.DWA_STATES[:2]])
def test_jl_first_min_matches_oracle_dwa_plan(state):
    """On the reference DWA searcher (and two perturbed states) jl_first_min of the oracle's 1271 costs is the
    index or_dwa_plan keeps with mpj_isless (the oracle is pinned to DWATrajectory.csv's 127 choices)."""
    p = configs.dwa_params()
    best, bc, costs = oracle.dwa_plan(p, np.array(state), np.array(configs.GOAL_REF), configs.dwa_control_samples(),
                                      np.array(configs.OBSTACLES_REF))
    assert rc.jl_first_min(costs) == best
    assert costs[best] == bc


@pytest.mark.parametrize("costs, index", [
    ([3.0], 0),
    ([2.0, 1.0, 3.0], 1),
    ([1.0, 1.0, 1.0], 0),
    ([5.0, 2.0, 7.0, 2.0, 2.0], 1),
    ([4.0, 3.0, 3.0, 1.0, 9.0, 1.0], 3),
    ([NAN, 2.0, 1.0, 1.0], 2),
    ([2.0, NAN, 1.0], 2),
    ([1.0, NAN, 2.0], 0),
    ([1.0, 2.0, NAN], 0),
    ([NAN, NAN, NAN], 0),
    ([NAN, NAN, 7.0], 2),
    ([0.0, -0.0], 1),
    ([-0.0, 0.0], 0),
    ([0.0, -0.0, -0.0, 0.0], 1),
    ([NAN, 0.0, -0.0], 2),
    ([float("inf"), NAN, float("inf")], 0),
    ([float("inf"), -float("inf"), NAN], 1),
])
def test_jl_first_min_hand_written(costs, index):
    assert rc.jl_first_min(costs) == index
    assert rc.jl_first_min(np.array(costs)) == index


# -------------------------------------------------- coverage of the input sets
def _consistent(c):
    """feas == not (bound or circle or grid) for every rollout, the causes recomputed from the trajectory."""
    b, ci, g = rc.causes(c)
    assert np.array_equal(c["feas"].astype(bool), ~(b | ci | g))
    return b, ci, g


def _scenes_differ(c, skip=()):
    """Every per-scene input differs from scene to scene: an offset that reads another scene's rows shows."""
    for k in ("X0", "goal", "ctrl", "unom", "obs", "grid"):
        if c[k] is not None and k not in skip:
            assert len({row.tobytes() for row in c[k]}) == len(c[k]), k


def test_mixed_batch_reaches_every_cause():
    c = rc.mixed_batch()
    b, ci, g = _consistent(c)
    _scenes_differ(c)
    # with the grids handed round by one scene the grid hits are others: they come from the scene's own grid
    moved = dict(c, grid=np.roll(c["grid"], 1, axis=0))
    assert not np.array_equal(rc.causes(moved)[2], g)
    assert c["ctrl"].shape == (3, 300, 7, 2) and c["p"].K != 300 and c["p"].ctrl_cost == 1
    assert np.abs(c["unom"]).min() > 0.0
    f = c["feas"].astype(bool)
    for s in range(3):
        assert 0 < f[s].sum() < 300, s  # feasible and infeasible rollouts in every scene
    # infeasible through each cause alone
    assert (b & ~ci & ~g).any() and (ci & ~b & ~g).any() and (g & ~b & ~ci).any()
    assert len(np.unique(c["cost"])) == c["cost"].size  # no accidental duplicates: a swapped row shows
    # the idle lane pairs of the last block and the scenes behind scene 0 hold their own rollouts
    assert 300 % rc.RPB != 0
    assert not np.array_equal(c["cost"][0], c["cost"][1]) and not np.array_equal(c["cost"][1], c["cost"][2])


@pytest.mark.parametrize("name", rc.FEATURES)
def test_feature_cases_reach_their_feature(name):
    c = rc.feature_case(name)
    b, ci, g = _consistent(c)
    _scenes_differ(c)
    p = c["p"]
    assert c["ctrl"].shape == (2, 70, 5, 2)
    if name == "grid_only":
        assert p.n_obs == 0 and c["obs"] is None and p.ctrl_cost == 0
        assert g.any() and not g.all()
    elif name == "circles_only":
        assert p.grid_nx == 0 and c["grid"] is None and p.ctrl_cost == 0
        assert 0 < ci[0].sum() < 70
    elif name == "ctrl_cost_only":
        assert p.n_obs == 0 and p.grid_nx == 0 and p.ctrl_cost == 1
        # the term is there: the same rollouts without it cost something else, everywhere
        q = configs.mppi_params(K=p.K, H=p.H, T=p.H * p.dt, n_obs=0, ctrl_cost=0)
        _, plain, _ = rc.oracle_rollouts(q, c["X0"], c["goal"], c["ctrl"], None, None, None, False)
        assert (plain != c["cost"]).all()
    else:
        assert p.ctrl_cost == 0 and c["unom"] is not None and np.abs(c["unom"]).min() > 0.0
        assert ci.any() and g.any()


@pytest.mark.parametrize("K, H", rc.RAGGED)
def test_ragged_cases(K, H):
    c = rc.ragged_case(K, H)
    b, ci, g = _consistent(c)
    _scenes_differ(c)
    assert c["ctrl"].shape == (2, K, H, 2) and c["traj"].shape == (2, K, H + 1, 7)
    assert c["X0"][1, 5] > c["p"].XU[5]  # out of bounds at j = 0, where nothing is evaluated
    if K > 1:  # one step decides: the circle in scene 0 (H = 1), the ux bound in scene 1
        f = c["feas"].astype(bool)
        assert ci[0].any() and b[1].any() and 0 < f.sum() < 2 * K
        assert 0 < f[1].sum() < K
        if H == 1:
            assert 0 < f[0].sum() < K


def test_dwa_batch():
    c = rc.dwa_batch()
    b, ci, g = _consistent(c)
    _scenes_differ(c, skip=("ctrl",))  # scenes 0 and 1 share the table as it is, scene 2 has it reversed
    assert np.array_equal(c["ctrl"][0], configs.dwa_control_samples()) and np.array_equal(c["ctrl"][1], c["ctrl"][0])
    assert np.array_equal(c["ctrl"][2], c["ctrl"][0][::-1])
    assert c["ctrl"].shape == (3, 1271, 2) and c["p"].H == 20
    dx, dy = c["X0"][1, 0] - c["obs"][1, 0, 0], c["X0"][1, 1] - c["obs"][1, 0, 1]
    assert dx * dx + dy * dy < c["obs"][1, 0, 2] ** 2  # scene 1 starts inside a circle
    assert ci[1].all() and 0 < ci[2].sum() < 1271 and not ci[0].any()
    f = c["feas"].astype(bool)
    assert 0 < f[0].sum() < 1271 and 0 < f[2].sum() < 1271


@pytest.mark.parametrize("name", rc.ARGMIN)
def test_argmin_cases(name):
    c = rc.argmin_case(name)
    _consistent(c)
    _scenes_differ(c)
    cost, K = c["cost"], c["cost"].shape[1]
    assert K == dict(k1=1, k257=257).get(name, 600) and c["const"] and c["ctrl"].shape == (2, K, 2)
    bits = cost.view(np.int64)
    for s in range(2):
        ties = c["ties"][s]
        if ties:  # bit-identical minimal costs at exactly the intended indices
            m = cost[s].min()
            assert sorted(np.where(bits[s] == bits[s][ties[0]])[0]) == sorted(ties), s
            assert cost[s][ties[0]] == m and sorted(np.where(cost[s] == m)[0]) == sorted(ties)
            assert c["expect"][s] == min(ties)
    nan = np.isnan(cost)
    T = rc.ARGMIN_NT
    if name == "same_thread":
        for s in range(2):
            assert len({i % T for i in c["ties"][s]}) == 1
    elif name == "cross_thread":
        for s in range(2):
            first = min(c["ties"][s])
            # a thread before the winner's carries a later tied index into the combine
            assert any(i % T < first % T and i > first for i in c["ties"][s])
    elif name == "later_passes":
        assert T <= c["expect"][0] < 2 * T and c["expect"][1] >= (K // T) * T
    elif name == "k257":
        assert c["expect"][0] == 256
    elif name == "nan_row0":
        assert nan[:, 0].all() and nan.sum() == 2 and (c["expect"] > 0).all()
    elif name == "nan_winner_grid":
        assert c["p"].grid_nx > 0 and c["grid"] is not None and nan.sum() == 2
        for s in range(2):
            w = int(np.where(nan[s])[0][0])
            assert c["expect"][s] != w and np.isnan(c["traj"][s, w]).any()
            assert cost[s, c["expect"][s]] == np.nanmin(cost[s])
    elif name == "nan_all":
        assert nan.all() and (c["expect"] == 0).all()


@pytest.mark.parametrize("n", rc.EULER_N)
def test_euler_inputs(n):
    st, ctrl = rc.euler_inputs(n)
    assert st.shape == (n, 7) and ctrl.shape == (n, 2)
    assert len({r.tobytes() for r in st}) == n and len({r.tobytes() for r in ctrl}) == n
    assert st[0, 5] < 0
    fin, his = rc.euler_reference(n, 5)
    assert his.shape == (n, 5, 7) and np.array_equal(his[:, -1], fin, equal_nan=True)
    if n >= 31:
        assert st[3, 5] == 0 and 0 < st[7, 5] < 1e-3
        assert abs(st[12, 4]) > 3 * np.pi / 4 and abs(st[13, 4]) > 3 * np.pi / 4
        assert abs(st[21, 4]) > 900 and abs(st[22, 4]) > 900
        assert abs(st[25, 2]) > 30 and abs(st[28, 3]) > 20
        assert np.isnan(st[16]).any() and np.isnan(fin[16]).any()
        # NaN stays with its own vehicles: the 0 / 0 one and the NaN state
        assert sorted(np.where(np.isnan(fin).any(axis=1))[0]) == [16, 30]
        assert st[30, 5] + 0.01 == 0.0 and (n == 31 or st[31, 5] + 0.01 == 0.0)


def test_dwa_states_have_an_infeasible_best():
    p = configs.dwa_params()
    goal, smp, obs = np.array(configs.GOAL_REF), configs.dwa_control_samples(), np.array(configs.OBSTACLES_REF)
    feas = []
    for x in rc.DWA_STATES:
        best, _, _ = oracle.dwa_plan(p, x, goal, smp, obs)
        feas.append(oracle.rollout(p, x, goal, smp[best], None, obs, None, const_ctrl=True)[1])
    assert True in feas and False in feas
