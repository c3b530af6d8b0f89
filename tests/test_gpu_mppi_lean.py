"""GPU parity of the plan kernel's lean instance (mppi_plan_kernel<.., LEAN>) with the generic one.

plan_launch picks the lean instance for a collecting call with device noise, a grid, the control
cost, no circle obstacles and one rollout per lane; MPGPU_PLAN_LEAN=0 forces the generic instance.
Both run the same block partition, so every output -- MPPICtrl included -- must be the same bits.
One scene per case is also checked against the oracle (test_gpu_mppi._check_plan tolerances).
Shapes are the smallest that reach what can break: inactive lanes of a partial block, the scene
offset of the wave-uniform store base, H below the four priority levels, the bound slow path and a
rollout off the grid, the FeasibilityCount prefix ending in the partial block, and the calls that
must fall back to the generic instance."""
import os

import numpy as np
import pytest

import oracle
from motionplanning_amd import configs
from motionplanning_amd.abi import MP_NOISE_PHILOX
from motionplanning_amd.mppi import mppi_plan_batch

from test_gpu_mppi import _check_plan

pytestmark = pytest.mark.gpu

SPEC = configs.grid_spec()
GRID = configs.rasterize_circles(configs.OBSTACLES_CFG1, SPEC)


def _params(K, H, **kw):
    kw.setdefault("n_obs", 0)
    kw.setdefault("feasibility_count", K)
    kw.setdefault("grid", SPEC)
    return configs.mppi_params(K=K, H=H, T=H * 0.15, noise_mode=MP_NOISE_PHILOX, seed=77, offset=2, **kw)


def _unom(S, H, seed=4):
    r = np.random.default_rng(seed)
    return np.stack([np.c_[r.uniform(-0.1, 0.1, H), r.uniform(-0.5, 0.5, H)] for _ in range(S)])


def _run(p, X0, goal, un, obs, grid, env, collect=True, ctx=None):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return mppi_plan_batch(p, X0, goal, un, obs, grid, None, collect=collect, ctx=ctx)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _lean_vs_generic(ctx, p, X0, goal, un, lpr="1"):
    S = X0.shape[0]
    grid = np.stack([GRID] * S)
    lean = _run(p, X0, goal, un, None, grid, {"MPGPU_LPR": lpr}, ctx=ctx)
    gen = _run(p, X0, goal, un, None, grid, {"MPGPU_LPR": lpr, "MPGPU_PLAN_LEAN": "0"}, ctx=ctx)
    for k in ("U", "traj", "cost", "feasible", "rollout_count", "feasible_count"):
        assert np.array_equal(lean[k], gen[k]), k
    for k in ("traj_soa", "ctrl_soa", "cost", "feas"):
        assert np.array_equal(lean["coll"][k], gen["coll"][k]), k
    return lean


def _scenes(S):
    X0 = np.tile(configs.X0_REF, (S, 1))
    X0[:, 0] = 20.0 * np.arange(S)  # scene 1 starts 10 m before the first occupied cells
    X0[:, 1] = 0.4 * np.arange(S)
    return X0, np.tile(configs.GOAL_REF, (S, 1))


def test_inactive_lanes_and_scene_offset(ctx):
    """S=2, K=300, H=7: block 1 of each scene has 212 inactive lanes; scene 1's stores sit behind scene 0's."""
    p = _params(300, 7)
    X0, goal = _scenes(2)
    un = _unom(2, 7)
    out = _lean_vs_generic(ctx, p, X0, goal, un)
    assert not np.array_equal(out["coll"]["traj_soa"][0], out["coll"]["traj_soa"][1])
    for s in range(2):
        p.scene_base = s  # the oracle's single scene draws scene s's Philox stream (counter word: scene index)
        ref = oracle.mppi_plan(p, X0[s], goal[s], un[s], None, GRID, None, collect=True)
        _check_plan(out, ref, s)


def test_h_below_quarter_levels(ctx):
    """H=3 < 4: the three priority thresholds fall on steps 1, 2 and past the horizon."""
    p = _params(64, 3)
    X0, goal = _scenes(1)
    un = _unom(1, 3)
    out = _lean_vs_generic(ctx, p, X0, goal, un)
    _check_plan(out, oracle.mppi_plan(p, X0[0], goal[0], un[0], None, GRID, None, collect=True), 0)


def test_bound_violation_and_off_grid(ctx):
    """A start 0.1 m inside the y bound (the grid's edge too), heading outwards: some rollouts cross it --
    a slack term in their cost (the wave-uniform bound slow path) and cells off the grid -- others steer back."""
    H = 12
    p = _params(300, H)
    X0, goal = _scenes(1)
    X0[0, 1], X0[0, 4] = 19.9, 0.02
    un = _unom(1, H)
    ref = oracle.mppi_plan(p, X0[0], goal[0], un[0], None, GRID, None, collect=True)
    tr = ref["coll"]["traj"][:, 1:, :]  # the states the bounds are evaluated at
    out_b = ((tr < np.array(configs.XL_REF)) | (tr > np.array(configs.XU_REF))).any(axis=(1, 2))
    off = (tr[:, :, 1] >= configs.XU_REF[1]).any(axis=1)  # fy >= gny: off the grid
    feas = np.asarray(ref["coll"]["feas"]).astype(bool)
    assert feas.any() and (~feas).any()
    assert out_b.any() and off.any() and (~out_b).any()
    assert (np.asarray(ref["coll"]["cost"])[out_b] > configs.SLACK_PENALTY * 1e-6).all()
    out = _lean_vs_generic(ctx, p, X0, goal, un)
    _check_plan(out, ref, 0)


def test_feasibility_prefix_in_partial_block(ctx):
    """FeasibilityCount reached inside block 1 (rollouts 256..299, 212 inactive lanes behind them)."""
    K, H = 300, 7
    p = _params(K, H, feasibility_count=270)
    X0, goal = _scenes(1)
    un = _unom(1, H)
    ref = oracle.mppi_plan(p, X0[0], goal[0], un[0], None, GRID, None, collect=True)
    assert 257 < ref["rollout_count"] < K + 1
    out = _lean_vs_generic(ctx, p, X0, goal, un)
    _check_plan(out, ref, 0)


@pytest.mark.parametrize("case", ["circles", "no_ctrl_cost", "no_grid", "no_collect"])
def test_fallback_to_generic(ctx, case):
    """Calls outside the lean instance's facts take the generic instance and still match the oracle."""
    K, H = 300, 7
    kw, obs, grid, collect = {}, None, GRID, True
    if case == "circles":
        kw["n_obs"] = 2
        obs = np.array(configs.OBSTACLES_REF[:2])
    elif case == "no_ctrl_cost":
        kw["ctrl_cost"] = 0
    elif case == "no_grid":
        kw["grid"], grid = None, None
    else:
        collect = False
    p = _params(K, H, **kw)
    X0, goal = _scenes(1)
    X0[0, 0] = 40.0
    un = _unom(1, H)
    out = _run(p, X0, goal, un, None if obs is None else obs[None], None if grid is None else grid[None],
               {"MPGPU_LPR": "1"}, collect=collect, ctx=ctx)
    ref = oracle.mppi_plan(p, X0[0], goal[0], un[0], obs, grid, None, collect=True)
    _check_plan(out, ref, 0, coll=collect)
