"""GPU parity of the public entry points mp_rollout (rollout_kernel, argmin_kernel) and mp_vehicle_euler
(euler_kernel) with the CPU oracle, called directly: per-step and constant controls, S > 1, ragged K, each
optional feature alone, every output array, the argmin's ties and NaN ordering, the plant's partial blocks and
data-dependent paths, and the argument checks.  DWAPlan, the Python surface on top, is checked against
oracle.dwa_plan.

Every comparison of cost, feasibility, trajectory, argmin and plant state is exact (rollout_cases.assert_same:
NaN equals NaN, every other double bit for bit) -- the standard tests/test_gpu_mppi.py states for rollouts.
The inputs and their references come from tests/rollout_cases.py; tests/test_rollout_cases.py asserts on the
oracle alone that they reach what each test here is about.
"""
import ctypes

import numpy as np
import pytest

import oracle
import rollout_cases as rc
from motionplanning_amd import configs
from motionplanning_amd.abi import MP_ERR_INVALID, MP_OK, MPPIParams, ptr
from motionplanning_amd.rollout import rollout_batch, vehicle_euler

pytestmark = pytest.mark.gpu


def _run(ctx, c, sl=slice(None), want_traj=True, want_argmin=True):
    def part(a):
        return None if a is None else a[sl]

    return rollout_batch(c["p"], c["X0"][sl], c["goal"][sl], c["ctrl"][sl], U_nom=part(c["unom"]),
                         obstacles=part(c["obs"]), grid=part(c["grid"]), want_traj=want_traj, want_argmin=want_argmin,
                         ctx=ctx)


def _check(r, c, sl=slice(None), what=""):
    rc.assert_same(r["cost"], c["cost"][sl], what + " cost")
    rc.assert_same(r["feas"], c["feas"][sl], what + " feas")
    assert r["feas"].dtype == np.uint8
    if r["traj"] is not None:
        rc.assert_same(r["traj"], c["traj"][sl], what + " traj")
    if r["argmin"] is not None:
        ref = np.array([rc.jl_first_min(row) for row in c["cost"][sl]], np.int32)
        np.testing.assert_array_equal(r["argmin"], ref, err_msg=what + " argmin")


# ---------------------------------------------------------------- mp_rollout
def test_per_step_controls_mixed_batch(ctx):
    """ctrl_stride_h = 2, S = 3, K = 300 (84 idle lane pairs in each scene's last block), circles, grid read from
    global memory and the control cost evaluated per step, every output; p.K != K."""
    c = rc.mixed_batch()
    assert c["p"].K != c["ctrl"].shape[1]
    _check(_run(ctx, c), c)


@pytest.mark.parametrize("K, H", rc.RAGGED)
def test_ragged_k(ctx, K, H):
    """K around the 128 rollouts of a block, H = 1 (no obstacle or bound cost before the terminal step) and 2."""
    c = rc.ragged_case(K, H)
    _check(_run(ctx, c), c)


def test_constant_controls_batched_and_alone(ctx):
    """ctrl_stride_h = 0 with the DWA sample table for three states in one call: equal to the oracle, and to the
    same three scenes in three S = 1 calls (batching invariance)."""
    c = rc.dwa_batch()
    whole = _run(ctx, c)
    _check(whole, c, what="batched")
    for s in range(3):
        one = _run(ctx, c, slice(s, s + 1))
        _check(one, c, slice(s, s + 1), what="scene %d alone" % s)
        for k in ("cost", "feas", "traj", "argmin"):
            rc.assert_same(one[k][0], whole[k][s], "scene %d %s" % (s, k))


@pytest.mark.parametrize("name", rc.FEATURES)
def test_each_feature_alone(ctx, name):
    """Grid only (obstacles = NULL), circles only, control cost only, and a U_nom passed with ctrl_cost = 0."""
    c = rc.feature_case(name)
    _check(_run(ctx, c), c)


@pytest.mark.parametrize("name", rc.ARGMIN)
def test_argmin(ctx, name):
    """First minimum with Julia's isless per scene: ties within a thread's strided scan and across threads,
    minima in the later passes, K = 1 and 257, NaN costs (one case with the occupancy grid present)."""
    c = rc.argmin_case(name)
    r = _run(ctx, c, want_traj=False)
    _check(r, c)
    np.testing.assert_array_equal(r["argmin"], c["expect"])
    assert r["argmin"].dtype == np.int32
    for s in range(2):  # and of the device's own costs
        assert r["argmin"][s] == rc.jl_first_min(r["cost"][s])


def test_no_optional_outputs(ctx):
    """argmin = NULL and traj = NULL: cost and feas alone."""
    c = rc.mixed_batch()
    r = _run(ctx, c, want_traj=False, want_argmin=False)
    assert r["traj"] is None and r["argmin"] is None
    _check(r, c)


def test_workspace_reuse(ctx):
    """A large call, then smaller and different ones on the same context: the cached device buffers hand no
    stale row to the later calls."""
    big = rc.dwa_batch()
    _check(_run(ctx, big), big, what="large")
    for small in (rc.feature_case("unom_ignored"), rc.ragged_case(1, 1), rc.argmin_case("nan_row0")):
        _check(_run(ctx, small), small, what="after the large call")


def _raw_rollout(ctx, p, S, K, c, stride=2, unom=None, obs="case", grid="case", cost="new", traj=None):
    cost = np.full((max(S, 1), max(K, 1)), -7.0) if isinstance(cost, str) else cost
    feas = np.full((max(S, 1), max(K, 1)), 9, np.uint8)
    obs = c["obs"] if isinstance(obs, str) else obs
    grid = c["grid"] if isinstance(grid, str) else grid
    st = ctx.lib.mp_rollout(ctx.handle, ctypes.byref(p), S, K, ptr(c["X0"]), ptr(c["goal"]), ptr(c["ctrl"]), stride,
                            ptr(unom), ptr(obs), ptr(grid), ptr(traj), ptr(cost), ptr(feas), None)
    return st, ctx.lib.mp_last_error(ctx.handle).decode(), cost, feas


def test_rollout_argument_checks(ctx):
    """Each bad argument returns MP_ERR_INVALID with a message naming it and writes nothing; a valid call
    afterwards works."""
    c = rc.feature_case("unom_ignored")  # circles and grid, ctrl_cost = 0
    p = c["p"]
    S, K = c["ctrl"].shape[:2]
    q = MPPIParams.from_buffer_copy(p)
    q.ctrl_cost = 1
    bad = [("S (0)", dict(p=p, S=0, K=K)),
           ("K (0)", dict(p=p, S=S, K=0)),
           ("ctrl_stride_h", dict(p=p, S=S, K=K, stride=1)),
           ("NULL", dict(p=p, S=S, K=K, cost=None)),
           ("U_nom", dict(p=q, S=S, K=K, unom=None)),
           ("obstacles", dict(p=p, S=S, K=K, obs=None)),
           ("grid", dict(p=p, S=S, K=K, grid=None))]
    for word, kw in bad:
        st, msg, cost, feas = _raw_rollout(ctx, c=c, **kw)
        assert st == MP_ERR_INVALID, (word, st, msg)
        assert msg and word in msg, (word, msg)
        assert cost is None or (cost == -7.0).all()
        assert (feas == 9).all()
    st, msg, cost, feas = _raw_rollout(ctx, p, S, K, c)
    assert st == MP_OK, msg
    rc.assert_same(cost, c["cost"])
    rc.assert_same(feas, c["feas"])


# ---------------------------------------------------------- mp_vehicle_euler
@pytest.mark.parametrize("nsteps", rc.EULER_STEPS)
@pytest.mark.parametrize("n", rc.EULER_N)
def test_euler_matches_oracle(ctx, n, nsteps):
    """n around the 32 vehicles of a block (one, the last partial block, three blocks), distinct states and
    controls, the clamp / wide-reduction / NaN states of rollout_cases.EULER_SPECIAL among them: final states
    and the whole history equal oracle.vehicle_euler per vehicle, so a NaN vehicle leaves the others alone."""
    st, ctrl = rc.euler_inputs(n)
    fin, his = rc.euler_reference(n, nsteps)
    s, h = vehicle_euler(st, ctrl, rc.EULER_DT, nsteps, ctx=ctx)
    rc.assert_same(s, fin, "states")
    rc.assert_same(h, his, "history")
    clean = ~np.isnan(fin).any(axis=1)
    assert np.isfinite(s[clean]).all() and np.isfinite(h[clean]).all()


def test_euler_without_history(ctx):
    st, ctrl = rc.euler_inputs(70)
    s, h = vehicle_euler(st, ctrl, rc.EULER_DT, 5, want_his=False, ctx=ctx)
    assert h is None
    rc.assert_same(s, rc.euler_reference(70, 5)[0])


@pytest.mark.parametrize("with_his", [True, False])
def test_euler_zero_steps(ctx, with_his):
    """nsteps = 0 returns the states unchanged and writes nothing else."""
    st, ctrl = rc.euler_inputs(33)
    s = np.array(st)
    his = np.full((33, 2, 7), -3.25) if with_his else None
    ctx.check(ctx.lib.mp_vehicle_euler(ctx.handle, 33, ptr(s), ptr(ctrl), rc.EULER_DT, 0, ptr(his)))
    rc.assert_same(s, st)
    assert his is None or (his == -3.25).all()


def test_euler_chaining(ctx):
    """Two calls of 3 + 4 steps equal one call of 7 (and the oracle's 7)."""
    st, ctrl = rc.euler_inputs(70)
    s3, h3 = vehicle_euler(st, ctrl, rc.EULER_DT, 3, ctx=ctx)
    s7c, h4 = vehicle_euler(s3, ctrl, rc.EULER_DT, 4, ctx=ctx)
    s7, h7 = vehicle_euler(st, ctrl, rc.EULER_DT, 7, ctx=ctx)
    rc.assert_same(s7c, s7)
    rc.assert_same(np.concatenate([h3, h4], axis=1), h7)
    fin, his = rc.euler_reference(70, 7)
    rc.assert_same(s7, fin)
    rc.assert_same(h7, his)


def test_euler_argument_checks(ctx):
    st, ctrl = rc.euler_inputs(33)
    for n, nsteps, states in ((0, 5, st), (33, -1, st), (33, 5, None)):
        s = None if states is None else np.array(states)
        his = np.full((33, 5, 7), -3.25)
        rv = ctx.lib.mp_vehicle_euler(ctx.handle, n, ptr(s), ptr(ctrl), rc.EULER_DT, nsteps, ptr(his))
        assert rv == MP_ERR_INVALID, (n, nsteps)
        assert ctx.lib.mp_last_error(ctx.handle).decode()
        assert (his == -3.25).all() and (s is None or np.array_equal(s, st, equal_nan=True))
    s, _ = vehicle_euler(st, ctrl, rc.EULER_DT, 5, ctx=ctx)
    rc.assert_same(s, rc.euler_reference(33, 5)[0])


# ------------------------------------------------------------------- DWAPlan
@pytest.mark.parametrize("i", range(len(rc.DWA_STATES)))
def test_dwa_plan_matches_oracle(ctx, i):
    """DWAPlan on the reference searcher at states off the CSV trajectory (the last one's best candidate is
    infeasible): best_index, cost, Feasibility and Control equal oracle.dwa_plan's."""
    from motionplanning_amd.dwa import DWAPlan, ShiftInitialCondition, reference_dwa

    d = reference_dwa()
    ShiftInitialCondition(d, rc.DWA_STATES[i])
    assert DWAPlan(d, ctx=ctx) is None
    p = configs.dwa_params()
    goal, smp, obs = np.array(configs.GOAL_REF), configs.dwa_control_samples(), np.array(configs.OBSTACLES_REF)
    best, bc, costs = oracle.dwa_plan(p, rc.DWA_STATES[i], goal, smp, obs)
    feas = oracle.rollout(p, rc.DWA_STATES[i], goal, smp[best], None, obs, None, const_ctrl=True)[1]
    assert d.r.best_index == best == rc.jl_first_min(costs)
    rc.assert_same(np.float64(d.r.cost), np.float64(bc))
    assert d.r.Feasibility == ("Feasible" if feas else "InFeasible")
    rc.assert_same(d.r.Control, smp[best])
    if i == len(rc.DWA_STATES) - 1:
        assert d.r.Feasibility == "InFeasible"
